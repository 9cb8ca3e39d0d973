"""The joint covariance of a query batch and the posterior draws on the GPU at their edges (cov_strip_kernel,
cov_gram_kernel, cov_block_kernel and mix_cov_kernel of pmk_cov.hip, the host path of pmk_query_items_cov / _mix_cov /
_fetch_cov / _fetch_cov_dev / _get_items_cov, samplemixtureGP), on the inputs of tests/_cov_edge_cases.py and the workloads
of tests/_grad_edge_cases.py; tests/test_cov_edges_refs.py asserts on the CPU what each input was chosen for.

  A. more strips than workgroups on a tree of 1024 leaves: a workgroup of cov_strip_kernel runs several tasks, a patch of
     six block rows behind one of one and the other way round, a full strip next to a strip of one item (seven waves that
     only walk the barriers), the ring of two point tiles entered at either parity; D = 2, 1 and 4, fp32, mixed families;
  B. patches of 5, 6 and 7 block rows with every count of last-row pairs, D = 1 and 4, Spline34 at D = 1 and a family of
     the shared switch, fp32 at D = 4; item counts of 31, 32, 33, 63, 64, 65, 96 and 512 (two full strips);
  C. the blend: every profile, more neighbours than PLAN_STAGE, 12 and more items per query, a real D = 4 tree, t == 0,
     training points and twins as queries, plan radius 0 and 1e300, fp32 models, Nq = 0, 1, 15, 16, 17 and 33, padded
     leading dimensions of pmk_query_fetch_cov_dev and pmk_query_get_items_cov;
  D. draws: duplicated queries (a singular covariance), Nq = 1, a batch that touches a failed patch, z of a wrong shape
     and as a numpy array.

Bounds, all those of tests/test_gpu_cov.py: the reference is _cov_refs.RegionRef / mix_cov_ref in long double, fed with the
device's own items; the error unit of a block entry is (n + 32) u kappa2(L) (k0 + |V_a| |V_b|), that of a blended entry the
wn-weighted sum of its regions' units; every err / unit stays <= RATIO_MAX = 10 and kappa2(L) <= 10^3.  "Bits" is
np.array_equal on the uint64 views.

Found by this module (the joint covariance): mix_cov_kernel summed an entry in the item order of its
lower-indexed query, a chain of fused multiply-adds, so twins had rows that differed in the last bit
(test_training_points_and_twins_as_queries[dups], test_draws_of_duplicated_queries); it now sums in ascending region index,
and test_batches_around_the_tile_of_the_blend_keep_their_bits holds a shuffled sub-batch to the bits of the full batch.

Every measured ratio is printed ("COVEDGE {json}", run with -s); a run of the whole module writes them to
profiles/cov_edges_accuracy.json.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import patchmixturekriging_amd as pmk
from patchmixturekriging_amd import mixture as M

import _cov_cases as CC
import _cov_edge_cases as CE
import _cov_refs as CR
import _grad_edge_cases as EC
from test_cov_edges_refs import a_region_groups, grouped_cov
from test_gpu_cov import _check_blocks, _device_blocks, _fitted, _main, _main_model, _staged
from test_gpu_grad import _explicit_query, _tree8, _worst_ratio

pytestmark = pytest.mark.gpu

U_OF, SIGMA2, RATIO_MAX, KAPPA_MAX = CC.U_OF, CC.SIGMA2, CC.RATIO_MAX, CC.KAPPA_MAX
_RECORDS = []
TESTS = {"schedule", "deep_patches", "weight_family", "many_items", "twelve_items", "d4_tree", "on_plane", "training_points",
         "plan_radius", "f32_model", "nq_edges", "padded_fetch", "duplicated_queries", "one_query", "failed_patch"}
ACCURACY_JSON = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "cov_edges_accuracy.json")


def _record(**kw):
    _RECORDS.append(kw)
    print("COVEDGE " + json.dumps(kw, sort_keys=True))


@pytest.fixture(scope="module", autouse=True)
def _write_accuracy_file():
    """only a run of the whole module replaces the file"""
    yield
    if {r["test"] for r in _RECORDS} >= TESTS:
        with open(ACCURACY_JSON, "w") as f:
            f.write("[\n" + ",\n".join(" " + json.dumps(r, sort_keys=True) for r in _RECORDS) + "\n]\n")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


_REFS = {}


def _ref(key, oth, X, sigma2):
    """the long-double factor of one patch (or point set), built once per process"""
    if key not in _REFS:
        _REFS[key] = CR.RegionRef(oth, X, sigma2)
    return _REFS[key]


def _blocks_with_items(q, P):
    """item_covs of the regions that hold items (a tree of 2048 leaves has few of them)"""
    counts = np.diff(q.region_offsets(P))
    out = {}
    for r in np.nonzero(counts)[0]:
        idx, S = q.item_covs(int(r))
        assert len(idx) == counts[r]
        out[int(r)] = (idx.astype(np.int64), S)
    return out


# ------------------------------------------------------------------------------------------ A. several strips per workgroup
@pytest.mark.parametrize("D,dtype,mixed", CE.A_CASES)
def test_a_workgroup_runs_strips_of_patches_of_different_depth(D, dtype, mixed):
    import torch
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    sizes, counts = CE.a_sizes(), CE.a_counts()
    s = CE.schedule(counts, sizes, ncu)
    assert s["ntasks"] >= 2 * ncu + 3 and s["slots"] == ncu, s
    assert s["deep_to_one"] >= 1 and s["one_to_deep"] >= 1 and s["full_to_single"] >= 1 and s["single_to_full"] >= 1, s
    assert s["parity"] >= 1, s
    P = CE.A_P
    Xs = CE.a_patches(D, dtype)
    xq, region = CE.a_items(D, dtype)
    keys = [CE.a_set_key(r, sizes) for r in range(P)]
    th = None if mixed else CC.FAMILIES["spline34"][0]
    fit_th = [CC.FAMILIES[CE.a_family(k, True)][0] for k in keys] if mixed else th
    model = _fitted(Xs, [np.sin(X[:, 0]) for X in Xs], fit_th, dtype, CE.a_tree(D))
    assert np.all(model.info() == 0)
    q = _explicit_query(model, xq, region)
    q.items_cov(th)
    blocks = _device_blocks(q, P)
    assert sorted(blocks) == list(range(P))
    for r, (idx, S) in blocks.items():
        assert np.array_equal(idx, np.nonzero(region == r)[0]), r
        assert same_bits(S, S.T), r                                  # symmetric bit for bit
    # a second run on the same query gives the same bits
    q.items_cov(th)
    for r, (_, S) in _device_blocks(q, P).items():
        assert same_bits(S, blocks[r][1]), r
    # bits: the items of 32 consecutive regions in a query of their own, where every workgroup has one task
    for lo, hi in CE.a_pieces():
        sel = np.nonzero((region >= lo) & (region < hi))[0]
        assert len(CE.cov_tasks(counts[lo:hi])[0]) <= ncu
        q2 = _explicit_query(model, xq[sel], region[sel])
        q2.items_cov(th)
        for r in range(lo, hi):
            idx2, S2 = q2.item_covs(r)
            assert np.array_equal(sel[idx2], blocks[r][0]) and same_bits(S2, blocks[r][1]), r
    # accuracy: every region of two and more block rows, every eighth of the others
    worst = kappa = 0.0
    worst_at = None
    for key, regs in a_region_groups(sizes).items():
        ref = _ref(("A", D, dtype, mixed) + key, CC.FAMILIES[CE.a_family(key, mixed)][1], Xs[regs[0]], SIGMA2[dtype])
        kappa = max(kappa, ref.kappa)
        for r, out in zip(regs, grouped_cov(ref, [xq[blocks[r][0]] for r in regs])):
            assert not out["clamped"].any()
            err = np.abs(np.asarray(blocks[r][1], dtype=CR.LD) - out["S"]).astype(np.float64)
            ratio = _worst_ratio(err, (sizes[r] + 32) * U_OF[dtype] * out["unit"])
            if ratio > worst:
                worst, worst_at = ratio, r
    _record(group="A", test="schedule", D=D, dtype=dtype, mixed=mixed, ncu=int(ncu), items=int(len(xq)), blocks=worst,
            worst_region=worst_at, kappa=kappa, checked_regions=len(CE.a_checked_regions()), **s)
    assert kappa <= KAPPA_MAX and worst <= RATIO_MAX, (kappa, worst, worst_at)


# ------------------------------------------------------------------------------------------ B. depth, dimension, strip counts
@pytest.mark.parametrize("D,dtype,family", CE.B_CASES)
def test_patches_of_five_to_seven_block_rows_and_counts_on_the_boundaries(D, dtype, family):
    th, oth = CC.FAMILIES[family]
    Xs = CE.b_patches(D, dtype)
    xq, region = CE.b_items(D, dtype)
    assert [CE.block_rows(len(X)) for X in Xs] == CE.B_NT and [CE.last_pairs(len(X)) for X in Xs] == CE.B_PAIRS
    model = _fitted(Xs, [np.sin(X[:, 0]) for X in Xs], th, dtype, _tree8(D))
    assert np.all(model.info() == 0)
    q = _explicit_query(model, xq, region)
    q.items_cov(th)
    blocks = _device_blocks(q, 8)
    for r, c in enumerate(CE.B_COUNTS):
        assert len(blocks[r][0]) == c and np.array_equal(blocks[r][0], np.nonzero(region == r)[0]), r
    refs = {r: _ref(("B", D, dtype, family, r), oth, Xs[r], SIGMA2[dtype]) for r in range(8)}
    worst, kappa, _, _ = _check_blocks(blocks, xq, refs, dtype)     # ascending rows, symmetric bits, the reference
    _record(group="B", test="deep_patches", D=D, dtype=dtype, family=family, blocks=worst, kappa=kappa)
    # bits: the two diagonal parts of the region of two full strips equal the blocks of two queries of 256 items
    r2 = CE.B_TWO_STRIPS
    idx6, S6 = blocks[r2]
    for half in (0, 1):
        part = slice(CE.TQ * half, CE.TQ * (half + 1))
        sel = idx6[part]
        qh = _explicit_query(model, xq[sel], region[sel])
        qh.items_cov(th)
        idx2, S2 = qh.item_covs(r2)
        assert np.array_equal(idx2, np.arange(CE.TQ)) and same_bits(S2, S6[part, part]), half
    # an entry of the off-diagonal part keeps its bits in a query of five items
    others = [int(np.nonzero(region == r)[0][0]) for r in (0, 3, 7)]
    for a, b in ((0, 2 * CE.TQ - 1), (3, CE.TQ + 44), (CE.TQ - 1, CE.TQ)):
        ja, jb = int(idx6[a]), int(idx6[b])
        sub = np.array([others[0], jb, others[1], ja, others[2]])
        q5 = _explicit_query(model, xq[sub], region[sub])
        q5.items_cov(th)
        idx2, S2 = q5.item_covs(r2)
        assert list(idx2) == [1, 3]
        assert same_bits(S2[1, 0], S6[a, b]) and same_bits(S2[0, 1], S6[b, a]) and same_bits(S2[1, 1], S6[a, a]) \
            and same_bits(S2[0, 0], S6[b, b]), (a, b)
    assert kappa <= KAPPA_MAX and worst <= RATIO_MAX, (kappa, worst)


# ------------------------------------------------------------------------------------------ C. the blend
_CMODELS = {}


def _cmodel(name):
    """the model of a workload of _grad_edge_cases as test_gpu_vgrad_edges builds it, single-output and without a trend"""
    if name not in _CMODELS:
        wl = EC.workload(name)
        model = M.DeviceModel(wl.Xs, [np.ascontiguousarray(y[:, 0]) for y in wl.Ys(1)], dtype=wl.dtype)
        model.fit(wl.th, SIGMA2[wl.dtype])
        assert np.all(model.info() == 0)
        model.set_bsp(wl.root, 0)
        _CMODELS[name] = model
    return EC.workload(name), _CMODELS[name]


def blend_checks(wl, model, wth, owth, radius=None, Xq=None):
    """the staged covariance of a batch and what every blend must satisfy -> dict(q, Cov, dbg, blocks, and the measured
    ratios blocks, blend, diag_vs_vq, kappa); the caller records and asserts the ratios"""
    Xq = wl.Xq if Xq is None else Xq
    q = _staged(model, Xq, wl.radius if radius is None else radius, wl.delta, wl.th, wth)
    P = len(wl.Xs)
    blocks = _blocks_with_items(q, P)
    refs = {r: _ref(("C", wl.name, r), wl.oth, wl.Xs[r], SIGMA2[wl.dtype]) for r in blocks}
    worst, kappa, S_ref, units = _check_blocks(blocks, CC.rnd(Xq, wl.dtype), refs, wl.dtype)
    dbg = q.debug()
    off, reg = dbg["item_offsets"], dbg["item_region"]
    ref_cov, unit = CR.mix_cov_ref((off, reg), S_ref, dbg["item_t"], owth, units)
    Cov = q.fetch_cov()
    Vq = q.fetch()[1]
    assert np.all(np.isfinite(Cov))
    blend = _worst_ratio(np.abs(np.asarray(Cov, dtype=CR.LD) - ref_cov).astype(np.float64), unit)
    assert same_bits(Cov, Cov.T)                                                     # symmetric bit for bit
    shared = CR.shared_region_mask((off, reg))
    assert np.all(Cov[~shared] == 0) and not np.signbit(Cov[~shared]).any()          # + 0 exactly off the mask
    # the diagonal is Vq where no query holds two items of one region (there it carries their cross term)
    single = np.array([len(set(reg[off[j]:off[j + 1]])) == off[j + 1] - off[j] for j in range(q.Nq)])
    diag = _worst_ratio(np.abs(np.diag(Cov) - Vq)[single], np.diag(unit)[single])
    return dict(q=q, Cov=Cov, dbg=dbg, blocks=blocks, shared=shared, single=single,
                ratios=dict(blocks=worst, blend=blend, diag_vs_vq=diag, kappa=kappa, largest_m=int(np.diff(off).max()),
                            neighbour_items=int(off[-1] - q.Nq), queries_with_a_doubled_region=int((~single).sum())))


def ratios_ok(rt):
    return rt["kappa"] <= KAPPA_MAX and max(rt["blocks"], rt["blend"], rt["diag_vs_vq"]) <= RATIO_MAX


@pytest.mark.parametrize("wname", list(EC.weight_kernels(1.0)))
def test_every_profile_as_the_blending_weight(wname):
    wl, model = _cmodel("base2")
    wth, owth = EC.weight_kernels(wl.radius)[wname]
    # ModSqExp is a profile of tau alone, one-dimensional whatever D: blend_profile_ok admits it here as it does for
    # pmk_query_mix and pmk_query_mix_vgrad (code 0), and only a profile that is no function of tau is refused (-2)
    q = M.DeviceQuery(model, wl.Xq)
    q.plan(wl.radius, wl.delta)
    q.items(wl.th)
    q.mix(wth)
    q.items_cov(wl.th)
    d, bb = wth.desc(), pmk.BrownianBridge10(1.0).desc()
    assert pmk.lib().pmk_query_mix_cov(q.h, C.byref(bb)) == -2
    assert pmk.lib().pmk_query_mix_cov(q.h, C.byref(d)) == 0
    out = blend_checks(wl, model, wth, owth)
    assert same_bits(q.fetch_cov(), out["Cov"])
    _record(group="C", test="weight_family", weight=wname, **out["ratios"])
    assert out["ratios"]["neighbour_items"] >= 40 and not out["shared"].all() and ratios_ok(out["ratios"]), out["ratios"]


@pytest.mark.parametrize("which", list(EC.C_RADII))
def test_more_neighbours_than_the_stage_holds(which):
    wl, model = _cmodel("many")
    radius = EC.C_RADII[which]
    wth, owth = EC.spline34_weight(radius)
    out = blend_checks(wl, model, wth, owth, radius=radius)
    cnt = np.diff(out["dbg"]["item_offsets"]) - 1
    _record(group="C", test="many_items", radius=radius, **out["ratios"])
    assert cnt.max() > EC.PLAN_STAGE and ratios_ok(out["ratios"]), out["ratios"]


def test_twelve_and_more_items_per_query():
    wl, model = _cmodel("polygon")
    wth, owth = EC.spline34_weight(wl.radius)
    out = blend_checks(wl, model, wth, owth)
    _record(group="C", test="twelve_items", leaves=len(wl.Xs), **out["ratios"])
    assert len(wl.Xs) == 2048 and out["q"].Nq == 48 and np.diff(out["dbg"]["item_offsets"]).min() >= 12
    assert out["shared"].all() and ratios_ok(out["ratios"]), out["ratios"]


def test_a_tree_at_four_dimensions():
    wl, model = _cmodel("L7_D4")
    wth, owth = EC.spline34_weight(wl.radius)
    out = blend_checks(wl, model, wth, owth)
    _record(group="C", test="d4_tree", **out["ratios"])
    assert wl.D == 4 and out["ratios"]["neighbour_items"] >= 40 and not out["shared"].all() and ratios_ok(out["ratios"]), out["ratios"]


def test_query_on_a_plane():
    wl, model = _cmodel("on_plane")
    wth, owth = EC.spline34_weight(wl.radius)
    out = blend_checks(wl, model, wth, owth)
    off, t, reg = out["dbg"]["item_offsets"], out["dbg"]["item_t"], out["dbg"]["item_region"]
    assert off[1] == 2 and t[0] == 0.0 and t[1] == 0.0 and reg[0] != reg[1]
    # w(0) = 1: both weights are 1/2, and Cov[0, 0] is a quarter of each item's variance, for bits
    S0, S1 = out["blocks"][int(reg[0])], out["blocks"][int(reg[1])]
    v0, v1 = S0[1][list(S0[0]).index(0), list(S0[0]).index(0)], S1[1][list(S1[0]).index(0), list(S1[0]).index(0)]
    assert same_bits(out["Cov"][0, 0], 0.25 * v0 + 0.25 * v1)
    wth2, owth2 = EC.weight_kernels(wl.radius)["trq"]                # w(0) = 0.7 against the home weight 1
    out2 = blend_checks(wl, model, wth2, owth2)
    _record(group="C", test="on_plane", trq=out2["ratios"], **out["ratios"])
    assert ratios_ok(out["ratios"]) and ratios_ok(out2["ratios"]), (out["ratios"], out2["ratios"])


@pytest.mark.parametrize("name", ["grid", "dups"])
def test_training_points_and_twins_as_queries(name):
    wl, model = _cmodel(name)
    wth, owth = EC.spline34_weight(wl.radius)
    out = blend_checks(wl, model, wth, owth)
    Cov, dbg = out["Cov"], out["dbg"]
    neighbour = np.ones(len(dbg["item_t"]), dtype=bool)
    neighbour[dbg["item_offsets"][1:] - 1] = False                   # the home item is the last of its query
    exact = int(np.sum(neighbour & (np.abs(dbg["item_t"]) < 1e-12)))
    rec = dict(group="C", test="training_points", case=name, items_on_a_plane=exact, **out["ratios"])
    if name == "dups":
        # twins: equal points have equal items, columns of V, Gram chains and blends, so their rows and columns are equal
        # bit for bit, and Cov[j, k] is the variance Cov[j, j] itself unless the diagonal was clamped
        groups = CE.twin_groups(wl.Xq)
        assert len(groups) >= 20
        # the blocks first: the rows of two twins in a region block are one Gram chain over equal columns of V
        for r, (idx, S) in out["blocks"].items():
            for g in groups:
                rows = [int(np.nonzero(idx == j)[0][0]) for j in g if np.count_nonzero(idx == j) == 1]
                assert all(same_bits(S[rows[0]], S[a]) and same_bits(S[rows[0], rows[0]], S[rows[0], a]) for a in rows[1:]), (r, g)
        d = np.diag(Cov)
        for g in groups:
            for k in g[1:]:
                j = g[0]
                assert same_bits(Cov[j], Cov[k]) and same_bits(Cov[:, j], Cov[:, k]), (j, k)
                assert d[j] > 10 * CE.MIN_V                          # far from the clamp
                assert same_bits(Cov[j, k], Cov[j, j]) and same_bits(Cov[k, k], Cov[j, j]), (j, k)
        rec.update(twin_groups=len(groups), smallest_twin_variance=float(min(d[g[0]] for g in groups)))
    _record(**rec)
    assert exact >= 10 and ratios_ok(out["ratios"]), rec


def same_home_count(home):
    return int((home[:, None] == home[None, :]).sum())


@pytest.mark.parametrize("radius", [0.0, 1e300])
def test_plan_radius_zero_and_huge(radius):
    wl, model = _cmodel("base2")
    wth, owth = EC.weight_kernels(0.8)["gaussian"]
    out = blend_checks(wl, model, wth, owth, radius=radius)
    q, Cov = out["q"], out["Cov"]
    if radius == 0.0:
        # home items alone: Cov is nonzero only inside the groups of one home leaf, and is the home block itself there
        home = out["dbg"]["home"]
        assert q.total == q.Nq
        same_home = home[:, None] == home[None, :]
        assert np.array_equal(out["shared"], same_home) and np.all(Cov[~same_home] == 0) and np.count_nonzero(Cov[same_home]) > 0
        for r, (idx, S) in out["blocks"].items():
            assert same_bits(Cov[np.ix_(idx, idx)], S), r
    else:
        assert out["ratios"]["neighbour_items"] >= 300 and out["shared"].sum() > same_home_count(out["dbg"]["home"])
    _record(group="C", test="plan_radius", radius=radius, **out["ratios"])
    assert ratios_ok(out["ratios"]), out["ratios"]


def test_an_fp32_model_blends_in_double():
    wl, model = _cmodel("base2_f32")
    wth, owth = EC.spline34_weight(wl.radius)
    out = blend_checks(wl, model, wth, owth)
    _record(group="C", test="f32_model", **out["ratios"])
    assert wl.dtype == "f32" and out["ratios"]["neighbour_items"] >= 40 and ratios_ok(out["ratios"]), out["ratios"]


def test_batches_around_the_tile_of_the_blend_keep_their_bits():
    wl, model = _cmodel("base2")
    wth, owth = EC.spline34_weight(wl.radius)
    full = blend_checks(wl, model, wth, owth)
    Cov = full["Cov"]
    for n in CE.C_NQ_EDGES:
        # the first n queries, in their order
        qn = _staged(model, wl.Xq[:n], wl.radius, wl.delta, wl.th, wth)
        got = qn.fetch_cov()
        assert got.shape == (n, n) and same_bits(got, Cov[:n, :n]), n
    # and in another order: an entry sums over its regions in ascending region index, whichever query comes first
    order = np.random.default_rng(8).permutation(full["q"].Nq)[:33]
    assert np.any(np.diff(order) < 0) and (full["shared"][np.ix_(order, order)].sum() - 33) // 2 >= 100
    got = _staged(model, wl.Xq[order], wl.radius, wl.delta, wl.th, wth).fetch_cov()
    assert same_bits(got, Cov[np.ix_(order, order)])
    # no query at all: every stage answers 0 and the result is a (0, 0) array
    L = pmk.lib()
    q0 = M.DeviceQuery(model, np.zeros((0, wl.D)))
    assert q0.plan(wl.radius, wl.delta) == 0
    q0.items(wl.th)
    q0.mix(wth)
    d, w = wl.th.desc(), wth.desc()
    buf = np.full((1, 1), -7.0)
    assert L.pmk_query_items_cov(q0.h, C.byref(d)) == 0 and L.pmk_query_mix_cov(q0.h, C.byref(w)) == 0
    assert L.pmk_query_fetch_cov(q0.h, M._d(buf), 1) == 0 and buf[0, 0] == -7.0
    assert q0.fetch_cov().shape == (0, 0)
    _record(group="C", test="nq_edges", sizes=[0] + CE.C_NQ_EDGES, **full["ratios"])
    assert ratios_ok(full["ratios"]), full["ratios"]


def test_padded_leading_dimensions_of_the_fetches():
    import torch
    wl, model = _cmodel("base2")
    wth, _ = EC.spline34_weight(wl.radius)
    q = _staged(model, wl.Xq, wl.radius, wl.delta, wl.th, wth)
    Cov = q.fetch_cov()
    Nq, L = q.Nq, pmk.lib()
    # pmk_query_fetch_cov_dev with ldc = Nq + 3: the same bits, the padding untouched
    dev = torch.device("cuda", model.ctx.device)
    out = torch.full((Nq, Nq + 3), -7.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    assert L.pmk_query_fetch_cov_dev(q.h, C.c_void_p(out.data_ptr()), Nq + 3) == 0
    model.ctx.synchronize()
    host = out.cpu().numpy()
    assert same_bits(host[:, :Nq], Cov) and np.all(host[:, Nq:] == -7.0)
    assert L.pmk_query_fetch_cov_dev(q.h, C.c_void_p(out.data_ptr()), Nq - 1) == -4
    # pmk_query_get_items_cov with lds = m + 3
    regions = 0
    for r in range(len(wl.Xs)):
        idx, S = q.item_covs(r)
        m = len(idx)
        if m == 0:
            continue
        idx2 = np.full(m, -1, dtype=np.int32)
        S2 = np.full((m, m + 3), -7.0)
        assert L.pmk_query_get_items_cov(q.h, r, None, idx2.ctypes.data_as(C.POINTER(C.c_int32)), M._d(S2), m + 3) == 0
        assert np.array_equal(idx2, idx) and same_bits(S2[:, :m], S) and np.all(S2[:, m:] == -7.0), r
        assert L.pmk_query_get_items_cov(q.h, r, None, None, M._d(S2), m - 1) == -4
        regions += 1
    _record(group="C", test="padded_fetch", Nq=int(Nq), regions=regions)
    assert regions == len(wl.Xs)


# ------------------------------------------------------------------------------------------ D. draws
def _main_eta(m, model=None):
    """the eta of the main workload, fitted through fitmixtureGP_, or carrying `model` (fitted through the staged route)"""
    th, _ = CC.FAMILIES["spline34"]
    eta = pmk.MixtureGPType(m.Xs, pmk.fetchhyperplanes(m.root))
    if model is None:
        pmk.fitmixtureGP_(eta, [np.ascontiguousarray(m.y[i]) for i in m.inds], th, SIGMA2["f64"])
    else:
        eta._model = model
    return eta


def test_draws_of_duplicated_queries():
    import torch
    m = _main("f64")
    th, oth = CC.FAMILIES["spline34"]
    eta = _main_eta(m)
    X8 = CE.corner_queries(m)
    Xq = np.vstack([X8, X8])
    Nq, n, u = 16, 2048, U_OF["f64"]
    args = (Xq, eta, m.root, m.LEVELS, m.RADIUS, m.DELTA, m.wth)
    Yq, Vq, Cov = pmk.querymixtureGP_cov(*args)
    for j in range(8):
        assert same_bits(Cov[j], Cov[j + 8]) and same_bits(Cov[j, j + 8], Cov[j, j]) and same_bits(Yq[j], Yq[j + 8])
    dev = torch.device("cuda", 0)
    z = torch.randn((n, Nq), dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    draws, jitter = pmk.samplemixtureGP(*args, n, z=z)                # returns: the ladder reaches a factorisation
    assert tuple(draws.shape) == (n, Nq) and bool(torch.isfinite(draws).all())
    scale = float(np.trace(Cov)) / Nq
    ladder = CE.jitter_ladder(scale)
    step = int(np.argmin([abs(jitter - v) for v in ladder]))
    assert jitter == 0.0 if step == 0 else abs(jitter - ladder[step]) <= 1e-12 * ladder[step], (jitter, ladder)
    # draws - Yq is z L^T with L L^T = Cov + jitter I, within the bound of test_gpu_cov.test_posterior_draws: 10 units of
    # the blended entries plus 2 (Nq + 1) u sqrt(C_ii C_jj) for the Cholesky in double (Higham, Accuracy and Stability,
    # Thm 10.3) and the recovery of L from z
    Lt = torch.linalg.lstsq(z, draws - torch.as_tensor(Yq, device=dev)[None, :]).solution
    Lh = Lt.cpu().numpy().T
    q = _staged(eta._model, Xq, m.RADIUS, m.DELTA, th, m.wth, fitted=True)
    assert same_bits(q.fetch_cov(), Cov)
    refs = {r: _ref(("main", r), oth, m.Xs[r], SIGMA2["f64"]) for r in range(4)}
    _, _, S_ref, units = _check_blocks(_device_blocks(q, 4), Xq, refs, "f64")
    dbg = q.debug()
    _, unit = CR.mix_cov_ref((dbg["item_offsets"], dbg["item_region"]), S_ref, dbg["item_t"], m.owth, units)
    A = Cov + jitter * np.eye(Nq)
    bound = RATIO_MAX * unit + 2 * (Nq + 1) * u * np.sqrt(np.outer(np.diag(A), np.diag(A)))
    ratio = RATIO_MAX * float((np.abs(Lh @ Lh.T - A) / bound).max())
    # a twin pair: draws_j - draws_k = z . (l_j - l_k) for the rows l of L, and |l_j - l_k|^2 = A_jj + A_kk - 2 A_jk of
    # L L^T = A + E; Cov_jj = Cov_kk = Cov_jk for bits, so the jitter leaves 2 jitter and E at most bound_jj + bound_kk +
    # 2 bound_jk.  By Cauchy-Schwarz |draws_ij - draws_ik| <= |z_i| sqrt(that), plus the roundings of the two products in
    # double, 2 (Nq + 2) u (|Yq_j| + |z_i| . |l_j|)
    zh = z.cpu().numpy()
    dh = draws.cpu().numpy()
    znorm = np.sqrt((zh * zh).sum(1))
    worst_diff = worst_twin = 0.0
    for j in range(8):
        k = j + 8
        gap = np.sqrt(2 * jitter + bound[j, j] + bound[k, k] + 2 * bound[j, k])
        allow = znorm * gap + 2 * (Nq + 2) * u * (abs(Yq[j]) + np.abs(zh) @ np.abs(Lh[j]))
        diff = np.abs(dh[:, j] - dh[:, k])
        worst_diff = max(worst_diff, float(diff.max()))
        worst_twin = max(worst_twin, float((diff / allow).max()))
    _record(group="D", test="duplicated_queries", jitter=jitter, ladder_step=step, scale=scale, llt_ratio=ratio,
            worst_twin_difference=worst_diff, twin_difference_over_allowance=worst_twin, smallest_variance=float(np.diag(Cov).min()))
    assert ratio <= RATIO_MAX and worst_twin <= 1.0, (ratio, worst_twin)


def test_draws_of_one_query():
    import torch
    m = _main("f64")
    eta = _main_eta(m)
    Xq = CE.corner_queries(m)[:1]
    args = (Xq, eta, m.root, m.LEVELS, m.RADIUS, m.DELTA, m.wth)
    Yq, Vq, Cov = pmk.querymixtureGP_cov(*args)
    assert Cov.shape == (1, 1) and Cov[0, 0] > 0
    n = 257
    z = np.random.default_rng(4).standard_normal((n, 1))             # a numpy z is accepted
    draws, jitter = pmk.samplemixtureGP(*args, n, z=z)
    assert jitter == 0.0 and tuple(draws.shape) == (n, 1)
    s = np.sqrt(Cov[0, 0])
    want = Yq[0] + z[:, 0] * s
    # the square root, the product and the sum round once each: a few ulp of the larger operand
    tol = 4 * 2.0 ** -52 * (abs(Yq[0]) + np.abs(z[:, 0]) * s)
    err = np.abs(draws.cpu().numpy()[:, 0] - want)
    _record(group="D", test="one_query", worst_err_over_tol=float((err / tol).max()))
    assert np.all(err <= tol)
    dev = torch.device("cuda", 0)
    zt = torch.as_tensor(z, device=dev)
    again, _ = pmk.samplemixtureGP(*args, n, z=zt)
    assert torch.equal(again, draws)
    for bad in (np.zeros((n, 2)), np.zeros((n + 1, 1)), np.zeros(n)):
        with pytest.raises(ValueError):
            pmk.samplemixtureGP(*args, n, z=bad)


def test_draws_of_a_batch_that_touches_a_failed_patch():
    import torch
    m = _main("f64")
    th, _ = CC.FAMILIES["spline34"]
    # fitmixtureGP_ raises on a failed patch, so the model is fitted through the staged route and handed to an eta
    broken = M.DeviceModel(m.Xs, [np.ascontiguousarray(m.y[i]) for i in m.inds], dtype="f64")
    diag = [np.zeros(len(x)) for x in m.Xs]
    diag[2][3] = -3.0                                                # the factorisation of this patch fails
    broken.set_diag(diag)
    broken.fit(th, SIGMA2["f64"])
    assert broken.info()[2] != 0 and np.all(np.delete(broken.info(), 2) == 0)
    eta = _main_eta(m, broken)
    X8 = CE.corner_queries(m)
    args = (X8, eta, m.root, m.LEVELS, m.RADIUS, m.DELTA, m.wth)
    _, _, Cov = pmk.querymixtureGP_cov(*args)
    assert np.isnan(Cov).any()                                       # the corner queries blend the failed patch
    with pytest.raises(np.linalg.LinAlgError, match="NaN"):
        pmk.samplemixtureGP(*args, 64)
    # what torch makes of such a matrix, for the record: the reason the function looks before it factors
    _, info = torch.linalg.cholesky_ex(torch.as_tensor(Cov, device=torch.device("cuda", 0)))
    # queries of the same model that avoid the failed patch still draw
    q = M.DeviceQuery(broken, m.Xq)
    q.plan(m.RADIUS, m.DELTA)
    dbg = q.debug()
    off, reg = dbg["item_offsets"], dbg["item_region"]
    clean = np.array([not (reg[off[j]:off[j + 1]] == 2).any() for j in range(len(m.Xq))])
    Xc = m.Xq[clean][:8]
    assert len(Xc) == 8
    draws, jitter = pmk.samplemixtureGP(Xc, eta, m.root, m.LEVELS, m.RADIUS, m.DELTA, m.wth, 64,
                                        generator=torch.Generator(device=torch.device("cuda", 0)).manual_seed(5))
    assert tuple(draws.shape) == (64, 8) and bool(torch.isfinite(draws).all())
    _record(group="D", test="failed_patch", cholesky_ex_info_on_nan=int(info), jitter_of_the_clean_batch=jitter,
            nan_entries=int(np.isnan(Cov).sum()))

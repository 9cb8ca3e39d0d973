"""The gradient of the blended variance on the GPU at its edges (vgrad_strip_kernel, item_trend_grads_kernel,
trend_vgrad_kernel and mix_vgrad_kernel of pmk_vgrad.hip, the capacity-grown buffers of pmk_query_items_vgrad /
pmk_query_mix_vgrad), on the inputs of tests/_vgrad_edge_cases.py and the workloads of tests/_grad_edge_cases.py;
tests/test_vgrad_edges_refs.py asserts on the CPU what each input was chosen for.

  A. more strips than workgroups: 2 ncu + 3 strips, so that a workgroup runs a second and a third pass of its task loop
     (parked products zeroed again, the ring of point tiles and the strip workspace reused after a patch of another nt, a
     full strip behind a strip of one item);
  B. the clamp on the device: a patch of separated points with a tiny sigma2, where k(x,x) - b < min_v without any ABI
     route to min_v; under a trend the clamp holds the simple-kriging part only;
  C. the trend's sibling kernel with its q columns at R = 1 and at R = 16 - q, item lists of 1 .. 257 items in more than 32
     chunks of 16, patches of 5, 6 and 7 block rows;
  D. the blend: every family as the blending profile, more neighbours than PLAN_STAGE and 12 to 14 items, t == 0, training
     points as queries, plan radii 0, 1e150 and 1e300, query ranges off the 256-thread blocks, re-plans and a trend that is
     set, cleared and set again on one query, the order of the calls, mixed families per patch.

Bounds, all those of tests/test_gpu_vgrad.py:
  items    err <= RATIO_MAX (n + 32) u unit against _vgrad_refs.PatchRef, RATIO_MAX = 10; under a trend the trend's part
           GV - GV0 (GV0: the same model without the trend) within TREND_RATIO_MAX = 1 of its own unit;
  blend    |err| <= 16 m 2^-53 mag against mix_vgrad_ref fed with the device's own items; on the lattice workload a query
           on which a plain float64 evaluation of the same formula exceeds this bound is left out, as the item checks leave
           out such inputs (vblend_ratio: slopes dw that cancel in sum_j dw_j; 3 of 512 queries);
  fd       central differences of the device's own Vq, h = 2^-17 of the domain width, tolerance
           |fd_2h - fd_h| + 2 eps_f / h, on 16 queries whose item signature is constant over the stencil (fp64 models);
  bits     np.array_equal on the uint64 views wherever a test says "bits".

Every measured ratio is printed ("VGRADEDGE {json}", run with -s); a run of the whole module writes them to
profiles/vgrad_edges_accuracy.json.
"""
import ctypes as C
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest

import patchmixturekriging_amd as pmk
from patchmixturekriging_amd import mixture as M

import _grad_edge_cases as EC
import _vgrad_edge_cases as VE
import _vgrad_refs as VR
import test_gpu_grad_edges as GE
from test_gpu_grad import FAMILIES, U_OF, Blend, _explicit_query, _model, _round, _targets, _tree8, _worst_ratio
from test_gpu_vgrad import RATIO_MAX, SIGMA2, TREND_RATIO_MAX, _predict_var, _staged

pytestmark = pytest.mark.gpu

_RECORDS = []
TESTS = {"schedule", "clamp", "clamp_trend", "clamp_blend", "trend_columns", "trend_chunks", "block_rows", "weight_family",
         "many_items", "twelve_items", "deep_tree", "staged_vs_walk", "on_plane", "training_points", "huge_radius", "ranges",
         "buffer_lifetime", "mixed_families"}
ACCURACY_JSON = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "vgrad_edges_accuracy.json")
same_bits = GE.same_bits


def _record(**kw):
    _RECORDS.append(kw)
    print("VGRADEDGE " + json.dumps(kw, sort_keys=True))


@pytest.fixture(scope="module", autouse=True)
def _write_accuracy_file():
    """only a run of the whole module replaces the file"""
    yield
    if {r["test"] for r in _RECORDS} >= TESTS:
        with open(ACCURACY_JSON, "w") as f:
            f.write("[\n" + ",\n".join(" " + json.dumps(r, sort_keys=True) for r in _RECORDS) + "\n]\n")


# ------------------------------------------------------------------------------------------ items
def _fit_patches(Xs, Ys, thetas, sigma2s, dtype, trend=None):
    """test_gpu_grad._model with a noise of its own for every patch"""
    model = M.DeviceModel(Xs, [np.ascontiguousarray(y[:, 0]) for y in Ys], dtype=dtype)
    model.fit_patches(thetas, sigma2s)
    model.set_targets_multi(Ys)
    model.set_trend(trend)
    model.solve_multi()
    model.set_bsp(_tree8(Xs[0].shape[1]), 0)
    return model


def _run_items(model, xq, region, th):
    """explicit items through items_multi and items_vgrad (th None: the model's own kernels); U and v keep their bits"""
    q = _explicit_query(model, xq, region)
    if th is None:
        q.items_multi_fitted(True)
    else:
        q.items_multi(th, True)
    U0, v0 = q.item_values_multi()
    q.items_vgrad(th)
    U1, v1 = q.item_values_multi()
    assert same_bits(U1, U0) and same_bits(v1, v0)
    return q


def _clear_trend(model):
    model.set_trend(None)
    model.solve_multi()


def item_ratios(GV, xq, region, refs, dtype, GV0=None, flagged=()):
    """test_gpu_vgrad._item_ratios with the references passed in (region -> PatchRef, built once) and without its
    assertion that no item is clamped: PatchRef.items holds a clamped item to the trend's part alone -> (worst err / e_d,
    largest kappa2(L), worst error of the trend's part GV - GV0 over its own unit)"""
    worst, kappa, worst_trend = 0.0, 0.0, 0.0
    u = U_OF[dtype]
    for r in sorted(set(int(x) for x in region)):
        sel = np.nonzero(region == r)[0]
        if r in flagged:
            assert np.all(np.isnan(GV[sel])), r
            continue
        ref = refs[r]
        kappa = max(kappa, ref.kappa()[0])
        out = ref.items(xq[sel])
        assert np.all(np.isfinite(GV[sel])), r
        err = np.abs(np.asarray(GV[sel], dtype=VR.LD) - out["grad"]).astype(np.float64)
        worst = max(worst, _worst_ratio(err, (ref.n + 32) * u * out["unit"]))
        if GV0 is not None:
            assert np.all(np.isfinite(GV0[sel])), r
            part = np.asarray(GV[sel], dtype=VR.LD) - np.asarray(GV0[sel], dtype=VR.LD)
            err = np.abs(part - out["trend"]).astype(np.float64)
            round2 = 4 * 2.0 ** -53 * np.abs(out["grad"]).astype(np.float64)      # the device's sum and this difference
            worst_trend = max(worst_trend, _worst_ratio(np.maximum(err - round2, 0.0), (ref.n + 32) * u * out["tunit"]))
    return worst, kappa, worst_trend


def _flagged(Xs, trend):
    return {r for r, X in enumerate(Xs) if len(X) < VE.trend_q(trend, X.shape[1])}


# ------------------------------------------------------------------------------------------ A. more strips than workgroups
@pytest.mark.parametrize("D,dtype,trend", VE.A_CASES)
def test_a_workgroup_runs_several_strips(D, dtype, trend):
    import torch
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    th, oth = FAMILIES["spline34"]
    Xs = VE.a_patches(D, dtype)
    counts = VE.a_counts(ncu, D)
    s = VE.schedule(counts, VE.A_SIZES, D, ncu)
    assert s["strips"] == 2 * ncu + 3 and s["grid"] == ncu and s["most_tasks"] == 3, s
    assert s["nt_down"] >= 1 and s["nt_up"] >= 1 and s["full_after_one"] >= 1, s
    xq, region = VE.items_of(VE.A_SEED + D, Xs, counts, dtype)
    model = _model(Xs, [_targets(X, 1) for X in Xs], th, dtype, trend)
    assert np.all(model.info() == 0)
    flagged = _flagged(Xs, trend)
    assert flagged == ({3} if trend else set())
    GV = _run_items(model, xq, region, th).item_vgrads()
    # bits: the same items in sub-queries of at most ncu strips, where every workgroup has one task
    parts = [_run_items(model, xq[lo:hi], region[lo:hi], th).item_vgrads() for lo, hi in VE.a_pieces(counts, D, ncu)]
    assert same_bits(np.vstack(parts), GV)
    # accuracy: the first, the middle and the last item of every region
    pick = VE.ends_and_middle(counts)
    GV0 = None
    if trend:
        _clear_trend(model)
        GV0 = _run_items(model, xq[pick], region[pick], th).item_vgrads()
    refs = {r: VE.patch_ref(("A", D, dtype, r), oth, Xs[r], SIGMA2[dtype], trend) for r in range(8) if r not in flagged}
    worst, kappa, worst_trend = item_ratios(GV[pick], xq[pick], region[pick], refs, dtype, GV0, flagged)
    _record(group="A", test="schedule", D=D, dtype=dtype, trend=trend, ncu=int(ncu), items=int(len(xq)), ratio=worst, kappa=kappa,
            trend_ratio=worst_trend, **s)
    assert kappa <= VR.KAPPA_MAX and worst <= RATIO_MAX and worst_trend <= TREND_RATIO_MAX, (kappa, worst, worst_trend)


# ------------------------------------------------------------------------------------------ B. the clamp
def _clamp_model(family, dtype, trend=None, tiny=True):
    th, oth = FAMILIES[family]
    Xs, xq, region, kind = VE.b_inputs(family, dtype)
    s2 = [SIGMA2[dtype]] * 8
    if tiny:
        s2[VE.B_PATCH] = VE.B_SIGMA2[dtype]
    model = _fit_patches(Xs, [_targets(X, 1) for X in Xs], [th] * 8, s2, dtype, trend)
    assert np.all(model.info() == 0)
    return model, Xs, xq, region, kind


def _clamp_refs(family, dtype, Xs, trend, flagged):
    oth = FAMILIES[family][1]
    refs = {r: VE.patch_ref(("B", "ordinary", family, dtype, r), oth, Xs[r], SIGMA2[dtype], trend) for r in range(8)
            if r != VE.B_PATCH and r not in flagged}
    refs[VE.B_PATCH] = VE.patch_ref(("B", family, dtype), oth, Xs[VE.B_PATCH], VE.B_REF_SIGMA2[dtype], trend)
    return refs


@pytest.mark.parametrize("family,dtype", VE.B_FAMILIES)
def test_the_clamp_holds_on_the_device(family, dtype):
    model, Xs, xq, region, kind = _clamp_model(family, dtype)
    q = _run_items(model, xq, region, None)
    GV, v = q.item_vgrads(), q.item_values_multi()[1]
    sep = region == VE.B_PATCH
    Gs, vs = GV[sep], v[sep]
    clamped, inside, outside = kind == VE.CLAMPED, kind == VE.INSIDE, kind == VE.OUTSIDE
    assert np.array_equal(vs == VE.MIN_V, clamped), vs
    zero = np.zeros((1, 2))
    assert same_bits(Gs[clamped], np.repeat(zero, clamped.sum(), 0))                 # + 0.0 in all D components
    assert np.all(vs[outside] == 1.0) and same_bits(Gs[outside], np.repeat(zero, outside.sum(), 0))
    assert np.all(Gs[inside] != 0)
    refs = _clamp_refs(family, dtype, Xs, None, set())
    worst, kappa, _ = item_ratios(GV, xq, region, refs, dtype)
    worst_inside, _, _ = item_ratios(Gs[inside], xq[sep][inside], region[sep][inside], refs, dtype)
    # the other seven patches do not notice: a model whose eighth patch has the ordinary noise gives them the same bits
    model2 = _clamp_model(family, dtype, tiny=False)[0]
    q2 = _run_items(model2, xq, region, None)
    assert same_bits(q2.item_vgrads()[~sep], GV[~sep]) and same_bits(q2.item_values_multi()[1][~sep], v[~sep])
    assert not np.any(q2.item_values_multi()[1][sep] == VE.MIN_V)
    _record(group="B", test="clamp", family=family, dtype=dtype, ratio=worst, ratio_inside_a_support=worst_inside, kappa=kappa,
            clamped=int(clamped.sum()))
    assert kappa <= VR.KAPPA_MAX and worst <= RATIO_MAX, (kappa, worst)


@pytest.mark.parametrize("trend", ["constant", "linear"])
def test_a_clamped_item_keeps_the_trends_part(trend):
    family, dtype = "spline34", "f64"
    model, Xs, xq, region, kind = _clamp_model(family, dtype, trend)
    flagged = _flagged(Xs, trend)
    assert np.all(np.delete(model.trend_info(), sorted(flagged)) == 0)
    q = _run_items(model, xq, region, None)
    GV, v = q.item_vgrads(), q.item_values_multi()[1]
    _clear_trend(model)
    q0 = _run_items(model, xq, region, None)
    GV0, v0 = q0.item_vgrads(), q0.item_values_multi()[1]
    sep = np.nonzero(region == VE.B_PATCH)[0]
    held = sep[kind == VE.CLAMPED]
    assert np.all(v0[held] == VE.MIN_V) and same_bits(GV0[held], np.zeros((len(held), 2)))
    assert np.all(v[held] >= VE.MIN_V) and np.all(np.isfinite(GV[held]))
    refs = _clamp_refs(family, dtype, Xs, trend, flagged)
    # the clamped items alone: GV is the trend's part, GV0 is exactly zero
    w_held, _, wt_held = item_ratios(GV[held], xq[held], region[held], refs, dtype, GV0[held])
    worst, kappa, worst_trend = item_ratios(GV, xq, region, refs, dtype, GV0, flagged)
    if trend == "linear":
        assert np.any(GV[held] != 0)                                 # 2 z . y_d with y_d = L_G^-1 e_{1+d}
    _record(group="B", test="clamp_trend", trend=trend, ratio=worst, trend_ratio=worst_trend, clamped_ratio=w_held,
            clamped_trend_ratio=wt_held, kappa=kappa, kappa_LG=refs[VE.B_PATCH].kappa()[1])
    assert wt_held <= TREND_RATIO_MAX and w_held <= RATIO_MAX, (wt_held, w_held)
    assert kappa <= VR.KAPPA_MAX and worst <= RATIO_MAX and worst_trend <= TREND_RATIO_MAX, (kappa, worst, worst_trend)


CANCEL_MIN = 16.0


def vblend_ratio(q, hp_v, owth, lattice=None):
    """worst err / bound of fetch_vgrad against mix_vgrad_ref fed with the device's own items -> (ratio, largest m,
    neighbour items).

    lattice: a dict, for the workloads on a lattice.  There two parallel planes at t and -t give a query weight slopes
    that cancel in sum_j dw_j, and the bound, stated in the magnitudes after that cancellation, cannot be met in double
    (_vgrad_edge_cases.plain_mix_vgrad).  The rule of the item checks decides: a query on which a plain float64 numpy
    evaluation of the same formula, fed with the same items, itself exceeds the bound is unsuitable and left out of the
    ratio; a device result above the bound where the plain evaluation is not stays a failure.  An unsuitable query must
    show the cause, a magnitude before the cancellation (mag2) of more than CANCEL_MIN = 16 times the one after it (the
    whole factor of the bound), and is held to 16 m 2^-53 mag2 instead.  The dict receives unsuitable (count),
    unsuitable_plain_ratio, unsuitable_device_ratio (worst, of the bound) and unsuitable_wide_ratio (of the wider one)."""
    dV = q.fetch_vgrad()
    v = q.item_values_multi()[1]
    GV = q.item_vgrads()
    plane = q.item_grads()[1]
    dbg = q.debug()
    off, t = dbg["item_offsets"], dbg["item_t"]
    assert np.all(np.isfinite(dV))
    worst = 0.0
    out = dict(unsuitable=0, unsuitable_plain_ratio=0.0, unsuitable_device_ratio=0.0, unsuitable_wide_ratio=0.0)
    for j in range(q.Nq):
        items = range(off[j], off[j + 1])
        ref, mag = VR.mix_vgrad_ref(items, GV, v, t, plane, hp_v, owth)
        c = 16 * len(items) * 2.0 ** -53
        bound = c * mag.astype(np.float64)
        err = np.abs(np.asarray(dV[j], dtype=VR.LD) - ref).astype(np.float64)
        ratio = _worst_ratio(err, bound)
        if lattice is not None and len(items) > 1:
            plain, mag2 = VE.plain_mix_vgrad(items, GV, v, t, plane, hp_v, owth)
            plain_ratio = _worst_ratio(np.abs(np.asarray(plain, dtype=VR.LD) - ref).astype(np.float64), bound)
            if plain_ratio > 1.0:
                assert np.any(mag2 > CANCEL_MIN * mag.astype(np.float64)), (j, plain_ratio, mag2, mag)
                wide = _worst_ratio(err, c * mag2)
                out.update(unsuitable=out["unsuitable"] + 1, unsuitable_plain_ratio=max(out["unsuitable_plain_ratio"], plain_ratio),
                           unsuitable_device_ratio=max(out["unsuitable_device_ratio"], ratio),
                           unsuitable_wide_ratio=max(out["unsuitable_wide_ratio"], wide))
                assert wide <= 1.0, (j, wide)
                continue
        worst = max(worst, ratio)
    if lattice is not None:
        assert out["unsuitable"] <= q.Nq // 50                       # a few queries of the lattice, not the workload
        lattice.update(out)
    return worst, int(np.diff(off).max()), int(off[-1] - q.Nq)


@pytest.mark.parametrize("trend", [None, "linear"])
def test_the_blend_of_clamped_items(trend):
    wl = EC.workload("grid")
    th = pmk.Spline34KernelType(VE.B_BLEND_THETA)
    Ys = wl.Ys(2)
    model = M.DeviceModel(wl.Xs, [np.ascontiguousarray(y[:, 0]) for y in Ys], dtype="f64")
    model.fit(th, VE.B_BLEND_SIGMA2)
    model.set_targets_multi(Ys)
    model.set_trend(trend)
    model.solve_multi()
    assert np.all(model.info() == 0)
    model.set_bsp(wl.root, 0)
    Xq = np.vstack([wl.Xq, np.random.default_rng(77).uniform(-wl.box, wl.box, wl.Xq.shape)])
    # A Gaussian blending profile.  Where the home item is clamped (GV = 0, v = 1e-12) and the neighbour lies outside every
    # support (GV = 0, v = 1), dVq is the neighbour's weight term alone, and a compact profile would be judged on its own
    # conditioning: every neighbour of a lattice point sits at |t| = 0.53 of a radius 0.6, where the rounding of r = a |t|
    # is 47 u of (1 - r)^11 against a bound of 32 u, and a plain float64 evaluation reaches 1.14 of the bound
    wth, owth = EC.weight_kernels(wl.radius)["gaussian"]
    q = M.DeviceQuery(model, Xq)
    q.plan(wl.radius, wl.delta)
    q.items_multi(th, True)
    q.items_grad(th)
    q.items_vgrad(th)
    q.mix_multi(wth)
    q.mix_grad(wth)
    q.mix_vgrad(wth)
    lat = {}
    ratio, m, n_nb = vblend_ratio(q, wl.hp_v, owth, lat)
    rec = dict(group="B", test="clamp_blend", trend=trend, ratio=ratio, neighbour_items=n_nb, **lat)
    if trend is None:
        # queries with every item clamped: GV is +0.0 there and dVq is the weight term sum 2 wn_i v_i dwn_i alone
        v, GV, dV = q.item_values_multi()[1], q.item_vgrads(), q.fetch_vgrad()
        off = q.debug()["item_offsets"]
        held = v == VE.MIN_V
        full = np.array([off[j + 1] - off[j] > 1 and held[off[j]:off[j + 1]].all() for j in range(q.Nq)])
        assert full.sum() >= 10 and held.sum() >= len(wl.Xq) and not held.all()
        assert same_bits(GV[held], np.zeros((held.sum(), 2)))
        assert np.any(dV[full] != 0)
        free_nb = int(sum(1 for j in range(q.Nq) if off[j + 1] - off[j] > 1 and not held[off[j]:off[j + 1]].any()))
        rec.update(clamped_items=int(held.sum()), queries_all_clamped=int(full.sum()), queries_with_neighbours_none_clamped=free_nb)
    _record(**rec)
    assert n_nb >= 40 and ratio <= 1.0, (n_nb, ratio)


# ------------------------------------------------------------------------------------------ C. columns, chunks, block rows
@pytest.mark.parametrize("D,dtype,trend,R", VE.C_COLUMN_CASES)
def test_trend_columns_at_both_ends_of_the_block(D, dtype, trend, R):
    th, oth = FAMILIES["spline34"]
    Xs, xq, region = VE.c_column_inputs(D, dtype)
    assert R + VE.trend_q(trend, D) <= 16
    model = _model(Xs, [_targets(X, R) for X in Xs], th, dtype, trend)
    assert np.all(model.info() == 0)
    flagged = _flagged(Xs, trend)
    GV = _run_items(model, xq, region, th).item_vgrads()
    _clear_trend(model)
    GV0 = _run_items(model, xq, region, th).item_vgrads()
    refs = {r: VE.patch_ref(("Ccol", D, dtype, r), oth, Xs[r], SIGMA2[dtype], trend) for r in range(8) if r not in flagged}
    worst, kappa, worst_trend = item_ratios(GV, xq, region, refs, dtype, GV0, flagged)
    _record(group="C", test="trend_columns", D=D, dtype=dtype, trend=trend, R=R, ratio=worst, trend_ratio=worst_trend, kappa=kappa)
    assert kappa <= VR.KAPPA_MAX and worst <= RATIO_MAX and worst_trend <= TREND_RATIO_MAX, (kappa, worst, worst_trend)


@pytest.mark.parametrize("D,dtype", VE.C_CHUNK_CASES)
def test_trend_items_keep_their_bits_whatever_shares_their_chunk(D, dtype):
    th, oth = FAMILIES["spline34"]
    Xs = VE.c_chunk_patches(D, dtype)
    model = _model(Xs, [_targets(X, 1) for X in Xs], th, dtype, "linear")
    assert np.all(model.info() == 0) and np.all(model.trend_info() == 0)
    rng = np.random.default_rng(550 + D)
    runs = []
    for k, batch in enumerate(VE.C_CHUNK_BATCHES):
        chunks = VE.chunk_count(batch)
        assert chunks > 32 and chunks % 8 != 0
        xq, region = VE.items_of(1500 + 10 * D + k, Xs, batch, dtype)
        GV = _run_items(model, xq, region, th).item_vgrads()
        assert np.all(np.isfinite(GV))
        # the same items in another order, with other companions in front of them and between them
        perm = rng.permutation(len(region))
        extra_r = rng.integers(0, 8, 37).astype(np.int32)
        extra_x = _round(rng.uniform(-2.5, 2.5, (37, D)), dtype)
        q2 = _run_items(model, np.vstack([extra_x[:20], xq[perm], extra_x[20:]]),
                        np.concatenate([extra_r[:20], region[perm], extra_r[20:]]), th)
        assert same_bits(q2.item_vgrads()[20:20 + len(region)], GV[perm]), k
        runs.append((batch, xq, region, GV))
    # accuracy, the trend's part included, at both ends and in the middle of every region's list
    _clear_trend(model)
    refs = {r: VE.patch_ref(("Cchunk", D, dtype, r), oth, Xs[r], SIGMA2[dtype], "linear") for r in range(8)}
    worst = kappa = worst_trend = 0.0
    for batch, xq, region, GV in runs:
        pick = VE.ends_and_middle(batch)
        GV0 = _run_items(model, xq[pick], region[pick], th).item_vgrads()
        w, kp, wt = item_ratios(GV[pick], xq[pick], region[pick], refs, dtype, GV0)
        worst, kappa, worst_trend = max(worst, w), max(kappa, kp), max(worst_trend, wt)
    _record(group="C", test="trend_chunks", D=D, dtype=dtype, ratio=worst, trend_ratio=worst_trend, kappa=kappa,
            chunks=[VE.chunk_count(b) for b in VE.C_CHUNK_BATCHES])
    assert kappa <= VR.KAPPA_MAX and worst <= RATIO_MAX and worst_trend <= TREND_RATIO_MAX, (kappa, worst, worst_trend)


@pytest.mark.parametrize("dtype,trend", VE.C_ROW_CASES)
def test_patches_of_five_six_and_seven_block_rows(dtype, trend):
    th, oth = FAMILIES["spline34"]
    Xs, xq, region = VE.c_row_inputs(dtype)
    model = _model(Xs, [_targets(X, 2) for X in Xs], th, dtype, trend)
    assert np.all(model.info() == 0)
    GV = _run_items(model, xq, region, th).item_vgrads()
    GV0 = None
    if trend:
        _clear_trend(model)
        GV0 = _run_items(model, xq, region, th).item_vgrads()
    refs = {r: VE.patch_ref(("Crow", dtype, r), oth, Xs[r], SIGMA2[dtype], trend) for r in sorted(set(int(x) for x in region))}
    worst, kappa, worst_trend = item_ratios(GV, xq, region, refs, dtype, GV0)
    _record(group="C", test="block_rows", dtype=dtype, trend=trend, ratio=worst, trend_ratio=worst_trend, kappa=kappa)
    assert kappa <= VR.KAPPA_MAX and worst <= RATIO_MAX and worst_trend <= TREND_RATIO_MAX, (kappa, worst, worst_trend)


# ------------------------------------------------------------------------------------------ D. the blend at its edges
class VDev(GE.Dev):
    """test_gpu_grad_edges.Dev with the variance and its gradient: items_multi(…, True), items_grad, items_vgrad, mix_multi,
    mix_grad, mix_vgrad"""

    def items(self, q, variance=True):
        super().items(q, True)
        q.items_vgrad(None if self.own else self.wl.th)

    def run(self, wth, Xq=None, radius=None):
        q = super().run(wth, Xq, radius, True)
        q.mix_vgrad(wth)
        return q


_VDEVS = {}


def _vdev(name, **kw):
    key = (name, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _VDEVS:
        _VDEVS[key] = VDev(EC.workload(name), **kw)
    return _VDEVS[key]


def vfd_on_stable_queries(dev, wth, pred):
    """the central-difference rule of tests/test_gpu_vgrad.py on 16 stencil-stable queries of the workload, at least 4 of
    which satisfy pred -> (worst err / tol, how many do); unasserted, so that the caller records the ratio first"""
    wl = dev.wl
    pick, n_pred = wl.stable_pick(pred)
    assert len(pick) == 16 and n_pred >= 4
    Xc = wl.Xq[pick]
    h = wl.width * 2.0 ** -17
    dV = dev.run(wth, Xc).fetch_vgrad()
    b = SimpleNamespace(model=dev.model, wth=wth, radius=wl.radius, delta=wl.delta, R=dev.R)
    Vfd = _predict_var(b, np.vstack([p for x in Xc for p in wl.stencil(x, h)])).reshape(len(Xc), wl.D, 4)
    worst = 0.0
    for k, x in enumerate(Xc):
        home, reg = wl.signature(x)[:2]
        eps_f = 0.0
        for r in list(reg) + [home]:
            ref = VE.patch_ref(("fd", wl.name, dev.oths[r].family, dev.sigma2s[r], r), dev.oths[r], wl.Xs[r], dev.sigma2s[r], wl.trend)
            eps_f = max(eps_f, (len(wl.Xs[r]) + 32) * 2.0 ** -53 * float(ref.items(x[None, :])["vunit"][0]))
        for d in range(wl.D):
            fp, fm, fp2, fm2 = Vfd[k, d]
            fd_h, fd_2h = (fp - fm) / (2 * h), (fp2 - fm2) / (4 * h)
            worst = max(worst, abs(fd_h - dV[k, d]) / (abs(fd_2h - fd_h) + 2 * eps_f / h))
    return worst, n_pred


def _sigma2s(dev, sigma2s=None):
    dev.sigma2s = list(sigma2s) if sigma2s is not None else [SIGMA2[dev.dtype]] * len(dev.wl.Xs)
    return dev


@pytest.mark.parametrize("name,wname", [("base2", w) for w in EC.weight_kernels(1.0)] + [("base3", "modsqexp")])
def test_every_family_as_the_blending_profile(name, wname):
    wl, dev = EC.workload(name), _sigma2s(_vdev(name))
    wth, owth = EC.weight_kernels(wl.radius)[wname]
    q = dev.run(wth)
    ratio, m, n_nb = vblend_ratio(q, wl.hp_v, owth)
    assert n_nb >= 40
    fd, with_nb = vfd_on_stable_queries(dev, wth, EC.has_neighbours)
    _record(group="D", test="weight_family", D=wl.D, weight=wname, ratio=ratio, fd_ratio=fd, neighbour_items=n_nb,
            fd_with_neighbours=with_nb)
    assert ratio <= 1.0 and fd <= 1.0, (ratio, fd)


def test_failed_patch_gives_nan_even_at_weight_zero_and_the_rest_keep_their_bits():
    """the test of that name in tests/test_gpu_grad_edges.py for dVq: an item of the failed patch makes its query NaN in
    the gradient of the variance as in the variance, also where its weight is exactly 0"""
    r = EC.A_RADIUS[2]
    wth, owth = EC.weight_kernels(r)["spline34_narrow"]
    sound, broken = Blend(2, 3, "spline34", "constant", radius=r), Blend(2, 3, "spline34", "constant", diag_patch=2, radius=r)
    assert broken.model.info()[2] != 0 and np.all(np.delete(broken.model.info(), 2) == 0)
    sound.wth = broken.wth = wth
    qs, qb = _staged(sound), _staged(broken)
    Gs, Gb = qs.item_vgrads(), qb.item_vgrads()
    plane = qb.item_grads()[1]
    dbg = qb.debug()
    reg, off, t = dbg["item_region"], dbg["item_offsets"], dbg["item_t"]
    bad_item = reg == 2
    assert bad_item.any() and not bad_item.all()
    assert np.all(np.isnan(Gb[bad_item])) and same_bits(Gb[~bad_item], Gs[~bad_item])
    w = np.where(plane >= 0, VR.GR.phi(owth, np.abs(t)), 1.0)
    nq = len(sound.Xq)
    bad_q = np.array([bad_item[off[j]:off[j + 1]].any() for j in range(nq)])
    weightless = np.array([np.all(w[off[j]:off[j + 1]][bad_item[off[j]:off[j + 1]]] == 0.0) for j in range(nq)])
    assert np.any(bad_q & weightless)                               # a query whose only failed items have weight 0
    dVs, dVb = qs.fetch_vgrad(), qb.fetch_vgrad()
    assert bad_q.any() and not bad_q.all()
    assert np.all(np.isnan(dVb[bad_q])) and same_bits(dVb[~bad_q], dVs[~bad_q])
    assert np.array_equal(np.isnan(qb.fetch_multi(3)[1]), bad_q) and np.all(np.isfinite(dVs))


@pytest.mark.parametrize("which", list(EC.C_RADII))
def test_more_neighbours_than_the_stage_holds(which):
    wl, dev = EC.workload("many"), _vdev("many")
    radius = EC.C_RADII[which]
    wth, owth = EC.spline34_weight(radius)
    q = dev.run(wth, radius=radius)
    cnt = np.diff(q.debug()["item_offsets"]) - 1
    assert cnt.max() > EC.PLAN_STAGE
    ratio, m, n_nb = vblend_ratio(q, wl.hp_v, owth)
    _record(group="D", test="many_items", radius=radius, ratio=ratio, largest_m=m, neighbour_items=n_nb)
    assert m == cnt.max() + 1 and ratio <= 1.0, (m, ratio)


def test_twelve_and_more_items_per_query():
    wl, dev = EC.workload("polygon"), _vdev("polygon")
    wth, owth = EC.spline34_weight(wl.radius)
    q = dev.run(wth)
    assert np.diff(q.debug()["item_offsets"]).min() >= 12
    ratio, m, n_nb = vblend_ratio(q, wl.hp_v, owth)
    _record(group="D", test="twelve_items", ratio=ratio, largest_m=m, neighbour_items=n_nb)
    assert m >= 12 and ratio <= 1.0, (m, ratio)


def test_the_deep_tree():
    wl, dev = EC.workload("L10"), _vdev("L10")
    wth, owth = EC.spline34_weight(wl.radius)
    q = dev.run(wth)
    plane, _ = GE.check_planes(wl, q, wl.Xq, wl.plan())
    ratio, m, n_nb = vblend_ratio(q, wl.hp_v, owth)
    _record(group="D", test="deep_tree", planes=int(wl.P - 1), max_plane=int(plane.max()), ratio=ratio, neighbour_items=n_nb)
    assert plane.max() >= 256 and n_nb >= 40 and ratio <= 1.0, (plane.max(), n_nb, ratio)


def test_the_staged_copy_and_the_second_walk_give_the_same_bits():
    wl, dev = EC.workload("many"), _vdev("many")
    wth, _ = EC.spline34_weight(wl.radius)
    a, b, heavy, light = EC.reorderings(wl)
    out = []
    for order in (a, b):
        q = dev.run(wth, wl.Xq[order])
        off = q.debug()["item_offsets"]
        out.append((off, np.diff(off) - 1, q.item_vgrads(), q.item_values_multi()[1], q.fetch_vgrad()))
    assert out[0][1][:256].max() > EC.PLAN_STAGE and out[1][1][:256].max() <= EC.PLAN_STAGE
    where_b = np.argsort(b)                                          # position of query j in order B
    (offa, _, Ga, va, dVa), (offb, _, Gb, vb, dVb) = out
    for pa, j in enumerate(a):
        pb = where_b[j]
        sa, sb = slice(offa[pa], offa[pa + 1]), slice(offb[pb], offb[pb + 1])
        assert same_bits(Ga[sa], Gb[sb]) and same_bits(va[sa], vb[sb]) and same_bits(dVa[pa], dVb[pb]), j
    _record(group="D", test="staged_vs_walk", queries=len(a), heavy=len(heavy))


def test_query_on_a_plane():
    wl, dev = EC.workload("on_plane"), _vdev("on_plane")
    wth, owth = EC.spline34_weight(wl.radius)
    q = dev.run(wth)
    dbg = q.debug()
    off, t = dbg["item_offsets"], dbg["item_t"]
    assert off[1] == 2 and t[0] == 0.0 and t[1] == 0.0
    GV, dV = q.item_vgrads(), q.fetch_vgrad()
    assert np.all(np.isfinite(GV[:2])) and np.all(GV[:2] != 0) and not np.array_equal(GV[0], GV[1])
    # w(0) = 1 and c = 0: both weights are 1/2, dwn = 0, and dVq is a quarter of each item's gradient, for bits
    assert np.all(np.isfinite(dV)) and same_bits(dV[0], 0.25 * GV[0] + 0.25 * GV[1])
    ratio, _, _ = vblend_ratio(q, wl.hp_v, owth)
    wth, owth = EC.weight_kernels(wl.radius)["trq"]                  # w(0) = 0.7 against the home weight 1
    ratio_trq, _, _ = vblend_ratio(dev.run(wth), wl.hp_v, owth)
    _record(group="D", test="on_plane", ratio=ratio, ratio_trq=ratio_trq)
    assert ratio <= 1.0 and ratio_trq <= 1.0


@pytest.mark.parametrize("name", ["grid", "dups"])
def test_training_points_as_queries(name):
    wl, dev = EC.workload(name), _vdev(name)
    assert wl.trend == "linear"
    wth, owth = EC.spline34_weight(wl.radius)
    q = dev.run(wth)
    plane, dbg = GE.check_planes(wl, q, wl.Xq, wl.plan())
    assert np.all(np.isfinite(q.item_vgrads())) and np.all(np.isfinite(q.fetch_vgrad()))
    exact = int(np.sum((plane >= 0) & (np.abs(dbg["item_t"]) < 1e-12)))
    lat = {} if name == "grid" else None
    ratio, m, n_nb = vblend_ratio(q, wl.hp_v, owth, lat)
    _record(group="D", test="training_points", case=name, ratio=ratio, neighbour_items=n_nb, items_on_a_plane=exact, **(lat or {}))
    assert exact >= 10 and ratio <= 1.0, (exact, ratio)


@pytest.mark.parametrize("radius", [0.0] + EC.HUGE_RADII)
def test_plan_radius_zero_and_huge(radius):
    wl, dev = EC.workload("base2"), _vdev("base2")
    wth, owth = EC.weight_kernels(0.8)["gaussian"]
    q = dev.run(wth, radius=radius)
    if radius == 0.0:
        assert q.total == q.Nq
        assert same_bits(q.fetch_vgrad(), q.item_vgrads())           # the home item's gradient, for bits
        return
    ratio, m, n_nb = vblend_ratio(q, wl.hp_v, owth)
    _record(group="D", test="huge_radius", radius=radius, ratio=ratio, neighbour_items=n_nb)
    assert n_nb >= 300 and ratio <= 1.0, (n_nb, ratio)


def _range_query(nq):
    wl, dev = EC.workload("base2"), _vdev("base2")
    q = M.DeviceQuery(dev.model, wl.queries(nq))
    q.plan(wl.radius, wl.delta)
    dev.items(q)
    wa, wb = EC.spline34_weight(wl.radius)[0], EC.weight_kernels(wl.radius)["gaussian"][0]
    q.mix_multi(wa)
    return q, wa, wb


@pytest.mark.parametrize("nq", EC.E_NQ)
def test_ranges_that_tile_the_queries_equal_the_full_range(nq):
    q, wa, wb = _range_query(nq)
    q.mix_vgrad(wa)
    A = q.fetch_vgrad()
    q.mix_vgrad(wb)
    B = q.fetch_vgrad()
    has_nb = np.diff(q.debug()["item_offsets"]) > 1
    assert np.all(np.isfinite(A)) and (nq == 1 or not np.array_equal(A[has_nb], B[has_nb]))
    for q0, q1 in EC.range_chain(nq):                                # over the rows of B: every row is written again
        q.mix_vgrad(wa, q0, q1)
    assert same_bits(q.fetch_vgrad(), A)
    for at in sorted({0, nq // 2, nq}):                              # q0 == q1 is accepted and changes nothing
        q.mix_vgrad(wb, at, at)
    assert same_bits(q.fetch_vgrad(), A)
    L, d = pmk.lib(), wa.desc()
    for q0, q1 in ((-1, nq), (0, nq + 1), (nq, nq - 1), (1, 0)):
        assert L.pmk_query_mix_vgrad(q.h, C.byref(d), q0, q1) == -3, (q0, q1)
    assert same_bits(q.fetch_vgrad(), A)
    _record(group="D", test="ranges", Nq=nq, chain=EC.range_chain(nq), with_neighbours=int(has_nb.sum()))


def test_rows_outside_a_range_keep_their_bits():
    q, wa, wb = _range_query(513)
    q.mix_vgrad(wb)
    B = q.fetch_vgrad()
    q.mix_vgrad(wa)
    A = q.fetch_vgrad()
    q.mix_vgrad(wb, 100, 300)
    got = q.fetch_vgrad()
    inside = np.zeros(513, dtype=bool)
    inside[100:300] = True
    assert same_bits(got[~inside], A[~inside]) and same_bits(got[inside], B[inside])
    has_nb = np.diff(q.debug()["item_offsets"]) > 1
    assert not np.array_equal(A[inside & has_nb], B[inside & has_nb]) and (has_nb & ~inside).sum() >= 20


def test_replans_and_a_trend_that_comes_and_goes_on_one_query():
    """d_gv and d_gh grow by capacity with the plan (items x D, items x D q); d_gh is needed under a trend, not without
    one, and again.  A query object holds its points for life, so d_dvq (Nq x D) is sized once"""
    wl = EC.workload("base2")
    wth, _ = EC.spline34_weight(wl.radius)
    L, d = pmk.lib(), wl.th.desc()
    dev = VDev(wl)

    def results(q):
        dev.items(q)
        q.mix_multi(wth)
        q.mix_grad(wth)
        q.mix_vgrad(wth)
        return q.fetch_vgrad(), q.item_vgrads(), q.fetch_multi(dev.R)[1], q.fetch_grad()

    small, large = EC.F_RADII["small"], EC.F_RADII["large"]
    q = M.DeviceQuery(dev.model, wl.Xq)
    sizes, trend_now = [], None
    for stage, (radius, trend) in enumerate([(small, None), (large, None), (large, "linear"), (small, None), (large, "linear"),
                                             (small, "constant")]):
        if trend != trend_now:
            dev.model.set_trend(trend)
            assert L.pmk_query_items_vgrad(q.h, C.byref(d)) == -3    # stale until the solve and new items
            dev.model.solve_multi()
            trend_now = trend
        q.plan(radius, wl.delta)
        got = results(q)
        fresh = M.DeviceQuery(dev.model, wl.Xq)
        fresh.plan(radius, wl.delta)
        want = results(fresh)
        assert q.total == fresh.total
        sizes.append((q.total * wl.D, q.total * wl.D * VE.trend_q(trend, wl.D)))
        for g, w, what in zip(got, want, ("fetch_vgrad", "item_vgrads", "Vq", "fetch_grad")):
            assert same_bits(g, w), (stage, what)
    gv, gh = zip(*sizes)
    assert gv[0] < gv[1] == gv[2] > gv[3] < gv[4] and gh[0] == gh[1] == 0 < gh[2] and gh[3] == 0 < gh[4] > gh[5] > 0
    _record(group="D", test="buffer_lifetime", gv_values=list(gv), gh_values=list(gh))


def test_the_order_of_the_calls_changes_no_bit():
    wl, dev = EC.workload("base2"), _vdev("base2")
    wth, _ = EC.spline34_weight(wl.radius)
    qa = dev.run(wth)                                                # items_vgrad before mix_multi and mix_grad
    qb = M.DeviceQuery(dev.model, wl.Xq)
    qb.plan(wl.radius, wl.delta)
    qb.items_multi(wl.th, True)
    qb.mix_multi(wth)
    qb.items_grad(wl.th)
    qb.mix_grad(wth)
    qb.items_vgrad(wl.th)                                            # and after them
    qb.mix_vgrad(wth)
    assert same_bits(qa.item_vgrads(), qb.item_vgrads()) and same_bits(qa.fetch_vgrad(), qb.fetch_vgrad())
    assert same_bits(qa.fetch_multi(dev.R)[1], qb.fetch_multi(dev.R)[1]) and same_bits(qa.fetch_grad(), qb.fetch_grad())


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_planned_blend_over_mixed_families_and_noise_per_patch(dtype):
    name = "base2" if dtype == "f64" else "base2_f32"
    wl = EC.workload(name)
    dev = _sigma2s(_vdev(name, thetas=EC.MIXED_NAMES, sigma2s=EC.MIXED_SIGMA2[dtype]), EC.MIXED_SIGMA2[dtype])
    wth, owth = EC.spline34_weight(wl.radius)
    q = dev.run(wth)
    _, dbg = GE.check_planes(wl, q, wl.Xq, wl.plan())
    item_q = np.repeat(np.arange(q.Nq), np.diff(dbg["item_offsets"]))
    xq, region = _round(wl.Xq, dtype)[item_q], dbg["item_region"].astype(np.int32)
    want_x, want_r = VE.plan_items(wl, dtype)
    assert np.array_equal(xq, want_x) and np.array_equal(region, want_r)      # the items the CPU file checked
    refs = {r: VE.patch_ref(("Dmixed", dtype, r), dev.oths[r], wl.Xs[r], dev.sigma2s[r]) for r in range(len(wl.Xs))}
    items, kappa, _ = item_ratios(q.item_vgrads(), xq, region, refs, dtype)
    ratio, m, n_nb = vblend_ratio(q, wl.hp_v, owth)
    rec = dict(group="D", test="mixed_families", dtype=dtype, item_ratio=items, kappa=kappa, ratio=ratio, neighbour_items=n_nb)
    fd = 0.0
    if dtype == "f64":
        fd, with_nb = vfd_on_stable_queries(dev, wth, EC.has_neighbours)
        rec.update(fd_ratio=fd, fd_with_neighbours=with_nb)
    _record(**rec)
    assert n_nb >= 40 and kappa <= VR.KAPPA_MAX and items <= RATIO_MAX and ratio <= 1.0 and fd <= 1.0, rec

"""The inputs of tests/test_gpu_vgrad_edges.py, checked on the CPU (no device compute): every input of
tests/_vgrad_edge_cases.py has the property its GPU test relies on, so that a failure of the GPU module is a property of the
device code and not of its inputs.

  A. the schedule: for chips of 64, 256 and 304 compute units the item counts give 2 ncu + 3 strips, a workgroup with three
     tasks, consecutive tasks from a patch of more block rows to one of fewer and the other way, and a full strip behind a
     strip of one item in the same workgroup; the cuts of the bits check leave every part at most ncu strips;
  B. the clamp: on the separated patch k(x,x) - b lies below min_v / 10 where the item is meant to be clamped and above
     10 min_v where it is not, kappa2(L) = 1, and in fp32 the diagonal 1 + sigma2 rounds to 1;
  C. the counts of the chunk batches, the trend's column ranges, the block rows of the large patches;
  and for every per-item accuracy input of A, B, C and of the planned blend over mixed families (group D): a numpy / LAPACK
  evaluation of the item formula in the model's own precision stays below one error unit e_d of tests/_vgrad_refs.py, its
  trend part below one unit of its own, and kappa2(L) <= 10^3 -- the check of tests/test_vgrad_refs.py on the new inputs.
"""
import numpy as np
import pytest

import _grad_edge_cases as EC
import _vgrad_edge_cases as VE
import _vgrad_refs as VR
from test_gpu_grad import FAMILIES, _round
from test_vgrad_refs import U53, _plain_item_grads


def plain_ratios(ref, oth, X, sigma2, xq, trend, dtype, free=None):
    """worst err / unit of the plain evaluation against the reference over the items `free` (default: all; a clamped item
    has no simple-kriging gradient to compare), and of the trend's part over its own unit on all items"""
    T_, u = (np.float32, 2.0 ** -24) if dtype == "f32" else (np.float64, U53)
    n = len(X)
    free = np.ones(len(xq), dtype=bool) if free is None else free
    out = ref.items(xq)
    plain = _plain_item_grads(oth, X, sigma2, xq, trend, T_)
    err = np.abs(plain - out["grad"]).astype(np.float64)[free]
    unit = (n + 32) * u * out["unit"][free]
    assert np.all(err[unit == 0] == 0)
    worst = float((err[unit > 0] / unit[unit > 0]).max()) if np.any(unit > 0) else 0.0
    worst_trend = 0.0
    if trend:
        part = plain - _plain_item_grads(oth, X, sigma2, xq, None, T_)
        err = np.maximum(np.abs(part - out["trend"]).astype(np.float64) - 4 * U53 * np.abs(plain), 0.0)
        tunit = (n + 32) * u * out["tunit"]
        assert np.all(err[tunit == 0] == 0)
        worst_trend = float((err[tunit > 0] / tunit[tunit > 0]).max())
    return worst, worst_trend


def check_regions(key, oth, Xs, sigma2, xq, region, trend, dtype):
    """the one-unit and kappa2 conditions on the items (xq, region) -> (worst, worst of the trend's part)"""
    worst = worst_trend = 0.0
    for r in sorted(set(int(x) for x in region)):
        if len(Xs[r]) < VE.trend_q(trend, Xs[r].shape[1]):
            continue                                                 # flagged on the device: NaN, nothing to compare
        ref = VE.patch_ref(key + (r,), oth, Xs[r], sigma2, trend)
        assert ref.kappa()[0] <= VR.KAPPA_MAX, (key, r, ref.kappa())
        w, wt = plain_ratios(ref, oth, Xs[r], sigma2, xq[region == r], trend, dtype)
        worst, worst_trend = max(worst, w), max(worst_trend, wt)
    print("VGRADEDGEUNIT %s trend=%s plain worst err/unit=%.3g trend part=%.3g" % (key, trend, worst, worst_trend))
    assert worst < 1.0 and worst_trend < 1.0, (key, worst, worst_trend)
    return worst, worst_trend


# ------------------------------------------------------------------------------------ A. more strips than workgroups
def test_the_patches_of_the_schedule_have_the_block_rows_it_needs():
    assert [VE.block_rows(n) for n in VE.A_SIZES] == [6, 1, 3, 1, 3, 2, 1, 1]
    assert [VE.strip_cap(D) for D in (1, 2, 3, 4)] == [128, 80, 64, 48]


@pytest.mark.parametrize("ncu", VE.A_NCU)
@pytest.mark.parametrize("D", sorted({c[0] for c in VE.A_CASES}))
def test_some_workgroup_runs_three_strips_of_every_kind(D, ncu):
    counts = VE.a_counts(ncu, D)
    cap = VE.strip_cap(D)
    s = VE.schedule(counts, VE.A_SIZES, D, ncu)
    assert s["strips"] == 2 * ncu + 3 and s["grid"] == ncu
    assert s["most_tasks"] == 3
    assert s["nt_down"] >= 1 and s["nt_up"] >= 1 and s["full_after_one"] >= 1, s
    assert sorted(r for r, c in enumerate(counts) if c % cap == 1) == sorted(VE.A_ONE_ITEM_ENDS)
    assert all(c >= 3 for c in counts)                               # a first, a middle and a last item in every region
    pieces = VE.a_pieces(counts, D, ncu)                             # asserts <= ncu strips a piece
    assert pieces[0][0] == 0 and pieces[-1][1] == sum(counts) and all(a[1] == b[0] for a, b in zip(pieces[:-1], pieces[1:]))
    assert all(lo % cap for lo, _ in pieces[1:])
    # without the second pass: the largest list of tests/test_gpu_vgrad.py stays below the smallest chip here
    assert VE.schedule([257] * 8, VE.A_SIZES, 4, 64)["most_tasks"] == 1


@pytest.mark.parametrize("D,dtype,trend", VE.A_CASES)
def test_a_plain_evaluation_stays_below_one_unit_on_the_schedule_inputs(D, dtype, trend):
    oth = FAMILIES["spline34"][1]
    Xs = VE.a_patches(D, dtype)
    for ncu in VE.A_NCU:
        counts = VE.a_counts(ncu, D)
        xq, region = VE.items_of(VE.A_SEED + D, Xs, counts, dtype)
        pick = VE.ends_and_middle(counts)
        assert len(pick) == 24
        check_regions(("A", D, dtype), oth, Xs, VR.SIGMA2[dtype], xq[pick], region[pick], trend, dtype)


# ------------------------------------------------------------------------------------ B. the clamp
@pytest.mark.parametrize("family,dtype", VE.B_FAMILIES)
def test_the_clamp_decisions_and_their_margin(family, dtype):
    oth = FAMILIES[family][1]
    Xs, xq, region, kind = VE.b_inputs(family, dtype)
    Z = Xs[VE.B_PATCH]
    support = 1.0 / oth.p[0]
    assert len(Z) == 130 and VE.block_rows(130) == 2 and (130 - 128 + 31) >> 5 == 1
    d = np.sqrt(((Z[:, None, :] - Z[None, :, :]) ** 2).sum(2))
    assert d[d > 0].min() == 3.0 * support
    assert np.array_equal(Z, _round(Z, "f32")) and np.array_equal(Z[65], np.zeros(2))
    if dtype == "f32":
        assert np.float32(1.0) + np.float32(VE.B_SIGMA2["f32"]) == np.float32(1.0)      # the device factors K itself
    ref = VE.patch_ref(("B", family, dtype), oth, Z, VE.B_REF_SIGMA2[dtype])
    kl = ref.kappa()[0]
    assert abs(kl - 1.0) <= 1e-12
    xs = xq[region == VE.B_PATCH]
    assert len(xs) == len(kind) and {VE.CLAMPED, VE.INSIDE, VE.OUTSIDE} == set(kind)
    out = ref.items(xs, VE.MIN_V)
    assert np.array_equal(out["clamped"], kind == VE.CLAMPED)
    var = np.asarray(ref.items(xs, -1.0)["v"], dtype=np.float64)     # nothing clamped: k(x,x) - b itself
    assert np.all((var < VE.MIN_V / 10) | (var > 10 * VE.MIN_V)), var
    assert np.all(var[kind == VE.OUTSIDE] == float(ref.kself)) and np.all(np.asarray(out["grad"], dtype=np.float64)[kind == VE.OUTSIDE] == 0)
    assert np.all(np.asarray(out["grad"], dtype=np.float64)[kind == VE.CLAMPED] == 0)
    assert np.all(np.abs(np.asarray(out["grad"], dtype=np.float64)[kind == VE.INSIDE]).max(1) > 1e-4)
    # clamped queries in the first and in the last block row, on a point and off it
    on = np.array([np.any(np.all(Z == x, axis=1)) for x in xs])
    rows = np.array([np.argmin(((Z - x) ** 2).sum(1)) // VE.TILE for x in xs])
    for where in (0, 1):
        assert np.any((kind == VE.CLAMPED) & on & (rows == where))
    assert np.any((kind == VE.CLAMPED) & ~on)
    # every sum b has one term: the decision cannot depend on the order of summation
    kq, _ = ref.operands(xs)
    assert np.all((np.asarray(kq) != 0).sum(0) <= 1)
    for trend in (None, "constant", "linear"):
        tr = VE.patch_ref(("B", family, dtype), oth, Z, VE.B_REF_SIGMA2[dtype], trend)
        if trend == "linear" and dtype == "f64" and family == "spline34":
            assert 10 < tr.kappa()[1] < 100                          # kappa2(L_G) of the centred lattice's linear trend: 34
        if trend and dtype == "f64":
            held = tr.items(xs, VE.MIN_V)
            assert np.array_equal(held["clamped"], kind == VE.CLAMPED)
            assert np.array_equal(held["grad"][kind == VE.CLAMPED], held["trend"][kind == VE.CLAMPED])
        w, wt = plain_ratios(tr, oth, Z, VE.B_SIGMA2[dtype], xs, trend, dtype, free=kind != VE.CLAMPED)
        print("VGRADEDGEUNIT B %s %s trend=%s plain worst err/unit=%.3g trend part=%.3g" % (family, dtype, trend, w, wt))
        assert w < 1.0 and wt < 1.0, (trend, w, wt)
    # and the ordinary patches of the same model
    ordinary = region != VE.B_PATCH
    check_regions(("B", "ordinary", family, dtype), oth, Xs, VR.SIGMA2[dtype], xq[ordinary], region[ordinary], None, dtype)


def test_the_blend_of_the_clamp_has_a_model_kernel_narrower_than_the_lattice():
    wl = EC.workload("grid")
    d = np.sqrt(((wl.X[:, None, :] - wl.X[None, :, :]) ** 2).sum(2))
    assert d[d > 0].min() == 0.25 and 1.0 / VE.B_BLEND_THETA < 0.25
    cnt = wl.counts()
    assert cnt.sum() >= 40 and len(wl.Xq) == 512
    # a training point in the eps-set of every patch of its items is clamped in all of them
    member = lambda r, x: bool(np.any(np.all(wl.Xs[r] == x, axis=1)))
    full = [j for j, s in enumerate(wl.plan()) if len(s[1]) and all(member(r, wl.Xq[j]) for r in list(s[1]) + [s[0]])]
    assert len(full) >= 10


def test_the_lattice_has_a_few_queries_whose_weight_slopes_cancel():
    """Two parallel planes at t and -t give a lattice point slopes dw that cancel in sum_j dw_j to the last bits.  The bound
    of the blend is stated in the magnitudes after that cancellation and no evaluation in double meets it there
    (_vgrad_edge_cases.plain_mix_vgrad): the GPU tests on this workload leave out the queries on which a plain float64
    evaluation itself exceeds the bound.  Here: such queries exist and are a few of the workload"""
    wl = EC.workload("grid")
    _, owth = EC.spline34_weight(wl.radius)
    cancelling = 0
    for s in wl.plan():
        planes, ts = list(s[2]), np.asarray(s[3], dtype=np.float64)
        if len(ts) < 2:
            continue
        dw = -(VR.GR.psi(owth, np.abs(ts)) * ts)[:, None] * wl.hp_v[planes]
        cancelling += int(np.any(np.abs(dw.sum(0)) < 1e-10 * np.abs(dw).sum(0)))
    assert 1 <= cancelling <= len(wl.Xq) // 50, cancelling


# ------------------------------------------------------------------------------------ C. columns, chunks, block rows
def test_the_trend_columns_sit_at_both_ends_of_the_block():
    seen = set()
    for D, dtype, trend, R in VE.C_COLUMN_CASES:
        q = VE.trend_q(trend, D)
        assert R in (1, 16 - q) and R + q <= 16
        seen.add((D, dtype, trend, R == 1))
    assert {(D, dt, tr) for D, dt, tr, _ in seen} == {(D, dt, tr) for D in (2, 4) for dt in ("f64", "f32") for tr in ("constant", "linear")}
    assert {(D, tr, lo) for D, _, tr, lo in seen} >= {(D, "linear", lo) for D in (2, 4) for lo in (True, False)}
    assert {(tr, lo) for _, _, tr, lo in seen} >= {("constant", True), ("constant", False)}


@pytest.mark.parametrize("D,dtype,trend", sorted({c[:3] for c in VE.C_COLUMN_CASES}))
def test_a_plain_evaluation_stays_below_one_unit_on_the_column_inputs(D, dtype, trend):
    Xs, xq, region = VE.c_column_inputs(D, dtype)
    check_regions(("Ccol", D, dtype), FAMILIES["spline34"][1], Xs, VR.SIGMA2[dtype], xq, region, trend, dtype)


def test_the_chunk_batches():
    flat = [c for b in VE.C_CHUNK_BATCHES for c in b]
    assert all(flat.count(c) == 1 for c in VE.C_EDGE_COUNTS) and all(len(b) == 8 for b in VE.C_CHUNK_BATCHES)
    for b in VE.C_CHUNK_BATCHES:
        n = VE.chunk_count(b)
        assert n > 32 and n % 8 != 0 and n % 4 != 0, (b, n)          # more than eight workgroups, the last one ragged
    assert VE.chunk_count([5, 3, 17, 4, 6, 9, 0, 2]) == 8            # what the first suite deals: two workgroups


@pytest.mark.parametrize("D,dtype", VE.C_CHUNK_CASES)
def test_a_plain_evaluation_stays_below_one_unit_on_the_chunk_inputs(D, dtype):
    Xs = VE.c_chunk_patches(D, dtype)
    for k, batch in enumerate(VE.C_CHUNK_BATCHES):
        xq, region = VE.items_of(1500 + 10 * D + k, Xs, batch, dtype)
        pick = VE.ends_and_middle(batch)
        check_regions(("Cchunk", D, dtype), FAMILIES["spline34"][1], Xs, VR.SIGMA2[dtype], xq[pick], region[pick], "linear", dtype)


@pytest.mark.parametrize("dtype,trend", VE.C_ROW_CASES)
def test_a_plain_evaluation_stays_below_one_unit_on_the_block_row_inputs(dtype, trend):
    Xs, xq, region = VE.c_row_inputs(dtype)
    big = [n for n, c in zip(VE.C_ROW_SIZES, VE.C_ROW_COUNTS) if c and n > 500]
    assert [VE.block_rows(n) for n in big] == [5, 6, 7]
    assert [(n - (VE.block_rows(n) - 1) * VE.TILE + 31) >> 5 for n in big] == [1, 1, 4]
    check_regions(("Crow", dtype), FAMILIES["spline34"][1], Xs, VR.SIGMA2[dtype], xq, region, trend, dtype)


# ------------------------------------------------------------------------------------ D. the planned blend over mixed families
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_a_plain_evaluation_stays_below_one_unit_on_the_mixed_family_blend(dtype):
    wl = EC.workload("base2" if dtype == "f64" else "base2_f32")
    xq, region = VE.plan_items(wl, dtype)
    assert len(xq) - len(wl.Xq) >= 40                                # neighbour items
    for r, (name, s2) in enumerate(zip(EC.MIXED_NAMES, EC.MIXED_SIGMA2[dtype])):
        sel = region == r
        assert sel.any()
        ref = VE.patch_ref(("Dmixed", dtype, r), FAMILIES[name][1], wl.Xs[r], s2)
        assert ref.kappa()[0] <= VR.KAPPA_MAX, (r, name, ref.kappa())
        w, _ = plain_ratios(ref, FAMILIES[name][1], wl.Xs[r], s2, xq[sel], None, dtype)
        print("VGRADEDGEUNIT D mixed %s patch %d %s plain worst err/unit=%.3g" % (dtype, r, name, w))
        assert w < 1.0, (r, name, w)

"""Blended leave-one-out on the GPU at its edges: pmk_query_items_loo and pmk_query_items_loo_multi at D = 1, 3 and 4, on
patches of 1, 2, q, q + 1 points, at item counts around one block of 256, across a growth of the leave-one-out arena, with
query-side diagonal addends, with homeless and with duplicated points.  The workloads are those of
tests/_loo_blend_edge_cases.py; tests/test_loo_blend_edges_refs.py asserts on the CPU what they were chosen for.

Reference of the accuracy tests: BRUTE FORCE, every patch that holds point j fitted again without it (tests/_loo_blend_refs.py,
tests/_loo_blend_multi_refs.py: the oracle without a trend, long double with one).  Bounds:
  * dimensions, item counts, duplicates, the mixed tree: those of tests/test_gpu_loo_blend.py, |dY| <= cond_2 u max|Y| and
    |dV| <= cond_2 u (k(0) + sigma2), u = 2^-53 for fp64 models and 2^-24 for fp32 models: both ratios <= 1;
  * small patches (1, 2, 4 points without a trend; n = q + 1 with one): cond_2 u does not describe them (cond_2 = 1 on a
    one-point patch, and at n = q + 1 the division by a small Q_ii amplifies), so the rule of tests/test_gpu_trend.py: the
    device may be at 10 x max(1, what the fp64 closed form on the CPU achieves on the same inputs in the same unit); the
    margin is for summation order.
n <= q with a trend: no leave-one-out prediction exists from fewer points than basis functions; the library answers NaN.
Item counts, patch sizes and index lists are compared with the oracle's, never written down.  Bit claims are fp64 only and
have no tolerance; they reuse the helpers of tests/test_gpu_loo_blend.py and tests/test_gpu_loo_blend_multi.py.

Every measured ratio is printed before it is asserted ("measured {json}"); with PMK_WRITE_PROFILES=1 in the environment a
run of the whole module writes them to profiles/loo_blend_edges.json.  The committed file is one such run on an MI355X:
  * dimensions, fp64: D = 1 and D = 3 at most 0.014 of the bound of the means and 0.028 of that of the variances; D = 4,
    where cond_2 is only 42, 0.18 and 0.31 (the closed form on the CPU: 0.20 and 0.28); fp32 at most 0.13 and 0.21;
  * item counts, duplicates, the mixed tree: at most 0.046 and 0.0098;
  * small patches without a trend: 1.05 and 1.00 on the one-point patches, exactly the CPU's figures; at most 0.12 and 0.11
    on two and four points (CPU 0.073 and 0.062);
  * n = q + 1: D = 2 linear 51.8 and 2030 in the blend (CPU 15.3 and 510, so the bounds are 153 and 5100) and 715 / 387 in
    the per-patch values (CPU 963 / 247); D = 1 linear 0.35 and 3.7 (CPU 0.36 and 2.1); D = 2 constant 0.24 and 0.25.
"""
import json
import os

import numpy as np
import pytest

import patchmixturekriging_amd as pmk
from oracle import oracle as O

import _loo_blend_refs as BR
import _loo_blend_multi_refs as MR
import _loo_blend_edge_cases as EC
import _trend_refs as TR
import test_gpu_loo_blend as TB
import test_gpu_loo_blend_multi as TM
from test_gpu_loo_blend import same_bits

pytestmark = pytest.mark.gpu

TH = pmk.Spline34KernelType(BR.A)
SIGMA2, DELTA = BR.SIGMA2, BR.DELTA
U = {"f64": 2.0 ** -53, "f32": 2.0 ** -24}
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "loo_blend_edges.json")
_MEASURED = []


def _record(**kw):
    print("measured " + json.dumps(kw))
    _MEASURED.append(kw)


@pytest.fixture(scope="module", autouse=True)
def _write_profile():
    yield
    if os.environ.get("PMK_WRITE_PROFILES") == "1":
        with open(PROFILE, "w") as f:
            json.dump(_MEASURED, f, indent=1)
            f.write("\n")


def _wth(radius, oracle=False):
    if radius <= 0.0:               # no neighbour has a weight at radius 0: any profile serves
        radius = 1.0
    return O.kernel(O.SPLINE34, 1.0 / radius) if oracle else pmk.Spline34KernelType(1.0 / radius)


_TREES, _MODELS = {}, {}


def _tree(o):
    key = (o.X.shape, float(o.X[0, 0]), o.levels)
    if key not in _TREES:
        _TREES[key] = pmk.setuppartition(o.X, o.levels)[0]
    return _TREES[key]


def _check_lists(m, o):
    """the device's index lists are the oracle's"""
    off, inds = m.patch_index()
    assert m.P == o.P
    for r, s in enumerate(o.sets):
        assert np.array_equal(inds[off[r]:off[r + 1]], s), r


def _single(o, dtype="f64", cache=None):
    """tree model of the oracle's column 0, fitted, with the leave-one-out diagonal"""
    if cache is not None and (cache, dtype) in _MODELS:
        return _MODELS[(cache, dtype)]
    m = pmk.DeviceModel.from_tree(_tree(o), o.X, o.y, eps=o.eps, dtype=dtype)
    m.fit(TH, SIGMA2)
    assert np.all(m.info() == 0)
    m.loo()
    _check_lists(m, o)
    if cache is not None:
        _MODELS[(cache, dtype)] = m
    return m


def _multi(o, dtype="f64"):
    m = TM._build(_tree(o), o.X, o.Y, o.eps, o.trend, dtype)
    assert np.all(m.info() == 0) and np.all(m.trend_info() == 0)
    _check_lists(m, o)
    return m


def _staged(m, X, radius, noisy=False):
    q = pmk.DeviceQuery(m, X)
    total = q.plan(radius, DELTA)
    nm, ns = q.items_loo(noisy)
    q.mix(_wth(radius))
    Y, V = q.fetch()
    return q, total, nm, ns, Y, V


def _staged_multi(m, X, radius, noisy=False):
    q = pmk.DeviceQuery(m, X)
    total = q.plan(radius, DELTA)
    nm, no = q.items_loo_multi(noisy, True)
    q.mix_multi(_wth(radius))
    MU, V = q.fetch_multi(m.R)
    return q, total, nm, no, MU, V


def _counts_agree(o, radius, total, nm, ns):
    ototal, oother, multi, homeless = o.counts(radius)
    assert (total, ns) == (ototal, oother), (total, ns, ototal, oother)
    assert nm + ns == total
    return multi, homeless


def _single_case(o, radius, dtype, test, bound_from_fp64=False, **tags):
    """Y, V of every point against the refits -> the device model, its results and the bounds used"""
    m = _single(o, dtype)
    q, total, nm, ns, Y, V = _staged(m, o.X, radius)
    multi, homeless = _counts_agree(o, radius, total, nm, ns)
    w = _wth(radius, True)
    Yr, Vr = o.blend_refit(w, radius)
    cond, ymax, k0s2 = o.cond2(), np.abs(o.y).max(), o.k0() + SIGMA2
    ry, rv = BR.ratios(Y, V, Yr, Vr, cond, U[dtype], ymax, k0s2)
    by = bv = 1.0
    rec = dict(test=test, path="single", dtype=dtype, radius=radius, items=total, n_member=nm, n_strip=ns,
               points_2_neighbours=multi, homeless=homeless, cond2=cond, dY_ratio=ry, dV_ratio=rv, **tags)
    if bound_from_fp64:
        Yc, Vc = o.blend_closed(w, radius)
        cy, cv = BR.ratios(Yc, Vc, Yr, Vr, cond, U["f64"], ymax, k0s2)
        by, bv = 10.0 * max(1.0, cy), 10.0 * max(1.0, cv)
        rec.update(fp64_cpu_dY_ratio=cy, fp64_cpu_dV_ratio=cv)
    _record(bound_dY=by, bound_dV=bv, **rec)
    assert ry <= by and rv <= bv, (test, tags, ry, rv, by, bv)
    return m, q, (by * cond * U[dtype] * ymax, bv * cond * U[dtype] * k0s2), (multi, homeless)


def _multi_case(o, radius, dtype, test, bound_from_fp64=False, points=None, **tags):
    m = _multi(o, dtype)
    q, total, nm, no, MU, V = _staged_multi(m, o.X, radius)
    multi, homeless = _counts_agree(o, radius, total, nm, no)
    w = _wth(radius, True)
    pts, MUr, Vr = o.blend(w, o.items(radius, "ref", points=points))
    cond, ymax, k0s2 = o.cond2(), np.abs(o.Y).max(), o.k0() + SIGMA2
    ry, rv = MR.ratios(MU[pts], V[pts], MUr, Vr, cond, U[dtype], ymax, k0s2)
    by = bv = 1.0
    rec = dict(test=test, path="multi", dtype=dtype, trend=o.trend, R=o.R, radius=radius, items=total, n_member=nm,
               n_other=no, points=len(pts), points_2_neighbours=multi, homeless=homeless, cond2=cond, dY_ratio=ry,
               dV_ratio=rv, **tags)
    if bound_from_fp64:
        _, MUc, Vc = o.blend(w, o.items(radius, "closed64", points=points))
        cy, cv = MR.ratios(MUc, Vc, MUr, Vr, cond, U["f64"], ymax, k0s2)
        by, bv = 10.0 * max(1.0, cy), 10.0 * max(1.0, cv)
        rec.update(fp64_cpu_dY_ratio=cy, fp64_cpu_dV_ratio=cv)
    _record(bound_dY=by, bound_dV=bv, **rec)
    assert ry <= by and rv <= bv, (test, tags, ry, rv, by, bv)
    return m, q, (by * cond * U[dtype] * ymax, bv * cond * U[dtype] * k0s2), (MU, V)


# ------------------------------------------------------------------------------------ 1. dimensions
@pytest.mark.parametrize("name", list(EC.DIMS))
def test_dimensions_single_output(name):
    """D = 1, 3, 4 and a deep tree at D = 3: Y and V of every point against the refits, both ratios <= 1.  The D = 1
    workload has points whose home patch does not hold them (eps = 0 and a point on the far side of its leaf's plane by
    rounding): their home item takes the non-member route, and they are held to the bound like the rest"""
    c = EC.DIMS[name]
    o = EC.dim_oracle(name)
    _, _, _, (multi, homeless) = _single_case(o, c["radius"], "f64", "dimensions", workload=name, D=c["D"])
    assert multi >= 1 and (homeless >= 1) == c["homeless"]


@pytest.mark.parametrize("name, trend, R", EC.DIM_MULTI)
def test_dimensions_multi_output(name, trend, R):
    """the same for R columns without a trend, with the constant and the linear one; at D = 4 the linear trend has
    q = 5 = TQ_MAX basis functions, and R = 11 (linear) and R = 15 (constant) fill the 16 columns of a row"""
    c = EC.DIMS[name]
    _multi_case(EC.dim_oracle(name, trend, R), c["radius"], "f64", "dimensions", workload=name, D=c["D"])


def test_dimensions_fp32_single_output():
    c = EC.DIMS["D1"]
    _single_case(EC.dim_oracle("D1"), c["radius"], "f32", "dimensions_fp32", workload="D1", D=1)


@pytest.mark.parametrize("name, trend, R", [("D3", "linear", 3), ("D4", "linear", 11)])
def test_dimensions_fp32_multi_output(name, trend, R):
    c = EC.DIMS[name]
    _multi_case(EC.dim_oracle(name, trend, R), c["radius"], "f32", "dimensions_fp32", workload=name, D=c["D"])


# ------------------------------------------------------------------------------------ 2. bits at D = 1 and D = 4
def _check_item_bits_single(m, X, y, radius, noisy):
    """the check of tests/test_gpu_loo_blend.py's test 2 through its helpers: members are numpy on pmk_model_get_loo,
    non-members pmk_query_items_fitted (+ sigma2 with noisy, one add)"""
    q, total, nm, ns, Y, V = _staged(m, X, radius, noisy)
    dbg = q.debug()
    q2 = pmk.DeviceQuery(m, X)
    assert q2.plan(radius, DELTA) == total
    q2.items_fitted()
    dbg2 = q2.debug()
    assert np.array_equal(dbg["item_region"], dbg2["item_region"]) and np.array_equal(dbg["item_offsets"], dbg2["item_offsets"])
    member, rows, u, v = TB._expected_items(m, dbg, dbg2, y, [SIGMA2] * m.P, noisy)
    assert int(member.sum()) == nm and int((~member).sum()) == ns
    assert same_bits(dbg["item_u"][member], u[member]) and same_bits(dbg["item_v"][member], v[member])
    assert same_bits(dbg["item_u"][~member], u[~member]) and same_bits(dbg["item_v"][~member], v[~member])
    off = dbg["item_offsets"]
    alone = np.nonzero(np.diff(off) == 1)[0]
    if len(alone):          # weight 1: Yq and Vq are the item's
        assert same_bits(Y[alone], dbg["item_u"][off[alone]]) and same_bits(V[alone], dbg["item_v"][off[alone]])
    return dbg, member, nm, ns


@pytest.mark.parametrize("noisy", [False, True])
@pytest.mark.parametrize("name", ["D1", "D4"])
def test_item_bits_single_output(name, noisy):
    c = EC.DIMS[name]
    o = EC.dim_oracle(name)
    m = _single(o, cache=name)
    dbg, member, nm, ns = _check_item_bits_single(m, o.X, o.y, c["radius"], noisy)
    assert nm > 0 and ns > 0
    if c["homeless"]:       # a home item (the last of its point) that is a non-member
        last = dbg["item_offsets"][1:] - 1
        assert (~member[last]).sum() == o.counts(c["radius"])[3] >= 1


@pytest.mark.parametrize("noisy", [False, True])
@pytest.mark.parametrize("name, R", [("D1", 3), ("D4", 11)])
def test_item_bits_multi_output(name, R, noisy):
    c = EC.DIMS[name]
    o = EC.dim_oracle(name, "linear", R)
    m = _multi(o)
    nm, no = TM._check_item_bits(m, o.X, o.Y, c["radius"], noisy, [SIGMA2] * m.P)
    assert nm > 0 and no > 0


# ------------------------------------------------------------------------------------ 3. small patches, no trend
@pytest.mark.parametrize("N", EC.SMALL_PLAIN)
def test_small_patches_single_output(N):
    """patches of exactly 1, 2, 4 points; on a one-point patch the refit has no points and the member item is the prior"""
    o = EC.small_oracle(2, N, None)
    r = EC.SMALL["radius"]
    assert [len(s) for s in o.sets] == [N // 8] * 8
    m, q, (tol_y, tol_v), _ = _single_case(o, r, "f64", "small_patches", bound_from_fp64=True, n=N // 8, D=2)
    if N == 8:
        for noisy in (False, True):
            qn, _, nm, _, _, _ = _staged(m, o.X, r, noisy)
            dbg = qn.debug()
            home = dbg["item_offsets"][1:] - 1
            assert nm == N
            assert np.abs(dbg["item_u"][home]).max() <= tol_y
            assert np.abs(dbg["item_v"][home] - (o.k0() + (SIGMA2 if noisy else 0.0))).max() <= tol_v


@pytest.mark.parametrize("N", EC.SMALL_PLAIN)
def test_small_patches_multi_output(N):
    o = EC.small_oracle(2, N, None)
    r = EC.SMALL["radius"]
    m, q, (tol_y, tol_v), _ = _multi_case(o, r, "f64", "small_patches", bound_from_fp64=True, n=N // 8, D=2)
    if N == 8:
        for noisy in (False, True):
            qn, _, nm, _, _, _ = _staged_multi(m, o.X, r, noisy)
            Ug, vg = qn.item_values_multi()
            home = qn.debug()["item_offsets"][1:] - 1
            assert nm == N
            assert np.abs(Ug[home]).max() <= tol_y
            assert np.abs(vg[home] - (o.k0() + (SIGMA2 if noisy else 0.0))).max() <= tol_v


# ------------------------------------------------------------------------------------ 4. small patches with a trend
@pytest.mark.parametrize("D, N, trend", EC.SMALL_TREND)
def test_small_patches_with_a_trend_at_q_plus_one_points(D, N, trend):
    """n = q + 1: leaving one point out leaves an exactly determined trend fit, 1 / Q_ii is large.  The blend against
    refits, and pmk_model_get_loo_multi of the same model against n refits per patch (tests/_trend_refs.brute_force_loo),
    both by the rule of tests/test_gpu_trend.py with kappa_2(U) u max|reference| as the unit per patch"""
    o = EC.small_oracle(D, N, trend)
    q = EC.Q_OF[trend](D)
    assert [len(s) for s in o.sets] == [q + 1] * 8
    m, _, _, _ = _multi_case(o, EC.SMALL["radius"], "f64", "small_patches_trend", bound_from_fp64=True, n=q + 1, D=D)
    RES, VAR = m.loo_values_multi()
    worst = dict(res=(0.0, 0.0), var=(0.0, 0.0))
    failures = []
    for p, s in enumerate(o.sets):
        K, H = o.fits[p]["K"], MR.basis(o.X[s], trend)
        ev = np.linalg.eigvalsh(K + SIGMA2 * np.eye(len(s)))
        res_ld, var_ld = TR.brute_force_loo(K, SIGMA2, o.Y[s], H)
        f = TR.gls_fp64(K, SIGMA2, o.Y[s], H)
        for name, dev, f64, ref in (("res", RES[p], f["res"], res_ld), ("var", VAR[p], f["var"], var_ld)):
            unit = float(ev[-1] / ev[0]) * U["f64"] * float(np.abs(ref).max())
            d = float(np.abs(np.asarray(dev, dtype=TR.LD) - ref).max()) / unit
            c = float(np.abs(np.asarray(f64, dtype=TR.LD) - ref).max()) / unit
            if d >= worst[name][0]:
                worst[name] = (d, c)
            if not d <= 10.0 * max(1.0, c):
                failures.append((p, name, d, c))
    _record(test="small_patches_trend_values", path="loo_values_multi", D=D, n=q + 1, trend=trend,
            res_ratio=worst["res"][0], fp64_cpu_res_ratio=worst["res"][1], var_ratio=worst["var"][0],
            fp64_cpu_var_ratio=worst["var"][1])
    assert not failures, failures


# ------------------------------------------------------------------------------------ 5. n <= q: no such prediction
def _items_against_expected(m, q, X, Y, radius, total, noisy, small):
    """every member item of a patch in `small` is NaN; every other item has the bits of numpy on loo_values_multi()
    (member) or of pmk_query_items_multi_fitted (+ sigma2 with noisy) -> (member, region, Ug, vg)"""
    dbg = q.debug()
    _, fitted = TM._fitted_items(m, X, radius, total)
    member, Ue, ve = TM._expected_items(m, dbg, fitted, Y, [SIGMA2] * m.P, noisy)
    Ug, vg = q.item_values_multi()
    inside = member & np.isin(dbg["item_region"], small)
    assert inside.any()
    assert np.isnan(Ug[inside]).all() and np.isnan(vg[inside]).all()
    assert same_bits(Ug[~inside], Ue[~inside]) and same_bits(vg[~inside], ve[~inside])
    assert np.isfinite(Ug[~inside]).all() and np.isfinite(vg[~inside]).all()
    return member, dbg["item_region"], inside


@pytest.mark.parametrize("D, N, trend", EC.AT_Q)
def test_patches_of_exactly_q_points_have_no_leave_one_out_values(D, N, trend):
    """every patch has n = q points: the fit is fine (tinfo = 0, finite weights and beta) and pmk_model_get_loo_multi
    answers NaN.  Without the guard on n <= q in trend_loo_values_kernel, measured on an MI355X: D = 2, linear, n = 3 gave
    the finite "residuals" [-2.04, 0.33, -0.48] with "variances" [-4.5e15, -5.0e14, -9.0e14] (Q_ii is rounding noise
    around 0); one point under the constant trend gave -inf and +inf (Q_ii == 0.0)"""
    o = EC.small_oracle(D, N, trend)
    assert [len(s) for s in o.sets] == [EC.Q_OF[trend](D)] * 8
    m = _multi(o)
    assert all(np.isfinite(Cw).all() for Cw in m.weights_multi()) and np.isfinite(m.trend()[0]).all()
    RES, VAR = m.loo_values_multi()
    print("loo_values_multi of patch 0:", RES[0].tolist(), VAR[0].tolist())
    for p in range(m.P):
        assert np.isnan(RES[p]).all() and np.isnan(VAR[p]).all(), (p, RES[p], VAR[p])


@pytest.mark.parametrize("noisy", [False, True])
@pytest.mark.parametrize("D, N, trend", EC.AT_Q)
def test_patches_of_exactly_q_points_answer_nan_in_the_blend(D, N, trend, noisy):
    """the same models through pmk_query_items_loo_multi: every point is a member of its home patch, so Yq and Vq are
    NaN everywhere; every member item is NaN, every non-member item is the fitted predictor's, bit for bit, and finite.
    This test does not look at pmk_model_get_loo_multi's values for the members: it holds loo_member_multi_kernel's own
    guard"""
    o = EC.small_oracle(D, N, trend)
    qn, r = EC.Q_OF[trend](D), EC.SMALL["radius"]
    assert [len(s) for s in o.sets] == [qn] * 8
    m = _multi(o)
    q, total, nm, no, MU, V = _staged_multi(m, o.X, r, noisy)
    _counts_agree(o, r, total, nm, no)
    assert nm == N and no > 0
    print("Yq[:3], Vq[:3]:", MU[:3].tolist(), V[:3].tolist())
    assert np.isnan(MU).all() and np.isnan(V).all()
    member, _, inside = _items_against_expected(m, q, o.X, o.Y, r, total, noisy, np.arange(m.P))
    assert np.array_equal(inside, member) and (~member).sum() == no


def test_a_tree_with_leaves_of_q_points_among_larger_ones():
    """clustered points: some eps-lists have n = q = 3 points, the others n >= q + 2.  A point with a member item in a
    small patch is NaN; every other point is finite and meets the refit bound, also where it reaches a small patch as a
    non-member"""
    o = EC.mixed_oracle()
    qn, r = EC.Q_OF[o.trend](o.D), EC.MIXED["radius"]
    sizes = np.array([len(s) for s in o.sets])
    assert np.all((sizes == qn) | (sizes >= qn + 2)) and (sizes == qn).sum() >= 2 and (sizes >= qn + 2).sum() >= 2
    small = np.nonzero(sizes == qn)[0]
    home, regs, _ = o.plan(r)
    hit = np.array([any(o.row_of(int(p), j) >= 0 and sizes[int(p)] == qn for p in list(regs[j]) + [int(home[j])])
                    for j in range(len(o.X))])
    clean = np.nonzero(~hit)[0].tolist()
    assert any(sizes[int(p)] == qn for j in clean for p in regs[j])
    m, q, _, (MU, V) = _multi_case(o, r, "f64", "mixed_tree", points=clean, D=o.D)
    assert np.all(m.trend_info() == 0)
    assert np.isnan(MU[hit]).all() and np.isnan(V[hit]).all()
    assert np.isfinite(MU[~hit]).all() and np.isfinite(V[~hit]).all()
    RES, VAR = m.loo_values_multi()
    for p in range(m.P):
        assert np.isnan(RES[p]).all() == np.isnan(VAR[p]).all() == (p in small), p
        assert np.isnan(RES[p]).any() == (p in small)
    for noisy in (False, True):
        qn_, total, _, _, _, _ = _staged_multi(m, o.X, r, noisy)
        _items_against_expected(m, qn_, o.X, o.Y, r, total, noisy, small)


# ------------------------------------------------------------------------------------ 6. item counts around one block
def _timed_context():
    ctx = pmk.Context(0)
    ctx.enable_timers(True)
    return ctx


@pytest.mark.parametrize("N", EC.COUNT_NS)
def test_home_items_only_at_one_block_and_one_more(N):
    """total == N == 256 and 257 (one block of the per-item kernels, and one item more), no non-member at all: nothing
    runs after the scan, no inner query is created, and Y, V are numpy on pmk_model_get_loo.  At N = 257 the tree splits
    odd counts, its planes pass through the median points, and only the radius 0 has no neighbour items"""
    o = EC.count_oracle(N)
    r0 = EC.radius_with_no_neighbours(o)
    assert o.counts(r0) == (N, 0, 0, 0)
    ctx = _timed_context()
    m = pmk.DeviceModel.from_tree(_tree(o), o.X, o.y, eps=None, ctx=ctx)
    m.fit(TH, SIGMA2)
    assert np.all(m.info() == 0)
    m.loo()
    _check_lists(m, o)
    q, total, nm, ns, Y, V = _staged(m, o.X, r0)
    assert (total, nm, ns) == (N, N, 0)
    assert TM._stage_recorded(ctx, "loo_items") and not TM._stage_recorded(ctx, "items")
    res, var = m.loo_values()
    off, inds = m.patch_index()
    Ye, Ve = np.empty(N), np.empty(N)
    for p in range(m.P):
        s = inds[off[p]:off[p + 1]]
        Ye[s], Ve[s] = o.y[s] - res[p], np.maximum(var[p] - SIGMA2, 1e-12)
    assert same_bits(Y, Ye) and same_bits(V, Ve)
    # R columns under the linear trend
    om = EC.count_oracle(N, "linear")
    mm = TM._build(_tree(om), om.X, om.Y, None, "linear", ctx=ctx)
    assert np.all(mm.info() == 0) and np.all(mm.trend_info() == 0)
    qm, total, nm, no, MU, Vm = _staged_multi(mm, om.X, r0)
    assert (total, nm, no) == (N, N, 0)
    assert TM._stage_recorded(ctx, "loo_items_multi")
    for stage in ("items", "items_multi", "trend_items"):
        assert not TM._stage_recorded(ctx, stage), stage
    RES, VAR = mm.loo_values_multi()
    MUe, Vme = np.empty((N, 3)), np.empty(N)
    for p in range(mm.P):
        s = inds[off[p]:off[p + 1]]
        MUe[s], Vme[s] = om.Y[s] - RES[p], np.maximum(VAR[p] - SIGMA2, 1e-12)
    assert same_bits(MU, MUe) and same_bits(Vm, Vme)
    ctx.synchronize()


@pytest.mark.parametrize("N", EC.COUNT_NS)
def test_the_fewest_non_members(N):
    """n_strip == 1 with total == 257 on the N = 256 data set, at a radius found by bisection on the oracle's counts.  On
    the N = 257 data set no radius has exactly one non-member: its two median points lie on their planes (t == 0) and come
    together at every positive radius, so there the smallest case is n_strip == 2 with total == 259"""
    o = EC.count_oracle(N)
    r0 = EC.radius_with_no_neighbours(o)
    r1 = EC.radius_with_one_non_member(o, r0)
    if N == 256:
        assert o.counts(r1)[:2] == (257, 1)
    else:
        assert r1 is None
        r1 = 1e-9
        assert o.counts(r1)[:2] == (259, 2)
    want = o.counts(r1)[:2]
    m, q, _, _ = _single_case(o, r1, "f64", "item_counts", N=N)
    for noisy in (False, True):
        _, _, nm, ns = _check_item_bits_single(m, o.X, o.y, r1, noisy)
        assert (nm + ns, ns) == want
    om = EC.count_oracle(N, "linear")
    mm, _, _, _ = _multi_case(om, r1, "f64", "item_counts", N=N)
    for noisy in (False, True):
        q_, total, nm, no, _, _ = _staged_multi(mm, om.X, r1, noisy)
        assert (total, no) == want
        _, fitted = TM._fitted_items(mm, om.X, r1, total)
        member, Ue, ve = TM._expected_items(mm, q_.debug(), fitted, om.Y, [SIGMA2] * mm.P, noisy)
        Ug, vg = q_.item_values_multi()
        assert int((~member).sum()) == no and same_bits(Ug, Ue) and same_bits(vg, ve)


# ------------------------------------------------------------------------------------ 7. buffer growth
def _grow_radii():
    return (EC.GROW["small"], EC.GROW["large"], EC.GROW["small"])


def _assert_growth(o):
    """the second plan does not fit what the first reserved: the leave-one-out arena of the library holds
    total + total / 8 + 1024 items after its first reservation (loo_reserve) and grows only beyond that; the inner query's
    item arrays follow the number of non-members"""
    ts, ss = o.counts(EC.GROW["small"])[:2]
    tl, sl = o.counts(EC.GROW["large"])[:2]
    assert tl > ts + ts // 8 + 1024, (ts, tl)
    assert sl - ss > ts // 8 + 1024, (ss, sl)


def test_growth_single_output():
    """small -> large -> small on ONE query: the arena is freed and carved again with live state behind it, then reused.
    After each plan Y, V and the items have the bits of a fresh query at that radius"""
    o = EC.grow_oracle()
    _assert_growth(o)
    m = _single(o)
    q = pmk.DeviceQuery(m, o.X)
    for r in _grow_radii():
        fq, ftotal, fnm, fns, FY, FV = _staged(m, o.X, r)
        assert (ftotal, fns) == o.counts(r)[:2]
        total = q.plan(r, DELTA)
        nm, ns = q.items_loo()
        q.mix(_wth(r))
        Y, V = q.fetch()
        assert (total, nm, ns) == (ftotal, fnm, fns)
        assert same_bits(Y, FY) and same_bits(V, FV), r
        d, fd = q.debug(), fq.debug()
        assert np.array_equal(d["item_region"], fd["item_region"])
        assert same_bits(d["item_u"], fd["item_u"]) and same_bits(d["item_v"], fd["item_v"]), r


def test_growth_multi_output_and_a_new_row_length():
    """the same with R = 3 columns under the linear trend, where the rows of per-item means grow too; then R = 13 on the
    same model and the same query: the row length changes under buffers that have grown already"""
    o = EC.grow_oracle("linear")
    _assert_growth(o)
    m = _multi(o)
    q = pmk.DeviceQuery(m, o.X)

    def rounds():
        for r in _grow_radii():
            fq, ftotal, fnm, fno, FMU, FV = _staged_multi(m, o.X, r)
            assert (ftotal, fno) == o.counts(r)[:2]
            total = q.plan(r, DELTA)
            nm, no = q.items_loo_multi()
            q.mix_multi(_wth(r))
            MU, V = q.fetch_multi(m.R)
            assert (total, nm, no) == (ftotal, fnm, fno)
            assert MU.shape == (len(o.X), m.R)
            assert same_bits(MU, FMU) and same_bits(V, FV), r
            (Ug, vg), (Uf, vf) = q.item_values_multi(), fq.item_values_multi()
            assert np.array_equal(q.debug()["item_region"], fq.debug()["item_region"])
            assert same_bits(Ug, Uf) and same_bits(vg, vf), r

    rounds()
    _, Y13 = MR.targets(13)
    m.set_targets_multi_global(np.asfortranarray(Y13))
    m.solve_multi()
    assert m.R == 13 and np.all(m.trend_info() == 0)
    rounds()


# ------------------------------------------------------------------------------------ 8. query-side diagonal addends
def _addends(N):
    return 0.01 + 0.04 * np.random.default_rng(77).uniform(size=N)


@pytest.mark.parametrize("noisy", [False, True])
def test_query_diagonal_addends_single_output(noisy):
    """pmk_query_set_diag on the query of a blended leave-one-out: a non-member item carries its point's addend as
    pmk_query_items_fitted does; a member item is a property of the fit and ignores it"""
    eps, radius = 0.3, 0.6
    X, y = BR.workload()
    o = EC._cached(("base", eps), lambda: BR.Oracle(X, y, eps, EC.UNIFORM))
    m = _single(o, cache="base")
    add = _addends(len(X))
    plain = _staged(m, X, radius, noisy)[0].debug()
    q = pmk.DeviceQuery(m, X)
    q.set_diag(add)
    total = q.plan(radius, DELTA)
    nm, ns = q.items_loo(noisy)
    dbg = q.debug()
    q2 = pmk.DeviceQuery(m, X)
    q2.set_diag(add)
    assert q2.plan(radius, DELTA) == total
    q2.items_fitted()
    member, _, u, v = TB._expected_items(m, dbg, q2.debug(), y, [SIGMA2] * m.P, noisy)
    assert int((~member).sum()) == ns > 0 and nm > 0
    assert same_bits(dbg["item_u"][~member], u[~member]) and same_bits(dbg["item_v"][~member], v[~member])
    assert same_bits(dbg["item_u"][member], plain["item_u"][member]) and same_bits(dbg["item_v"][member], plain["item_v"][member])
    # the addend is in there: every non-member variance moved, by about its point's addend
    point = np.repeat(np.arange(len(X)), np.diff(dbg["item_offsets"]))
    moved = dbg["item_v"][~member] - plain["item_v"][~member]
    assert np.all(moved > 0) and np.abs(moved - add[point[~member]]).max() <= 1e-9
    q.set_diag(None)
    q.items_loo(noisy)
    again = q.debug()
    assert same_bits(again["item_u"], plain["item_u"]) and same_bits(again["item_v"], plain["item_v"])


@pytest.mark.parametrize("noisy", [False, True])
def test_query_diagonal_addends_multi_output(noisy):
    eps, radius = 0.3, 0.6
    X, Y = MR.targets(3)
    o = EC._cached(("base_multi", eps), lambda: MR.MultiOracle(X, Y, eps, EC.UNIFORM, "linear"))
    m = _multi(o)
    add = _addends(len(X))
    Up, vp = _staged_multi(m, X, radius, noisy)[0].item_values_multi()
    q = pmk.DeviceQuery(m, X)
    q.set_diag(add)
    total = q.plan(radius, DELTA)
    nm, no = q.items_loo_multi(noisy)
    dbg = q.debug()
    Ug, vg = q.item_values_multi()
    q2 = pmk.DeviceQuery(m, X)
    q2.set_diag(add)
    assert q2.plan(radius, DELTA) == total
    q2.items_multi_fitted(True)
    member, Ue, ve = TM._expected_items(m, dbg, q2.item_values_multi(), Y, [SIGMA2] * m.P, noisy)
    assert int((~member).sum()) == no > 0 and nm > 0
    assert same_bits(Ug[~member], Ue[~member]) and same_bits(vg[~member], ve[~member])
    assert same_bits(Ug[member], Up[member]) and same_bits(vg[member], vp[member])
    point = np.repeat(np.arange(len(X)), np.diff(dbg["item_offsets"]))
    moved = vg[~member] - vp[~member]
    assert np.all(moved > 0) and np.abs(moved - add[point[~member]]).max() <= 1e-9
    q.set_diag(None)
    q.items_loo_multi(noisy)
    Ua, va = q.item_values_multi()
    assert same_bits(Ua, Up) and same_bits(va, vp)


# ------------------------------------------------------------------------------------ 9. duplicated points
@pytest.mark.parametrize("trend", [None, "linear"])
def test_duplicated_points_are_told_apart_by_index(trend):
    """ten points stand twice in the data under two global indices, with different targets: both twins are members of
    the same patches in different rows, the lookup goes by index, and leaving one out keeps the other"""
    o = EC.dup_oracle(trend)
    c = EC.DUP
    h, r = c["N"] // 2, c["radius"]
    if trend is None:
        m, q, _, _ = _single_case(o, r, "f64", "duplicates", D=c["D"])
        Y, V = q.fetch()
        MU = Y[:, None]
    mm, qm, _, (MUm, Vm) = _multi_case(o, r, "f64", "duplicates", D=c["D"])
    dbg = qm.debug()
    off, reg = dbg["item_offsets"], dbg["item_region"]
    row_of = TM._row_lookup(mm)
    for k in range(c["pairs"]):
        a, b = k, h + k
        assert np.array_equal(o.X[a], o.X[b])
        ra, rb = reg[off[a]:off[a + 1]], reg[off[b]:off[b + 1]]
        assert np.array_equal(ra, rb)                       # the same point: the same items
        rows_a, rows_b = [row_of(int(p), a) for p in ra], [row_of(int(p), b) for p in rb]
        assert rows_a[-1] >= 0 and rows_b[-1] >= 0          # both are members of their home patch
        assert all((x >= 0) == (y >= 0) and (x < 0 or x != y) for x, y in zip(rows_a, rows_b)), (rows_a, rows_b)
        for col in range(o.R):
            assert o.Y[a, col] != o.Y[b, col] and MUm[a, col] != MUm[b, col], (k, col)
        if trend is None:
            assert MU[a, 0] != MU[b, 0]

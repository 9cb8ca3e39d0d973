"""Per-patch kernels and noise on the GPU: pmk_model_fit_patches, pmk_model_set_kernels, pmk_model_get_hyper, the
*_fitted predict calls and the selection helper.

The per-patch kernels are separate instantiations of the uniform ones that read theta (and sigma2) of the workgroup's
patch from device arrays; everything else is the same instruction stream.  So the main claim is BIT IDENTITY
(np.array_equal): what patch r gets from a per-patch fit is what it gets from the uniform fit at (theta_r, sigma2_r),
whatever its neighbours' hyperparameters are -- provided both run the same compile-time family (Spline34 if every patch
is Spline34, the run-time switch otherwise).  Shapes: D = 2, patch sizes that cross the 64- and
128-row tile edges, give 1..6 block rows and put the tallest patch off position 0 (the fit schedule sorts by tile count:
a theta indexed by sorted position instead of patch id shows).  Values are checked against the CPU oracle with the
bounds of tests/test_gpu_family_parity.py (fit) and of SURVEY section 8(d) (predict).
"""
import ctypes as C

import numpy as np
import pytest

import patchmixturekriging_amd as pmk
from patchmixturekriging_amd import _lib
from patchmixturekriging_amd import mixture as M
from oracle import oracle as O

import _query_refs as R

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
EPS64 = float(np.finfo(np.float64).eps)
SIZES = [63, 700, 1, 257, 129, 65, 127]
A_R = [1 / 2.0, 1 / 3.0, 1 / 4.0, 1 / 5.0, 1 / 6.0, 2 / 5.0, 2 / 7.0]             # distinct Spline34 a_r
S2_R = [1e-3, 1e-5, 1e-2, 3e-4, 3e-5, 1e-4, 3e-3]                                 # distinct sigma2_r in [1e-5, 1e-2]


def _f(X):
    return np.sin(X[:, 0]) * np.cos(0.5 * X[:, -1])


def _ragged(D=2, lo=-4.0, hi=4.0, seed=4711, sizes=SIZES):
    rng = np.random.default_rng(seed)
    Xs = [rng.uniform(lo, hi, (n, D)) for n in sizes]
    return Xs, [_f(x) for x in Xs]


def _factors(model, r):
    return model.get(r, M.GET_L), model.get(r, M.GET_C), model.get(r, M.GET_LINV_DIAG)


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


_CACHE = {}


def _s34_thetas():
    return [pmk.Spline34KernelType(a) for a in A_R]


def _uniform_refs(dtype):
    """patch r of the uniform fit at (theta_r, sigma2_r), for every r: computed once, shared, never changed"""
    key = ("uniform", dtype)
    if key not in _CACHE:
        Xs, ys = _ragged()
        model = pmk.DeviceModel(Xs, ys, dtype=dtype)
        refs = []
        for r, (th, s2) in enumerate(zip(_s34_thetas(), S2_R)):
            model.fit(th, s2)
            assert model.info()[r] == 0
            refs.append(_factors(model, r))
        _CACHE[key] = refs
    return _CACHE[key]


# ------------------------------------------------------------------------------------ 1. neighbours do not matter
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_a_patch_does_not_depend_on_its_neighbours_theta(dtype):
    Xs, ys = _ragged()
    refs = _uniform_refs(dtype)
    model = pmk.DeviceModel(Xs, ys, dtype=dtype)
    ths = _s34_thetas()
    model.fit_patches(ths, S2_R)
    assert np.all(model.info() == 0)
    for r in range(len(SIZES)):
        got = _factors(model, r)
        for name, g, w in zip(("L", "c", "Linv"), got, refs[r]):
            assert np.array_equal(g, w), "patch %d (n = %d): %s differs from the uniform fit at (theta_%d, sigma2_%d)" % (
                r, SIZES[r], name, r, r)
    descs, s2 = model.hyper()
    assert [d[0] for d in descs] == [1] * len(SIZES) and [d[1] for d in descs] == [0] * len(SIZES)
    assert [d[2][0] for d in descs] == A_R and s2.tolist() == S2_R
    # GET_K rebuilds patch r with its own theta (in fp64, on the coordinates the model holds: rounded to fp32 in an f32 model)
    for r in (0, 3):
        K = model.get(r, M.GET_K)
        Xr = Xs[r] if dtype == "f64" else Xs[r].astype(np.float32).astype(np.float64)
        assert np.abs(K - O.kernel_matrix(O.kernel(O.SPLINE34, A_R[r]), Xr)).max() <= 1e-14
    # P copies of one (theta, sigma2) are the plain fit on every patch, and a plain fit reports P copies
    model.fit_patches([ths[4]] * len(SIZES), [S2_R[4]] * len(SIZES))
    same = [_factors(model, r) for r in range(len(SIZES))]
    model.fit(ths[4], S2_R[4])
    for r in range(len(SIZES)):
        assert _same(same[r], _factors(model, r)), r
    descs, s2 = model.hyper()
    assert [d[2][0] for d in descs] == [A_R[4]] * len(SIZES) and s2.tolist() == [S2_R[4]] * len(SIZES)


# ------------------------------------------------------------------------------------ 2. mixed families
# parameters, domains and noise levels of tests/test_gpu_family_parity.py (FAMILIES), whose bounds are applied below;
# kappa(U) eps32 <= 1e-3 is what those bounds assume and is asserted per patch
MIXED_2D = [("spline34", pmk.Spline34KernelType(1.0), O.kernel(O.SPLINE34, 1.0), 0.05),
            ("spline12", pmk.Spline12KernelType(1.0), O.kernel(O.SPLINE12, 1.0), 0.05),
            ("spline32", pmk.Spline32KernelType(1.0), O.kernel(O.SPLINE32, 1.0), 0.05),
            ("gaussian", pmk.GaussianKernel1DType(4.0), O.kernel(O.GAUSSIAN, 4.0), 0.05),
            ("rq", pmk.RationalQuadraticKernelType(0.1), O.kernel(O.RQ, 0.1), 0.05),
            ("trq", pmk.TunableRationalQuadraticKernelType(0.1, 0.7), O.kernel(O.TRQ, 0.1, 0.7), 0.05),
            ("spline34", pmk.Spline34KernelType(0.5), O.kernel(O.SPLINE34, 0.5), 0.02)]
MIXED_1D = [("spline34", pmk.Spline34KernelType(1.0), O.kernel(O.SPLINE34, 1.0), 0.05),
            ("modsqexp", pmk.ModulatedSqExpKernelType(4.0, 3.0), O.kernel(O.MODSQEXP, 4.0, 3.0), 0.05),
            ("bb10", pmk.BrownianBridge10(1.0), O.kernel(O.BB10, 1.0), 0.05),
            ("bb2eps", pmk.BrownianBridge2eps(2.5), O.kernel(O.BB2EPS, 2.5), 3.0),
            ("spline32", pmk.Spline32KernelType(1.0), O.kernel(O.SPLINE32, 1.0), 0.05),
            ("bb10", pmk.BrownianBridge10(1.0), O.kernel(O.BB10, 1.0), 0.02),
            ("modsqexp", pmk.ModulatedSqExpKernelType(4.0, 3.0), O.kernel(O.MODSQEXP, 4.0, 3.0), 0.1)]


def _mixed_case(D):
    if D == 2:
        Xs, ys = _ragged(2, -2.0, 2.0, seed=4712)
        return MIXED_2D, Xs, [np.sin(3 * x[:, 0]) + x[:, -1] ** 2 for x in Xs]
    Xs, ys = _ragged(1, 0.0, 1.0, seed=4713)
    return MIXED_1D, Xs, [np.sin(3 * x[:, 0]) + x[:, -1] ** 2 for x in Xs]


def _residual(U, c, y):
    return np.linalg.norm(U @ c - y) / (np.linalg.norm(U) * np.linalg.norm(c) + np.linalg.norm(y))


@pytest.mark.parametrize("D", [2, 1])
def test_mixed_families(D):
    spec, Xs, ys = _mixed_case(D)
    model = pmk.DeviceModel(Xs, ys)
    model.fit_patches([s[1] for s in spec], [s[3] for s in spec])
    assert np.all(model.info() == 0), model.info()
    got = [_factors(model, r) for r in range(len(Xs))]
    descs, s2 = model.hyper()
    assert [d[0] for d in descs] == [s[1].family for s in spec] and s2.tolist() == [s[3] for s in spec]
    uni = pmk.DeviceModel(Xs, ys)
    for r, (fam, th, oth, sigma2) in enumerate(spec):
        X, y = Xs[r], ys[r]
        L, c, _ = got[r]
        if fam != "spline34":                   # both run the run-time family switch: the same bits
            uni.fit(th, sigma2)
            assert uni.info()[r] == 0
            assert _same(got[r], _factors(uni, r)), (r, fam)
        fo = O.fit_patch(oth, X, y, sigma2)
        assert fo["info"] == 0, (r, fam)
        U = O.kernel_matrix(oth, X) + sigma2 * np.eye(len(y))
        assert R.kappa(U) * EPS32 <= 1e-3, (r, fam, R.kappa(U))
        back = np.linalg.norm(L @ L.T - U) / np.linalg.norm(U)
        res = _residual(U, c, y)
        print("D=%d patch %d %s n=%d: backward %.2e residual %.2e |dL| %.2e dc_lu %.2e" % (
            D, r, fam, len(y), back, res, np.abs(L - fo["L"]).max(), np.linalg.norm(c - fo["c_lu"]) / np.linalg.norm(fo["c_lu"])))
        assert np.all(np.triu(L, 1) == 0)
        assert back <= 1e-14, (r, fam, back)
        assert res <= 1e-13, (r, fam, res)
        assert np.abs(L - fo["L"]).max() <= 1e-8, (r, fam)
        assert np.linalg.norm(c - fo["c_chol"]) / np.linalg.norm(fo["c_chol"]) <= 1e-6, (r, fam)
        assert np.linalg.norm(c - fo["c_lu"]) / np.linalg.norm(fo["c_lu"]) <= 1e-6, (r, fam)
        K = model.get(r, M.GET_K)               # rebuilt with the patch's own family
        assert np.abs(K - (U - sigma2 * np.eye(len(y)))).max() <= 1e-13, (r, fam)


def test_bad_kernels_are_refused_and_the_patch_is_named():
    Xs, ys = _ragged()
    model = pmk.DeviceModel(Xs, ys)
    L = model.ctx.L
    ths = _s34_thetas()
    descs, s2 = M.patch_hyper(ths, S2_R, len(SIZES))
    descs[5].family = 99
    assert L.pmk_model_fit_patches(model.h, descs, s2.ctypes.data_as(C.POINTER(C.c_double))) == -2
    assert "patch 5" in L.pmk_last_error().decode()
    ths[2] = pmk.ModulatedSqExpKernelType(4.0, 3.0)             # D = 2
    with pytest.raises(_lib.PmkError, match="patch 2"):
        model.fit_patches(ths, S2_R)
    assert L.pmk_model_fit_patches(model.h, None, s2.ctypes.data_as(C.POINTER(C.c_double))) == -1
    assert L.pmk_model_fit_patches(model.h, descs, None) == -1
    # set_kernels is for loaded models: a fit records its own kernels
    model.fit_patches(_s34_thetas(), S2_R)
    with pytest.raises(_lib.PmkError):
        model.set_kernels(_s34_thetas())


# ------------------------------------------------------------------------------------ 3. a failed patch stays local
def _scores(model):
    logdet, quad = model.evidence()
    model.loo()
    res, var = model.loo_values()
    return logdet, quad, res, var


def test_a_failed_patch_stays_local():
    """patch 3: points 0 and 1 coincide and sigma2_3 = 0, so U[:2, :2] = [[1, 1], [1, 1]] and pivot 2 is 1 - 1 * 1 = 0 in
    any precision and any summation order"""
    Xs, ys = _ragged()
    refs = _uniform_refs("f64")
    healthy = pmk.DeviceModel(Xs, ys)
    healthy.fit_patches(_s34_thetas(), S2_R)
    want = _scores(healthy)
    bad = 3
    Xb = [x.copy() for x in Xs]
    Xb[bad][1] = Xb[bad][0]
    s2 = list(S2_R)
    s2[bad] = 0.0
    model = pmk.DeviceModel(Xb, ys)
    model.fit_patches(_s34_thetas(), s2)
    info = model.info()
    assert info[bad] == 2, info
    assert np.all(np.delete(info, bad) == 0), info
    for r in range(len(SIZES)):
        if r != bad:
            assert _same(_factors(model, r), refs[r]), r
    logdet, quad, res, var = _scores(model)
    assert np.isnan(logdet[bad]) and np.isnan(quad[bad])
    assert np.all(np.isnan(res[bad])) and np.all(np.isnan(var[bad]))
    for r in range(len(SIZES)):
        if r != bad:
            assert logdet[r] == want[0][r] and quad[r] == want[1][r], r
            assert np.array_equal(res[r], want[2][r]) and np.array_equal(var[r], want[3][r]), r


# ------------------------------------------------------------------------------------ 4. other paths through the fit
def test_forced_split_mode():
    Xs, ys = _ragged(sizes=[700, 300], seed=4714)
    ths, s2 = [pmk.Spline34KernelType(1 / 3.0), pmk.Spline34KernelType(1 / 5.0)], [1e-3, 1e-4]
    L = pmk.default_context().L
    model = pmk.DeviceModel(Xs, ys)
    assert L.pmk_test_model_set_split(model.h, 1) == 0
    model.fit_patches(ths, s2)
    assert np.all(model.info() == 0)
    got = [_factors(model, r) for r in range(2)]
    uni = pmk.DeviceModel(Xs, ys)
    assert L.pmk_test_model_set_split(uni.h, 1) == 0
    for r in range(2):
        uni.fit(ths[r], s2[r])
        assert _same(got[r], _factors(uni, r)), r
    # the batched path sums in another order: close, and not what is compared above
    batched = pmk.DeviceModel(Xs, ys)
    batched.fit_patches(ths, s2)
    assert np.abs(batched.get(0, M.GET_L) - got[0][0]).max() <= 1e-10


def test_fit_with_diagonal_addends():
    Xs, ys = _ragged()
    rng = np.random.default_rng(4715)
    dg = [rng.uniform(0.0, 0.5, n) for n in SIZES]
    model = pmk.DeviceModel(Xs, ys)
    model.set_diag(dg)
    model.fit_patches(_s34_thetas(), S2_R)
    assert np.all(model.info() == 0)
    got = [_factors(model, r) for r in range(len(SIZES))]
    plain = _uniform_refs("f64")
    uni = pmk.DeviceModel(Xs, ys)
    uni.set_diag(dg)
    for r, (th, s2) in enumerate(zip(_s34_thetas(), S2_R)):
        uni.fit(th, s2)
        assert _same(got[r], _factors(uni, r)), r
        if SIZES[r] > 1:
            assert not np.array_equal(got[r][0], plain[r][0]), r        # the addends matter
    K = model.get(1, M.GET_K)
    assert np.abs(K - O.kernel_matrix(O.kernel(O.SPLINE34, A_R[1]), Xs[1]) - np.diag(dg[1])).max() <= 1e-14


def test_solve_multi_evidence_and_loo_after_a_per_patch_fit():
    Xs, ys = _ragged()
    Ys = [np.stack([y, np.cos(x[:, 0] - x[:, 1]), 0.3 * x[:, 1] - 0.1], 1) for x, y in zip(Xs, ys)]
    model = pmk.DeviceModel(Xs, ys)
    model.fit_patches(_s34_thetas(), S2_R)
    model.set_targets_multi(Ys)
    model.solve_multi()
    Cs = model.weights_multi()
    logdet, quad, res, var = _scores(model)
    logdet_m, quad_m = model.evidence_multi()
    uni = pmk.DeviceModel(Xs, ys)
    uni.set_targets_multi(Ys)
    for r, (th, s2) in enumerate(zip(_s34_thetas(), S2_R)):
        uni.fit(th, s2)
        uni.solve_multi()
        assert np.array_equal(uni.weights_multi()[r], Cs[r]), r
        ul, uq, ur, uv = _scores(uni)
        assert ul[r] == logdet[r] and uq[r] == quad[r], r
        assert np.array_equal(ur[r], res[r]) and np.array_equal(uv[r], var[r]), r
        ulm, uqm = uni.evidence_multi()
        assert ulm[r] == logdet_m[r] and np.array_equal(uqm[r], quad_m[r]), r
    # a new per-patch fit invalidates both, as pmk_model_fit does
    model.fit_patches(_s34_thetas(), S2_R)
    with pytest.raises(_lib.PmkError):
        model.loo_values()
    with pytest.raises(_lib.PmkError):
        model.evidence_multi()
    assert model.ctx.L.pmk_model_evidence_multi(model.h, None, None) == -3        # the library refuses as well
    assert model.ctx.L.pmk_model_get_loo(model.h, None, None) == -3


# ------------------------------------------------------------------------------------ 5.-8. predict
LEVELS, EPS_OVERLAP, RADIUS, DELTA, NQ, EMPTY = 3, 0.5, 0.4, 1e-5, 3000, 2
PRED = {
    # per-leaf hyperparameters: distinct Spline34 a_r and sigma2_r in [1e-5, 1e-2]
    "s34": ([pmk.Spline34KernelType(a) for a in (1 / 4.0, 1 / 3.0, 1 / 5.0, 2 / 7.0)],
            [O.kernel(O.SPLINE34, a) for a in (1 / 4.0, 1 / 3.0, 1 / 5.0, 2 / 7.0)], [1e-5, 1e-3, 1e-2, 1e-4]),
    # mixed families at the noise level of tests/test_gpu_family_parity.py (kappa(U) eps32 <= 1e-3, asserted)
    "mixed": ([pmk.Spline34KernelType(0.5), pmk.Spline32KernelType(0.5), pmk.GaussianKernel1DType(4.0),
               pmk.RationalQuadraticKernelType(0.1)],
              [O.kernel(O.SPLINE34, 0.5), O.kernel(O.SPLINE32, 0.5), O.kernel(O.GAUSSIAN, 4.0), O.kernel(O.RQ, 0.1)],
              [0.05, 0.05, 0.02, 0.1]),
}
WTH, OWTH = pmk.Spline34KernelType(1 / RADIUS), O.kernel(O.SPLINE34, 1 / RADIUS)


def _tree_case():
    """~1500 training points on a 3-level tree (4 leaves, eps-overlap) and 3000 queries none of which touches leaf EMPTY
    (neither as home nor as neighbour: filtered with the oracle's plan), so that region gets no strip task while the
    others get several strips each"""
    if "tree" in _CACHE:
        return _CACHE["tree"]
    rng = np.random.Generator(np.random.PCG64(4716))
    N = 1500
    X = np.stack([rng.uniform(-5, 5, N), rng.uniform(-10, 10, N)], 1)
    y = np.sin(X[:, 0]) * np.cos(0.3 * X[:, 1])
    root, _, _ = pmk.setuppartition(X, LEVELS)
    X_set, X_set_inds, _, _ = pmk.organizetrainingsets(root, LEVELS, X, EPS_OVERLAP)
    assert len(X_set) == 4
    ob = O.BSP(X, LEVELS)
    cand = np.stack([rng.uniform(-5, 5, 3 * NQ), rng.uniform(-10, 10, 3 * NQ)], 1)
    home, off, reg, _ = R.oracle_plan(ob, cand, RADIUS, DELTA)
    touches = home == EMPTY
    nbq = np.repeat(np.arange(len(cand)), np.diff(off))
    touches[nbq[reg == EMPTY]] = True
    Xq = np.ascontiguousarray(cand[~touches][:NQ])
    assert len(Xq) == NQ
    out = dict(X=X, ys=[y[i] for i in X_set_inds], Xq=Xq, root=root, X_set=X_set, ob=ob)
    _CACHE["tree"] = out
    return out


def _predict_case(name, dtype):
    """the per-patch fit and predict of one configuration, with the uniform items(theta_r) runs on the SAME plan"""
    key = ("pred", name, dtype)
    if key in _CACHE:
        return _CACHE[key]
    t = _tree_case()
    ths, oths, s2 = PRED[name]
    m = pmk.DeviceModel(t["X_set"], t["ys"], dtype=dtype)
    m.fit_patches(ths, s2)
    assert np.all(m.info() == 0)
    m.set_bsp(t["root"], 0)
    q = pmk.DeviceQuery(m, t["Xq"])
    q.plan(RADIUS, DELTA)
    counts = np.diff(q.region_offsets(4))
    # the shapes this test is about: a region of several strips (one lock-step group), a region without any item
    assert counts[EMPTY] == 0 and counts.max() > 2 * R.TQ, counts
    assert len(R.strip_counts(int(counts.max()))) >= 3
    q.items_fitted()
    q.mix(WTH)
    Yq, Vq = q.fetch()
    dbg = q.debug()
    uniform = []
    for th in ths:
        q.items(th)
        d = q.debug()
        uniform.append((d["item_u"].copy(), d["item_v"].copy()))
    out = dict(m=m, q=q, Yq=Yq, Vq=Vq, dbg=dbg, uniform=uniform, counts=counts)
    _CACHE[key] = out
    return out


def _blend_tolerance(dbg, item_u, item_v):
    """Yq = sum w u and Vq = sum w (v w) over at most 4 items with w = w~ / sum w~: the device and numpy sum in their own
    orders and each operation rounds once, so they differ by at most (items + 3) eps of sum |w u| (resp. sum w^2 v);
    16 eps covers 4 items with room for the division"""
    off = dbg["item_offsets"]
    ty, tv = np.empty(len(off) - 1), np.empty(len(off) - 1)
    for j in range(len(ty)):
        s = slice(off[j], off[j + 1])
        w = dbg["item_w"][s] / dbg["item_w"][s].sum()
        ty[j], tv[j] = 16 * EPS64 * (w @ np.abs(item_u[s])), 16 * EPS64 * (w @ (item_v[s] * w))
    return ty, tv


@pytest.mark.parametrize("name", ["s34", "mixed"])
def test_predict_single_output(name):
    t = _tree_case()
    p = _predict_case(name, "f64")
    ths, oths, s2 = PRED[name]
    dbg, reg = p["dbg"], p["dbg"]["item_region"]
    assert off_ok(dbg)
    for r in range(4):
        idx = np.nonzero(reg == r)[0]
        assert len(idx) == p["counts"][r]
        uu, uv = p["uniform"][r]
        assert np.array_equal(dbg["item_u"][idx], uu[idx]), "region %d: item_u differs from items(theta_%d)" % (r, r)
        assert np.array_equal(dbg["item_v"][idx], uv[idx]), "region %d: item_v differs from items(theta_%d)" % (r, r)
        for o in range(4):                      # and theta matters: another region's theta gives other values
            if o != r and len(idx):
                assert not np.array_equal(p["uniform"][o][0][idx], uu[idx]), (r, o)
    # the blend of the device's own items
    Y, V = R.blend_reference(dbg, dbg["item_u"], dbg["item_v"])
    ty, tv = _blend_tolerance(dbg, dbg["item_u"], dbg["item_v"])
    assert np.all(np.abs(p["Yq"] - Y) <= ty) and np.all(np.abs(p["Vq"] - V) <= tv)
    # independently: queryinner! with theta_r on the oracle's own fits, blended
    off = dbg["item_offsets"]
    u_ref, v_ref = np.empty(off[-1]), np.empty(off[-1])
    for r in range(4):
        idx = np.nonzero(reg == r)[0]
        if not len(idx):
            continue
        fo = O.fit_patch(oths[r], t["X_set"][r], t["ys"][r], s2[r])
        assert fo["info"] == 0
        qj = np.searchsorted(off, idx, side="right") - 1
        mu, var, _, _ = R.queryinner_reference(oths[r], t["X_set"][r], fo["c_lu"], fo["L"], t["Xq"][qj])
        u_ref[idx], v_ref[idx] = mu, var
    oY, oV = R.blend_reference(dbg, u_ref, v_ref)
    R.assert_fp64_values(p["Yq"], p["Vq"], oY, oV, name)
    # the one-shot entry point
    Y1, V1 = np.empty(NQ), np.empty(NQ)
    w = WTH.desc()
    _lib.check(p["m"].ctx.L.pmk_predict_mixture_fitted(p["m"].h, C.byref(w), NQ, M._d(t["Xq"]), RADIUS, DELTA, M._d(Y1), M._d(V1)))
    assert np.array_equal(Y1, p["Yq"]) and np.array_equal(V1, p["Vq"])


def off_ok(dbg):
    off = dbg["item_offsets"]
    return off[0] == 0 and off[-1] == len(dbg["item_region"]) and np.all(np.diff(off) >= 1)


def test_predict_single_output_fp32_against_the_fp64_device_run():
    """fp32 items are bit-identical to the uniform fp32 runs; values against the fp64 DEVICE run with the fp32 bounds of
    tests/test_gpu_family_parity.py: forward errors scaled by kappa(U) eps32, with kappa(U) eps32 <= 1e-3 asserted"""
    t = _tree_case()
    p32, p64 = _predict_case("mixed", "f32"), _predict_case("mixed", "f64")
    ths, oths, s2 = PRED["mixed"]
    dbg, reg = p32["dbg"], p32["dbg"]["item_region"]
    assert np.array_equal(reg, p64["dbg"]["item_region"]) and np.array_equal(dbg["item_w"], p64["dbg"]["item_w"])
    kmax = 0.0
    for r in range(4):
        idx = np.nonzero(reg == r)[0]
        uu, uv = p32["uniform"][r]
        assert np.array_equal(dbg["item_u"][idx], uu[idx]) and np.array_equal(dbg["item_v"][idx], uv[idx]), r
        if not len(idx):
            continue
        k = R.kappa(O.kernel_matrix(oths[r], t["X_set"][r]) + s2[r] * np.eye(len(t["X_set"][r])))
        assert k * EPS32 <= 1e-3, (r, k)
        kmax = max(kmax, k)
        # |k| <= 1 for these families and |L^-1 k|^2 <= k(x, x) = 1: scales |k|.|c| <= |c|_1 and k(x,x) + |L^-1 k|^2 <= 2
        msc = np.abs(p64["m"].get(r, M.GET_C)).sum()
        du = np.abs(dbg["item_u"][idx] - p64["dbg"]["item_u"][idx])
        dv = np.abs(dbg["item_v"][idx] - p64["dbg"]["item_v"][idx])
        print("region %d: kappa eps32 %.2e, max |du| %.2e (bound %.2e), max |dv| %.2e (bound %.2e)" % (
            r, k * EPS32, du.max(), 50 * k * EPS32 * (msc + 1), dv.max(), 50 * k * EPS32 * 3))
        assert np.all(du <= 50 * k * EPS32 * (msc + 1)), (r, du.max())
        assert np.all(dv <= 50 * k * EPS32 * 3), (r, dv.max())
    Y, V = p64["Yq"], p64["Vq"]
    assert np.abs(p32["Yq"] - Y).max() <= 50 * kmax * EPS32 * max(1, np.abs(Y).max())
    assert np.all(np.abs(p32["Vq"] - V) <= 50 * kmax * EPS32 * 3)


def _item_means(m, dbg, Xq, run):
    """per-item means [T, R] through a query of explicit (point, region) items: one item per 'query', whose mixture weight
    is 1 / 1, so that Yq of that query IS the item's mean (1.0 * u)"""
    off, reg = dbg["item_offsets"], dbg["item_region"]
    qj = np.searchsorted(off, np.arange(off[-1]), side="right") - 1
    xs = np.ascontiguousarray(Xq[qj])
    rg = np.ascontiguousarray(reg, dtype=np.int32)
    q = pmk.DeviceQuery.from_items(m, len(rg), xs.ctypes.data, rg.ctypes.data)
    run(q)
    q.mix_multi(WTH)
    return q.fetch_multi(m.R)


def test_predict_multi_output():
    t = _tree_case()
    p = _predict_case("s34", "f64")
    ths, _, s2 = PRED["s34"]
    m, dbg, reg = p["m"], p["dbg"], p["dbg"]["item_region"]
    Ys = [np.stack([y, np.cos(0.4 * x[:, 0] - 0.2 * x[:, 1]), 0.3 * x[:, 1] - 0.1], 1) for x, y in zip(t["X_set"], t["ys"])]
    m.set_targets_multi(Ys)
    m.solve_multi()
    per_r = [_item_means(m, dbg, t["Xq"], lambda q, th=th: q.items_multi(th, False))[0] for th in ths]
    for variance in (False, True):
        U, v = _item_means(m, dbg, t["Xq"], lambda q: q.items_multi_fitted(variance))
        assert U.shape == (len(reg), 3) and (v is not None) == variance
        for r in range(4):
            idx = np.nonzero(reg == r)[0]
            assert np.array_equal(U[idx], per_r[r][idx]), (variance, r)
            for o in range(4):
                if o != r and len(idx):
                    assert not np.array_equal(per_r[o][idx], per_r[r][idx]), (r, o)
        if variance:                            # item order = the order given: v of item i is test 5's item_v[i]
            assert np.array_equal(v, dbg["item_v"])
    # the planned query: Vq is test 5's, and column 0 (the single-output targets) blends to test 5's Yq up to the solves
    q = pmk.DeviceQuery(m, t["Xq"])
    q.plan(RADIUS, DELTA)
    q.items_multi_fitted(True)
    q.mix_multi(WTH)
    Yq, Vq = q.fetch_multi(3)
    assert np.array_equal(Vq, p["Vq"])
    assert np.all(np.abs(Yq[:, 0] - p["Yq"]) <= 1e-7 * np.maximum(1, np.abs(p["Yq"])))
    q.items_multi_fitted(False)
    q.mix_multi(WTH)
    Y0, V0 = q.fetch_multi(3)
    assert V0 is None and np.array_equal(Y0, Yq)
    Y1, V1 = np.empty((NQ, 3), order="F"), np.empty(NQ)
    w = WTH.desc()
    _lib.check(m.ctx.L.pmk_predict_mixture_multi_fitted(m.h, C.byref(w), NQ, M._d(t["Xq"]), RADIUS, DELTA, M._d(Y1), NQ, M._d(V1)))
    assert np.array_equal(Y1, Yq) and np.array_equal(V1, Vq)


def test_loaded_model_needs_kernels_then_gives_the_same_bits():
    t = _tree_case()
    p = _predict_case("s34", "f64")
    ths, _, _ = PRED["s34"]
    m = p["m"]
    loaded = pmk.DeviceModel.from_factors(t["X_set"], m.weights(), [m.get(r, M.GET_L) for r in range(4)])
    loaded.set_bsp(t["root"], 0)
    q = pmk.DeviceQuery(loaded, t["Xq"])
    q.plan(RADIUS, DELTA)
    with pytest.raises(_lib.PmkError):
        q.items_fitted()
    assert q.L.pmk_query_items_fitted(q.h) == -3                  # the library refuses as well
    assert q.L.pmk_model_get_hyper(loaded.h, None, None) == -3
    loaded.set_kernels(ths)
    descs, s2 = loaded.hyper()
    assert [d[2][0] for d in descs] == [th.a for th in ths] and np.all(np.isnan(s2))
    q.items_fitted()
    q.mix(WTH)
    Yq, Vq = q.fetch()
    dbg = q.debug()
    assert np.array_equal(dbg["item_u"], p["dbg"]["item_u"]) and np.array_equal(dbg["item_v"], p["dbg"]["item_v"])
    assert np.array_equal(Yq, p["Yq"]) and np.array_equal(Vq, p["Vq"])


@pytest.mark.parametrize("th", [pmk.Spline34KernelType(1 / 4.0), pmk.Spline32KernelType(0.5)], ids=["spline34", "spline32"])
def test_fitted_calls_after_a_plain_fit_are_the_explicit_theta_calls(th):
    t = _tree_case()
    m = pmk.DeviceModel(t["X_set"], t["ys"])
    m.fit(th, 0.01)
    assert np.all(m.info() == 0)
    m.set_bsp(t["root"], 0)
    q = pmk.DeviceQuery(m, t["Xq"])
    q.plan(RADIUS, DELTA)
    q.items(th); q.mix(WTH)
    Y0, V0 = q.fetch()
    d0 = q.debug()
    q.items_fitted(); q.mix(WTH)
    Y1, V1 = q.fetch()
    d1 = q.debug()
    assert np.array_equal(d0["item_u"], d1["item_u"]) and np.array_equal(d0["item_v"], d1["item_v"])
    assert np.array_equal(Y0, Y1) and np.array_equal(V0, V1)
    Ys = [np.stack([y, 0.5 * y + 0.1], 1) for y in t["ys"]]
    m.set_targets_multi(Ys)
    m.solve_multi()
    q.items_multi(th, True); q.mix_multi(WTH)
    Ym0, Vm0 = q.fetch_multi(2)
    q.items_multi_fitted(True); q.mix_multi(WTH)
    Ym1, Vm1 = q.fetch_multi(2)
    assert np.array_equal(Ym0, Ym1) and np.array_equal(Vm0, Vm1) and np.array_equal(Vm1, V0)
    eta = pmk.MixtureGPType(t["X_set"], pmk.fetchhyperplanes(t["root"]))
    pmk.fitmixtureGP_(eta, t["ys"], th, 0.01)
    Y2, V2, _ = pmk.querymixtureGP_patches(t["Xq"], eta, t["root"], LEVELS, RADIUS, DELTA, WTH)
    assert np.array_equal(Y2, Y0) and np.array_equal(V2, V0)


# ------------------------------------------------------------------------------------ 9. selection
SEL_SIZES, SEL_OMEGA = [129, 257, 63, 300], (0.5, 1.5, 3.0, 6.0)
SEL_A, SEL_S2 = (1 / 8.0, 1 / 4.0, 1 / 2.0, 1.0), (1e-4, 1e-2)


def _selection_case():
    rng = np.random.default_rng(71)
    Xs = [rng.uniform(-4, 4, (n, 2)) for n in SEL_SIZES]
    ys = [np.sin(w * x[:, 0]) * np.cos(w * x[:, 1]) for w, x in zip(SEL_OMEGA, Xs)]
    cands = [(a, s2) for a in SEL_A for s2 in SEL_S2]
    return Xs, ys, cands


def _evidence_fp64(Xs, ys, cands):
    """log marginal likelihood of every (candidate, patch) from the oracle's kernel matrix, in numpy"""
    out = np.empty((len(cands), len(Xs)))
    for g, (a, s2) in enumerate(cands):
        oth = O.kernel(O.SPLINE34, a)
        for r, (X, y) in enumerate(zip(Xs, ys)):
            U = O.kernel_matrix(oth, X) + s2 * np.eye(len(y))
            assert R.kappa(U) <= 8e5
            Lc = np.linalg.cholesky(U)
            c = np.linalg.solve(U, y)
            out[g, r] = -0.5 * (y @ c) - np.log(np.diag(Lc)).sum() - 0.5 * len(y) * np.log(2 * np.pi)
    return out


def _loo_score(res, var):
    return float(np.sum(-0.5 * np.log(var) - res * res / (2.0 * var) - 0.5 * np.log(2.0 * np.pi)))


@pytest.mark.parametrize("score", ["evidence", "loo"])
def test_selection(score):
    Xs, ys, cands = _selection_case()
    pc = [(pmk.Spline34KernelType(a), s2) for a, s2 in cands]
    if score == "evidence":
        # what keeps this test meaningful: four different winners, every best-to-second gap far above the score error
        ref = _evidence_fp64(Xs, ys, cands)
        w_ref = pmk.select_candidates(ref)
        assert [cands[w] for w in w_ref] == [(1 / 8.0, 1e-4), (1 / 4.0, 1e-4), (1 / 2.0, 1e-4), (1.0, 1e-4)]
        assert len(set(w_ref.tolist())) > 1
        for r in range(len(Xs)):
            top = np.sort(ref[:, r])[::-1]
            assert top[0] - top[1] >= 1e-3 * abs(top[0]), (r, top[:2])
    # through the existing calls, candidate by candidate
    want = np.empty((len(pc), len(Xs)))
    eta0 = pmk.MixtureGPType(Xs, None)
    for g, (th, s2) in enumerate(pc):
        pmk.fitmixtureGP_(eta0, ys, th, s2)
        if score == "evidence":
            want[g] = pmk.logevidencemixtureGP(eta0)
        else:
            res, var = pmk.loomixtureGP(eta0)
            want[g] = [_loo_score(a, b) for a, b in zip(res, var)]
    w_want = pmk.select_candidates(want)
    eta = pmk.MixtureGPType(Xs, None)
    out, winners, scores = pmk.selectmixtureGP_(eta, ys, pc, score=score)
    assert out is eta
    assert np.array_equal(scores, want) and np.array_equal(winners, w_want)
    if score == "evidence":
        assert np.array_equal(winners, w_ref)
        assert np.abs(scores - ref).max() <= 1e-5 * np.abs(ref).max()
    # the model it leaves is the per-patch fit with the winners
    ths, s2s = [pc[w][0] for w in winners], [pc[w][1] for w in winners]
    assert eta.sigma2_set == s2s and eta.theta_set == ths
    m = pmk.DeviceModel(Xs, ys)
    m.fit_patches(ths, s2s)
    for r in range(len(Xs)):
        assert _same(_factors(eta._model, r), _factors(m, r)), r
        assert np.array_equal(eta.c_set[r], m.get(r, M.GET_C))
        assert np.array_equal(eta.L_set[r], m.get(r, M.GET_L))


def test_selection_scores_nan_where_a_candidate_cannot_be_factorised():
    """patch 1 has a duplicated point: the candidate with sigma2 = 0 fails there (NaN, not an exception) and cannot win"""
    Xs, ys, _ = _selection_case()
    Xs = [x.copy() for x in Xs]
    Xs[1][1] = Xs[1][0]
    ys = [y.copy() for y in ys]
    ys[1][1] = ys[1][0]
    pc = [(pmk.Spline34KernelType(0.25), 0.0), (pmk.Spline34KernelType(0.25), 1e-2)]
    eta = pmk.MixtureGPType(Xs, None)
    _, winners, scores = pmk.selectmixtureGP_(eta, ys, pc)
    assert np.isnan(scores[0, 1]) and not np.isnan(scores[1]).any() and winners[1] == 1
    assert eta.sigma2_set[1] == 1e-2

"""GPU parity matrix over what tests/test_gpu_parity.py checks for the headline case only (Spline34, fp64): every
kernel family through the generic slab build and the factorisation, D = 1..4, fp32 next to fp64, ragged batches that
straddle the 64-row slab tiles and the 128-row factor tiles, the fp32 split path, per-family predict strips across
the TQ = 256-column strip boundary, and DPP kernels through the two exchange forms of the sharded predict.

References: the CPU oracle (oracle/oracle.py) and LAPACK (scipy.linalg) in fp64.  fp64 is held to the bounds of
tests/test_gpu_parity.py.  fp32 has no reference semantics (the reference is Float64-only) and is judged by
backward error and residual in multiples of eps32, and by forward errors scaled by kappa(U) eps32; every case
asserts kappa(U) eps32 <= 1e-3, so that a later change of parameters cannot make those bounds vacuous.
"""

import numpy as np
import pytest
import scipy.linalg as sla

import patchmixturekriging_amd as pmk
from patchmixturekriging_amd import mixture as M
from oracle import oracle as O

from _query_refs import blend_reference as _blend_reference, queryinner_reference as _queryinner_reference

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
SIZES = [1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 385, 700]   # 64- and 128-row tile edges

# name -> (product kernel, oracle kernel, dimensions, domain, sigma2 or {D: sigma2}).  sigma2 keeps kappa(U) eps32 <= 1e-3
# at n = 700 (asserted per case).  BB2eps: the reference's formula gives an indefinite K (lambda_min(K) ~ -1.9 in 1-D,
# -3e-3 in 2-D at n = 700), so its noise level is what makes U positive definite -- K still enters every entry of U.
FAMILIES = {
    "spline34": (pmk.Spline34KernelType(1.0), O.kernel(O.SPLINE34, 1.0), (1, 2, 3, 4), "box", 0.05),
    "spline12": (pmk.Spline12KernelType(1.0), O.kernel(O.SPLINE12, 1.0), (1, 2, 3), "box", 0.05),
    "spline32": (pmk.Spline32KernelType(1.0), O.kernel(O.SPLINE32, 1.0), (1, 2, 3, 4), "box", 0.05),
    "gaussian": (pmk.GaussianKernel1DType(4.0), O.kernel(O.GAUSSIAN, 4.0), (1, 2, 3), "box", 0.05),
    "rq": (pmk.RationalQuadraticKernelType(0.1), O.kernel(O.RQ, 0.1), (1, 2, 3), "box", 0.05),
    "trq": (pmk.TunableRationalQuadraticKernelType(0.1, 0.7), O.kernel(O.TRQ, 0.1, 0.7), (1, 2, 3), "box", 0.05),
    "modsqexp": (pmk.ModulatedSqExpKernelType(4.0, 3.0), O.kernel(O.MODSQEXP, 4.0, 3.0), (1,), "box", 0.05),
    "bb10": (pmk.BrownianBridge10(1.0), O.kernel(O.BB10, 1.0), (1, 2), "unit", 0.05),
    "bb20": (pmk.BrownianBridge20(1.0), O.kernel(O.BB20, 1.0), (1, 2), "unit", 0.02),
    "bb1eps": (pmk.BrownianBridge1eps(4.5), O.kernel(O.BB1EPS, 4.5), (1, 2), "unit", 0.05),
    "bb2eps": (pmk.BrownianBridge2eps(2.5), O.kernel(O.BB2EPS, 2.5), (1, 2), "unit", {1: 3.0, 2: 5e-3}),
    "bb10_semiinf": (pmk.BrownianBridgeSemiInfDomain(pmk.BrownianBridge10(1.0)), O.kernel(O.BB10, 1.0, flags=O.FLAG_SEMIINF),
                     (1, 2), "semiinf", 0.05),
}
CASES = [(f, D, dt) for f, spec in FAMILIES.items() for D in spec[2] for dt in ("f64", "f32")]


def _ids(c):
    return "%s-%dd-%s" % c


def kappa(U):
    """2-norm condition number of a symmetric positive definite U (= np.linalg.cond(U), through eigvalsh: the same
    number at a fraction of the cost of an SVD)"""
    ev = np.linalg.eigvalsh(U)
    assert ev[0] > 0, ev[0]
    return float(ev[-1] / ev[0])


def _points(rng, domain, n, D):
    if domain == "unit":
        return rng.uniform(0.0, 1.0, (n, D))
    if domain == "semiinf":
        return rng.uniform(0.0, 5.0, (n, D))
    return rng.uniform(-2.0, 2.0, (n, D))


def _targets(X):
    return np.sin(3 * X[:, 0]) + X[:, -1] ** 2


_CACHE = {}


def _fitted(fam, D, dtype):
    """one ragged batch per (family, D, dtype), fitted once and shared by the fit and the predict tests; the fp64 LAPACK
    factor and weights of every patch (the oracle's U) come with it"""
    key = (fam, D, dtype)
    if key in _CACHE:
        return _CACHE[key]
    th, oth, _, domain, sigma2 = FAMILIES[fam]
    sigma2 = sigma2[D] if isinstance(sigma2, dict) else sigma2
    rng = np.random.Generator(np.random.PCG64(1000 + 17 * D + list(FAMILIES).index(fam)))
    Xs = [_points(rng, domain, n, D) for n in SIZES]
    ys = [_targets(x) for x in Xs]
    model = pmk.DeviceModel(Xs, ys, dtype=dtype)
    model.fit(th, sigma2)
    refs = []
    for X, y in zip(Xs, ys):
        U = O.kernel_matrix(oth, X) + sigma2 * np.eye(len(y))
        Lref = sla.cholesky(U, lower=True, check_finite=False)
        cref = sla.cho_solve((Lref, True), y, check_finite=False)
        refs.append((U, Lref, cref))
    out = dict(th=th, oth=oth, sigma2=sigma2, Xs=Xs, ys=ys, model=model, refs=refs, kappa=kappa(refs[-1][0]))
    _CACHE[key] = out
    return out


def _residual(U, c, y):
    return np.linalg.norm(U @ c - y) / (np.linalg.norm(U) * np.linalg.norm(c) + np.linalg.norm(y))


def _check_inverted_blocks(model, r, L, tol):
    n = L.shape[0]
    Ni = model.get(r, M.GET_LINV_DIAG)
    for b in range(Ni.shape[0]):
        lo, hi = 32 * b, min(32 * (b + 1), n)
        if lo >= n:
            assert np.array_equal(Ni[b], -np.eye(32))            # identity padding
            continue
        blk = L[lo:hi, lo:hi]
        assert np.abs(-Ni[b][:hi - lo, :hi - lo] @ blk - np.eye(hi - lo)).max() <= tol, (r, b)
        assert np.all(np.triu(Ni[b], 1) == 0)


# ------------------------------------------------------------------------------------ A. fit parity matrix
@pytest.mark.parametrize("fam,D,dtype", CASES, ids=[_ids(c) for c in CASES])
def test_fit_parity_matrix(fam, D, dtype):
    f = _fitted(fam, D, dtype)
    model, kap = f["model"], f["kappa"]
    assert kap * EPS32 <= 1e-3, kap                                # the fp32 bounds below are not vacuous
    assert np.all(model.info() == 0), model.info()
    worst = [0.0] * 4
    for r, (X, y, (U, Lref, cref)) in enumerate(zip(f["Xs"], f["ys"], f["refs"])):
        L, c = model.get(r, M.GET_L), model.get(r, M.GET_C)
        assert np.all(np.triu(L, 1) == 0)
        back = np.linalg.norm(L @ L.T - U) / np.linalg.norm(U)
        res = _residual(U, c, y)
        if dtype == "f64":
            fo = O.fit_patch(f["oth"], X, y, f["sigma2"])
            assert fo["info"] == 0
            assert res <= 1e-13, (r, res)
            assert back <= 1e-14, (r, back)
            assert np.abs(L - fo["L"]).max() <= 1e-8, (r, np.abs(L - fo["L"]).max())
            assert np.linalg.norm(c - fo["c_chol"]) / np.linalg.norm(fo["c_chol"]) <= 1e-6
            _check_inverted_blocks(model, r, L, 1e-9)
        else:
            dL = np.linalg.norm(L - Lref) / np.linalg.norm(Lref)
            dc = np.linalg.norm(c - cref) / np.linalg.norm(cref)
            k = kappa(U)
            assert back <= 200 * EPS32, (r, back / EPS32)
            assert res <= 200 * EPS32, (r, res / EPS32)
            assert dL <= 10 * k * EPS32, (r, dL / (k * EPS32))
            assert dc <= 10 * k * EPS32, (r, dc / (k * EPS32))
            _check_inverted_blocks(model, r, L, 64 * np.sqrt(k) * EPS32)
            worst = [max(a, b) for a, b in zip(worst, (back / EPS32, res / EPS32, dL / (k * EPS32), dc / (k * EPS32)))]
    if dtype == "f32":
        print("%s D=%d f32: kappa %.3g, backward %.1f eps, residual %.1f eps, dL %.3f kappa eps, dc %.3f kappa eps"
              % ((fam, D, kap) + tuple(worst)))


@pytest.mark.parametrize("D", [2, 3])
def test_fused_kernel_matrix_build_is_bit_identical_fp32(monkeypatch, D):
    """the fp32 twin of test_gpu_parity.py::test_fused_kernel_matrix_build_is_bit_identical: Spline34's fused build of
    the tiles below the diagonal (PMK_FUSE_K1=1, the default) against the unfused build + read, on a ragged batch"""
    rng = np.random.default_rng(50 + D)
    sizes = [1, 63, 64, 65, 127, 128, 129, 257, 300, 640, 1000, 1111, 2000]
    Xs = [rng.uniform(-4, 4, (n, D)) for n in sizes]
    ys = [np.sin(x[:, 0]) * np.cos(0.5 * x[:, 1]) for x in Xs]
    th = pmk.Spline34KernelType(1 / 3.0)
    got = []
    for fuse in ("0", "1"):
        monkeypatch.setenv("PMK_FUSE_K1", fuse)
        model, cs, info = pmk.fit_patches(Xs, ys, th, 1e-2, dtype="f32")
        assert np.all(info == 0)
        got.append([(cs[r], model.get(r, M.GET_L), model.get(r, M.GET_LINV_DIAG)) for r in range(len(sizes))])
    for (c0, L0, N0), (c1, L1, N1) in zip(*got):
        assert np.array_equal(c0, c1) and np.array_equal(L0, L1) and np.array_equal(N0, N1)


# ------------------------------------------------------------------------------------ B. fp32 split path
@pytest.mark.parametrize("P,n,D", [(1, 8192, 3), (3, 3000, 2)])
def test_split_path_fp32_matches_batched_path_and_lapack(P, n, D):
    """fp32 twin of test_split_path_matches_batched_path_and_lapack and of the chained-solve test: pmk_test_model_set_split
    modes 0 (batched), 1 (split, automatic solves), 2 (split, block-by-block solves) and 3 (split, chained solves) on
    dtype f32, each against LAPACK in fp64 with kappa-scaled bounds and against one another; ragged sizes included"""
    rng = np.random.Generator(np.random.PCG64(300 + n))
    sizes = [n - 256 * r for r in range(P)]
    Xs = [rng.uniform(0, 1, (m, D)) for m in sizes]
    ys = [np.sin(3 * x[:, 0]) + x[:, -1] ** 2 for x in Xs]
    a, sigma2 = (6.0, 1e-2) if D == 3 else (3.0, 5e-2)
    th, oth = pmk.Spline34KernelType(a), O.kernel(O.SPLINE34, a)
    ctx = pmk.default_context()
    out = {}
    for mode in (0, 1, 2, 3):
        m = pmk.DeviceModel(Xs, ys, dtype="f32")
        assert ctx.L.pmk_test_model_set_split(m.h, mode) == 0
        m.fit(th, sigma2)
        assert np.all(m.info() == 0)
        out[mode] = [(m.get(r, M.GET_L), m.get(r, M.GET_C)) for r in range(P)]
    for r in range(P):
        U = O.kernel_matrix(oth, Xs[r]) + sigma2 * np.eye(sizes[r])
        k = kappa(U)
        assert k * EPS32 <= 1e-3, k
        Lref = sla.cholesky(U, lower=True, check_finite=False)
        cref = sla.cho_solve((Lref, True), ys[r], check_finite=False)
        for mode, (L, c) in ((mo, out[mo][r]) for mo in out):
            back = np.linalg.norm(L @ L.T - U) / np.linalg.norm(U)
            assert back <= 200 * EPS32 and _residual(U, c, ys[r]) <= 200 * EPS32, (mode, back / EPS32)
            assert np.linalg.norm(L - Lref) / np.linalg.norm(Lref) <= 10 * k * EPS32, mode
            assert np.linalg.norm(c - cref) / np.linalg.norm(cref) <= 10 * k * EPS32, mode
        L0, c0 = out[0][r]
        for mode in (1, 2, 3):
            L1, c1 = out[mode][r]
            assert np.linalg.norm(L1 - L0) / np.linalg.norm(L0) <= 10 * k * EPS32, mode
            assert np.linalg.norm(c1 - c0) / np.linalg.norm(c0) <= 10 * k * EPS32, mode
    # the automatic choice: split for few patches of >= 32 tiles, the batched path otherwise
    auto = pmk.DeviceModel(Xs, ys, dtype="f32"); auto.fit(th, sigma2)
    assert np.array_equal(auto.get(0, M.GET_C), out[1 if n == 8192 else 0][0][1])


# ------------------------------------------------------------------------------------ C. predict parity per family
@pytest.mark.parametrize("fam,D,dtype", CASES, ids=[_ids(c) for c in CASES])
def test_predict_strip_parity_matrix(fam, D, dtype):
    """predict_strip_kernel over one region (DeviceModel.queryinner) on the 1-, 129- and 700-point patches of the fit
    matrix, with query counts around the strip's TQ = 256-column boundary (257 and 513 are dealt over two and three
    strips), against queryinner! on the device's own factors"""
    f = _fitted(fam, D, dtype)
    model, th, oth = f["model"], f["th"], f["oth"]
    assert np.all(model.info() == 0)
    rng = np.random.Generator(np.random.PCG64(77 + D))
    domain = FAMILIES[fam][3]
    for r in (SIZES.index(1), SIZES.index(129), SIZES.index(700)):
        X = f["Xs"][r]
        c, L = model.get(r, M.GET_C), model.get(r, M.GET_L)
        k = kappa(f["refs"][r][0])
        for nq in (1, 127, 128, 129, 255, 256, 257, 300, 513):
            Xq = _points(rng, domain, nq, D)
            if nq >= 127:
                Xq[:5] = X[:5]                                     # at training points: the variance sits at the floor
            mu, var = model.queryinner(r, th, Xq)
            mref, vref, mscale, vscale = _queryinner_reference(oth, X, c, L, Xq)
            if dtype == "f64":
                assert np.all(np.abs(mu - mref) <= 1e-9 * np.maximum(1, np.abs(mref))), (r, nq)
                assert np.all(np.abs(var - vref) <= 1e-9 + 1e-5 * vref), (r, nq, np.abs(var - vref).max())
            else:
                assert np.all(np.abs(mu - mref) <= 50 * np.sqrt(k) * EPS32 * (mscale + 1)), (r, nq)
                # + 1: fp32 kernel values carry absolute errors ~ eps32 times their terms, which for the bridges are
                # ~ 1 where k(x, x) = x (1 - x) is not (min(x, z) - x z cancels near the ends of [0, 1])
                assert np.all(np.abs(var - vref) <= 50 * k * EPS32 * (vscale + 1)), (r, nq, np.abs(var - vref).max())
            for j in (0, nq - 1):                                   # and queryinner! of the oracle itself
                om, ov = O.queryinner(oth, X, c, L, Xq[j])
                assert abs(om - mref[j]) <= 1e-12 * max(1, abs(om)) + 1e-14 * mscale[j]
                assert abs(ov - vref[j]) <= 1e-12 * max(1, vscale[j])


def _mixture_case(seed, N=2400, levels=4, eps=0.3):
    rng = np.random.Generator(np.random.PCG64(seed))
    X = np.stack([rng.uniform(-5, 5, N), rng.uniform(-10, 10, N)], 1)
    y = np.sin(X[:, 0]) * np.cos(0.3 * X[:, 1])
    Xq = np.stack([rng.uniform(-5, 5, 700), rng.uniform(-10, 10, 700)], 1)
    root, _, _ = pmk.setuppartition(X, levels)
    X_set, X_set_inds, _, _ = pmk.organizetrainingsets(root, levels, X, eps)
    return X, [y[i] for i in X_set_inds], Xq, root, X_set


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_mixture_with_generic_fit_and_weight_kernels(dtype):
    """fitmixtureGP! + querymixtureGP! with a Spline32 fit kernel and a Gaussian weight kernel (neither is the Spline34
    specialisation): integer outputs identical to the oracle in both dtypes; values against O.query_mixture on the
    oracle's fp64 fits (fp64) or against queryinner! on the device's own fp32 factors, blended with the device's weights
    and the weights themselves against the Gaussian profile (fp32)"""
    X, ys, Xq, root, X_set = _mixture_case(61)
    levels, radius, delta, sigma2 = 4, 0.5, 1e-5, 0.05
    th, oth = pmk.Spline32KernelType(0.5), O.kernel(O.SPLINE32, 0.5)
    wth, owth = pmk.GaussianKernel1DType(4.0), O.kernel(O.GAUSSIAN, 4.0)
    m = pmk.DeviceModel(X_set, ys, dtype=dtype); m.fit(th, sigma2); m.set_bsp(root, 0)
    assert np.all(m.info() == 0)
    q = pmk.DeviceQuery(m, Xq); q.plan(radius, delta); q.items(th); q.mix(wth)
    Yq, Vq = q.fetch()
    dbg = q.debug()
    ob = O.BSP(X, levels)
    fits = [O.fit_patch(oth, xs, yy, sigma2) for xs, yy in zip(X_set, ys)]
    oY, oV, ohome, ooff, oreg, ots = O.query_mixture(ob, oth, owth, X_set, [f["c_lu"] for f in fits], [f["L"] for f in fits],
                                                     Xq, radius, delta, debug=True, nthreads=8)
    off = dbg["item_offsets"]
    assert np.array_equal(dbg["home"], ohome)
    assert np.array_equal(np.diff(off) - 1, np.diff(ooff))
    nb = np.ones(off[-1], bool); nb[off[1:] - 1] = False            # items without the home item (last per query)
    assert np.array_equal(dbg["item_region"][nb], oreg) and np.array_equal(dbg["item_t"][nb], ots)
    assert np.array_equal(dbg["item_region"][~nb], ohome)
    wref = np.array([1.0 if not b else O.profile(owth, abs(t)) for b, t in zip(nb, dbg["item_t"])])
    assert np.abs(dbg["item_w"] - wref).max() <= 1e-15
    if dtype == "f64":
        assert np.all(np.abs(Yq - oY) <= 1e-7 * np.maximum(1, np.abs(oY))), np.abs(Yq - oY).max()
        assert np.all(np.abs(Vq - oV) <= 1e-9 + 1e-5 * oV)
        return
    u_ref, v_ref = np.empty(off[-1]), np.empty(off[-1])
    ks = {}
    for r in np.unique(dbg["item_region"]):
        idx = np.nonzero(dbg["item_region"] == r)[0]
        qj = np.searchsorted(off, idx, side="right") - 1
        c, L = m.get(int(r), M.GET_C), m.get(int(r), M.GET_L)
        ks[r] = kappa(O.kernel_matrix(oth, X_set[r]) + sigma2 * np.eye(len(X_set[r])))
        assert ks[r] * EPS32 <= 1e-3
        mu, var, msc, vsc = _queryinner_reference(oth, X_set[r], c, L, Xq[qj])
        u_ref[idx], v_ref[idx] = mu, var
        assert np.all(np.abs(dbg["item_u"][idx] - mu) <= 50 * np.sqrt(ks[r]) * EPS32 * (msc + 1))
        assert np.all(np.abs(dbg["item_v"][idx] - var) <= 50 * ks[r] * EPS32 * vsc)
    Y, V = _blend_reference(dbg, u_ref, v_ref)
    kmax = max(ks.values())
    assert np.all(np.abs(Yq - Y) <= 50 * kmax * EPS32 * np.maximum(1, np.abs(Y)))
    assert np.all(np.abs(Vq - V) <= 50 * kmax * EPS32 * (V + 1e-3))
    # and the fp32 blend near the oracle's fp64 mixture (forward error of the fit: kappa-scaled)
    assert np.abs(Yq - oY).max() <= 50 * kmax * EPS32 * max(1, np.abs(oY).max())


def _dpp_kernel():
    canon = pmk.Spline34KernelType(1 / 4.0)
    wm = lambda x: 0.8 * np.sin(0.7 * x[0]) + 0.1 * x[1]      # noqa: E731
    return pmk.AdaptiveKernelDPPType(canon, wm), O.kernel(O.SPLINE34, 1 / 4.0)


def _dpp_model(X_set, ys, th, sigma2, root, dtype):
    m = pmk.DeviceModel([M.kernel_points(th, x) for x in X_set], ys, dtype=dtype)
    m.set_diag([th.diag_addend(x) for x in X_set])
    m.fit(th, sigma2)
    assert np.all(m.info() == 0)
    m.set_bsp(root, 0)
    return m


def _dpp_query(m, th, Xq):
    q = pmk.DeviceQuery(m, M.kernel_points(th, Xq))
    q.set_diag(th.diag_addend(Xq))                           # as querymixtureGP_ sets it
    return q


def test_dpp_mixture_fp32_against_oracle_with_qdiag():
    """fp32 twin of the DPP part of test_dpp_kernels_and_warp_kernels_in_the_mixture_path: the per-query addend in the fp32
    strip kernel, item by item against queryinner! (qdiag) on the device's own fp32 factors"""
    X, ys, Xq, root, X_set = _mixture_case(53)
    levels, radius, delta, sigma2 = 4, 0.5, 1e-5, 5e-2
    th, ocm = _dpp_kernel()
    wth = pmk.Spline34KernelType(1 / radius)
    m = _dpp_model(X_set, ys, th, sigma2, root, "f32")
    q = _dpp_query(m, th, Xq); q.plan(radius, delta); q.items(th); q.mix(wth)
    Yq, Vq = q.fetch()
    dbg = q.debug()
    ob = O.BSP(X, levels)
    off = dbg["item_offsets"]
    for j in range(0, len(Xq), 7):
        h = ob.findpartition(Xq[j])
        reg, _, _, _ = ob.neighbours(Xq[j], radius, delta, h)
        assert dbg["home"][j] == h and np.array_equal(dbg["item_region"][off[j]:off[j + 1]][:-1], reg)
    qd = th.diag_addend(Xq)
    assert qd.max() > 0.1                                      # the addend is not negligible against k(x, x) = 1
    u_ref, v_ref = np.empty(off[-1]), np.empty(off[-1])
    kmax = 0.0
    for r in np.unique(dbg["item_region"]):
        idx = np.nonzero(dbg["item_region"] == r)[0]
        qj = np.searchsorted(off, idx, side="right") - 1
        Xa = th.augment(X_set[r])
        U = O.kernel_matrix(ocm, Xa) + np.diag(th.diag_addend(X_set[r])) + sigma2 * np.eye(len(Xa))
        k = kappa(U)
        assert k * EPS32 <= 1e-3
        kmax = max(kmax, k)
        c, L = m.get(int(r), M.GET_C), m.get(int(r), M.GET_L)
        assert np.linalg.norm(L @ L.T - U) / np.linalg.norm(U) <= 200 * EPS32
        mu, var, msc, vsc = _queryinner_reference(ocm, Xa, c, L, th.augment(Xq[qj]), qdiag=qd[qj])
        u_ref[idx], v_ref[idx] = mu, var
        assert np.all(np.abs(dbg["item_u"][idx] - mu) <= 50 * np.sqrt(k) * EPS32 * (msc + 1))
        assert np.all(np.abs(dbg["item_v"][idx] - var) <= 50 * k * EPS32 * vsc), np.abs(dbg["item_v"][idx] - var).max()
        for i, j in zip(idx[:2], qj[:2]):                     # spot checks against the oracle's queryinner itself
            om, ov = O.queryinner(ocm, Xa, c, L, th.augment(Xq[j][None, :])[0], qdiag=qd[j])
            assert abs(ov - v_ref[i]) <= 1e-12 and abs(om - u_ref[i]) <= 1e-12 * max(1, abs(om)) + 1e-14 * msc.max()
    Y, V = _blend_reference(dbg, u_ref, v_ref)
    assert np.all(np.abs(Yq - Y) <= 50 * kmax * EPS32 * np.maximum(1, np.abs(Y)))
    assert np.all(np.abs(Vq - V) <= 50 * kmax * EPS32 * (V + 1e-3))


# ------------------------------------------------------------------------------------ D. DPP kernels through the exchange
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_dpp_kernel_through_the_exchange_forms_loopback(dtype):
    """a one-rank communicator with the exchange forced on (include/pmk_test.h): the per-query addend of a DPP kernel must
    travel with the requests and be added on the owner, so that pmk_query_predict_sharded and _allgather reproduce the
    single-model Yq / Vq bit for bit; then a non-DPP predict on the same communicator (whose remote query object is
    reused) must again equal its single-model result"""
    X, ys, Xq, root, X_set = _mixture_case(71)
    radius, delta, sigma2 = 0.5, 1e-5, 5e-2
    th, _ = _dpp_kernel()
    wth = pmk.Spline34KernelType(1 / radius)
    ctx = pmk.default_context()
    m = _dpp_model(X_set, ys, th, sigma2, root, dtype)
    q = _dpp_query(m, th, Xq); total = q.plan(radius, delta); q.items(th); q.mix(wth)
    Y0, V0 = q.fetch()
    comm = pmk.Comm(ctx, 0, 1, pmk.comm_unique_id())
    assert ctx.L.pmk_test_comm_force_exchange(comm.h, 1) == 0
    for _ in range(2):
        q2 = _dpp_query(m, th, Xq)
        assert q2.predict_sharded(comm, th, wth, radius, delta) == total
        Y1, V1 = q2.fetch()
        bad = np.nonzero(V1 != V0)[0]
        assert len(bad) == 0, "sharded: %d of %d Vq differ, e.g. %r vs %r" % (len(bad), len(V0), V1[bad[:3]], V0[bad[:3]])
        assert np.array_equal(Y1, Y0)
        q3 = _dpp_query(m, th, Xq)
        assert q3.predict_allgather(comm, th, wth, radius, delta) == total
        Y2, V2 = q3.fetch()
        assert np.array_equal(Y2, Y0) and np.array_equal(V2, V0)
    sent, recv = comm.last_bytes()
    assert sent == 0 and recv == 0
    # the same model and communicator (the same remote query object) with a query that carries no addend: nothing stale
    qn = pmk.DeviceQuery(m, M.kernel_points(th, Xq)); qn.plan(radius, delta); qn.items(th); qn.mix(wth)
    Yn, Vn = qn.fetch()
    assert not np.array_equal(Vn, V0)                          # the addend matters here
    for _ in range(2):
        qs = pmk.DeviceQuery(m, M.kernel_points(th, Xq))
        qs.predict_sharded(comm, th, wth, radius, delta)
        Ys, Vs = qs.fetch()
        assert np.array_equal(Ys, Yn) and np.array_equal(Vs, Vn)
    # a plain (non-DPP) kernel on another model, on the same communicator
    ths = pmk.Spline34KernelType(1 / 4.0)
    mp = pmk.DeviceModel(X_set, ys, dtype=dtype); mp.fit(ths, sigma2); mp.set_bsp(root, 0)
    qp = pmk.DeviceQuery(mp, Xq); qp.plan(radius, delta); qp.items(ths); qp.mix(wth)
    Yp, Vp = qp.fetch()
    for _ in range(2):
        qs = pmk.DeviceQuery(mp, Xq)
        qs.predict_sharded(comm, ths, wth, radius, delta)
        Ys, Vs = qs.fetch()
        assert np.array_equal(Ys, Yp) and np.array_equal(Vs, Vp)
    # and the DPP model once more after the plain one
    q4 = _dpp_query(m, th, Xq)
    q4.predict_sharded(comm, th, wth, radius, delta)
    Y4, V4 = q4.fetch()
    assert np.array_equal(Y4, Y0) and np.array_equal(V4, V0)
    comm.close()


# ------------------------------------------------------------------------------------ E. headline batch, every patch
@pytest.mark.timeout(1200)
def test_config_C_every_patch_against_lapack():
    """BASELINE config C (headline): 256 patches x 2000 points, fp64 -- EVERY patch against LAPACK on the oracle's kernel
    matrix: backward error, residual, and the factor element by element.  The host work (~4 TFLOP of matmul) runs in a
    thread pool while the next patches come off the device."""
    from concurrent.futures import ThreadPoolExecutor
    import time
    t0 = time.time()
    N, levels = 512000, 9
    rng = np.random.Generator(np.random.PCG64(25))
    X = np.stack([rng.uniform(-5, 5, N), rng.uniform(-10, 10, N)], 1)
    A = np.array([[1.0, 0.4], [0.4, 1.0]]) * 0.1
    q = np.einsum("ni,ij,nj->n", X, A, X)
    y = np.sinc((q / 3.2) ** 2) * (np.linalg.norm(X, axis=1) / 4) ** 3
    th, oth, sigma2 = pmk.Spline34KernelType(1 / 15), O.kernel(O.SPLINE34, 1 / 15), 1e-5
    root, X_parts, X_parts_inds = pmk.setuppartition(X, levels)
    assert [len(p) for p in X_parts] == [2000] * 256
    ys = [y[i] for i in X_parts_inds]
    model = pmk.DeviceModel(X_parts, ys)
    model.fit(th, sigma2)
    assert np.all(model.info() == 0)

    def check(r, L, c):
        U = O.kernel_matrix(oth, X_parts[r])
        U[np.diag_indices(2000)] += sigma2
        back = np.linalg.norm(L @ L.T - U) / np.linalg.norm(U)
        res = _residual(U, c, ys[r])
        dL = np.abs(L - sla.cholesky(U, lower=True, check_finite=False)).max()
        return r, back, res, dL

    out = []
    with ThreadPoolExecutor(4) as ex:
        for r0 in range(0, 256, 16):                       # bounded host memory: 16 patches in flight
            futs = [ex.submit(check, r, model.get(r, M.GET_L), model.get(r, M.GET_C)) for r in range(r0, r0 + 16)]
            out += [f.result() for f in futs]
    worst = [max(o[k] for o in out) for k in (1, 2, 3)]
    print("config C, all 256 patches in %.1f s: backward %.2e, residual %.2e, max |L - L_lapack| %.2e"
          % ((time.time() - t0,) + tuple(worst)))
    for r, back, res, dL in out:
        assert back <= 1e-14 and res <= 1e-13 and dL <= 1e-8, (r, back, res, dL)

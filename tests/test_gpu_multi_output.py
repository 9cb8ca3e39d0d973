"""Multi-output targets on the GPU: R target columns per patch that share one factor (pmk_model_set_targets_multi,
pmk_model_solve_multi, pmk_query_items_multi / _mix_multi / _fetch_multi, pmk_predict_mixture_multi).

References: the CPU oracle run once per column (O.fit_patch, O.query_mixture) and LAPACK (scipy.linalg) in fp64.  fp32
is judged as in tests/test_gpu_family_parity.py: residuals in multiples of eps32 and forward errors scaled by
kappa(U) eps32, with kappa(U) eps32 <= 1e-3 asserted so that those bounds are not vacuous.
"""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg as sla

import patchmixturekriging_amd as pmk
from patchmixturekriging_amd import _lib
from patchmixturekriging_amd import mixture as M
from oracle import oracle as O

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
SIZES = [1, 63, 65, 127, 129, 257, 700]         # across the 64- and 128-row tile edges
SIGMA2 = 1e-5
# the weight tests compare two solves from one factor at 1e-12: kappa(U) <= 3.4e4 for these patches at 1e-3 (3.3e6 at 1e-5,
# where two correct summation orders already differ by ~1e-12)
SIGMA2_W = 1e-3
A = 1 / 3.0


def _targets(X, R, shift=0.0):
    cols = [np.sin((0.5 + 0.3 * j) * X[:, 0] + shift) * np.cos((0.2 + 0.1 * j) * X[:, -1]) + 0.1 * j for j in range(R)]
    return np.stack(cols, 1)


def _U(oth, X, sigma2):
    return O.kernel_matrix(oth, X) + sigma2 * np.eye(len(X))


def kappa(U):
    ev = np.linalg.eigvalsh(U)
    assert ev[0] > 0
    return float(ev[-1] / ev[0])


def _ragged(seed, D=2):
    rng = np.random.default_rng(seed)
    return [rng.uniform(-4, 4, (n, D)) for n in SIZES]


def _fit_multi(Xs, Ys, th, sigma2, dtype="f64"):
    model = M.DeviceModel(Xs, [y[:, 0].copy() for y in Ys], dtype=dtype)
    model.fit(th, sigma2)
    assert np.all(model.info() == 0)
    model.set_targets_multi(Ys)
    model.solve_multi()
    return model, model.weights_multi()


def _rel_residual(U, Cm, Y):
    return np.linalg.norm(U @ Cm - Y) / (np.linalg.norm(U) * np.linalg.norm(Cm))


# ------------------------------------------------------------------------------------ 1. weights
@pytest.mark.parametrize("R", [1, 3, 16])
def test_weights_vs_oracle_per_column(R):
    Xs = _ragged(31)
    Ys = [_targets(X, R) for X in Xs]
    th, oth = pmk.Spline34KernelType(A), O.kernel(O.SPLINE34, A)
    model, Cs = _fit_multi(Xs, Ys, th, SIGMA2_W)
    for r, (X, Y, Cm) in enumerate(zip(Xs, Ys, Cs)):
        assert Cm.shape == (len(X), R)
        U = _U(oth, X, SIGMA2_W)
        assert _rel_residual(U, Cm, Y) <= 1e-14, (r, _rel_residual(U, Cm, Y))
        for j in range(R):
            f = O.fit_patch(oth, X, Y[:, j], SIGMA2_W)
            assert f["info"] == 0
            assert np.linalg.norm(Cm[:, j] - f["c_lu"]) / np.linalg.norm(f["c_lu"]) <= 1e-6, (r, j)
        # column 0 is the single-output fit's c (same factor, a different summation order)
        c0 = model.get(r, M.GET_C)
        assert np.linalg.norm(Cm[:, 0] - c0) <= 1e-12 * np.linalg.norm(c0), r


# ------------------------------------------------------------------------------------ 2. reuse of the factor
def test_new_targets_reuse_the_factor():
    Xs = _ragged(32)
    th, oth = pmk.Spline34KernelType(A), O.kernel(O.SPLINE34, A)
    model, C1 = _fit_multi(Xs, [_targets(X, 4) for X in Xs], th, SIGMA2_W)
    Ls = [model.get(r, M.GET_L) for r in range(len(Xs))]
    Y2 = [_targets(X, 5, shift=1.3) for X in Xs]
    model.set_targets_multi(Y2)
    model.solve_multi()
    C2 = model.weights_multi()
    for r, X in enumerate(Xs):
        assert np.array_equal(model.get(r, M.GET_L), Ls[r])            # no refactorisation
        U = _U(oth, X, SIGMA2_W)
        assert _rel_residual(U, C2[r], Y2[r]) <= 1e-14
        ref = sla.solve(U, Y2[r], assume_a="pos")
        assert np.linalg.norm(C2[r] - ref) <= 1e-6 * np.linalg.norm(ref)
    # the same from a model rebuilt from host factors (checkpoint / resume)
    cs = model.weights()
    loaded = M.DeviceModel.from_factors(Xs, cs, Ls)
    Lb = [loaded.get(r, M.GET_L) for r in range(len(Xs))]
    loaded.set_targets_multi(Y2)
    loaded.solve_multi()
    C3 = loaded.weights_multi()
    for r, X in enumerate(Xs):
        assert np.array_equal(loaded.get(r, M.GET_L), Lb[r])
        assert np.linalg.norm(C3[r] - C2[r]) <= 1e-12 * np.linalg.norm(C2[r]), r


# ------------------------------------------------------------------------------------ 3. mixture
def _mixgp_case(N, levels, eps, radius, nq, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    X = np.stack([rng.uniform(-5, 5, N), rng.uniform(-10, 10, N)], 1)
    Xq = np.stack([rng.uniform(-5, 5, nq), rng.uniform(-10, 10, nq)], 1)
    root, _, _ = pmk.setuppartition(X, levels)
    X_set, X_set_inds, _, _ = pmk.organizetrainingsets(root, levels, X, eps)
    return X, Xq, root, X_set, X_set_inds


def _oracle_mixture(X, levels, oth, owth, X_set, ys, Xq, radius, delta, sigma2):
    ob = O.BSP(X, levels)
    fits = [O.fit_patch(oth, xs, y, sigma2) for xs, y in zip(X_set, ys)]
    oY, oV = O.query_mixture(ob, oth, owth, X_set, [f["c_lu"] for f in fits], [f["L"] for f in fits], Xq, radius, delta,
                             nthreads=8)
    return oY, oV


def test_mixture_vs_oracle_per_column():
    levels, eps, a, radius, delta, R = 4, 0.6, 1 / 4.0, 0.5, 1e-5, 4      # the test_mixture_small_vs_oracle workload
    X, Xq, root, X_set, X_set_inds = _mixgp_case(1500, levels, eps, radius, 700, 25)
    Yall = _targets(X, R)
    th, wth = pmk.Spline34KernelType(a), pmk.Spline34KernelType(1 / radius)
    oth, owth = O.kernel(O.SPLINE34, a), O.kernel(O.SPLINE34, 1 / radius)
    eta = pmk.MixtureGPType(X_set, pmk.fetchhyperplanes(root))
    pmk.fitmixtureGP_multi_(eta, [Yall[i] for i in X_set_inds], th, SIGMA2)
    assert len(eta.C_set) == len(X_set) and eta.C_set[0].shape[1] == R
    Yq, Vq = pmk.querymixtureGP_multi(Xq, eta, root, levels, radius, delta, th, SIGMA2, wth)
    assert Yq.shape == (len(Xq), R)
    for j in range(R):
        oY, oV = _oracle_mixture(X, levels, oth, owth, X_set, [Yall[i, j] for i in X_set_inds], Xq, radius, delta, SIGMA2)
        assert np.all(np.abs(Yq[:, j] - oY) <= 1e-7 * np.maximum(1, np.abs(oY))), (j, np.abs(Yq[:, j] - oY).max())
        assert np.all(np.abs(Vq - oV) <= 1e-9 + 1e-5 * oV)
    # Vq is the single-output predictor's, bit for bit
    Y1, V1, _ = pmk.querymixtureGP(Xq, eta, root, levels, radius, delta, th, SIGMA2, wth)
    assert np.array_equal(Vq, V1)
    # mean only: no triangular solve, the same means
    Ym, Vm = pmk.querymixtureGP_multi(Xq, eta, root, levels, radius, delta, th, SIGMA2, wth, variance=False)
    assert Vm is None
    assert np.all(np.abs(Ym - Yq) <= 1e-12 * np.maximum(1, np.abs(Yq)))
    # the one-shot entry point agrees with the staged one
    L = pmk.lib()
    Y1s = np.empty((len(Xq), R), order="F")
    d, w = th.desc(), wth.desc()
    Xc = np.ascontiguousarray(Xq)
    _lib.check(L.pmk_predict_mixture_multi(eta._model.h, C.byref(d), C.byref(w), len(Xq), M._d(Xc), radius, delta,
                                           M._d(Y1s), len(Xq), None), "pmk_predict_mixture_multi")
    assert np.array_equal(Y1s, Ym)


# ------------------------------------------------------------------------------------ 4. fp32
@pytest.mark.parametrize("R", [1, 3, 16])
def test_weights_f32(R):
    Xs = _ragged(33)
    Ys = [_targets(X, R) for X in Xs]
    sigma2 = 0.05
    th, oth = pmk.Spline34KernelType(1.0), O.kernel(O.SPLINE34, 1.0)
    model, Cs = _fit_multi(Xs, Ys, th, sigma2, dtype="f32")
    for r, (X, Y, Cm) in enumerate(zip(Xs, Ys, Cs)):
        U = _U(oth, X, sigma2)
        k = kappa(U)
        assert k * EPS32 <= 1e-3, k
        assert _rel_residual(U, Cm, Y) <= 200 * EPS32, (r, _rel_residual(U, Cm, Y) / EPS32)
        ref = sla.solve(U, Y, assume_a="pos")
        for j in range(R):
            dc = np.linalg.norm(Cm[:, j] - ref[:, j]) / np.linalg.norm(ref[:, j])
            assert dc <= 10 * k * EPS32, (r, j, dc / (k * EPS32))


def test_mixture_f32():
    levels, eps, a, radius, delta, R, sigma2 = 4, 0.6, 1.0, 0.5, 1e-5, 4, 0.05
    X, Xq, root, X_set, X_set_inds = _mixgp_case(1500, levels, eps, radius, 500, 26)
    Yall = _targets(X, R)
    th, wth = pmk.Spline34KernelType(a), pmk.Spline34KernelType(1 / radius)
    oth, owth = O.kernel(O.SPLINE34, a), O.kernel(O.SPLINE34, 1 / radius)
    kmax = 0.0
    for xs in X_set:
        k = kappa(_U(oth, xs, sigma2))
        assert k * EPS32 <= 1e-3
        kmax = max(kmax, k)
    Ys = [Yall[i] for i in X_set_inds]
    model, _ = _fit_multi(X_set, Ys, th, sigma2, dtype="f32")
    model.set_bsp(root, 0)
    q = M.DeviceQuery(model, Xq)
    q.plan(radius, delta)
    q.items_multi(th, True)
    q.mix_multi(wth)
    Yq, Vq = q.fetch_multi(R)
    # the single-output fp32 predictor on the same model and plan: the same variance, bit for bit
    q.items(th)
    q.mix(wth)
    _, V1 = q.fetch()
    assert np.array_equal(Vq, V1)
    for j in range(R):
        oY, oV = _oracle_mixture(X, levels, oth, owth, X_set, [y[:, j] for y in Ys], Xq, radius, delta, sigma2)
        assert np.abs(Yq[:, j] - oY).max() <= 50 * kmax * EPS32 * max(1, np.abs(oY).max()), j
        assert np.all(np.abs(Vq - oV) <= 50 * kmax * EPS32 * (oV + 1e-3))


# ------------------------------------------------------------------------------------ 5. split mode, other families
def test_split_mode_solve():
    rng = np.random.default_rng(35)
    X = rng.uniform(-8, 8, (4096, 2))
    Y = _targets(X, 3)
    th, oth = pmk.Spline34KernelType(1 / 3.0), O.kernel(O.SPLINE34, 1 / 3.0)
    model = M.DeviceModel([X], [Y[:, 0].copy()])
    model.fit(th, SIGMA2)
    assert np.all(model.info() == 0)
    model.set_targets_multi([Y])
    model.solve_multi()
    Cm = model.weights_multi()[0]
    U = _U(oth, X, SIGMA2)
    assert _rel_residual(U, Cm, Y) <= 1e-14
    ref = sla.solve(U, Y, assume_a="pos")
    assert np.linalg.norm(Cm - ref) <= 1e-6 * np.linalg.norm(ref)


@pytest.mark.parametrize("D", [1, 3])
def test_items_means_other_family(D):
    rng = np.random.Generator(np.random.PCG64(40 + D))
    N, levels, eps, radius, delta, R, sigma2 = 800, 3, 0.3, 0.3, 1e-5, 3, 0.05
    X = rng.uniform(-2, 2, (N, D))
    Xq = rng.uniform(-2, 2, (300, D))
    root, _, _ = pmk.setuppartition(X, levels)
    X_set, X_set_inds, _, _ = pmk.organizetrainingsets(root, levels, X, eps)
    Yall = _targets(X, R)
    th, oth = pmk.GaussianKernel1DType(4.0), O.kernel(O.GAUSSIAN, 4.0)
    wth, owth = pmk.Spline34KernelType(1 / radius), O.kernel(O.SPLINE34, 1 / radius)
    eta = pmk.MixtureGPType(X_set, pmk.fetchhyperplanes(root))
    pmk.fitmixtureGP_multi_(eta, [Yall[i] for i in X_set_inds], th, sigma2)
    Yq, Vq = pmk.querymixtureGP_multi(Xq, eta, root, levels, radius, delta, th, sigma2, wth, variance=False)
    assert Vq is None
    for j in range(R):
        oY, _ = _oracle_mixture(X, levels, oth, owth, X_set, [Yall[i, j] for i in X_set_inds], Xq, radius, delta, sigma2)
        assert np.all(np.abs(Yq[:, j] - oY) <= 1e-7 * np.maximum(1, np.abs(oY))), (j, np.abs(Yq[:, j] - oY).max())


# ------------------------------------------------------------------------------------ 6. errors
def _raw_targets(L, model, R, Ys):
    PA = M._dp * model.P
    ld = np.array([y.shape[0] for y in Ys], dtype=np.int64)
    return L.pmk_model_set_targets_multi(model.h, R, PA(*[M._d(y) for y in Ys]), M._i(ld))


def test_errors():
    L = pmk.lib()
    Xs = _ragged(36)[:3]
    th = pmk.Spline34KernelType(A)
    model = M.DeviceModel(Xs, [X[:, 0].copy() for X in Xs])
    model.fit(th, SIGMA2)
    Ys = [np.asfortranarray(_targets(X, 16)) for X in Xs]
    for R in (0, 17):
        assert _raw_targets(L, model, R, Ys) < 0
        assert b"R=%d" % R in L.pmk_last_error()
    assert L.pmk_model_solve_multi(model.h) < 0                       # no targets yet
    assert b"targets" in L.pmk_last_error()
    # a model that holds only part of the leaves
    rng = np.random.default_rng(37)
    X = rng.uniform(-4, 4, (400, 2))
    root, X_parts, _ = pmk.setuppartition(X, 3)                        # 4 leaves
    part = M.DeviceModel(X_parts[:2], [x[:, 0].copy() for x in X_parts[:2]])
    part.fit(th, SIGMA2)
    part.set_targets_multi([_targets(x, 2) for x in X_parts[:2]])
    part.solve_multi()
    part.set_bsp(root, 0)
    q = M.DeviceQuery(part, X[:10])
    q.plan(0.3, 1e-5)
    with pytest.raises(pmk.PmkError, match="holds 2 of 4 leaves"):
        q.items_multi(th, False)
    # Vq that was never computed
    full = M.DeviceModel(X_parts, [x[:, 0].copy() for x in X_parts])
    full.fit(th, SIGMA2)
    full.set_targets_multi([_targets(x, 2) for x in X_parts])
    full.solve_multi()
    full.set_bsp(root, 0)
    q = M.DeviceQuery(full, X[:10])
    q.plan(0.3, 1e-5)
    q.items_multi(th, False)
    q.mix_multi(pmk.Spline34KernelType(1 / 0.3))
    Yq, Vq = np.empty((10, 2), order="F"), np.empty(10)
    assert L.pmk_query_fetch_multi(q.h, M._d(Yq), 10, M._d(Vq)) < 0
    assert b"Vq was not computed" in L.pmk_last_error()
    assert L.pmk_query_fetch_multi(q.h, M._d(Yq), 10, None) == 0

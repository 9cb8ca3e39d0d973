"""Model selection from the resident factor on the GPU: pmk_model_evidence(_multi), pmk_model_loo, pmk_model_get_loo(_multi)
and the front-end functions over them.

References: numpy.longdouble (tests/_loo_refs.py) on the device's own factor (which isolates the leave-one-out kernel from
the factorisation's error) and on the oracle's kernel matrix (end to end); LAPACK trtri in double where long double would
take too long.  u = 2^-53 for fp64 models, 2^-24 for fp32 models; cond_2 per rung from the conditioning fixtures.

d = diag((L L^T)^-1) is read back as 1 / var (pmk_model_get_loo returns var = 1 / d, one IEEE division in double): the two
roundings of 2^-53 this adds are far inside every bound below (the tightest is n u with n >= 128).

Run with -s to see every measured ratio (profiles/model_selection_accuracy.json records one such run).
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import patchmixturekriging_amd as pmk
from patchmixturekriging_amd import _lib
from patchmixturekriging_amd import mixture as M
from oracle import oracle as O

import _loo_refs as LR

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LD = LR.LD
_dp = C.POINTER(C.c_double)


def _record(**kw):
    """every figure is printed before it is asserted; tools/model_selection_accuracy.py collects these lines"""
    print("measured " + json.dumps(kw))


_FIX = {}


def _fixture(name):
    if name not in _FIX:
        _FIX[name] = np.load(os.path.join(GOLDEN, "conditioning_%s.npz" % name))
    return _FIX[name]


# (problem, precision, rung): p1 at the four fp64 and the three fp32 rungs, p2 at sigma2 = 1e-4 and 1e-10
CASES = [("p1", "f64", k) for k in range(4)] + [("p1", "f32", k) for k in range(3)] + [("p2", "f64", 0), ("p2", "f64", 3)]
CASE_IDS = ["%s-%s-%d" % c for c in CASES]


def _case(name, dtype, k):
    g = _fixture(name)
    sigma2 = float(g["sigma2_" + dtype][k])
    cond = float(g["cond_" + dtype][k])
    if name == "p2":
        assert sigma2 == (1e-4, None, None, 1e-10)[k]
    return g, sigma2, cond


def _fit_batch(g, sigma2, dtype):
    """the problem's patch batched with its 257-point companion, so that the batch is ragged"""
    th = pmk.Spline34KernelType(float(g["theta"]))
    model = M.DeviceModel([g["X"], g["Xc"]], [g["y"], g["yc"]], dtype=dtype)
    model.fit(th, sigma2)
    assert np.all(model.info() == 0)
    return model


_K = {}


def _oracle_K(name, which="X"):
    if (name, which) not in _K:
        g = _fixture(name)
        _K[(name, which)] = O.kernel_matrix(O.kernel(O.SPLINE34, float(g["theta"])), g[which])
    return _K[(name, which)]


def _d_of(var):
    return 1.0 / np.asarray(var)


def _rel_err(d, dstar):
    return float((np.abs(d.astype(LD) - dstar) / dstar).max())


def _device_y(y, dtype):
    """the targets as the device holds them"""
    return y.astype(np.float32).astype(np.float64) if dtype == "f32" else y


# ------------------------------------------------------------------------------------ 4. the kernel against the device's factor
@pytest.mark.parametrize("name, dtype, k", CASES, ids=CASE_IDS)
def test_d_against_the_devices_own_factor(name, dtype, k):
    """max_i |d_i - d*_i| / d*_i <= n u, d* = squared column norms of L^-1 in long double for the L the device holds:
    substitution is componentwise backward stable with constant gamma_n ~ n u.
    Measured on an MI355X (profiles/model_selection_accuracy.json): 0.019 .. 0.23 of n u in fp64, 0.020 .. 0.042 in fp32."""
    g, sigma2, _ = _case(name, dtype, k)
    u = LR.unit_roundoff(dtype)
    model = _fit_batch(g, sigma2, dtype)
    model.loo()
    _, var = model.loo_values()
    for r in range(2):
        n = int(model.n[r])
        dstar = LR.linv_colnorms_ld(model.get(r, M.GET_L))
        ratio = _rel_err(_d_of(var[r]), dstar) / (n * u)
        _record(test="d_vs_device_factor", problem=name, dtype=dtype, sigma2=sigma2, patch=r, n=n, ratio_to_n_u=ratio)
        assert ratio <= 1.0, (name, dtype, sigma2, r, ratio)


# ------------------------------------------------------------------------------------ 5. end to end against long double
@pytest.mark.parametrize("name, dtype, k", CASES, ids=CASE_IDS)
def test_d_and_residuals_end_to_end(name, dtype, k):
    """reference on the oracle's kernel matrix: max_i |d_i - d*_i| / d*_i <= cond_2 u and
    max_i |res_i - res*_i| <= cond_2 u max |y|.
    Measured on an MI355X: d at most 0.056 (fp64) and 0.025 (fp32) of its bound, the residuals at most 0.010 and 0.18."""
    g, sigma2, cond = _case(name, dtype, k)
    u = LR.unit_roundoff(dtype)
    model = _fit_batch(g, sigma2, dtype)
    model.loo()
    res, var = model.loo_values()
    ref = LR.loo_reference(_oracle_K(name), sigma2, g["y"])
    rd = _rel_err(_d_of(var[0]), ref["d"]) / (cond * u)
    rr = float(np.abs(res[0].astype(LD) - ref["res"]).max()) / (cond * u * np.abs(g["y"]).max())
    _record(test="end_to_end", problem=name, dtype=dtype, sigma2=sigma2, cond2=cond, d_ratio_to_cond_u=rd,
            res_ratio_to_cond_u_maxy=rr)
    assert rd <= 1.0, (name, dtype, sigma2, rd)
    assert rr <= 1.0, (name, dtype, sigma2, rr)
    # the companion patch: its cond_2 is not in the fixture, so it is computed here
    Kc = _oracle_K(name, "Xc")
    ev = np.linalg.eigvalsh(Kc + sigma2 * np.eye(len(Kc)))
    condc = float(ev[-1] / ev[0])
    refc = LR.loo_reference(Kc, sigma2, g["yc"])
    rdc = _rel_err(_d_of(var[1]), refc["d"]) / (condc * u)
    rrc = float(np.abs(res[1].astype(LD) - refc["res"]).max()) / (condc * u * np.abs(g["yc"]).max())
    _record(test="end_to_end_companion", problem=name, dtype=dtype, sigma2=sigma2, cond2=condc, d_ratio_to_cond_u=rdc,
            res_ratio_to_cond_u_maxy=rrc)
    assert rdc <= 1.0 and rrc <= 1.0, (name, dtype, sigma2, rdc, rrc)


# ------------------------------------------------------------------------------------ 6. evidence
_summation_error_and_bound = LR.summation_error_and_bound


@pytest.mark.parametrize("name, dtype, k", CASES, ids=CASE_IDS)
def test_evidence(name, dtype, k):
    """logdet and quad against long-double sums over the device's own L diagonal, y and c (summation bound), and logdet
    end to end against the long-double reference in fp64 (loose: it catches a wrong sum).
    Measured on an MI355X: at most 0.0012 and 0.0018 of the summation bounds; end to end 3.5e-11 .. 1.6e-5 absolute
    against bounds of 3.6e-5 .. 107."""
    g, sigma2, cond = _case(name, dtype, k)
    model = _fit_batch(g, sigma2, dtype)
    logdet, quad = model.evidence()
    ys = [g["y"], g["yc"]]
    for r in range(2):
        n = int(model.n[r])
        Ldiag = np.diag(model.get(r, M.GET_L)).astype(LD)
        c = model.get(r, M.GET_C).astype(LD)
        y = _device_y(ys[r], dtype).astype(LD)
        e1, b1 = _summation_error_and_bound(n, logdet[r], LD(2) * np.log(Ldiag))
        e2, b2 = _summation_error_and_bound(n, quad[r], y * c)
        _record(test="evidence_vs_device_vectors", problem=name, dtype=dtype, sigma2=sigma2, patch=r,
                logdet_err=e1, logdet_bound=b1, quad_err=e2, quad_bound=b2)
        assert e1 <= b1, (name, dtype, sigma2, r, e1, b1)
        assert e2 <= b2, (name, dtype, sigma2, r, e2, b2)
    if dtype == "f64":
        # end to end: first-order tr(U^-1 dU) with the backward error of the factor; loose, catches a wrong sum
        ref = LR.loo_reference(_oracle_K(name), sigma2, g["y"])
        n = int(model.n[0])
        err, bound = abs(float(LD(logdet[0]) - ref["logdet"])), n * cond * 1e-14
        _record(test="logdet_end_to_end", problem=name, dtype=dtype, sigma2=sigma2, err=err, bound=bound)
        assert err <= bound, (name, sigma2, err, bound)
    # the front end assembles the log marginal likelihood from the two
    eta = pmk.MixtureGPType([g["X"], g["Xc"]], None)
    eta._model = model
    lml = pmk.logevidencemixtureGP(eta)
    assert np.array_equal(lml, -0.5 * quad - 0.5 * logdet - 0.5 * model.n * np.log(2 * np.pi))


# ------------------------------------------------------------------------------------ 7. meaning
def test_loo_is_the_prediction_without_the_point():
    """three ragged patches at sigma2 = 1e-2: for 8 points i of the first, a model WITHOUT point i is fitted and queried at
    x_i (pmk_model_queryinner_ex with min_v = -inf: the unclamped variance).  y_i - res_i must be that mean within
    1e-7 max(1, |mu|), var_i - sigma2 that variance within 1e-9 + 1e-5 v."""
    rng = np.random.Generator(np.random.PCG64(7171))
    sigma2, th = 1e-2, pmk.Spline34KernelType(1 / 4.0)
    Xs = [rng.uniform(-4, 4, (n, 2)) for n in (300, 420, 257)]
    ys = [np.sin(X[:, 0]) * np.cos(0.5 * X[:, 1]) for X in Xs]
    eta = pmk.MixtureGPType(Xs, None)
    pmk.fitmixtureGP_(eta, ys, th, sigma2)
    res, var = pmk.loomixtureGP(eta)
    assert [len(a) for a in res] == [300, 420, 257] and [len(a) for a in var] == [300, 420, 257]
    d = th.desc()
    for i in [0, 1, 127, 128, 200, 255, 256, 299]:
        keep = np.arange(300) != i
        m1 = M.DeviceModel([Xs[0][keep]], [ys[0][keep]])
        m1.fit(th, sigma2)
        assert m1.info()[0] == 0
        xq = np.ascontiguousarray(Xs[0][i:i + 1])
        mu, v = np.empty(1), np.empty(1)
        _lib.check(m1.ctx.L.pmk_model_queryinner_ex(m1.h, 0, C.byref(d), 1, xq.ctypes.data_as(_dp), -np.inf,
                                                    mu.ctypes.data_as(_dp), v.ctypes.data_as(_dp)), "pmk_model_queryinner_ex")
        em = abs((ys[0][i] - res[0][i]) - mu[0]) / (1e-7 * max(1.0, abs(mu[0])))
        ev = abs((var[0][i] - sigma2) - v[0]) / (1e-9 + 1e-5 * v[0])
        _record(test="meaning", point=i, mean_ratio=em, var_ratio=ev)
        assert em <= 1.0, (i, ys[0][i] - res[0][i], mu[0])
        assert ev <= 1.0, (i, var[0][i] - sigma2, v[0])


# ------------------------------------------------------------------------------------ 8. multi-output
def test_multi_output_columns():
    """R = 3 on the p1 sigma2 = 1e-6 batch: one d serves every column"""
    g, sigma2, cond = _case("p1", "f64", 1)
    assert sigma2 == 1e-6
    u = LR.U64
    Xs = [g["X"], g["Xc"]]
    Ys = [np.stack([np.sin(X[:, 0]) * np.cos(0.5 * X[:, 1]), np.cos(0.5 * X[:, 0]) + 0.1 * X[:, 1], 0.3 * X[:, 0] - np.sin(X[:, 1])], 1)
          for X in Xs]
    assert np.array_equal(Ys[0][:, 0], g["y"])
    eta = pmk.MixtureGPType(Xs, None)
    pmk.fitmixtureGP_multi_(eta, Ys, pmk.Spline34KernelType(float(g["theta"])), sigma2)
    model = eta._model
    RES, varm = pmk.loomixtureGP_multi(eta)
    res1, var1 = model.loo_values()
    for r in range(2):
        assert RES[r].shape == (len(Xs[r]), 3)
        assert np.array_equal(varm[r], var1[r])                    # bit for bit: the same d
    ref = LR.loo_reference(_oracle_K("p1"), sigma2, Ys[0])
    for j in range(3):
        rr = float(np.abs(RES[0][:, j].astype(LD) - ref["res"][:, j]).max()) / (cond * u * np.abs(Ys[0][:, j]).max())
        _record(test="multi_res", column=j, res_ratio_to_cond_u_maxy=rr)
        assert rr <= 1.0, (j, rr)
    logdet, quad = model.evidence_multi()
    assert quad.shape == (2, 3)
    assert np.array_equal(logdet, model.evidence()[0])
    Cs = model.weights_multi()
    for r in range(2):
        for j in range(3):
            err, bound = _summation_error_and_bound(len(Xs[r]), quad[r, j], Ys[r][:, j].astype(LD) * Cs[r][:, j].astype(LD))
            _record(test="multi_quad", patch=r, column=j, err=err, bound=bound)
            assert err <= bound, (r, j, err, bound)
    lml = pmk.logevidencemixtureGP_multi(eta)
    assert lml.shape == (2, 3) and np.all(np.isfinite(lml))


# ------------------------------------------------------------------------------------ 9. shapes
_trtri_colnorms = LR.trtri_colnorms


def oracle_f(X):
    return np.sin(X[:, 0]) * np.cos(0.5 * X[:, 1])


@pytest.mark.timeout(600)
def test_config_C_full_size():
    """256 patches x 2000 points (the data of test_config_C_full_size_properties).  K is positive semi-definite, so
    U^-1 <= I / sigma2 and 1 / d_i >= sigma2; Spline34 entries are <= 1, so cond_2 <= n / sigma2 + 1 and the relative error
    cond_2 u of the end-to-end bound is n u absolute."""
    N, levels, sigma2 = 512000, 9, 1e-5
    rng = np.random.Generator(np.random.PCG64(25))
    X = np.stack([rng.uniform(-5, 5, N), rng.uniform(-10, 10, N)], 1)
    y = oracle_f(X)
    th = pmk.Spline34KernelType(1 / 15)
    root, X_parts, X_parts_inds = pmk.setuppartition(X, levels)
    assert [len(p) for p in X_parts] == [2000] * 256
    model = pmk.DeviceModel(X_parts, [y[i] for i in X_parts_inds])
    model.fit(th, sigma2)
    assert np.all(model.info() == 0)
    model.loo()
    res, var = model.loo_values()
    n, u = 2000, LR.U64
    allv = np.stack(var)
    assert allv.shape == (256, n) and np.all(np.isfinite(allv)) and np.all(allv > 0)
    assert np.all(np.isfinite(np.stack(res)))
    _record(test="config_C", min_var_minus_sigma2=float(allv.min() - sigma2), slack=n * u)
    assert np.all(allv >= sigma2 - n * u)
    for r in (0, 101, 255):
        ratio = float((np.abs(_d_of(var[r]) - _trtri_colnorms(model.get(r, M.GET_L))) / _d_of(var[r])).max()) / (n * u)
        _record(test="config_C_d_vs_trtri", patch=r, ratio_to_n_u=ratio)
        assert ratio <= 1.0, (r, ratio)
    logdet, quad = model.evidence()
    assert np.all(np.isfinite(logdet)) and np.all(quad > 0)


@pytest.mark.timeout(600)
def test_split_mode_single_problem():
    """P = 1 with 33 tiles takes the split factorisation path; the leave-one-out kernel is the same one"""
    rng = np.random.Generator(np.random.PCG64(9191))
    n = 4224
    X = rng.uniform(-6, 6, (n, 2))
    model = M.DeviceModel([X], [oracle_f(X)])
    model.fit(pmk.Spline34KernelType(1 / 3.0), 1e-4)
    assert model.info()[0] == 0
    model.loo()
    _, var = model.loo_values()
    ratio = float((np.abs(_d_of(var[0]) - _trtri_colnorms(model.get(0, M.GET_L))) / _d_of(var[0])).max()) / (n * LR.U64)
    _record(test="split_mode", n=n, ratio_to_n_u=ratio)
    assert ratio <= 1.0, ratio


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_one_to_three_tiles_exactly(dtype):
    """n = 128, 256, 257, 384 (and 1): a first strip only, an odd tile count (a 128-column last strip), and the edge of
    the identity padding"""
    rng = np.random.Generator(np.random.PCG64(9292))
    sizes = [128, 256, 257, 384, 1]
    Xs = [rng.uniform(-4, 4, (n, 2)) for n in sizes]
    sigma2 = 1e-2
    model = M.DeviceModel(Xs, [oracle_f(X) for X in Xs], dtype=dtype)
    model.fit(pmk.Spline34KernelType(1 / 4.0), sigma2)
    assert np.all(model.info() == 0)
    model.loo()
    _, var = model.loo_values()
    u = LR.unit_roundoff(dtype)
    for r, n in enumerate(sizes):
        assert len(var[r]) == n
        dstar = LR.linv_colnorms_ld(model.get(r, M.GET_L))
        # n = 1: d = fl(fl(1 / L_11)^2) carries up to 3 roundoffs of its own and the read-back as 1 / var two of 2^-53,
        # which n u = u cannot hold: 4 u there
        ratio = _rel_err(_d_of(var[r]), dstar) / (max(n, 4) * u)
        _record(test="tile_edges", dtype=dtype, n=n, ratio_to_max_n_4_u=ratio)
        assert ratio <= 1.0, (n, ratio)


@pytest.mark.parametrize("D, th", [(1, pmk.Spline34KernelType(1 / 2.0)), (3, pmk.Spline34KernelType(1 / 3.0)),
                                   (2, pmk.RationalQuadraticKernelType(0.5))], ids=["D1", "D3", "RQ"])
def test_other_dimensions_and_a_second_family(D, th):
    """the kernel has no D and no family in it: one case each shows that the launcher takes them"""
    rng = np.random.Generator(np.random.PCG64(9393 + D))
    Xs = [rng.uniform(-3, 3, (n, D)) for n in (300, 140)]
    model = M.DeviceModel(Xs, [np.sin(X[:, 0]) for X in Xs])
    model.fit(th, 1e-2)
    assert np.all(model.info() == 0)
    model.loo()
    _, var = model.loo_values()
    for r, X in enumerate(Xs):
        n = len(X)
        ratio = _rel_err(_d_of(var[r]), LR.linv_colnorms_ld(model.get(r, M.GET_L))) / (n * LR.U64)
        _record(test="dims_families", D=D, n=n, ratio_to_n_u=ratio)
        assert ratio <= 1.0, (D, n, ratio)


# ------------------------------------------------------------------------------------ 10. state and failure
def _raw(model):
    return model.ctx.L, model.h


def _ptrs(arrs):
    return (_dp * len(arrs))(*[a.ctypes.data_as(_dp) for a in arrs])


def test_state_rules_of_the_library():
    rng = np.random.Generator(np.random.PCG64(9494))
    Xs = [rng.uniform(-4, 4, (n, 2)) for n in (200, 130)]
    ys = [oracle_f(X) for X in Xs]
    th = pmk.Spline34KernelType(1 / 4.0)
    model = M.DeviceModel(Xs, ys)
    L, h = _raw(model)
    res, var = [np.empty(len(X)) for X in Xs], [np.empty(len(X)) for X in Xs]
    ld = np.array([len(X) for X in Xs], dtype=np.int64)
    RES = [np.empty((len(X), 2), order="F") for X in Xs]
    two = np.empty(2)
    last = lambda: L.pmk_last_error().decode()
    # no factor yet
    assert L.pmk_model_loo(h) < 0 and "no factor" in last()
    assert L.pmk_model_evidence(h, two.ctypes.data_as(_dp), None) < 0 and "no factor" in last()
    assert L.pmk_model_get_loo(h, _ptrs(res), _ptrs(var)) < 0 and "no factor" in last()
    model.fit(th, 1e-2)
    # get_loo before pmk_model_loo
    assert L.pmk_model_get_loo(h, _ptrs(res), _ptrs(var)) < 0 and "pmk_model_loo has not run" in last()
    assert L.pmk_model_loo(h) == 0
    assert L.pmk_model_get_loo(h, _ptrs(res), None) == 0 and L.pmk_model_get_loo(h, None, _ptrs(var)) == 0
    # *_multi before pmk_model_solve_multi
    assert L.pmk_model_get_loo_multi(h, _ptrs(RES), ld.ctypes.data_as(C.POINTER(C.c_int64)), _ptrs(var)) < 0
    assert "pmk_model_solve_multi has not run" in last()
    four = np.empty(4)
    assert L.pmk_model_evidence_multi(h, two.ctypes.data_as(_dp), four.ctypes.data_as(_dp)) < 0
    assert "pmk_model_solve_multi has not run" in last()
    # new weights need no new pass: res follows the resident c, var does not move
    var0 = [v.copy() for v in var]
    c2 = [np.cos(X[:, 0]) for X in Xs]
    assert L.pmk_model_set_weights(h, _ptrs(c2)) == 0
    assert L.pmk_model_get_loo(h, _ptrs(res), _ptrs(var)) == 0
    for r in range(2):
        assert np.array_equal(var[r], var0[r])
        assert np.allclose(res[r], c2[r] * var0[r], rtol=1e-14, atol=0)
    # solve_multi after the pass: no new pass either
    model.set_targets_multi([np.stack([y, 2 * y], 1) for y in ys])
    model.solve_multi()
    assert L.pmk_model_get_loo_multi(h, _ptrs(RES), ld.ctypes.data_as(C.POINTER(C.c_int64)), _ptrs(var)) == 0
    for r in range(2):
        assert np.array_equal(var[r], var0[r])
        assert np.allclose(RES[r][:, 1], 2 * RES[r][:, 0], rtol=1e-9)
    # a second fit with another sigma2 invalidates d
    model.fit(th, 1e-3)
    assert L.pmk_model_get_loo(h, _ptrs(res), _ptrs(var)) < 0 and "pmk_model_loo has not run" in last()
    with pytest.raises(_lib.PmkError):
        model.loo_values()
    model.loo()
    _, var2 = model.loo_values()
    for r, X in enumerate(Xs):
        n = len(X)
        ratio = _rel_err(_d_of(var2[r]), LR.linv_colnorms_ld(model.get(r, M.GET_L))) / (n * LR.U64)
        assert ratio <= 1.0, (r, ratio)
        assert not np.array_equal(var2[r], var0[r])
        assert np.all(var2[r] >= 1e-3 - n * LR.U64) and var2[r].min() < 1e-2


def test_a_model_from_factors_has_residuals_but_no_quad():
    rng = np.random.Generator(np.random.PCG64(9595))
    Xs = [rng.uniform(-4, 4, (n, 2)) for n in (200, 130)]
    ys = [oracle_f(X) for X in Xs]
    th = pmk.Spline34KernelType(1 / 4.0)
    model = M.DeviceModel(Xs, ys)
    model.fit(th, 1e-2)
    model.loo()
    res, var = model.loo_values()
    logdet, _ = model.evidence()
    loaded = M.DeviceModel.from_factors(Xs, model.weights(), [model.get(r, M.GET_L) for r in range(2)])
    loaded.loo()
    res2, var2 = loaded.loo_values()
    for r in range(2):
        assert np.array_equal(var2[r], var[r]) and np.array_equal(res2[r], res[r])
    with pytest.raises(_lib.PmkError):
        loaded.evidence()
    assert np.array_equal(loaded.evidence(quad=False)[0], logdet)
    L, h = _raw(loaded)
    two = np.empty(2)
    assert L.pmk_model_evidence(h, two.ctypes.data_as(_dp), two.ctypes.data_as(_dp)) < 0
    assert "holds no targets" in L.pmk_last_error().decode()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_a_failed_patch_returns_nan_and_leaves_the_others_alone(dtype):
    """one patch has a NaN coordinate (info > 0 there, reported cleanly by the fit): NaN in all four outputs of that patch,
    the other patches meet the bound of the kernel test"""
    rng = np.random.default_rng(42)
    n, sigma2 = 300, 1e-2
    Xs = [rng.uniform(-4, 4, (n, 2)) for _ in range(3)]
    Xs[1][130, 1] = np.nan
    ys = [oracle_f(np.nan_to_num(X)) for X in Xs]
    model = M.DeviceModel(Xs, ys, dtype=dtype)
    model.fit(pmk.Spline34KernelType(1 / 3.0), sigma2)
    assert model.info().tolist() == [0, 131, 0]
    model.loo()
    res, var = model.loo_values()
    logdet, quad = model.evidence()
    assert np.all(np.isnan(res[1])) and np.all(np.isnan(var[1])) and np.isnan(logdet[1]) and np.isnan(quad[1])
    u = LR.unit_roundoff(dtype)
    for r in (0, 2):
        assert np.all(np.isfinite(res[r])) and np.isfinite(logdet[r]) and np.isfinite(quad[r])
        ratio = _rel_err(_d_of(var[r]), LR.linv_colnorms_ld(model.get(r, M.GET_L))) / (n * u)
        _record(test="beside_a_failed_patch", dtype=dtype, patch=r, ratio_to_n_u=ratio)
        assert ratio <= 1.0, (r, ratio)

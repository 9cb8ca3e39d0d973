"""CPU-side checks of the model-selection entry points (no device compute): the header, the ctypes table and the Julia
ccalls agree on the five symbols; the long-double reference of the GPU tests (tests/_loo_refs.py) agrees with brute-force
refits without a point; the Python front end rejects calls in the wrong state before any device call."""
import numpy as np
import pytest
import scipy.linalg as sla

import patchmixturekriging_amd as pmk
from patchmixturekriging_amd import _lib
from patchmixturekriging_amd import mixture as M
from oracle import oracle as O
from test_julia_binding import header_prototypes, julia_ccalls

import _loo_refs as LR

NEW = ["pmk_model_evidence", "pmk_model_evidence_multi", "pmk_model_loo", "pmk_model_get_loo", "pmk_model_get_loo_multi"]

CTYPES = {"c_int": "i32", "c_int64": "i64", "c_long": "i64", "c_double": "f64"}


def _cat(t):
    return CTYPES.get(getattr(t, "__name__", ""), "ptr")


# ------------------------------------------------------------------------------------ 1. the three descriptions of the ABI
def test_header_and_signatures_agree():
    protos = header_prototypes()
    L = pmk.lib()
    for name in NEW:
        assert name in protos, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(L, name), name
        res, args = _lib.SIGNATURES[name]
        cret, cargs = protos[name]
        assert [_cat(a) for a in args] == cargs, name
        assert _cat(res) == cret, name
    assert L.pmk_version() == 103


def test_julia_ccalls_of_the_new_symbols_match_the_header():
    protos = header_prototypes()
    seen = set()
    for name, ret, args, line in julia_ccalls():
        if name in NEW:
            assert (ret, args) == protos[name], (name, line)
            seen.add(name)
    assert seen == set(NEW), sorted(set(NEW) - seen)


def test_the_front_end_exports_the_four_functions():
    for name in ("logevidencemixtureGP", "logevidencemixtureGP_multi", "loomixtureGP", "loomixtureGP_multi"):
        assert callable(getattr(pmk, name)), name
    for name in ("evidence", "evidence_multi", "loo", "loo_values", "loo_values_multi"):
        assert callable(getattr(pmk.DeviceModel, name)), name


# ------------------------------------------------------------------------------------ 2. the reference against brute force
@pytest.mark.parametrize("sigma2", [1e-2, 1e-5])
def test_closed_form_reference_against_refits_without_a_point(sigma2):
    """A 300-point 2-D Spline34(1/4) patch: for 9 points i, fit the other 299 with LAPACK and predict at x_i (queryinner! of
    mixtureGP.jl:296-316, unclamped).  The closed form of tests/_loo_refs.py must give the same mean, within the project's
    1e-7 max(1, |mu|), and var_i - sigma2 must be the latent variance 1 - |L^-1 k|^2, within 1e-9 + 1e-5 v."""
    rng = np.random.Generator(np.random.PCG64(5151))
    n = 300
    X = rng.uniform(-4, 4, (n, 2))
    y = np.sin(X[:, 0]) * np.cos(0.5 * X[:, 1])
    oth = O.kernel(O.SPLINE34, 1 / 4.0)
    K = O.kernel_matrix(oth, X)
    ref = LR.loo_reference(K, sigma2, y)
    mu_cf = (y.astype(LR.LD) - ref["res"]).astype(np.float64)
    v_cf = (ref["var"] - LR.LD(sigma2)).astype(np.float64)
    worst_mu = worst_v = 0.0
    for i in [0, 1, 37, 99, 150, 151, 222, 298, 299]:
        keep = np.arange(n) != i
        Ui = K[np.ix_(keep, keep)] + sigma2 * np.eye(n - 1)
        Li = sla.cholesky(Ui, lower=True)
        k = K[keep, i]
        mu = k @ sla.cho_solve((Li, True), y[keep])
        w = sla.solve_triangular(Li, k, lower=True)
        v = 1.0 - w @ w                                     # Spline34: k(x, x) = 1
        tol_mu, tol_v = 1e-7 * max(1.0, abs(mu)), 1e-9 + 1e-5 * v
        worst_mu = max(worst_mu, abs(mu_cf[i] - mu) / tol_mu)
        worst_v = max(worst_v, abs(v_cf[i] - v) / tol_v)
        assert abs(mu_cf[i] - mu) <= tol_mu, (i, mu_cf[i], mu)
        assert abs(v_cf[i] - v) <= tol_v, (i, v_cf[i], v)
    print("sigma2 %.0e: closed form vs refit, worst ratio to the tolerance: mean %.2g, variance %.2g" % (sigma2, worst_mu, worst_v))


def test_reference_pieces_agree_with_lapack():
    """the reference's d, logdet and quad against LAPACK in double on a well-conditioned patch (catches a wrong formula,
    not a rounding)"""
    rng = np.random.Generator(np.random.PCG64(5152))
    X = rng.uniform(-4, 4, (200, 2))
    Y = np.stack([np.sin(X[:, 0]), np.cos(X[:, 1])], 1)
    K = O.kernel_matrix(O.kernel(O.SPLINE34, 1 / 4.0), X)
    ref = LR.loo_reference(K, 1e-2, Y)
    U = K + 1e-2 * np.eye(200)
    Ui = np.linalg.inv(U)
    assert np.allclose(ref["d"].astype(float), np.diag(Ui), rtol=1e-10)
    assert np.allclose(ref["C"].astype(float), Ui @ Y, rtol=1e-8, atol=1e-12)
    assert abs(float(ref["logdet"]) - np.linalg.slogdet(U)[1]) <= 1e-9
    assert np.allclose(ref["quad"].astype(float), np.einsum("ij,ij->j", Y, Ui @ Y), rtol=1e-10)
    assert np.allclose(LR.linv_colnorms_ld(np.linalg.cholesky(U)).astype(float), np.diag(Ui), rtol=1e-10)


# ------------------------------------------------------------------------------------ 3. state rules of the front end
class _NoDeviceLib:
    """stands in for the loaded library: any call into it is a failure of the test"""

    def __getattr__(self, name):
        raise AssertionError("a device call was made: %s" % name)


class _Ctx:
    L = _NoDeviceLib()
    h = None


def _model(**state):
    m = object.__new__(M.DeviceModel)          # no constructor: it would create a device model
    m.ctx, m.h, m.P, m.R, m.n = _Ctx(), None, 2, 3, np.array([5, 7])
    m._has_factor = m._has_targets = m._loo_done = m._multi_solved = False
    for k, v in state.items():
        setattr(m, k, v)
    return m


@pytest.mark.parametrize("call, state", [
    (lambda m: m.evidence(), {}),                                                             # no factor
    (lambda m: m.loo(), {}),
    (lambda m: m.loo_values(), {}),
    (lambda m: m.evidence(), dict(_has_factor=True)),                                         # built from factors: no y
    (lambda m: m.loo_values(), dict(_has_factor=True, _has_targets=True)),                    # loo() has not run
    (lambda m: m.loo_values_multi(), dict(_has_factor=True, _has_targets=True, _loo_done=True)),   # solve_multi has not
    (lambda m: m.evidence_multi(), dict(_has_factor=True, _has_targets=True)),
    (lambda m: m.loo_values_multi(), dict(_has_factor=True, _has_targets=True, _multi_solved=True)),
])
def test_wrong_state_is_refused_before_any_device_call(call, state):
    with pytest.raises(_lib.PmkError):
        call(_model(**state))


@pytest.mark.parametrize("fn", ["logevidencemixtureGP", "logevidencemixtureGP_multi", "loomixtureGP", "loomixtureGP_multi"])
def test_module_functions_need_a_fitted_model(fn, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(M, "DeviceModel", no_device)
    eta = pmk.MixtureGPType([np.zeros((5, 2)), np.zeros((7, 2))], None)
    with pytest.raises(_lib.PmkError):
        getattr(pmk, fn)(eta)


def test_a_new_fit_invalidates_the_python_side_state(monkeypatch):
    """fit() resets what loo() and solve_multi() had established (the library does the same: pmk_model_fit)"""
    class _Lib:
        def pmk_model_fit(self, *a):
            return 0
    m = _model(_has_factor=True, _has_targets=True, _loo_done=True, _multi_solved=True)
    m.ctx.L = _Lib()
    m.fit(pmk.Spline34KernelType(1.0), 1e-3)
    assert m._has_factor and not m._loo_done and not m._multi_solved
    m.ctx.L = _NoDeviceLib()
    with pytest.raises(_lib.PmkError):
        m.loo_values()

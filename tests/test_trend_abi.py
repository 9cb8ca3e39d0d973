"""CPU-side checks of kriging with a trend (no device compute): the header, the ctypes table and the Julia ccalls agree
on the three new symbols; the long-double reference of tests/_trend_refs.py equals n brute-force leave-one-out refits;
the Python front end rejects a bad trend before any device call."""
import re

import numpy as np
import pytest

import patchmixturekriging_amd as pmk
from patchmixturekriging_amd import _lib
from patchmixturekriging_amd import mixture as M
from oracle import oracle as O
from test_julia_binding import header_prototypes, julia_ccalls
from test_multi_output_abi import _cat, _NoDevice
import _trend_refs as T

NEW = ["pmk_model_set_trend", "pmk_model_get_trend", "pmk_model_trend_info"]


def _header():
    return open(_lib.os.path.join(_lib._HERE, "..", "include", "pmk.h")).read()


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
    txt = _header()
    assert "enum { PMK_TREND_NONE = -1, PMK_TREND_CONSTANT = 0, PMK_TREND_LINEAR = 1 };" in txt
    assert M.TREND_DEGREES == {None: -1, "none": -1, "constant": 0, "linear": 1}
    flat = re.sub(r"[\s*]+", " ", txt)
    assert "beta is with respect to raw coordinates" in flat and "the trend term is added after the clamp" in flat
    assert L.pmk_version() == 103


def test_library_exports_everything_declared():
    L = pmk.lib()
    for name in header_prototypes():
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES, name


def test_julia_ccalls_of_the_new_symbols_match_the_header():
    protos = header_prototypes()
    seen = set()
    for name, ret, args, line in julia_ccalls():
        if name in NEW:
            assert (ret, args) == protos[name], (name, line)
            seen.add(name)
    assert seen == set(NEW)


def test_host_state_calls_need_no_device():
    """the argument checks of the three symbols run before any device call"""
    L = pmk.lib()
    assert L.pmk_model_set_trend(None, 0) == -1
    assert L.pmk_model_get_trend(None, None, None, None) == -1
    assert L.pmk_model_trend_info(None, None) == -1
    assert b"pmk_model_trend_info" in L.pmk_last_error()


# ------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("trend,D", [("constant", 2), ("linear", 1), ("linear", 2)])
def test_reference_equals_brute_force_refits(trend, D):
    rng = np.random.default_rng(7 + D)
    n, R, sigma2 = 40, 2, 1e-3
    X = rng.uniform(-2, 2, (n, D))
    Y = np.stack([np.sin(X[:, 0]) + 0.5 * X[:, -1] + 1.0, np.cos(2 * X[:, 0]) - 0.3], 1)
    K = O.kernel_matrix(O.kernel(O.SPLINE34, 1 / 3.0), X)
    H = T.basis(X, trend)
    ref = T.trend_reference(K, sigma2, Y, H)
    res, var = T.brute_force_loo(K, sigma2, Y, H)
    scale = float(np.abs(res).max())
    assert float(np.abs(ref["res"] - res).max()) <= 1e-13 * scale
    assert float(np.abs(ref["var"] - var).max()) <= 1e-13 * float(var.max())
    # the constraint and the quadratic form: H^T C = 0, Y^T C = (y - H beta)^T U^-1 (y - H beta)
    assert float(np.abs(H.T @ ref["C"]).max()) <= 1e-15 * float(np.abs(H).max() * np.abs(ref["C"]).sum())
    quad = (np.asarray(Y, dtype=T.LD) * ref["C"]).sum(0)
    assert float(np.abs(quad - ref["quad"]).max()) <= 1e-13 * float(np.abs(ref["quad"]).max())
    # the fp64 yardstick computes the same thing
    f = T.gls_fp64(K, sigma2, Y, H)
    assert float(np.abs(f["beta"] - ref["beta"]).max()) <= 1e-9 * float(np.abs(ref["beta"]).max())
    assert float(np.abs(f["res"] - ref["res"]).max()) <= 1e-9 * scale


def test_reference_prediction_far_away_is_the_trend():
    rng = np.random.default_rng(3)
    X = rng.uniform(-2, 2, (30, 2))
    y = 2 + 3 * X[:, 0] - X[:, 1]
    oth = O.kernel(O.SPLINE34, 1 / 3.0)
    ref = T.trend_reference(O.kernel_matrix(oth, X), 1e-3, y, T.basis(X, "linear"))
    assert np.allclose(np.asarray(ref["beta"][:, 0], dtype=float), [2, 3, -1], atol=1e-12)
    xq = np.array([[50.0, -70.0]])
    mu, v = T.predict_reference(ref, O.cross_kernel_matrix(oth, xq, X), [1.0], T.basis(xq, "linear"))
    assert abs(float(mu[0, 0]) - (2 + 150 + 70)) <= 1e-9
    assert float(v[0]) > 1.0            # k(x, x) plus the uncertainty of the extrapolated plane


# ------------------------------------------------------------------------------------------ validation, no device call
def _no_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(M, "fitmixtureGP_", no_device)
    monkeypatch.setattr(M, "DeviceModel", no_device)


def test_unknown_trend_name(monkeypatch):
    _no_device(monkeypatch)
    Ys = [np.zeros((5, 2)), np.zeros((7, 2))]
    for bad in ("quadratic", "", 1, "Linear"):
        with pytest.raises(ValueError, match="trend must be"):
            pmk.fitmixtureGP_trend_(_NoDevice([5, 7]), Ys, pmk.Spline34KernelType(1.0), 1e-5, trend=bad)


@pytest.mark.parametrize("R,trend", [(16, "constant"), (14, "linear"), (15, "linear")])
def test_too_many_columns(R, trend, monkeypatch):
    _no_device(monkeypatch)
    Ys = [np.zeros((5, R)), np.zeros((7, R))]           # D = 2: q = 1 or 3
    with pytest.raises(ValueError, match="R = %d target columns and q = " % R):
        pmk.fitmixtureGP_trend_(_NoDevice([5, 7]), Ys, pmk.Spline34KernelType(1.0), 1e-5, trend=trend)
    assert M.trend_columns("linear", 2, 13) == 3 and M.trend_columns("constant", 4, 15) == 1
    assert M.trend_columns(None, 4, 16) == 0


def test_closure_kernel_is_refused(monkeypatch):
    _no_device(monkeypatch)

    class Warped:
        warped = True

    class WithDiag:
        def diag_addend(self, X):
            return np.zeros(len(X))

    Ys = [np.zeros(5), np.zeros(7)]
    for th in (Warped(), WithDiag()):
        with pytest.raises(TypeError, match="closure-carrying"):
            pmk.fitmixtureGP_trend_(_NoDevice([5, 7]), Ys, th, 1e-5, trend="constant")


def test_stage_timers_and_docs_name_the_feature():
    assert '"trend_gls", "trend_items"' in _header()
    root = _lib.os.path.join(_lib._HERE, "..")
    for doc, word in (("DESIGN.md", "trend_gls_kernel"), ("README.md", "fitmixtureGP_trend_"), ("INTEGRATION.md", "pmk_model_set_trend")):
        assert word in open(_lib.os.path.join(root, doc), encoding="utf-8").read(), doc

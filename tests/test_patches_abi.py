"""CPU-side checks of the per-patch hyperparameter entry points (no device compute): the header, the ctypes table, the
library and the Julia ccalls agree on the new symbols; the Python front end refuses wrong lengths, closure-carrying
kernels and calls in the wrong state before any device call; the winner rule of the selection helper on hand-made
score arrays."""
import numpy as np
import pytest

import patchmixturekriging_amd as pmk
from patchmixturekriging_amd import _lib
from patchmixturekriging_amd import mixture as M
from test_julia_binding import header_prototypes, julia_ccalls

NEW = ["pmk_model_fit_patches", "pmk_model_set_kernels", "pmk_model_get_hyper", "pmk_query_items_fitted",
       "pmk_query_items_multi_fitted", "pmk_predict_mixture_fitted", "pmk_predict_mixture_multi_fitted"]
# what the Julia module binds: the one-shots cover the staged *_fitted calls there
JULIA_BOUND = ["pmk_model_fit_patches", "pmk_model_get_hyper", "pmk_predict_mixture_fitted", "pmk_predict_mixture_multi_fitted"]

CTYPES = {"c_int": "i32", "c_int64": "i64", "c_long": "i64", "c_double": "f64"}


def _cat(t):
    return CTYPES.get(getattr(t, "__name__", ""), "ptr")


# ------------------------------------------------------------------------------------ 1. the three descriptions of the ABI
def test_header_signatures_and_library_agree():
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


def test_declared_argument_lists():
    """the proposal of the issue, argument by argument"""
    protos = header_prototypes()
    assert protos["pmk_model_fit_patches"] == ("i32", ["ptr", "ptr", "ptr"])
    assert protos["pmk_model_set_kernels"] == ("i32", ["ptr", "ptr"])
    assert protos["pmk_model_get_hyper"] == ("i32", ["ptr", "ptr", "ptr"])
    assert protos["pmk_query_items_fitted"] == ("i32", ["ptr"])
    assert protos["pmk_query_items_multi_fitted"] == ("i32", ["ptr", "i32"])
    assert protos["pmk_predict_mixture_fitted"] == ("i32", ["ptr", "ptr", "i64", "ptr", "f64", "f64", "ptr", "ptr"])
    assert protos["pmk_predict_mixture_multi_fitted"] == ("i32", ["ptr", "ptr", "i64", "ptr", "f64", "f64", "ptr", "i64", "ptr"])


def test_julia_ccalls_of_the_new_symbols_match_the_header():
    protos = header_prototypes()
    seen = set()
    for name, ret, args, line in julia_ccalls():
        if name in NEW:
            assert (ret, args) == protos[name], (name, line)
            seen.add(name)
    assert set(JULIA_BOUND) <= seen, sorted(set(JULIA_BOUND) - seen)


def test_the_front_end_exports_the_new_names():
    for name in ("fitmixtureGP_patches_", "querymixtureGP_patches", "querymixtureGP_multi_patches", "selectmixtureGP_",
                 "select_candidates"):
        assert callable(getattr(pmk, name)), name
    for name in ("fit_patches", "set_kernels", "hyper"):
        assert callable(getattr(pmk.DeviceModel, name)), name
    for name in ("items_fitted", "items_multi_fitted"):
        assert callable(getattr(pmk.DeviceQuery, name)), name


def test_null_arguments_are_refused_by_the_library():
    """NULL arrays return -1 (a NULL model as well: nothing is dereferenced)"""
    L = pmk.lib()
    assert L.pmk_model_fit_patches(None, None, None) == -1
    assert L.pmk_model_set_kernels(None, None) == -1
    assert L.pmk_model_get_hyper(None, None, None) == -1
    assert L.pmk_query_items_fitted(None) == -1
    assert L.pmk_query_items_multi_fitted(None, 1) == -1
    assert L.pmk_predict_mixture_fitted(None, None, 0, None, 0.5, 1e-5, None, None) == -1
    assert L.pmk_predict_mixture_multi_fitted(None, None, 0, None, 0.5, 1e-5, None, 0, None) == -1


# ------------------------------------------------------------------------------------ 2. validation before any device call
class _NoDeviceLib:
    """stands in for the loaded library: any call into it is a failure of the test"""

    def __getattr__(self, name):
        raise AssertionError("a device call was made: %s" % name)


class _Ctx:
    L = _NoDeviceLib()
    h = None


def _model(P=3, **state):
    m = object.__new__(M.DeviceModel)          # no constructor: it would create a device model
    m.ctx, m.h, m.P, m.n = _Ctx(), None, P, np.arange(5, 5 + P)
    m._has_factor = m._has_targets = m._loo_done = m._multi_solved = m._has_kernels = False
    for k, v in state.items():
        setattr(m, k, v)
    return m


def _closure_kernels():
    canon = pmk.Spline34KernelType(0.25)
    wf = lambda x: 0.5 * x[0]      # noqa: E731
    return [pmk.AdaptiveKernelType(canon, wf), pmk.AdaptiveKernelDPPType(canon, wf),
            pmk.AdaptiveKernelMultiWarpType(canon, [wf], [1.0]), pmk.AdaptiveKernelMultiWarpDPPType(canon, [wf], [1.0], 0.5),
            pmk.FastAdaptiveKernelType(canon, [wf], None, [1.0])]


S34 = pmk.Spline34KernelType


@pytest.mark.parametrize("thetas, sigma2s", [
    ([S34(1.0)] * 2, [1e-3] * 3),                      # too few kernels
    ([S34(1.0)] * 4, [1e-3] * 3),                      # too many
    ([S34(1.0)] * 3, [1e-3] * 2),                      # too few noise variances
    ([S34(1.0)] * 3, [1e-3] * 4),
    ([], []),
])
def test_wrong_lengths_are_refused_before_any_device_call(thetas, sigma2s):
    with pytest.raises(ValueError):
        _model().fit_patches(thetas, sigma2s)
    eta = pmk.MixtureGPType([np.zeros((5, 2)), np.zeros((6, 2)), np.zeros((7, 2))], None)
    with pytest.raises(ValueError):
        pmk.fitmixtureGP_patches_(eta, [np.zeros(5), np.zeros(6), np.zeros(7)], thetas, sigma2s)
    if len(thetas) != 3:
        with pytest.raises(ValueError):
            _model(_has_factor=True).set_kernels(thetas)


@pytest.mark.parametrize("k", range(5))
def test_closure_carrying_kernels_are_refused_before_any_device_call(k, monkeypatch):
    bad = _closure_kernels()[k]
    thetas = [S34(1.0), bad, S34(0.5)]
    with pytest.raises(TypeError, match="patch 1"):
        _model().fit_patches(thetas, [1e-3] * 3)
    with pytest.raises(TypeError, match="patch 1"):
        _model(_has_factor=True).set_kernels(thetas)

    def no_device(*a, **kw):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(M, "DeviceModel", no_device)
    eta = pmk.MixtureGPType([np.zeros((5, 2)), np.zeros((6, 2)), np.zeros((7, 2))], None)
    ys = [np.zeros(5), np.zeros(6), np.zeros(7)]
    with pytest.raises(TypeError):
        pmk.fitmixtureGP_patches_(eta, ys, thetas, [1e-3] * 3)
    with pytest.raises(TypeError):
        pmk.selectmixtureGP_(eta, ys, [(S34(1.0), 1e-3), (bad, 1e-3)])


def test_fitted_queries_need_a_model_with_kernels(monkeypatch):
    q = object.__new__(M.DeviceQuery)
    q.model, q.L, q.h = _model(_has_factor=True), _NoDeviceLib(), None       # built from factors, no set_kernels yet
    with pytest.raises(_lib.PmkError):
        q.items_fitted()
    with pytest.raises(_lib.PmkError):
        q.items_multi_fitted(variance=False)
    eta = pmk.MixtureGPType([np.zeros((5, 2))], None)
    for fn in (pmk.querymixtureGP_patches, pmk.querymixtureGP_multi_patches):
        with pytest.raises(_lib.PmkError):
            fn(np.zeros((2, 2)), eta, None, 1, 0.5, 1e-5, S34(2.0))


def test_selection_arguments_are_checked_before_any_device_call(monkeypatch):
    def no_device(*a, **kw):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(M, "DeviceModel", no_device)
    eta = pmk.MixtureGPType([np.zeros((5, 2))], None)
    with pytest.raises(ValueError):
        pmk.selectmixtureGP_(eta, [np.zeros(5)], [(S34(1.0), 1e-3)], score="aic")
    with pytest.raises(ValueError):
        pmk.selectmixtureGP_(eta, [np.zeros(5)], [])


def test_a_per_patch_fit_sets_the_python_side_state():
    class _Lib:
        def pmk_model_fit_patches(self, h, descs, s2):
            self.got = ([(d.family, d.p[0]) for d in descs], [s2[i] for i in range(3)])
            return 0
    m = _model(_loo_done=True, _multi_solved=True)
    m.ctx.L = _Lib()
    m.fit_patches([S34(1.0), pmk.GaussianKernel1DType(4.0), S34(0.5)], [1e-2, 1e-3, 1e-4])
    assert m.ctx.L.got == ([(1, 1.0), (4, 4.0), (1, 0.5)], [1e-2, 1e-3, 1e-4])      # descriptor r and sigma2 r of patch r
    assert m._has_factor and m._has_kernels and not m._loo_done and not m._multi_solved


# ------------------------------------------------------------------------------------ 3. the winner rule
def test_select_candidates_takes_the_highest_score():
    s = np.array([[-3.0, 5.0, 0.0],
                  [-1.0, 4.0, 0.5],
                  [-2.0, 9.0, -7.0]])
    w = pmk.select_candidates(s)
    assert w.tolist() == [1, 2, 1] and w.dtype == np.int64


def test_select_candidates_ties_go_to_the_lowest_index():
    s = np.array([[1.0, 2.0, -1.0],
                  [3.0, 2.0, -1.0],
                  [3.0, 2.0, -1.0],
                  [0.0, 1.0, -2.0]])
    assert pmk.select_candidates(s).tolist() == [1, 0, 0]


def test_select_candidates_skips_nan():
    nan = np.nan
    s = np.array([[nan, 1.0, nan],
                  [2.0, nan, nan],
                  [1.0, 0.0, -np.inf],
                  [nan, nan, nan]])
    assert pmk.select_candidates(s).tolist() == [1, 0, 2]      # -inf is a score; NaN is not


def test_select_candidates_all_nan_raises_and_names_the_patch():
    s = np.array([[1.0, np.nan, 2.0],
                  [0.0, np.nan, 3.0]])
    with pytest.raises(ValueError, match="patch 1"):
        pmk.select_candidates(s)
    with pytest.raises(ValueError):
        pmk.select_candidates(np.empty((0, 3)))

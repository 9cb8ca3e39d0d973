"""CPU-side checks of the multi-output blended leave-one-out (no device compute): the header, the ctypes table and the
Julia ccalls agree on the three symbols; the Python functions exist; every refusal of the front end is raised before any
device call; the closed form of tests/_loo_blend_multi_refs.py (the identity the device code implements, with and without
a trend) agrees with refits without the point."""
import numpy as np
import pytest

import patchmixturekriging_amd as pmk
from patchmixturekriging_amd import _lib
from patchmixturekriging_amd import mixture as M
from oracle import oracle as O
from test_julia_binding import header_prototypes, julia_ccalls

import _loo_blend_refs as BR
import _loo_blend_multi_refs as MR

NEW = ["pmk_query_items_loo_multi", "pmk_predict_mixture_loo_multi", "pmk_query_get_items_multi"]
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


def test_the_front_end_exports_the_functions():
    for name in ("loomixtureGP_blend_multi", "selectblendGP_multi_"):
        assert callable(getattr(pmk, name)), name
    assert callable(pmk.DeviceQuery.items_loo_multi) and callable(pmk.DeviceQuery.item_values_multi)


# ------------------------------------------------------------------------------------ 2. state rules of the front end
class _NoDeviceLib:
    """stands in for the loaded library: any call into it is a failure of the test"""

    def __getattr__(self, name):
        raise AssertionError("a device call was made: %s" % name)


class _Ctx:
    L = _NoDeviceLib()
    h = None


_DeviceModel, _DeviceQuery = M.DeviceModel, M.DeviceQuery
GOOD = dict(_from_tree=True, N=9, R=3, _all_leaves=True, _has_kernels=True, _has_factor=True, _loo_done=True, _multi_solved=True)


def _query(Nq=9, **state):
    m = object.__new__(_DeviceModel)         # no constructors: they would create device objects
    m.ctx, m.h, m.P = _Ctx(), None, 2
    for k, v in {**GOOD, **state}.items():
        setattr(m, k, v)
    q = object.__new__(_DeviceQuery)
    q.model, q.L, q.h, q.Nq = m, _Ctx.L, None, Nq
    return q


@pytest.mark.parametrize("Nq, state, text", [
    (9, dict(_from_tree=False), "from_tree"),                   # a list-route model
    (8, {}, "8 points"),                                        # Nq = N - 1
    (9, dict(_all_leaves=False), "shard"),                      # a shard of the leaves
    (9, dict(_has_kernels=False), "no kernels"),
    (9, dict(_loo_done=False), "loo()"),                        # before loo(), or after a new fit
    (9, dict(_multi_solved=False), "solve_multi"),              # before solve_multi, after set_trend or new targets
])
def test_items_loo_multi_is_refused_before_any_device_call(Nq, state, text):
    with pytest.raises(_lib.PmkError, match=text.replace("(", r"\(").replace(")", r"\)")):
        _query(Nq, **state).items_loo_multi()


def test_the_good_state_reaches_the_library():
    """the control of the test above: with every condition met the call goes through to the (absent) library"""
    with pytest.raises(AssertionError, match="pmk_query_items_loo_multi"):
        _query().items_loo_multi()


class _ItemsLib:
    """a library that accepts the items call and records the leading dimension the download is asked with"""

    def __init__(self):
        self.ldu = None

    def pmk_query_items_loo_multi(self, *a):
        return 0

    def pmk_query_get_items_multi(self, h, U, ldu, v):
        self.ldu = ldu
        return 0


def test_item_values_multi_uses_the_columns_of_the_items_run():
    """the library writes R_items columns, those of the items run: targets set again with another R before the download
    do not change the shape, and without an items run on the query the download is refused before any device call"""
    q = _query()
    q.total = 4
    with pytest.raises(_lib.PmkError, match="has run"):
        q.item_values_multi()
    q.L = _ItemsLib()
    q.items_loo_multi()
    q.model.R = 5
    U, v = q.item_values_multi()
    assert U.shape == (4, 3) and v.shape == (4,) and q.L.ldu == 3


class _Lib:
    """a library whose state-changing calls succeed and do nothing"""

    def pmk_model_fit(self, *a):
        return 0

    def pmk_model_set_trend(self, *a):
        return 0

    def pmk_model_set_targets_multi_global(self, *a):
        return 0


@pytest.mark.parametrize("change, text", [
    (lambda m: m.fit(pmk.Spline34KernelType(1.0), 1e-3), r"loo\(\)"),
    (lambda m: m.set_trend("linear"), "solve_multi"),
    (lambda m: m.set_targets_multi_global(np.zeros((9, 2), order="F")), "solve_multi"),
])
def test_a_new_fit_a_new_trend_and_new_targets_make_the_scores_stale(change, text):
    q = _query()
    q.model.ctx.L = _Lib()
    change(q.model)
    q.model.ctx.L = _NoDeviceLib()
    with pytest.raises(_lib.PmkError, match=text):
        q.items_loo_multi()


@pytest.mark.parametrize("fn", ["loomixtureGP_blend_multi", "selectblendGP_multi_"])
def test_module_functions_need_a_fitted_and_solved_tree_model(fn, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(M, "DeviceModel", no_device)
    monkeypatch.setattr(M, "DeviceQuery", no_device)
    wth = pmk.Spline34KernelType(2.0)
    args = {"loomixtureGP_blend_multi": (None, 0.5, 1e-5, wth),
            "selectblendGP_multi_": (None, np.zeros((12, 3)), [(0.5, 1e-5, wth)])}[fn]
    eta = pmk.MixtureGPType([np.zeros((5, 2)), np.zeros((7, 2))], None)
    with pytest.raises(_lib.PmkError, match="fitmixtureGP_ must run"):        # never fitted
        getattr(pmk, fn)(eta, *args)
    eta._model = _query(_from_tree=False).model                               # fitted, but from lists of patches
    with pytest.raises(_lib.PmkError, match="from_tree"):
        getattr(pmk, fn)(eta, *args)
    eta._model = _query(_multi_solved=False, N=12).model                      # fitted by fitmixtureGP_ only
    with pytest.raises(_lib.PmkError, match="fitmixtureGP_multi_ or fitmixtureGP_trend_"):
        getattr(pmk, fn)(eta, *args)
    eta._model = _query(_X_global=None, N=12).model                           # built from a device array, no X passed
    with pytest.raises(_lib.PmkError, match="pass X"):
        getattr(pmk, fn)(eta, *args)


def test_selectblendGP_multi_refuses_bad_arguments():
    eta = pmk.MixtureGPType([np.zeros((5, 2))], None)
    with pytest.raises(ValueError):
        pmk.selectblendGP_multi_(eta, None, np.zeros((5, 2)), [])
    eta._model = _query(N=12).model
    with pytest.raises(ValueError, match="12 x 3"):
        pmk.selectblendGP_multi_(eta, None, np.zeros((12, 2)), [(0.5, 1e-5, pmk.Spline34KernelType(2.0))])


# ------------------------------------------------------------------------------------ 3. the identity against brute force
@pytest.fixture(scope="module")
def oracles():
    X, Y = MR.targets(3)
    cache = {}

    def get(eps, trend):
        if (eps, trend) not in cache:
            cache[(eps, trend)] = MR.MultiOracle(X, Y, eps, [(("s34", BR.A), BR.SIGMA2)], trend)
        return cache[(eps, trend)]
    return get


@pytest.mark.parametrize("trend", MR.TRENDS)
@pytest.mark.parametrize("eps, radius", BR.CASES)
def test_closed_form_against_refits_without_the_point(oracles, eps, radius, trend):
    """Every 7th point, 3 target columns, in fp64 numpy / scipy: every patch that holds j fitted again without it (the
    GLS drift included) and the blended predictor at x_j, against the closed form (member: Y_i - C_i / Q_ii and
    1 / Q_ii - sigma2 with Q_ii = d_i - |L_G^-1 C_H[i]|^2; non-member: the fitted predictor).  Bounds: the solve's forward
    error, |dY| <= cond_2 u max|Y| and |dV| <= cond_2 u (k(0) + sigma2) with u = 2^-53.  Measured: at most 0.0063 and 0.0025
    of the bounds (max |dY| 5.2e-14, max |dV| 3.9e-15), the same with and without a trend."""
    o = oracles(eps, trend)
    wth = O.kernel(O.SPLINE34, 1.0 / radius)
    pts = list(range(0, BR.N, 7))
    total, other, multi, homeless = o.counts(radius)
    assert homeless == 0 and multi >= 1
    assert (other == 0) == (radius <= eps), (eps, radius, other)
    _, MUr, Vr = o.blend(wth, o.items(radius, "refit64", points=pts))
    _, MUc, Vc = o.blend(wth, o.items(radius, "closed64", points=pts))
    ry, rv = MR.ratios(MUc, Vc, MUr, Vr, o.cond2(), 2.0 ** -53, np.abs(o.Y).max(), o.k0() + BR.SIGMA2)
    print("eps %g radius %g trend %s: %d points; ratios to the bounds: mean %.3g, variance %.3g (max |dY| %.3g, |dV| %.3g)"
          % (eps, radius, trend, len(pts), ry, rv, np.abs(MUc - MUr).max(), np.abs(Vc - Vr).max()))
    assert ry <= 1.0 and rv <= 1.0, (ry, rv)


def test_the_trend_matters_for_the_column_with_a_slope(oracles):
    """the workload is no stand-in: with the linear trend the leave-one-out means of column 2 move by far more than the
    bound of the test above, so a device path that ignored the trend would be caught"""
    a, b = oracles(0.3, None), oracles(0.3, "linear")
    wth = O.kernel(O.SPLINE34, 1.0 / 0.6)
    pts = list(range(0, BR.N, 7))
    _, MUa, _ = a.blend(wth, a.items(0.6, "closed64", points=pts))
    _, MUb, _ = b.blend(wth, b.items(0.6, "closed64", points=pts))
    bound = a.cond2() * 2.0 ** -53 * np.abs(a.Y).max()
    assert np.abs(MUa[:, 2] - MUb[:, 2]).max() > 1e3 * bound


def test_recorded_refits_are_the_long_double_refits(oracles):
    """tests/golden/loo_blend_multi_refits.npz against a fresh long-double refit, three rows per (eps, trend): the file
    belongs to this workload and this reference code"""
    for eps in sorted({e for e, _ in BR.CASES}):
        for trend in ("constant", "linear"):
            o = oracles(eps, trend)
            rec = o._recorded()
            assert len(rec) == sum(len(s) for s in o.sets), (eps, trend, len(rec))
            for r, j in [(0, int(o.sets[0][0])), (1, int(o.sets[1][len(o.sets[1]) // 2])), (o.P - 1, int(o.sets[-1][-1]))]:
                mu, v = o.refitref_compute(r, j)
                # a reference for bounds of cond_2 u max|Y| must itself be reproducible far below them
                tol = 1e-3 * o.cond2() * 2.0 ** -53
                assert np.abs(np.asarray(mu, dtype=np.float64) - rec[(r, j)][0]).max() <= tol * np.abs(o.Y).max(), (r, j)
                assert abs(float(v) - rec[(r, j)][1]) <= tol * (o.k0() + BR.SIGMA2), (r, j)

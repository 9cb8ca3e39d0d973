"""CPU-side checks of the blended leave-one-out (no device compute): the header, the ctypes table and the Julia ccalls
agree on the two symbols; the Python functions exist; every refusal of the front end is raised before any device call;
the closed form of tests/_loo_blend_refs.py (the identity the device code implements) agrees with oracle refits without
the point."""
import numpy as np
import pytest

import patchmixturekriging_amd as pmk
from patchmixturekriging_amd import _lib
from patchmixturekriging_amd import mixture as M
from oracle import oracle as O
from test_julia_binding import header_prototypes, julia_ccalls

import _loo_blend_refs as BR

NEW = ["pmk_query_items_loo", "pmk_predict_mixture_loo"]
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
    for name in ("loomixtureGP_blend", "selectblendGP_"):
        assert callable(getattr(pmk, name)), name
    assert callable(pmk.DeviceQuery.items_loo)


# ------------------------------------------------------------------------------------ 2. state rules of the front end
class _NoDeviceLib:
    """stands in for the loaded library: any call into it is a failure of the test"""

    def __getattr__(self, name):
        raise AssertionError("a device call was made: %s" % name)


class _Ctx:
    L = _NoDeviceLib()
    h = None


_DeviceModel, _DeviceQuery = M.DeviceModel, M.DeviceQuery
GOOD = dict(_from_tree=True, N=9, _all_leaves=True, _has_kernels=True, _has_factor=True, _loo_done=True)


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
])
def test_items_loo_is_refused_before_any_device_call(Nq, state, text):
    with pytest.raises(_lib.PmkError, match=text.replace("(", r"\(").replace(")", r"\)")):
        _query(Nq, **state).items_loo()


def test_the_good_state_reaches_the_library():
    """the control of the test above: with every condition met the call goes through to the (absent) library"""
    with pytest.raises(AssertionError, match="pmk_query_items_loo"):
        _query().items_loo()


def test_a_new_fit_makes_the_blended_scores_stale():
    class _Lib:
        def pmk_model_fit(self, *a):
            return 0
    q = _query()
    q.model.ctx.L = _Lib()
    q.model.fit(pmk.Spline34KernelType(1.0), 1e-3)
    q.model.ctx.L = _NoDeviceLib()
    with pytest.raises(_lib.PmkError, match=r"loo\(\)"):
        q.items_loo()


class _OkLib:
    """stands in for the loaded library: every call succeeds and writes nothing"""

    def __getattr__(self, name):
        return lambda *a: 0


MODEL_MIRROR = ("_from_tree", "_all_leaves", "_has_factor", "_has_targets", "_has_kernels", "_loo_done", "_multi_solved",
                "R", "_X", "_X_global", "_index", "theta", "sigma2")
QUERY_MIRROR = ("Xq", "has_diag", "total", "first_owned", "num_owned", "R_items", "variance", "grad_items", "vgrad_items",
                "block_F", "block_variance")


def test_every_birth_of_a_query_carries_the_same_mirror():
    """the constructor, from_items and a bare object.__new__ differ only in what the birth itself knows: the host copy of
    the points and, for from_items, the item counts"""
    m = _query().model
    m.ctx.L, m.D = _OkLib(), 2
    born = {"constructor": _DeviceQuery(m, np.zeros((6, 2))), "from_items": _DeviceQuery.from_items(m, 6, None, None),
            "bare": object.__new__(_DeviceQuery)}
    for how, q in born.items():
        for name in QUERY_MIRROR:
            assert hasattr(q, name), (how, name)
    for name in set(QUERY_MIRROR) - {"Xq", "total", "num_owned"}:
        assert len({getattr(q, name) for q in born.values()}) == 1, name
    assert born["constructor"].Xq.shape == (6, 2) and born["from_items"].Xq is None and born["bare"].Xq is None
    assert (born["constructor"].total, born["constructor"].num_owned) == (0, 0)         # until plan()
    assert (born["from_items"].total, born["from_items"].num_owned) == (6, 6)
    assert born["constructor"].Nq == born["from_items"].Nq == 6
    bare = object.__new__(_DeviceModel)
    for name in MODEL_MIRROR:
        assert hasattr(bare, name), name


@pytest.mark.parametrize("change", [
    lambda m: m.reserve(3),
    lambda m: m._append(np.zeros((1, 2)), np.zeros(1), None, np.array([1], dtype=np.int32), None),
    lambda m: m._remove(np.array([0], dtype=np.int32), np.array([2], dtype=np.int64)),
], ids=["reserve", "append", "remove"])
def test_changed_rows_make_loo_and_the_columns_stale_and_keep_the_factor(change):
    m = _query(_multi_solved=True, R=3, n=np.array([5, 7])).model
    m.ctx.L = _OkLib()
    change(m)
    assert (m._loo_done, m._multi_solved, m.R) == (False, False, 0)
    assert m._has_factor and m._has_kernels


@pytest.mark.parametrize("fn", ["loomixtureGP_blend", "selectblendGP_"])
def test_module_functions_need_a_fitted_tree_model(fn, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(M, "DeviceModel", no_device)
    monkeypatch.setattr(M, "DeviceQuery", no_device)
    wth = pmk.Spline34KernelType(2.0)
    args = {"loomixtureGP_blend": (None, 0.5, 1e-5, wth), "selectblendGP_": (None, np.zeros(12), [(0.5, 1e-5, wth)])}[fn]
    eta = pmk.MixtureGPType([np.zeros((5, 2)), np.zeros((7, 2))], None)
    with pytest.raises(_lib.PmkError, match="fitmixtureGP_ must run"):        # never fitted
        getattr(pmk, fn)(eta, *args)
    eta._model = _query(_from_tree=False).model                               # fitted, but from lists of patches
    with pytest.raises(_lib.PmkError, match="from_tree"):
        getattr(pmk, fn)(eta, *args)
    eta._model = _query(_X_global=None, N=12).model                           # built from a device array, no X passed
    with pytest.raises(_lib.PmkError, match="pass X"):
        getattr(pmk, fn)(eta, *args)


def test_selectblendGP_refuses_an_empty_candidate_list():
    eta = pmk.MixtureGPType([np.zeros((5, 2))], None)
    with pytest.raises(ValueError):
        pmk.selectblendGP_(eta, None, np.zeros(5), [])


# ------------------------------------------------------------------------------------ 3. the identity against brute force
@pytest.fixture(scope="module")
def oracles():
    X, y = BR.workload()
    return {eps: BR.Oracle(X, y, eps, [(("s34", BR.A), BR.SIGMA2)]) for eps in sorted({e for e, _ in BR.CASES})}


@pytest.mark.parametrize("eps, radius", BR.CASES)
def test_closed_form_against_refits_without_the_point(oracles, eps, radius):
    """All 620 points: every patch that holds j refitted without it and query_mixture at x_j, against the closed form
    (member: y_i - c_i / d_i and 1 / d_i - sigma2; non-member: queryinner!).  Bounds: the solve's forward error,
    |dY| <= cond_2 u max|y| and |dV| <= cond_2 u (k(0) + sigma2) with u = 2^-53.  Measured: 0.010 / 0.0023, 0.010 / 0.0023
    and 0.012 / 0.0014 of the bounds (max |dY| 2e-14)."""
    o = oracles[eps]
    wth = O.kernel(O.SPLINE34, 1.0 / radius)
    total, strip, multi, homeless = o.counts(radius)
    assert homeless == 0 and multi >= 1
    assert (strip == 0) == (radius <= eps), (eps, radius, strip)
    assert 0 <= strip < total
    Yr, Vr = o.blend_refit(wth, radius)
    Yc, Vc = o.blend_closed(wth, radius)
    ry, rv = BR.ratios(Yc, Vc, Yr, Vr, o.cond2(), 2.0 ** -53, np.abs(o.y).max(), o.k0() + BR.SIGMA2)
    print("eps %g radius %g: %d items, %d non-members; ratios to the bounds: mean %.3g, variance %.3g"
          % (eps, radius, total, strip, ry, rv))
    assert ry <= 1.0 and rv <= 1.0, (ry, rv)


def test_the_written_out_blend_is_query_mixture(oracles):
    """blend_items (used where query_mixture cannot go: per-patch hyperparameters) against the oracle's query_mixture on
    the fitted model, at every training point: a few roundings of the sums apart"""
    o = oracles[0.3]
    radius = 0.6
    wth = O.kernel(O.SPLINE34, 1.0 / radius)
    home, regs, tss = o.plan(radius)
    Yq, Vq = O.query_mixture(o.bsp, o.th[0], wth, [o.X[s] for s in o.sets], [f["c_chol"] for f in o.fits],
                             [f["L"] for f in o.fits], o.X, radius, BR.DELTA)
    for j in range(0, BR.N, 7):
        uv = [O.queryinner(o.th[int(r)], o.X[o.sets[int(r)]], o.fits[int(r)]["c_chol"], o.fits[int(r)]["L"], o.X[j])
              for r in list(regs[j]) + [home[j]]]
        Y, V = BR.blend_items(wth, tss[j], [a for a, _ in uv], [b for _, b in uv])
        assert abs(Y - Yq[j]) <= 8 * 2.0 ** -53 * max(1.0, abs(Yq[j])) and abs(V - Vq[j]) <= 8 * 2.0 ** -53 * max(Vq[j], 1e-12), j

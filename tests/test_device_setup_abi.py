"""CPU-side checks of the device-resident set-up (no device compute): the header, the ctypes table, the library and the
Julia ccalls agree on the new symbols; the library refuses NULL handles without a device; the Python front end refuses
non-contiguous input, wrong dtypes and shapes, Vq after a mean-only run, closure-carrying kernels and *_global calls on a
model built from lists before any device call."""
import ctypes as C

import numpy as np
import pytest

import patchmixturekriging_amd as pmk
from patchmixturekriging_amd import _lib
from patchmixturekriging_amd import mixture as M
from test_julia_binding import header_prototypes, julia_ccalls

NEW = ["pmk_model_create_from_bsp", "pmk_model_patch_index", "pmk_model_set_targets_global",
       "pmk_model_set_targets_multi_global", "pmk_model_set_diag_global", "pmk_query_fetch_dev", "pmk_query_fetch_multi_dev"]
# what the Julia module binds: MixtureGPType(root, X, eps) and fitmixtureGP!(eta, y, theta, sigma2)
JULIA_BOUND = ["pmk_model_create_from_bsp", "pmk_model_patch_index", "pmk_model_set_targets_global"]

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
    assert protos["pmk_model_create_from_bsp"] == ("i32", ["ptr", "ptr", "i64", "ptr", "ptr", "f64", "i64", "i64", "i32", "ptr"])
    assert protos["pmk_model_patch_index"] == ("i32", ["ptr", "ptr", "ptr", "ptr"])
    assert protos["pmk_model_set_targets_global"] == ("i32", ["ptr", "ptr"])
    assert protos["pmk_model_set_targets_multi_global"] == ("i32", ["ptr", "i32", "ptr", "i64"])
    assert protos["pmk_model_set_diag_global"] == ("i32", ["ptr", "ptr"])
    assert protos["pmk_query_fetch_dev"] == ("i32", ["ptr", "ptr", "ptr"])
    assert protos["pmk_query_fetch_multi_dev"] == ("i32", ["ptr", "ptr", "i64", "ptr"])


def test_julia_ccalls_of_the_new_symbols_match_the_header():
    protos = header_prototypes()
    seen = set()
    for name, ret, args, line in julia_ccalls():
        if name in NEW:
            assert (ret, args) == protos[name], (name, line)
            seen.add(name)
    assert set(JULIA_BOUND) <= seen, sorted(set(JULIA_BOUND) - seen)


def test_the_front_end_exports_the_new_names():
    for name in ("from_tree", "patch_index", "set_targets_global", "set_targets_multi_global", "set_diag_global"):
        assert callable(getattr(pmk.DeviceModel, name)), name
    for name in ("fetch_into", "fetch_multi_into"):
        assert callable(getattr(pmk.DeviceQuery, name)), name
    assert callable(pmk.MixtureGPType.from_tree)


def test_null_arguments_are_refused_by_the_library():
    """NULL model, tree, context or out: a negative status and a text, nothing dereferenced, no device needed"""
    L = pmk.lib()
    X = np.zeros((4, 2))
    root, _, _ = pmk.setuppartition(np.random.default_rng(0).uniform(-1, 1, (16, 2)), 2)
    tree = M._native(root).h
    h = C.c_void_p()

    def refused(rc):
        assert rc < 0, rc
        assert L.pmk_last_error().decode() != ""

    refused(L.pmk_model_create_from_bsp(None, tree, 4, X.ctypes.data, None, -1.0, 0, 0, 0, C.byref(h)))      # no context
    refused(L.pmk_model_create_from_bsp(None, None, 4, X.ctypes.data, None, -1.0, 0, 0, 0, C.byref(h)))      # no tree
    refused(L.pmk_model_create_from_bsp(None, tree, 4, None, None, -1.0, 0, 0, 0, C.byref(h)))               # no points
    assert L.pmk_model_create_from_bsp(None, tree, 4, X.ctypes.data, None, -1.0, 0, 0, 0, None) == -7         # no out
    assert L.pmk_model_create_from_bsp(None, tree, 4, X.ctypes.data, None, -1.0, 0, 0, 7, C.byref(h)) == -8   # dtype
    assert h.value is None
    refused(L.pmk_model_patch_index(None, None, None, None))
    refused(L.pmk_model_set_targets_global(None, X.ctypes.data))
    refused(L.pmk_model_set_targets_multi_global(None, 1, X.ctypes.data, 4))
    refused(L.pmk_model_set_diag_global(None, None))
    refused(L.pmk_query_fetch_dev(None, None, None))
    refused(L.pmk_query_fetch_multi_dev(None, None, 0, None))


# ------------------------------------------------------------------------------------ 2. validation before any device call
class _NoDeviceLib:
    """stands in for the loaded library: any call into it is a failure of the test"""

    def __getattr__(self, name):
        raise AssertionError("a device call was made: %s" % name)


class _Ctx:
    L = _NoDeviceLib()
    h = None


class _DeviceArray:
    """what a torch device tensor shows through __cuda_array_interface__ (never dereferenced here)"""

    def __init__(self, shape, typestr="<f8", strides=None):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (0x1000, False), "version": 2,
                                         "strides": strides}


def _tree(monkeypatch, D=2):
    """a real host tree (pmk_bsp_build has no device part); afterwards every context is the no-device stand-in"""
    root, _, _ = pmk.setuppartition(np.random.default_rng(1).uniform(-1, 1, (64, D)), 3)
    monkeypatch.setattr(M, "default_context", lambda: _Ctx())
    return root


def _model(tree=True, P=4, N=64, **state):
    m = object.__new__(M.DeviceModel)          # no constructor: it would create a device model
    m.ctx, m.h, m.P, m.N, m.D, m.n = _Ctx(), None, P, N, 2, np.full(P, N // P)
    m._from_tree, m._index, m.R = tree, None, 3
    m._has_factor = m._has_targets = m._loo_done = m._multi_solved = m._has_kernels = False
    for k, v in state.items():
        setattr(m, k, v)
    return m


BAD_X = [
    ("non-contiguous rows", lambda: np.zeros((64, 4))[:, :2]),
    ("Fortran order", lambda: np.asfortranarray(np.zeros((64, 2)))),
    ("float32", lambda: np.zeros((64, 2), dtype=np.float32)),
    ("integers", lambda: np.zeros((64, 2), dtype=np.int64)),
    ("a vector", lambda: np.zeros(64)),
    ("the wrong D", lambda: np.zeros((64, 3))),
    ("three axes", lambda: np.zeros((8, 8, 2))),
    ("a list", lambda: [[0.0, 0.0]] * 64),
    ("device float32", lambda: _DeviceArray((64, 2), "<f4")),
    ("device strided", lambda: _DeviceArray((64, 2), strides=(32, 8))),
    ("device wrong D", lambda: _DeviceArray((64, 3))),
]


@pytest.mark.parametrize("what, make", BAD_X, ids=[b[0] for b in BAD_X])
def test_from_tree_refuses_bad_points_before_any_device_call(what, make, monkeypatch):
    root = _tree(monkeypatch)
    with pytest.raises(ValueError):
        M.DeviceModel.from_tree(root, make())
    with pytest.raises(ValueError):
        pmk.MixtureGPType.from_tree(root, make(), eps=0.1)


BAD_Y = [
    ("too short", lambda: np.zeros(63)),
    ("a matrix", lambda: np.zeros((64, 1))),
    ("strided", lambda: np.zeros(128)[::2]),
    ("float32", lambda: np.zeros(64, dtype=np.float32)),
    ("device too long", lambda: _DeviceArray((65,))),
    ("device strided", lambda: _DeviceArray((64,), strides=(16,))),
]


@pytest.mark.parametrize("what, make", BAD_Y, ids=[b[0] for b in BAD_Y])
def test_bad_targets_are_refused_before_any_device_call(what, make, monkeypatch):
    root = _tree(monkeypatch)
    with pytest.raises(ValueError):
        M.DeviceModel.from_tree(root, np.zeros((64, 2)), make())
    with pytest.raises(ValueError):
        _model().set_targets_global(make())
    with pytest.raises(ValueError):
        _model().set_diag_global(make())


def test_from_tree_refuses_bad_options_before_any_device_call(monkeypatch):
    root = _tree(monkeypatch)
    X = np.zeros((64, 2))
    with pytest.raises(ValueError):
        M.DeviceModel.from_tree(root, X, eps=-0.5)
    with pytest.raises(ValueError):
        M.DeviceModel.from_tree(root, X, eps=float("nan"))
    with pytest.raises(ValueError):
        M.DeviceModel.from_tree(root, X, dtype="f16")
    with pytest.raises(ValueError):
        M.DeviceModel.from_tree(root, np.zeros((0, 2)))
    with pytest.raises(_lib.PmkError):
        M.DeviceModel.from_tree(root.left, X)            # not the root that setuppartition returned


@pytest.mark.parametrize("make", [
    lambda: np.zeros((64, 3)),                           # C order: rows are not contiguous columns
    lambda: np.zeros((63, 3), order="F"),                # the wrong N
    lambda: np.zeros((64, 17), order="F"),               # R > PMK_MAX_OUTPUTS
    lambda: np.zeros((64, 0), order="F"),
    lambda: np.zeros((64, 3), dtype=np.float32, order="F"),
    lambda: _DeviceArray((64, 3)),                       # a C-contiguous device matrix
    lambda: _DeviceArray((64, 3), strides=(8, 8 * 60)),  # leading dimension below N
])
def test_bad_multi_targets_are_refused_before_any_device_call(make):
    with pytest.raises(ValueError):
        _model().set_targets_multi_global(make())


def test_multi_targets_pass_their_leading_dimension():
    class _Lib:
        def pmk_model_set_targets_multi_global(self, h, R, ptr, ldy):
            self.got = (R, ptr, ldy)
            return 0
    m = _model(_multi_solved=True)
    m.ctx.L = _Lib()
    big = np.zeros((69, 3), order="F")
    m.set_targets_multi_global(big[:64])                 # N x R inside a column-major block with ldy = N + 5
    assert m.ctx.L.got == (3, big.ctypes.data, 69) and m.R == 3 and not m._multi_solved
    m.set_targets_multi_global(_DeviceArray((64, 2), strides=(8, 8 * 70)))
    assert m.ctx.L.got == (2, 0x1000, 70) and m.R == 2
    m.set_targets_multi_global(np.zeros(64))             # a vector is one column
    assert m.ctx.L.got[0] == 1 and m.ctx.L.got[2] == 64


def test_global_setters_move_the_state_flags_like_the_per_patch_forms():
    class _Lib:
        def pmk_model_set_targets_global(self, h, ptr):
            return 0

        def pmk_model_set_diag_global(self, h, ptr):
            self.diag = ptr
            return 0
    for call in (lambda m: m.set_targets_global(np.zeros(64)), lambda m: m.set_diag_global(np.zeros(64)),
                 lambda m: m.set_diag_global(None)):
        m = _model(_has_factor=True, _loo_done=True, _multi_solved=True)
        m.ctx.L = _Lib()
        call(m)
        assert not m._has_factor and m._loo_done and m._multi_solved     # exactly what set_targets / set_diag do
    assert m.ctx.L.diag is None


@pytest.mark.parametrize("call", [
    lambda m: m.set_targets_global(np.zeros(64)),
    lambda m: m.set_targets_multi_global(np.zeros((64, 2), order="F")),
    lambda m: m.set_diag_global(np.zeros(64)),
    lambda m: m.set_diag_global(None),
    lambda m: m.patch_index(),
])
def test_global_calls_on_a_model_built_from_lists_are_refused_before_any_device_call(call):
    with pytest.raises(_lib.PmkError, match="lists"):
        call(_model(tree=False))


def _query(variance, R=3, Nq=10):
    q = object.__new__(M.DeviceQuery)
    q.model, q.L, q.h, q.Nq = _model(R=R), _NoDeviceLib(), None, Nq
    if variance is not None:
        q.variance = variance
    return q


def test_fetch_into_validates_before_any_device_call():
    q = _query(True)
    for bad in (np.zeros(10), _DeviceArray((9,)), _DeviceArray((10,), "<f4"), _DeviceArray((10,), strides=(16,)),
                _DeviceArray((10, 1))):
        with pytest.raises(ValueError):
            q.fetch_into(bad)
        with pytest.raises(ValueError):
            q.fetch_into(_DeviceArray((10,)), bad)
    for bad in (np.zeros((10, 3), order="F"), _DeviceArray((10, 3)), _DeviceArray((10, 2), strides=(8, 80)),
                _DeviceArray((9, 3), strides=(8, 80)), _DeviceArray((10, 3), strides=(8, 72)), _DeviceArray((10,))):
        with pytest.raises(ValueError):
            q.fetch_multi_into(bad)
    with pytest.raises(ValueError):
        q.fetch_multi_into(_DeviceArray((10, 3), strides=(8, 80)), _DeviceArray((11,)))


@pytest.mark.parametrize("variance", [False, None])
def test_vq_after_a_mean_only_run_is_refused_before_any_device_call(variance):
    q = _query(variance)
    with pytest.raises(ValueError, match="mean-only"):
        q.fetch_multi_into(_DeviceArray((10, 3), strides=(8, 80)), _DeviceArray((10,)))


def _closure_kernels():
    canon = pmk.Spline34KernelType(0.25)
    wf = lambda x: 0.5 * x[0]      # noqa: E731
    return [pmk.AdaptiveKernelType(canon, wf), pmk.AdaptiveKernelDPPType(canon, wf),
            pmk.AdaptiveKernelMultiWarpType(canon, [wf], [1.0]), pmk.AdaptiveKernelMultiWarpDPPType(canon, [wf], [1.0], 0.5),
            pmk.FastAdaptiveKernelType(canon, [wf], None, [1.0])]


@pytest.mark.parametrize("k", range(5))
def test_closure_carrying_kernels_are_refused_on_the_tree_route_before_any_device_call(k):
    bad = _closure_kernels()[k]
    with pytest.raises(TypeError, match="closure"):
        _model().fit(bad, 1e-3)
    eta = object.__new__(pmk.MixtureGPType)
    eta._from_tree, eta._tree_model = True, _model()
    eta._setup(4, None)
    with pytest.raises(TypeError, match="closure"):
        pmk.fitmixtureGP_(eta, np.zeros(64), bad, 1e-3)
    with pytest.raises(TypeError, match="closure"):
        pmk.fitmixtureGP_multi_(eta, np.zeros((64, 2), order="F"), bad, 1e-3)
    with pytest.raises(TypeError):
        pmk.fitmixtureGP_patches_(eta, np.zeros(64), [pmk.Spline34KernelType(1.0)] * 3 + [bad], [1e-3] * 4)

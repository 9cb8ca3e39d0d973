"""CPU-side checks of the multi-output entry points (no device compute): the header, the ctypes table and the Julia
ccalls agree on the new symbols, and the Python front end rejects malformed targets before any device call."""
import numpy as np
import pytest

import patchmixturekriging_amd as pmk
from patchmixturekriging_amd import _lib
from patchmixturekriging_amd import mixture as M
from test_julia_binding import header_prototypes, julia_ccalls

NEW = ["pmk_model_set_targets_multi", "pmk_model_solve_multi", "pmk_model_get_weights_multi", "pmk_query_items_multi",
       "pmk_query_mix_multi", "pmk_query_fetch_multi", "pmk_predict_mixture_multi"]

CTYPES = {"c_int": "i32", "c_int64": "i64", "c_long": "i64", "c_double": "f64"}


def _cat(t):
    name = getattr(t, "__name__", "")
    if name in CTYPES:
        return CTYPES[name]
    return "ptr"


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
    assert "#define PMK_MAX_OUTPUTS 16" in open(pmk._lib.os.path.join(pmk._lib._HERE, "..", "include", "pmk.h")).read()
    assert M.MAX_OUTPUTS == 16


def test_julia_ccalls_of_the_new_symbols_match_the_header():
    protos = header_prototypes()
    seen = set()
    for name, ret, args, line in julia_ccalls():
        if name in NEW:
            assert (ret, args) == protos[name], (name, line)
            seen.add(name)
    # the one-shot entry point is a convenience of the C ABI; the Julia front end uses the staged calls
    assert seen == set(NEW) - {"pmk_predict_mixture_multi"}, sorted(set(NEW) - seen)


class _NoDevice:
    """a MixtureGPType stand-in whose device model must never be touched"""

    def __init__(self, sizes):
        self.X_parts = [np.zeros((n, 2)) for n in sizes]
        self._model = None


@pytest.mark.parametrize("Y_parts", [
    [np.zeros((5, 2)), np.zeros((6, 2))],            # rows do not match the patch sizes
    [np.zeros((5, 17)), np.zeros((7, 17))],          # R > 16
    [np.zeros((5, 0)), np.zeros((7, 0))],            # R = 0
    [np.zeros((5, 2)), np.zeros((7, 3))],            # R differs between patches
    [np.zeros((5, 2))],                              # one patch missing
])
def test_python_validation_before_any_device_call(Y_parts, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(M, "fitmixtureGP_", no_device)
    monkeypatch.setattr(M, "DeviceModel", no_device)
    with pytest.raises(ValueError):
        pmk.fitmixtureGP_multi_(_NoDevice([5, 7]), Y_parts, pmk.Spline34KernelType(1.0), 1e-5)


def test_validation_accepts_vectors_as_one_column():
    Ys = M.multi_targets([np.arange(5.0), np.arange(7.0)], [5, 7])
    assert [y.shape for y in Ys] == [(5, 1), (7, 1)]
    assert all(y.flags.f_contiguous for y in Ys)

"""CPU-side checks of the removal's C ABI (pmk_model_remove / pmk_model_removable): the library exports the symbols
include/pmk.h declares, the Python signatures exist, the version is unchanged, and the refusals that need no device (there
is no model without one, so: a NULL model, whatever else is passed) return their codes and say why."""
import ctypes as C
import os
import re

import numpy as np

import patchmixturekriging_amd as pmk
from patchmixturekriging_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_declared_exported_and_bound():
    L = pmk.lib()
    txt = open(os.path.join(ROOT, "include", "pmk.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("pmk_model_remove", "pmk_model_removable"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES, name
    assert re.search(r"#define\s+PMK_REMOVE_MAX_ROWS\s+(\d+)", code)
    cap = int(re.search(r"#define\s+PMK_REMOVE_MAX_ROWS\s+(\d+)", code).group(1))
    assert cap >= 16 and cap == pmk.mixture.MAX_REMOVE_ROWS
    assert L.pmk_version() == 103
    assert callable(pmk.removemixtureGP_)
    for name in ("removable", "remove", "remove_global"):
        assert callable(getattr(pmk.mixture.DeviceModel, name)), name


def test_refusals_that_need_no_device():
    L = pmk.lib()
    patch = np.zeros(1, dtype=np.int32)
    row = np.zeros(1, dtype=np.int64)
    rows = np.zeros(1, dtype=np.int64)
    pp, rp = patch.ctypes.data_as(C.POINTER(C.c_int32)), row.ctypes.data_as(C.POINTER(C.c_int64))
    assert L.pmk_model_remove(None, 1, pp, rp) == -1
    assert b"pmk_model_remove: model is NULL" in L.pmk_last_error()
    assert L.pmk_model_remove(None, 0, None, None) == -1            # the model comes first, even with nothing to do
    assert L.pmk_model_remove(None, -1, pp, rp) == -1
    assert L.pmk_model_removable(None, rows.ctypes.data_as(C.POINTER(C.c_int64))) == -1
    assert b"pmk_model_removable: NULL argument" in L.pmk_last_error()
    assert rows[0] == 0 and patch[0] == 0 and row[0] == 0

"""CPU-side checks of the C ABI of pmk_model_reserve: the library exports the symbol include/pmk.h declares, the host
sanitizer build has a stand-in for its launcher, the Python signature and the public names exist, the version is
unchanged, the Julia module binds the symbol with the header's types, and the refusals that need no device (there is no
model without one, so: NULL arguments) return their code and say why."""
import ctypes as C
import os
import re

import numpy as np

import patchmixturekriging_amd as pmk
from patchmixturekriging_amd import _lib
import test_julia_binding as JB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "patchmixturekriging_amd", "csrc")


def test_symbol_is_declared_exported_and_bound():
    L = pmk.lib()
    txt = open(os.path.join(ROOT, "include", "pmk.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint\s+pmk_model_reserve\s*\(\s*pmk_model\s*\*\s*m\s*,\s*const\s+int64_t\s*\*\s*rows\s*\)\s*;", code)
    assert hasattr(L, "pmk_model_reserve") and "pmk_model_reserve" in _lib.SIGNATURES
    test_h = open(os.path.join(ROOT, "include", "pmk_test.h")).read()
    assert re.search(r"\bint\s+pmk_test_model_buffers\s*\(", test_h)
    assert hasattr(L, "pmk_test_model_buffers") and "pmk_test_model_buffers" in _lib.SIGNATURES
    assert L.pmk_test_model_buffers(None, None, None, None) == -1
    assert L.pmk_version() == 103
    assert callable(pmk.reservemixtureGP_)
    for name in ("reserve", "capacity"):
        assert callable(getattr(pmk.mixture.DeviceModel, name)), name
    import inspect
    assert "reserve" in inspect.signature(pmk.mixture.DeviceModel.from_tree).parameters
    assert "reserve" in inspect.signature(pmk.MixtureGPType.from_tree).parameters
    assert pmk.mixture.MAX_APPEND_PATCH_ROWS == 128


def test_the_build_knows_the_new_sources():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    for obj in ("pmk_api_reserve.o", "pmk_reserve.o", "f32_pmk_reserve.o"):
        assert obj in mk, obj
    assert "pmk_api_reserve.cpp" in re.search(r"^API_SRCS\s*=(.*)$", mk, flags=re.M).group(1)       # the sanitizer build's list
    stubs = open(os.path.join(CSRC, "pmk_nogpu_stubs.cpp")).read()
    assert re.search(r"\bint\s+launch_reserve\s*\(", stubs)
    internal = open(os.path.join(CSRC, "pmk_internal.h")).read()
    assert re.search(r"\bint\s+launch_reserve\s*\(", internal)


def test_refusals_that_need_no_device():
    L = pmk.lib()
    rows = np.full(3, 7, dtype=np.int64)
    rp = rows.ctypes.data_as(C.POINTER(C.c_int64))
    assert L.pmk_model_reserve(None, rp) == -1
    assert b"pmk_model_reserve: NULL argument" in L.pmk_last_error()
    assert L.pmk_model_reserve(None, None) == -1
    assert np.array_equal(rows, [7, 7, 7])


def test_julia_binds_the_symbol_with_the_headers_types():
    protos = JB.header_prototypes()
    assert protos["pmk_model_reserve"] == ("i32", ["ptr", "ptr"])
    calls = [c for c in JB.julia_ccalls() if c[0] == "pmk_model_reserve"]
    assert len(calls) == 1 and calls[0][1] == "i32" and calls[0][2] == ["ptr", "ptr"]
    code = JB._julia_code()
    assert re.search(r"^\s*function\s+reservemixtureGP!\(", code, flags=re.M)
    exports = re.search(r"^export\s+((?:.|\n)*?)\n\s*\n", code, flags=re.M).group(1)
    assert "reservemixtureGP!" in exports

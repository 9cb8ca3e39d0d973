"""The ABI of the block draws without a device: every new symbol is declared, exported and bound with the header's argument
categories, the refusals that need no device return their codes, the front ends know their methods, and the Julia module
binds the calls (checked statically by tests/test_julia_binding.py; here only that they are there)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import patchmixturekriging_amd as pmk
from patchmixturekriging_amd import _lib
from patchmixturekriging_amd import mixture as M
from test_julia_binding import JL, header_prototypes

NEW = ["pmk_query_items_cov_blocks", "pmk_query_factor_cov", "pmk_query_factor_info", "pmk_query_get_items_cov_factor",
       "pmk_query_draw"]


def _cat(t):
    if t in (C.c_int, C.c_int32):
        return "i32"
    if t is C.c_int64:
        return "i64"
    if t is C.c_double:
        return "f64"
    return "ptr"


def test_every_new_symbol_is_declared_exported_and_bound():
    protos = header_prototypes()
    L = pmk.lib()
    for name in NEW:
        assert name in protos and hasattr(L, name) and name in _lib.SIGNATURES, name
        ret, args = _lib.SIGNATURES[name]
        assert (_cat(ret), [_cat(a) for a in args]) == protos[name], name
    jl = open(JL, encoding="utf-8").read()
    for name in NEW:
        assert re.search(r"ccall\(\(:%s,\s*libpmk\)" % name, jl), name
    assert "samplemixtureGP_blocks" in jl


def test_refusals_that_need_no_device():
    L = pmk.lib()
    th = pmk.Spline34KernelType(1.0).desc()
    z = np.zeros(4)
    assert L.pmk_query_items_cov_blocks(None, C.byref(th), 0) == -1 and b"pmk_query_items_cov_blocks" in L.pmk_last_error()
    assert L.pmk_query_factor_cov(None, None) == -1 and b"pmk_query_factor_cov" in L.pmk_last_error()
    assert L.pmk_query_factor_info(None, None, None) == -1 and b"pmk_query_factor_info" in L.pmk_last_error()
    assert L.pmk_query_get_items_cov_factor(None, 0, None, None, 0) == -1
    assert b"pmk_query_get_items_cov_factor" in L.pmk_last_error()
    assert L.pmk_query_draw(None, C.byref(th), 1, z.ctypes.data, 4, z.ctypes.data, 4) == -1
    assert b"pmk_query_draw" in L.pmk_last_error()
    assert L.pmk_query_draw(None, C.byref(th), 0, None, 0, None, 0) == -1           # no plan comes before n_draws = 0


def test_the_front_ends_know_their_methods():
    for fn in (pmk.samplemixtureGP, pmk.samplemixtureGP_multi):
        with pytest.raises(ValueError, match="method"):
            fn(None, None, None, 3, 0.5, 1e-5, None, 1, method="sparse")
    for name in ("items_cov_blocks", "factor_cov", "factor_info", "item_cov_factor", "draw"):
        assert callable(getattr(M.DeviceQuery, name)), name


def test_the_documents_name_the_new_calls():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    integration = open(os.path.join(root, "INTEGRATION.md"), encoding="utf-8").read()
    for name in NEW:
        assert name in integration, name
    assert "pmk_draw.hip" in open(os.path.join(root, "DESIGN.md"), encoding="utf-8").read()

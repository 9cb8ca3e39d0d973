"""The ABI of block kriging without a device: every new symbol is declared, exported and bound with the header's argument
categories, the refusals that need no device return their codes, the front ends exist with their signatures, and the
Julia module binds the calls (their argument tuples are checked statically by tests/test_julia_binding.py)."""
import ctypes as C
import inspect
import os
import re

import numpy as np

import patchmixturekriging_amd as pmk
from patchmixturekriging_amd import _lib
from patchmixturekriging_amd import mixture as M
from test_draw_abi import _cat
from test_julia_binding import JL, header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["pmk_query_items_block", "pmk_query_fetch_block", "pmk_query_fetch_block_dev", "pmk_query_get_items_block",
       "pmk_predict_mixture_block_fitted"]


def test_every_new_symbol_is_declared_exported_and_bound():
    protos = header_prototypes()
    L = pmk.lib()
    for name in NEW:
        assert name in protos and hasattr(L, name) and name in _lib.SIGNATURES, name
        ret, args = _lib.SIGNATURES[name]
        assert (_cat(ret), [_cat(a) for a in args]) == protos[name], name
    jl = open(JL, encoding="utf-8").read()
    for name in ("pmk_query_items_block", "pmk_query_fetch_block", "pmk_predict_mixture_block_fitted"):
        assert re.search(r"ccall\(\(:%s,\s*libpmk\)" % name, jl), name
    assert re.search(r"^export(?:.|\n)*?querymixtureGP_block", jl, flags=re.M) and "function querymixtureGP_block(" in jl
    header = open(os.path.join(ROOT, "include", "pmk.h"), encoding="utf-8").read()
    assert re.search(r"#define\s+PMK_BLOCK_MAX_MEMBERS\s+4096\b", header)


def test_refusals_that_need_no_device():
    L = pmk.lib()
    th = pmk.Spline34KernelType(1.0).desc()
    g, a, y = np.zeros(4, dtype=np.int32), np.ones(4), np.zeros(4)
    gp = g.ctypes.data_as(C.POINTER(C.c_int32))
    assert L.pmk_query_items_block(None, C.byref(th), C.byref(th), 1, gp, M._d(a), 1) == -1
    assert b"pmk_query_items_block" in L.pmk_last_error()
    assert L.pmk_query_fetch_block(None, M._d(y), 4, None) == -1 and b"pmk_query_fetch_block" in L.pmk_last_error()
    assert L.pmk_query_fetch_block_dev(None, None, 4, None) == -1
    assert L.pmk_query_get_items_block(None, None, None, None, None, None, None, None, None, None) == -1
    assert b"pmk_query_get_items_block" in L.pmk_last_error()
    assert L.pmk_predict_mixture_block_fitted(None, C.byref(th), 4, M._d(y), 0.5, 1e-5, 1, gp, M._d(a), M._d(y), 1, None) == -1


def test_the_front_ends_and_their_signatures():
    for name in ("items_block", "fetch_block", "fetch_block_into", "item_blocks"):
        assert callable(getattr(M.DeviceQuery, name)), name
    assert list(inspect.signature(pmk.querymixtureGP_block).parameters) == \
        ["Xq", "group", "a", "eta", "root", "levels", "radius", "delta", "weight_theta", "variance"]
    assert inspect.signature(pmk.querymixtureGP_block).parameters["variance"].default is True
    assert list(inspect.signature(M.DeviceQuery.items_block).parameters)[:4] == ["self", "group", "a", "weight_theta"]


def test_the_documents_and_the_build_name_the_new_code():
    design = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
    readme = open(os.path.join(ROOT, "README.md"), encoding="utf-8").read()
    assert "pmk_block.hip" in design and "querymixtureGP_block" in readme and "tests/test_gpu_block.py" in readme
    mk = open(os.path.join(ROOT, "patchmixturekriging_amd", "csrc", "Makefile"), encoding="utf-8").read()
    assert mk.count("pmk_block.o") == 4 and mk.count("pmk_api_block.o") == 2           # both object lists, both element types
    stubs = open(os.path.join(ROOT, "patchmixturekriging_amd", "csrc", "pmk_nogpu_stubs.cpp"), encoding="utf-8").read()
    for name in ("launch_items_block", "launch_block_weights", "launch_block_heads", "launch_block_aggregates",
                 "launch_block_reduce", "launch_cov_trend_items"):
        assert name in stubs, name

"""Shared by the multi-output edge tests (tests/test_gpu_multi_edges.py): the parameters of multi_solve_kernel and
item_means_kernel (csrc/pmk_multi.hip), the host rule that deals a region's items into chunks, and the references.

As in tests/_query_refs.py the parameters are READ from the sources and every rule restated here in Python is asserted,
at import, to be still present verbatim in the source (whitespace aside): a changed chunk size, k-step or workgroup
shape makes the tests fail instead of leaving their edge cases beside the edges.  Needs no GPU."""
import os
import re

import numpy as np
import scipy.linalg as sla

from oracle import oracle as O
from _query_refs import CSRC, TILE, device_constant, kappa, restates, source_text  # noqa: F401  (re-exported)

LD = np.longdouble


def header_define(name):
    """the value of `#define NAME <integer>` in include/pmk.h"""
    with open(os.path.join(CSRC, "..", "..", "include", "pmk.h")) as f:
        m = re.search(r"^#define\s+%s\s+(\d+)\b" % name, f.read(), re.M)
    assert m, name
    return int(m.group(1))


IM_THREADS = device_constant("IM_THREADS", "pmk_multi.hip")     # item_means_kernel: one wave per chunk
MS_THREADS = device_constant("MS_THREADS", "pmk_multi.hip")     # multi_solve_kernel: one workgroup per patch
PMK_MAX_OUTPUTS = header_define("PMK_MAX_OUTPUTS")              # columns of a block: targets plus trend basis
restates("pmk_multi.hip", "constexpr int RP = PMK_MAX_OUTPUTS;")

# chunks_of: the host prefix over the regions, and what a wave makes of its chunk index
restates("pmk_api.cpp", "(q->roff[(size_t)r + 1] - q->roff[(size_t)r] + 15) / 16")
restates("pmk_multi.hip",
         "const int64_t first = roff[r] + (g - cpre[r]) * 16;",
         "const int count = (int)min((int64_t)16, roff[r + 1] - first);")
CHUNK = 16                                                      # items of a full chunk (the 16 rows of the MFMA's A operand)
# workgroup_of: IM_THREADS / 64 consecutive chunks per workgroup (xcd_remap permutes workgroups, not their contents)
restates("pmk_multi.hip",
         "const int64_t g = (int64_t)xcd_remap((int)blockIdx.x, (int)gridDim.x) * (IM_THREADS / 64) + wave;",
         "const unsigned grid = (unsigned)((q->mchunks + IM_THREADS / 64 - 1) / (IM_THREADS / 64));")
WAVES = IM_THREADS // 64
# the walk over the patch: 8 rows per step, two MFMA k-steps of 4
restates("pmk_multi.hip", "for (int k0 = 0; k0 < n; k0 += 8)", "const int ka = k0 + lg, kb = k0 + 4 + lg;")
KSTEP = 8


def chunks_of(counts):
    """item_means_kernel's chunks for the per-region item counts, in launch order: (region, items in the chunk).  A region
    with c items has ceil(c / 16) chunks, all full but the last; an empty region has none (a repeated entry of the
    chunk prefix)"""
    out = []
    for r, c in enumerate(counts):
        c = int(c)
        out += [(r, min(CHUNK, c - f)) for f in range(0, c, CHUNK)]
    return out


def workgroup_of(chunk):
    """the workgroup (before xcd_remap) whose wave chunk % WAVES serves this chunk"""
    return chunk // WAVES


def item_means_reference(oth, X, C, xq):
    """kq . C[:, j] for every query row and column in numpy.longdouble from the oracle's cross_kernel_matrix (fp64 values
    widened, so exact products and a long-double sum), and the scale S[i, j] = sum_k |kq_ik| |C_kj|.
    -> mu [m, R] (long double), S [m, R] (float64), Kq [m, n]"""
    C = np.asarray(C, dtype=np.float64)
    if C.ndim == 1:
        C = C[:, None]
    Kq = O.cross_kernel_matrix(oth, np.atleast_2d(xq), X)          # m x n
    mu = np.asarray(Kq, dtype=LD) @ np.asarray(C, dtype=LD)
    return mu, np.abs(Kq) @ np.abs(C), Kq


def lapack_weights(U, Y):
    """U^-1 Y by LAPACK's Cholesky solve in fp64"""
    return sla.solve(U, Y, assume_a="pos")


def rel_residual(U, Cm, Y):
    """|U C - Y|_F / (|U|_F |C|_F), the figure of tests/test_gpu_multi_output.py"""
    return float(np.linalg.norm(U @ Cm - Y) / (np.linalg.norm(U) * np.linalg.norm(Cm)))

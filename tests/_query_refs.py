"""Shared by the GPU predict tests (tests/test_gpu_query_edges.py, tests/test_gpu_family_parity.py): the predict path's
size thresholds, the host-side rules that pick its branches (strip dealing, scan blocks, sort blocks, live rows of the
last block row), and the fp64 references (CPU oracle, numpy, scipy).

The thresholds are READ from the HIP sources.  The rules are expressions, so they are restated here in Python; the
source text each restates is asserted, at import, to be still present verbatim in the HIP source (whitespace aside).
Either way a change of the device's parameters or rules makes the tests fail instead of leaving them vacuous."""
import os
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import scipy.linalg as sla

from oracle import oracle as O

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "patchmixturekriging_amd", "csrc")
NTHREADS = 8
_SRC = {}


def source_text(source):
    """csrc/<source> with every run of whitespace collapsed to one blank"""
    if source not in _SRC:
        with open(os.path.join(CSRC, source)) as f:
            _SRC[source] = " ".join(f.read().split())
    return _SRC[source]


def device_constant(name, source):
    """the value of `constexpr int NAME = <integer>;` in csrc/<source>"""
    m = re.search(r"constexpr\s+int\s+[^;]*\b%s\s*=\s*(\d+)\s*[,;]" % name, source_text(source))
    assert m, (name, source)
    return int(m.group(1))


def restates(source, *texts):
    """the device code that a rule below restates is still in csrc/<source>, verbatim"""
    for text in texts:
        assert " ".join(text.split()) in source_text(source), (source, text)


def _scan_pass():
    """block sums scan_offsets_kernel takes per pass: its loop step, which must equal its LDS array"""
    body = source_text("pmk_kernels.hip").split("void scan_offsets_kernel", 1)[1].split("__global__", 1)[0]
    step = re.findall(r"b0 \+= (\d+)\)", body)
    sh = re.findall(r"__shared__ int64_t sh\[(\d+)\]", body)
    assert len(step) == 1 and sh == step, (step, sh)
    return int(step[0])


TILE = device_constant("TILE", "pmk_internal.h")                          # factor tile edge (rows of a block row)
TQ = device_constant("TQ", "pmk_internal.h")                              # query columns of a strip task
WCOLS = device_constant("WCOLS", "pmk_predict.hip")                       # query columns of one wave of a strip
PLAN_LDS_NODES = device_constant("PLAN_LDS_NODES", "pmk_kernels.hip")     # plan_kernel<.., LDS = true> up to this many nodes
PLAN_STAGE = device_constant("PLAN_STAGE", "pmk_kernels.hip")             # neighbour hits the fill pass copies
SORT_LDS_BINS = device_constant("SORT_LDS_BINS", "pmk_kernels.hip")       # sort_hist_lds_kernel up to this many regions
restates("pmk_kernels.hip", "SCAN_BLOCK = 256 * SCAN_PER_THREAD;")
SCAN_BLOCK = 256 * device_constant("SCAN_PER_THREAD", "pmk_kernels.hip")  # entries per block of the prefix scan
SCAN_PASS = _scan_pass()                                                  # block sums scan_offsets_kernel takes per pass

restates("pmk_predict.hip",                                               # strip_counts: build_strip_tasks
         "const int64_t nstrips = (e - b + TQ - 1) / TQ, w = (e - b + nstrips - 1) / nstrips;",
         "for (int64_t f = b; f < e; f += w) {",
         "t.count = (int32_t)((e - f) < w ? (e - f) : w);")
restates("pmk_predict.hip", "const int last_pairs = (pd.n - (pd.nt - 1) * TILE + 31) >> 5;")     # last_pairs
restates("pmk_api.cpp", "d.nt = (int32_t)((n[r] + TILE - 1) / TILE);")
restates("pmk_kernels.hip", "const int64_t nb = (n + 1 + SCAN_BLOCK - 1) / SCAN_BLOCK;")          # scan_blocks
restates("pmk_kernels.hip", "const int bitems = (int)std::max<int64_t>(1024, 64 * ((2 * P + 63) / 64));",  # sort_block_items
         "if (P <= SORT_LDS_BINS) {")


def strip_counts(cnt):
    """build_strip_tasks' dealing rule for one region with cnt items: nstrips = ceil(cnt / TQ) strips of
    w = ceil(cnt / nstrips) columns, the last one the remainder"""
    if cnt <= 0:
        return []
    nstrips = -(-cnt // TQ)
    w = -(-cnt // nstrips)
    return [min(w, cnt - f) for f in range(0, cnt, w)]


def strip_tasks(region_counts):
    """the column counts of every strip task of a plan (regions in order)"""
    return [c for n in region_counts for c in strip_counts(int(n))]


def last_pairs(n):
    """32-row pairs of the last block row of an n-point patch that are not identity padding (predict_strip_kernel)"""
    nt = -(-n // TILE)
    return (n - (nt - 1) * TILE + 31) >> 5


def scan_blocks(Nq):
    """blocks of the prefix scan over the Nq + 1 item offsets (exclusive_scan_i32_to_i64)"""
    return -(-(Nq + 1) // SCAN_BLOCK)


def sort_block_items(P):
    """items per block of the counting sort (launch_sort_items)"""
    return max(1024, 64 * ((2 * P + 63) // 64))


def kappa(U):
    ev = np.linalg.eigvalsh(U)
    assert ev[0] > 0, ev[0]
    return float(ev[-1] / ev[0])


def oracle_fits(oth, X_set, ys, sigma2):
    """fitmixtureGP! of the oracle, patch by patch (LU weights, Cholesky factor); every info must be 0"""
    with ThreadPoolExecutor(NTHREADS) as ex:
        fits = list(ex.map(lambda a: O.fit_patch(oth, a[0], a[1], sigma2), zip(X_set, ys)))
    assert all(f["info"] == 0 for f in fits)
    return fits


def oracle_mixture(ob, oth, owth, X_set, fits, Xq, radius, delta):
    """querymixtureGP! of the oracle with debug outputs -> Yq, Vq, home, nb offsets, nb regions, nb t"""
    return O.query_mixture(ob, oth, owth, X_set, [f["c_lu"] for f in fits], [f["L"] for f in fits], Xq, radius, delta,
                           debug=True, nthreads=NTHREADS)


def oracle_plan(ob, Xq, radius, delta):
    """home, nb offsets, nb regions, nb t of the oracle's querymixtureGP! alone: every patch is a one-point stand-in
    (c = 0, L = 1), which the integer outputs and t do not depend on"""
    D = ob.D
    Xs = [np.zeros((1, D))] * ob.P
    _, _, home, off, reg, ts = O.query_mixture(ob, O.kernel(O.SPLINE34, 1.0), O.kernel(O.SPLINE34, 1.0), Xs,
                                               [np.zeros(1)] * ob.P, [np.ones((1, 1))] * ob.P, Xq, radius, delta,
                                               debug=True, nthreads=NTHREADS)
    return home, off, reg, ts


def assert_plan_matches(dbg, ohome, ooff, oreg, ots, what=""):
    """home leaf, item offsets (the device's carry the home item last: one more per query), neighbour regions and t of
    every query bit for bit; reports the first differing query"""
    off = dbg["item_offsets"]
    bad = np.nonzero(dbg["home"] != ohome)[0]
    assert len(bad) == 0, "%s home: %d queries differ, first %d: %d vs oracle %d" % (
        what, len(bad), bad[0], dbg["home"][bad[0]], ohome[bad[0]])
    dcount = np.diff(off) - 1
    bad = np.nonzero(dcount != np.diff(ooff))[0]
    assert len(bad) == 0, "%s neighbour count: %d queries differ, first %d: %d vs oracle %d" % (
        what, len(bad), bad[0], dcount[bad[0]], np.diff(ooff)[bad[0]])
    assert np.array_equal(off - np.arange(len(off)), ooff), what    # every offset, exactly: off[j] = ooff[j] + j
    nb = np.ones(off[-1], bool)
    nb[off[1:] - 1] = False                                      # the home item is last per query
    reg, t = dbg["item_region"], dbg["item_t"]
    bad = np.nonzero((reg[nb] != oreg) | (t[nb] != ots))[0]
    if len(bad):
        j = int(np.searchsorted(ooff, bad[0], side="right") - 1)
        raise AssertionError("%s neighbours: %d items differ, first of query %d: (%d, %r) vs oracle (%d, %r)" % (
            what, len(bad), j, reg[nb][bad[0]], t[nb][bad[0]], oreg[bad[0]], ots[bad[0]]))
    assert np.array_equal(reg[~nb], ohome) and np.all(t[~nb] == 0.0), what


def assert_fp64_values(Yq, Vq, oY, oV, what=""):
    """|dYq| <= 1e-7 max(1, |Yq|), |dVq| <= 1e-9 + 1e-5 Vq; a NaN anywhere is out of bounds"""
    by = ~(np.abs(Yq - oY) <= 1e-7 * np.maximum(1, np.abs(oY)))
    bv = ~(np.abs(Vq - oV) <= 1e-9 + 1e-5 * oV)
    for name, bad, a, b in (("Yq", by, Yq, oY), ("Vq", bv, Vq, oV)):
        j = np.nonzero(bad)[0]
        assert len(j) == 0, "%s %s: %d queries out of bounds, first %d: %r vs oracle %r" % (what, name, len(j), j[0],
                                                                                           a[j[0]], b[j[0]])


def queryinner_reference(oth, X, c, L, Xq, qdiag=None):
    """queryinner! for a block of queries on the given factors: mu = k.c, var = max(k(x,x) + addend - |L^-1 k|^2, 1e-12),
    and the scales the fp32 bounds use (|k|.|c|, k(x,x) + |L^-1 k|^2)"""
    K = O.cross_kernel_matrix(oth, X, Xq)                      # n x nq
    W = sla.solve_triangular(L, K, lower=True, check_finite=False)
    kxx = np.array([O.kernel_eval(oth, x, x) for x in Xq])
    if qdiag is not None:
        kxx = kxx + qdiag
    w2 = np.einsum("ij,ij->j", W, W)
    return K.T @ c, np.maximum(kxx - w2, 1e-12), np.abs(K).T @ np.abs(c), np.abs(kxx) + w2


def blend_reference(dbg, per_item_u, per_item_v):
    """querymixtureGP!'s blend of per-item values with the device's weights: Yq = w.u, Vq = w.(v w), w normalised"""
    Y, V = np.empty(len(dbg["home"])), np.empty(len(dbg["home"]))
    off = dbg["item_offsets"]
    for j in range(len(Y)):
        s = slice(off[j], off[j + 1])
        w = dbg["item_w"][s] / dbg["item_w"][s].sum()
        Y[j], V[j] = w @ per_item_u[s], w @ (per_item_v[s] * w)
    return Y, V


def seq_sumsq(z, p):
    """the oracle's distance (norm2_diff): the sequential sum of squares of z - p, before its one sqrt"""
    s = None
    for a, b in zip(z, p):
        r = float(a) - float(b)
        s = r * r if s is None else s + r * r
    return s

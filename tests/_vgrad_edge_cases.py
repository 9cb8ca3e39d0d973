"""Inputs of the variance-gradient edge tests (tests/test_vgrad_edges_refs.py on the CPU, tests/test_gpu_vgrad_edges.py on
the GPU): host data only, built here once per process, so that what the CPU file asserts of an input (the schedule of the
strips, the clamp decisions and their margin, the one-unit and kappa2 conditions of tests/_vgrad_refs.py) holds of the
input the GPU file runs.  The blends of group D run on the workloads of tests/_grad_edge_cases.py.

  A. more strips than workgroups: eight regions with patches of A_SIZES points and item counts that give 2 ncu + 3 strips;
  B. one patch of separated points with a tiny sigma2, where k(x,x) - b falls below min_v = 1e-12 on a training point;
  C. the trend's sibling kernel at R = 1 and R = 16 - q, item lists of 1 .. 257 items in chunks of 16, patches of 5, 6 and
     7 block rows.
"""
import numpy as np

import _vgrad_refs as VR
from _loo_refs import LD, backward_ld, cholesky_ld, forward_ld
from test_gpu_grad import FAMILIES, _round

TILE = 128                                                   # rows of a block row
MIN_V = 1e-12                                                # the clamp of the query ABI


def strip_cap(D):
    """items of one strip of vgrad_strip_kernel: vgrad_strip_items of pmk_internal.h"""
    return 8 * 2 * (16 // (D + 1))


def block_rows(n):
    return (n + TILE - 1) // TILE


class TrendRef(VR.PatchRef):
    """PatchRef(th, X, sigma2, trend) on the long-double factor `base` already holds: no second Cholesky of the patch"""

    def __init__(self, base, trend):
        self.__dict__.update(base.__dict__)
        H = np.hstack([np.ones((self.n, 1), dtype=LD)] + ([self.X] if trend == "linear" else []))
        self.C_H = backward_ld(self.L, forward_ld(self.L, H))
        G = H.T @ self.C_H
        self.LG = cholesky_ld((G + G.T) / LD(2))
        self.q = self.C_H.shape[1]
        self._kappa = None


_REFS = {}


def patch_ref(key, oth, X, sigma2, trend=None):
    """the long-double reference of one patch, built once per process under (key, trend); the trended references share
    the factor of the plain one"""
    if (key, None) not in _REFS:
        _REFS[(key, None)] = VR.PatchRef(oth, X, sigma2)
    if (key, trend) not in _REFS:
        _REFS[(key, trend)] = TrendRef(_REFS[(key, None)], trend)
    return _REFS[(key, trend)]


def region_points(seed, r, X, cnt, dtype):
    """cnt query points of region r as VR.case_items draws them (around the patch, the first on a training point), from a
    generator of its own: the first k points do not depend on cnt.  Its rule for a one-point patch holds here for every
    patch of fewer than 16 points: query k lies within half a unit per coordinate of point k mod n.  Seven points in
    [-2, 2]^4 are as alone as one: a query 2.3 away from the nearest of them sits at the edge of the support, where the
    error unit does not see the lost digits of t = 1 - r, and a plain evaluation reaches 1.9 units there."""
    rng = np.random.default_rng([seed, r])
    D = X.shape[1]
    if len(X) < 16:
        pts = X[np.arange(cnt) % len(X)] + rng.uniform(-0.5, 0.5, (cnt, D))
    else:
        pts = rng.uniform(-2.5, 2.5, (cnt, D))
    if cnt:
        pts[0] = X[len(X) // 2]
    return _round(pts, dtype)


def items_of(seed, Xs, counts, dtype):
    """(xq [m, D], region [m]) of region_points, region after region"""
    xq = np.vstack([region_points(seed, r, Xs[r], c, dtype) for r, c in enumerate(counts)])
    return xq, np.repeat(np.arange(len(counts), dtype=np.int32), counts)


def ends_and_middle(counts):
    """indices into the item list: the first, the middle and the last item of every region"""
    first = np.concatenate([[0], np.cumsum(counts)])
    return np.array(sorted({int(first[r]) + k for r, c in enumerate(counts) if c for k in (0, c // 2, c - 1)}), dtype=np.int64)


# ------------------------------------------------------------------------------------ A. more strips than workgroups
A_SIZES = [641, 7, 257, 1, 300, 129, 40, 128]               # nt 6, 1, 3, 1, 3, 2, 1, 1
A_ONE_ITEM_ENDS = (0, 2, 5)                                  # regions whose last strip holds one item: seven idle waves
A_CASES = [(1, "f64", None), (4, "f64", None), (2, "f32", None), (4, "f64", "linear")]
A_NCU = (64, 256, 304)                                       # the chip sizes the CPU file asserts the schedule for
A_SEED = 1200


def a_patches(D, dtype):
    rng = np.random.default_rng(900 + D)
    return [_round(rng.uniform(-2, 2, (n, D)), dtype) for n in A_SIZES]


def a_counts(ncu, D):
    """items per region: 2 ncu + 3 strips dealt evenly to the eight regions; the regions of A_ONE_ITEM_ENDS end on a
    strip of one item, the last region on half a strip, every other strip is full"""
    cap = strip_cap(D)
    base, extra = divmod(2 * ncu + 3, 8)
    strips = [base + (1 if r < extra else 0) for r in range(8)]
    counts = [(s - 1) * cap + 1 if r in A_ONE_ITEM_ENDS else s * cap for r, s in enumerate(strips)]
    counts[7] -= cap // 2
    return counts


def strip_prefix(counts, D):
    """strips per region as a prefix, as pmk_query_items_vgrad computes it"""
    cap = strip_cap(D)
    pre = [0]
    for c in counts:
        pre.append(pre[-1] + (c + cap - 1) // cap)
    return pre


def schedule(counts, sizes, D, ncu):
    """what launch_items_vgrad and the task loop of vgrad_strip_kernel make of the item counts: min(strips, ncu)
    workgroups, workgroup b runs the strips b, b + grid, b + 2 grid, ... -> dict(strips, grid, most_tasks, nt_down, nt_up,
    full_after_one): the most tasks of a workgroup, and how many consecutive task pairs of one workgroup go from a patch
    of more block rows to one of fewer, the other way, and from a one-item strip to a full one"""
    cap, pre = strip_cap(D), strip_prefix(counts, D)
    T = pre[-1]
    grid = min(T, ncu)
    region = np.repeat(np.arange(len(counts)), np.diff(pre))
    items = np.concatenate([np.minimum(cap, c - cap * np.arange((c + cap - 1) // cap)) for c in counts]).astype(np.int64)
    nt = np.array([block_rows(sizes[r]) for r in region])
    assert len(region) == len(items) == T and items.sum() == sum(counts) and items.min() >= 1
    g = np.arange(max(T - grid, 0))
    return dict(strips=int(T), grid=int(grid), most_tasks=int((T + grid - 1) // grid), nt_down=int((nt[g] > nt[g + grid]).sum()),
                nt_up=int((nt[g] < nt[g + grid]).sum()), full_after_one=int(((items[g] == 1) & (items[g + grid] == cap)).sum()))


def a_pieces(counts, D, ncu, pieces=3):
    """cuts of the item list into `pieces` parts at items that are no strip boundaries; every part alone has at most ncu
    strips, so that each of its workgroups runs one task"""
    total = sum(counts)
    cuts = [0] + [k * total // pieces + 7 for k in range(1, pieces)] + [total]
    first = np.concatenate([[0], np.cumsum(counts)])
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        part = [int(min(hi, first[r + 1]) - max(lo, first[r])) for r in range(len(counts))]
        assert strip_prefix([max(c, 0) for c in part], D)[-1] <= ncu
    return list(zip(cuts[:-1], cuts[1:]))


# ------------------------------------------------------------------------------------ B. the clamp
B_FAMILIES = [("spline34", "f64"), ("spline34", "f32"), ("spline32", "f64")]
# sigma2 of the separated patch, through fit_patches.  On a training point k(x,x) - b = sigma2 / (1 + sigma2), and r
# supports off it 56/3 r^2 more (Spline34): with sigma2 = 1e-13 that is 1.0002e-13 at r = 1e-9, a hair above min_v / 10;
# 5e-14 leaves the factor 10 on both sides of min_v for every item
B_SIGMA2 = {"f64": 5e-14, "f32": 1e-9}
# The matrix the device factors.  fp64: 1 + 5e-14 is a double next to the exact sum.  fp32: 1 + 1e-9 rounds to 1, the
# diagonal is k(0) = 1 exactly, and the reference takes sigma2 = 0 (tests/test_vgrad_edges_refs.py asserts the rounding)
B_REF_SIGMA2 = {"f64": 5e-14, "f32": 0.0}
B_OFF = {"f64": 1e-3, "f32": 0.05}                           # "well inside a support", in supports
B_PATCH = 7                                                  # the separated patch; the others are VR.case_patches
B_COUNTS = [5, 3, 17, 4, 6, 9, 2, 0]                         # items of the ordinary patches
CLAMPED, INSIDE, OUTSIDE = 0, 1, 2


def separated_lattice(support):
    """13 x 10 = 130 points (two block rows, last_pairs 1) at a spacing of three supports; point 65 is the origin, where
    an offset of 1e-9 supports survives the rounding to float32"""
    i, j = np.meshgrid(np.arange(13) - 6, np.arange(10) - 5, indexing="ij")
    return np.ascontiguousarray(3.0 * support * np.stack([i.ravel(), j.ravel()], 1).astype(np.float64))


def b_inputs(family, dtype):
    """(Xs, xq, region, kind): eight patches at D = 2, the last one separated; the items of the ordinary patches first,
    then those of the separated patch with their kind: on a training point or 1e-9 supports off one (CLAMPED), B_OFF
    supports off one (INSIDE), outside every support (OUTSIDE)"""
    support = 1.0 / FAMILIES[family][1].p[0]
    Xs = VR.case_patches(1100, 2, dtype)
    Z = separated_lattice(support)
    Xs[B_PATCH] = Z
    xq, region = VR.case_items(1101, Xs, B_COUNTS, dtype)
    e = lambda a: np.array([np.cos(a), np.sin(a)])
    pts, kind = [], []
    for k in (3, 65, 128, 129):                              # first and last block row
        pts.append(Z[k]); kind.append(CLAMPED)
    for k, a in ((65, 0.7), (65, 3.9), (129, 2.2), (3, 5.1)):
        pts.append(Z[k] + 1e-9 * support * e(a)); kind.append(CLAMPED)
    for k, a in ((65, 1.1), (128, 0.3), (40, 4.0), (129, 2.9)):
        pts.append(Z[k] + B_OFF[dtype] * support * e(a)); kind.append(INSIDE)
    for p in (Z[65] + 1.5 * support, Z[0] + np.array([1.5 * support, 0.0]), Z[129] + 1.01 * support * e(0.4),
              np.array([500.0, -300.0]) * support):
        pts.append(p); kind.append(OUTSIDE)
    xq = np.vstack([xq, _round(np.array(pts), dtype)])
    region = np.concatenate([region, np.full(len(pts), B_PATCH, dtype=np.int32)])
    return Xs, xq, region, np.array(kind)


# the blend: the lattice workload "grid" of tests/_grad_edge_cases.py (spacing 1/4) under a model kernel of support 1/5
B_BLEND_THETA = 5.0
B_BLEND_SIGMA2 = 1e-13


def plan_items(wl, dtype):
    """(xq [m, D], region [m]) of the items the oracle's plan gives the queries of a workload: per query its neighbour
    regions in hyperplane order, then its home"""
    Xq = _round(wl.Xq, dtype)
    xq, region = [], []
    for j, s in enumerate(wl.plan()):
        for r in list(s[1]) + [s[0]]:
            xq.append(Xq[j])
            region.append(int(r))
    return np.array(xq), np.array(region, dtype=np.int32)


def plain_mix_vgrad(items, GV, v, t, plane, hp_v, wth):
    """_vgrad_refs.mix_vgrad_ref in plain float64 numpy: what a careful evaluation of the blend in the device's own
    precision gives -> (dVq [D], mag2 [D]).  mag2 is the magnitude of mix_vgrad_ref taken BEFORE the cancellation in
    dwn_i = (dw_i - wn_i sum_j dw_j) / S:  sum_i (|wn_i^2 GV_i| + |2 wn_i v_i| (|dw_i| + wn_i sum_j |dw_j|) / S).
    On a lattice two parallel planes at t and -t give slopes dw that cancel in sum_j dw_j to the last bits; the rounding
    of each dw (phi and psi in double) then reaches dVq through the home item's term, whose own magnitude is zero: the
    bound 16 m 2^-53 mag of the blend does not see it, and no evaluation in double can meet it there."""
    items = list(items)
    tt = np.asarray(t, dtype=np.float64)[items]
    w = VR.GR.phi(wth, np.abs(tt))
    w[-1] = 1.0
    S = w.sum()
    wn = w / S
    nv = np.zeros((len(items), np.asarray(hp_v).shape[1]))
    for k, it in enumerate(items[:-1]):
        nv[k] = hp_v[plane[it]]
    dw = -(VR.GR.psi(wth, np.abs(tt)) * tt)[:, None] * nv
    dw[-1] = 0.0
    dwn = (dw - wn[:, None] * dw.sum(0)[None, :]) / S
    a = (wn * wn)[:, None] * np.asarray(GV, dtype=np.float64)[items]
    c = 2.0 * wn * np.asarray(v, dtype=np.float64)[items]
    mag2 = (np.abs(a) + np.abs(c)[:, None] * (np.abs(dw) + wn[:, None] * np.abs(dw).sum(0)[None, :]) / S).sum(0)
    return (a + c[:, None] * dwn).sum(0), mag2


# ------------------------------------------------------------------------------------ C. columns, chunks, block rows
C_COUNTS = [5, 3, 17, 4, 6, 9, 0, 2]                         # those of tests/test_gpu_vgrad.py


def trend_q(trend, D):
    return {None: 0, "constant": 1, "linear": 1 + D}[trend]


# (D, dtype, trend, R): R = 1 and R = 16 - q, the first and the last place of the q trend columns in the 16-column block
C_COLUMN_CASES = [(2, "f64", "linear", 1), (2, "f64", "linear", 13), (4, "f64", "linear", 1), (4, "f64", "linear", 11),
                  (2, "f64", "constant", 15), (4, "f64", "constant", 1), (4, "f64", "constant", 15), (2, "f32", "linear", 1),
                  (2, "f32", "linear", 13), (4, "f32", "linear", 11), (4, "f32", "constant", 15), (2, "f32", "constant", 1)]


def c_column_inputs(D, dtype):
    """patches and items of the column cases: those of VR.case_patches / VR.case_items, one set per (D, dtype)"""
    Xs = VR.case_patches(1300 + D, D, dtype)
    xq, region = VR.case_items(1310 + D, Xs, list(np.roll(C_COUNTS, D)), dtype)
    return Xs, xq, region


C_CHUNK_SIZES = [129, 40, 130, 7, 257, 128, 33, 131]         # of test_items_keep_their_bits_whatever_shares_their_strip
C_CHUNK_CASES = [(2, "f64"), (4, "f64"), (2, "f32")]
# its item counts and 15, 16, 17, six to a batch; two further regions bring every batch above 32 chunks of 16 items
C_CHUNK_BATCHES = [[1, 47, 48, 49, 63, 64, 150, 90], [20, 0, 65, 79, 80, 81, 127, 128], [129, 161, 0, 30, 257, 15, 16, 17]]
C_EDGE_COUNTS = [1, 47, 48, 49, 63, 64, 65, 79, 80, 81, 127, 128, 129, 161, 257, 15, 16, 17]


def chunk_count(counts):
    """chunks of 16 items per region, summed: the waves item_trend_grads_kernel deals, four to a workgroup"""
    return sum((c + 15) // 16 for c in counts)


def c_chunk_patches(D, dtype):
    rng = np.random.default_rng(500 + D)
    return [_round(rng.uniform(-2, 2, (n, D)), dtype) for n in C_CHUNK_SIZES]


C_ROW_SIZES = [513, 7, 641, 40, 896, 1, 33, 129]             # nt 5, 6, 7 and last_pairs 1, 1, 4 on the patches 0, 2, 4
C_ROW_COUNTS = [5, 0, 17, 0, 9, 0, 0, 3]
C_ROW_CASES = [("f64", None), ("f64", "linear"), ("f32", None)]


def c_row_inputs(dtype):
    rng = np.random.default_rng(1400)
    Xs = [_round(rng.uniform(-2, 2, (n, 2)), dtype) for n in C_ROW_SIZES]
    xq, region = VR.case_items(1401, Xs, C_ROW_COUNTS, dtype)
    return Xs, xq, region

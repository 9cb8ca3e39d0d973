"""Inputs of the joint-covariance edge tests (tests/test_cov_edges_refs.py on the CPU, tests/test_gpu_cov_edges.py on the
GPU): host data only, built here once per process, so that what the CPU file asserts of an input (the schedule of the
strips, the block rows and last-row pairs, the twins, kappa2(L) <= 10^3 and a plain evaluation below one error unit) holds
of the input the GPU file runs.  The blends of group C run on the workloads of tests/_grad_edge_cases.py, the draws of
group D on the main workload of tests/_cov_cases.py.

  A. a tree of 1024 leaves whose patches cycle through classes of one, two, three and six block rows; one item in most
     regions, 256, 257 and 513 in a few: more strips than any chip has compute units, so that a workgroup of
     cov_strip_kernel runs several tasks of different depth and fill;
  B. eight patches of 5, 6 and 7 block rows (and two of one) with every count of last-row pairs, item counts on the wave
     (32), Gram piece (64) and strip (256) boundaries.
"""
import numpy as np

import patchmixturekriging_amd as pmk

import _cov_cases as CC

TILE = 128                                                   # rows of a block row
TQ = CC.TQ                                                   # items of a strip
MIN_V = 1e-12                                                # the clamp of the query ABI


def block_rows(n):
    return (n + TILE - 1) // TILE


def last_pairs(n):
    """32-row pairs of the last block row that are not identity padding (cov_strip_kernel)"""
    return (n - (block_rows(n) - 1) * TILE + 31) >> 5


def cov_tasks(counts):
    """cov_tasks_from_plan (pmk_api_query.cpp) restated: the strips of every region in region order, a region's items
    dealt evenly over ceil(m / 256) strips -> (region, items) of every task"""
    region, items = [], []
    for r, m in enumerate(counts):
        if m == 0:
            continue
        nstrips = (m + TQ - 1) // TQ
        w = (m + nstrips - 1) // nstrips
        for f in range(0, m, w):
            region.append(r)
            items.append(min(m - f, w))
    return np.array(region, dtype=np.int64), np.array(items, dtype=np.int64)


def schedule(counts, sizes, ncu):
    """what launch_items_cov and the task loop of cov_strip_kernel make of the item counts: slots = min(ntasks, ncu)
    workgroups, workgroup b runs the tasks b, b + slots, b + 2 slots, ... -> the number of consecutive task pairs of one
    workgroup that go from a patch of nt >= 5 to one of nt = 1 (deep_to_one), the other way (one_to_deep), from a full
    strip to a strip of one item (full_to_single), the other way (single_to_full), and across a change of the parity of
    nt (parity: the ring of two point tiles starts on the other tile)"""
    region, items = cov_tasks(counts)
    T = len(region)
    slots = min(T, ncu)
    nt = np.array([block_rows(sizes[r]) for r in region])
    g = np.arange(max(T - slots, 0))
    a, b = g, g + slots
    return dict(ntasks=int(T), slots=int(slots), most_tasks=int((T + slots - 1) // slots),
                deep_to_one=int(((nt[a] >= 5) & (nt[b] == 1)).sum()), one_to_deep=int(((nt[a] == 1) & (nt[b] >= 5)).sum()),
                full_to_single=int(((items[a] == TQ) & (items[b] == 1)).sum()),
                single_to_full=int(((items[a] == 1) & (items[b] == TQ)).sum()),
                parity=int(((nt[a] - nt[b]) % 2 == 1).sum()))


def schedule_ok(s, ncu):
    return (s["ntasks"] >= 2 * ncu + 3 and s["slots"] == ncu and min(s["deep_to_one"], s["one_to_deep"], s["full_to_single"],
                                                                     s["single_to_full"], s["parity"]) >= 1)


# ------------------------------------------------------------------------------------ A. several strips per workgroup
A_LEVELS, A_P = 11, 1024
A_CYCLE = [1, 7, 40, 128, 129, 257, 300, None]              # None: 641 points in 16 of the regions, 90 in the others
A_DEEP, A_SHALLOW = 641, 90
A_VARIANTS = 3                                               # point sets per class: regions r, r + 64, r + 256, r + 304 differ
# items of the regions that hold more than one: full strips on patches of 1, 641 (six block rows) and 129 points, pairs
# of 129 + 128 items on 7 and 300 points, three strips of 171 on 90 and 257 points
A_HEAVY = {150: 256, 263: 257, 411: 256, 598: 513, 647: 256, 806: 257, 932: 513}
A_CASES = [(2, "f64", False), (1, "f64", False), (4, "f32", False), (2, "f64", True)]  # D, dtype, mixed families
A_NCU = (64, 256, 304)
A_PIECE = 32                                                 # regions of a sub-query of the bits check
A_MIXED = ["spline34", "gaussian", "rq", "spline12"]
A_SEED = 1700


def a_class(r):
    """the size class of region r: the cycle, shifted so that the regions a workgroup of 64, 256 or 304 runs one after
    the other fall in different classes"""
    return (r + r // 16 + r // 128) % 8


def a_variant(r):
    return (r // 8) % A_VARIANTS


def a_sizes():
    sizes, seen = [], 0
    for r in range(A_P):
        n = A_CYCLE[a_class(r)]
        if n is None:
            n = A_DEEP if seen % 8 == 3 else A_SHALLOW
            seen += 1
        sizes.append(n)
    return sizes


def a_counts():
    return [A_HEAVY.get(r, 1) for r in range(A_P)]


def a_set_key(r, sizes=None):
    """regions of one (class, variant, size) share a point set, and a long-double factor: 27 sets for 1024 patches"""
    n = (sizes or a_sizes())[r]
    return (a_class(r), a_variant(r), n)


def a_family(key, mixed):
    return A_MIXED[(key[0] + key[1]) % len(A_MIXED)] if mixed else "spline34"


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def a_tree(D):
    """1024 leaves, as test_gpu_grad._tree8 builds its eight: explicit items name their regions"""
    return _cached(("a_tree", D), lambda: pmk.setuppartition(np.random.default_rng(5).uniform(-4, 4, (2 * A_P, D)), A_LEVELS)[0])


def a_patches(D, dtype):
    def make():
        sizes = a_sizes()
        sets = {}
        for r in range(A_P):
            key = a_set_key(r, sizes)
            if key not in sets:
                rng = np.random.default_rng([A_SEED, D, key[0], key[1], key[2]])
                sets[key] = CC.rnd(rng.uniform(-2, 2, (key[2], D)), dtype)
        return [sets[a_set_key(r, sizes)] for r in range(A_P)]
    return _cached(("a_patches", D, dtype), make)


def region_points(rng, X, cnt, dtype):
    """cnt query points of a region as _cov_cases.edge_items draws them: around the patch, within half a unit per
    coordinate of its points where it has fewer than 16; the first of two or more on a training point"""
    D = X.shape[1]
    if len(X) < 16:
        pts = X[np.arange(cnt) % len(X)] + rng.uniform(-0.5, 0.5, (cnt, D))
    else:
        pts = rng.uniform(-2.5, 2.5, (cnt, D))
    if cnt >= 2:
        pts[0] = X[len(X) // 2]
    return CC.rnd(pts, dtype)


def a_items(D, dtype):
    """(xq [m, D], region [m]) in a shuffled order"""
    def make():
        Xs, counts = a_patches(D, dtype), a_counts()
        xq = np.vstack([region_points(np.random.default_rng([A_SEED + 1, D, r]), Xs[r], c, dtype) for r, c in enumerate(counts)])
        region = np.repeat(np.arange(A_P, dtype=np.int32), counts)
        perm = np.random.default_rng(A_SEED + 2 + D).permutation(len(region))
        return np.ascontiguousarray(xq[perm]), np.ascontiguousarray(region[perm])
    return _cached(("a_items", D, dtype), make)


def a_checked_regions():
    """the regions whose blocks meet the long-double reference: nt >= 2, every eighth of the others, and the heavy ones"""
    sizes = a_sizes()
    return [r for r in range(A_P) if block_rows(sizes[r]) >= 2 or r % 8 == 0 or r in A_HEAVY]


def a_pieces():
    return [(lo, lo + A_PIECE) for lo in range(0, A_P, A_PIECE)]


# ------------------------------------------------------------------------------------ B. depth, dimension, strip counts
B_SIZES = [513, 672, 673, 864, 865, 896, 64, 33]
B_NT = [5, 6, 6, 7, 7, 7, 1, 1]
B_PAIRS = [1, 1, 2, 3, 4, 4, 2, 2]
B_COUNTS = [31, 32, 33, 63, 64, 65, 512, 96]
B_CASES = [(1, "f64", "spline34"), (4, "f64", "spline34"), (4, "f32", "spline34"), (1, "f64", "gaussian")]
B_TWO_STRIPS = 6                                             # the region of two full strips
B_SEED = 1800


def b_patches(D, dtype):
    return _cached(("b_patches", D, dtype),
                   lambda: [CC.rnd(np.random.default_rng([B_SEED, D, r]).uniform(-2, 2, (n, D)), dtype) for r, n in enumerate(B_SIZES)])


def b_items(D, dtype):
    return _cached(("b_items", D, dtype), lambda: CC.edge_items(b_patches(D, dtype), B_COUNTS, dtype, B_SEED + 10 + D))


# ------------------------------------------------------------------------------------ C. the blend
C_NQ_EDGES = [1, 15, 16, 17, 33]
# name of the input -> (workload of _grad_edge_cases, plan radius or None for the workload's own)
C_INPUTS = {"many_mid": ("many", 0.8), "many_wide": ("many", 10.0), "polygon": ("polygon", None), "L7_D4": ("L7_D4", None),
            "on_plane": ("on_plane", None), "grid": ("grid", None), "dups": ("dups", None), "radius_0": ("base2", 0.0),
            "radius_1e300": ("base2", 1e300), "base2_f32": ("base2_f32", None)}


def plan_items(plan):
    """(item_offsets, item_region, item_t) of a plan of _grad_edge_cases.Workload.plan: per query its neighbours in
    hyperplane order, home last"""
    off, reg, t = [0], [], []
    for home, regs, _, ts in plan:
        reg += [int(r) for r in regs] + [int(home)]
        t += [float(v) for v in ts] + [0.0]
        off.append(len(reg))
    return np.array(off, dtype=np.int64), np.array(reg, dtype=np.int64), np.array(t)


def twin_groups(Xq):
    """lists of query indices (two or more, ascending) whose points are equal in every coordinate"""
    seen = {}
    for j, x in enumerate(np.asarray(Xq)):
        seen.setdefault(x.tobytes(), []).append(j)
    return [g for g in seen.values() if len(g) > 1]


# ------------------------------------------------------------------------------------ D. draws
def corner_queries(m):
    """the eight queries of test_gpu_cov.test_posterior_draws, around the corner where the four leaves of the main
    workload meet"""
    centre = np.mean([x.mean(0) for x in m.Xs], 0)
    return centre + np.random.default_rng(9).uniform(-0.5, 0.5, (8, 2))


def jitter_ladder(scale):
    """the jitters samplemixtureGP may return for a covariance of trace / Nq = scale: 0.0, then 2^-52 scale times 10^k up
    to 2^-26 scale"""
    out, j = [0.0], 2.0 ** -52 * scale
    while j <= 2.0 ** -26 * scale:
        out.append(j)
        j = 10.0 * j
    return out

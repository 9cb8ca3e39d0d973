"""Named, deterministic, tiny point sets on which the geometry code decides exactly AT its comparisons: projections equal
to a hyperplane offset, tied projections, pairs exactly on a kernel's support radius, empty leaves.  Shared by
tests/test_oracle_bsp.py (host against the oracle, CPU) and tests/test_gpu_degenerate_geometry.py (device against host).

Every coordinate is a small multiple of a power of two, so sums, differences and squared distances of lattice points are
exact in fp64 and "on the plane" / "on the radius" are statements about integers."""
import numpy as np

H = 0.25
MODES = [(1, 0), (-1, 0), (1, 1)]                        # (sign_mode, dot_mode)
EPS_LIST = [0.0, H, 0.3, float("inf"), float("nan"), 1e300, -0.1]


def lattice(nx, ny, h=H):
    """nx x ny points of spacing h centred on the origin, x slowest"""
    xs = (np.arange(nx) - (nx - 1) / 2.0) * h
    ys = (np.arange(ny) - (ny - 1) / 2.0) * h
    gx, gy = np.meshgrid(xs, ys, indexing="ij")
    return np.ascontiguousarray(np.stack([gx.ravel(), gy.ravel()], 1))


def lattice_steps(nx, ny):
    """the same points as integers: twice the offset from the centre in steps of h (exact for even and odd counts)"""
    gx, gy = np.meshgrid(2 * np.arange(nx) - (nx - 1), 2 * np.arange(ny) - (ny - 1), indexing="ij")
    return np.stack([gx.ravel(), gy.ravel()], 1).astype(np.int64)


def collinear():
    k = np.arange(-128, 129, dtype=np.float64)
    return np.ascontiguousarray(np.stack([0.25 * k, 0.125 * k], 1))


def flat3d():
    X = lattice(25, 20)
    return np.ascontiguousarray(np.concatenate([X, np.full((len(X), 1), 0.5)], 1))


def pm0_1d():
    return np.array([-0.0, 0.0] * 10 + list(range(-20, 21)), dtype=np.float64)[:, None]


def _repeat(points, times):
    return np.ascontiguousarray(np.tile(np.asarray(points, dtype=np.float64), (times, 1)))


def dups5():
    return _repeat([[0.0, 0.0], [1.0, 0.5], [-0.5, 1.25], [2.0, -1.0], [-1.5, -2.25]], 100)


def dups3():
    return _repeat([[0.0, 0.0], [1.0, 0.5], [-0.5, 1.25]], 50)


def dups2():
    return _repeat([[0.0, 0.0], [1.0, 0.5]], 50)


def allsame():
    return _repeat([[0.75, -1.25]], 64)


def small_n():
    return np.array([[0.0, 0.0], [1.0, 0.5], [-0.5, 1.25], [2.0, -1.0], [-1.5, -2.25]])


# name -> (points, levels): trees that build
BUILDS = {
    "lattice33x31": (lattice(33, 31), 4),                # odd counts everywhere: points ON hyperplanes, c = +-0
    "lattice32x32": (lattice(32, 32), 4),                # 1024 points: exactly one pairwise-summation block at the root
    "lattice33x32": (lattice(33, 32), 4),                # 1056 > 1024: two summation blocks at the root
    "lattice65x63": (lattice(65, 63), 6),
    "collinear": (collinear(), 4),
    "flat3d": (flat3d(), 4),
    "pm0_1d": (pm0_1d(), 3),                             # -0.0 and +0.0 tie around the median
    "dups5": (dups5(), 4),                               # empty leaves at the last level
}
# name -> (points, levels, status, text of the refusal, first empty node of the oracle, its depth)
REFUSED = {
    "dups2": (dups2(), 4, -3, "BSP node 0 at depth 2 has no points", 0, 2),
    "dups3": (dups3(), 4, -3, "BSP node 0 at depth 2 has no points", 0, 2),
    "allsame": (allsame(), 3, -3, "BSP node 0 at depth 1 has no points", 0, 1),
    "small_n": (small_n(), 5, -4, "N=5 < 2^(levels-1)", 0, 3),     # refused by its size, before the build would find the node
}


def eps_list(name):
    """pm0_1d also takes eps = 0.5 and 1.0, where e == c +- eps holds exactly for integer points"""
    return EPS_LIST + ([0.5, 1.0] if name == "pm0_1d" else [])


def bits(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a.view(np.uint64)


def projections(v, c, X, dot_mode):
    """e = dot(v, x) of every point against every hyperplane as the tree computes it (sequential; products and sums
    either separate or fused) -> (nodes, N).  The fused form rounds the exact a*b + s once (float(Fraction) rounds
    correctly)."""
    from fractions import Fraction
    X = np.asarray(X, dtype=np.float64)
    out = np.empty((len(c), len(X)))
    for k in range(len(c)):
        s = v[k][0] * X[:, 0]
        for d in range(1, X.shape[1]):
            if dot_mode:
                a = Fraction(float(v[k][d]))
                s = np.array([float(a * Fraction(float(x)) + Fraction(float(t))) for x, t in zip(X[:, d], s)])
            else:
                s = s + v[k][d] * X[:, d]
        out[k] = s
    return out

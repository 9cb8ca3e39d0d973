"""Oracle BSP (partition.jl) vs the independent Python restatement in tests/golden and the
invariants the reference asserts in its examples.  CPU only."""
import numpy as np
import pytest
from hypothesis import given, settings, strategies as st

from oracle import oracle as O


@pytest.mark.parametrize("name", ["bsp_2d.npz", "bsp_3d.npz"])
def test_bsp_matches_golden_bit_exact(golden, name):
    g = golden(name)
    b = O.BSP(g["X"], int(g["levels"]))
    v, c = b.hyperplanes()
    assert np.array_equal(v, g["hp_v"]) and np.array_equal(c, g["hp_c"])
    off, inds = b.leaves()
    assert np.array_equal(off, g["leaf_off"]) and np.array_equal(inds, g["leaf_inds"])
    soff, sinds, loff, lists = b.assign(g["X"], float(g["eps"]))
    assert np.array_equal(soff, g["set_off"]) and np.array_equal(sinds, g["set_inds"])
    assert np.array_equal(loff, g["list_off"]) and np.array_equal(lists, g["lists"])
    home = np.array([b.findpartition(x) for x in g["Xq"]])
    assert np.array_equal(home, g["home"])
    nb_reg, nb_t, nb_off = [], [], [0]
    for x, h in zip(g["Xq"], home):
        reg, ts, zs, keep = b.neighbours(x, float(g["radius"]), float(g["delta"]), h)
        nb_reg += list(reg); nb_t += list(ts[keep]); nb_off.append(len(nb_reg))
    assert np.array_equal(nb_off, g["nb_off"]) and np.array_equal(nb_reg, g["nb_reg"])
    assert np.array_equal(nb_t, g["nb_t"])


def test_reference_invariants():
    rng = np.random.default_rng(3)
    X = rng.uniform(-1, 1, (3000, 2))
    levels = 6
    b = O.BSP(X, levels)
    v, c = b.hyperplanes()
    off, inds = b.leaves()
    # patchGP_partitioning.jl:198  #hyperplanes == #leaves - 1
    assert len(c) == b.P - 1 == 2 ** (levels - 1) - 1
    # every point in exactly one leaf, ascending original indices (mask indexing keeps order)
    assert sorted(inds.tolist()) == list(range(len(X)))
    for l in range(b.P):
        seg = inds[off[l]:off[l + 1]]
        assert np.all(np.diff(seg) > 0)
        # leaf of its own points (partition.jl:151-153 sanity assertion analogue)
        assert all(b.findpartition(X[i]) == l for i in seg[:5])
    # patchGP_partitioning.jl:214-215: |z - p| == |t| within 1e-10 (unit normals)
    p = np.array([0.1, 0.16])
    home = b.findpartition(p)
    reg, ts, zs, keep = b.neighbours(p, 0.3, 1e-5, home)
    d = np.linalg.norm(zs[keep] - p, axis=1)
    assert np.linalg.norm(d - np.abs(ts[keep])) < 1e-10
    assert np.abs(np.linalg.norm(v, axis=1) - 1).max() < 4e-16
    assert home not in reg
    # eps = 0 assignment reproduces the leaves except for points exactly on a plane
    soff, sinds, loff, lists = b.assign(X, 0.0)
    on_plane = len(X) - (loff[1:] - loff[:-1]).sum()
    assert on_plane >= 0 and np.all(np.diff(loff) <= 1)


def test_first_point_quirk_and_split_sizes():
    # partition.jl:89-94: the normal is (X[1]-mean)/|.| of the node's FIRST point, not PCA
    rng = np.random.default_rng(5)
    X = rng.normal(size=(1000, 3))
    b = O.BSP(X, 2)
    v, c = b.hyperplanes()
    z = X[0] - O.mean_pairwise(X)
    assert np.allclose(v[0], z / np.linalg.norm(z), rtol=0, atol=2e-16)
    off, _ = b.leaves()
    assert np.array_equal(np.diff(off), [500, 500])       # even N: exact halves
    b = O.BSP(X[:999], 2)
    off, _ = b.leaves()
    assert np.array_equal(np.diff(off), [499, 500])       # odd N: the median point goes right


def test_preorder_and_leaf_order():
    # dev/btree_easy.jl:56-68: left before right; pre-order = root, left subtree, right subtree
    rng = np.random.default_rng(9)
    X = rng.uniform(0, 1, (64, 2))
    b3 = O.BSP(X, 3)
    v3, c3 = b3.hyperplanes()
    b2 = O.BSP(X, 2)
    v2, c2 = b2.hyperplanes()
    assert np.array_equal(v3[0], v2[0]) and c3[0] == c2[0]
    off, inds = b2.leaves()
    left = O.BSP(X[inds[off[0]:off[1]]], 2).hyperplanes()
    right = O.BSP(X[inds[off[1]:off[2]]], 2).hyperplanes()
    assert np.array_equal(v3[1], left[0][0]) and c3[1] == left[1][0]
    assert np.array_equal(v3[2], right[0][0]) and c3[2] == right[1][0]


def test_mean_median_stdlib_semantics():
    rng = np.random.default_rng(11)
    X = rng.normal(size=(5000, 2)) * 1e3
    mu = O.mean_pairwise(X)
    # pairwise: split at mid, blocks <= 1024 summed left to right
    def pw(a):
        if len(a) <= 1024:
            s = a[0] + a[1]
            for x in a[2:]:
                s = s + x
            return s
        mid = (len(a) - 1) >> 1
        return pw(a[:mid + 1]) + pw(a[mid + 1:])
    assert np.array_equal(mu, pw(list(X)) / len(X))
    assert O.median([3.0, 1.0, 2.0]) == 2.0
    assert O.median([1e308, 1e308]) == 1e308              # a/2 + b/2 does not overflow
    assert O.median([1.0, 2.0, 4.0, 8.0]) == 3.0


@settings(max_examples=25, deadline=None)
@given(st.integers(0, 2**31), st.integers(2, 3), st.integers(2, 5))
def test_assign_band_property(seed, D, levels):
    rng = np.random.default_rng(seed)
    N = 40 * 2 ** (levels - 1)
    X = rng.uniform(-1, 1, (N, D))
    b = O.BSP(X, levels)
    eps = 0.07
    soff, sinds, loff, lists = b.assign(X, eps)
    # every point lists its own leaf, regions ascending, X_set_inds ascending (partition.jl:323-345)
    for n in range(0, N, 7):
        l = lists[loff[n]:loff[n + 1]]
        assert b.findpartition(X[n]) in l and np.all(np.diff(l) > 0)
    for r in range(b.P):
        assert np.all(np.diff(sinds[soff[r]:soff[r + 1]]) > 0)
    off, _ = b.leaves()
    assert np.all(np.diff(soff) >= np.diff(off))


# ------------------------------------------------------------------------------------ gridded, collinear, duplicated points
# The host build and eps-assignment (pmk_bsp.cpp, which the GPU tests hold the device to) against the oracle on inputs
# where projections EQUAL hyperplane offsets, tie with one another, or leave leaves empty: tests/_degenerate.py.
import patchmixturekriging_amd as pmk
from patchmixturekriging_amd import partition as PT

import _degenerate as G

_TREES = {}


def _trees(name, sign_mode, dot_mode):
    """host tree and oracle tree of one input in one mode pair, built once"""
    key = (name, sign_mode, dot_mode)
    if key not in _TREES:
        X, levels = G.BUILDS[name]
        root, _, inds = pmk.setuppartition(X, levels, sign_mode=sign_mode, dot_mode=dot_mode)
        _TREES[key] = (root, inds, O.BSP(X, levels, sign_mode=sign_mode, dot_mode=dot_mode))
    return _TREES[key]


@pytest.mark.parametrize("sign_mode,dot_mode", G.MODES)
@pytest.mark.parametrize("name", list(G.BUILDS))
def test_degenerate_build_host_vs_oracle(name, sign_mode, dot_mode):
    X, levels = G.BUILDS[name]
    root, inds, ob = _trees(name, sign_mode, dot_mode)
    hv, hc = PT.hyperplane_arrays(root)
    ov, oc = ob.hyperplanes()
    assert np.array_equal(G.bits(hv), G.bits(ov))
    assert np.array_equal(hc, oc) and np.array_equal(np.signbit(hc), np.signbit(oc))
    assert np.array_equal(G.bits(hc), G.bits(oc))          # a zero offset is +0.0 on both sides
    assert not np.any(np.signbit(hc) & (hc == 0))
    off, oi = ob.leaves()
    assert np.array_equal(np.cumsum([0] + [len(i) for i in inds]), off) and np.array_equal(np.concatenate(inds), oi)
    E = G.projections(ov, oc, X, dot_mode)
    on_plane, zero_c, empty = int((E == oc[:, None]).sum()), int((oc == 0).sum()), int((np.diff(off) == 0).sum())
    print("%s (%d, %d): %d (point, plane) pairs with e == c, %d offsets equal to zero, %d empty leaves, leaf sizes %s"
          % (name, sign_mode, dot_mode, on_plane, zero_c, empty, np.diff(off).tolist() if levels < 6 else "..."))
    assert on_plane > 0                                      # every input puts points exactly on a hyperplane
    if name in ("lattice33x31", "pm0_1d", "collinear"):
        assert zero_c > 0
    if name == "dups5":
        assert np.array_equal(np.diff(off), [0, 100, 0, 100, 0, 100, 100, 100])
    else:
        assert empty == 0


@pytest.mark.parametrize("sign_mode,dot_mode", G.MODES)
@pytest.mark.parametrize("name", list(G.BUILDS))
def test_degenerate_eps_assignment_host_vs_oracle(name, sign_mode, dot_mode):
    X, levels = G.BUILDS[name]
    root, _, ob = _trees(name, sign_mode, dot_mode)
    ov, oc = ob.hyperplanes()
    E = G.projections(ov, oc, X, dot_mode)
    N, P = len(X), ob.P
    for eps in G.eps_list(name):
        X_set, X_set_inds, regions, _ = pmk.organizetrainingsets(root, levels, X, eps)
        soff, sinds, loff, lists = ob.assign(X, eps)
        assert np.array_equal(np.cumsum([0] + [len(i) for i in X_set_inds]), soff)
        assert np.array_equal(np.concatenate(X_set_inds), sinds)
        assert np.array_equal(np.cumsum([0] + [len(l) for l in regions]), loff)
        assert np.array_equal(np.concatenate(regions), lists)
        for xs, ix in zip(X_set, X_set_inds):
            assert np.array_equal(G.bits(xs), G.bits(X[ix]))
        per_point = np.diff(loff)
        nowhere, everywhere, total = int((per_point == 0).sum()), int((per_point == P).sum()), int(soff[-1])
        with np.errstate(invalid="ignore"):
            on_band = int(((E == (oc + eps)[:, None]) | (E == (oc - eps)[:, None])).sum())
        print("%s (%d, %d) eps=%r: %d pairs, %d points in no leaf, %d in every leaf, %d empty sets, %d (point, plane) "
              "pairs with e == c +- eps" % (name, sign_mode, dot_mode, eps, total, nowhere, everywhere,
                                            int((np.diff(soff) == 0).sum()), on_band))
        if eps == 0.0:
            assert 0 < nowhere and total == N - nowhere     # a point with e == c on its way down is in no leaf
        if np.isnan(eps):
            assert total == 0 and nowhere == N
        if eps in (float("inf"), 1e300):
            assert total == N * P and everywhere == N
        if eps == -0.1:
            assert total < N
        if name == "pm0_1d" and eps in (0.5, 1.0):
            assert on_band > 0
            # strict at the root: e == c + eps is not left of it, e == c - eps not right of it
            for n in np.nonzero(E[0] == oc[0] + eps)[0]:
                assert np.all(regions[n] >= P // 2)
            for n in np.nonzero(E[0] == oc[0] - eps)[0]:
                assert np.all(regions[n] < P // 2)
            if eps == 1.0:
                assert np.any(E[0] == oc[0] + eps) and np.any(E[0] == oc[0] - eps)


@pytest.mark.parametrize("name", list(G.REFUSED))
def test_degenerate_refusals_host_vs_oracle(name):
    X, levels, status, text, node, depth = G.REFUSED[name]
    for sign_mode, dot_mode in G.MODES:
        with pytest.raises(pmk.PmkError) as err:
            pmk.setuppartition(X, levels, sign_mode=sign_mode, dot_mode=dot_mode)
        assert "(%d): " % status in str(err.value) and text in str(err.value), str(err.value)
        with pytest.raises(RuntimeError):                   # gethyperplane of an empty node
            O.BSP(X, levels, sign_mode=sign_mode, dot_mode=dot_mode)
        # the oracle one level short of its refusal: the node is its first empty leaf, and no shallower tree has one
        sizes = np.diff(O.BSP(X, depth + 1, sign_mode=sign_mode, dot_mode=dot_mode).leaves()[0])
        assert int(np.argmax(sizes == 0)) == node and sizes[node] == 0 and depth + 1 < levels
        if depth > 1:
            assert np.all(np.diff(O.BSP(X, depth, sign_mode=sign_mode, dot_mode=dot_mode).leaves()[0]) > 0)
    print("%s: refused with %d (%s) at levels = %d; the oracle's first empty node is node %d at depth %d"
          % (name, status, text, levels, node, depth))

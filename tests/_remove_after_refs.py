"""Inputs and references of the tests of what runs AFTER a removal (tests/test_remove_after_refs.py on the CPU,
tests/test_gpu_remove_after.py on the GPU): host data and the oracle only.

  Oracle / MultiOracle   tests/_append_after_refs.Oracle / MultiOracle for a model that LOST points: the tree is that of
                         the points the model was built on (a removal keeps it), the index lists are the oracle's
                         assignment of the whole array under that tree with the entries of a set G deleted, and the fits
                         are those of the reduced lists.  The global numbering is unchanged (a removed index is never
                         given again), so row_of, plan, counts, blend_refit and blend_refit_noisy work as they are: a
                         point of G is a member of no patch, every one of its items is a non-member item, and
                         blend_refit refits nothing for it.
  removed_set            G of tests/_append_cases.Tree by a RULE: the first and the last entry of every patch's list (the
                         ends of the bisection patch_holds of pmk_items.h), the global points 0 and N - 1, two points of
                         every pair of overlapping patches, and a seeded fill from the points only patch 0 holds so that
                         patch 0 loses exactly its 20 removable rows and ends at 129, the edge of its band
  tree_oracle            (Tree, G, Oracle) of a precision, made once
  leaves_case            a tree whose patches are its own leaves (eps=None) and the ends of every leaf's list as G
  mixed_steps            removals and appends mixed on one tree model, with the oracle's lists after every step
"""
import numpy as np

from oracle import oracle as O

import _append_after_refs as AA
import _append_cases as AC
import _remove_cases as RC

hyper, targets2 = AA.hyper, AA.targets2
LD_ROWS = 128                                           # a patch's ld is 128 ceil(n / 128) of the n it was built with


class ReducedBSP(O.BSP):
    """O.BSP whose assignment (and whose leaf lists) leave out the global points `removed`: what a model's index lists are
    after remove_global"""

    def __init__(self, X, levels, removed):
        super().__init__(X, levels)
        self.removed = np.array(sorted(int(g) for g in removed), dtype=np.int64)

    def leaves(self):
        off, inds = super().leaves()
        leaf = np.repeat(np.arange(self.P), np.diff(off))
        keep = ~np.isin(inds, self.removed)
        return np.concatenate([[0], np.cumsum(np.bincount(leaf[keep], minlength=self.P))]).astype(np.int64), inds[keep]

    def assign(self, X, eps):
        off, inds, loff, lists = super().assign(X, eps)
        patch = np.repeat(np.arange(self.P), np.diff(off))
        point = np.repeat(np.arange(len(loff) - 1), np.diff(loff))
        keep, pkeep = ~np.isin(inds, self.removed), ~np.isin(point, self.removed)
        noff = np.concatenate([[0], np.cumsum(np.bincount(patch[keep], minlength=self.P))]).astype(np.int64)
        nloff = np.concatenate([[0], np.cumsum(np.bincount(point[pkeep], minlength=len(loff) - 1))]).astype(np.int64)
        return noff, inds[keep], nloff, lists[pkeep]


class _ReducedTree:
    def _tree(self, X, levels):
        return ReducedBSP(self._X0, levels, self.G)


class Oracle(_ReducedTree, AA.Oracle):
    """AA.Oracle of the points X under the tree of the first len(X0) of them, without the global points `removed`"""

    def __init__(self, X0, X, y, eps, hyper, levels, removed):
        self.G = np.array(sorted(int(g) for g in removed), dtype=np.int64)
        super().__init__(X0, X, y, eps, hyper, levels)


class MultiOracle(_ReducedTree, AA.MultiOracle):
    def __init__(self, X0, X, Y, eps, hyper, trend, levels, removed):
        assert eps is not None
        self.G = np.array(sorted(int(g) for g in removed), dtype=np.int64)
        super().__init__(X0, X, Y, eps, hyper, trend, levels)


def tree_lists(t, X, removed=()):
    """the ascending index lists of the points X under the tree of t.X without `removed`"""
    off, inds, _, _ = ReducedBSP(t.X, t.LEVELS, removed).assign(X, t.EPS)
    return [np.sort(inds[off[r]:off[r + 1]]) for r in range(len(off) - 1)]


def multiplicity(sets, N):
    """number of lists that hold each of the points 0 .. N - 1"""
    return np.bincount(np.concatenate(sets), minlength=N)


def edge_points(sets, N, seed=2010):
    """the part of G the rule names outright: the first and the last entry of every list, the points 0 and N - 1, and two
    points (seeded) of every pair of patches that share points"""
    G = {int(s[0]) for s in sets} | {int(s[-1]) for s in sets} | {0, N - 1}
    rng = np.random.default_rng(seed)
    P = len(sets)
    for a in range(P):
        for b in range(a + 1, P):
            both = np.setdiff1d(np.intersect1d(sets[a], sets[b]), sorted(G))
            if len(both) >= 2:
                G |= {int(j) for j in rng.choice(both, 2, replace=False)}
    return np.array(sorted(G), dtype=np.int64)


def removed_set(sets, N, patch=0, seed=2011):
    """G: edge_points and a seeded fill from the points that `patch` alone holds, so that it loses exactly its removable rows"""
    G = edge_points(sets, N)
    mult = multiplicity(sets, N)
    lost = int(np.isin(sets[patch], G).sum())
    room = RC.removable(len(sets[patch])) - lost
    assert room >= 0
    own = np.setdiff1d(sets[patch][mult[sets[patch]] == 1], G)
    fill = np.random.default_rng(seed).choice(own, room, replace=False)
    return np.array(sorted(set(G.tolist()) | {int(j) for j in fill}), dtype=np.int64)


_TREE = {}


def tree_oracle(dtype):
    """(AC.Tree, G, Oracle of its 400 points without G) of a precision, made once"""
    if dtype not in _TREE:
        t = AC.Tree(dtype)
        G = removed_set(tree_lists(t, t.X), len(t.X))
        _TREE[dtype] = (t, G, Oracle(t.X, t.X, t.y, t.EPS, hyper(dtype), t.LEVELS, G))
    return _TREE[dtype]


LEAF_LEVELS = 3


def leaves_case(dtype="f64"):
    """(X, y, G, Oracle) of 200 points under a tree of 4 leaves with eps=None: the patches are the tree's own leaves, a point
    is a row of its home leaf only.  G: the first and the last entry of every leaf's list and the points 0 and 199"""
    rng = np.random.default_rng(31)
    X = AC.rnd(rng.uniform(-3, 3, (200, 2)), dtype)
    y = AC.target(X)
    off, inds = O.BSP(X, LEAF_LEVELS).leaves()
    G = {0, len(X) - 1}
    for r in range(len(off) - 1):
        s = np.sort(inds[off[r]:off[r + 1]])
        G |= {int(s[0]), int(s[-1])}
    G = np.array(sorted(G), dtype=np.int64)
    return X, y, G, Oracle(X, X, y, None, hyper(dtype), LEAF_LEVELS, G)


def kept_points(o, patch=0):
    """three kept points of `patch` alone (its new first entry, a middle one, its new last entry that it alone holds) and
    three kept points that two patches hold"""
    mult = multiplicity(o.sets, len(o.X))
    s = o.sets[patch]
    own = s[mult[s] == 1]
    two = np.nonzero(mult == 2)[0]
    return [int(s[0]), int(own[len(own) // 2]), int(s[-1])], [int(two[0]), int(two[len(two) // 2]), int(two[-1])]


def multi_points(o, G, patch=0):
    """the points of the multi-output test: 20 kept points of `patch` (its first and last entries among them), 18 other
    kept points (every 14th of the rest) and 6 points of G (its first, its last and four between)"""
    s = o.sets[patch]
    mine = [int(v) for v in s[np.linspace(0, len(s) - 1, 20).round().astype(int)]]
    rest = np.setdiff1d(np.setdiff1d(np.arange(len(o.X)), G), s)
    other = [int(v) for v in rest[5::14][:18]]
    gone = [int(v) for v in G[np.linspace(0, len(G) - 1, 6).round().astype(int)]]
    assert len(set(mine)) == 20 and len(other) == 18 and len(set(gone)) == 6
    return mine, other, gone


# ---- appends and removals mixed on one tree model
class Step:
    """one call: kind "remove" (points: global indices) or "append" (points: X_new, y_new); after it the model holds N
    global indices, the lists `sets` and `removed` is everything that ever left"""

    def __init__(self, kind, points, N, sets, removed, X, y):
        self.kind, self.points, self.N, self.sets, self.removed, self.X, self.y = kind, points, N, sets, removed, X, y


def mixed_steps(dtype):
    """(Tree, steps): remove the edge points, append the tree's 18 new points, remove two old points (the first entry
    of patch 1, and the last old entry of patch 3, which stands just before its appended ones) and three of the just-appended ones (two that one patch holds and one
    that two hold), append four more points"""
    t = AC.Tree(dtype)
    n0 = len(t.X)
    steps = []
    X, y, removed = t.X, t.y, np.zeros(0, dtype=np.int64)

    def push(kind, points):
        steps.append(Step(kind, points, len(X), tree_lists(t, X, removed), removed.copy(), X, y))

    removed = edge_points(tree_lists(t, t.X), n0)
    push("remove", removed.copy())
    X, y = t.Xall, t.yall
    push("append", (t.Xnew, t.ynew))
    old, sets = steps[0].sets, steps[-1].sets
    mult = multiplicity(sets, len(X))[n0:]
    third = np.array([int(old[1][0]), int(old[3][-1]), n0 + int(np.nonzero(mult == 1)[0][0]),
                      n0 + int(np.nonzero(mult == 1)[0][-1]), n0 + int(np.nonzero(mult == 2)[0][0])], dtype=np.int64)
    assert third[0] < n0 and third[1] < n0 and len(set(third.tolist())) == 5
    removed = np.sort(np.concatenate([removed, third]))
    push("remove", np.sort(third))
    Xmore = AC.rnd(np.random.default_rng(2012).uniform(-2.9, 2.9, (4, 2)), dtype)
    X, y = np.ascontiguousarray(np.vstack([X, Xmore])), np.concatenate([y, AC.target(Xmore)])
    push("append", (Xmore, AC.target(Xmore)))
    return t, steps


def ld_of(n):
    return LD_ROWS * ((n + LD_ROWS - 1) // LD_ROWS)

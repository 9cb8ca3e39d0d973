"""Block kriging restated in numpy.longdouble (tests/test_block_refs.py, tests/test_gpu_block.py): mean and kriging variance
of sum_j a[j] f(x_j) over the queries j of a group, in the aggregated form the device computes.

With wn the normalised blend weights of the mix (tests/_cov_refs.py: blend_weights) and w_i = a_{j(i)} wn_i, the items of one
(region r, group f) pair, an aggregate, in the order of the sorted item list (ascending query, a query's items in their
order), give with the patch's long-double factor, C_H and L_G of tests/_cov_multi_refs.py:

    kbar = sum_i w_i k(X, x_i)        Vbar = L^-1 kbar
    kappa = sum_{i, i'} w_i w_i' k(x_i, x_i') + sum_i w_i^2 addend_{j(i)}
    zbar = sum_i w_i z_i,             z_i = L_G^-1 (h(x_i) - C_H^T k(X, x_i))
    s = max(kappa - |Vbar|^2, min_v sum_i w_i^2) + |zbar|^2
    Var_f = sum_r s_{r, f}            Mean_f[c] = sum over the items i of f: w_i u_{i, c}

The error unit of a group is E_f = sum_r sum_{i, i' in (r, f)} |w_i| |w_i'| e_r(i, i') with e_r the unit of a block entry
of tests/_cov_refs.py (and its trend part of tests/_cov_multi_refs.py), the factor (n_r + 32) u included.
"""
import numpy as np

import _cov_refs as CR
import _cov_multi_refs as CMR
from _loo_refs import LD, forward_ld


def item_weights(items, t, wth, a):
    """w [total] in long double in item order, and the query of every item"""
    off = np.asarray(items[0], dtype=np.int64)
    query_of = np.repeat(np.arange(len(off) - 1), np.diff(off))
    return np.asarray(a, dtype=LD)[query_of] * CR.blend_weights(off, t, wth), query_of


def aggregates(items, group):
    """[(region, group, item indices in sorted order)] in the order of the sorted item list: by region, stable in item
    order; group is non-decreasing in the query, so an aggregate is a run"""
    off, reg = np.asarray(items[0], dtype=np.int64), np.asarray(items[1], dtype=np.int64)
    group = np.asarray(group, dtype=np.int64)
    assert np.all(np.diff(group) >= 0)
    query_of = np.repeat(np.arange(len(off) - 1), np.diff(off))
    order = np.argsort(reg, kind="stable")
    out = []
    for p in order:
        key = (int(reg[p]), int(group[query_of[p]]))
        if out and out[-1][:2] == key:
            out[-1][2].append(int(p))
        else:
            out.append((key[0], key[1], [int(p)]))
    return [(r, f, np.array(m, dtype=np.int64)) for r, f, m in out]


def block_ref(items, t, wth, group, a, F, refs, Xq, u, addend=None, min_v=1e-12, item_means=None):
    """dict(Var [F] long double, unit [F] float64, Mean [F, R] (with item_means [total, R] in item order), aggs: one dict
    per aggregate with region, group, count, kappa, vn2, zn2, sw2, unit, margin = (kappa - vn2 - floor) / unit).
    refs[r]: the TrendRegionRef of region r; u: the epsilon of the model's element type.  The solve is linear in its
    right-hand side: Vbar = sum_i w_i V_i and zbar = sum_i w_i z_i from one substitution per region."""
    w, query_of = item_weights(items, t, wth, a)
    Xq = np.asarray(Xq, dtype=np.float64)
    Var, unit = np.zeros(F, dtype=LD), np.zeros(F)
    aggs, region_cov = [], {}
    reg = np.asarray(items[1], dtype=np.int64)
    order = np.argsort(reg, kind="stable")
    for r in sorted(set(int(v) for v in reg)):
        sel = order[reg[order] == r]
        ad = None if addend is None else np.asarray(addend, dtype=np.float64)[query_of[sel]]
        c = refs[r].cov(Xq[query_of[sel]], ad, min_v)
        region_cov[r] = (dict((int(p), k) for k, p in enumerate(sel)), c)
    for r, f, mem in aggregates(items, group):
        ref = refs[r]
        place, c = region_cov[r]
        k = np.array([place[int(p)] for p in mem], dtype=np.int64)
        jq = query_of[mem]
        wm = w[mem]
        Xm = np.asarray(Xq[jq], dtype=LD).reshape(-1, ref.D)
        Vbar = c["V"][:, k] @ wm
        kappa = wm @ CR.kern(ref.th, Xm, Xm) @ wm
        if addend is not None:
            kappa = kappa + (wm * wm) @ np.asarray(np.asarray(addend, dtype=np.float64)[jq], dtype=LD)
        vn2 = Vbar @ Vbar
        zn2 = LD(0)
        if ref.q > 0:
            zbar = c["Z"][:, k] @ wm
            zn2 = zbar @ zbar
        sw2 = wm @ wm
        floor = LD(min_v) * sw2
        s = max(kappa - vn2, floor) + zn2
        aw = np.abs(np.asarray(wm, dtype=np.float64))
        E = float(aw @ ((ref.n + 32) * u * c["unit"][np.ix_(k, k)]) @ aw)
        Var[f] += s
        unit[f] += E
        aggs.append(dict(region=r, group=f, count=len(mem), kappa=kappa, vn2=vn2, zn2=zn2, sw2=sw2, unit=E,
                         margin=float((kappa - vn2 - floor) / LD(E)) if E > 0 else np.inf))
    out = dict(Var=Var, unit=unit, aggs=aggs, w=w, query_of=query_of)
    if item_means is not None:
        U = np.asarray(item_means, dtype=LD)
        Mean = np.zeros((F, U.shape[1]), dtype=LD)
        np.add.at(Mean, np.asarray(group, dtype=np.int64)[query_of], w[:, None] * U)
        out["Mean"] = Mean
    return out


def plain_block_var(items, t, wth, group, a, F, ths, Xs, sigma2, trend, Xq, T_, addend=None, min_v=1e-12):
    """Var [F] by a plain numpy / LAPACK evaluation in the model's precision T_ (the blocks of
    tests/_cov_multi_refs.py: plain_region_cov, off-diagonal entries unclamped) summed against the double weights: what a
    careful evaluation of a^T Cov a in that precision gives"""
    w, query_of = item_weights(items, t, wth, a)
    w = np.asarray(w, dtype=np.float64)
    Var = np.zeros(F)
    for r, f, mem in aggregates(items, group):
        jq = query_of[mem]
        S = CMR.plain_region_cov(ths[r], Xs[r], sigma2, np.asarray(Xq)[jq], T_, trend,
                                 None if addend is None else np.asarray(addend)[jq], min_v)
        Var[f] += w[mem] @ S @ w[mem]
    return Var

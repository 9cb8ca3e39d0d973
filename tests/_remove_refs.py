"""A numpy.longdouble restatement of the row deletion from the Cholesky factor (pmk_model_remove), independent of the
device code and of the oracle: tests/test_remove_refs.py pins it to cholesky_ld of the reduced Gram matrix and to
oracle.fit_patch on the reduced point set; tests/test_gpu_remove.py takes its error unit from here.

For a patch with U = K + sigma2 I (+ addends) = L L^T, z = L^-1 y and the removed rows r_1 < ... < r_m, k0 = r_1:
L~ = L[keep, :] has L~ L~^T = U[keep, keep] and L~ z = y[keep].  New row j of the trailing block B = L[keep >= k0, k0:] is
the old row p_j and ends at column j + s_j, s_j = #{removed rows < p_j}.  One Householder reflector per new column j, on
the columns j .. j + s_j, made from row j (v = x + sign(x_0) |x| e_0), then the sign of column j flipped so that the
diagonal is +|x|; applied to the rows below and to z^T[k0:]:

    B Q = [L'_22 0]     z' = [ z[:k0] ; (Q^T z[k0:])[:t] ]     c' = L'^-T z'

The sweep here works on WHOLE rows (every column from j on) and reports what it finds right of j + s_j when row j's turn
comes: the band claim is that this is exactly zero.

The error unit of an entry of L' or of c', for a model of unit round-off u, with n and L those of the patch BEFORE the call:

    e = (n + 32) u kappa2(L) max |L|

the unit of tests/_append_refs.py: the resident factor carries the error of a fit of n rows, and the deletion, being
orthogonal, adds a term of the same form.
"""
import numpy as np

import _append_refs as AR
from _loo_refs import LD, backward_ld, cholesky_ld, forward_ld

U_OF, gram, kappa_of, unit, ratio = AR.U_OF, AR.gram, AR.kappa_of, AR.unit, AR.ratio


def shifts(n, rows):
    """(keep, s): the ascending complement of rows in range(n) and, per kept row, the removed rows before it"""
    rows = np.asarray(rows, dtype=np.int64)
    keep = np.setdiff1d(np.arange(n), rows)
    return keep, np.searchsorted(rows, keep)


def delete_rows_ld(L, z, rows):
    """dict(L [n', n'], z [n'], c [n'], fill) in long double by the reflector sweep on the factor L and z = L^-1 y; fill
    is the largest magnitude found right of a row's span j + s_j when its reflector is made"""
    L, z = np.asarray(L, dtype=LD), np.asarray(z, dtype=LD)
    n, rows = len(L), sorted(int(r) for r in rows)
    if not rows:
        return dict(L=L.copy(), z=z.copy(), c=backward_ld(L, z), fill=0.0)
    keep, s_all = shifts(n, rows)
    k0, m = rows[0], len(rows)
    n1, t = n - m, n - m - k0
    tail = keep[k0:]
    s = s_all[k0:]
    B = L[tail, k0:].copy()                     # t x (t + m)
    zt = z[k0:].copy()
    fill = 0.0
    for j in range(t):
        e = j + int(s[j])
        if e + 1 < t + m:
            fill = max(fill, float(np.abs(B[j, e + 1:]).max()))
        x = B[j, j:]                            # the whole rest of the row: zeros right of e if the band claim holds
        nrm = np.sqrt(x @ x)
        sg = LD(-1) if x[0] < 0 else LD(1)
        v = x.copy()
        v[0] += sg * nrm
        beta = LD(1) / (nrm * (nrm + abs(x[0])))
        w = B[j + 1:, j:] @ v
        B[j + 1:, j:] -= beta * np.outer(w, v)
        B[j + 1:, j] *= -sg
        wz = zt[j:] @ v
        zt[j:] -= beta * wz * v
        zt[j] *= -sg
        B[j, j:] = 0
        B[j, j] = nrm
    L1 = np.zeros((n1, n1), dtype=LD)
    L1[:k0, :k0] = L[:k0, :k0]
    L1[k0:, :k0] = L[tail, :k0]
    L1[k0:, k0:] = B[:, :t]
    z1 = np.concatenate([z[:k0], zt[:t]])
    return dict(L=L1, z=z1, c=backward_ld(L1, z1), fill=fill)


def remove_ref(th, X, y, sigma2, rows, diag=None):
    """the deletion applied to the long-double factor of the full patch, and the factor of the reduced Gram matrix beside
    it: dict(L, z, c, fill, L_full, z_full, c_full, L_chol, c_chol)"""
    U = gram(th, X, sigma2, diag)
    L = cholesky_ld(U)
    z = forward_ld(L, np.asarray(y, dtype=LD))
    out = delete_rows_ld(L, z, rows)
    keep, _ = shifts(len(L), rows)
    Lc = cholesky_ld(U[np.ix_(keep, keep)])
    out.update(L_full=L, z_full=z, c_full=backward_ld(L, z), L_chol=Lc,
               c_chol=backward_ld(Lc, forward_ld(Lc, np.asarray(y, dtype=LD)[keep])))
    return out

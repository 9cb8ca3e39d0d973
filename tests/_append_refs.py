"""A numpy.longdouble restatement of the border of the Cholesky factor (pmk_model_append), independent of the device
code and of the oracle: tests/test_append_refs.py pins it to oracle.fit_patch on the extended point set and to
oracle.cholesky_lower of the extended K + sigma2 I; tests/test_gpu_append.py takes its error unit from here.

For a patch X with U = K + sigma2 I (+ addends) = L L^T, z = L^-1 y, and m new points Xn with targets yn:

    L' = [ L    0   ]    L21^T = V = L^-1 k(X, Xn)
         [ L21  L22 ]    L22 L22^T = k(Xn, Xn) + sigma2 I (+ addends) - V^T V
    z' = [ z ; L22^-1 (yn - L21 z) ]        c' = L'^-T z'

The kernels are those of tests/_cov_refs.py (kern), the Cholesky and the substitutions those of tests/_loo_refs.py.

The error unit of an entry of L' or of c', for a model of unit round-off u:

    e = (n + m + 32) u kappa2(L') max |L'|

the unit of the fit's own tests scaled to the largest entry of the factor: a backward-stable factorisation of n + m rows
moves an entry of L' by about (n + m) u kappa2(L') |L'|, and the 32 covers the roundings of the kernel values themselves.
The inputs of tests/_append_cases.py keep kappa2(L') <= 10^3 and the weights of the size of the factor's entries, so that
one unit also bounds what a plain double-precision evaluation of c' loses (tests/test_append_refs.py asserts both).
"""
import numpy as np

import _cov_refs as CR
from _loo_refs import LD, backward_ld, cholesky_ld, forward_ld

U_OF = {"f64": 2.0 ** -53, "f32": 2.0 ** -24}


def gram(th, X, sigma2, diag=None):
    """U = K + sigma2 I + diag(addends) in long double"""
    X = np.asarray(X, dtype=LD)
    U = CR.kern(th, X, X) + LD(sigma2) * np.eye(len(X), dtype=LD)
    if diag is not None:
        U[np.diag_indices(len(X))] += np.asarray(diag, dtype=LD)
    return U


def border_ref(th, X, y, sigma2, Xn, yn, diag=None, diagn=None):
    """dict(L [n + m, n + m], z [n + m], c [n + m]) in long double by the border of the factor of the first n points"""
    X, Xn = np.asarray(X, dtype=LD), np.asarray(Xn, dtype=LD).reshape(-1, np.asarray(X).shape[1])
    n, m = len(X), len(Xn)
    L = cholesky_ld(gram(th, X, sigma2, diag))
    z = forward_ld(L, np.asarray(y, dtype=LD))
    V = forward_ld(L, CR.kern(th, X, Xn))
    S = gram(th, Xn, sigma2, diagn) - V.T @ V
    L22 = cholesky_ld((S + S.T) / LD(2))
    z2 = forward_ld(L22, np.asarray(yn, dtype=LD) - V.T @ z)
    Lp = np.zeros((n + m, n + m), dtype=LD)
    Lp[:n, :n], Lp[n:, :n], Lp[n:, n:] = L, V.T, L22
    zp = np.concatenate([z, z2])
    return dict(L=Lp, z=zp, c=backward_ld(Lp, zp))


def kappa_of(U):
    """kappa2(L) = sqrt(cond2(U))"""
    s = np.linalg.svd(np.asarray(U, dtype=np.float64), compute_uv=False)
    return float(np.sqrt(s[0] / s[-1]))


def unit(n_total, dtype, kappa, L):
    """e = (n + m + 32) u kappa2(L') max |L'|"""
    return (n_total + 32) * U_OF[dtype] * kappa * float(np.abs(np.asarray(L, dtype=np.float64)).max())


def ratio(got, want, e):
    """max |got - want| / e; NaN anywhere is infinitely wrong"""
    d = np.abs(np.asarray(got, dtype=LD) - np.asarray(want, dtype=LD)).astype(np.float64)
    return float("inf") if np.isnan(d).any() else float(d.max() / e) if d.size else 0.0

"""The joint posterior covariance under a trend, restated in numpy.longdouble (tests/test_cov_multi_refs.py,
tests/test_gpu_cov_multi.py): tests/_cov_refs.py extended by the trend's term.

Per region r (patch X, U = K + sigma2 I = L L^T, basis H (n x q) of tests/_trend_refs.py, C_H = U^-1 H,
G = H^T C_H = L_G L_G^T) and its items x_1 .. x_m:

    V_a = L^-1 k(X, x_a),   rho_a = h(x_a) - C_H^T k(X, x_a),   z_a = L_G^-1 rho_a
    S[a, b] = k(x_a, x_b) - V_a . V_b + z_a . z_b                               for a != b, not clamped
    S[a, a] = max( k(x_a, x_a) + addend_a - |V_a|^2, min_v ) + |z_a|^2          the trend's term after the clamp

which is k_ab - [k_a; h_a]^T [[U, H], [H^T, 0]]^-1 [k_b; h_b] (kkt_cov, an independent route: one dense solve of the
saddle-point system by Gaussian elimination with partial pivoting, in long double).  The blend is mix_cov_ref of
_cov_refs.py, unchanged.  Without a trend (trend None) everything is RegionRef of _cov_refs.py.

The error unit of a block entry, before the factor (n + 32) u (u of the model's element type), is the e(a, b) of
_cov_refs.py plus the trend's part

    |dz_a| |z_b| + |z_a| |dz_b|,   |dz| = kappa2(U) |L_G^-1|_2 ( |h| + | |C_H|^T |kq| | )

rho = h - C_H^T kq is computed from a C_H that the two substitutions perturb by n u kappa2(U) |C_H| entrywise in the
worst case, and L_G^-1 carries that to z; h itself is exact, its norm covers the roundings of the small solve.
"""
import numpy as np

import _cov_refs as CR
import _trend_refs as TR
from _loo_refs import LD, backward_ld, cholesky_ld, forward_ld


def basis_ld(X, trend):
    return np.asarray(TR.basis(np.asarray(X, dtype=np.float64), trend), dtype=LD)


class TrendRegionRef(CR.RegionRef):
    """one patch with its trend: the long-double factor, C_H and L_G, built once and shared by every batch of items"""

    def __init__(self, th, X, sigma2, trend):
        super().__init__(th, X, sigma2)
        self.trend = trend
        if trend is None:
            self.q = 0
            return
        self.H = basis_ld(self.X, trend)
        self.q = self.H.shape[1]
        self.CH = backward_ld(self.L, forward_ld(self.L, self.H))
        G = self.H.T @ self.CH
        self.G = (G + G.T) / LD(2)
        self.LG = cholesky_ld(self.G)
        s = np.linalg.svd(np.asarray(self.LG, dtype=np.float64), compute_uv=False)
        self.kappa_G = float(s[0] / s[-1])                   # kappa2(L_G)
        self.norm_LGinv = float(1.0 / s[-1])                 # |L_G^-1|_2

    def cov(self, Xq, addend=None, min_v=1e-12):
        """dict(S, unit, V, clamped) of _cov_refs.RegionRef.cov, S and unit with the trend's part, and Z [q, m]"""
        out = super().cov(Xq, addend, min_v)
        if self.q == 0:
            return out
        Xq = np.asarray(Xq, dtype=LD).reshape(-1, self.D)
        Kq = CR.kern(self.th, self.X, Xq)                    # n x m
        Hq = basis_ld(Xq, self.trend)                        # m x q
        rho = Hq - Kq.T @ self.CH
        Z = forward_ld(self.LG, rho.T)                       # q x m
        T = Z.T @ Z
        out["S"] = out["S"] + (T + T.T) / LD(2)              # the diagonal: after the clamp
        nz = np.sqrt(np.asarray((Z * Z).sum(0), dtype=np.float64))
        hn = np.sqrt(np.asarray((Hq * Hq).sum(1), dtype=np.float64))
        ak = np.abs(Kq).T @ np.abs(self.CH)                  # m x q: |C_H|^T |kq|
        an = np.sqrt(np.asarray((ak * ak).sum(1), dtype=np.float64))
        dz = self.kappa ** 2 * self.norm_LGinv * (hn + an)   # kappa2(U) = kappa2(L)^2
        out["unit"] = out["unit"] + np.outer(dz, nz) + np.outer(nz, dz)
        out["Z"] = Z
        return out


def solve_ld(A, B):
    """A^-1 B in long double by Gaussian elimination with partial pivoting (A square, any symmetric or not)"""
    A = np.array(A, dtype=LD)
    B = np.array(B, dtype=LD)
    n = A.shape[0]
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if p != k:
            A[[k, p]] = A[[p, k]]
            B[[k, p]] = B[[p, k]]
        f = A[k + 1:, k] / A[k, k]
        A[k + 1:, k:] -= f[:, None] * A[k, k:][None, :]
        B[k + 1:] -= f[:, None] * B[k][None, :]
    X = np.zeros_like(B)
    for k in range(n - 1, -1, -1):
        X[k] = (B[k] - A[k, k + 1:] @ X[k + 1:]) / A[k, k]
    return X


def kkt_cov(K, sigma2, H, Kq, Kqq, Hq):
    """k_ab - [k_a; h_a]^T [[U, H], [H^T, 0]]^-1 [k_b; h_b] in long double from kernel matrices: K [n, n], Kq [n, m],
    Kqq [m, m], H [n, q], Hq [m, q].  No clamp, no addend."""
    K, H, Kq, Kqq, Hq = (np.asarray(a, dtype=LD) for a in (K, H, Kq, Kqq, Hq))
    n, q = H.shape
    A = np.zeros((n + q, n + q), dtype=LD)
    A[:n, :n] = K
    A[np.arange(n), np.arange(n)] += LD(sigma2)
    A[:n, n:] = H
    A[n:, :n] = H.T
    rhs = np.vstack([Kq, Hq.T])
    S = Kqq - rhs.T @ solve_ld(A, rhs)
    return (S + S.T) / LD(2)


def plain_region_cov(th, X, sigma2, Xq, T_, trend, addend=None, min_v=1e-12):
    """the block in the model's own precision T_ with numpy and LAPACK (plain_region_cov of _cov_refs.py) plus the
    trend's term as a careful evaluation in that precision takes it: C_H and a = kq^T C_H in T_, the sums over the rows
    that make G, the small factor and the small solves in double, as on the device"""
    import scipy.linalg as sla
    S = CR.plain_region_cov(th, X, sigma2, Xq, T_, addend, min_v)
    if trend is None:
        return S
    Xt, Xqt = np.asarray(X).astype(T_), np.asarray(Xq).astype(T_)
    n = len(Xt)
    U = (CR.kern(th, Xt, Xt) + T_(sigma2) * np.eye(n, dtype=T_)).astype(T_)
    H = TR.basis(Xt.astype(np.float64), trend)
    CH = sla.cho_solve(sla.cho_factor(U, lower=True), H.astype(T_))
    assert CH.dtype == T_
    a = (CR.kern(th, Xt, Xqt).astype(T_).T @ CH).astype(np.float64)      # m x q
    G = H.T @ CH.astype(np.float64)
    LG = sla.cholesky((G + G.T) / 2, lower=True)
    rho = TR.basis(Xqt.astype(np.float64), trend) - a
    Z = sla.solve_triangular(LG, rho.T, lower=True)
    return S + Z.T @ Z

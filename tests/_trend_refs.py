"""Long-double references for kriging with a trend (tests/test_trend_abi.py, tests/test_gpu_trend.py): the per-patch
generalised-least-squares drift, the universal-kriging prediction and the trend-aware leave-one-out values.

numpy.longdouble with the plain column Cholesky and row substitutions of tests/_loo_refs.py; the kernel matrices come
from the CPU oracle and are widened, so the references are exact to ~19 digits for the matrix the device sees.

    U = K + sigma2 I = L L^T,  H = basis(X) (n x q),  [C_Y | C_H] = U^-1 [Y | H],  d = diag(U^-1)
    G = H^T C_H,  beta = G^-1 H^T C_Y,  C = C_Y - C_H beta
    query:  mu = kq C + h(x*) beta,  v = max(k(x*, x*) - |L^-1 kq^T|^2, min_v) + rho^T G^-1 rho,  rho = h(x*) - kq C_H
    leave-one-out:  Q_ii = d_i - C_H[i, :] G^-1 C_H[i, :]^T,  res = C / Q,  var = 1 / Q
    evidence:  quad = (y - H beta)^T U^-1 (y - H beta)

brute_force_loo refits the universal-kriging predictor n times without point i: what the closed form must equal.
"""
import numpy as np

from _loo_refs import LD, cholesky_ld, forward_ld, backward_ld, loo_reference

TRENDS = {"constant": 0, "linear": 1}


def basis(X, trend):
    """H: [1] or [1, x_1 .. x_D] in the raw coordinates"""
    X = np.asarray(X, dtype=np.float64)
    if X.ndim == 1:
        X = X[:, None]
    one = np.ones((X.shape[0], 1))
    return one if trend == "constant" else np.hstack([one, X])


def _spd_solve_ld(G, B):
    L = cholesky_ld(G)
    return backward_ld(L, forward_ld(L, B)), L


def trend_reference(K, sigma2, Y, H):
    """dict(C_Y, C_H, G, LG, beta, C, d, Q, res, var, quad, L) in long double"""
    Y = np.asarray(Y, dtype=LD)
    if Y.ndim == 1:
        Y = Y[:, None]
    H = np.asarray(H, dtype=LD)
    R = Y.shape[1]
    base = loo_reference(K, sigma2, np.hstack([Y, H]))
    C_Y, C_H = base["C"][:, :R], base["C"][:, R:]
    G = H.T @ C_H
    G = (G + G.T) / LD(2)
    beta, LG = _spd_solve_ld(G, H.T @ C_Y)
    Cw = C_Y - C_H @ beta
    W = forward_ld(LG, C_H.T)                        # q x n: L_G^-1 C_H^T
    Q = base["d"] - (W * W).sum(0)
    resid = Y - H @ beta
    L = base["L"]
    Z = forward_ld(L, resid)
    return dict(C_Y=C_Y, C_H=C_H, G=G, LG=LG, beta=beta, C=Cw, d=base["d"], Q=Q, res=Cw / Q[:, None], var=LD(1) / Q,
                quad=(Z * Z).sum(0), L=L)


def predict_reference(ref, Kq, kqq, Hq, min_v=1e-12):
    """(mu [m, R], v [m]) for m query points: Kq = k(xq, X) (m x n), kqq = k(xq, xq) (m), Hq = basis(xq)"""
    Kq, Hq = np.asarray(Kq, dtype=LD), np.asarray(Hq, dtype=LD)
    mu = Kq @ ref["C"] + Hq @ ref["beta"]
    Z = forward_ld(ref["L"], Kq.T)
    v_sk = np.maximum(np.asarray(kqq, dtype=LD) - (Z * Z).sum(0), LD(min_v))
    rho = Hq - Kq @ ref["C_H"]
    W = forward_ld(ref["LG"], rho.T)
    return mu, v_sk + (W * W).sum(0)


def brute_force_loo(K, sigma2, Y, H):
    """(res [n, R], var [n]) from n refits without point i, in long double: res_i = y_i - mu_-i(x_i), var_i = the
    universal-kriging variance of y_i (noise included) from the other n - 1 points"""
    K = np.asarray(K, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    if Y.ndim == 1:
        Y = Y[:, None]
    n = K.shape[0]
    res, var = np.zeros(Y.shape, dtype=LD), np.zeros(n, dtype=LD)
    for i in range(n):
        keep = np.arange(n) != i
        ref = trend_reference(K[np.ix_(keep, keep)], sigma2, Y[keep], H[keep])
        mu, v = predict_reference(ref, K[i:i + 1, keep], [K[i, i] + sigma2], H[i:i + 1], min_v=-np.inf)
        res[i] = np.asarray(Y[i], dtype=LD) - mu[0]
        var[i] = v[0]
    return res, var


# ---- the same quantities in plain fp64 (scipy / LAPACK): what a careful fp64 implementation achieves on the same inputs,
# the yardstick of the GPU tests' bounds
def gls_fp64(K, sigma2, Y, H):
    import scipy.linalg as sla
    Y = np.asarray(Y, dtype=np.float64)
    if Y.ndim == 1:
        Y = Y[:, None]
    H = np.asarray(H, dtype=np.float64)
    n, R = Y.shape
    U = np.asarray(K, dtype=np.float64) + sigma2 * np.eye(n)
    cf = sla.cho_factor(U, lower=True)
    S = sla.cho_solve(cf, np.hstack([Y, H]))
    C_Y, C_H = S[:, :R], S[:, R:]
    G = H.T @ C_H
    gf = sla.cho_factor((G + G.T) / 2, lower=True)
    beta = sla.cho_solve(gf, H.T @ C_Y)
    Cw = C_Y - C_H @ beta
    Linv = sla.solve_triangular(cf[0], np.eye(n), lower=True)
    d = (Linv * Linv).sum(0)
    W = sla.solve_triangular(gf[0], C_H.T, lower=True)
    Q = d - (W * W).sum(0)
    resid = Y - H @ beta
    Z = sla.solve_triangular(cf[0], resid, lower=True)
    return dict(U=U, C_Y=C_Y, C_H=C_H, G=G, LG=np.tril(gf[0]), beta=beta, C=Cw, Q=Q, res=Cw / Q[:, None], var=1.0 / Q,
                quad=(Z * Z).sum(0), L=np.tril(cf[0]))


def predict_fp64(ref, Kq, kqq, Hq, min_v=1e-12):
    import scipy.linalg as sla
    mu = Kq @ ref["C"] + Hq @ ref["beta"]
    Z = sla.solve_triangular(ref["L"], Kq.T, lower=True)
    v_sk = np.maximum(np.asarray(kqq) - (Z * Z).sum(0), min_v)
    rho = Hq - Kq @ ref["C_H"]
    W = sla.solve_triangular(ref["LG"], rho.T, lower=True)
    return mu, v_sk + (W * W).sum(0)


def kkt_ratios(U, H, Y, Cw, beta, u, C_Y, C_H):
    """relative residuals of U C + H beta = Y and H^T C = 0, each normalised by the norms of its terms, in units of n u.
    The terms of the second are those of C = C_Y - C_H beta (C itself may be exactly zero: one point and a constant
    trend); C_Y and C_H are only normalisers and come from the fp64 solve."""
    U, H, Y, Cw, beta = (np.asarray(a, dtype=LD) for a in (U, H, Y, Cw, beta))
    n = U.shape[0]

    def f(a):
        return float(np.linalg.norm(np.asarray(a, dtype=np.float64)))
    r1 = f(U @ Cw + H @ beta - Y) / (f(U) * f(Cw) + f(H) * f(beta) + f(Y))
    r2 = f(H.T @ Cw) / (f(H) * (f(C_Y) + f(C_H) * f(beta)))
    return r1 / (n * u), r2 / (n * u)

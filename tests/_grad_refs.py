"""An independent numpy restatement of the gradient of the blended mean (tests/test_grad_refs.py, tests/test_gpu_grad.py).

For a stationary kernel k(x, z) = phi(|x - z|):  grad_x k = psi(tau) (x - z) with psi = phi'(tau) / tau, written here from
the closed forms (r = a tau, t = max(1 - r, 0)) and not from the device header:

    Spline34  -(56/3) a^2 (5 r + 1) t^5      Spline12  -12 a^2 t^2       Spline32  -20 a^2 t^3
    Gaussian  -2 p0 exp(-p0 tau^2)           RQ  -3 p0^(3/2) / (p0 + tau^2)^(5/2)       TRQ  p1 times RQ
    ModSqExp  exp(-p0 tau^2) (-2 p0 cos(p1 tau) - p1^2 sinc(p1 tau)),  sinc(0) = 1

A kernel is the oracle's descriptor (oracle.kernel(family, p0, p1)): only .family and .p are read.

    item:   G[d, c] = sum_k psi(tau_k) (x_d - z_{k,d}) C[k, c]  (+ beta[1 + d, c] with a linear trend)
    blend:  w_i = phi_w(|t_i|) (home: 1), S = sum w_i, Y_c = sum w_i u_{i,c} / S,
            dY_c/dx_d = (1 / S) sum_i [ w_i G_{i,d,c} + (u_{i,c} - Y_c) dw_i/dx_d ],  dw_i/dx_d = -psi_w(|t_i|) t_i v_{plane(i),d}
"""
import numpy as np

LD = np.longdouble
SPLINE34, SPLINE12, SPLINE32, GAUSSIAN, RQ, TRQ, MODSQEXP = 1, 2, 3, 4, 5, 6, 7
COMPACT = (SPLINE34, SPLINE12, SPLINE32)


def phi(th, tau):
    """the profile itself, in the working type of tau (float64 or longdouble arrays)"""
    tau = np.asarray(tau)
    T = tau.dtype.type
    p0, p1 = T(th.p[0]), T(th.p[1])
    r = tau * p0
    t = np.maximum(T(1) - r, T(0))
    f = th.family
    if f == SPLINE34:
        return (T(35) * r * r + T(18) * r + T(3)) * t ** 6 / T(3)
    if f == SPLINE12:
        return (T(3) * r + T(1)) * t ** 3
    if f == SPLINE32:
        return (T(4) * r + T(1)) * t ** 4
    if f == GAUSSIAN:
        return np.exp(-p0 * tau * tau)
    if f in (RQ, TRQ):
        v = p0 ** T(1.5) / (p0 + tau * tau) ** T(1.5)
        return p1 * v if f == TRQ else v
    if f == MODSQEXP:
        return np.exp(-p0 * tau * tau) * np.cos(p1 * tau)
    raise ValueError("no stationary profile for family %d" % f)


def psi(th, tau):
    """phi'(tau) / tau, finite at tau = 0, exactly 0 outside a compact support"""
    tau = np.asarray(tau)
    T = tau.dtype.type
    p0, p1 = T(th.p[0]), T(th.p[1])
    r = tau * p0
    t = np.maximum(T(1) - r, T(0))
    f = th.family
    if f == SPLINE34:
        return -(T(56) / T(3)) * p0 * p0 * (T(5) * r + T(1)) * t ** 5
    if f == SPLINE12:
        return -T(12) * p0 * p0 * t ** 2
    if f == SPLINE32:
        return -T(20) * p0 * p0 * t ** 3
    if f == GAUSSIAN:
        return -T(2) * p0 * np.exp(-p0 * tau * tau)
    if f in (RQ, TRQ):
        v = -T(3) * p0 ** T(1.5) / (p0 + tau * tau) ** T(2.5)
        return p1 * v if f == TRQ else v
    if f == MODSQEXP:
        x = p1 * tau
        safe = np.where(x == 0, T(1), x)
        sinc = np.where(x == 0, T(1), np.sin(safe) / safe)
        return np.exp(-p0 * tau * tau) * (-T(2) * p0 * np.cos(x) - p1 * p1 * sinc)
    raise ValueError("no stationary profile for family %d" % f)


def support(th):
    """the radius beyond which phi' is negligible: the support of a spline, else where |phi'| has fallen far below its
    maximum"""
    if th.family in COMPACT:
        return 1.0 / th.p[0]
    if th.family in (GAUSSIAN, MODSQEXP):
        return 8.0 / np.sqrt(th.p[0])
    return 60.0 * np.sqrt(th.p[0])


def lip(th, grid=200001):
    """max |phi'(tau)| = max |psi(tau) tau| on a dense grid of the support"""
    tau = np.linspace(0.0, support(th), grid)
    return float(np.abs(psi(th, tau) * tau).max())


def item_grad_ref(th, Xpatch, Cw, xq, beta=None):
    """G [D, R] in long double for one query point xq [D] against the patch's points [n, D] and weights [n, R]; beta
    [1 + D, R]: the coefficients of a linear trend"""
    X = np.asarray(Xpatch, dtype=LD)
    Cw = np.asarray(Cw, dtype=LD)
    if Cw.ndim == 1:
        Cw = Cw[:, None]
    diff = np.asarray(xq, dtype=LD)[None, :] - X                      # n x D
    tau = np.sqrt((diff * diff).sum(1))
    A = psi(th, tau)[:, None] * diff                                  # n x D
    G = A.T @ Cw
    if beta is not None:
        G = G + np.asarray(beta, dtype=LD)[1:]
    return G


def mix_grad_ref(items, G, U, t, plane, hp_v, wth):
    """dY [R, D] of one query in long double and the magnitude sum_i (|w_i G_i| + |(u_i - Y) dw_i|) / S [R, D] that the
    rounding bound of the blend is stated in.  items: the indices of the query's items (neighbours in hyperplane order,
    home last); G [total, R, D], U [total, R], t [total], plane [total]; hp_v [P - 1, D] the pre-order normals."""
    items = list(items)
    tt = np.asarray(t, dtype=LD)[items]
    w = phi(wth, np.abs(tt))
    w[-1] = LD(1)
    S = w.sum()
    Ui = np.asarray(U, dtype=LD)[items]                               # m x R
    Gi = np.asarray(G, dtype=LD)[items]                               # m x R x D
    Y = (w[:, None] * Ui).sum(0) / S
    v = np.zeros((len(items), np.asarray(hp_v).shape[1]), dtype=LD)
    for k, it in enumerate(items[:-1]):
        v[k] = np.asarray(hp_v, dtype=LD)[plane[it]]
    dw = -(psi(wth, np.abs(tt)) * tt)[:, None] * v                    # m x D
    dw[-1] = LD(0)
    a = w[:, None, None] * Gi
    b = (Ui - Y[None, :])[:, :, None] * dw[:, None, :]
    return (a + b).sum(0) / S, (np.abs(a) + np.abs(b)).sum(0) / S

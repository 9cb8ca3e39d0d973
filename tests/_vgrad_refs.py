"""An independent numpy.longdouble restatement of the gradient of the blended variance (tests/test_vgrad_refs.py,
tests/test_gpu_vgrad.py).  phi and psi are those of tests/_grad_refs.py, the Cholesky and the substitutions those of
tests/_loo_refs.py.

Per item (query x, patch X, U = K + sigma2 I = L L^T), kq_k = phi(tau_k), g_{d,k} = psi(tau_k) (x_d - z_{k,d}):

    V = L^-1 kq,  W_d = L^-1 g_d,  b = |V|^2,  v_sk = max(k(x,x) - b, min_v)
    d v_sk / dx_d = -2 V . W_d  where k(x,x) - b >= min_v, exactly 0 where the clamp holds

with a trend of q basis functions h (1, or 1 and the coordinates), C_H = U^-1 H and L_G L_G^T = H^T C_H (the reference's
own, from its own factor, unless they are passed in):

    v = v_sk + |z|^2,  z = L_G^-1 rho,  rho = h(x) - kq C_H
    d v / dx_d += 2 z . y_d,  y_d = L_G^-1 d_d rho,  (d_d rho)_a = [a = 1 + d, linear only] - (g_d C_H)_a

Blend, items in the order of the mix (neighbours in hyperplane order, home last): w_i = phi_w(|t_i|) (home: 1), S = sum w_i,
wn_i = w_i / S, Vq = sum wn_i^2 v_i:

    dVq/dx_d = sum_i [ wn_i^2 d_d v_i + 2 wn_i v_i d_d wn_i ],  d_d wn_i = (d_d w_i - wn_i sum_j d_d w_j) / S,
    d_d w_i = -psi_w(|t_i|) t_i v_{plane(i),d} for a neighbour, 0 for the home item.

The error unit of an item's gradient (what a backward-stable sweep over the n rows can be held to):

    e_d = (n + 32) u [ kappa2(L) |V|_2 |W_d|_2 + t_d ],
    t_d = kappa2(L_G) [ kappa2(L) |z|_2 |y_d|_2 + |L_G^-1|_2 (M_z |y_d|_2 + |z|_2 M_{y,d}) ],
    M_z = | |h| + |kq| |C_H| |_2,  M_{y,d} = | |d_d h| + |g_d| |C_H| |_2.

First term: the substitution perturbs V and W_d by n u kappa2(L) relative to their norms, and their product by the sum.
t_d is its analogue for 2 z . y_d, to first order.  z and y_d come out of the substitution with L_G (kappa2(L_G)) from
right-hand sides built on C_H = U^-1 H as the model solved it (kappa2(L) |z| |y_d|: the analogue proper).  But rho and
d_d rho are sums of n + q products that cancel -- inside the data h is nearly kq C_H -- so their rounding is (n + 32) u
of the sum of their terms' magnitudes (the entries of M_z, M_y), not of their own norms; L_G^-1 carries it into z and y_d,
and the product moves by |dz| |y_d| + |z| |dy_d|.  A unit in |z| |y_d| alone is too tight: a plain evaluation in the
model's precision reaches 3.5 of it on the inputs in use.  A product of the worst cases of both factors
(|L_G^-1|^2 M_z M_y, or kappa2(L)^2) is too loose: in fp32 it exceeds the trend's whole contribution many times over.
The trend's part is also held to (n + 32) u t_d alone (`trend`, `tunit`): in fp32 the first term of e_d is larger than the
whole trend part, and a check of the sum would not see it.  t_d bounds every sum by its worst case already, so that check
allows one unit, not ten.  Its tolerance is then, per patch in the median, 1e-14 to 5e-9 of the trend's part in fp64; in
fp32 1e-4 to 7e-3 of it for the constant trend and for the linear trend on patches of up to 129 points, and 0.02 to 0.4 of
it for the linear trend on larger patches, where z and y_d are themselves the remainders of sums 1e3 times their size.
tests/test_vgrad_refs.py holds a plain numpy / LAPACK evaluation in the model's own precision below one unit, for the
sum and for the trend's part.
The same unit for the variance itself: v_unit = kappa2(L) (k(x,x) + b) + kappa2(L_G) (kappa2(L) |z|^2 + 2 |L_G^-1| M_z |z|).
"""
import numpy as np

import _grad_refs as GR
from _loo_refs import LD, backward_ld, cholesky_ld, forward_ld


def _kernel_matrix_ld(th, X):
    X = np.asarray(X, dtype=LD)
    diff = X[:, None, :] - X[None, :, :]
    return GR.phi(th, np.sqrt((diff * diff).sum(2)))


class PatchRef:
    """one patch: its long-double factor, built once and shared by every query point"""

    def __init__(self, th, X, sigma2, trend=None, C_H=None, LG=None):
        """trend: None, "constant" or "linear"; C_H, LG: the trend's operands if not the reference's own"""
        self.th = th
        self.X = np.asarray(X, dtype=LD)
        if self.X.ndim == 1:
            self.X = self.X[:, None]
        self.n, self.D = self.X.shape
        self.U = _kernel_matrix_ld(th, self.X) + LD(sigma2) * np.eye(self.n, dtype=LD)
        self.L = cholesky_ld(self.U)
        self.kself = GR.phi(th, np.zeros(1, dtype=LD))[0]
        if trend and C_H is None:
            H = np.hstack([np.ones((self.n, 1), dtype=LD)] + ([self.X] if trend == "linear" else []))
            C_H = backward_ld(self.L, forward_ld(self.L, H))
            G = H.T @ C_H
            LG = cholesky_ld((G + G.T) / LD(2))
        self.C_H = None if C_H is None else np.asarray(C_H, dtype=LD).reshape(self.n, -1)
        self.LG = None if LG is None else np.asarray(LG, dtype=LD)
        self.q = 0 if self.C_H is None else self.C_H.shape[1]
        self._kappa = None

    def kappa(self):
        """(kappa2(L), kappa2(L_G), |L_G^-1|_2) in double: kappa2(L) = sqrt(cond2(U))"""
        if self._kappa is None:
            s = np.linalg.svd(np.asarray(self.U, dtype=np.float64), compute_uv=False)
            kg = li = 0.0
            if self.q:
                sg = np.linalg.svd(np.asarray(self.LG, dtype=np.float64), compute_uv=False)
                kg, li = sg[0] / sg[-1], 1.0 / sg[-1]
            self._kappa = (float(np.sqrt(s[0] / s[-1])), float(kg), float(li))
        return self._kappa

    def operands(self, Xq):
        """kq [n, m] and g [n, m, D] of m query points"""
        diff = np.asarray(Xq, dtype=LD)[None, :, :] - self.X[:, None, :]
        tau = np.sqrt((diff * diff).sum(2))
        return GR.phi(self.th, tau), GR.psi(self.th, tau)[:, :, None] * diff

    def items(self, Xq, min_v=1e-12):
        """m query points at once -> dict(v [m], grad [m, D], unit [m, D] (e_d / ((n + 32) u)), vunit [m], clamped [m],
        trend [m, D] the trend's part of grad, tunit [m, D] its own unit t_d / ((n + 32) u))"""
        Xq = np.asarray(Xq, dtype=LD).reshape(-1, self.D)
        m, D, n = len(Xq), self.D, self.n
        kq, g = self.operands(Xq)
        VW = forward_ld(self.L, np.concatenate([kq[:, :, None], g], 2).reshape(n, m * (1 + D))).reshape(n, m, 1 + D)
        V, W = VW[:, :, 0], VW[:, :, 1:]
        b = (V * V).sum(0)
        clamped = self.kself - b < LD(min_v)
        v = np.where(clamped, LD(min_v), self.kself - b)
        grad = np.where(clamped[:, None], LD(0), -LD(2) * (V[:, :, None] * W).sum(0))
        kl, kg, li = self.kappa()
        unit = kl * np.sqrt(np.asarray(b, dtype=np.float64))[:, None] * np.sqrt(np.asarray((W * W).sum(0), dtype=np.float64))
        vunit = kl * np.asarray(self.kself + b, dtype=np.float64)
        trend, tunit = np.zeros((m, D), dtype=LD), np.zeros((m, D))
        if self.q:
            q = self.q
            h = np.concatenate([np.ones((m, 1), dtype=LD), Xq], 1)[:, :q]                     # m x q
            z = forward_ld(self.LG, (h - kq.T @ self.C_H).T)                                   # q x m
            dh = np.zeros((D, q), dtype=LD)
            if q > 1:
                dh[np.arange(D), 1 + np.arange(D)] = LD(1)
            gC = np.einsum("nmd,nq->qmd", g, self.C_H)
            y = forward_ld(self.LG, (dh.T[:, None, :] - gC).reshape(q, m * D)).reshape(q, m, D)
            v = v + (z * z).sum(0)
            trend = LD(2) * (z[:, :, None] * y).sum(0)
            grad = grad + trend
            nz = np.sqrt(np.asarray((z * z).sum(0), dtype=np.float64))                        # m
            ny = np.sqrt(np.asarray((y * y).sum(0), dtype=np.float64))                        # m x D
            Mz = np.asarray(np.sqrt(((np.abs(h) + np.abs(kq).T @ np.abs(self.C_H)) ** 2).sum(1)), dtype=np.float64)
            My = np.asarray(np.sqrt(((np.abs(dh).T[:, None, :] + np.einsum("nmd,nq->qmd", np.abs(g), np.abs(self.C_H))) ** 2).sum(0)),
                            dtype=np.float64)
            tunit = kg * (kl * nz[:, None] * ny + li * (Mz[:, None] * ny + nz[:, None] * My))
            unit = unit + tunit
            vunit = vunit + kg * (kl * nz ** 2 + 2 * li * Mz * nz)
        return dict(v=v, grad=grad, unit=unit, vunit=vunit, clamped=np.asarray(clamped), trend=trend, tunit=tunit)


def item_vgrad_ref(th, X, sigma2, xq, min_v=1e-12, trend=None, C_H=None, LG=None):
    """the gradient [D] of one item's variance in long double, from the points, theta and sigma2 with its own Cholesky"""
    return PatchRef(th, X, sigma2, trend, C_H, LG).items(np.asarray(xq)[None, :], min_v)["grad"][0]


def mix_vgrad_ref(items, GV, v, t, plane, hp_v, wth):
    """dVq [D] of one query in long double and the magnitude sum_i (|wn_i^2 GV_i| + |2 wn_i v_i d wn_i|) [D] that the
    rounding bound of the blend is stated in.  items: the indices of the query's items (neighbours in hyperplane order, home
    last); GV [total, D], v [total], t [total], plane [total]; hp_v [P - 1, D] the pre-order normals."""
    items = list(items)
    tt = np.asarray(t, dtype=LD)[items]
    w = GR.phi(wth, np.abs(tt))
    w[-1] = LD(1)
    S = w.sum()
    wn = w / S
    vi = np.asarray(v, dtype=LD)[items]
    Gi = np.asarray(GV, dtype=LD)[items]                                # m x D
    nv = np.zeros((len(items), np.asarray(hp_v).shape[1]), dtype=LD)
    for k, it in enumerate(items[:-1]):
        nv[k] = np.asarray(hp_v, dtype=LD)[plane[it]]
    dw = -(GR.psi(wth, np.abs(tt)) * tt)[:, None] * nv                  # m x D
    dw[-1] = LD(0)
    dwn = (dw - wn[:, None] * dw.sum(0)[None, :]) / S
    a = (wn * wn)[:, None] * Gi
    b = (LD(2) * wn * vi)[:, None] * dwn
    return (a + b).sum(0), (np.abs(a) + np.abs(b)).sum(0)


# ---- the inputs of the per-item accuracy cases, shared by the CPU check of the unit and by the GPU tests
SIZES = [1, 127, 128, 129, 257, 300, 90, 200]       # one to three block rows; last_pairs 1, 4, 4, 1, 1, 2, 3, 3
SIGMA2 = {"f64": 1e-2, "f32": 0.05}
KAPPA_MAX = 1e3


def case_patches(seed, D, dtype):
    rng = np.random.default_rng(seed)
    Xs = [rng.uniform(-2, 2, (n, D)) for n in SIZES]
    return [x.astype(np.float32).astype(np.float64) for x in Xs] if dtype == "f32" else Xs


def case_items(seed, Xs, counts, dtype):
    """(xq [m, D], region [m]): per region random points around the patch, the first on a training point.  The error
    unit knows the conditioning of the solve, not that of the profile: near the edge of a compact support t = 1 - r has
    lost its digits before it is raised to a power, and far out a Gaussian's argument is large.  Where hundreds of points
    contribute, the well-conditioned ones carry the sums; a patch of one point has nothing else, so its queries stay
    within half a unit per coordinate of the point.  tests/test_vgrad_refs.py holds a plain evaluation in the model's own
    precision below one unit on exactly these inputs."""
    rng = np.random.default_rng(seed)
    D = Xs[0].shape[1]
    xq, region = [], []
    for r, cnt in enumerate(counts):
        if cnt == 0:
            continue
        pts = rng.uniform(-2.5, 2.5, (cnt, D))
        if len(Xs[r]) == 1:
            pts = Xs[r][0] + rng.uniform(-0.5, 0.5, (cnt, D))
        pts[0] = Xs[r][len(Xs[r]) // 2]
        xq.append(pts)
        region += [r] * cnt
    xq = np.vstack(xq)
    return (xq.astype(np.float32).astype(np.float64) if dtype == "f32" else xq), np.array(region, dtype=np.int32)

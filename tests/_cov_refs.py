"""An independent numpy.longdouble restatement of the joint posterior covariance of a query batch under the blend
(tests/test_cov_refs.py, tests/test_gpu_cov.py).  The profiles are those of tests/_grad_refs.py, the Cholesky and the
substitutions those of tests/_loo_refs.py: the construction of tests/_vgrad_refs.py's PatchRef.

Per region r (patch X, U = K + sigma2 I = L L^T) and its items x_1 .. x_m:

    V_a = L^-1 k(X, x_a)
    S[a, b] = k(x_a, x_b) - V_a . V_b                               for a != b, not clamped
    S[a, a] = max( k(x_a, x_a) + addend_a - |V_a|^2, min_v )

Blend, items of a query in the order of the mix (neighbours in hyperplane order, home last): w_i = phi_w(|t_i|) (home: 1),
wn_i = w_i / sum w:

    Cov[j, j'] = sum over the regions r that hold an item of both:  wn_{r,j} wn_{r,j'} S_r[a(j), a(j')]

and exactly 0 where two queries share no region.  The neighbour search of the reference can accept one leaf through two
hyperplanes; a query then holds two items of that region, and every pair of items of j and j' in a common region is a
term of the sum: that is the covariance of the two blends as they are.  The diagonal entry of such a query carries the
cross term of its two items, which the Vq of the mix (a sum of the items' variances) does not.

The error unit of a block entry, before the factor (n + 32) u (u = 2^-53 or 2^-24 by the model's type):

    e(a, b) = kappa2(L) ( k0 + |V_a| |V_b| ),   k0 = sqrt(k(x_a, x_a) k(x_b, x_b))

the construction of _vgrad_refs.py's vunit: the substitution perturbs V_a by n u kappa2(L) |V_a|, so the product V_a . V_b
moves by that times |V_b| and the same with a and b exchanged; the kernel value itself is a few roundings of k0, which
kappa2(L) >= 1 covers.  For a stationary family k0 = k(0); the Brownian-bridge families have no k(0) and take the geometric
mean of the two diagonal values, which is the same number where the kernel is stationary.  The unit of a blended entry is
the wn-weighted sum of its regions' units, factors (n_r + 32) u included.
"""
import numpy as np

import _grad_refs as GR
from _loo_refs import LD, cholesky_ld, forward_ld

BB10 = 10


def kern(th, A, B):
    """k(a_i, b_j) [len(A), len(B)] in the type of A: a stationary profile of the distance, or the Brownian bridge
    min(x, z) - x z as a product over the coordinates"""
    A, B = np.asarray(A), np.asarray(B)
    if th.family == BB10:
        a, b = A[:, None, :], B[None, :, :]
        return (np.minimum(a, b) - a * b).prod(2)
    diff = A[:, None, :] - B[None, :, :]
    return GR.phi(th, np.sqrt((diff * diff).sum(2)))


class RegionRef:
    """one patch: its long-double factor, built once and shared by every batch of items"""

    def __init__(self, th, X, sigma2):
        self.th = th
        self.X = np.asarray(X, dtype=LD)
        if self.X.ndim == 1:
            self.X = self.X[:, None]
        self.n, self.D = self.X.shape
        self.U = kern(th, self.X, self.X) + LD(sigma2) * np.eye(self.n, dtype=LD)
        self.L = cholesky_ld(self.U)
        s = np.linalg.svd(np.asarray(self.U, dtype=np.float64), compute_uv=False)
        self.kappa = float(np.sqrt(s[0] / s[-1]))            # kappa2(L) = sqrt(cond2(U))

    def cov(self, Xq, addend=None, min_v=1e-12):
        """dict(S [m, m] long double, unit [m, m] float64 = e(a, b) without (n + 32) u, V [n, m], clamped [m])"""
        Xq = np.asarray(Xq, dtype=LD).reshape(-1, self.D)
        m = len(Xq)
        V = forward_ld(self.L, kern(self.th, self.X, Xq))
        Kqq = kern(self.th, Xq, Xq)
        S = Kqq - V.T @ V
        S = (S + S.T) / LD(2)
        d = np.diag(Kqq) + (LD(0) if addend is None else np.asarray(addend, dtype=LD)) - (V * V).sum(0)
        clamped = d < LD(min_v)
        S[np.arange(m), np.arange(m)] = np.where(clamped, LD(min_v), d)
        nv = np.sqrt(np.asarray((V * V).sum(0), dtype=np.float64))
        kd = np.sqrt(np.abs(np.asarray(np.diag(Kqq), dtype=np.float64)))
        unit = self.kappa * (np.outer(kd, kd) + np.outer(nv, nv))
        return dict(S=S, unit=unit, V=V, clamped=np.asarray(clamped))


def region_cov_ref(th, X, sigma2, Xq, addend=None, min_v=1e-12):
    """the block S [m, m] of one region in long double, from the points, theta and sigma2 with its own Cholesky"""
    return RegionRef(th, X, sigma2).cov(Xq, addend, min_v)["S"]


def blend_weights(item_offsets, t, wth):
    """wn [total] in long double: the normalised weights of the mix, items of a query contiguous with the home item last"""
    off = np.asarray(item_offsets, dtype=np.int64)
    w = GR.phi(wth, np.abs(np.asarray(t, dtype=LD)))
    w[off[1:] - 1] = LD(1)
    wn = np.empty_like(w)
    for j in range(len(off) - 1):
        seg = w[off[j]:off[j + 1]]
        wn[off[j]:off[j + 1]] = seg / seg.sum()
    return wn


def mix_cov_ref(items, S_blocks, t, wth, unit_blocks=None):
    """Cov [Nq, Nq] in long double (and its unit, float64, with unit_blocks) from the item lists of pmk_query_debug.
    items: (item_offsets [Nq + 1], item_region [total]); S_blocks[r] = (query index of each row, S_r) for every region with
    items; t [total] the items' signed distances; unit_blocks[r]: the unit of S_r with its factor (n_r + 32) u."""
    off, reg = np.asarray(items[0], dtype=np.int64), np.asarray(items[1], dtype=np.int64)
    Nq = len(off) - 1
    wn = blend_weights(off, t, wth)
    query_of = np.repeat(np.arange(Nq), np.diff(off))
    Cov = np.zeros((Nq, Nq), dtype=LD)
    unit = np.zeros((Nq, Nq))
    for r, (idx, S) in S_blocks.items():
        idx = np.asarray(idx, dtype=np.int64)
        sel = np.nonzero(reg == r)[0]
        sel = sel[np.argsort(query_of[sel], kind="stable")]
        assert np.array_equal(query_of[sel], idx), r          # the rows ascend in the query index, items in their order
        ww = np.outer(wn[sel], wn[sel])
        # a query may hold two items of a region (one leaf accepted through two hyperplanes): every pair is a term
        np.add.at(Cov, (idx[:, None], idx[None, :]), ww * np.asarray(S, dtype=LD))
        if unit_blocks is not None:
            np.add.at(unit, (idx[:, None], idx[None, :]), np.asarray(ww, dtype=np.float64) * unit_blocks[r])
    return (Cov, unit) if unit_blocks is not None else Cov


def shared_region_mask(items):
    """[Nq, Nq] bool: the two queries have an item in a common region"""
    off, reg = np.asarray(items[0], dtype=np.int64), np.asarray(items[1], dtype=np.int64)
    Nq = len(off) - 1
    query_of = np.repeat(np.arange(Nq), np.diff(off))
    A = np.zeros((Nq, int(reg.max()) + 1 if len(reg) else 1), dtype=bool)
    A[query_of, reg] = True
    return (A.astype(np.int64) @ A.T.astype(np.int64)) > 0


def plain_region_cov(th, X, sigma2, Xq, T_, addend=None, min_v=1e-12):
    """the block in the model's own precision T_ (float64 or float32) with numpy and LAPACK: what a careful evaluation in
    that precision gives; the last subtraction and the clamp in double, as on the device"""
    import scipy.linalg as sla
    X, Xq = np.asarray(X).astype(T_), np.asarray(Xq).astype(T_)
    n = len(X)
    U = (kern(th, X, X) + T_(sigma2) * np.eye(n, dtype=T_)).astype(T_)
    L = sla.cholesky(U, lower=True)
    assert L.dtype == T_
    V = sla.solve_triangular(L, kern(th, X, Xq).astype(T_), lower=True)
    Kqq = kern(th, Xq, Xq).astype(T_).astype(np.float64)
    S = Kqq - (V.T @ V).astype(np.float64)
    d = np.diag(Kqq) + (0.0 if addend is None else np.asarray(addend, dtype=np.float64)) - (V * V).sum(0).astype(np.float64)
    S[np.arange(len(Xq)), np.arange(len(Xq))] = np.maximum(d, min_v)
    return S

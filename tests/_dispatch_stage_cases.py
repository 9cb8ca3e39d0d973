"""Inputs and references of the dispatch tests of the later stages (tests/test_dispatch_stage_refs.py on the CPU,
tests/test_gpu_dispatch_stages.py on the GPU): host data only, so that what the CPU file asserts of an input holds of the
input the GPU file runs.

The workload is that of tests/test_gpu_dispatch.py in its "ragged" shape: 600 points in [-1, 1]^D, four leaves whose eps-sets
hold two block rows, 100 points, two block rows and exactly 128 points, 257 queries, the plan radius 0.3.  fp32 cases round
points and queries through float32 (tests/_cov_cases.py: rnd).  Every stage runs with the sigma2 of its own cases module,
where the preconditions of its error unit were established: tests/_vgrad_refs.py for both gradients, tests/_cov_cases.py for
the covariance, tests/_block_cases.py for block kriging (10 in fp32).

A hyperparameter list is named by a key and holds (family, a, sigma2) per patch:
    "spline34", "spline32"      uniform: a = 1, the stage's sigma2 (THETAS of tests/test_gpu_dispatch.py)
    "distinct34", "distinct32"  DISTINCT: a_r = a (1 + r / 4), sigma2_r = sigma2 (1 + r / 2); patch 0 is the uniform one.
                                At D = 4: a_r = a / (1 + r / 4), see below
    "mixed"                     MIXED of tests/test_gpu_dispatch.py: Spline34 and Spline32 alternating
and, on the D = 2 input inside (0.05, 0.95)^2 only, "bb": Spline34, BB10, RQ, BB10 (the kernels of tests/_cov_cases.py; the
Brownian bridge is a product over the coordinates).

Three inputs did not meet what tests/test_dispatch_stage_refs.py asserts and were changed; no bound was:
  * D = 4, DISTINCT: with a_r = 1.25 to 1.75 (supports of 0.8 to 0.57) a query has 0 to 5 points of its patch inside the
    support, some at r = 0.97 and more, where t = 1 - r has lost the digits that the unit of tests/_vgrad_refs.py assumes
    are carried by other points (a plain float64 evaluation reaches 1.001 units; a query with no point has no unit at all).
    The ranges grow instead: a_r = a / (1 + r / 4), 70 and more points per query.
  * fp32 covariance at D = 1 and D = 2: sigma2 = 10 and 0.2, not 0.05.  600 points on a segment of length 2 (in a square
    of side 2) leave a posterior so tight that the Spline34 and the Spline32 blocks of a region differ by 32 to 73 (31 to
    49) units only; with these values by 619 (149) and more.  At D = 1 sigma2 = 1 still gives 87.
  * D = 1, fp32, block kriging: sigma2 = 100, not 10: the mixed-sign aggregates lie 33 units above their floor (100: 126).
And one case that the stages' own sigma2 cannot serve at all: a Spline32 descriptor (a = 1) handed to a stage on a Spline34
fit is no posterior, k_eval(x, x) - |L_fit^-1 k_eval|^2 need not be positive, and with sigma2 = 0.01 or 0.05 it is negative
for 104 to 340 of the items (any range of the Spline32 kernel between 1 and 2 leaves 11 and more clamped).  Those cases run
on a fit with sigma2 = 1 (TWO_KERNEL; the fp32 covariance and block kriging at D = 1 keep the 10 and 100 from above), where
no item is clamped and every aggregate clears its floor by 100 units.

TwoKernel is the reference of a stage evaluated with theta_eval on a patch factored with theta_fit: what a launcher computes
that is handed a descriptor other than the model's.
"""
import numpy as np

import patchmixturekriging_amd as pmk
from oracle import oracle as O
import _block_cases as BC
import _cov_cases as CC
import _cov_multi_refs as CMR
import _cov_refs as CR
import _grad_refs as GR
import _vgrad_refs as VR
from _loo_refs import LD, cholesky_ld, forward_ld
from test_gpu_dispatch import A, DELTA, EPS_OVERLAP, LEVELS, MIXED, OWTH, P, RADIUS, SHAPES, THETAS, WTH, _data

STAGES = ("grad", "vgrad", "cov", "block")
STAGE_SIGMA2 = {"grad": VR.SIGMA2, "vgrad": VR.SIGMA2, "cov": CC.SIGMA2, "block": BC.SIGMA2}
SIGMA2_AT = {("cov", 1, "f32"): 10.0, ("cov", 2, "f32"): 0.2, ("block", 1, "f32"): 100.0}         # inputs that were changed: see above
# a Spline32 descriptor on a Spline34 fit: (D, dtype) -> sigma2 of the fit per stage, see above
TWO_KERNEL = {(3, "f64"): dict(grad=1.0, vgrad=1.0, cov=1.0, block=1.0), (1, "f32"): dict(grad=1.0, vgrad=1.0, cov=10.0, block=100.0)}
U_OF, KAPPA_MAX, RATIO_MAX, MARGIN_MIN = CC.U_OF, CC.KAPPA_MAX, CC.RATIO_MAX, BC.MARGIN_MIN
APART_MIN = 100.0                                            # units by which two kernels must differ to be told apart
DIMS, DTYPES, FAMS, RCOLS = (1, 2, 3, 4), ("f64", "f32"), ("spline34", "spline32"), 2
TREND = "linear"                                             # of the multi-output covariance form
BB_NAMES = ["spline34", "bb10", "rq", "bb10"]
BB_DTYPES = ("f64",)                                         # fp32 with sigma2 = 10: six RQ aggregates within 100 units of their floor
BB_SCALE = 0.45                                              # [-1, 1] -> [0.05, 0.95]

_PMK = {"spline34": pmk.Spline34KernelType, "spline32": pmk.Spline32KernelType}
_ORC = {"spline34": O.SPLINE34, "spline32": O.SPLINE32}
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def kernel(fam, a=A):
    """(the package's kernel, the oracle's descriptor)"""
    if fam in CC.FAMILIES and fam not in _PMK:
        return CC.FAMILIES[fam]
    return THETAS[fam] if a == A else (_PMK[fam](a), O.kernel(_ORC[fam], a))


def sigma2(stage, D, dtype):
    return SIGMA2_AT.get((stage, D, dtype), STAGE_SIGMA2[stage][dtype])


def hyper(key, sigma2, D):
    """[(family, a, sigma2)] per patch"""
    if key in FAMS:
        return [(key, A, sigma2)] * P
    if key in ("distinct34", "distinct32"):
        scale = [1 + r / 4 for r in range(P)]
        return [("spline3" + key[-1], A * scale[r] if D < 4 else A / scale[r], sigma2 * (1 + r / 2)) for r in range(P)]
    if key == "mixed":
        return [(f, A, sigma2) for f in MIXED]
    assert key == "bb", key
    return [(f, A, sigma2) for f in BB_NAMES]


class Workload:
    """the ragged batch of tests/test_gpu_dispatch.py with R = 2 target columns, the oracle's plan and the groups of block
    kriging: runs of 1, 2, 3, .. consecutive queries, coefficients of a perturbed block average with mixed signs"""

    LEVELS, DELTA = LEVELS, DELTA

    def __init__(self, D, dtype, unit_square=False):
        d = _data(D, "ragged")
        self.D, self.dtype, self.RADIUS, self.wth, self.owth = D, dtype, RADIUS, WTH, OWTH
        self.X, self.root, Xs, Xq = d["X"], d["root"], d["X_set"], d["Xq"]
        if unit_square:                                      # the same points, inside (0.05, 0.95)^D, under a tree of their own
            self.X, Xq, self.RADIUS = 0.5 + BB_SCALE * self.X, 0.5 + BB_SCALE * Xq, BB_SCALE * RADIUS
            self.root, _, _ = pmk.setuppartition(self.X, LEVELS)
            Xs, _, _, _ = pmk.organizetrainingsets(self.root, LEVELS, self.X, BB_SCALE * EPS_OVERLAP)
            Xs = [x[:SHAPES["ragged"].get(r, len(x))] for r, x in enumerate(Xs)]
            self.wth, self.owth = pmk.Spline34KernelType(1 / self.RADIUS), O.kernel(O.SPLINE34, 1 / self.RADIUS)
            assert 0.05 < min(self.X.min(), Xq.min()) and max(self.X.max(), Xq.max()) < 0.95
        self.Xs, self.Xq = [CC.rnd(np.ascontiguousarray(x), dtype) for x in Xs], CC.rnd(Xq, dtype)
        assert [(len(x) + 127) // 128 for x in self.Xs] == [2, 1, 2, 1] and len(self.Xs[3]) == 128
        self.Ys = [np.ascontiguousarray(np.stack([np.sin(3 * x[:, 0]) + x[:, -1] ** 2, np.cos(2 * x[:, 0] - x[:, -1])], 1))
                   for x in self.Xs]
        self.items = CC.oracle_items(self)                   # (item_offsets, item_region, item_t)
        off, reg = self.items[0], self.items[1]
        self.query_of = np.repeat(np.arange(len(off) - 1), np.diff(off))
        self.sel = {r: np.nonzero(reg == r)[0] for r in range(P)}        # ascending in the query: the rows of a block
        self.group = BC.cut(len(self.Xq), tuple(range(1, 64)))
        self.F = int(self.group[-1]) + 1
        rng = np.random.default_rng(9200 + D)
        self.a = BC.averages(self.group, rng) * np.where(rng.uniform(size=len(self.Xq)) < 0.4, -1.0, 1.0)

    def points(self, r):
        """the query points of region r's items, in the row order of its block"""
        return self.Xq[self.query_of[self.sel[r]]]


def workload(D, dtype, unit_square=False):
    return cached(("w", D, dtype, unit_square), lambda: Workload(D, dtype, unit_square))


# ------------------------------------------------------------------------------------------ references, one factor per patch
class PatchRefOf(VR.PatchRef):
    """the PatchRef of tests/_vgrad_refs.py on the long-double factor of a TrendRegionRef, and on its C_H and L_G where it has
    a trend: the same U and L and the same basis (1, x), built once"""

    def __init__(self, ref):
        self.th, self.X, self.n, self.D, self.U, self.L = ref.th, ref.X, ref.n, ref.D, ref.U, ref.L
        self.kself = GR.phi(ref.th, np.zeros(1, dtype=LD))[0]
        self.C_H, self.LG, self.q = (ref.CH, ref.LG, ref.q) if ref.q else (None, None, 0)
        self._kappa = (ref.kappa, ref.kappa_G, ref.norm_LGinv) if ref.q else (ref.kappa, 0.0, 0.0)


class _Factored(CR.RegionRef):
    """the RegionRef part of a TrendRegionRef taken from `base`, an existing reference: no second Cholesky"""
    base = None

    def __init__(self, th, X, sigma2):
        self.__dict__.update(self.base.__dict__)


def region_ref(w, r, h, trend=None):
    """the TrendRegionRef of patch r of workload w under h = (family, a, sigma2); the factor is shared by every trend"""
    fam, a, s2 = h
    oth = kernel(fam, a)[1]
    key = ("ref", w.D, w.dtype, w.RADIUS, r, fam, a, s2)
    base = cached(key + (None,), lambda: CMR.TrendRegionRef(oth, w.Xs[r], s2, None))
    if trend is None:
        return base
    on_factor = type("TrendOnFactor", (CMR.TrendRegionRef, _Factored), {"base": base})
    return cached(key + (trend,), lambda: on_factor(oth, w.Xs[r], s2, trend))


def patch_ref(w, r, h, trend=None, ev=None):
    """the PatchRef of patch r; ev = (family, a): evaluated with that kernel on the patch's own factor, C_H and L_G"""
    ref = cached(("pref", w.D, w.dtype, w.RADIUS, r, trend) + tuple(h), lambda: PatchRefOf(region_ref(w, r, h, trend)))
    return ref if ev is None else with_theta(ref, kernel(*ev)[1])


class TwoKernel:
    """A stage evaluated with theta_eval on a patch factored with theta_fit and sigma2 (U_fit = K_fit + sigma2 I = L L^T):

        V_a = L^-1 k_eval(X, x_a),  S[a, b] = k_eval(x_a, x_b) - V_a . V_b,  S[a, a] = max(k_eval(x_a, x_a) + addend_a - |V_a|^2, min_v)
        W_d = L^-1 (psi_eval(tau) (x_d - X_d)),  d v / dx_d = -2 V . W_d, exactly 0 where the clamp holds

    with the units of tests/_cov_refs.py and tests/_vgrad_refs.py on kappa2(L) of the factor in use.  It answers cov() as a
    RegionRef and items() as a PatchRef do, without a trend, and serves tests/_block_refs.py: block_ref as a region's reference.
    The gradient of an item mean needs no factor: it is GR.item_grad_ref with theta_eval on the model's weights."""

    trend, q = None, 0

    def __init__(self, th_fit, X, sigma2, th_eval, L=None, kappa=None):
        self.th = th_eval
        self.X = np.asarray(X, dtype=LD).reshape(len(X), -1)
        self.n, self.D = self.X.shape
        if L is None:
            U = CR.kern(th_fit, self.X, self.X) + LD(sigma2) * np.eye(self.n, dtype=LD)
            L = cholesky_ld(U)
            s = np.linalg.svd(np.asarray(U, dtype=np.float64), compute_uv=False)
            kappa = float(np.sqrt(s[0] / s[-1]))
        self.L, self.kappa = L, kappa

    @classmethod
    def on(cls, ref, th_eval):
        """on the factor of a RegionRef"""
        return cls(None, ref.X, None, th_eval, ref.L, ref.kappa)

    def cov(self, Xq, addend=None, min_v=1e-12):
        Xq = np.asarray(Xq, dtype=LD).reshape(-1, self.D)
        m = len(Xq)
        V = forward_ld(self.L, CR.kern(self.th, self.X, Xq))
        Kqq = CR.kern(self.th, Xq, Xq)
        S = Kqq - V.T @ V
        S = (S + S.T) / LD(2)
        b = (V * V).sum(0)
        d = np.diag(Kqq) + (LD(0) if addend is None else np.asarray(addend, dtype=LD)) - b
        clamped = d < LD(min_v)
        S[np.arange(m), np.arange(m)] = np.where(clamped, LD(min_v), d)
        nv, kd = np.sqrt(np.asarray(b, dtype=np.float64)), np.sqrt(np.abs(np.asarray(np.diag(Kqq), dtype=np.float64)))
        return dict(S=S, unit=self.kappa * (np.outer(kd, kd) + np.outer(nv, nv)), V=V, clamped=np.asarray(clamped))

    def items(self, Xq, min_v=1e-12):
        Xq = np.asarray(Xq, dtype=LD).reshape(-1, self.D)
        diff = Xq[None, :, :] - self.X[:, None, :]                                         # n x m x D
        tau = np.sqrt((diff * diff).sum(2))
        V = forward_ld(self.L, GR.phi(self.th, tau))
        g = GR.psi(self.th, tau)[:, :, None] * diff
        W = forward_ld(self.L, g.reshape(self.n, -1)).reshape(g.shape)
        b = (V * V).sum(0)
        kself = GR.phi(self.th, np.zeros(1, dtype=LD))[0]
        clamped = kself - b < LD(min_v)
        grad = np.where(clamped[:, None], LD(0), -LD(2) * (V[:, :, None] * W).sum(0))
        unit = self.kappa * np.sqrt(np.asarray(b, dtype=np.float64))[:, None] * np.sqrt(np.asarray((W * W).sum(0), dtype=np.float64))
        return dict(v=np.where(clamped, LD(min_v), kself - b), grad=grad, unit=unit, clamped=np.asarray(clamped))


def lapack_weights(ref, Y, dtype):
    """U^-1 Y by LAPACK in double from the reference's matrix, rounded to the model's type: weights such as a model of this
    patch holds.  The GPU file takes the device's own (tests/test_gpu_grad.py)."""
    return CC.rnd(np.linalg.solve(np.asarray(ref.U, dtype=np.float64), np.asarray(Y, dtype=np.float64)), dtype)


_LIP = {}


def lip(oth):
    key = (oth.family, oth.p[0], oth.p[1])
    if key not in _LIP:
        _LIP[key] = GR.lip(oth)
    return _LIP[key]


def grad_unit(oth, n, Cw, u):
    """[R]: the bound of tests/test_gpu_grad.py for the gradient of an item mean on a patch of n points with weights Cw"""
    return (n + 32) * u * lip(oth) * np.abs(np.asarray(Cw).reshape(n, -1)).sum(0)


def item_grads(oth, X, Cw, xq, T_=LD):
    """G [m, R, D] of GR.item_grad_ref for m query points at once, in the type T_"""
    X, Cw, xq = np.asarray(X).astype(T_), np.asarray(Cw).astype(T_).reshape(len(X), -1), np.asarray(xq).astype(T_)
    diff = xq[:, None, :] - X[None, :, :]                                                  # m x n x D
    tau = np.sqrt((diff * diff).sum(2))
    return np.einsum("mnd,nr->mrd", GR.psi(oth, tau)[:, :, None] * diff, Cw)


def hypers(w, key, stage):
    """the list of a key under the stage's sigma2; a key (family, sigma2) is that uniform list whatever the stage"""
    if isinstance(key, tuple):
        return hyper(key[0], key[1], w.D)
    return hyper(key, sigma2(stage, w.D, w.dtype), w.D)


def refs_of(w, key, stage, trend=None, ev=None, only=None):
    """{r: reference} of the regions that hold items; ev = (family, a): TwoKernel with that kernel, in region `only` or in all"""
    hs = hypers(w, key, stage)
    out = {r: region_ref(w, r, hs[r], trend) for r in range(P) if len(w.sel[r])}
    if ev is not None:
        for r in (out if only is None else [only]):
            out[r] = TwoKernel.on(out[r], kernel(*ev)[1]) if trend is None else with_theta(out[r], kernel(*ev)[1])
    return out


def with_theta(ref, th_eval):
    """a TrendRegionRef or a PatchRef that evaluates th_eval on the factor, C_H and L_G of `ref`: TwoKernel under a trend
    (rho = h - C_H^T k_eval).  Without a trend it is TwoKernel itself, which tests/test_dispatch_stage_refs.py asserts."""
    import copy
    out = copy.copy(ref)
    out.th = th_eval
    if hasattr(out, "kself"):                                # a PatchRef: k_eval(x, x)
        out.kself = GR.phi(th_eval, np.zeros(1, dtype=LD))[0]
    return out


def block_out(w, key, ev=None, only=None):
    """BR.block_ref of the workload's groups on the oracle's plan"""
    import _block_refs as BR
    return cached(("block", w.D, w.dtype, w.RADIUS, key, ev, only), lambda: BR.block_ref(
        w.items[:2], w.items[2], w.owth, w.group, w.a, w.F, refs_of(w, key, "block", None, ev, only), w.Xq, U_OF[w.dtype]))


def stage_outputs(w, key, stage, r, ev=None):
    """(reference values, unit with its factor (n + 32) u, items or aggregates that sit on their clamp) of one region of one
    stage under the list `key`, flattened.  ev: a (family, a) to evaluate the stage with in place of the patch's own
    (TwoKernel).  grad: the gradients of the item means on the LAPACK weights of the patch; vgrad: the gradients of the item
    variances; cov: the region's block; block: kappa - |Vbar|^2 of the region's aggregates, "block:kappa" and "block:vn2"
    either piece alone (block_self_kernel and block_strip_kernel make one each)."""
    dtype = w.dtype
    h = hypers(w, key, stage[:5])[r]
    ref, u, xq = region_ref(w, r, h), U_OF[dtype], w.points(r)
    oth = kernel(h[0], h[1])[1]
    oev = oth if ev is None else kernel(*ev)[1]
    two = ref if ev is None else TwoKernel.on(ref, oev)
    if stage == "grad":
        Cw = cached(("C", w.D, dtype, w.RADIUS, r) + tuple(h), lambda: lapack_weights(ref, w.Ys[r], dtype))
        G = item_grads(oev, w.Xs[r], Cw, xq)
        return G.reshape(-1), np.broadcast_to(grad_unit(oth, ref.n, Cw, u)[None, :, None], G.shape).reshape(-1), 0
    if stage == "vgrad":
        out = (patch_ref(w, r, h) if ev is None else two).items(xq)
        return out["grad"].reshape(-1), ((ref.n + 32) * u * out["unit"]).reshape(-1), int(out["clamped"].sum())
    if stage == "cov":
        c = two.cov(xq)
        return c["S"].reshape(-1), ((ref.n + 32) * u * c["unit"]).reshape(-1), int(c["clamped"].sum())
    aggs = [x for x in block_out(w, key, ev, None if ev is None else r)["aggs"] if x["region"] == r]
    if stage != "block":                                     # "block:kappa", "block:vn2": one piece alone, for the separation
        return np.array([x[stage[6:]] for x in aggs], dtype=LD), np.array([x["unit"] for x in aggs]), 0
    return (np.array([x["kappa"] - x["vn2"] for x in aggs], dtype=LD), np.array([x["unit"] for x in aggs]),
            sum(1 for x in aggs if x["margin"] < MARGIN_MIN))


def ratio(err, unit):
    """max err / unit over the entries with a unit; an entry without one admits no error"""
    err, unit = np.asarray(err, dtype=np.float64).reshape(-1), np.asarray(unit, dtype=np.float64).reshape(-1)
    if np.any(err[unit == 0] > 0):
        return float("inf")
    return float((err[unit > 0] / unit[unit > 0]).max()) if np.any(unit > 0) else 0.0


def apart(w, key, stage, r, ev):
    """the largest distance, in units, between region r's outputs and the same stage evaluated with `ev`"""
    a, unit, _ = stage_outputs(w, key, stage, r)
    b, _, _ = stage_outputs(w, key, stage, r, ev)
    return ratio(np.abs(a - b), unit)


def plain(w, key, stage):
    """the worst ratio of a plain numpy / LAPACK evaluation of the stage in the model's precision against the reference:
    tests/test_vgrad_refs.py: _plain_item_grads, tests/_cov_multi_refs.py: plain_region_cov (without and with the trend of
    the multi-output form), tests/_block_refs.py: plain_block_var with each patch's own sigma2, and for the gradient of the
    mean the reference's own formula in that precision on the same weights"""
    def make():
        import _block_refs as BR
        from test_vgrad_refs import _plain_item_grads
        T_ = np.float64 if w.dtype == "f64" else np.float32
        hs, worst = hypers(w, key, stage), 0.0
        if stage == "block":
            out = block_out(w, key)
            wgt, query_of = BR.item_weights(w.items[:2], w.items[2], w.owth, w.a)
            wgt, Var = np.asarray(wgt, dtype=np.float64), np.zeros(w.F)
            for r, f, mem in BR.aggregates(w.items[:2], w.group):
                S = CMR.plain_region_cov(kernel(*hs[r][:2])[1], w.Xs[r], hs[r][2], w.Xq[query_of[mem]], T_, None)
                Var[f] += wgt[mem] @ S @ wgt[mem]
            return ratio(np.abs(Var - np.asarray(out["Var"], dtype=np.float64)), out["unit"])
        for r in range(P):
            oth, xq = kernel(*hs[r][:2])[1], w.points(r)
            val, unit, _ = stage_outputs(w, key, stage, r)
            if stage == "grad":
                Cw = _CACHE[("C", w.D, w.dtype, w.RADIUS, r) + tuple(hs[r])]
                got = item_grads(oth, w.Xs[r], Cw, xq, T_)
            elif stage == "vgrad":
                got = _plain_item_grads(oth, w.Xs[r], hs[r][2], xq, None, T_)
                # under the trend of the second form: the sum, and the trend's part in its own unit (tests/test_vgrad_refs.py)
                o = patch_ref(w, r, hs[r], TREND).items(xq)
                both = _plain_item_grads(oth, w.Xs[r], hs[r][2], xq, TREND, T_)
                nu = (len(w.Xs[r]) + 32) * U_OF[w.dtype]
                part = np.maximum(np.abs(both - got - o["trend"]).astype(np.float64) - 4 * 2.0 ** -53 * np.abs(o["grad"]).astype(np.float64), 0.0)
                worst = max(worst, ratio(np.abs(both - o["grad"]), nu * o["unit"]), ratio(part, nu * o["tunit"]))
            else:
                got = CR.plain_region_cov(oth, w.Xs[r], hs[r][2], xq, T_)
                c = region_ref(w, r, hs[r], TREND).cov(xq)
                trend = CMR.plain_region_cov(oth, w.Xs[r], hs[r][2], xq, T_, TREND)
                worst = max(worst, ratio(np.abs(trend - c["S"]), (len(w.Xs[r]) + 32) * U_OF[w.dtype] * c["unit"]))
            worst = max(worst, ratio(np.abs(np.asarray(got, dtype=LD).reshape(-1) - val), unit))
        return worst
    return cached(("plain", w.D, w.dtype, w.RADIUS, key, stage), make)

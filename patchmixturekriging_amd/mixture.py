"""Mixture-of-GP model: Python mirror of src/RKHS/mixtureGP.jl over the C ABI.

Mutating Julia functions keep their name with a trailing underscore instead of the bang:
fitmixtureGP! -> fitmixtureGP_, querymixtureGP! -> querymixtureGP_.  Region indices are 0-based.
"""
import ctypes as C

import numpy as np

from . import _lib
from .context import default_context
from .kernels import as_points
from .partition import _native, findpartition, hyperplane_arrays

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int64)

GET_C, GET_L, GET_K, GET_LINV_DIAG = 0, 1, 2, 3


def _d(a):
    return a.ctypes.data_as(_dp)


def _i(a):
    return a.ctypes.data_as(_ip)


def _i32(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _dps(arrays, P):
    """the array of P pointers to a list of float64 arrays (one per patch)"""
    return (_dp * P)(*[_d(a) for a in arrays])


class GlobalArray:
    """a float64 array of all points, on the host (numpy) or on the device (anything with __cuda_array_interface__, such
    as a torch tensor): address, shape and strides in elements, validated without any device call.  `keep` holds the
    owner alive while the library reads it."""

    def __init__(self, a, what):
        self.keep = a
        if isinstance(a, np.ndarray):
            if a.dtype != np.float64:
                raise ValueError("%s must be float64, not %s" % (what, a.dtype))
            self.device, self.ptr, self.shape = False, a.ctypes.data, tuple(a.shape)
            strides = a.strides
        else:
            try:
                cai = a.__cuda_array_interface__
            except (AttributeError, TypeError, RuntimeError):
                raise ValueError("%s must be a numpy array or a device array (__cuda_array_interface__), not %s"
                                 % (what, type(a).__name__))
            if cai["typestr"] not in ("<f8", "=f8", "|f8"):
                raise ValueError("%s must be float64, not %s" % (what, cai["typestr"]))
            self.device, self.ptr, self.shape = True, int(cai["data"][0]), tuple(int(v) for v in cai["shape"])
            strides = cai.get("strides")
            if strides is None:                 # C-contiguous
                strides, acc = [], 8
                for v in reversed(self.shape):
                    strides.insert(0, acc)
                    acc *= max(v, 1)
        if any(int(v) % 8 for v in strides):
            raise ValueError("%s: strides must be whole float64 elements" % what)
        self.strides = tuple(int(v) // 8 for v in strides)
        self.what = what

    def vector(self, N):
        """N contiguous values"""
        if self.shape != (int(N),):
            raise ValueError("%s must have shape (%d,), not %s" % (self.what, N, self.shape))
        if N > 1 and self.strides != (1,):
            raise ValueError("%s must be contiguous" % self.what)
        return self

    def points(self, D=None):
        """point-major (N, D), C-contiguous"""
        if len(self.shape) != 2 or (D is not None and self.shape[1] != D):
            raise ValueError("%s must have shape (N, %s), not %s" % (self.what, "D" if D is None else D, self.shape))
        N, D = self.shape
        if N * D > 0 and (self.strides[1] != 1 and D > 1 or self.strides[0] != D and N > 1):
            raise ValueError("%s must be C-contiguous" % self.what)
        return self

    def columns(self, N):
        """(N, R) column-major with leading dimension ld >= N (a vector is one column) -> R, ld"""
        if len(self.shape) == 1:
            self.vector(N)
            return 1, max(int(N), 1)
        if len(self.shape) != 2 or self.shape[0] != int(N):
            raise ValueError("%s must have shape (%d, R), not %s" % (self.what, N, self.shape))
        R = self.shape[1]
        if not 1 <= R <= MAX_OUTPUTS:
            raise ValueError("R = %d target columns, outside 1..%d" % (R, MAX_OUTPUTS))
        if N > 1 and self.strides[0] != 1:
            raise ValueError("%s must be column-major (Fortran order)" % self.what)
        ld = self.strides[1] if R > 1 else max(int(N), 1)
        if ld < N:
            raise ValueError("%s: leading dimension %d < N = %d" % (self.what, ld, N))
        return R, ld


def _refuse_closure_kernel(theta, who):
    """the tree route packs the tree's own D coordinates: the closure-carrying (warp-feature and DPP) kernels evaluate on
    more coordinates than the tree has, or need a point-dependent diagonal term"""
    if hasattr(theta, "diag_addend") or getattr(theta, "warped", False):
        raise TypeError("%s: closure-carrying kernels (%s) are not available on a model built from a tree and global "
                        "points; build the model from lists of patches" % (who, type(theta).__name__))


class PosDefException(np.linalg.LinAlgError):
    """cholesky(U) of the reference throws PosDefException(k) (mixtureGP.jl:109)"""

    def __init__(self, patch, k):
        super().__init__("patch %d: matrix is not positive definite; Cholesky factorization failed "
                         "(leading minor %d)" % (patch, k))
        self.patch = patch
        self.info = k


class DeviceModel:
    """pmk_model: the fitted per-patch factors, resident on the GPU"""

    # The mirror of the library's model state (include/pmk.h), so that a call in the wrong state is refused before any
    # device call.  These are the values of a model just created from points; every birth path (the constructor,
    # from_tree, a test's object.__new__) sets only what differs, and only the calls named here change them.
    _from_tree = False      # built by from_tree: the *_global calls serve it, append / remove take their _global forms
    _all_leaves = False     # from_tree: the model holds every leaf of its tree, not a shard (blended leave-one-out)
    _has_factor = False     # a factor is resident: fit, fit_patches, from_factors; new targets or addends drop it
    _has_targets = True     # the model holds y: False only on a model built by from_factors
    _has_kernels = False    # the kernels of the factor are known: fit, fit_patches, set_kernels
    _loo_done = False       # loo() ran on the resident factor; a new factor and changed rows make it stale
    _multi_solved = False   # solve_multi ran on it; stale after a new factor, changed rows, new R columns, set_trend
    R = 0                   # the columns of set_targets_multi(_global); changed rows (reserve, append, remove) discard them
    _X = None               # X: the points of every patch (from_tree: cut from _X_global on first use)
    _X_global = None        # from_tree on a host array: that array, extended by append_global
    _index = None           # patch_index() of a from_tree model, read back once; append_global and remove_global reset it
    theta = None            # of the last fit(); None after fit_patches (thetas, sigma2s then)
    sigma2 = None

    def _new_factor(self):
        """fit, fit_patches: the factor, z and c are those of the kernels given; d and the multi-output weights are stale"""
        self._has_factor = self._has_targets = self._has_kernels = True
        self._loo_done = self._multi_solved = False

    def _rows_changed(self):
        """reserve, append, remove: loo() is stale and the multi-output targets are discarded (set_targets_multi again)"""
        self._loo_done = self._multi_solved = False
        self.R = 0

    def _targets_replaced(self):
        """set_targets(_global), set_diag(_global): the resident factor no longer belongs to the model's y and addends"""
        self._has_factor = False

    def __init__(self, X_parts, y_parts, ctx=None, _factors=None, dtype="f64"):
        self.ctx = ctx or default_context()
        L = self.ctx.L
        self.X = [as_points(x) for x in X_parts]
        self.P = len(self.X)
        if self.P == 0:
            raise ValueError("no patches")
        self.D = self.X[0].shape[1]
        self.n = np.array([x.shape[0] for x in self.X], dtype=np.int64)
        ys = [np.ascontiguousarray(y, dtype=np.float64) for y in y_parts]
        for x, y in zip(self.X, ys):
            if x.shape[0] != len(y):
                raise ValueError("length(c) == length(X) must hold per patch")     # mixtureGP.jl:298
        P = self.P
        h = C.c_void_p()
        self.dtype = dtype
        if _factors is None:
            # dtype "f32": fp32 storage + fp32 MFMA on the device (BASELINE config E); host buffers stay float64
            _lib.check(L.pmk_model_create_ex(self.ctx.h, self.D, P, _i(self.n), _dps(self.X, P), _dps(ys, P),
                                             {"f64": 0, "f32": 1}[dtype], C.byref(h)), "pmk_model_create")
        else:
            Ls = [np.asfortranarray(l, dtype=np.float64) for l in _factors]
            ldl = np.array([l.shape[0] for l in Ls], dtype=np.int64)
            _lib.check(L.pmk_model_load(self.ctx.h, self.D, P, _i(self.n), _dps(self.X, P), _dps(ys, P), _dps(Ls, P),
                                        _i(ldl), C.byref(h)), "pmk_model_load")
            self._has_factor, self._has_targets = True, False       # factors but no y and no theta: set_kernels
        self.h = h

    @classmethod
    def from_tree(cls, root, X, y=None, eps=None, ctx=None, dtype="f64", leaf_base=0, P=None, reserve=None):
        """pmk_model_create_from_bsp: the model of the tree `root` and ONE global point array X (N, D), numpy or a device
        array (a torch tensor), float64 and contiguous; y likewise, N targets, or None (zero until set_targets_global).
        eps=None: patch r is the tree's own leaf leaf_base + r; eps >= 0: its eps-set (organizetrainingsets).  The
        library assigns, gathers and packs on the GPU; the tree is attached.  The result equals
        DeviceModel(X_set, y_set) on the host-cut lists bit for bit.  reserve: rows for reserve(), straight after
        creation."""
        xa = GlobalArray(X, "X").points(getattr(root, "_D", None))
        N = xa.shape[0]
        ya = None if y is None else GlobalArray(y, "y").vector(N)
        if dtype not in ("f64", "f32"):
            raise ValueError("dtype must be 'f64' or 'f32'")
        if eps is not None and not float(eps) >= 0:
            raise ValueError("eps must be None (the tree's leaves) or >= 0")
        if N < 1:
            raise ValueError("no points")
        nat = _native(root)
        self = cls.__new__(cls)
        self.ctx = ctx or default_context()
        L = self.ctx.L
        h = C.c_void_p()
        _lib.check(L.pmk_model_create_from_bsp(self.ctx.h, nat.h, N, xa.ptr, None if ya is None else ya.ptr,
                                               -1.0 if eps is None else float(eps), int(leaf_base), int(P or 0),
                                               {"f64": 0, "f32": 1}[dtype], C.byref(h)), "pmk_model_create_from_bsp")
        self.h = h
        self.dtype, self.D, self.N = dtype, xa.shape[1], N
        self._from_tree, self._X_global = True, (None if xa.device else X)
        self.leaf_base = int(leaf_base)
        self._root, self._eps = root, (None if eps is None else float(eps))     # append_global assigns with them
        self.P = int(L.pmk_model_num_patches(h))
        self._all_leaves = self.leaf_base == 0 and self.P == int(L.pmk_bsp_num_leaves(nat.h))
        off, _ = self.patch_index()
        self.n = np.diff(off)
        if reserve is not None:
            self.reserve(reserve)
        return self

    @property
    def X(self):
        """the points of every patch; on a model built by from_tree they are cut from the index list on first use, and
        only if X was a host array (None otherwise: the points never came to the host)"""
        if self._X is None and self._X_global is not None:
            off, inds = self.patch_index()
            self._X = [self._X_global[inds[off[r]:off[r + 1]]] for r in range(self.P)]
        return self._X

    @X.setter
    def X(self, value):
        self._X = value

    def _need_tree_model(self, who):
        if not self._from_tree:
            raise _lib.PmkError("%s: the model was built from lists of patches, not by from_tree" % who)

    def patch_index(self):
        """pmk_model_patch_index -> (offsets [P+1], inds): row i of patch r is the global point inds[offsets[r] + i]"""
        self._need_tree_model("patch_index")
        if self._index is None:
            L = self.ctx.L
            off = np.empty(self.P + 1, dtype=np.int64)
            _lib.check(L.pmk_model_patch_index(self.h, None, _i(off), None), "pmk_model_patch_index")
            inds = np.empty(max(int(off[-1]), 1), dtype=np.int64)
            _lib.check(L.pmk_model_patch_index(self.h, None, None, _i(inds)), "pmk_model_patch_index")
            self._index = (off, inds[:int(off[-1])])
        return self._index

    def set_targets_global(self, y):
        """pmk_model_set_targets_global: the N targets of ALL points (numpy or device array) through the index list.
        With a device array this only enqueues on the context's stream."""
        self._need_tree_model("set_targets_global")
        ya = GlobalArray(y, "y").vector(self.N)
        _lib.check(self.ctx.L.pmk_model_set_targets_global(self.h, ya.ptr), "pmk_model_set_targets_global")
        self._targets_replaced()

    def set_targets_multi_global(self, Y):
        """pmk_model_set_targets_multi_global: Y is (N, R) column-major (Fortran order; its column stride is the leading
        dimension), or a vector for R = 1"""
        self._need_tree_model("set_targets_multi_global")
        ya = GlobalArray(Y, "Y")
        R, ld = ya.columns(self.N)
        _lib.check(self.ctx.L.pmk_model_set_targets_multi_global(self.h, R, ya.ptr, ld), "pmk_model_set_targets_multi_global")
        self.R = R
        self._multi_solved = False

    def set_diag_global(self, diag):
        """pmk_model_set_diag_global: N addends of the kernel's diagonal through the index list (None clears it)"""
        self._need_tree_model("set_diag_global")
        da = None if diag is None else GlobalArray(diag, "diag").vector(self.N)
        self._targets_replaced()
        _lib.check(self.ctx.L.pmk_model_set_diag_global(self.h, None if da is None else da.ptr), "pmk_model_set_diag_global")

    @classmethod
    def from_factors(cls, X_parts, c_set, L_set, ctx=None):
        """device model from host factors (c_set, L_set of a fitted MixtureGPType): checkpoint / resume"""
        return cls(X_parts, c_set, ctx, _factors=L_set)

    def queryinner(self, patch, theta, Xq):
        """queryinner! batched over Xq against one patch -> (mu, var)"""
        Xq = as_points(Xq)
        mu, var = np.empty(Xq.shape[0]), np.empty(Xq.shape[0])
        d = theta.desc()
        _lib.check(self.ctx.L.pmk_model_queryinner(self.h, int(patch), C.byref(d), Xq.shape[0], _d(Xq), _d(mu), _d(var)),
                   "pmk_model_queryinner")
        return mu, var

    def __del__(self):
        if getattr(self, "h", None):
            self.ctx.L.pmk_model_destroy(self.h)
            self.h = None

    def set_targets(self, y_parts):
        ys = [np.ascontiguousarray(y, dtype=np.float64) for y in y_parts]
        _lib.check(self.ctx.L.pmk_model_set_targets(self.h, _dps(ys, self.P)), "pmk_model_set_targets")
        self._targets_replaced()

    def set_diag(self, diag_parts):
        """pmk_model_set_diag: per-point addend of the kernel's diagonal for the next fits (None clears it)"""
        self._targets_replaced()
        if diag_parts is None:
            _lib.check(self.ctx.L.pmk_model_set_diag(self.h, None), "pmk_model_set_diag")
            return
        ds = [np.ascontiguousarray(d, dtype=np.float64) for d in diag_parts]
        for d, n in zip(ds, self.n):
            if len(d) != n:
                raise ValueError("one addend per point")
        _lib.check(self.ctx.L.pmk_model_set_diag(self.h, _dps(ds, self.P)), "pmk_model_set_diag")

    def fit(self, theta, sigma2):
        """enqueue kernel build + Cholesky + solves for every patch"""
        if self._from_tree:
            _refuse_closure_kernel(theta, "fit")
        d = theta.desc()
        _lib.check(self.ctx.L.pmk_model_fit(self.h, C.byref(d), float(sigma2)), "pmk_model_fit")
        self.theta, self.sigma2 = theta, float(sigma2)
        self._new_factor()

    def fit_patches(self, thetas, sigma2s):
        """pmk_model_fit_patches: the fit with one kernel and one noise variance PER PATCH (thetas[r], sigma2s[r] belong
        to patch r; families may differ).  Enqueues like fit()."""
        descs, s2 = patch_hyper(thetas, sigma2s, self.P)
        _lib.check(self.ctx.L.pmk_model_fit_patches(self.h, descs, _d(s2)), "pmk_model_fit_patches")
        self.theta, self.sigma2 = None, None
        self.thetas, self.sigma2s = list(thetas), [float(v) for v in s2]
        self._new_factor()

    def set_kernels(self, thetas):
        """pmk_model_set_kernels: the kernels of a model built by from_factors (which holds factors but no theta), for
        DeviceQuery.items_fitted / items_multi_fitted"""
        descs, _ = patch_hyper(thetas, None, self.P)
        _lib.check(self.ctx.L.pmk_model_set_kernels(self.h, descs), "pmk_model_set_kernels")
        self.thetas = list(thetas)
        self._has_kernels = True

    def hyper(self):
        """pmk_model_get_hyper -> (descs, sigma2 [P]): the hyperparameters the resident factor belongs to, descs[r] =
        (family, flags, (p0, p1, p2, p3)) of patch r.  After a plain fit() P copies of its theta and sigma2."""
        descs = (_lib.KernelDesc * self.P)()
        s2 = np.empty(self.P)
        _lib.check(self.ctx.L.pmk_model_get_hyper(self.h, descs, _d(s2)), "pmk_model_get_hyper")
        return [(int(d.family), int(d.flags), tuple(float(v) for v in d.p)) for d in descs], s2

    def info(self):
        info = np.zeros(self.P, dtype=np.int32)
        _lib.check(self.ctx.L.pmk_model_info(self.h, _i32(info)), "pmk_model_info")
        return info

    def weights(self):
        """c_set: the weights of every patch, one device-to-host transfer for the whole model"""
        out = [np.empty(int(n)) for n in self.n]
        _lib.check(self.ctx.L.pmk_model_get_weights(self.h, _dps(out, self.P)), "pmk_model_get_weights")
        return out

    def get(self, patch, what):
        n = int(self.n[patch])
        if what == GET_C:
            out = np.empty(n)
            ld = 0
        elif what == GET_LINV_DIAG:
            nt = (n + 127) // 128
            out = np.empty((4 * nt, 32, 32))
            ld = 0
        else:
            out = np.empty((n, n), order="F")
            ld = n
        _lib.check(self.ctx.L.pmk_model_get(self.h, patch, what, _d(out), ld), "pmk_model_get")
        if what == GET_LINV_DIAG:
            out = np.transpose(out, (0, 2, 1)).copy()      # column-major blocks -> [block][row][col]
        return out

    def set_targets_multi(self, Y_parts):
        """pmk_model_set_targets_multi: R target columns per patch (Y_parts[r] is n_r x R, or a vector for R = 1)"""
        Ys = multi_targets(Y_parts, self.n)
        R = Ys[0].shape[1]
        ldy = np.array([y.shape[0] for y in Ys], dtype=np.int64)
        _lib.check(self.ctx.L.pmk_model_set_targets_multi(self.h, R, _dps(Ys, self.P), _i(ldy)),
                   "pmk_model_set_targets_multi")
        self.R = R
        self._multi_solved = False

    def solve_multi(self):
        """pmk_model_solve_multi: C = (L L^T)^-1 Y for every column from the resident factor (no refactorisation)"""
        _lib.check(self.ctx.L.pmk_model_solve_multi(self.h), "pmk_model_solve_multi")
        self._multi_solved = True

    def weights_multi(self):
        """the n_r x R weights of every patch (one device-to-host transfer)"""
        R = self.R
        if R < 1:
            raise _lib.PmkError("set_targets_multi has not run on this model")
        out = [np.empty((int(n), R), order="F") for n in self.n]
        ldc = np.array([int(n) for n in self.n], dtype=np.int64)
        _lib.check(self.ctx.L.pmk_model_get_weights_multi(self.h, _dps(out, self.P), _i(ldc)),
                   "pmk_model_get_weights_multi")
        return out

    # ---- kriging with a trend: one GLS drift per patch on the multi-output path (include/pmk.h)
    def set_trend(self, trend):
        """pmk_model_set_trend: "none" / None (simple kriging), "constant" (ordinary kriging, h = [1]) or "linear" (universal
        kriging, h(x) = [1, x_1 .. x_D] in the raw coordinates).  Host state only: the multi-output weights become stale,
        run solve_multi again."""
        _lib.check(self.ctx.L.pmk_model_set_trend(self.h, trend_degree(trend)), "pmk_model_set_trend")
        self._multi_solved = False

    def trend(self):
        """pmk_model_get_trend -> (beta_set, G_set) of the last solve_multi: beta_set[r] is q x R (coefficients of
        [1, x_1 .. x_D] per target column), G_set[r] = H^T U^-1 H (q x q).  q = 0 without a trend."""
        self._need(multi=True)
        q = C.c_int(0)
        _lib.check(self.ctx.L.pmk_model_get_trend(self.h, C.byref(q), None, None), "pmk_model_get_trend")
        q = int(q.value)
        beta, G = np.zeros((self.P, self.R, q)), np.zeros((self.P, q, q))
        if q:
            _lib.check(self.ctx.L.pmk_model_get_trend(self.h, None, _d(beta), _d(G)), "pmk_model_get_trend")
        return [beta[r].T.copy() for r in range(self.P)], [G[r].T.copy() for r in range(self.P)]

    def trend_info(self):
        """pmk_model_trend_info -> int32 [P]: 0 ok; a in 1..q: pivot a of the Cholesky of G_r is <= 0 or NaN; n_r + 1: the
        patch has fewer points than basis functions"""
        self._need(multi=True)
        flags = np.zeros(self.P, dtype=np.int32)
        _lib.check(self.ctx.L.pmk_model_trend_info(self.h, _i32(flags)), "pmk_model_trend_info")
        return flags

    # ---- model selection from the resident factor (per patch: a point of several overlapping patches has a score in each)
    def _need(self, factor=True, loo=False, multi=False, targets=False):
        if factor and not self._has_factor:
            raise _lib.PmkError("no factor: fit the model (or build it with from_factors) first")
        if targets and not self._has_targets:
            raise _lib.PmkError("a model built from factors holds no targets: y^T c is not available")
        if multi and not self._multi_solved:
            raise _lib.PmkError("solve_multi has not run on the resident factor")
        if loo and not self._loo_done:
            raise _lib.PmkError("loo() has not run on the resident factor")

    def evidence(self, quad=True):
        """pmk_model_evidence -> (logdet [P], quad [P] or None): log det (K + sigma2 I) = 2 sum log L_ii and y^T c of
        every patch; NaN where the factorisation failed"""
        self._need(targets=quad)
        logdet, q = np.empty(self.P), (np.empty(self.P) if quad else None)
        _lib.check(self.ctx.L.pmk_model_evidence(self.h, _d(logdet), None if q is None else _d(q)), "pmk_model_evidence")
        return logdet, q

    def evidence_multi(self):
        """pmk_model_evidence_multi -> (logdet [P], quad [P, R]): quad[r, j] = Y_r[:, j]^T C_r[:, j]"""
        self._need(multi=True)
        logdet, q = np.empty(self.P), np.empty((self.P, self.R), order="F")
        _lib.check(self.ctx.L.pmk_model_evidence_multi(self.h, _d(logdet), _d(q)), "pmk_model_evidence_multi")
        return logdet, q

    def loo(self):
        """pmk_model_loo: d = diag((L L^T)^-1) of every patch from the resident factor (enqueues; no refit)"""
        self._need()
        _lib.check(self.ctx.L.pmk_model_loo(self.h), "pmk_model_loo")
        self._loo_done = True

    def loo_values(self):
        """pmk_model_get_loo -> (res, var), one vector per patch: res_i = c_i / d_i = y_i - mu_-i (the leave-one-out
        mean is y_i - res_i), var_i = 1 / d_i (includes sigma2)"""
        self._need(loo=True)
        res, var = [np.empty(int(n)) for n in self.n], [np.empty(int(n)) for n in self.n]
        _lib.check(self.ctx.L.pmk_model_get_loo(self.h, _dps(res, self.P), _dps(var, self.P)), "pmk_model_get_loo")
        return res, var

    def loo_values_multi(self):
        """pmk_model_get_loo_multi -> (RES, var): RES[r] is n_r x R (one residual column per target column), var is
        shared by the columns.  With a trend of q basis functions a patch of n_r <= q points returns NaN in both: leaving
        one point out leaves fewer points than basis functions"""
        self._need(loo=True, multi=True)
        RES = [np.empty((int(n), self.R), order="F") for n in self.n]
        var = [np.empty(int(n)) for n in self.n]
        ld = np.array([int(n) for n in self.n], dtype=np.int64)
        _lib.check(self.ctx.L.pmk_model_get_loo_multi(self.h, _dps(RES, self.P), _i(ld), _dps(var, self.P)),
                   "pmk_model_get_loo_multi")
        return RES, var

    def set_bsp(self, root, leaf_base=0):
        _lib.check(self.ctx.L.pmk_model_set_bsp(self.h, _native(root).h, int(leaf_base)), "pmk_model_set_bsp")
        self.leaf_base = int(leaf_base)

    # ---- appending observations to the resident factor in place: the border of the Cholesky factor (include/pmk.h)
    def capacity(self):
        """pmk_model_capacity -> int64 [P]: the points every patch can still take, ld_r - n_r; ld_r = 128 ceil(n_r / 128)
        until reserve() gives more"""
        free = np.empty(self.P, dtype=np.int64)
        _lib.check(self.ctx.L.pmk_model_capacity(self.h, _i(free)), "pmk_model_capacity")
        return free

    def reserve(self, rows):
        """pmk_model_reserve: afterwards capacity() >= rows, an int for every patch or one value per patch -> capacity().
        Patches that lack the room get a larger stride ld_r (the model moves into a new layout, the old one is freed); none
        is shrunk.  Works before and after a fit; a fitted model keeps its factor, weights and info bit for bit.  loo(), the
        multi-output targets and the trend state have to be set again; queries created earlier keep their plan."""
        rows = np.ascontiguousarray(np.broadcast_to(np.asarray(rows), (self.P,)) if np.ndim(rows) == 0 else rows)
        if rows.shape != (self.P,) or not np.issubdtype(rows.dtype, np.integer):
            raise ValueError("rows must be an int or %d ints, one per patch" % self.P)
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        _lib.check(self.ctx.L.pmk_model_reserve(self.h, _i(rows)), "pmk_model_reserve")
        self._rows_changed()
        return self.capacity()

    def _need_appendable(self, who):
        self._need()
        if not self._has_targets:
            raise _lib.PmkError("%s: a model built from factors holds no targets: z cannot be extended" % who)

    def _append(self, x, y, diag, patch, gidx):
        _lib.check(self.ctx.L.pmk_model_append(self.h, len(y), _d(x), _d(y), None if diag is None else _d(diag), _i32(patch),
                                               None if gidx is None else _i(gidx)), "pmk_model_append")
        self.n = self.n + np.bincount(patch, minlength=self.P).astype(np.int64)
        self._rows_changed()

    def append(self, X_new_parts, y_new_parts, diag_parts=None):
        """pmk_model_append: X_new_parts[r] (m_r x D, m_r = 0 allowed) become the rows n_r .. n_r + m_r - 1 of patch r, with
        targets y_new_parts[r] and, on a model with set_diag addends, diag_parts[r] (None: zeros) -> info.  L, z and c of the
        resident factor are extended in place (no refit); loo() and the multi-output targets have to be set again."""
        self._need_appendable("append")
        if self._from_tree:
            raise _lib.PmkError("append: a model built by from_tree takes append_global")
        x, y, diag, patch, parts = append_items(X_new_parts, y_new_parts, diag_parts, self.n, self.D, self.capacity())
        if len(y):
            self._append(x, y, diag, patch, None)
            self.X = [np.ascontiguousarray(np.vstack([a, b])) for a, b in zip(self.X, parts)]
        return self.info()

    def append_global(self, X_new, y_new):
        """pmk_model_append on a model built by from_tree: the points X_new (m x D) with targets y_new get the global
        indices N, N + 1, ... and go to the patches the tree assigns them at the eps of from_tree (pmk_bsp_assign; eps=None:
        the home leaf only) -> (first_global_index, n_items).  A point of several eps-sets is one item in each.  The tree's
        own leaf lists are not updated."""
        self._need_tree_model("append_global")
        self._need_appendable("append_global")
        if not self._all_leaves:
            raise _lib.PmkError("append_global: the model holds a shard of the tree's leaves")
        Xn = as_points(X_new)
        yn = np.ascontiguousarray(y_new, dtype=np.float64).reshape(-1)
        if Xn.shape[1] != self.D:
            raise ValueError("X_new must have shape (m, %d), not %s" % (self.D, Xn.shape))
        if len(yn) != Xn.shape[0]:
            raise ValueError("one target per new point: %d targets for %d points" % (len(yn), Xn.shape[0]))
        if not (np.all(np.isfinite(Xn)) and np.all(np.isfinite(yn))):
            raise ValueError("non-finite coordinate or target")
        first, m = int(self.N), Xn.shape[0]
        if m == 0:
            return first, 0
        L, h = self.ctx.L, _native(self._root).h
        if self._eps is None:
            point = np.arange(m, dtype=np.int64)
            patch = np.array([findpartition(Xn[i], self._root) for i in range(m)], dtype=np.int64)     # raises on an error code
        else:
            off = np.empty(self.P + 1, dtype=np.int64)
            _lib.check(L.pmk_bsp_assign(h, m, _d(Xn), self._eps, _i(off), None, None, None), "pmk_bsp_assign")
            inds, loff = np.empty(max(int(off[-1]), 1), dtype=np.int64), np.empty(m + 1, dtype=np.int64)
            lists = np.empty(max(int(off[-1]), 1), dtype=np.int64)
            _lib.check(L.pmk_bsp_assign(h, m, _d(Xn), self._eps, _i(off), _i(inds), _i(loff), _i(lists)), "pmk_bsp_assign")
            point = np.repeat(np.arange(m, dtype=np.int64), np.diff(loff))     # point-major: ascending within a patch
            patch = lists[:int(loff[-1])].copy()
        check_append_counts(np.bincount(patch, minlength=self.P), self.n, self.capacity())
        self._append(np.ascontiguousarray(Xn[point]), np.ascontiguousarray(yn[point]), None, patch.astype(np.int32),
                     np.ascontiguousarray(first + point))
        self.N = first + m
        self._index = self._X = None        # read back / cut again on first use
        if self._X_global is not None:
            self._X_global = np.ascontiguousarray(np.vstack([self._X_global, Xn]))
        return first, len(point)

    # ---- removing observations from the resident factor in place: row deletion from the Cholesky factor (include/pmk.h)
    def removable(self):
        """pmk_model_removable -> int64 [P]: the rows every patch can still lose, n_r - 128 (ceil(n_r / 128) - 1) - 1 (a
        patch stays in its last block row)"""
        rows = np.empty(self.P, dtype=np.int64)
        _lib.check(self.ctx.L.pmk_model_removable(self.h, _i(rows)), "pmk_model_removable")
        return rows

    def _remove(self, patch, row):
        _lib.check(self.ctx.L.pmk_model_remove(self.h, len(row), _i32(patch), _i(row)), "pmk_model_remove")
        self.n = self.n - np.bincount(patch, minlength=self.P).astype(np.int64)
        self._rows_changed()

    def remove(self, rows_parts):
        """pmk_model_remove: rows_parts[r] is an integer array (empty allowed) of ZERO-based row indices of patch r as it
        stands before the call -> info.  L, z and c of the resident factor are reduced in place (no refit), the rows that
        stay keep their order; loo() and the multi-output targets have to be set again."""
        self._need_appendable("remove")
        if self._from_tree:
            raise _lib.PmkError("remove: a model built by from_tree takes remove_global")
        patch, row, parts = remove_items(rows_parts, self.n)
        if len(row):
            self._remove(patch, row)
            self.X = [np.ascontiguousarray(np.delete(x, p, axis=0)) for x, p in zip(self.X, parts)]
        return self.info()

    def remove_global(self, indices):
        """pmk_model_remove on a model built by from_tree: the global points `indices` (zero-based) leave every patch that
        holds them (patch_index()) -> n_items, the rows removed.  N does not change and the *_global setters still take N
        values; a point no patch holds is a ValueError.  The tree's own leaf lists are not updated."""
        self._need_tree_model("remove_global")
        self._need_appendable("remove_global")
        g = np.ascontiguousarray(indices, dtype=np.int64).reshape(-1)
        if len(np.unique(g)) != len(g):
            raise ValueError("remove_global: a global index is given twice")
        if len(g) and (g.min() < 0 or g.max() >= self.N):
            raise ValueError("remove_global: a global index outside 0 .. %d" % (self.N - 1))
        if len(g) == 0:
            return 0
        off, inds = self.patch_index()
        at = np.nonzero(np.isin(inds, g))[0]
        missing = np.setdiff1d(g, inds[at])
        if len(missing):
            raise ValueError("remove_global: no patch holds the global point %d" % int(missing[0]))
        patch = (np.searchsorted(off, at, side="right") - 1).astype(np.int32)
        row = np.ascontiguousarray(at - off[patch])
        check_remove_counts(np.bincount(patch, minlength=self.P), self.n)
        self._remove(patch, row)
        keep = np.ones(len(inds), dtype=bool)
        keep[at] = False
        self._index = (np.concatenate([[0], np.cumsum(self.n)]).astype(np.int64), inds[keep])
        self._X = None                      # cut again on first use
        return len(row)


class DeviceQuery:
    """pmk_query: a resident batch of query points and its (query, region) work items"""

    # The mirror of the library's query state (include/pmk.h): what a fetch has to allocate, and what is refused
    # before any device call.  These are the values of a query just created from points; every birth path (the
    # constructor, from_items, a test's object.__new__) sets only what differs, and only the calls named here change them.
    Xq = None               # the host copy of the points; None for a device array and after from_items
    has_diag = False        # set_diag / set_diag_device addends of k(xq, xq) are set
    total = 0               # the items of the plan: plan, predict_sharded, predict_allgather; from_items: its n
    first_owned = 0         # plan: the items of this rank's own leaves are [first_owned, first_owned + num_owned)
    num_owned = 0
    R_items = 0             # the columns of the last items_multi / _multi_fitted / _loo_multi; 0 after a new plan
    variance = False        # ... and whether they ran with the variance
    grad_items = False      # items_grad ran on these items
    vgrad_items = False     # items_vgrad ran on these items
    block_F = 0             # the groups of the last items_block
    block_variance = False  # ... and whether it ran with the variance

    def _items_replaced(self, R, variance):
        """plan (R = 0), items_multi, items_multi_fitted, items_loo_multi: the multi-output items are those of R columns,
        with or without the variance, and the gradients of the earlier ones are gone, as in the library"""
        self.variance, self.R_items = bool(variance), int(R)
        self.grad_items = self.vgrad_items = False

    def __init__(self, model, Xq):
        self.model = model
        if isinstance(Xq, np.ndarray) or not hasattr(Xq, "__cuda_array_interface__"):
            self.Xq = as_points(Xq)
            ptr = _d(self.Xq)
            self.Nq = self.Xq.shape[0]
        else:                                   # a device array (torch tensor): no host copy
            xa = GlobalArray(Xq, "Xq").points(model.D)
            self._keep = Xq
            ptr = C.cast(C.c_void_p(xa.ptr), _dp)
            self.Nq = xa.shape[0]
        h = C.c_void_p()
        _lib.check(model.ctx.L.pmk_query_create(model.h, self.Nq, ptr, C.byref(h)), "pmk_query_create")
        self.h = h
        self.L = model.ctx.L

    def set_diag(self, diag):
        """pmk_query_set_diag: per-query addend of k(xq, xq) in the predictive variance (None clears it)"""
        if diag is None:
            _lib.check(self.L.pmk_query_set_diag(self.h, None), "pmk_query_set_diag")
            self.has_diag = False
            return
        d = np.ascontiguousarray(diag, dtype=np.float64)
        if len(d) != self.Nq:
            raise ValueError("one addend per query point")
        _lib.check(self.L.pmk_query_set_diag(self.h, _d(d)), "pmk_query_set_diag")
        self.has_diag = True

    def set_diag_device(self, diag_dev_ptr):
        """pmk_query_set_diag from a device array of Nq float64 (the addends received with a batch of requests)"""
        _lib.check(self.L.pmk_query_set_diag(self.h, C.cast(C.c_void_p(diag_dev_ptr), _dp)), "pmk_query_set_diag")
        self.has_diag = True

    def export_request_diag(self, first, n, diag_dev_ptr):
        """addends of k(xq, xq) of the sorted items [first, first + n) into a caller-owned device array (zeros when the
        query has none); True if the query carries addends"""
        return _lib.check(self.L.pmk_query_export_request_diag(self.h, int(first), int(n), diag_dev_ptr),
                          "pmk_query_export_request_diag") == 1

    @classmethod
    def from_items(cls, model, n, xq_ptr, region_ptr):
        """pmk_query_create_items: n explicit (point, region) items received from other ranks; xq_ptr / region_ptr
        are raw host or device addresses (float64 n x D point-major, int32 n)"""
        self = cls.__new__(cls)
        self.model, self.Nq, self.L = model, int(n), model.ctx.L
        h = C.c_void_p()
        _lib.check(self.L.pmk_query_create_items(model.h, int(n), xq_ptr, region_ptr, C.byref(h)), "pmk_query_create_items")
        self.h = h
        self.total = self.num_owned = int(n)
        return self

    def __del__(self):
        if getattr(self, "h", None):
            self.L.pmk_query_destroy(self.h)
            self.h = None

    def export_requests(self, first, n, xq_dev_ptr, region_dev_ptr):
        """(point, region) of the sorted items [first, first + n) into caller-owned device arrays"""
        _lib.check(self.L.pmk_query_export_requests(self.h, int(first), int(n), xq_dev_ptr, region_dev_ptr),
                   "pmk_query_export_requests")

    def export_results(self, u_dev_ptr, v_dev_ptr):
        """(u, v) in item order into caller-owned device arrays of length `total`"""
        _lib.check(self.L.pmk_query_export_results(self.h, u_dev_ptr, v_dev_ptr), "pmk_query_export_results")

    def plan(self, radius, delta):
        _lib.check(self.L.pmk_query_plan(self.h, float(radius), float(delta)), "pmk_query_plan")
        t, f, o = C.c_int64(), C.c_int64(), C.c_int64()
        _lib.check(self.L.pmk_query_counts(self.h, C.byref(t), C.byref(f), C.byref(o)))
        self.total, self.first_owned, self.num_owned = t.value, f.value, o.value
        self._items_replaced(0, self.variance)      # a new plan discards the items; the variance flag stays as it was
        return self.total

    def region_offsets(self, P_global):
        off = np.empty(P_global + 1, dtype=np.int64)
        _lib.check(self.L.pmk_query_region_offsets(self.h, _i(off)))
        return off

    def items(self, theta):
        d = theta.desc()
        _lib.check(self.L.pmk_query_items(self.h, C.byref(d)), "pmk_query_items")

    def _range(self, q0, q1):
        """the queries [q0, q1) of a mix call; q1=None: to the last"""
        return int(q0), int(self.Nq if q1 is None else q1)

    def items_fitted(self):
        """pmk_query_items_fitted: stage 2 with the model's own kernels (region r with the theta it was fitted with)"""
        _need_kernels(self.model)
        _lib.check(self.L.pmk_query_items_fitted(self.h), "pmk_query_items_fitted")

    def _blend_loo_model(self, who):
        """the model, if the blended leave-one-out can run on it with this query (the states the library refuses too)"""
        m = self.model
        if not m._from_tree:
            raise _lib.PmkError("%s: the model was built from lists of patches, not by from_tree" % who)
        if self.Nq != m.N:
            raise _lib.PmkError("%s: the query has %d points, the model %d: query j must be training point j"
                                % (who, self.Nq, m.N))
        if not m._all_leaves:
            raise _lib.PmkError("%s: the model holds a shard of the leaves; the blended leave-one-out needs all" % who)
        if not m._has_kernels:
            raise _lib.PmkError("the model holds no kernels: fit it first")
        return m

    def items_loo(self, noisy=False):
        """pmk_query_items_loo: stage 2 of the blended leave-one-out, for a query whose points ARE the training points of a
        tree-built model (query j = global point j) -> (n_member, n_strip).  An item whose patch holds the point comes
        from the resident leave-one-out values (no strip); any other item is items_fitted's.  noisy: the variances include
        each patch's sigma2.  Follow with mix() and fetch() as after items()."""
        m = self._blend_loo_model("items_loo")
        m._need(loo=True)
        nm, ns = C.c_int64(), C.c_int64()
        _lib.check(self.L.pmk_query_items_loo(self.h, int(bool(noisy)), C.byref(nm), C.byref(ns)), "pmk_query_items_loo")
        return nm.value, ns.value

    def items_loo_multi(self, noisy=False, variance=True):
        """pmk_query_items_loo_multi: items_loo for the R target columns of the multi-output path, with the model's trend
        if it has one -> (n_member, n_other).  A member item is mu_c = Y[i, c] - C[i, c] / Q_ii with variance 1 / Q_ii
        (- sigma2_r), Q the trend-aware diagonal of loo_values_multi(); any other item is items_multi_fitted's.
        With a trend of q basis functions a member item of a patch of n <= q points is NaN (means and variance): no
        leave-one-out prediction exists from fewer than q points; a non-member item of such a patch stays valid.
        variance=False: means only, no strip kernel runs.  Follow with mix_multi() and fetch_multi()."""
        m = self._blend_loo_model("items_loo_multi")
        m._need(loo=True)           # the library's order: a new fit makes both stale and is told about loo() first
        m._need(multi=True)
        nm, no = C.c_int64(), C.c_int64()
        _lib.check(self.L.pmk_query_items_loo_multi(self.h, int(bool(noisy)), int(bool(variance)), C.byref(nm), C.byref(no)),
                   "pmk_query_items_loo_multi")
        self._items_replaced(m.R, variance)
        return nm.value, no.value

    def item_values_multi(self):
        """pmk_query_get_items_multi -> (U [total, R], v [total] or None after a mean-only run): the per-item results of
        items_multi, items_multi_fitted or items_loo_multi in the item order of debug()"""
        R = self.R_items                        # the R of the items run: the library writes that many columns
        if R < 1:
            raise _lib.PmkError("item_values_multi: no items_multi, items_multi_fitted or items_loo_multi has run")
        T = max(int(self.total), 1)
        U = np.empty((T, R))
        v = np.empty(T) if self.variance else None
        _lib.check(self.L.pmk_query_get_items_multi(self.h, _d(U), R, None if v is None else _d(v)),
                   "pmk_query_get_items_multi")
        return U[:self.total], (None if v is None else v[:self.total])

    def items_multi_fitted(self, variance=True):
        """pmk_query_items_multi_fitted: items_multi with the model's own kernels"""
        _need_kernels(self.model)
        _lib.check(self.L.pmk_query_items_multi_fitted(self.h, int(bool(variance))), "pmk_query_items_multi_fitted")
        self._items_replaced(self.model.R, variance)

    def item_buffers(self):
        u, v = C.c_void_p(), C.c_void_p()
        _lib.check(self.L.pmk_query_item_buffers(self.h, C.byref(u), C.byref(v)))
        return u.value, v.value

    def predict_sharded(self, comm, theta, weight_theta, radius, delta):
        """pmk_query_predict_sharded: one predict step of a model sharded over `comm` (collective; RCCL inside the
        library, everything on the context's stream).  Returns this rank's item count."""
        d, w = theta.desc(), weight_theta.desc()
        t = C.c_int64()
        _lib.check(self.L.pmk_query_predict_sharded(self.h, comm.h, C.byref(d), C.byref(w), float(radius), float(delta),
                                                    C.byref(t)), "pmk_query_predict_sharded")
        self.total = t.value
        return t.value

    def predict_allgather(self, comm, theta, weight_theta, radius, delta):
        """pmk_query_predict_allgather: the same step with REPLICATED queries (this object holds all of them): every
        rank plans all queries, evaluates the items of its own leaves, one RCCL all-gather of padded (u, v) slices, every
        rank blends all queries (collective).  Returns the item count of the whole job."""
        d, w = theta.desc(), weight_theta.desc()
        t = C.c_int64()
        _lib.check(self.L.pmk_query_predict_allgather(self.h, comm.h, C.byref(d), C.byref(w), float(radius), float(delta),
                                                      C.byref(t)), "pmk_query_predict_allgather")
        self.total = t.value
        return t.value

    def mix(self, weight_theta, q0=0, q1=None):
        d = weight_theta.desc()
        _lib.check(self.L.pmk_query_mix(self.h, C.byref(d), *self._range(q0, q1)), "pmk_query_mix")

    def fetch(self):
        Yq, Vq = np.empty(self.Nq), np.empty(self.Nq)
        _lib.check(self.L.pmk_query_fetch(self.h, _d(Yq), _d(Vq)), "pmk_query_fetch")
        return Yq, Vq

    @staticmethod
    def _device_out(a, what):
        ga = GlobalArray(a, what)
        if not ga.device:
            raise ValueError("%s must be a device array (__cuda_array_interface__); fetch() returns host arrays" % what)
        return ga

    @classmethod
    def _device_out_c(cls, a, what, shape):
        """a C-contiguous device array of exactly `shape` (its last extent is Nq: nothing to check on an empty batch)"""
        ga = cls._device_out(a, what)
        strides = tuple(int(np.prod(shape[k + 1:], dtype=np.int64)) for k in range(len(shape)))
        if ga.shape != shape or (shape[-1] > 0 and ga.strides != strides):
            raise ValueError("%s must be a C-contiguous device array of shape (%s), not %s"
                             % (what, ", ".join("%d" % v for v in shape), ga.shape))
        return ga

    def fetch_into(self, Yq, Vq=None):
        """pmk_query_fetch_dev: the mixed results into device arrays of Nq float64 (torch tensors): device-to-device on
        the context's stream, no host synchronisation"""
        ya = self._device_out(Yq, "Yq").vector(self.Nq)
        va = None if Vq is None else self._device_out(Vq, "Vq").vector(self.Nq)
        _lib.check(self.L.pmk_query_fetch_dev(self.h, ya.ptr, None if va is None else va.ptr), "pmk_query_fetch_dev")

    def fetch_multi_into(self, Yq, Vq=None):
        """pmk_query_fetch_multi_dev: Yq is a device array (Nq, R) in column-major order (its column stride is the leading
        dimension); Vq (Nq) only if the items ran with the variance"""
        R = self.model.R
        ya = self._device_out(Yq, "Yq")
        if len(ya.shape) != 2 or ya.shape[1] != R:
            raise ValueError("Yq must have shape (%d, %d), not %s" % (self.Nq, R, ya.shape))
        _, ld = ya.columns(self.Nq)
        if Vq is not None and not self.variance:
            raise ValueError("Vq was not computed: the items ran mean-only (variance=False)")
        va = None if Vq is None else self._device_out(Vq, "Vq").vector(self.Nq)
        _lib.check(self.L.pmk_query_fetch_multi_dev(self.h, ya.ptr, ld, None if va is None else va.ptr),
                   "pmk_query_fetch_multi_dev")

    def items_multi(self, theta, variance=True):
        d = theta.desc()
        _lib.check(self.L.pmk_query_items_multi(self.h, C.byref(d), int(bool(variance))), "pmk_query_items_multi")
        self._items_replaced(self.model.R, variance)

    def mix_multi(self, weight_theta, q0=0, q1=None):
        d = weight_theta.desc()
        _lib.check(self.L.pmk_query_mix_multi(self.h, C.byref(d), *self._range(q0, q1)), "pmk_query_mix_multi")

    def fetch_multi(self, R):
        """(Yq [Nq, R], Vq or None)"""
        Yq = np.empty((self.Nq, R), order="F")
        Vq = np.empty(self.Nq) if self.variance else None
        _lib.check(self.L.pmk_query_fetch_multi(self.h, _d(Yq), max(self.Nq, 1), None if Vq is None else _d(Vq)),
                   "pmk_query_fetch_multi")
        return Yq, Vq

    # ---- gradient of the blended mean (pmk_grad.hip)
    def items_grad(self, theta=None):
        """pmk_query_items_grad: the gradient of every item mean of the last items_multi / items_multi_fitted on this plan,
        with `theta` for every patch or (None) the model's own kernels.  Closure-carrying kernels raise TypeError and
        Brownian-bridge kernels ValueError before any device call."""
        ptr, _keep = _theta_arg(self.model, theta, _grad_kernel, "items_grad")
        _lib.check(self.L.pmk_query_items_grad(self.h, ptr), "pmk_query_items_grad")
        self.grad_items = True

    def mix_grad(self, weight_theta, q0=0, q1=None):
        """pmk_query_mix_grad: the gradient of the blend of mix_multi for queries [q0, q1), the item list held fixed"""
        d = _grad_kernel(weight_theta, "mix_grad")
        _lib.check(self.L.pmk_query_mix_grad(self.h, C.byref(d), *self._range(q0, q1)), "pmk_query_mix_grad")

    def fetch_grad(self):
        """dYq [Nq, R, D]: dYq[j, c, d] = dY_c/dx_d at query j"""
        R, D = int(self.R_items), int(self.model.D)
        if R < 1:
            raise _lib.PmkError("fetch_grad: no items_multi or items_multi_fitted has run")
        buf = np.empty((R, D, max(self.Nq, 1)))                 # dYq[j + lddy (d + D c)]
        _lib.check(self.L.pmk_query_fetch_grad(self.h, _d(buf), max(self.Nq, 1)), "pmk_query_fetch_grad")
        return np.ascontiguousarray(buf[:, :, :self.Nq].transpose(2, 0, 1))

    def fetch_grad_into(self, dYq):
        """pmk_query_fetch_grad_dev: dYq is a device array of shape (R, D, Nq), C-contiguous (element [c, d, j] is
        dY_c/dx_d at query j): device-to-device on the context's stream, no host synchronisation"""
        ga = self._device_out_c(dYq, "dYq", (int(self.R_items), int(self.model.D), self.Nq))
        _lib.check(self.L.pmk_query_fetch_grad_dev(self.h, ga.ptr, max(self.Nq, 1)), "pmk_query_fetch_grad_dev")

    def item_grads(self):
        """pmk_query_get_items_grad -> (G [total, R, D], plane [total]) in the item order of debug(): G[i, c, d] is the
        gradient of item i's mean of column c; plane[i] is the pre-order hyperplane (row of fetchhyperplanes' arrays) a
        neighbour item was accepted at, -1 for a home item.  G is None before items_grad."""
        R, D = int(self.R_items), int(self.model.D)
        T = max(int(self.total), 1)
        plane = np.empty(T, dtype=np.int32)
        G = np.empty((T, R, D)) if self.grad_items and R >= 1 else None
        _lib.check(self.L.pmk_query_get_items_grad(self.h, None if G is None else _d(G), R * D, _i32(plane)),
                   "pmk_query_get_items_grad")
        return (None if G is None else G[:self.total]), plane[:self.total]

    # ---- gradient of the blended variance (pmk_vgrad.hip)
    def items_vgrad(self, theta=None):
        """pmk_query_items_vgrad: the gradient of every item variance of the last items_multi / items_multi_fitted on this
        plan, which must have run with the variance; `theta` for every patch or (None) the model's own kernels.  A query
        with set_diag addends is refused.  Closure-carrying kernels raise TypeError and Brownian-bridge kernels ValueError
        before any device call."""
        ptr, _keep = _theta_arg(self.model, theta, _grad_kernel, "items_vgrad")
        _lib.check(self.L.pmk_query_items_vgrad(self.h, ptr), "pmk_query_items_vgrad")
        self.vgrad_items = True

    def mix_vgrad(self, weight_theta, q0=0, q1=None):
        """pmk_query_mix_vgrad: the gradient of the blended variance of mix_multi for queries [q0, q1), the item list held
        fixed"""
        d = _grad_kernel(weight_theta, "mix_vgrad")
        _lib.check(self.L.pmk_query_mix_vgrad(self.h, C.byref(d), *self._range(q0, q1)), "pmk_query_mix_vgrad")

    def fetch_vgrad(self):
        """dVq [Nq, D]: dVq[j, d] = dVq/dx_d at query j"""
        D = int(self.model.D)
        buf = np.empty((D, max(self.Nq, 1)))                    # dVq[j + lddv d]
        _lib.check(self.L.pmk_query_fetch_vgrad(self.h, _d(buf), max(self.Nq, 1)), "pmk_query_fetch_vgrad")
        return np.ascontiguousarray(buf[:, :self.Nq].T)

    def fetch_vgrad_into(self, dVq):
        """pmk_query_fetch_vgrad_dev: dVq is a device array of shape (D, Nq), C-contiguous (element [d, j] is dVq/dx_d at
        query j): device-to-device on the context's stream, no host synchronisation"""
        ga = self._device_out_c(dVq, "dVq", (int(self.model.D), self.Nq))
        _lib.check(self.L.pmk_query_fetch_vgrad_dev(self.h, ga.ptr, max(self.Nq, 1)), "pmk_query_fetch_vgrad_dev")

    def item_vgrads(self):
        """pmk_query_get_items_vgrad -> GV [total, D] in the item order of debug(): GV[i, d] is the gradient of item i's
        variance"""
        if not self.vgrad_items:
            raise _lib.PmkError("item_vgrads: items_vgrad has not run on this plan")
        D = int(self.model.D)
        GV = np.empty((max(int(self.total), 1), D))
        _lib.check(self.L.pmk_query_get_items_vgrad(self.h, _d(GV), D), "pmk_query_get_items_vgrad")
        return GV[:self.total]

    # ---- joint covariance of the batch (pmk_cov.hip)
    def items_cov(self, theta=None):
        """pmk_query_items_cov: the posterior covariance block of every region over its items of this plan, with `theta`
        for every patch or (None) the model's own kernels.  Single-output path: no trend, no targets needed.  Serves a
        query made by from_items too.  Closure-carrying kernels raise TypeError before any device call."""
        ptr, _keep = _theta_arg(self.model, theta, _closure_free_kernel, "items_cov")
        _lib.check(self.L.pmk_query_items_cov(self.h, ptr), "pmk_query_items_cov")

    def items_cov_multi(self, theta=None):
        """pmk_query_items_cov_multi: items_cov on the multi-output path, after items_multi / items_multi_fitted on this
        plan.  Under the model's trend the blocks carry its term z_a . z_b (the universal-kriging covariance, whose diagonal
        is the item variance of items_multi); without one they are those of items_cov bit for bit.  `theta` is the kernel
        given to the items call, or (None) the model's own.  mix_cov, fetch_cov and item_covs serve the results.
        Closure-carrying kernels raise TypeError before any device call."""
        ptr, _keep = _theta_arg(self.model, theta, _closure_free_kernel, "items_cov_multi")
        _lib.check(self.L.pmk_query_items_cov_multi(self.h, ptr), "pmk_query_items_cov_multi")

    def mix_cov(self, weight_theta):
        """pmk_query_mix_cov: the joint covariance of the whole batch under the blend of mix()"""
        d = _closure_free_kernel(weight_theta, "mix_cov")
        _lib.check(self.L.pmk_query_mix_cov(self.h, C.byref(d)), "pmk_query_mix_cov")

    def fetch_cov(self):
        """Cov [Nq, Nq], symmetric: Cov[j, k] is the posterior covariance of the blended field at queries j and k"""
        n = max(self.Nq, 1)
        buf = np.empty((n, n))                      # Cov[j + ldc k]; symmetric, so the order does not matter
        _lib.check(self.L.pmk_query_fetch_cov(self.h, _d(buf), n), "pmk_query_fetch_cov")
        return buf[:self.Nq, :self.Nq]

    def fetch_cov_into(self, Cov):
        """pmk_query_fetch_cov_dev: Cov is a contiguous device array of shape (Nq, Nq) of float64 (a torch tensor):
        device-to-device on the context's stream, no host synchronisation"""
        ga = self._device_out_c(Cov, "Cov", (self.Nq, self.Nq))
        _lib.check(self.L.pmk_query_fetch_cov_dev(self.h, ga.ptr, max(self.Nq, 1)), "pmk_query_fetch_cov_dev")

    def item_covs(self, region):
        """pmk_query_get_items_cov -> (query_idx [m], S [m, m]): the block of one global region; row a belongs to query
        query_idx[a] (ascending)"""
        m = C.c_int64()
        _lib.check(self.L.pmk_query_get_items_cov(self.h, int(region), C.byref(m), None, None, 0), "pmk_query_get_items_cov")
        n = max(m.value, 1)
        idx = np.empty(n, dtype=np.int32)
        S = np.empty((n, n))
        _lib.check(self.L.pmk_query_get_items_cov(self.h, int(region), None, _i32(idx), _d(S), n), "pmk_query_get_items_cov")
        return idx[:m.value], S[:m.value, :m.value]

    # ---- block kriging: weighted sums over groups of queries (pmk_block.hip)
    def items_block(self, group, a, weight_theta, F=None, theta=None, variance=True):
        """pmk_query_items_block: mean and kriging variance of sum_j a[j] f(x_j) over the queries j of every group, after
        items_multi / items_multi_fitted on this plan.  group: int32 per query in [0, F), non-decreasing (the queries of a
        group are contiguous, a group may be empty); a: one coefficient per query; F: the number of groups (default: the
        last group + 1); theta: the kernel given to the items call, or (None) the model's own.  variance=False runs the
        weights and the mean reduction only.  Closure-carrying kernels raise TypeError before any device call."""
        _refuse_closure_kernel(weight_theta, "items_block")
        g = np.ascontiguousarray(group, dtype=np.int32).reshape(-1)
        c = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
        if len(g) != self.Nq or len(c) != self.Nq:
            raise ValueError("one group and one coefficient per query point (%d), not %d and %d" % (self.Nq, len(g), len(c)))
        if F is None:
            F = int(g[-1]) + 1 if len(g) else 0
        ptr, _keep = _theta_arg(self.model, theta, _closure_free_kernel, "items_block")
        w = weight_theta.desc()
        _lib.check(self.L.pmk_query_items_block(self.h, ptr, C.byref(w), int(F), _i32(g), _d(c), int(bool(variance))),
                   "pmk_query_items_block")
        self.block_F, self.block_variance = int(F), bool(variance)

    def fetch_block(self):
        """(Yb [F, R], Vb [F] or None after variance=False)"""
        F, R = self.block_F, int(self.R_items)
        Vb = np.empty(F) if self.block_variance else None
        buf = np.empty((max(F, 1), max(R, 1)), order="F")
        _lib.check(self.L.pmk_query_fetch_block(self.h, _d(buf), max(F, 1), None if Vb is None else _d(Vb)),
                   "pmk_query_fetch_block")
        return np.asfortranarray(buf[:F, :R]), Vb

    def fetch_block_into(self, Yb, Vb=None):
        """pmk_query_fetch_block_dev: Yb is a device array (F, R) in column-major order (its column stride is the leading
        dimension); Vb (F) only if items_block ran with the variance"""
        F, R = self.block_F, int(self.R_items)
        ya = self._device_out(Yb, "Yb")
        if len(ya.shape) != 2 or ya.shape != (F, R):
            raise ValueError("Yb must have shape (%d, %d), not %s" % (F, R, ya.shape))
        _, ld = ya.columns(F)
        if Vb is not None and not self.block_variance:
            raise ValueError("Vb was not computed: items_block ran mean-only (variance=False)")
        va = None if Vb is None else self._device_out(Vb, "Vb").vector(F)
        _lib.check(self.L.pmk_query_fetch_block_dev(self.h, ya.ptr, ld, None if va is None else va.ptr),
                   "pmk_query_fetch_block_dev")

    def item_blocks(self):
        """pmk_query_get_items_block -> dict of arrays, one entry per (region, group) aggregate in sorted-item order:
        region, group, first (sorted item), count, kappa, vnorm2 (|Vbar|^2), znorm2 (|zbar|^2), sw2 (sum w^2)"""
        n = C.c_int64()
        _lib.check(self.L.pmk_query_get_items_block(self.h, C.byref(n), None, None, None, None, None, None, None, None),
                   "pmk_query_get_items_block")
        k = max(n.value, 1)
        i32 = lambda: np.empty(k, dtype=np.int32)
        out = dict(region=i32(), group=i32(), first=np.empty(k, dtype=np.int64), count=i32(), kappa=np.empty(k),
                   vnorm2=np.empty(k), znorm2=np.empty(k), sw2=np.empty(k))
        _lib.check(self.L.pmk_query_get_items_block(self.h, None, _i32(out["region"]), _i32(out["group"]), _i(out["first"]),
                                                    _i32(out["count"]), _d(out["kappa"]), _d(out["vnorm2"]),
                                                    _d(out["znorm2"]), _d(out["sw2"])), "pmk_query_get_items_block")
        return {key: v[:n.value] for key, v in out.items()}

    # ---- posterior draws from the region blocks (pmk_draw.hip)
    def items_cov_blocks(self, theta=None, multi=False):
        """pmk_query_items_cov_blocks: the region blocks of items_cov (multi=False) or items_cov_multi (multi=True) for a
        batch of any size: what factor_cov and draw need.  mix_cov refuses such blocks on more than 16384 queries."""
        ptr, _keep = _theta_arg(self.model, theta, _closure_free_kernel, "items_cov_blocks")
        _lib.check(self.L.pmk_query_items_cov_blocks(self.h, ptr, 1 if multi else 0), "pmk_query_items_cov_blocks")

    def factor_cov(self, rel=None):
        """pmk_query_factor_cov: the Cholesky factor of every region block, block r as S_r + rel[r] (trace S_r / m_r) I
        (rel: P values, None for zeros).  Enqueues; a region already factored with the same rel[r] keeps its factor."""
        if rel is None:
            ptr = None
        else:
            rel = np.ascontiguousarray(rel, dtype=np.float64)
            if rel.shape != (int(self.model.P),):
                raise ValueError("rel must hold one value per patch (%d), not %s" % (self.model.P, rel.shape))
            ptr = _d(rel)
        _lib.check(self.L.pmk_query_factor_cov(self.h, ptr), "pmk_query_factor_cov")

    def factor_info(self):
        """pmk_query_factor_info -> (finfo [P] int32, jitter [P]): 0 factored or empty, k > 0 pivot k is <= 0 or NaN, -1 the
        patch is failed or its trend flagged; the absolute jitter that was added.  Blocks."""
        P = int(self.model.P)
        finfo, jitter = np.zeros(P, dtype=np.int32), np.zeros(P)
        rc = self.L.pmk_query_factor_info(self.h, _i32(finfo), _d(jitter))
        if rc < 0:
            _lib.check(rc, "pmk_query_factor_info")
        return finfo, jitter

    def item_cov_factor(self, region):
        """pmk_query_get_items_cov_factor -> L [m, m], lower triangular, of one global region; rows as in item_covs"""
        m = C.c_int64()
        _lib.check(self.L.pmk_query_get_items_cov_factor(self.h, int(region), C.byref(m), None, 0),
                   "pmk_query_get_items_cov_factor")
        n = max(m.value, 1)
        buf = np.zeros((n, n))                      # buf[b, a] = L[a + ldl b]
        _lib.check(self.L.pmk_query_get_items_cov_factor(self.h, int(region), None, _d(buf), n),
                   "pmk_query_get_items_cov_factor")
        return np.ascontiguousarray(buf[:m.value, :m.value].T)

    def draw(self, weight_theta, z, out=None):
        """pmk_query_draw: z [n_draws, total_items], row s the standard normals of draw s in sorted-item order (region r
        owns the columns region_offsets[r] .. region_offsets[r + 1] - 1, in the row order of item_covs) -> E [n_draws, Nq],
        the zero-mean part of the draws.  z and out are numpy arrays (the call blocks) or device arrays such as torch
        tensors (the call enqueues on the context's stream); out defaults to an array of the kind of z."""
        _refuse_closure_kernel(weight_theta, "draw")
        za = GlobalArray(z, "z")
        if len(za.shape) != 2 or za.shape[1] != int(self.total):
            raise _z_shape_error("(n_draws, %d)" % self.total, za.shape)
        n = za.shape[0]
        if za.shape[1] > 1 and za.strides[1] != 1:
            raise ValueError("z must have contiguous rows")
        ldz = za.strides[0] if n > 1 else max(int(self.total), 1)
        if out is None:
            if za.device:
                import torch
                out = torch.empty((n, self.Nq), dtype=torch.float64, device=z.device)
            else:
                out = np.empty((n, self.Nq))
        ea = GlobalArray(out, "out")
        if ea.shape != (n, self.Nq) or (self.Nq > 1 and ea.strides[1] != 1):
            raise ValueError("out must have shape (%d, %d) and contiguous rows, not %s" % (n, self.Nq, ea.shape))
        lde = ea.strides[0] if n > 1 else max(self.Nq, 1)
        d = weight_theta.desc()
        _lib.check(self.L.pmk_query_draw(self.h, C.byref(d), n, za.ptr, ldz, ea.ptr, lde), "pmk_query_draw")
        return out

    def debug(self):
        home = np.empty(self.Nq, dtype=np.int64)
        off = np.empty(self.Nq + 1, dtype=np.int64)
        T = max(self.total, 1)
        reg = np.empty(T, dtype=np.int64)
        t, w, u, v = (np.empty(T) for _ in range(4))
        _lib.check(self.L.pmk_query_debug(self.h, _i(home), _i(off), _i(reg), _d(t), _d(w), _d(u), _d(v)), "pmk_query_debug")
        n = self.total
        return dict(home=home, item_offsets=off, item_region=reg[:n], item_t=t[:n], item_w=w[:n], item_u=u[:n],
                    item_v=v[:n])


def _need_kernels(model):
    """the calls that run on the model's own kernels; the model of a query may be a test's plain stand-in"""
    if not getattr(model, "_has_kernels", False):
        raise _lib.PmkError("the model holds no kernels: fit it, or set_kernels on a model built from factors")


def _theta_arg(model, theta, check, who):
    """the pmk_kernel_desc * argument of a query call that takes `theta` for every patch or (None) the model's own kernels
    -> (pointer, descriptor).  check(theta, who) -> descriptor refuses what the call cannot take (_grad_kernel,
    _closure_free_kernel); the descriptor has to live until the library call returns."""
    if theta is None:
        _need_kernels(model)
        return None, None
    d = check(theta, who)
    return C.byref(d), d


def _closure_free_kernel(theta, who):
    """the descriptor of a kernel the covariance, block and draw calls accept: closure-carrying kernels are refused
    (TypeError) before any device call"""
    _refuse_closure_kernel(theta, who)
    return theta.desc()


def _grad_kernel(theta, who):
    """the descriptor of a kernel the gradient calls accept, checked before any device call: closure-carrying kernels are
    refused with the TypeError of the trend, the Brownian-bridge families (not differentiable on the diagonal) with a
    ValueError"""
    d = _closure_free_kernel(theta, who)
    if d.family >= 10:                          # PMK_BB10 .. PMK_BB2EPS
        raise ValueError("%s: %s is a Brownian-bridge kernel, which is not differentiable on the diagonal: no gradient"
                         % (who, type(theta).__name__))
    return d


def kernel_points(theta, X):
    """the points the device evaluates the kernel on: X itself, or X with the warp features appended for the
    closure-carrying kernels (kernels.py: AdaptiveKernelType & co.)"""
    return theta.augment(X) if getattr(theta, "warped", False) else as_points(X)


MAX_OUTPUTS = 16      # PMK_MAX_OUTPUTS


def multi_targets(Y_parts, n):
    """validate R-column targets against the patch sizes n -> list of float64 n_r x R Fortran arrays (ValueError before
    any device call)"""
    Ys = []
    for y in Y_parts:
        y = np.asarray(y, dtype=np.float64)
        if y.ndim == 1:
            y = y[:, None]
        if y.ndim != 2:
            raise ValueError("targets of a patch must be a vector or an n x R matrix")
        Ys.append(np.asfortranarray(y))
    if len(Ys) != len(n):
        raise ValueError("one target matrix per patch: got %d for %d patches" % (len(Ys), len(n)))
    R = Ys[0].shape[1] if Ys else 0
    if not 1 <= R <= MAX_OUTPUTS:
        raise ValueError("R = %d target columns, outside 1..%d" % (R, MAX_OUTPUTS))
    for r, (y, nr) in enumerate(zip(Ys, n)):
        if y.shape[0] != int(nr):
            raise ValueError("patch %d: %d target rows for %d points" % (r, y.shape[0], int(nr)))
        if y.shape[1] != R:
            raise ValueError("patch %d: %d target columns, patch 0 has %d" % (r, y.shape[1], R))
    return Ys


TREND_DEGREES = {None: -1, "none": -1, "constant": 0, "linear": 1}      # PMK_TREND_NONE / _CONSTANT / _LINEAR


def trend_degree(trend):
    """the PMK_TREND_* value of a trend name (ValueError for an unknown one, before any device call)"""
    if not isinstance(trend, (str, type(None))) or trend not in TREND_DEGREES:
        raise ValueError("trend must be 'none', 'constant' or 'linear', got %r" % (trend,))
    return TREND_DEGREES[trend]


def trend_columns(trend, D, R):
    """q of a trend on D coordinates, checked against the R target columns: R + q <= MAX_OUTPUTS (the basis shares the
    16-column blocks of the multi-output solve with the targets)"""
    q = {-1: 0, 0: 1, 1: 1 + int(D)}[trend_degree(trend)]
    if R + q > MAX_OUTPUTS:
        raise ValueError("R = %d target columns and q = %d trend columns exceed %d" % (R, q, MAX_OUTPUTS))
    return q


class TrendRankException(np.linalg.LinAlgError):
    """the trend basis of a patch is rank deficient (DeviceModel.trend_info)"""

    def __init__(self, patch, flag):
        super().__init__("patch %d: the trend basis is rank deficient (flag %d: a pivot of H^T U^-1 H, or n + 1 for a "
                         "patch with fewer points than basis functions)" % (patch, flag))
        self.patch = patch
        self.flag = flag


def patch_hyper(thetas, sigma2s, P):
    """validate per-patch hyperparameters before any device call -> (pmk_kernel_desc[P], float64 [P] or None).
    ValueError for a wrong length; TypeError for a closure-carrying kernel (anything with a diag_addend, or whose
    kernel_points appends warp features): those change the model's D, and a mix of them is not meaningful."""
    thetas = list(thetas)
    if len(thetas) != P:
        raise ValueError("one kernel per patch: got %d for %d patches" % (len(thetas), P))
    for r, th in enumerate(thetas):
        if hasattr(th, "diag_addend") or getattr(th, "warped", False):
            raise TypeError("patch %d: closure-carrying kernels (%s) cannot be set per patch" % (r, type(th).__name__))
    descs = (_lib.KernelDesc * P)(*[th.desc() for th in thetas])
    if sigma2s is None:
        return descs, None
    s2 = np.ascontiguousarray(sigma2s, dtype=np.float64).reshape(-1)
    if len(s2) != P:
        raise ValueError("one noise variance per patch: got %d for %d patches" % (len(s2), P))
    return descs, s2


MAX_APPEND_ITEMS = 16384     # PMK_COV_MAX_QUERIES: the appended items run through the covariance sweep
MAX_APPEND_PATCH_ROWS = 128  # the points one patch can take in one call (the border factors S in one LDS tile)


def check_append_counts(counts, n, free_rows=None):
    """the rows asked for against the free rows ld_r - n_r of every patch (free_rows: DeviceModel.capacity(); None: a model
    without reserved rows, ld_r = 128 ceil(n_r / 128)), against MAX_APPEND_PATCH_ROWS, and the items of one call against
    MAX_APPEND_ITEMS (ValueError before any device call)"""
    for r, (m, nr) in enumerate(zip(counts, n)):
        free = 128 * ((int(nr) + 127) // 128) - int(nr) if free_rows is None else int(free_rows[r])
        if m > free:
            raise ValueError("patch %d has %d free rows (n = %d), %d rows asked for" % (r, free, int(nr), int(m)))
        if m > MAX_APPEND_PATCH_ROWS:
            raise ValueError("%d points for patch %d in one call, the limit is %d per patch" % (int(m), r, MAX_APPEND_PATCH_ROWS))
    if int(np.sum(counts)) > MAX_APPEND_ITEMS:
        raise ValueError("%d items in one call, the limit is %d" % (int(np.sum(counts)), MAX_APPEND_ITEMS))


def append_items(X_new_parts, y_new_parts, diag_parts, n, D, free_rows=None):
    """validate the lists of DeviceModel.append against the patch sizes n and the dimension D -> (x [T, D], y [T],
    diag [T] or None, patch int32 [T], parts): the items grouped by patch, and the new points of every patch as (m_r, D)
    arrays.  ValueError for a wrong length, shape, a non-finite value or a full patch, before any device call."""
    P = len(n)
    parts, ys = list(X_new_parts), list(y_new_parts)
    ds = None if diag_parts is None else list(diag_parts)
    for what, lst in (("array of new points", parts), ("vector of new targets", ys), ("vector of addends", ds)):
        if lst is not None and len(lst) != P:
            raise ValueError("one %s per patch: got %d for %d patches" % (what, len(lst), P))
    out_x, out_y, out_d = [], [], []
    for r in range(P):
        x = np.asarray(parts[r], dtype=np.float64)
        if x.size == 0:
            x = x.reshape(0, D)
        elif x.ndim == 1:
            x = x.reshape(-1, D) if D == 1 else x.reshape(1, -1)
        if x.ndim != 2 or x.shape[1] != D:
            raise ValueError("patch %d: new points must have shape (m, %d), not %s" % (r, D, x.shape))
        y = np.asarray(ys[r], dtype=np.float64).reshape(-1)
        if len(y) != x.shape[0]:
            raise ValueError("patch %d: %d targets for %d new points" % (r, len(y), x.shape[0]))
        d = np.zeros(len(y)) if ds is None or ds[r] is None else np.asarray(ds[r], dtype=np.float64).reshape(-1)
        if len(d) != len(y):
            raise ValueError("patch %d: %d addends for %d new points" % (r, len(d), len(y)))
        if not (np.all(np.isfinite(x)) and np.all(np.isfinite(y)) and np.all(np.isfinite(d))):
            raise ValueError("patch %d: non-finite coordinate, target or addend" % r)
        out_x.append(np.ascontiguousarray(x))
        out_y.append(y)
        out_d.append(d)
    counts = np.array([len(y) for y in out_y], dtype=np.int64)
    check_append_counts(counts, n, free_rows)
    patch = np.repeat(np.arange(P, dtype=np.int32), counts)
    x = np.ascontiguousarray(np.vstack(out_x)) if P else np.zeros((0, D))
    diag = None if ds is None else np.ascontiguousarray(np.concatenate(out_d))
    return x, np.ascontiguousarray(np.concatenate(out_y)), diag, patch, out_x


MAX_REMOVE_ROWS = 32         # PMK_REMOVE_MAX_ROWS: the rows one patch can lose in one call


def check_remove_counts(counts, n):
    """the rows asked for against the rows every patch can lose, n_r - 128 (ceil(n_r / 128) - 1) - 1, and against
    MAX_REMOVE_ROWS (ValueError before any device call)"""
    for r, (m, nr) in enumerate(zip(counts, n)):
        can = int(nr) - 128 * ((int(nr) + 127) // 128 - 1) - 1
        if m > can:
            raise ValueError("patch %d has %d removable rows (n = %d), %d rows asked for" % (r, can, int(nr), int(m)))
        if m > MAX_REMOVE_ROWS:
            raise ValueError("%d rows of patch %d in one call, the limit is %d" % (int(m), r, MAX_REMOVE_ROWS))


def remove_items(rows_parts, n):
    """validate the lists of DeviceModel.remove against the patch sizes n -> (patch int32 [T], row int64 [T], parts): the
    items grouped by patch and every patch's rows, ascending.  ValueError for a wrong length, a non-integer array, a row
    out of range or given twice, or too many rows, before any device call."""
    P = len(n)
    parts = list(rows_parts)
    if len(parts) != P:
        raise ValueError("one array of rows per patch: got %d for %d patches" % (len(parts), P))
    out = []
    for r in range(P):
        a = np.asarray(parts[r])
        if a.size and not np.issubdtype(a.dtype, np.integer):
            raise ValueError("patch %d: the rows must be integers, not %s" % (r, a.dtype))
        a = np.sort(a.astype(np.int64).reshape(-1))
        if a.size and (a[0] < 0 or a[-1] >= int(n[r])):
            raise ValueError("patch %d: a row outside 0 .. %d" % (r, int(n[r]) - 1))
        if a.size > 1 and np.any(np.diff(a) == 0):
            raise ValueError("patch %d: a row is given twice" % r)
        out.append(a)
    counts = np.array([len(a) for a in out], dtype=np.int64)
    check_remove_counts(counts, n)
    patch = np.repeat(np.arange(P, dtype=np.int32), counts)
    row = np.ascontiguousarray(np.concatenate(out)) if P else np.zeros(0, dtype=np.int64)
    return patch, row, out


def fit_patches(X_parts, y_parts, theta, sigma2, ctx=None, dtype="f64"):
    """create + fit + info + weights: the batched path behind fitmixtureGP! and fitRKHS!.  X_parts are POSITIONS: for a
    warp-feature kernel the model is built on the augmented points, and a DPP kernel's point-dependent diagonal term goes
    in as the per-point addend (pmk_model_set_diag)."""
    model = DeviceModel([kernel_points(theta, x) for x in X_parts], y_parts, ctx, dtype=dtype)
    if hasattr(theta, "diag_addend"):
        model.set_diag([theta.diag_addend(x) for x in X_parts])
    model.fit(theta, sigma2)
    info = model.info()
    cs = model.weights()
    return model, cs, info


class _LazyFactors:
    """L_set / U_set of the reference, materialised from the device on first access"""

    def __init__(self, eta, what):
        self._eta, self._what, self._cache = eta, what, {}

    def __len__(self):
        return len(self._eta.c_set)

    def __getitem__(self, r):
        if r not in self._cache:
            if self._eta._model is None:
                raise _lib.PmkError("the model is not fitted")
            self._cache[r] = self._eta._model.get(r, self._what)
        return self._cache[r]


class MixtureGPType:
    """MixtureGPType(X_parts, hps)   (mixtureGP.jl:38-66)"""

    def __init__(self, X_parts, hps):
        self._from_tree = False
        self.X_parts = [as_points(x) for x in X_parts]
        self._setup(len(self.X_parts), hps)

    def _setup(self, N, hps):
        self.c_set = [None] * N
        self.sigma2_set = [None] * N
        self.hps = hps
        self._model = None
        self.U_set = _LazyFactors(self, GET_K)      # K without noise (mixtureGP.jl:99)
        self.L_set = _LazyFactors(self, GET_L)      # cholesky(U).L    (mixtureGP.jl:112)

    @classmethod
    def from_tree(cls, root, X, eps=None, hps=None, ctx=None, dtype="f64", reserve=None):
        """MixtureGPType on the patches of a tree, built on the device from ONE global point array (numpy or a device
        array): DeviceModel.from_tree.  eps=None: the tree's leaves (setuppartition); eps >= 0: the eps-sets
        (organizetrainingsets).  On such an eta fitmixtureGP_ / _multi_ / _patches_ take the GLOBAL targets (N values, or
        N x R) and refit this resident model: no model is created per call.  reserve: rows every patch (an int) or each
        patch can still take through appendmixtureGP_ (DeviceModel.reserve)."""
        model = DeviceModel.from_tree(root, X, None, eps, ctx, dtype, reserve=reserve)
        self = cls.__new__(cls)
        self._from_tree = True
        self._X_parts = None
        self._setup(model.P, hps)
        self._model = self._tree_model = model
        return self

    @property
    def X_parts(self):
        """the points of every patch (on an eta built by from_tree: cut on first use, None for a device X)"""
        if self._X_parts is None and self._from_tree:
            return self._tree_model.X
        return self._X_parts

    @X_parts.setter
    def X_parts(self, value):
        self._X_parts = value

    def __len__(self):
        return len(self.c_set)


def _store_fit(eta, model, cs, sigma2s):
    eta._model = model
    eta.U_set._cache.clear()
    eta.L_set._cache.clear()
    for r in range(len(cs)):
        eta.c_set[r] = cs[r]
        eta.sigma2_set[r] = float(sigma2s[r])


def _raise_if_failed(info):
    bad = np.nonzero(info)[0]
    if len(bad):
        raise PosDefException(int(bad[0]), int(info[bad[0]]))


def fitmixtureGP_(eta, y_parts, theta, sigma2):
    """fitmixtureGP!(η, y_parts, θ, σ²) -> η   (mixtureGP.jl:70-118).  On an eta built by MixtureGPType.from_tree
    y_parts is the GLOBAL target vector (numpy or device array) and the resident model is refitted."""
    if getattr(eta, "_from_tree", False):
        _refuse_closure_kernel(theta, "fitmixtureGP_")
        model = eta._tree_model
        model.set_targets_global(y_parts)
        model.fit(theta, sigma2)
        _raise_if_failed(model.info())
        _store_fit(eta, model, model.weights(), [sigma2] * model.P)
        return eta
    model, cs, info = fit_patches(eta.X_parts, y_parts, theta, sigma2)
    _raise_if_failed(info)
    _store_fit(eta, model, cs, [sigma2] * len(cs))
    return eta


def appendmixtureGP_(eta, X_new_parts, y_new_parts):
    """condition the fitted eta on new observations in place -> eta.  X_new_parts[r], y_new_parts[r] are the new points
    and targets of patch r (empty entries allowed); on an eta built by MixtureGPType.from_tree they are ONE array of new
    points and their targets, assigned to the patches by the tree (DeviceModel.append_global).  The resident factor is
    bordered, not refitted; c_set, L_set and U_set follow.  Raises PosDefException(patch, k) like fitmixtureGP_ when a
    new pivot fails: that patch is then failed as after a failed fit until the next fit (its scores, gradient, covariance
    and leave-one-out items are NaN; the plain item means and variances carry no mark, as after a failed fit), the others
    are conditioned as asked."""
    model = _fitted_model(eta, "appendmixtureGP_")
    if getattr(model, "theta", None) is not None:
        _refuse_closure_kernel(model.theta, "appendmixtureGP_")
    return _store_changed_rows(eta, model, model.append_global, model.append, X_new_parts, y_new_parts)


def _store_changed_rows(eta, model, on_tree, on_lists, *args):
    """the common end of appendmixtureGP_ and removemixtureGP_: the model's *_global call on an eta built by from_tree, its
    list call otherwise, then c_set, L_set, U_set and X_parts follow the resident model -> eta"""
    if getattr(eta, "_from_tree", False):
        on_tree(*args)
        info = model.info()
    else:
        info = on_lists(*args)
        eta.X_parts = model.X
    _store_fit(eta, model, model.weights(), eta.sigma2_set)
    eta.C_set = eta.beta_set = None     # the multi-output and trend state went with the rows: fit those again
    _raise_if_failed(info)
    return eta


def reservemixtureGP_(eta, rows):
    """room for appendmixtureGP_ in the resident model of eta -> eta: afterwards every patch can take `rows` more points
    (an int, or one value per patch), across 128-row block boundaries, at most 128 per patch and call
    (DeviceModel.reserve).  The fit is kept bit for bit; on an eta built by MixtureGPType.from_tree the call also works
    before the first fit."""
    model = eta._tree_model if getattr(eta, "_from_tree", False) else _fitted_model(eta, "reservemixtureGP_")
    model.reserve(rows)
    return eta


def removemixtureGP_(eta, rows_parts):
    """take observations out of the fitted eta in place -> eta.  rows_parts[r] are the ZERO-based rows of patch r to
    remove (empty entries allowed; Python indices, as everywhere in this package: the Julia module takes one-based ones);
    on an eta built by MixtureGPType.from_tree they are ONE array of zero-based GLOBAL point indices, removed from every
    patch that holds them (DeviceModel.remove_global).  The rows are deleted from the resident factor, which is not
    refitted; c_set, L_set, U_set and X_parts follow.  Raises PosDefException(patch, k) like fitmixtureGP_ when a new
    diagonal fails: that patch is then failed as after a failed fit until the next fit."""
    model = _fitted_model(eta, "removemixtureGP_")
    return _store_changed_rows(eta, model, model.remove_global, model.remove, rows_parts)


class MixtureGPDebugType:
    """MixtureGPDebugType(1.0)   (mixtureGP.jl:5-35)"""

    def __init__(self, dummy_val=1.0):
        self.w_tilde_set, self.u_set, self.v_set = [], [], []
        self.region_inds_set, self.p_region_ind_set = [], []
        self.hps_keep_flags_set, self.zs_set, self.ts_set = [], [], []


def _query_points(Xq):
    """query points as an (Nq, D) array; one point may come as a vector"""
    Xq = np.asarray(Xq, dtype=np.float64)
    if Xq.ndim == 1:
        Xq = Xq[None, :]
    return Xq


def querymixtureGP_(Yq, Vq, Xq, eta, root, levels, radius, delta, theta, sigma2, weight_theta, debug_vars,
                    debug_flag=False):
    """querymixtureGP!(Yq, Vq, Xq, η, root, levels, radius, δ, θ, σ², weight_θ, debug_vars; debug_flag)
    (mixtureGP.jl:159-294).  Yq and Vq are resized in place like the reference's resize!."""
    if eta._model is None:
        raise _lib.PmkError("fitmixtureGP_ must run before querymixtureGP_")
    Xq = as_points(Xq)
    model = eta._model
    model.set_bsp(root, 0)          # the tree lives in the positions; a warp-feature kernel's model has more coordinates
    q = DeviceQuery(model, kernel_points(theta, Xq))
    if hasattr(theta, "diag_addend"):
        q.set_diag(theta.diag_addend(Xq))
    q.plan(radius, delta)
    q.items(theta)
    q.mix(weight_theta)
    yq, vq = q.fetch()
    for dst, src in ((Yq, yq), (Vq, vq)):
        if isinstance(dst, list):
            dst[:] = src.tolist()
        else:
            dst.resize(len(src), refcheck=False)
            dst[:] = src
    if debug_flag:
        from .partition import findneighbourpartitions
        dbg = q.debug()
        off = dbg["item_offsets"]
        hps = eta.hps
        # the reference resize!s every field to Nq and assigns (mixtureGP.jl:185-195): a reused debug struct does not grow
        for name in ("w_tilde_set", "u_set", "v_set", "region_inds_set", "p_region_ind_set", "hps_keep_flags_set", "zs_set",
                     "ts_set"):
            getattr(debug_vars, name).clear()
        for j in range(q.Nq):
            s = slice(off[j], off[j + 1])
            debug_vars.w_tilde_set.append(dbg["item_w"][s].copy())
            debug_vars.u_set.append(dbg["item_u"][s].copy())
            debug_vars.v_set.append(dbg["item_v"][s].copy())
            debug_vars.region_inds_set.append(dbg["item_region"][off[j]:off[j + 1] - 1].copy())
            debug_vars.p_region_ind_set.append(int(dbg["home"][j]))
            _, ts, zs, keep = findneighbourpartitions(Xq[j], radius, root, levels, hps, int(dbg["home"][j]), delta)
            debug_vars.hps_keep_flags_set.append(keep)
            debug_vars.zs_set.append(zs)
            debug_vars.ts_set.append(ts)
    return None


def querymixtureGP(Xq, eta, root, levels, radius, delta, theta, sigma2, weight_theta, debug_flag=False):
    """querymixtureGP(Xq or xq, η, ...) -> Yq, Vq, debug_vars   (mixtureGP.jl:120-157)"""
    Xq = _query_points(Xq)
    Yq, Vq = np.empty(0), np.empty(0)
    dbg = MixtureGPDebugType(1.0)
    querymixtureGP_(Yq, Vq, Xq, eta, root, levels, radius, delta, theta, sigma2, weight_theta, dbg, debug_flag)
    return Yq, Vq, dbg


def queryinner(xq, X, theta, c, L):
    """queryinner(xq, X, θ, c, L) -> (μ, σ²)   (mixtureGP.jl:296-320): the factors are uploaded
    (pmk_model_load) and one strip of the prediction kernel runs against them"""
    xq = np.asarray(xq, dtype=np.float64)[None, :]
    model = DeviceModel.from_factors([kernel_points(theta, X)], [c], [L])
    if hasattr(theta, "diag_addend"):
        # k(xq, xq) carries the kernel's own diagonal term: unclamped variance from the device, term added, then the clamp
        Xk = kernel_points(theta, xq)
        mu, var = np.empty(1), np.empty(1)
        d = theta.desc()
        _lib.check(model.ctx.L.pmk_model_queryinner_ex(model.h, 0, C.byref(d), 1, _d(Xk), -np.inf, _d(mu), _d(var)),
                   "pmk_model_queryinner_ex")
        return float(mu[0]), float(max(var[0] + theta.diag_addend(xq)[0], 1e-12))
    mu, var = model.queryinner(0, theta, kernel_points(theta, xq))
    return float(mu[0]), float(var[0])


def _fit_columns(eta, Y_parts, theta, sigma2, who, trend=None):
    """fitmixtureGP_ on column 0, then the R columns as the model's multi-output targets -> the model.  On an eta built
    by from_tree (which takes no closure-carrying kernel) Y_parts is the GLOBAL (N, R) column-major array, whose first
    column is N contiguous values; otherwise one vector or n_r x R matrix per patch.  trend: R + q <= MAX_OUTPUTS is
    checked before the fit (None: q = 0, and the targets' own check has bounded R)."""
    if getattr(eta, "_from_tree", False):
        _refuse_closure_kernel(theta, who)
        model = eta._tree_model
        ya = GlobalArray(Y_parts, "Y")
        R, _ = ya.columns(model.N)
        if trend is not None:
            trend_columns(trend, model.D, R)
        col0 = Y_parts if len(ya.shape) == 1 else Y_parts[:, 0]
        fitmixtureGP_(eta, col0, theta, sigma2)
        model.set_targets_multi_global(Y_parts)
        return model
    Ys = multi_targets(Y_parts, [x.shape[0] for x in eta.X_parts])
    if trend is not None:
        trend_columns(trend, eta.X_parts[0].shape[1], Ys[0].shape[1])
    fitmixtureGP_(eta, [y[:, 0].copy() for y in Ys], theta, sigma2)
    model = eta._model
    model.set_targets_multi(Ys)
    return model


def fitmixtureGP_multi_(eta, Y_parts, theta, sigma2):
    """fitmixtureGP! (mixtureGP.jl:70-118) with R target columns per patch that share one factor: the fit runs once on
    column 0 (c_set, L_set as fitmixtureGP_ leaves them), then every column is solved from the resident factor
    (c = U \\ y of mixtureGP.jl:106 for R right-hand sides).  Stores eta.C_set (a list of n_r x R)."""
    eta.beta_set = None             # the coefficients of an earlier fitmixtureGP_trend_ do not belong to this fit
    model = _fit_columns(eta, Y_parts, theta, sigma2, "fitmixtureGP_multi_")
    if getattr(eta, "_from_tree", False):
        model.set_trend(None)           # the resident model may carry the trend of an earlier fitmixtureGP_trend_
    model.solve_multi()
    eta.C_set = model.weights_multi()
    return eta


def fitmixtureGP_trend_(eta, Y_parts, theta, sigma2, trend="constant"):
    """fitmixtureGP_multi_ with a trend: ordinary ("constant", h = [1]) or universal ("linear", h(x) = [1, x_1 .. x_D] in
    the raw coordinates) kriging with one generalised-least-squares drift per patch.  Y_parts as for fitmixtureGP_multi_
    (vectors or n_r x R columns; the GLOBAL (N,) or (N, R) array on an eta built by from_tree); R + q <= 16.  Runs fit ->
    multi-output targets -> trend -> solve and stores eta.C_set (the universal-kriging weights, n_r x R) and eta.beta_set
    (q x R per patch).  querymixtureGP_multi / _multi_patches, logevidencemixtureGP_multi (its quadratic form is then the
    GLS one) and loomixtureGP_multi serve unchanged.  Raises TrendRankException for a flagged patch."""
    trend_degree(trend)
    _refuse_closure_kernel(theta, "fitmixtureGP_trend_")     # a warp-feature model has more coordinates than positions
    model = _fit_columns(eta, Y_parts, theta, sigma2, "fitmixtureGP_trend_", trend)
    model.set_trend(trend)
    model.solve_multi()
    flags = model.trend_info()
    bad = np.nonzero(flags)[0]
    if len(bad):
        raise TrendRankException(int(bad[0]), int(flags[bad[0]]))
    eta.C_set = model.weights_multi()
    eta.beta_set = model.trend()[0]
    return eta


def querymixtureGP_multi(Xq, eta, root, levels, radius, delta, theta, sigma2, weight_theta, variance=True):
    """querymixtureGP (mixtureGP.jl:120-294) for the R columns of fitmixtureGP_multi_ -> (Yq [Nq, R], Vq or None).
    variance=False runs no triangular solve: the means need only kq . C (queryinner!, mixtureGP.jl:296-316)."""
    if eta._model is None or getattr(eta, "C_set", None) is None:
        raise _lib.PmkError("fitmixtureGP_multi_ must run before querymixtureGP_multi")
    Xq = as_points(_query_points(Xq))
    model = eta._model
    model.set_bsp(root, 0)
    q = DeviceQuery(model, kernel_points(theta, Xq))
    if hasattr(theta, "diag_addend"):
        q.set_diag(theta.diag_addend(Xq))
    q.plan(radius, delta)
    q.items_multi(theta, variance)
    q.mix_multi(weight_theta)
    return q.fetch_multi(model.R)


def querymixtureGP_grad(Xq, eta, root, levels, radius, delta, theta, sigma2, weight_theta, variance=False):
    """querymixtureGP_multi's blended means and their gradient -> (Yq [Nq, R], dYq [Nq, R, D]), dYq[j, c, d] = dY_c/dx_d,
    for the R columns of fitmixtureGP_multi_ or fitmixtureGP_trend_.  No triangular solve runs.  The derivative holds each
    query's item list fixed: where the list changes (the radius cut-off unless the weight profile vanishes there, a delta
    test, a change of home leaf) the blend itself jumps and has no derivative.  Closure-carrying kernels raise TypeError,
    Brownian-bridge kernels ValueError, before any device call.
    variance=True: also the blended variance and its gradient -> (Yq, Vq [Nq], dYq, dVq [Nq, D]), dVq[j, d] = dVq/dx_d;
    the strip kernel runs for the variance and the strip sweep with D + 1 right-hand sides for its gradient."""
    _grad_kernel(theta, "querymixtureGP_grad")
    _grad_kernel(weight_theta, "querymixtureGP_grad")
    if eta._model is None or getattr(eta, "C_set", None) is None:
        raise _lib.PmkError("fitmixtureGP_multi_ must run before querymixtureGP_grad")
    Xq = as_points(_query_points(Xq))
    model = eta._model
    model.set_bsp(root, 0)
    q = DeviceQuery(model, Xq)
    q.plan(radius, delta)
    q.items_multi(theta, bool(variance))
    q.items_grad(theta)
    if variance:
        q.items_vgrad(theta)
    q.mix_multi(weight_theta)
    q.mix_grad(weight_theta)
    if not variance:
        return q.fetch_multi(model.R)[0], q.fetch_grad()
    q.mix_vgrad(weight_theta)
    Yq, Vq = q.fetch_multi(model.R)
    return Yq, Vq, q.fetch_grad(), q.fetch_vgrad()


# ---- model selection: is this (theta, sigma2) any good on this patch?  The reference picks both by hand
# (examples/mixGP.jl:32-35).  Both scores come from the factor that fitmixtureGP_ left on the device; they are PER PATCH
# (overlapping eps-sets put a training point into several patches, and it has one score in each).
def _fitted_model(eta, who):
    if getattr(eta, "_model", None) is None:
        raise _lib.PmkError("fitmixtureGP_ must run before %s" % who)
    return eta._model


def _log_evidence(logdet, quad, n):
    """-1/2 y^T c - 1/2 log det (K + sigma2 I) - n/2 log(2 pi)"""
    return -0.5 * quad - 0.5 * logdet - 0.5 * n * np.log(2.0 * np.pi)


def logevidencemixtureGP(eta):
    """log marginal likelihood of every patch, -1/2 y^T c - 1/2 log det (K + sigma2 I) - n/2 log(2 pi)  -> array [P]"""
    model = _fitted_model(eta, "logevidencemixtureGP")
    logdet, quad = model.evidence()
    return _log_evidence(logdet, quad, model.n)


def logevidencemixtureGP_multi(eta):
    """the same for the R columns of fitmixtureGP_multi_ -> array [P, R] (one log det per patch serves every column)"""
    model = _fitted_model(eta, "logevidencemixtureGP_multi")
    logdet, quad = model.evidence_multi()
    return _log_evidence(logdet[:, None], quad, model.n[:, None])


def loomixtureGP(eta):
    """leave-one-out residuals and variances of every training point of every patch -> (res_set, var_set):
    res_set[r][i] = y_i - mu_-i (so mu_-i = y_i - res_set[r][i]), var_set[r][i] = the predictive variance of y_i from
    the other n_r - 1 points of patch r, noise included.  One pass over the resident factor, no refit."""
    model = _fitted_model(eta, "loomixtureGP")
    model.loo()
    return model.loo_values()


def loomixtureGP_multi(eta):
    """the same for the R columns of fitmixtureGP_multi_ -> (RES_set [n_r x R each], var_set)"""
    model = _fitted_model(eta, "loomixtureGP_multi")
    model._need(multi=True)
    model.loo()
    return model.loo_values_multi()


# ---- per-patch kernels and noise: MixtureGPType carries one sigma2 per patch (sigma2_set, mixtureGP.jl:44,114) and the
# reference fills it with one value; here every patch may have its own theta and sigma2, which is what the per-patch
# scores above are for.  The mixture weight kernel stays global.
def fitmixtureGP_patches_(eta, y_parts, thetas, sigma2s):
    """fitmixtureGP! (mixtureGP.jl:70-118) with thetas[r], sigma2s[r] for patch r -> eta.  Fills eta.sigma2_set[r] with
    the patch's own value and eta.theta_set; raises PosDefException(patch, k) like fitmixtureGP_."""
    patch_hyper(thetas, sigma2s, len(eta.c_set))
    if getattr(eta, "_from_tree", False):
        model = eta._tree_model
        model.set_targets_global(y_parts)           # the GLOBAL targets; the resident model is refitted
    else:
        model = DeviceModel(eta.X_parts, y_parts)
    model.fit_patches(thetas, sigma2s)
    _raise_if_failed(model.info())
    _store_fit(eta, model, model.weights(), sigma2s)
    eta.theta_set = list(thetas)
    return eta


def _patches_query(Xq, eta, root, radius, delta, who):
    if getattr(eta, "_model", None) is None or not getattr(eta._model, "_has_kernels", False):
        raise _lib.PmkError("fitmixtureGP_patches_ (or fitmixtureGP_) must run before %s" % who)
    Xq = _query_points(Xq)
    model = eta._model
    model.set_bsp(root, 0)
    q = DeviceQuery(model, as_points(Xq))
    q.plan(radius, delta)
    return q


def querymixtureGP_patches(Xq, eta, root, levels, radius, delta, weight_theta, debug_flag=False):
    """querymixtureGP (mixtureGP.jl:120-294) with the model's own kernels: region r is evaluated with the theta it was
    fitted with -> (Yq, Vq, debug dict or None: DeviceQuery.debug())"""
    q = _patches_query(Xq, eta, root, radius, delta, "querymixtureGP_patches")
    q.items_fitted()
    q.mix(weight_theta)
    Yq, Vq = q.fetch()
    return Yq, Vq, (q.debug() if debug_flag else None)


def _refuse_closure_front_end(eta, weight_theta, who):
    """closure-carrying kernels (the blending profile, then the theta of the fit) raise TypeError before any device call,
    as in the gradient front ends: their addends and warp features are functions of x the batch's joint covariance would
    have to carry"""
    _refuse_closure_kernel(weight_theta, who)
    theta = getattr(getattr(eta, "_model", None), "theta", None)
    if theta is not None:
        _refuse_closure_kernel(theta, who)


def _fitted_query(Xq, eta, root, radius, delta, weight_theta, who, multi, variance=True, mix=True):
    """the planned query of the covariance, draw and block front ends, closure-carrying kernels refused: the items on the
    model's own kernels, of the single-output path or (multi) of the R resident columns, and (mix) their blend"""
    _refuse_closure_front_end(eta, weight_theta, who)
    q = _patches_query(Xq, eta, root, radius, delta, who)
    if multi:
        q.model._need(multi=True)
        q.items_multi_fitted(variance)
    else:
        q.items_fitted()
    if mix:
        (q.mix_multi if multi else q.mix)(weight_theta)
    return q


def _cov_query(Xq, eta, root, radius, delta, weight_theta, who):
    """_fitted_query with the region blocks and the joint covariance of the batch"""
    q = _fitted_query(Xq, eta, root, radius, delta, weight_theta, who, False)
    q.items_cov()
    q.mix_cov(weight_theta)
    return q


def querymixtureGP_cov(Xq, eta, root, levels, radius, delta, weight_theta):
    """querymixtureGP_patches with the joint posterior covariance of the batch under the blend -> (Yq, Vq, Cov [Nq, Nq]).
    The patches are independent GPs: Cov[j, k] sums wn_j wn_k (k_r(x_j, x_k) - V_j . V_k) over the regions that hold an
    item of both queries, and is exactly 0 where they share none; its diagonal is Vq up to rounding.  Single-output path,
    no trend; at most 16384 queries."""
    q = _cov_query(Xq, eta, root, radius, delta, weight_theta, "querymixtureGP_cov")
    Yq, Vq = q.fetch()
    return Yq, Vq, q.fetch_cov()


def _z_shape_error(want, got):
    return ValueError("z must have shape %s, not %s" % (want, got))


def _normals(z, shape, dev, generator):
    """the standard normals of the draws as a float64 tensor of `shape` on `dev`: z if given, else from `generator`"""
    import torch

    if z is None:
        return torch.randn(shape, dtype=torch.float64, device=dev, generator=generator)
    z = torch.as_tensor(z, dtype=torch.float64, device=dev)
    if tuple(z.shape) != shape:
        raise _z_shape_error(shape, tuple(z.shape))
    return z


def _dense_draw(q, n_draws, R, generator, z, who, nan_patch):
    """method="dense" of the sampling front ends, on a query whose joint covariance is mixed -> (L, z, jitter): the
    covariance fetched into a device tensor, refused with `nan_patch` (what a patch behind a NaN suffers from) if it is
    not finite, its Cholesky factor under the jitter ladder of samplemixtureGP, and the normals z [n_draws, Nq] or
    (R columns) [n_draws, Nq, R]"""
    import torch

    dev = torch.device("cuda", q.model.ctx.device)
    Nq = q.Nq
    Cov = torch.empty((Nq, Nq), dtype=torch.float64, device=dev)
    q.fetch_cov_into(Cov)
    q.model.ctx.synchronize()                   # the copies ran on the context's stream, torch reads on its own
    if not bool(torch.isfinite(Cov).all()):
        # a query that blends a patch whose factorisation failed is NaN in its row and column; the factorisation need
        # not report a NaN through info, and the draws would be NaN with jitter == 0.0
        raise np.linalg.LinAlgError("%s: the joint covariance holds NaN or Inf entries: a query of the batch blends a patch "
                                    "%s" % (who, nan_patch))
    scale = float(torch.trace(Cov)) / max(Nq, 1)
    jitter, eye = 0.0, torch.eye(Nq, dtype=torch.float64, device=dev)
    while True:
        L, info = torch.linalg.cholesky_ex(Cov + jitter * eye if jitter else Cov)
        if int(info) == 0:
            break
        jitter = 2.0 ** -52 * scale if jitter == 0.0 else 10.0 * jitter
        if not jitter <= 2.0 ** -26 * scale:
            raise np.linalg.LinAlgError("%s: the joint covariance is not positive definite with a jitter of up to 2^-26 "
                                        "trace / Nq" % who)
    shape = (int(n_draws), Nq) if R is None else (int(n_draws), Nq, R)
    return L, _normals(z, shape, dev, generator), jitter


def _sample_blocks(q, multi, weight_theta, n_draws, generator, z, who):
    """method="blocks" of the sampling front ends, on a planned query whose means are mixed: the region blocks, their
    factors under the per-region jitter ladder, and the zero-mean draws E [n_draws, Nq] or [n_draws, Nq, R]
    -> (E, jitter)"""
    import torch

    dev = torch.device("cuda", q.model.ctx.device)
    P, R = int(q.model.P), (int(q.model.R) if multi else None)
    q.items_cov_blocks(None, multi)
    held = np.diff(q.region_offsets(P)) > 0
    rel = np.zeros(P)
    q.factor_cov(rel)
    while True:
        finfo, jit = q.factor_info()
        bad = np.nonzero(held & (finfo == -1))[0]
        if len(bad):
            raise np.linalg.LinAlgError("%s: region %d holds items of the batch and its patch is failed (DeviceModel.info())"
                                        " or its trend is flagged (DeviceModel.trend_info())" % (who, int(bad[0])))
        failed = np.nonzero(finfo > 0)[0]
        if not len(failed):
            break
        nxt = np.where(rel[failed] == 0.0, 2.0 ** -52, 10.0 * rel[failed])
        over = failed[~(nxt <= 2.0 ** -26)]
        if len(over):
            raise np.linalg.LinAlgError("%s: the block of region %d is not positive definite with a jitter of up to 2^-26 "
                                        "trace / m" % (who, int(over[0])))
        rel[failed] = nxt
        q.factor_cov(rel)
    jitter = float(jit.max()) if P else 0.0
    n, total = int(n_draws), int(q.total)
    z = _normals(z, (n, total) if R is None else (n, total, R), dev, generator)
    # every column's normals as one contiguous array, made before the first draw and held until the last has run: torch
    # writes them (and would reuse a freed one's memory) on its own stream, the library reads on the context's
    cols = [z.contiguous()] if R is None else [z[:, :, c].contiguous() for c in range(R)]
    torch.cuda.synchronize(dev)
    E = [q.draw(weight_theta, zc) for zc in cols]
    q.model.ctx.synchronize()                   # the draws are enqueued: torch reads them after this
    return (E[0] if R is None else torch.stack(E, dim=2)), jitter


def samplemixtureGP(Xq, eta, root, levels, radius, delta, weight_theta, n_draws, generator=None, z=None, method="dense"):
    """posterior draws of the latent blended field at Xq -> (draws [n_draws, Nq] as a torch device tensor, jitter).
    The joint covariance of querymixtureGP_cov is fetched into a device tensor and factored with torch's Cholesky
    (_dense_draw); if that fails, jitter * I is added, starting at 2^-52 trace / Nq and multiplied by 10 up to
    2^-26 trace / Nq, after which LinAlgError is raised.  A batch that blends a patch whose factorisation failed has NaN
    in its covariance and raises LinAlgError before any factorisation.  The jitter that was used is returned (0.0: none).  z
    [n_draws, Nq]: the standard normals to use; otherwise they are drawn from `generator`.  draws = Yq + z L^T.

    method="blocks" never forms the Nq x Nq matrix: every region block is factored on its own (DeviceQuery.factor_cov)
    and the draws are the blend of L_r z_r (DeviceQuery.draw), so Nq may exceed 16384.  z is then [n_draws, total_items]
    in sorted-item order.  The jitter ladder runs per region, for the failed regions only: rel = 2^-52, then x 10 while
    rel <= 2^-26, on the scale trace S_r / m_r; after that LinAlgError names the region.  A region that holds items and
    whose patch is failed raises LinAlgError before any draw.  The jitter returned is the largest absolute value added."""
    import torch

    if method not in ("dense", "blocks"):
        raise ValueError("method must be \"dense\" or \"blocks\", not %r" % (method,))
    who = "samplemixtureGP"
    if method == "blocks":
        q = _fitted_query(Xq, eta, root, radius, delta, weight_theta, who, False)
    else:
        q = _cov_query(Xq, eta, root, radius, delta, weight_theta, who)
    Yq = torch.empty(q.Nq, dtype=torch.float64, device=torch.device("cuda", q.model.ctx.device))
    q.fetch_into(Yq)
    if method == "blocks":
        E, jitter = _sample_blocks(q, False, weight_theta, n_draws, generator, z, who)
        return Yq[None, :] + E, jitter
    L, z, jitter = _dense_draw(q, n_draws, None, generator, z, who, "whose factorisation failed (DeviceModel.info())")
    return Yq[None, :] + z @ L.T, jitter


def _cov_multi_query(Xq, eta, root, radius, delta, weight_theta, who):
    """_cov_query on the multi-output path: the R blended means, the variances and the region blocks with the term of
    the model's trend, on what fitmixtureGP_multi_ / fitmixtureGP_trend_ left resident"""
    q = _fitted_query(Xq, eta, root, radius, delta, weight_theta, who, True)
    q.items_cov_multi()
    q.mix_cov(weight_theta)
    return q


def querymixtureGP_cov_multi(Xq, eta, root, levels, radius, delta, weight_theta):
    """querymixtureGP_multi_patches with the joint posterior covariance of the batch -> (Yq [Nq, R], Vq, Cov [Nq, Nq]),
    for the R columns of fitmixtureGP_multi_ or fitmixtureGP_trend_ (list-built and from_tree etas).  Under a trend Cov is
    the universal-kriging covariance: every region's term carries z_j . z_k of the drift's uncertainty, and its diagonal
    is the Vq the model predicts, up to rounding.  The covariance does not depend on the targets: the R columns are
    independent fields with a common kernel and share Cov.  At most 16384 queries."""
    q = _cov_multi_query(Xq, eta, root, radius, delta, weight_theta, "querymixtureGP_cov_multi")
    Yq, Vq = q.fetch_multi(q.model.R)
    return Yq, Vq, q.fetch_cov()


def querymixtureGP_block(Xq, group, a, eta, root, levels, radius, delta, weight_theta, variance=True):
    """block kriging (change of support) -> (Yb [F, R], Vb [F] or None): the prediction of sum_j a[j] f(x_j) over the
    queries j of every group and its kriging variance, for the R columns of fitmixtureGP_multi_ or fitmixtureGP_trend_
    (list-built and from_tree etas).  group: int per query, non-decreasing from 0 (F = group[-1] + 1); a: one coefficient
    per query.  A block average over g points is a = 1 / g, an integral takes quadrature weights, a contrast mixes signs.
    Vb is a^T Cov a of querymixtureGP_cov_multi without the Nq x Nq matrix and without its limit of 16384 queries.
    Closure-carrying kernels raise TypeError before any device call."""
    q = _fitted_query(Xq, eta, root, radius, delta, weight_theta, "querymixtureGP_block", True, variance=False, mix=False)
    q.items_block(group, a, weight_theta, variance=variance)
    return q.fetch_block()


def samplemixtureGP_multi(Xq, eta, root, levels, radius, delta, weight_theta, n_draws, generator=None, z=None,
                          method="dense"):
    """posterior draws of the R latent blended fields at Xq -> (draws [n_draws, Nq, R] as a torch device tensor, jitter).
    The joint covariance of querymixtureGP_cov_multi is factored once (_dense_draw: torch's Cholesky, the jitter ladder of
    samplemixtureGP) and serves every column: draws[:, :, c] = Yq[:, c] + z[:, :, c] L^T with independent standard normals
    per column.  z [n_draws, Nq, R]: the normals to use; otherwise they are drawn from `generator`.  A covariance that
    holds NaN (a batch that blends a patch whose factorisation failed or whose trend is flagged) raises LinAlgError
    before any factorisation.

    method="blocks": as in samplemixtureGP, on the blocks of items_cov_multi; z is [n_draws, total_items, R] in sorted-item
    order, and the factors serve every column."""
    import torch

    if method not in ("dense", "blocks"):
        raise ValueError("method must be \"dense\" or \"blocks\", not %r" % (method,))
    who = "samplemixtureGP_multi"
    if method == "blocks":
        q = _fitted_query(Xq, eta, root, radius, delta, weight_theta, who, True)
    else:
        q = _cov_multi_query(Xq, eta, root, radius, delta, weight_theta, who)
    R = int(q.model.R)
    Yq = torch.empty((R, q.Nq), dtype=torch.float64, device=torch.device("cuda", q.model.ctx.device))  # column-major (Nq, R)
    q.fetch_multi_into(Yq.T)
    if method == "blocks":
        E, jitter = _sample_blocks(q, True, weight_theta, n_draws, generator, z, who)
        return Yq.T[None, :, :] + E, jitter
    L, z, jitter = _dense_draw(q, n_draws, R, generator, z, who, "whose factorisation failed (DeviceModel.info()) or whose "
                               "trend is flagged (DeviceModel.trend_info())")
    # column by column, each as samplemixtureGP takes its draws
    return torch.stack([Yq[c][None, :] + z[:, :, c] @ L.T for c in range(R)], dim=2), jitter


def querymixtureGP_multi_patches(Xq, eta, root, levels, radius, delta, weight_theta, variance=True):
    """querymixtureGP_multi with the model's own kernels, for R target columns solved on the resident per-patch factor
    (eta._model.set_targets_multi + solve_multi) -> (Yq [Nq, R], Vq or None)"""
    q = _patches_query(Xq, eta, root, radius, delta, "querymixtureGP_multi_patches")
    q.model._need(multi=True)
    q.items_multi_fitted(variance)
    q.mix_multi(weight_theta)
    return q.fetch_multi(q.model.R)


def _first_best(scores, all_nan):
    """the index of the first of the highest scores; a NaN never wins, and if every score is NaN ValueError(all_nan)"""
    valid = np.nonzero(~np.isnan(scores))[0]
    if len(valid) == 0:
        raise ValueError(all_nan)
    return int(valid[int(np.argmax(scores[valid]))])               # argmax: the first of equal maxima


def select_candidates(scores):
    """winner per patch of a [G, P] score array (higher is better) -> int64 [P].  Ties go to the lowest candidate index,
    a NaN never wins, and a patch whose scores are all NaN raises ValueError naming the patch."""
    scores = np.asarray(scores, dtype=np.float64)
    if scores.ndim != 2 or scores.shape[0] < 1:
        raise ValueError("scores must be a [G, P] array with G >= 1")
    winners = np.empty(scores.shape[1], dtype=np.int64)
    for r in range(scores.shape[1]):
        winners[r] = _first_best(scores[:, r], "patch %d: every candidate scored NaN (no candidate could be factorised)" % r)
    return winners


def loo_log_pseudo_likelihood(res, var):
    """sum_i [-1/2 log var_i - res_i^2 / (2 var_i) - 1/2 log 2 pi] (Rasmussen & Williams eq. 5.10-5.11) of one patch"""
    return float(np.sum(-0.5 * np.log(var) - res * res / (2.0 * var) - 0.5 * np.log(2.0 * np.pi)))


def selectmixtureGP_(eta, y_parts, candidates, score="evidence"):
    """pick (theta, sigma2) per patch from `candidates`, a list of (theta, sigma2), and fit with the winners
    -> (eta, winners [P], scores [G, P]).

    Every candidate is fitted uniformly through the existing calls and scored per patch: "evidence" is the log marginal
    likelihood as logevidencemixtureGP computes it, "loo" the leave-one-out log pseudo-likelihood from loomixtureGP's
    residuals and variances.  A patch whose factorisation fails under a candidate scores NaN for it (no exception);
    select_candidates picks the winners, and one fitmixtureGP_patches_ with them leaves eta fitted.
    Cost: G fits (plus G leave-one-out passes for "loo") plus one fit."""
    if score not in ("evidence", "loo"):
        raise ValueError("score must be 'evidence' or 'loo'")
    candidates = list(candidates)
    if not candidates:
        raise ValueError("no candidates")
    P = len(eta.X_parts)
    for th, _ in candidates:             # the winners go into one per-patch fit: refuse what that fit would refuse, first
        patch_hyper([th] * P, None, P)
    scores = np.empty((len(candidates), P))
    model = DeviceModel(eta.X_parts, y_parts)
    for g, (th, s2) in enumerate(candidates):
        model.fit(th, s2)
        model.info()                     # failed patches score NaN below: the library reports them as NaN
        if score == "evidence":
            logdet, quad = model.evidence()
            scores[g] = _log_evidence(logdet, quad, model.n)
        else:
            model.loo()
            res, var = model.loo_values()
            with np.errstate(invalid="ignore", divide="ignore"):
                scores[g] = [loo_log_pseudo_likelihood(a, b) for a, b in zip(res, var)]
    winners = select_candidates(scores)
    fitmixtureGP_patches_(eta, y_parts, [candidates[w][0] for w in winners], [candidates[w][1] for w in winners])
    return eta, winners, scores



# ---- blended leave-one-out: cross-validate what is deployed, the mixture of querymixtureGP!, without refitting.  Leaving a
# training point out removes it from every patch that holds it; in those patches its prediction is the resident
# leave-one-out value, in a neighbour patch that never held it the ordinary queryinner!, and the blend is the unchanged one.
def _blend_model(eta, who):
    model = _fitted_model(eta, who)
    if not getattr(model, "_from_tree", False):
        raise _lib.PmkError("%s: eta must be built by MixtureGPType.from_tree (the map from patch rows to global points)" % who)
    if not getattr(model, "_has_kernels", False) or not model._has_factor:
        raise _lib.PmkError("%s: fit the model first" % who)
    return model


def _blend_query(model, X, who):
    if X is None:
        X = getattr(model, "_X_global", None)
        if X is None:
            raise _lib.PmkError("%s: the model was built from a device array and holds no host copy of X; pass X" % who)
    q = DeviceQuery(model, X)
    if q.Nq != model.N:
        raise _lib.PmkError("%s: X has %d points, the model %d" % (who, q.Nq, model.N))
    return q


def _blend_loo(model, q, radius, delta, weight_theta, noisy, variance=None):
    """one blended leave-one-out on the query of _blend_query -> what its fetch returns: loo() if it is stale, the plan,
    the items, the blend.  variance=None: the single-output path; else the R columns, with or without the variance"""
    if not model._loo_done:
        model.loo()
    q.plan(radius, delta)
    if variance is None:
        q.items_loo(noisy)
        q.mix(weight_theta)
        return q.fetch()
    q.items_loo_multi(noisy, variance)
    q.mix_multi(weight_theta)
    return q.fetch_multi(model.R)


def _blend_scores(model, q, candidates, R, score):
    """scores [G] (R=None) or [G, R] of the candidates (radius, delta, weight_theta): score(mu, var) of the blended
    leave-one-out with the noisy variances.  One query object, re-planned per candidate."""
    scores = np.empty(len(candidates) if R is None else (len(candidates), R))
    for g, (radius, delta, weight_theta) in enumerate(candidates):
        mu, var = _blend_loo(model, q, radius, delta, weight_theta, True, None if R is None else True)
        with np.errstate(invalid="ignore", divide="ignore"):
            scores[g] = score(mu, var)
    return scores


def loomixtureGP_blend(eta, root, radius, delta, weight_theta, X=None, noisy=False):
    """leave-one-out of the BLENDED predictor -> (mu_loo, var_loo), N values each: what querymixtureGP_patches would
    predict at training point j had the model been fitted without j, the tree held fixed.  No refit: one plan, a lookup
    per item whose patch holds the point, strips for the others, one mix.  eta: built by MixtureGPType.from_tree on `root`
    and fitted (the model carries the tree; `root` keeps the argument order of the query functions).  X: the N training
    points in global order (numpy or device array); default: the host array the model was built from.  noisy: variances
    of the observation (each patch's sigma2 included) rather than of the latent field.  Runs loo() if it is stale."""
    model = _blend_model(eta, "loomixtureGP_blend")
    q = _blend_query(model, X, "loomixtureGP_blend")
    return _blend_loo(model, q, radius, delta, weight_theta, noisy)


def selectblendGP_(eta, root, y, candidates, X=None):
    """score blending settings by the leave-one-out log pseudo-likelihood of the blended predictor -> (scores [G], best).
    candidates: a list of (radius, delta, weight_theta); scores[g] = loo_log_pseudo_likelihood(y - mu_g, var_g) with the
    noisy variances, y the N global targets the model was fitted to; best = the first argmax, a NaN never wins.  One query
    object, re-planned per candidate; the fit is not touched."""
    candidates = list(candidates)
    if not candidates:
        raise ValueError("no candidates")
    model = _blend_model(eta, "selectblendGP_")
    y = np.asarray(y, dtype=np.float64)
    if y.shape != (model.N,):
        raise ValueError("y must hold the %d global targets" % model.N)
    q = _blend_query(model, X, "selectblendGP_")
    scores = _blend_scores(model, q, candidates, None, lambda mu, var: loo_log_pseudo_likelihood(y - mu, var))
    return scores, _first_best(scores, "every candidate scored NaN")


# ---- the same for the multi-output path: R target columns, with or without a trend (fitmixtureGP_multi_ / _trend_)
def _blend_multi_model(eta, who):
    model = _blend_model(eta, who)
    if not getattr(model, "_multi_solved", False):
        raise _lib.PmkError("%s: fitmixtureGP_multi_ or fitmixtureGP_trend_ must run first (solve_multi has not run on the "
                            "resident factor)" % who)
    return model


def loomixtureGP_blend_multi(eta, root, radius, delta, weight_theta, X=None, noisy=False, variance=True):
    """loomixtureGP_blend for the R target columns of fitmixtureGP_multi_ or fitmixtureGP_trend_ -> (MU [N, R], var [N] or
    None): what querymixtureGP_multi_patches would predict at training point j had the model, trend included, been fitted
    without j, the tree held fixed.  No refit.  eta: built by MixtureGPType.from_tree; X, noisy as loomixtureGP_blend.
    variance=False: means only (no strip kernel runs anywhere).  Runs loo() if it is stale.
    With a trend of q basis functions, a point that is a member of a patch of n <= q points gets NaN in its row of MU and
    in var: without it the patch has fewer points than basis functions, so the prediction does not exist."""
    model = _blend_multi_model(eta, "loomixtureGP_blend_multi")
    q = _blend_query(model, X, "loomixtureGP_blend_multi")
    return _blend_loo(model, q, radius, delta, weight_theta, noisy, bool(variance))


def selectblendGP_multi_(eta, root, Y, candidates, X=None):
    """selectblendGP_ for R target columns -> (scores [G, R], best).  candidates: a list of (radius, delta, weight_theta);
    scores[g, c] = loo_log_pseudo_likelihood(Y[:, c] - MU_g[:, c], var_g) with the noisy variances, Y the (N, R) global
    targets the model holds; best = the first argmax of the row sums, a row with a NaN never wins, all-NaN raises
    ValueError.  One query object, re-planned per candidate; the fit is not touched."""
    candidates = list(candidates)
    if not candidates:
        raise ValueError("no candidates")
    model = _blend_multi_model(eta, "selectblendGP_multi_")
    Y = np.asarray(Y, dtype=np.float64)
    if Y.ndim == 1:
        Y = Y[:, None]
    if Y.shape != (model.N, model.R):
        raise ValueError("Y must hold the %d x %d global targets" % (model.N, model.R))
    q = _blend_query(model, X, "selectblendGP_multi_")
    scores = _blend_scores(model, q, candidates, model.R, lambda MU, var: [
        loo_log_pseudo_likelihood(Y[:, c] - MU[:, c], var) for c in range(model.R)])
    return scores, _first_best(scores.sum(axis=1), "every candidate scored NaN")

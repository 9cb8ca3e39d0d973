"""Launch dispatch coverage: every (D, FAM, PP, dtype) instantiation behind launch_kernel_matrix_slabs, launch_items and
launch_items_multi (pmk_dispatch.h) is reached, and is the right one.  The four launchers that came later (launch_items_grad,
launch_items_vgrad, launch_items_cov, launch_items_block): tests/test_gpu_dispatch_stages.py.

One launcher per kernel takes `th`: a descriptor (PP = false, FAM from that descriptor) or null for the model's device
arrays (PP = true, FAM from the model).  The uniform and the per-patch instantiation are the same instruction stream
(header of tests/test_gpu_patches.py), so with P copies of one theta they must agree BIT FOR BIT -- which a wrong PP or a
theta taken from the wrong place breaks -- while a wrong D or FAM that both sides share is caught by the CPU oracle.

Shapes: N = 600 points in [-1, 1]^D on a tree of two levels of splits (four leaves; setuppartition counts the root as a
level: LEVELS = 3) with eps-overlap, 257 queries, 3 target columns.  Four median-split leaves of 600 points hold 150 each
before the overlap, so their eps-sets all have two block rows (128 < n < 256, off the tile edge).  For one and two block
rows side by side every (D, theta, dtype) runs a second time on the "ragged" batch: the same tree and eps-sets with
leaves 1 and 3 cut to their first 100 and 128 points (nt = 1, the second exactly at the tile edge) beside the two-row
leaves 0 and 2; the oracle gets the same patches.  The 257 items of one region in the explicit-theta test are dealt over
two strips.  Both dtypes run at a = 1, sigma2 = 0.05, the setting of tests/test_gpu_family_parity.py, whose fp32 bounds
assume kappa(U) eps32 <= 1e-3: asserted per patch.

No tolerance is new.  Fit: tests/test_gpu_family_parity.py::test_fit_parity_matrix.  Mixture values: SURVEY section 8(d)
(_query_refs.assert_fp64_values) in fp64, tests/test_gpu_patches.py::test_predict_single_output_fp32_... in fp32.
Per-item values on the device's own factors: tests/test_gpu_family_parity.py::test_predict_strip_parity_matrix.
"""
import numpy as np
import pytest
import scipy.linalg as sla

import patchmixturekriging_amd as pmk
from patchmixturekriging_amd import mixture as M
from oracle import oracle as O

import _query_refs as R

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
N, NQ, RCOLS, LEVELS, P, EPS_OVERLAP, RADIUS, DELTA = 600, 257, 3, 3, 4, 0.1, 0.3, 1e-5
A, SIGMA2 = 1.0, 0.05
THETAS = {"spline34": (pmk.Spline34KernelType(A), O.kernel(O.SPLINE34, A)),
          "spline32": (pmk.Spline32KernelType(A), O.kernel(O.SPLINE32, A))}
WTH, OWTH = pmk.Spline34KernelType(1 / RADIUS), O.kernel(O.SPLINE34, 1 / RADIUS)
DIMS, DTYPES = (1, 2, 3, 4), ("f64", "f32")
SHAPES = {"even": None, "ragged": {1: 100, 3: 128}}          # leaf -> points kept of its eps-set

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _data(D, shape="even"):
    """points, tree, eps-sets, targets (column 0 is the single-output target) and queries of dimension D"""
    def cut():
        d = dict(_data(D))
        for key in ("X_set", "Ys", "ys"):
            d[key] = [a[:SHAPES[shape].get(r, len(a))] for r, a in enumerate(d[key])]
        assert [(len(x) + 127) // 128 for x in d["X_set"]] == [2, 1, 2, 1]
        return d

    def make():
        rng = np.random.Generator(np.random.PCG64(9100 + D))
        X = rng.uniform(-1, 1, (N, D))
        Y = np.stack([np.sin(3 * X[:, 0]) + X[:, -1] ** 2, np.cos(2 * X[:, 0] - X[:, -1]), 0.3 * X[:, -1] - 0.1], 1)
        Xq = rng.uniform(-1, 1, (NQ, D))
        root, _, _ = pmk.setuppartition(X, LEVELS)
        X_set, inds, _, _ = pmk.organizetrainingsets(root, LEVELS, X, EPS_OVERLAP)
        assert len(X_set) == P and all(128 < len(x) < 256 for x in X_set), [len(x) for x in X_set]
        return dict(X=X, Xq=Xq, root=root, X_set=X_set, Ys=[Y[i] for i in inds], ys=[Y[i, 0] for i in inds],
                    ob=O.BSP(X, LEVELS))
    return _cached(("data", D, shape), make if shape == "even" else cut)


def _oracle(D, fam, shape="even"):
    """the CPU oracle of one (D, theta): per patch U, kappa(U), the fits of the three columns and the LAPACK factor and
    weights; the mixture of every column.  Computed once, shared by both dtypes, never changed."""
    def make():
        d, oth = _data(D, shape), THETAS[fam][1]
        fits, U, kap, lapack = [], [], [], []
        for X, Yr in zip(d["X_set"], d["Ys"]):
            fits.append([O.fit_patch(oth, X, Yr[:, j], SIGMA2) for j in range(RCOLS)])
            assert all(f["info"] == 0 for f in fits[-1])
            U.append(O.kernel_matrix(oth, X) + SIGMA2 * np.eye(len(X)))
            kap.append(R.kappa(U[-1]))
            assert kap[-1] * EPS32 <= 1e-3, (D, fam, kap[-1])       # what the fp32 bounds assume
            Lref = sla.cholesky(U[-1], lower=True, check_finite=False)
            lapack.append((Lref, sla.cho_solve((Lref, True), Yr[:, 0], check_finite=False)))
        cols = [O.query_mixture(d["ob"], oth, OWTH, d["X_set"], [f[j]["c_lu"] for f in fits], [f[j]["L"] for f in fits],
                                d["Xq"], RADIUS, DELTA) for j in range(RCOLS)]
        return dict(fits=fits, U=U, kappa=kap, lapack=lapack, Y=np.stack([c[0] for c in cols], 1), V=cols[0][1])
    return _cached(("oracle", D, fam, shape), make)


def _factors(m, r):
    return m.get(r, M.GET_L), m.get(r, M.GET_C), m.get(r, M.GET_LINV_DIAG)


def _item_means(m, dbg, Xq, run):
    """per-item means [T, R] (and v [T]) through a query of explicit (point, region) items: one item per 'query', whose
    mixture weight is 1 / 1, so that Yq of that query IS the item's mean (tests/test_gpu_patches.py)"""
    off, reg = dbg["item_offsets"], dbg["item_region"]
    qj = np.searchsorted(off, np.arange(off[-1]), side="right") - 1
    xs = np.ascontiguousarray(Xq[qj])
    rg = np.ascontiguousarray(reg, dtype=np.int32)
    q = pmk.DeviceQuery.from_items(m, len(rg), xs.ctypes.data, rg.ctypes.data)
    run(q)
    q.mix_multi(WTH)
    return q.fetch_multi(m.R)


def _predict(m, d, th):
    """every predict call of one fitted model on one plan: th None runs only the *_fitted calls"""
    out = {}
    m.set_bsp(d["root"], 0)
    q = pmk.DeviceQuery(m, d["Xq"])
    q.plan(RADIUS, DELTA)
    calls = [("fitted", q.items_fitted, lambda qq, v=True: qq.items_multi_fitted(v))]
    if th is not None:
        calls.insert(0, ("theta", lambda: q.items(th), lambda qq, v=True: qq.items_multi(th, v)))
    m.set_targets_multi(d["Ys"])
    m.solve_multi()
    for name, items, items_multi in calls:
        items()
        q.mix(WTH)
        dbg = q.debug()
        Yq, Vq = q.fetch()
        items_multi(q)
        q.mix_multi(WTH)
        Ym, Vm = q.fetch_multi(RCOLS)
        U, v = _item_means(m, dbg, d["Xq"], items_multi)
        Um, none = _item_means(m, dbg, d["Xq"], lambda qq: items_multi(qq, False))          # mean-only: no strip launch
        assert none is None and np.array_equal(Um, U)
        out[name] = dict(dbg=dbg, u=dbg["item_u"], v=dbg["item_v"], Yq=Yq, Vq=Vq, Ym=Ym, Vm=Vm, means=U, means_v=v)
    out["C"] = m.weights_multi()
    return out


def _run(D, fam, dtype, shape="even"):
    """the uniform fit and the per-patch fit with P copies of (theta, sigma2), each with all of its predict calls"""
    def make():
        d, th = _data(D, shape), THETAS[fam][0]
        out = {}
        for mode in ("fit", "fit_patches"):
            m = pmk.DeviceModel(d["X_set"], d["ys"], dtype=dtype)
            if mode == "fit":
                m.fit(th, SIGMA2)
            else:
                m.fit_patches([th] * P, [SIGMA2] * P)
            assert np.all(m.info() == 0), m.info()
            out[mode] = dict(m=m, factors=[_factors(m, r) for r in range(P)], **_predict(m, d, th))
        return out
    return _cached(("run", D, fam, dtype, shape), make)


def _residual(U, c, y):
    return np.linalg.norm(U @ c - y) / (np.linalg.norm(U) * np.linalg.norm(c) + np.linalg.norm(y))


def _assert_fit(dtype, L, c, y, U, k, fo, lapack, what):
    """the bounds of tests/test_gpu_family_parity.py::test_fit_parity_matrix"""
    assert np.all(np.triu(L, 1) == 0), what
    back, res = np.linalg.norm(L @ L.T - U) / np.linalg.norm(U), _residual(U, c, y)
    if dtype == "f64":
        dL = np.abs(L - fo["L"]).max()
        dc = np.linalg.norm(c - fo["c_chol"]) / np.linalg.norm(fo["c_chol"])
        print("%s: backward %.2e residual %.2e |dL| %.2e dc %.2e" % (what, back, res, dL, dc))
        assert res <= 1e-13 and back <= 1e-14, (what, res, back)
        assert dL <= 1e-8, (what, dL)
        assert dc <= 1e-6, (what, dc)
    else:
        Lref, cref = lapack
        dL, dc = np.linalg.norm(L - Lref) / np.linalg.norm(Lref), np.linalg.norm(c - cref) / np.linalg.norm(cref)
        print("%s: backward %.1f eps residual %.1f eps dL %.3f kappa eps dc %.3f kappa eps" % (
            what, back / EPS32, res / EPS32, dL / (k * EPS32), dc / (k * EPS32)))
        assert back <= 200 * EPS32 and res <= 200 * EPS32, (what, back / EPS32, res / EPS32)
        assert dL <= 10 * k * EPS32, (what, dL / (k * EPS32))
        assert dc <= 10 * k * EPS32, (what, dc / (k * EPS32))


def _assert_items(dtype, u, v, mref, vref, mscale, vscale, k, what):
    """per-item values against queryinner! on the device's own factors: the bounds of
    tests/test_gpu_family_parity.py::test_predict_strip_parity_matrix (v is None: means only)"""
    if dtype == "f64":
        assert np.all(np.abs(u - mref) <= 1e-9 * np.maximum(1, np.abs(mref))), (what, np.abs(u - mref).max())
        assert v is None or np.all(np.abs(v - vref) <= 1e-9 + 1e-5 * vref), (what, np.abs(v - vref).max())
    else:
        assert np.all(np.abs(u - mref) <= 50 * np.sqrt(k) * EPS32 * (mscale + 1)), (what, np.abs(u - mref).max())
        assert v is None or np.all(np.abs(v - vref) <= 50 * k * EPS32 * (vscale + 1)), (what, np.abs(v - vref).max())


def _assert_mixture(dtype, Y, V, oY, oV, kmax, what):
    """mixture values against the oracle: SURVEY section 8(d) in fp64; in fp32 the bounds of
    tests/test_gpu_patches.py::test_predict_single_output_fp32_against_the_fp64_device_run (k(x, x) = 1 for both families)"""
    if dtype == "f64":
        R.assert_fp64_values(Y, V, oY, oV, what)
    else:
        print("%s: max |dY| %.2e (bound %.2e), max |dV| %.2e (bound %.2e)" % (
            what, np.abs(Y - oY).max(), 50 * kmax * EPS32 * max(1, np.abs(oY).max()), np.abs(V - oV).max(), 50 * kmax * EPS32 * 3))
        assert np.abs(Y - oY).max() <= 50 * kmax * EPS32 * max(1, np.abs(oY).max()), what
        assert np.all(np.abs(V - oV) <= 50 * kmax * EPS32 * 3), what


CASES = [(D, fam, dt, shape) for shape in SHAPES for D in DIMS for fam in THETAS for dt in DTYPES]


@pytest.mark.parametrize("D,fam,dtype,shape", CASES, ids=["%dd-%s-%s-%s" % c for c in CASES])
def test_uniform_and_per_patch_instantiations_agree_and_match_the_oracle(D, fam, dtype, shape):
    d, o, run = _data(D, shape), _oracle(D, fam, shape), _run(D, fam, dtype, shape)
    uni, pp = run["fit"], run["fit_patches"]
    # 1. fit: kmat_slab_kernel<D, FAM, false> against <D, FAM, true>
    for r in range(P):
        for name, a, b in zip(("L", "c", "Linv"), uni["factors"][r], pp["factors"][r]):
            assert np.array_equal(a, b), "patch %d: %s of fit and fit_patches differ" % (r, name)
    # 2. items: after either fit, theta by value and theta from the model; single- and multi-output
    ref = uni["theta"]
    for mode, res in (("fit", uni), ("fit_patches", pp)):
        for call in ("theta", "fitted"):
            got = res[call]
            for key in ("u", "v", "Yq", "Vq", "means", "means_v", "Ym", "Vm"):
                assert np.array_equal(got[key], ref[key]), "%s, items %s: %s differs" % (mode, call, key)
    assert np.array_equal(ref["means_v"], ref["v"]) and np.array_equal(ref["Vm"], ref["Vq"])
    # 3. the right dimension and family: the CPU oracle
    for r in range(P):
        L, c, _ = uni["factors"][r]
        _assert_fit(dtype, L, c, d["ys"][r], o["U"][r], o["kappa"][r], o["fits"][r][0], o["lapack"][r],
                    "D=%d %s %s patch %d (n = %d)" % (D, fam, dtype, r, len(c)))
    kmax = max(o["kappa"])
    _assert_mixture(dtype, ref["Yq"], ref["Vq"], o["Y"][:, 0], o["V"], kmax, "single-output")
    for j in range(RCOLS):
        _assert_mixture(dtype, ref["Ym"][:, j], ref["Vm"], o["Y"][:, j], o["V"], kmax, "multi-output column %d" % j)


MIXED = ["spline34", "spline32", "spline34", "spline32"]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", DIMS)
def test_mixed_list_takes_the_run_time_family_switch(D, dtype):
    """FAM = 0, PP = true in all three kernels.  The Spline32 patches are bit-identical to the uniform Spline32 run (the
    same compile-time family); the Spline34 patches ran another compile-time family than a uniform Spline34 fit does, so
    bits are not promised (tests/test_gpu_patches.py) and they are held to the oracle's bounds instead"""
    d = _data(D)
    m = pmk.DeviceModel(d["X_set"], d["ys"], dtype=dtype)
    m.fit_patches([THETAS[f][0] for f in MIXED], [SIGMA2] * P)
    assert np.all(m.info() == 0), m.info()
    got = _predict(m, d, None)["fitted"]
    s32 = _run(D, "spline32", dtype)["fit"]
    reg = got["dbg"]["item_region"]
    assert np.array_equal(reg, s32["theta"]["dbg"]["item_region"])
    off = got["dbg"]["item_offsets"]
    C = m.weights_multi()
    for r, fam in enumerate(MIXED):
        idx = np.nonzero(reg == r)[0]
        assert len(idx) > 0
        L, c, Ni = _factors(m, r)
        if fam == "spline32":
            for name, a, b in zip(("L", "c", "Linv"), (L, c, Ni), s32["factors"][r]):
                assert np.array_equal(a, b), "patch %d: %s differs from the uniform Spline32 fit" % (r, name)
            for key in ("u", "v", "means", "means_v"):
                assert np.array_equal(got[key][idx], s32["theta"][key][idx]), "region %d: %s" % (r, key)
            continue
        o, oth = _oracle(D, fam), THETAS[fam][1]
        what = "D=%d %s mixed patch %d" % (D, dtype, r)
        _assert_fit(dtype, L, c, d["ys"][r], o["U"][r], o["kappa"][r], o["fits"][r][0], o["lapack"][r], what)
        xq = d["Xq"][np.searchsorted(off, idx, side="right") - 1]
        mref, vref, msc, vsc = R.queryinner_reference(oth, d["X_set"][r], c, L, xq)
        _assert_items(dtype, got["u"][idx], got["v"][idx], mref, vref, msc, vsc, o["kappa"][r], what)
        assert np.array_equal(got["means_v"][idx], got["v"][idx])
        for j in range(RCOLS):
            mref, _, msc, _ = R.queryinner_reference(oth, d["X_set"][r], C[r][:, j], L, xq)
            _assert_items(dtype, got["means"][idx, j], None, mref, None, msc, None, o["kappa"][r], what + " column %d" % j)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", DIMS)
def test_explicit_theta_is_not_the_models(D, dtype):
    """pmk_query_items and pmk_model_queryinner_ex with a Spline32 theta on a model fitted with Spline34: FAM comes from
    the theta handed in, never from the model.  The same u and v from both calls, and -- because both go through the one
    launcher -- against queryinner! with the Spline32 kernel on the device's own factors"""
    import torch
    d, o = _data(D), _oracle(D, "spline34")
    m = _run(D, "spline34", dtype)["fit"]["m"]
    th, oth = THETAS["spline32"]
    xs = np.ascontiguousarray(np.tile(d["Xq"], (P, 1)))
    rg = np.repeat(np.arange(P, dtype=np.int32), NQ)
    q = pmk.DeviceQuery.from_items(m, len(rg), xs.ctypes.data, rg.ctypes.data)
    assert len(R.strip_counts(NQ)) == 2
    q.items(th)
    u = torch.empty(len(rg), dtype=torch.float64, device="cuda")
    v = torch.empty(len(rg), dtype=torch.float64, device="cuda")
    q.export_results(u.data_ptr(), v.data_ptr())
    m.ctx.synchronize()
    u, v = u.cpu().numpy(), v.cpu().numpy()
    for r in range(P):
        s = slice(r * NQ, (r + 1) * NQ)
        mu, var = m.queryinner(r, th, d["Xq"])
        assert np.array_equal(u[s], mu) and np.array_equal(v[s], var), r
        L, c, _ = _factors(m, r)
        mref, vref, msc, vsc = R.queryinner_reference(oth, d["X_set"][r], c, L, d["Xq"])
        _assert_items(dtype, mu, var, mref, vref, msc, vsc, o["kappa"][r], "D=%d %s patch %d, explicit Spline32" % (D, dtype, r))
        # and the two kernels differ by far more than any bound here: the check above can tell them apart
        m34 = R.queryinner_reference(THETAS["spline34"][1], d["X_set"][r], c, L, d["Xq"])[0]
        assert np.abs(m34 - mref).max() > 1e-3

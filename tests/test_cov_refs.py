"""CPU-side checks of the joint covariance of a query batch under the blend (no device compute).

a. tests/_cov_refs.py is pinned to the oracle on the workload of tests/test_grad_refs.py (D = 2, 4 leaves of about 40
   points, 64 queries): the diagonal of every region block equals the oracle's queryinner variance and the diagonal of the
   blend the oracle's query_mixture Vq, both within one error unit, for every stationary family.
b. For a tree of one leaf the blend equals the textbook K** - K*^T (K + sigma2 I)^-1 K*, computed by an independent route
   (scipy.linalg.cho_solve, no triangular V), within one unit.
c. The blended matrix is symmetric and its smallest eigenvalue is >= -(the largest sum of a row's units): |E|_2 <= |E|_inf
   for the symmetric error E of a positive semi-definite matrix.
d. Entries of queries that share no region are exact zeros.
e. On the inputs of tests/test_gpu_cov.py a plain numpy / LAPACK evaluation in the model's own precision stays below one
   unit, and kappa2(L) <= 10^3 for every patch: the GPU bound of 10 units has a checked margin.
f. The six symbols are in the header, the ctypes table, the library, the host-only stubs and the Julia ccalls;
   pmk_version() is 103; every refusal that needs no device returns its code; the Python front end refuses
   closure-carrying kernels before any device call.  These are the tests that fail without the feature.
"""
import ctypes as C
import re

import numpy as np
import pytest
import scipy.linalg as sla

import patchmixturekriging_amd as pmk
from patchmixturekriging_amd import _lib
from patchmixturekriging_amd import mixture as M
from oracle import oracle as O
from test_julia_binding import header_prototypes, julia_ccalls
from test_multi_output_abi import _cat, _NoDevice
from test_grad_refs import DELTA, FAMILIES, RADIUS, SIGMA2, U53, Workload
import _cov_cases as CC
import _cov_refs as CR

NEW = ["pmk_query_items_cov", "pmk_query_mix_cov", "pmk_query_fetch_cov", "pmk_query_fetch_cov_dev",
       "pmk_query_get_items_cov", "pmk_predict_mixture_cov_fitted"]


@pytest.fixture(scope="module")
def wl():
    return Workload()


def _items_of(wl):
    """(item_offsets, item_region, item_t) of the workload's queries from the oracle's plan"""
    off, reg, t = [0], [], []
    for x in wl.Xq:
        home, nb, _, ts = wl.signature(x)
        reg += list(nb) + [home]
        t += [float(v) for v in ts] + [0.0]
        off.append(len(reg))
    return np.array(off, dtype=np.int64), np.array(reg, dtype=np.int64), np.array(t)


def _reference(th, Xs, sigma2, items, Xq, wth, u=U53):
    """blocks, their units with the factor (n + 32) u, and the blend of the reference"""
    S_blocks, units, refs = {}, {}, {}
    for r, (idx, pts) in CC.blocks_of(items, Xq).items():
        refs[r] = CR.RegionRef(th, Xs[r], sigma2)
        out = refs[r].cov(pts)
        S_blocks[r] = (idx, out["S"])
        units[r] = (len(Xs[r]) + 32) * u * out["unit"]
    Cov, unit = CR.mix_cov_ref(items[:2], S_blocks, items[2], wth, units)
    return S_blocks, units, refs, Cov, unit


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_the_restatement_is_pinned_to_the_oracle(wl, family):
    th = FAMILIES[family]
    items = _items_of(wl)
    S_blocks, units, _, Cov, unit = _reference(th, wl.Xs, SIGMA2, items, wl.Xq, wl.wth)
    fits = [O.fit_patch(th, X, Y[:, 0], SIGMA2) for X, Y in zip(wl.Xs, wl.Ys)]
    worst = 0.0
    for r, (idx, S) in S_blocks.items():
        v = np.array([O.queryinner(th, wl.Xs[r], fits[r]["c_chol"], fits[r]["L"], wl.Xq[j])[1] for j in idx])
        ratio = np.abs(v - np.diag(S)).astype(np.float64) / np.diag(units[r])
        worst = max(worst, float(ratio.max()))
    _, Vq = O.query_mixture(wl.ob, th, wl.wth, wl.Xs, [f["c_chol"] for f in fits], [f["L"] for f in fits], wl.Xq, RADIUS, DELTA)
    worst_blend = float((np.abs(Vq - np.diag(Cov)).astype(np.float64) / np.diag(unit)).max())
    print("COVREF family=%s worst err/unit block diagonal=%.3g blend diagonal=%.3g" % (family, worst, worst_blend))
    assert worst <= 1.0 and worst_blend <= 1.0, (worst, worst_blend)
    # the single-block entry point is the same computation
    r, (idx, S) = next(iter(S_blocks.items()))
    assert np.array_equal(CR.region_cov_ref(th, wl.Xs[r], SIGMA2, wl.Xq[idx]), S)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_one_leaf_is_the_textbook_posterior_covariance(wl, family):
    th = FAMILIES[family]
    # a tree of one leaf has no hyperplane: every query has its home item alone, with weight 1
    Nq = len(wl.Xq)
    items = (np.arange(Nq + 1, dtype=np.int64), np.zeros(Nq, dtype=np.int64), np.zeros(Nq))
    _, _, _, Cov, unit = _reference(th, [wl.X], SIGMA2, items, wl.Xq, wl.wth)
    U = O.kernel_matrix(th, wl.X) + SIGMA2 * np.eye(len(wl.X))
    Ks = O.cross_kernel_matrix(th, wl.X, wl.Xq)
    if Ks.shape[0] != len(wl.X):
        Ks = Ks.T
    text = O.kernel_matrix(th, wl.Xq) - Ks.T @ sla.cho_solve(sla.cho_factor(U, lower=True), Ks)
    ratio = np.abs(text - Cov).astype(np.float64) / unit
    print("COVREF family=%s one leaf: worst err/unit against cho_solve=%.3g" % (family, ratio.max()))
    assert ratio.max() <= 1.0, ratio.max()


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_symmetric_nearly_positive_and_zero_without_a_shared_region(wl, family):
    items = _items_of(wl)
    _, _, _, Cov, unit = _reference(FAMILIES[family], wl.Xs, SIGMA2, items, wl.Xq, wl.wth)
    assert np.array_equal(Cov, Cov.T)
    lam = np.linalg.eigvalsh(np.asarray(Cov, dtype=np.float64))
    assert lam[0] >= -unit.sum(1).max(), (lam[0], unit.sum(1).max())
    shared = CR.shared_region_mask(items[:2])
    assert shared.any() and not shared.all() and np.all(np.diag(shared))
    assert np.all(Cov[~shared] == 0) and np.all(unit[~shared] == 0)
    assert np.count_nonzero(Cov[shared]) > 0.9 * shared.sum()


# ------------------------------------------------------------------------------------------ the unit on the GPU tests' inputs
def _plain_worst(oth, Xs, sigma2, blocks, dtype):
    T_, u = (np.float32, 2.0 ** -24) if dtype == "f32" else (np.float64, U53)
    worst = kappa = 0.0
    for r, (idx, pts) in blocks.items():
        ref = CR.RegionRef(oth[r] if isinstance(oth, list) else oth, Xs[r], sigma2)
        kappa = max(kappa, ref.kappa)
        out = ref.cov(pts)
        plain = CR.plain_region_cov(ref.th, Xs[r], sigma2, pts, T_)
        err = np.abs(plain - out["S"]).astype(np.float64)
        worst = max(worst, float((err / ((len(Xs[r]) + 32) * u * out["unit"])).max()))
    return worst, kappa


@pytest.mark.parametrize("family,dtype", [("spline34", "f64"), ("gaussian", "f64"), ("spline34", "f32")])
def test_a_plain_evaluation_stays_below_one_unit_on_the_main_workload(family, dtype):
    m = CC.Main(dtype)
    items = m.oracle_items()
    counts = np.bincount(items[1], minlength=4)
    assert counts.max() > 2 * CC.TQ and counts.min() < CC.TQ and 1 <= np.diff(items[0]).min() and np.diff(items[0]).max() <= 3
    assert all(256 < len(x) <= 300 and len(x) % 128 for x in m.Xs)
    worst, kappa = _plain_worst(CC.FAMILIES[family][1], m.Xs, CC.SIGMA2[dtype], CC.blocks_of(items, m.Xq), dtype)
    print("COVUNIT main family=%s dtype=%s plain worst err/unit=%.3g kappa2(L)=%.3g" % (family, dtype, worst, kappa))
    assert worst < 1.0 and kappa <= CC.KAPPA_MAX, (worst, kappa)


@pytest.mark.parametrize("D,dtype,mixed", [(2, "f64", False), (2, "f32", False), (3, "f64", False), (2, "f64", True), (2, "f32", True)])
def test_a_plain_evaluation_stays_below_one_unit_on_the_edge_inputs(D, dtype, mixed):
    Xs = CC.edge_patches(D, dtype)
    xq, region = CC.edge_items(Xs, CC.EDGE_COUNTS, dtype)
    blocks = {r: (np.nonzero(region == r)[0], xq[region == r]) for r in sorted(set(int(v) for v in region))}
    oth = [CC.FAMILIES[n][1] for n in CC.MIXED_NAMES] if mixed else CC.FAMILIES["spline34"][1]
    worst, kappa = _plain_worst(oth, Xs, CC.SIGMA2[dtype], blocks, dtype)
    print("COVUNIT edges D=%d dtype=%s mixed=%s plain worst err/unit=%.3g kappa2(L)=%.3g" % (D, dtype, mixed, worst, kappa))
    assert worst < 1.0 and kappa <= CC.KAPPA_MAX, (worst, kappa)


def test_a_plain_evaluation_stays_below_one_unit_on_the_many_leaves_workload():
    mm = CC.Many()
    items = CC.oracle_items(mm)
    assert len(mm.Xs) == 512 and len(set(int(r) for r in items[1])) > 304
    blocks = CC.blocks_of(items, mm.Xq)
    # the workload holds the case of a query with two items of one region, and the blend of the reference counts every pair
    twice = [r for r, (idx, _) in blocks.items() if np.any(np.diff(idx) == 0)]
    assert twice, "no query holds two items of one region"
    worst, kappa = _plain_worst(CC.FAMILIES["spline34"][1], mm.Xs, CC.SIGMA2["f64"], blocks, "f64")
    print("COVUNIT many plain worst err/unit=%.3g kappa2(L)=%.3g regions with a doubled query=%s" % (worst, kappa, twice))
    assert worst < 1.0 and kappa <= CC.KAPPA_MAX, (worst, kappa)
    th = CC.FAMILIES["spline34"][1]
    S_blocks, _, _, Cov, unit = _reference(th, mm.Xs, CC.SIGMA2["f64"], items, mm.Xq, mm.owth)
    r = twice[0]
    idx, S = S_blocks[r]
    a = int(np.nonzero(np.diff(idx) == 0)[0][0])
    j = int(idx[a])
    wn = CR.blend_weights(items[0], items[2], mm.owth)
    its = [i for i in range(items[0][j], items[0][j + 1]) if items[1][i] == r]
    assert len(its) == 2
    single = sum(float(wn[i]) ** 2 * float(CR.RegionRef(th, mm.Xs[int(items[1][i])], CC.SIGMA2["f64"]).cov(mm.Xq[j:j + 1])["S"][0, 0])
                 for i in range(items[0][j], items[0][j + 1]))
    cross = 2.0 * float(wn[its[0]] * wn[its[1]] * S[a, a + 1])
    assert abs(float(Cov[j, j]) - (single + cross)) <= 1e-14 * abs(single) and cross > 0
    assert np.array_equal(Cov, Cov.T) and np.linalg.eigvalsh(np.asarray(Cov, dtype=np.float64))[0] >= -unit.sum(1).max()


def test_a_plain_evaluation_stays_below_one_unit_on_the_brownian_bridge_inputs():
    Xs = CC.bb_patches()
    xq, region = CC.bb_items()
    blocks = {r: (np.nonzero(region == r)[0], xq[region == r]) for r in sorted(set(int(v) for v in region))}
    worst, kappa = _plain_worst(CC.FAMILIES["bb10"][1], Xs, CC.SIGMA2["f64"], blocks, "f64")
    print("COVUNIT bb10 plain worst err/unit=%.3g kappa2(L)=%.3g" % (worst, kappa))
    assert worst < 1.0 and kappa <= CC.KAPPA_MAX, (worst, kappa)
    # the restated bridge is the oracle's kernel
    oth = CC.FAMILIES["bb10"][1]
    assert np.allclose(CR.kern(oth, Xs[0], xq[:5]), O.cross_kernel_matrix(oth, xq[:5], Xs[0]).T.reshape(len(Xs[0]), 5), rtol=1e-14, atol=0)


# ------------------------------------------------------------------------------------------ the ABI (fails without the feature)
def _header():
    return open(_lib.os.path.join(_lib._HERE, "..", "include", "pmk.h")).read()


def test_header_and_signatures_agree():
    protos = header_prototypes()
    L = pmk.lib()
    for name in NEW:
        assert name in protos, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(L, name), name
        res, args = _lib.SIGNATURES[name]
        cret, cargs = protos[name]
        assert [_cat(a) for a in args] == cargs, name
        assert _cat(res) == cret, name
    assert L.pmk_version() == 103
    assert '"items_cov", "mix_cov"' in _header()
    assert "#define PMK_COV_MAX_QUERIES 16384" in _header()
    flat = re.sub(r"[\s*]+", " ", _header())
    assert "k_r(x_j, x_j') - V_{r,j} . V_{r,j'}" in flat and "Out of scope: a trend's term z . z'" in flat


def test_stub_launchers_and_julia_ccalls():
    stubs = open(_lib.os.path.join(_lib.CSRC, "pmk_nogpu_stubs.cpp")).read()
    for name in ("launch_items_cov", "launch_mix_cov"):
        assert name in stubs, name
    protos = header_prototypes()
    seen = set()
    for name, ret, args, line in julia_ccalls():
        if name in NEW:
            assert (ret, args) == protos[name], (name, line)
            seen.add(name)
    assert seen == set(NEW), set(NEW) - seen
    jl = open(_lib.os.path.join(_lib._HERE, "..", "julia", "PatchMixtureKriging", "src", "PatchMixtureKriging.jl"), encoding="utf-8").read()
    assert "function querymixtureGP_cov(" in jl and re.search(r"^export(?:.|\n)*?querymixtureGP_cov", jl, flags=re.M)


def test_argument_checks_need_no_device():
    L = pmk.lib()
    m, idx = C.c_int64(), (C.c_int32 * 1)()
    calls = {"pmk_query_items_cov": (lambda: L.pmk_query_items_cov(None, None), -1),
             "pmk_query_mix_cov": (lambda: L.pmk_query_mix_cov(None, None), -1),
             "pmk_query_fetch_cov": (lambda: L.pmk_query_fetch_cov(None, None, 0), -1),
             "pmk_query_fetch_cov_dev": (lambda: L.pmk_query_fetch_cov_dev(None, None, 0), -1),
             "pmk_query_get_items_cov": (lambda: L.pmk_query_get_items_cov(None, 0, C.byref(m), idx, None, 0), -1),
             "pmk_predict_mixture_cov_fitted": (lambda: L.pmk_predict_mixture_cov_fitted(None, None, 0, None, 0.0, 0.0, None, None,
                                                                                          None, 0), -1)}
    assert sorted(calls) == sorted(NEW)
    for name, (call, code) in calls.items():
        assert call() == code, name
        assert name.encode() in L.pmk_last_error(), name


def test_python_refuses_closure_kernels_before_any_device_call(monkeypatch):
    DQ = M.DeviceQuery

    def no_device(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(M, "DeviceQuery", no_device)

    class Warped:
        warped = True

    class WithDiag:
        def diag_addend(self, X):
            return np.zeros(len(X))

    class Fitted:
        """an eta whose model was fitted with a closure-carrying kernel"""
        def __init__(self, theta):
            self._model = type("Model", (), {"theta": theta, "_has_kernels": True})()

    ok = pmk.Spline34KernelType(1.0)
    Xq = np.zeros((3, 2))
    for th in (Warped(), WithDiag()):
        with pytest.raises(TypeError, match="closure-carrying"):
            pmk.querymixtureGP_cov(Xq, _NoDevice([5, 7]), None, 2, 1.0, 1e-5, th)
        with pytest.raises(TypeError, match="closure-carrying"):
            pmk.samplemixtureGP(Xq, _NoDevice([5, 7]), None, 2, 1.0, 1e-5, th, 4)
        with pytest.raises(TypeError, match="closure-carrying"):
            pmk.querymixtureGP_cov(Xq, Fitted(th), None, 2, 1.0, 1e-5, ok)
    # without a fit the front end says so, still before any device call
    with pytest.raises(_lib.PmkError, match="must run before querymixtureGP_cov"):
        pmk.querymixtureGP_cov(Xq, _NoDevice([5, 7]), None, 2, 1.0, 1e-5, ok)

    # the staged methods check their kernel before the library is asked
    class Handle:
        h, model, Nq = None, None, 0

        class L:
            def __getattr__(self, name):
                raise AssertionError("a library call was made: " + name)
        L = L()

    for th in (Warped(), WithDiag()):
        with pytest.raises(TypeError):
            DQ.items_cov(Handle(), th)
        with pytest.raises(TypeError):
            DQ.mix_cov(Handle(), th)
    with pytest.raises(_lib.PmkError, match="holds no kernels"):
        DQ.items_cov(Handle())


def test_exports_and_docs_name_the_feature():
    for name in ("querymixtureGP_cov", "samplemixtureGP"):
        assert hasattr(pmk, name), name
    for name in ("items_cov", "mix_cov", "fetch_cov", "fetch_cov_into", "item_covs"):
        assert hasattr(M.DeviceQuery, name), name
    root = _lib.os.path.join(_lib._HERE, "..")
    for doc, word in (("DESIGN.md", "pmk_cov.hip"), ("README.md", "querymixtureGP_cov"), ("README.md", "samplemixtureGP"),
                      ("INTEGRATION.md", "pmk_predict_mixture_cov_fitted")):
        assert word in open(_lib.os.path.join(root, doc), encoding="utf-8").read(), (doc, word)

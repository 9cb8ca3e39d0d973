"""CPU-side checks of the joint covariance on the multi-output path, under a trend (no device compute).

a. tests/_cov_multi_refs.py is pinned two ways on the workload of tests/test_grad_refs.py (D = 2, 4 leaves of about 40
   points, 64 queries) for a constant and a linear trend: every region block equals the dense saddle-point form
   k_ab - [k_a; h_a]^T [[U, H], [H^T, 0]]^-1 [k_b; h_b], built from the oracle's kernel matrices and solved by Gaussian
   elimination in long double, and its diagonal equals the universal-kriging variance of _trend_refs.predict_reference,
   both within one error unit.  Without a trend the restatement is that of _cov_refs.py bit for bit.
b. On the very inputs of tests/test_gpu_cov_multi.py (tests/_cov_multi_cases.py, and the many-leaves workload of
   tests/_cov_cases.py) a plain numpy / LAPACK evaluation in the model's own precision stays below one unit and
   kappa2(L) <= 10^3 for every patch; kappa2(L_G) is printed.  The GPU bound of 10 units has a checked margin.
c. The two symbols are in the header, the ctypes table, the library, the host-only stubs and the Julia ccalls;
   pmk_version() is 103; the refusals that need no device return their code; the Python front ends exist and refuse
   closure-carrying kernels before any device call.  These are the tests that fail without the feature.
"""
import re

import numpy as np
import pytest

import patchmixturekriging_amd as pmk
from patchmixturekriging_amd import _lib
from patchmixturekriging_amd import mixture as M
from oracle import oracle as O
from test_julia_binding import header_prototypes, julia_ccalls
from test_multi_output_abi import _cat, _NoDevice
from test_grad_refs import FAMILIES, SIGMA2, U53, Workload
from test_cov_refs import _items_of
import _cov_cases as CC
import _cov_multi_cases as CMC
import _cov_multi_refs as CMR
import _cov_refs as CR
import _trend_refs as TR

NEW = ["pmk_query_items_cov_multi", "pmk_predict_mixture_cov_multi_fitted"]


@pytest.fixture(scope="module")
def wl():
    return Workload()


def _cross(th, X, Xq):
    Ks = O.cross_kernel_matrix(th, X, Xq)
    return Ks if Ks.shape[0] == len(X) and Ks.shape[1] == len(Xq) else Ks.T


# ------------------------------------------------------------------------------------------ a. the restatement is pinned
@pytest.mark.parametrize("trend", CMC.TRENDS)
@pytest.mark.parametrize("family", ["spline34", "gaussian", "rq"])
def test_the_restatement_is_pinned_to_the_saddle_point_form_and_to_the_trend_reference(wl, family, trend):
    th = FAMILIES[family]
    items = _items_of(wl)
    worst = worst_diag = 0.0
    for r, (idx, pts) in CC.blocks_of(items, wl.Xq).items():
        X = wl.Xs[r]
        ref = CMR.TrendRegionRef(th, X, SIGMA2, trend)
        out = ref.cov(pts)
        assert not out["clamped"].any()
        unit = (len(X) + 32) * U53 * out["unit"]
        K, Kq, Kqq = O.kernel_matrix(th, X), _cross(th, X, pts), O.kernel_matrix(th, pts)
        H, Hq = TR.basis(X, trend), TR.basis(pts, trend)
        dense = CMR.kkt_cov(K, SIGMA2, H, Kq, Kqq, Hq)
        worst = max(worst, float((np.abs(dense - out["S"]).astype(np.float64) / unit).max()))
        assert np.array_equal(out["S"], out["S"].T)
        tref = TR.trend_reference(K, SIGMA2, wl.Ys[r], H)
        _, v = TR.predict_reference(tref, Kq.T, np.diag(Kqq), Hq)
        worst_diag = max(worst_diag, float((np.abs(v - np.diag(out["S"])).astype(np.float64) / np.diag(unit)).max()))
        # the trend's term is positive semi-definite: the block dominates the simple-kriging one on the diagonal
        plain = CR.RegionRef(th, X, SIGMA2).cov(pts)
        assert np.all(np.diag(out["S"]) >= np.diag(plain["S"])) and np.all(out["unit"] >= plain["unit"])
    print("COVMREF family=%s trend=%s worst err/unit against the saddle-point form=%.3g, diagonal against "
          "predict_reference=%.3g" % (family, trend, worst, worst_diag))
    assert worst <= 1.0 and worst_diag <= 1.0, (worst, worst_diag)


def test_without_a_trend_the_restatement_is_that_of_the_single_output_path(wl):
    th = FAMILIES["spline34"]
    idx, pts = CC.blocks_of(_items_of(wl), wl.Xq)[0]
    a, b = CMR.TrendRegionRef(th, wl.Xs[0], SIGMA2, None).cov(pts), CR.RegionRef(th, wl.Xs[0], SIGMA2).cov(pts)
    assert np.array_equal(a["S"], b["S"]) and np.array_equal(a["unit"], b["unit"])


def test_the_clamp_comes_before_the_trend_term():
    th = FAMILIES["spline34"]
    X = np.random.default_rng(3).uniform(-1, 1, (12, 2))
    ref = CMR.TrendRegionRef(th, X, 1e-9, "linear")
    pts = np.vstack([X[:3], [[0.3, 0.2]]])
    out = ref.cov(pts, min_v=1e-3)
    assert out["clamped"][:3].all() and not out["clamped"][3]
    z2 = np.asarray((out["Z"] * out["Z"]).sum(0))
    assert np.all(np.abs(np.diag(out["S"])[:3] - (CR.LD(1e-3) + z2[:3])) <= 1e-18)


def test_the_gaussian_elimination_solves():
    rng = np.random.default_rng(5)
    A, B = rng.normal(size=(9, 9)), rng.normal(size=(9, 3))
    A[0, 0] = 0.0                                               # a pivot search is needed
    assert np.allclose(np.asarray(CMR.solve_ld(A, B), dtype=np.float64), np.linalg.solve(A, B), rtol=1e-10, atol=1e-12)


# ------------------------------------------------------------------------------------------ b. the unit on the GPU tests' inputs
def _plain_worst(oth, Xs, sigma2, blocks, dtype, trend, skip=()):
    T_, u = (np.float32, 2.0 ** -24) if dtype == "f32" else (np.float64, U53)
    worst = kappa = kappa_G = 0.0
    for r, (idx, pts) in blocks.items():
        if r in skip:
            continue
        ref = CMR.TrendRegionRef(oth[r] if isinstance(oth, list) else oth, Xs[r], sigma2, trend)
        kappa, kappa_G = max(kappa, ref.kappa), max(kappa_G, ref.kappa_G)
        out = ref.cov(pts)
        assert not out["clamped"].any(), r
        plain = CMR.plain_region_cov(ref.th, Xs[r], sigma2, pts, T_, trend)
        err = np.abs(plain - out["S"]).astype(np.float64)
        worst = max(worst, float((err / ((len(Xs[r]) + 32) * u * out["unit"])).max()))
    return worst, kappa, kappa_G


@pytest.mark.parametrize("trend", CMC.TRENDS)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_a_plain_evaluation_stays_below_one_unit_on_the_main_workload(dtype, trend):
    m = CMC.Main(dtype)
    items = m.oracle_items()
    counts = np.bincount(items[1], minlength=4)
    assert CC.TQ < counts.max() <= 2 * CC.TQ and 0 < counts.min() < CC.TQ, counts
    assert 1 <= np.diff(items[0]).min() and np.diff(items[0]).max() <= 3 and (np.diff(items[0]) > 1).sum() > 50
    assert all(128 < len(x) <= 256 for x in m.Xs), [len(x) for x in m.Xs]
    worst, kappa, kappa_G = _plain_worst(CC.FAMILIES["spline34"][1], m.Xs, CC.SIGMA2[dtype], CC.blocks_of(items, m.Xq), dtype, trend)
    print("COVMUNIT main dtype=%s trend=%s plain worst err/unit=%.3g kappa2(L)=%.3g kappa2(L_G)=%.3g" % (dtype, trend, worst, kappa, kappa_G))
    assert worst < 1.0 and kappa <= CC.KAPPA_MAX, (worst, kappa)


@pytest.mark.parametrize("D,trend,dtype,mixed", [(2, "constant", "f64", False), (1, "linear", "f64", False), (2, "linear", "f64", False),
                                                 (4, "linear", "f64", False), (2, "linear", "f32", False), (2, "linear", "f64", True)])
def test_a_plain_evaluation_stays_below_one_unit_on_the_edge_inputs(D, trend, dtype, mixed):
    Xs = CMC.edge_patches(D, trend, dtype)
    xq, region = CMC.edge_items(Xs, dtype)
    q = CMC.Q_OF[trend](D)
    assert len(Xs[0]) == q and [len(x) for x in Xs] == CMC.edge_sizes(q)
    blocks = {r: (np.nonzero(region == r)[0], xq[region == r]) for r in sorted(set(int(v) for v in region))}
    assert [len(blocks[r][0]) if r in blocks else 0 for r in range(8)] == CMC.EDGE_COUNTS
    oth = [CC.FAMILIES[n][1] for n in CC.MIXED_NAMES] if mixed else CC.FAMILIES["spline34"][1]
    worst, kappa, kappa_G = _plain_worst(oth, Xs, CC.SIGMA2[dtype], blocks, dtype, trend, skip=CMC.flagged(D, trend))
    print("COVMUNIT edges D=%d trend=%s dtype=%s mixed=%s plain worst err/unit=%.3g kappa2(L)=%.3g kappa2(L_G)=%.3g"
          % (D, trend, dtype, mixed, worst, kappa, kappa_G))
    assert worst < 1.0 and kappa <= CC.KAPPA_MAX, (worst, kappa)


def test_a_plain_evaluation_stays_below_one_unit_on_the_many_leaves_workload():
    mm = CC.Many()
    items = CC.oracle_items(mm)
    blocks = CC.blocks_of(items, mm.Xq)
    assert [r for r, (idx, _) in blocks.items() if np.any(np.diff(idx) == 0)], "no query holds two items of one region"
    worst, kappa, kappa_G = _plain_worst(CC.FAMILIES["spline34"][1], mm.Xs, CC.SIGMA2["f64"], blocks, "f64", "constant")
    print("COVMUNIT many trend=constant plain worst err/unit=%.3g kappa2(L)=%.3g kappa2(L_G)=%.3g" % (worst, kappa, kappa_G))
    assert worst < 1.0 and kappa <= CC.KAPPA_MAX, (worst, kappa)


# ------------------------------------------------------------------------------------------ c. the ABI (fails without the feature)
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
    assert '"cov_trend"' in _header()
    flat = re.sub(r"[\s*]+", " ", _header())
    assert "S_r[a, b] = k_r(x_a, x_b) - V_a . V_b + z_a . z_b" in flat


def test_stub_launchers_makefile_and_julia_ccalls():
    stubs = open(_lib.os.path.join(_lib.CSRC, "pmk_nogpu_stubs.cpp")).read()
    assert "launch_cov_trend" in stubs
    mk = open(_lib.os.path.join(_lib.CSRC, "Makefile")).read()
    assert mk.count("pmk_cov_trend.o") == 2                     # the library and its A/B variant
    protos = header_prototypes()
    seen = set()
    for name, ret, args, line in julia_ccalls():
        if name in NEW:
            assert (ret, args) == protos[name], (name, line)
            seen.add(name)
    assert seen == set(NEW), set(NEW) - seen
    jl = open(_lib.os.path.join(_lib._HERE, "..", "julia", "PatchMixtureKriging", "src", "PatchMixtureKriging.jl"), encoding="utf-8").read()
    assert "function querymixtureGP_cov_multi(" in jl and re.search(r"^export(?:.|\n)*?querymixtureGP_cov_multi", jl, flags=re.M)


def test_argument_checks_need_no_device():
    L = pmk.lib()
    calls = {"pmk_query_items_cov_multi": (lambda: L.pmk_query_items_cov_multi(None, None), -1),
             "pmk_predict_mixture_cov_multi_fitted": (lambda: L.pmk_predict_mixture_cov_multi_fitted(
                 None, None, 0, None, 0.0, 0.0, None, 0, None, None, 0), -1)}
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
            pmk.querymixtureGP_cov_multi(Xq, _NoDevice([5, 7]), None, 2, 1.0, 1e-5, th)
        with pytest.raises(TypeError, match="closure-carrying"):
            pmk.samplemixtureGP_multi(Xq, _NoDevice([5, 7]), None, 2, 1.0, 1e-5, th, 4)
        with pytest.raises(TypeError, match="closure-carrying"):
            pmk.querymixtureGP_cov_multi(Xq, Fitted(th), None, 2, 1.0, 1e-5, ok)
    with pytest.raises(_lib.PmkError, match="must run before querymixtureGP_cov_multi"):
        pmk.querymixtureGP_cov_multi(Xq, _NoDevice([5, 7]), None, 2, 1.0, 1e-5, ok)

    class Handle:
        h, model, Nq = None, None, 0

        class L:
            def __getattr__(self, name):
                raise AssertionError("a library call was made: " + name)
        L = L()

    for th in (Warped(), WithDiag()):
        with pytest.raises(TypeError):
            DQ.items_cov_multi(Handle(), th)
    with pytest.raises(_lib.PmkError, match="holds no kernels"):
        DQ.items_cov_multi(Handle())


def test_exports_and_docs_name_the_feature():
    for name in ("querymixtureGP_cov_multi", "samplemixtureGP_multi"):
        assert hasattr(pmk, name), name
    assert hasattr(M.DeviceQuery, "items_cov_multi")
    root = _lib.os.path.join(_lib._HERE, "..")
    for doc, word in (("DESIGN.md", "pmk_cov_trend.hip"), ("README.md", "querymixtureGP_cov_multi"), ("README.md", "samplemixtureGP_multi"),
                      ("README.md", "test_gpu_cov_multi.py"), ("INTEGRATION.md", "pmk_predict_mixture_cov_multi_fitted")):
        assert word in open(_lib.os.path.join(root, doc), encoding="utf-8").read(), (doc, word)

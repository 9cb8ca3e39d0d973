"""The geometry side on gridded, collinear and duplicated points (tests/_degenerate.py): the device tree build, the device
eps-assignment, from_tree and its gather kernels, the query plan and every site that evaluates a compactly supported
kernel, on inputs where projections EQUAL hyperplane offsets, projections tie (-0.0 and +0.0 included), leaves are empty,
and pairs of points sit exactly ON the kernel's support radius.

References: the host build and assignment (pinned bit for bit by the oracle on the same inputs in
tests/test_oracle_bsp.py), the list route of the model constructors, the CPU oracle, and integer arithmetic on lattice
steps for the kernels' zero pattern.  Integer outputs, hyperplanes and everything that two routes compute with the same
kernels are compared on their raw bits.  Every test prints the number of edge cases it reached under -s and asserts that
it reached some."""
import ctypes as C

import numpy as np
import pytest

import patchmixturekriging_amd as pmk
from patchmixturekriging_amd import _lib
from patchmixturekriging_amd import mixture as M
from patchmixturekriging_amd import partition as PT
from oracle import oracle as O

import _degenerate as G
import _query_refs as R
from test_gpu_device_setup import _compare_fits, _compare_packed, _host_model, _packed, _sets, same_bits

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
A = 0.8                                                   # support 1 / a = 1.25 = 5 lattice steps
S34, OS34 = pmk.Spline34KernelType(A), O.kernel(O.SPLINE34, A)
SIGMA2 = 1e-3
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int64)


def ulps(a, b):
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


def _targets(X):
    return np.sin(0.7 * X[:, 0] + 0.2) * np.cos(0.3 * X[:, -1]) + 0.05 * X[:, 0]


def _tree_arrays(root, inds):
    v, c = PT.hyperplane_arrays(root)
    return v, c, np.cumsum([0] + [len(i) for i in inds]), np.concatenate(inds)


# ------------------------------------------------------------------------------------ 1. the device tree build
@pytest.mark.parametrize("name", list(G.BUILDS))
def test_device_build_on_degenerate_points(name):
    X, levels = G.BUILDS[name]
    for sign_mode, dot_mode in G.MODES:
        rh, _, Ih = pmk.setuppartition(X, levels, sign_mode=sign_mode, dot_mode=dot_mode)
        rd, _, Id = pmk.setuppartition(X, levels, sign_mode=sign_mode, dot_mode=dot_mode, device=True)
        (hv, hc, hoff, hi), (dv, dc, doff, di) = _tree_arrays(rh, Ih), _tree_arrays(rd, Id)
        assert np.array_equal(G.bits(hv), G.bits(dv)), (name, sign_mode, dot_mode)
        assert np.array_equal(hc, dc), (name, sign_mode, dot_mode, hc, dc)
        assert np.array_equal(np.signbit(hc), np.signbit(dc)), (name, sign_mode, dot_mode, hc, dc)
        assert np.array_equal(G.bits(hc), G.bits(dc))
        assert np.array_equal(hoff, doff) and np.array_equal(hi, di), (name, sign_mode, dot_mode)
        E = G.projections(hv, hc, X, dot_mode)
        print("%s (%d, %d): identical; %d (point, plane) pairs with e == c, %d zero offsets, %d empty leaves"
              % (name, sign_mode, dot_mode, int((E == hc[:, None]).sum()), int((hc == 0).sum()),
                 int((np.diff(hoff) == 0).sum())))
        assert np.any(E == hc[:, None])
        if name == "dups5":
            assert np.array_equal(np.diff(doff), [0, 100, 0, 100, 0, 100, 100, 100])


def test_device_build_refusals_match_the_host_and_leave_the_context_usable():
    for name, (X, levels, status, text, _, _) in G.REFUSED.items():
        for sign_mode, dot_mode in G.MODES:
            msgs = []
            for device in (False, True):
                with pytest.raises(pmk.PmkError) as err:
                    pmk.setuppartition(X, levels, sign_mode=sign_mode, dot_mode=dot_mode, device=device)
                msgs.append(str(err.value).replace("pmk_bsp_build_device", "pmk_bsp_build"))
            assert msgs[0] == msgs[1] and "(%d): " % status in msgs[1] and text in msgs[1], msgs
        print("%s: host and device refuse with %s" % (name, msgs[1]))
        X, levels = G.BUILDS["lattice33x31"]                # and the context builds the next tree
        rh, _, Ih = pmk.setuppartition(X, levels)
        rd, _, Id = pmk.setuppartition(X, levels, device=True)
        for a, b in zip(_tree_arrays(rh, Ih), _tree_arrays(rd, Id)):
            assert same_bits(a, b)


# ------------------------------------------------------------------------------------ 2. the device eps-assignment
@pytest.mark.parametrize("name", list(G.BUILDS))
def test_device_eps_assignment_on_degenerate_points(name):
    X, levels = G.BUILDS[name]
    N = len(X)
    for sign_mode, dot_mode in G.MODES:
        root, _, _ = pmk.setuppartition(X, levels, sign_mode=sign_mode, dot_mode=dot_mode)
        hv, hc = PT.hyperplane_arrays(root)
        E = G.projections(hv, hc, X, dot_mode)
        P = len(hc) + 1
        for eps in G.eps_list(name):
            Xh, Ih, Lh, _ = pmk.organizetrainingsets(root, levels, X, eps)
            Xd, Id, Ld, _ = pmk.organizetrainingsets(root, levels, X, eps, device=True)
            what = (name, sign_mode, dot_mode, eps)
            assert len(Ih) == len(Id) == P and len(Lh) == len(Ld) == N
            assert np.array_equal([len(i) for i in Ih], [len(i) for i in Id]), what
            assert np.array_equal(np.concatenate(Ih), np.concatenate(Id)), what
            assert np.array_equal([len(l) for l in Lh], [len(l) for l in Ld]), what
            assert np.array_equal(np.concatenate(Lh), np.concatenate(Ld)), what
            for a, b in zip(Xh, Xd):
                assert np.array_equal(G.bits(a), G.bits(b)), what
            per_point = np.array([len(l) for l in Ld])
            total, nowhere, everywhere = int(per_point.sum()), int((per_point == 0).sum()), int((per_point == P).sum())
            with np.errstate(invalid="ignore"):
                on_band = int(((E == (hc + eps)[:, None]) | (E == (hc - eps)[:, None])).sum())
            print("%s (%d, %d) eps=%r: identical; %d pairs, %d points in no leaf, %d in every leaf, %d empty sets, %d "
                  "(point, plane) pairs with e == c +- eps" % (what + (total, nowhere, everywhere,
                                                                sum(len(i) == 0 for i in Id), on_band)))
            if eps == 0.0:
                assert 0 < nowhere and total == N - nowhere < N
            if np.isnan(eps):
                assert total == 0
            if eps == float("inf"):
                assert total == N * P
            if name == "pm0_1d" and eps in (0.5, 1.0):
                assert on_band > 0
                for n in np.nonzero(E[0] == hc[0] + eps)[0]:   # strict: e == c + eps is not left of the root ...
                    assert np.all(Ld[n] >= P // 2)
                for n in np.nonzero(E[0] == hc[0] - eps)[0]:   # ... and e == c - eps is not right of it
                    assert np.all(Ld[n] < P // 2)
                if eps == 1.0:
                    assert np.any(E[0] == hc[0] + eps) and np.any(E[0] == hc[0] - eps)


# ------------------------------------------------------------------------------------ 3. from_tree against the list route
TREE_CASES = [(n, 0.0) for n in ("lattice33x31", "lattice32x32", "lattice33x32", "lattice65x63")] + [
    ("lattice33x31", G.H), ("lattice33x31", 0.3), ("lattice32x32", G.H), ("lattice33x32", 0.3), ("lattice65x63", 0.3),
    ("collinear", 0.0), ("collinear", 0.3), ("collinear", None), ("flat3d", 0.0), ("flat3d", 0.3), ("flat3d", None)]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name,eps", TREE_CASES, ids=["%s-eps%s" % c for c in TREE_CASES])
def test_from_tree_equals_the_list_route_on_degenerate_points(name, eps, dtype):
    X, levels = G.BUILDS[name]
    N = len(X)
    root, _, _ = pmk.setuppartition(X, levels)
    sets = _sets(root, levels, X, eps)
    used = np.zeros(N, dtype=int)
    for s in sets:
        used[s] += 1
    unused = np.nonzero(used == 0)[0]
    # the targets, the three output columns and the diagonal addend of a point that no patch gathers are NaN: they must
    # reach no buffer
    y = _targets(X)
    Y = np.asfortranarray(np.stack([_targets(X) + 0.1 * j * X[:, 0] for j in range(3)], 1))
    g = 0.5 + 0.25 * np.cos(X[:, 0]) ** 2
    y[unused], Y[unused], g[unused] = np.nan, np.nan, np.nan
    if eps == 0.0:
        assert len(unused) > 0
    if eps is not None and eps > 0:
        assert used.max() > 1 and used.sum() > N           # overlap
    sigma2 = SIGMA2 if dtype == "f64" else 1e-2
    tree = pmk.DeviceModel.from_tree(root, X, y, eps=eps, dtype=dtype)
    off, inds = tree.patch_index()
    assert np.array_equal(off, np.cumsum([0] + [len(s) for s in sets])) and np.array_equal(inds, np.concatenate(sets))
    assert len(np.intersect1d(inds, unused)) == 0
    host = _host_model(root, X, y, sets, dtype)
    _compare_packed(tree, host, name)
    for r in range(tree.P):
        for k in (0, 1):
            assert not np.any(np.isnan(_packed(tree, r, k)))
    _compare_fits(tree, host, S34, sigma2, (name, eps, dtype), need_ok=dtype == "f64")
    y2 = 0.5 * y + 1.0                                      # NaN where it was
    tree.set_targets_global(y2)
    host.set_targets([y2[s] for s in sets])
    _compare_packed(tree, host, "targets", buffers=(1,))
    _compare_fits(tree, host, S34, sigma2, (name, eps, dtype, "targets"), need_ok=dtype == "f64")
    tree.set_targets_multi_global(Y)
    host.set_targets_multi([Y[s] for s in sets])
    _compare_packed(tree, host, "multi", buffers=(3,))
    tree.solve_multi()
    host.solve_multi()
    for ca, cb in zip(tree.weights_multi(), host.weights_multi()):
        assert ca.shape[1] == 3 and same_bits(ca, cb)
        assert dtype == "f32" or not np.any(np.isnan(ca))
    tree.set_diag_global(g)
    host.set_diag([g[s] for s in sets])
    _compare_packed(tree, host, "diag", buffers=(2,))
    for r in range(tree.P):
        assert not np.any(np.isnan(_packed(tree, r, 2)))
    _compare_fits(tree, host, S34, sigma2, (name, eps, dtype, "diag"), need_ok=dtype == "f64")
    print("%s eps=%r %s: %d patches of %d..%d points, %d index entries for %d points, %d points in no patch: identical"
          % (name, eps, dtype, tree.P, min(tree.n), max(tree.n), off[-1], N, len(unused)))


def _list_route_status(ctx, X, sets):
    """pmk_model_create_ex on the host-cut lists, an empty one included -> status, message"""
    L = ctx.L
    P, D = len(sets), X.shape[1]
    n = np.array([len(s) for s in sets], dtype=np.int64)
    Xs = [np.ascontiguousarray(X[s]) if len(s) else np.zeros((1, D)) for s in sets]
    ys = [np.zeros(max(len(s), 1)) for s in sets]
    PA = _dp * P
    h = C.c_void_p()
    rc = L.pmk_model_create_ex(ctx.h, D, P, n.ctypes.data_as(_ip), PA(*[x.ctypes.data_as(_dp) for x in Xs]),
                               PA(*[v.ctypes.data_as(_dp) for v in ys]), 0, C.byref(h))
    msg = L.pmk_last_error().decode()
    if rc == 0:
        L.pmk_model_destroy(h)
    return rc, msg, h.value if rc else None


def test_empty_patches_are_refused_by_both_routes():
    import re
    L, ctx = pmk.lib(), pmk.default_context()
    Xl, ll = G.BUILDS["lattice33x31"]
    Xd, ld = G.BUILDS["dups5"]
    cases = [("dups5 leaves", Xd, ld, None), ("dups5 eps=0", Xd, ld, 0.0), ("lattice eps=NaN", Xl, ll, float("nan"))]
    for what, X, levels, eps in cases:
        root, _, _ = pmk.setuppartition(X, levels)
        sets = _sets(root, levels, X, eps)
        first_empty = int(np.argmax([len(s) == 0 for s in sets]))
        assert len(sets[first_empty]) == 0
        rc_l, msg_l, h_l = _list_route_status(ctx, X, sets)
        h = C.c_void_p()
        rc_t = L.pmk_model_create_from_bsp(ctx.h, M._native(root).h, len(X), X.ctypes.data, None,
                                           -1.0 if eps is None else eps, 0, 0, 0, C.byref(h))
        msg_t = L.pmk_last_error().decode()
        assert rc_l == rc_t == -4 and h.value is None and h_l is None, (what, rc_l, rc_t)
        named = [re.search(r"patch (\d+) has n=(\d+)", m) for m in (msg_l, msg_t)]
        assert all(named) and [m.groups() for m in named] == [(str(first_empty), "0")] * 2, (what, msg_l, msg_t)
        if eps is None or eps >= 0:                         # the wrapper hands the library's refusal on
            with pytest.raises(pmk.PmkError, match="patch %d" % first_empty):
                pmk.DeviceModel.from_tree(root, X, eps=eps)
        # a valid call on the same context afterwards
        root, _, _ = pmk.setuppartition(Xl, ll)
        m = pmk.DeviceModel.from_tree(root, Xl, _targets(Xl), eps=0.3)
        m.fit(S34, SIGMA2)
        assert np.all(m.info() == 0)
        print("%s: both routes refuse with -4, patch %d; a fit on the context afterwards succeeds" % (what, first_empty))


# ------------------------------------------------------------------------------------ 4. plan and mixture on the 33 x 31 lattice
RADIUS, DELTA = 0.5, 1e-5
WTH, OWTH = pmk.Spline34KernelType(1 / RADIUS), O.kernel(O.SPLINE34, 1 / RADIUS)


def _lattice_queries(X, hv, hc):
    """the lattice points, the cell centres, and for every internal node a few points projected onto its hyperplane"""
    rng = np.random.Generator(np.random.PCG64(41))
    onplane = []
    for v, c in zip(hv, hc):
        p = X[rng.integers(0, len(X), 12)]
        onplane.append(p + (c - p @ v)[:, None] * v[None, :])
    return np.ascontiguousarray(np.concatenate([X, X[:-1] + G.H / 2] + onplane))


@pytest.fixture(scope="module", params=[0, 1], ids=["plain-dot", "fma-dot"])
def lattice_mixture(request):
    """tree, eps-sets, oracle fits and the oracle's mixture on the 33 x 31 lattice in one dot mode, computed once"""
    dot_mode = request.param
    X, levels = G.BUILDS["lattice33x31"]
    y = _targets(X)
    root, _, _ = pmk.setuppartition(X, levels, dot_mode=dot_mode)
    X_set, X_set_inds, _, _ = pmk.organizetrainingsets(root, levels, X, 0.3)
    ys = [y[i] for i in X_set_inds]
    hv, hc = PT.hyperplane_arrays(root)
    Xq = _lattice_queries(X, hv, hc)
    ob = O.BSP(X, levels, dot_mode=dot_mode)
    fits = R.oracle_fits(OS34, X_set, ys, SIGMA2)
    kap = max(R.kappa(O.kernel_matrix(OS34, xs) + SIGMA2 * np.eye(len(xs))) for xs in X_set)
    ref = R.oracle_mixture(ob, OS34, OWTH, X_set, fits, Xq, RADIUS, DELTA)
    return dict(dot_mode=dot_mode, X=X, y=y, levels=levels, root=root, X_set=X_set, ys=ys, Xq=Xq, ref=ref, kappa=kap)


def _predict(m, Xq):
    q = pmk.DeviceQuery(m, Xq)
    q.plan(RADIUS, DELTA)
    q.items(S34)
    q.mix(WTH)
    Yq, Vq = q.fetch()
    return Yq, Vq, q.debug()


def test_plan_and_mixture_on_the_lattice_fp64(lattice_mixture):
    p = lattice_mixture
    oY, oV, ohome, ooff, oreg, ots = p["ref"]
    m = pmk.DeviceModel(p["X_set"], p["ys"])
    m.fit(S34, SIGMA2)
    m.set_bsp(p["root"], 0)
    assert np.all(m.info() == 0)
    Yq, Vq, dbg = _predict(m, p["Xq"])
    R.assert_plan_matches(dbg, ohome, ooff, oreg, ots, "dot_mode %d" % p["dot_mode"])
    zero_t = int((ots == 0).sum())
    print("dot_mode %d: %d queries, %d neighbour items, %d of them with t == 0; max kappa(U) %.0f"
          % (p["dot_mode"], len(Yq), len(ots), zero_t, p["kappa"]))
    assert zero_t > 0
    R.assert_fp64_values(Yq, Vq, oY, oV, "dot_mode %d" % p["dot_mode"])
    # the same queries through a device-built tree and a from_tree model
    rootd, _, _ = pmk.setuppartition(p["X"], p["levels"], dot_mode=p["dot_mode"], device=True)
    mt = pmk.DeviceModel.from_tree(rootd, p["X"], p["y"], eps=0.3)
    mt.fit(S34, SIGMA2)
    Yt, Vt, dbgt = _predict(mt, p["Xq"])
    assert same_bits(Yt, Yq) and same_bits(Vt, Vq)
    for k in ("home", "item_offsets", "item_region", "item_t", "item_w", "item_u", "item_v"):
        assert same_bits(dbgt[k], dbg[k]), k


def test_plan_and_items_on_the_lattice_fp32(lattice_mixture):
    p = lattice_mixture
    _, _, ohome, ooff, oreg, ots = p["ref"]
    assert p["kappa"] * EPS32 <= 1e-3, p["kappa"]
    m = pmk.DeviceModel(p["X_set"], p["ys"], dtype="f32")
    m.fit(S34, SIGMA2)
    m.set_bsp(p["root"], 0)
    assert np.all(m.info() == 0)
    Yq, Vq, dbg = _predict(m, p["Xq"])
    R.assert_plan_matches(dbg, ohome, ooff, oreg, ots, "f32, dot_mode %d" % p["dot_mode"])
    off = dbg["item_offsets"]
    worst = [0.0, 0.0]
    for r in np.unique(dbg["item_region"]):
        idx = np.nonzero(dbg["item_region"] == r)[0]
        qj = np.searchsorted(off, idx, side="right") - 1
        Xr = p["X_set"][int(r)]
        k = R.kappa(O.kernel_matrix(OS34, Xr) + SIGMA2 * np.eye(len(Xr)))
        mu, var, msc, vsc = R.queryinner_reference(OS34, Xr, m.get(int(r), M.GET_C), m.get(int(r), M.GET_L), p["Xq"][qj])
        du, dv = np.abs(dbg["item_u"][idx] - mu), np.abs(dbg["item_v"][idx] - var)
        worst = [max(worst[0], (du / (np.sqrt(k) * EPS32 * (msc + 1))).max()), max(worst[1], (dv / (k * EPS32 * (vsc + 1))).max())]
        assert np.all(du <= 50 * np.sqrt(k) * EPS32 * (msc + 1)), (r, du.max())
        assert np.all(dv <= 50 * k * EPS32 * (vsc + 1)), (r, dv.max())
    print("f32 dot_mode %d: %d items; worst du %.3f sqrt(kappa) eps32 (|k|.|c| + 1), dv %.3f kappa eps32 (scale + 1)"
          % (p["dot_mode"], off[-1], worst[0], worst[1]))


# ------------------------------------------------------------------------------------ 5. the edge of the kernels' support
# Distances on the lattice are integers: with twice the offsets in steps as coordinates, the support radius 5 steps is a
# squared distance of 100.  It occurs as (10, 0), (6, 8) and (8, 6), so sqrt_dist(1.5625) must be 1.25 exactly.
EDGE = 100
KERNELS = {"spline34": (S34, OS34),
           "spline32": (pmk.Spline32KernelType(A), O.kernel(O.SPLINE32, A)),
           "spline12": (pmk.Spline12KernelType(A), O.kernel(O.SPLINE12, A))}
LX, LS = G.lattice(33, 31), G.lattice_steps(33, 31)


def _d2(SA, SB):
    return ((SA[:, None, :] - SB[None, :, :]) ** 2).sum(-1)


def _check_pattern(K, d2, Ko, what, exact):
    """zeros exactly where integer arithmetic puts the pair outside the support (+0.0), non-zero inside; on the radius
    the oracle's pattern (exact) or a printed count; inside, 4 ulps of the oracle (exact)"""
    far, near, edge = d2 > EDGE, d2 < EDGE, d2 == EDGE
    assert edge.sum() > 0, what
    kb = np.ascontiguousarray(K).view(np.uint64)
    assert np.all(kb[far] == 0), (what, "outside", int((kb[far] != 0).sum()))
    assert np.all(K[near] != 0), (what, "inside", int((K[near] == 0).sum()))
    print("%s: %d pairs on the radius (device non-zero on %d, oracle on %s), %d inside, %d outside"
          % (what, edge.sum(), int((K[edge] != 0).sum()), "-" if Ko is None else int((Ko[edge] != 0).sum()), near.sum(),
             far.sum()))
    if exact:
        assert np.array_equal(K[edge] == 0, Ko[edge] == 0), what
        assert np.all(kb[edge & (K == 0)] == 0), what
        assert np.array_equal(K == 0, Ko == 0), what
        nz = Ko != 0
        assert ulps(K[nz], Ko[nz]).max() <= 4, (what, ulps(K[nz], Ko[nz]).max())


@pytest.mark.parametrize("fam", list(KERNELS))
def test_support_edge_in_the_kernel_matrix(fam):
    th, oth = KERNELS[fam]
    K, Ko = pmk.constructkernelmatrix(LX, th), O.kernel_matrix(oth, LX)
    assert np.array_equal(K, K.T)
    _check_pattern(K, _d2(LS, LS), Ko, fam + " symmetric", True)
    sel = np.arange(len(LX))[::-3][:300]                    # a cross matrix that is not a block of the symmetric one
    Kc, Kco = pmk.constructkernelmatrix(LX, LX[sel], th), O.cross_kernel_matrix(oth, LX, LX[sel])
    _check_pattern(Kc, _d2(LS, LS[sel]), Kco, fam + " cross", True)


@pytest.fixture(scope="module")
def lattice_sets():
    root, _, _ = pmk.setuppartition(LX, 4)
    _, inds, _, _ = pmk.organizetrainingsets(root, 4, LX, 0.3)
    return root, inds


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("fam", list(KERNELS))
def test_support_edge_in_the_fit_and_in_the_strip_kernel(lattice_sets, fam, dtype):
    root, inds = lattice_sets
    th, oth = KERNELS[fam]
    y = _targets(LX)
    sigma2 = SIGMA2 if dtype == "f64" else 1e-2
    m = pmk.DeviceModel([LX[i] for i in inds], [y[i] for i in inds], dtype=dtype)
    m.fit(th, sigma2)
    assert dtype == "f32" or np.all(m.info() == 0)
    exact = dtype == "f64"
    for r, ix in enumerate(inds):                           # GET_K of every fitted patch
        K = m.get(r, M.GET_K)
        assert np.array_equal(K, K.T)
        _check_pattern(K, _d2(LS[ix], LS[ix]), O.kernel_matrix(oth, LX[ix]) if exact else None,
                       "%s %s GET_K patch %d" % (fam, dtype, r), exact)
    # the strip kernel's cross-kernel: with one-hot weights the predicted mean of EVERY lattice point is one row of the
    # cross-kernel matrix (the other terms are exact zeros); rows on both sides of the 128-row tile edge
    L = m.ctx.L
    PA = _dp * m.P
    r = int(np.argmax([len(i) for i in inds]))
    n = len(inds[r])
    assert n > 129
    for i in (0, 127, 128, n - 1):
        cs = [np.zeros(len(ix)) for ix in inds]
        cs[r][i] = 1.0
        _lib.check(L.pmk_model_set_weights(m.h, PA(*[c.ctypes.data_as(_dp) for c in cs])), "pmk_model_set_weights")
        mu, var = m.queryinner(r, th, LX)
        row = inds[r][i]
        ko = np.array([O.kernel_eval(oth, x, LX[row]) for x in LX]) if exact else None
        _check_pattern(mu[None, :], _d2(LS[row:row + 1], LS), None if ko is None else ko[None, :],
                       "%s %s strip row %d of patch %d" % (fam, dtype, i, r), exact)
    # queries whose nearest point of the patch is exactly on the radius: the whole cross-kernel column is zero, so the
    # mean is 0 and (fp64) the variance is k(x, x) = 1 for any weights
    dmin = _d2(LS, LS[inds[r]]).min(1)
    ring, inner = np.nonzero(dmin == EDGE)[0], np.nonzero(dmin < EDGE)[0]
    assert len(ring) > 0
    cs = [np.ones(len(ix)) for ix in inds]
    _lib.check(L.pmk_model_set_weights(m.h, PA(*[c.ctypes.data_as(_dp) for c in cs])), "pmk_model_set_weights")
    mu, var = m.queryinner(r, th, LX)
    assert np.all(mu[ring] == 0) and np.all(mu[inner] != 0)
    if exact:
        assert np.all(var[ring] == 1.0)
    print("%s %s: %d lattice points have their nearest point of patch %d exactly on the radius: mean 0" % (fam, dtype, len(ring), r))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_support_edge_fused_and_unfused_fit_agree(lattice_sets, monkeypatch, dtype):
    _, inds = lattice_sets
    y = _targets(LX)
    assert max(len(i) for i in inds) > 128                  # tiles below the diagonal exist: the fused build runs
    got = []
    for fuse in ("0", "1"):
        monkeypatch.setenv("PMK_FUSE_K1", fuse)
        model, cs, info = pmk.fit_patches([LX[i] for i in inds], [y[i] for i in inds], S34, SIGMA2 if dtype == "f64" else 1e-2,
                                          dtype=dtype)
        assert dtype == "f32" or np.all(info == 0)
        got.append([(cs[r], model.get(r, M.GET_L), model.get(r, M.GET_LINV_DIAG), model.get(r, M.GET_K)) for r in range(len(inds))])
    for a, b in zip(*got):
        for u, v in zip(a, b):
            assert same_bits(u, v)
    edge = sum(int((_d2(LS[i], LS[i]) == EDGE).sum()) for i in inds)
    print("%s: fused and unfused fits identical on %d patches with %d pairs on the radius" % (dtype, len(inds), edge))
    assert edge > 0


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("fam", list(KERNELS))
def test_support_edge_in_the_item_kernels(lattice_sets, fam, dtype):
    """queries OUTSIDE the lattice whose nearest lattice point is exactly on the radius -- 5 steps off the right edge along
    a row, and (3, 4) / (4, 3) steps off the upper right corner: every item of such a query has an all-zero cross-kernel
    column, so every mixed mean is exactly 0, through the strip kernel (items), item_means_kernel (items_multi without the
    variance) and items_multi with it.  One step closer the means are non-zero."""
    root, inds = lattice_sets
    th, _ = KERNELS[fam]
    y = _targets(LX) + 2.0
    xmax, ymax, h = LX[:, 0].max(), LX[:, 1].max(), G.H
    rows = np.unique(LX[:, 1])
    on = np.concatenate([np.stack([np.full(len(rows), xmax + 5 * h), rows], 1),
                         [[xmax + 3 * h, ymax + 4 * h], [xmax + 4 * h, ymax + 3 * h]]])
    closer = np.concatenate([np.stack([np.full(len(rows), xmax + 4 * h), rows], 1), [[xmax + 3 * h, ymax + 3 * h]]])
    S = np.rint(np.concatenate([on, closer]) / (h / 2)).astype(np.int64)
    dmin = _d2(S, LS).min(1)
    assert np.all(dmin[:len(on)] == EDGE) and np.all(dmin[len(on):] < EDGE)
    Xq = np.ascontiguousarray(np.concatenate([on, closer]))
    m = pmk.DeviceModel([LX[i] for i in inds], [y[i] for i in inds], dtype=dtype)
    m.fit(th, SIGMA2 if dtype == "f64" else 1e-2)
    m.set_bsp(root, 0)
    Y3 = [np.asfortranarray(np.stack([y[i] + j for j in range(3)], 1)) for i in inds]
    m.set_targets_multi(Y3)
    m.solve_multi()
    q = pmk.DeviceQuery(m, Xq)
    q.plan(RADIUS, DELTA)
    q.items(th)
    q.mix(WTH)
    Yq, Vq = q.fetch()
    items = q.total
    assert np.all(Yq[:len(on)] == 0) and np.all(Yq[len(on):] != 0), (Yq[:len(on)], Yq[len(on):])
    for variance in (False, True):
        q.items_multi(th, variance)
        q.mix_multi(WTH)
        Ym, _ = q.fetch_multi(3)
        assert np.all(Ym[:len(on)] == 0) and np.all(Ym[len(on):] != 0), variance
    print("%s %s: %d queries (%d items) with their nearest training point exactly on the radius: means 0 through items, "
          "items_multi mean-only and items_multi with the variance; %d queries one step closer: non-zero"
          % (fam, dtype, len(on), items, len(closer)))

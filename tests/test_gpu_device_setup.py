"""Device-resident set-up on the GPU: a model from a tree and ONE global point array (pmk_model_create_from_bsp), targets
and the diagonal addend from global per-point arrays (pmk_model_set_*_global), predictions into device memory
(pmk_query_fetch_dev / _multi_dev).

The reference in every test is the EXISTING HOST ROUTE on the same inputs: the lists of organizetrainingsets or
setuppartition -> DeviceModel(X_set, y_set).  Equality is BITWISE: both routes end in the same device buffers and run
the same kernels, so there is no tolerance.  Arrays are compared on their raw bits, so that a NaN does not pass for equal
(nor +0 for -0).  Every test prints what it compared under -s.
"""
import ctypes as C

import numpy as np
import pytest

import patchmixturekriging_amd as pmk
from patchmixturekriging_amd import _lib
from patchmixturekriging_amd import dist as pd
from patchmixturekriging_amd import mixture as M

pytestmark = pytest.mark.gpu

S34 = pmk.Spline34KernelType(1 / 3.0)
RQ = pmk.RationalQuadraticKernelType(2.0)           # a family that takes the run-time switch of the kernels
WTH = pmk.Spline34KernelType(2.0)
SIGMA2 = 1e-3
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int64)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind == "f":
        return bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))
    return bool(np.array_equal(a, b))


def _points(N, D, seed):
    return np.random.default_rng(seed).uniform(-4, 4, (N, D))


def _targets(X, shift=0.0):
    return np.sin(0.7 * X[:, 0] + shift) * np.cos(0.3 * X[:, -1]) + 0.05 * X[:, 0]


def _sets(root, levels, X, eps):
    """the host route's index lists"""
    if eps is None:
        L = pmk.lib()
        h = M._native(root).h
        P = L.pmk_bsp_num_leaves(h)
        off, inds = np.empty(P + 1, dtype=np.int64), np.empty(len(X), dtype=np.int64)
        _lib.check(L.pmk_bsp_arrays(h, None, None, off.ctypes.data_as(_ip), inds.ctypes.data_as(_ip)))
        return [inds[off[r]:off[r + 1]].copy() for r in range(P)]
    return pmk.organizetrainingsets(root, levels, X, eps)[1]


def _host_model(root, X, y, sets, dtype="f64", leaf_base=0):
    m = pmk.DeviceModel([X[s] for s in sets], [y[s] for s in sets], dtype=dtype)
    m.set_bsp(root, leaf_base)
    return m


def _packed(m, r, what):
    L = m.ctx.L
    ld = C.c_int64()
    _lib.check(L.pmk_test_model_packed(m.h, r, what, C.byref(ld), None), "pmk_test_model_packed")
    width = {0: m.D, 1: 1, 2: 1, 3: M.MAX_OUTPUTS}[what]
    out = np.empty(ld.value * width)
    _lib.check(L.pmk_test_model_packed(m.h, r, what, C.byref(ld), out.ctypes.data_as(_dp)), "pmk_test_model_packed")
    return out


def _compare_fits(a, b, theta, sigma2, what, need_ok=True):
    """fit both models and compare everything a fit leaves behind, patch by patch"""
    a.fit(theta, sigma2)
    b.fit(theta, sigma2)
    ia, ib = a.info(), b.info()
    assert same_bits(ia, ib), (what, ia, ib)
    if need_ok:
        assert np.all(ia == 0), (what, ia)
    for ca, cb in zip(a.weights(), b.weights()):
        assert same_bits(ca, cb), what
    for r in range(a.P):
        for g in (M.GET_L, M.GET_K, M.GET_LINV_DIAG):
            assert same_bits(a.get(r, g), b.get(r, g)), (what, r, g)


def _compare_packed(a, b, what, buffers=(0, 1)):
    for r in range(a.P):
        for k in buffers:
            assert same_bits(_packed(a, r, k), _packed(b, r, k)), (what, "patch", r, "buffer", k)


# ------------------------------------------------------------------------------------ 1. bit identity of the fitted model
# (D, N, levels, eps, dot_mode, dtype): the smallest shapes that reach each packing edge
SHAPES = [
    ("tile multiples", 2, 1024, 3, None, 0, "f64"),       # leaves of exactly 256 points: no padding rows at all
    ("ragged", 2, 1027, 3, None, 0, "f64"),
    ("ragged fp32", 2, 1027, 3, None, 0, "f32"),
    ("one tile", 2, 200, 3, None, 0, "f64"),              # ~50 points per patch: one tile, mostly padding
    ("eps overlap", 2, 3000, 3, 0.35, 0, "f64"),
    ("eps overlap fp32", 2, 3000, 3, 0.35, 0, "f32"),
    ("D=1", 1, 700, 3, None, 0, "f64"),
    ("D=3", 3, 700, 3, 0.2, 0, "f64"),
    ("D=4", 4, 700, 3, None, 0, "f64"),
    ("fma dot", 2, 700, 3, 0.3, 1, "f64"),
    ("plain dot", 2, 700, 3, 0.3, 0, "f64"),
]


@pytest.mark.parametrize("name, D, N, levels, eps, dot_mode, dtype", SHAPES, ids=[s[0] for s in SHAPES])
def test_fitted_model_is_bit_identical_with_the_host_route(name, D, N, levels, eps, dot_mode, dtype):
    X = _points(N, D, 100 + N + D)
    y = _targets(X)
    root, _, _ = pmk.setuppartition(X, levels, dot_mode=dot_mode)
    sets = _sets(root, levels, X, eps)
    sizes = [len(s) for s in sets]
    if name == "tile multiples":
        assert sizes == [256] * 4, sizes
    if name == "one tile":
        assert max(sizes) < 128, sizes
    tree = pmk.DeviceModel.from_tree(root, X, y, eps=eps, dtype=dtype)
    off, inds = tree.patch_index()
    assert off.dtype == np.int64 and inds.dtype == np.int64
    assert np.array_equal(off, np.concatenate([[0], np.cumsum(sizes)]))
    assert np.array_equal(inds, np.concatenate(sets))
    assert np.array_equal(tree.n, sizes)
    if eps is not None and name.startswith("eps"):
        assert off[-1] > N, (off[-1], N)
        both = np.zeros(N, dtype=int)
        for s in sets:
            both[s] += 1
        for s in sets:
            assert np.any(both[s] > 1)                     # every patch shares points with a neighbour
    for r, s in enumerate(sets):
        assert same_bits(tree.X[r], X[s])                  # cut lazily from the index list
    host = _host_model(root, X, y, sets, dtype)
    _compare_packed(tree, host, name)                      # coordinates and targets WITH their padding rows
    if dtype == "f32":
        r = int(np.argmax(np.array(sizes) % 128 != 0))    # a patch that has padding rows
        pad = _packed(tree, r, 0).reshape(D, -1)[:, sizes[r]:]
        assert pad.size > 0 and np.all(np.isposinf(pad))   # 1e300 converted to fp32
    for theta in (S34, RQ):
        _compare_fits(tree, host, theta, 1e-2 if dtype == "f32" else SIGMA2, (name, type(theta).__name__),
                      need_ok=dtype == "f64")
    print("%s: %d patches %s, %d index entries, two kernels: identical" % (name, tree.P, sizes, off[-1]))


# ------------------------------------------------------------------------------------ 2. where the inputs live
def test_host_device_and_mixed_inputs_give_identical_models():
    import torch
    X = _points(1027, 2, 7)
    y = _targets(X)
    root, _, _ = pmk.setuppartition(X, 3)
    Xd, yd = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()
    torch.cuda.synchronize()
    ref = pmk.DeviceModel.from_tree(root, X, y, eps=0.3)
    ref.fit(S34, SIGMA2)
    for what, (xa, ya) in {"device": (Xd, yd), "mixed": (Xd, y), "mixed the other way": (X, yd)}.items():
        m = pmk.DeviceModel.from_tree(root, xa, ya, eps=0.3)
        assert same_bits(m.patch_index()[1], ref.patch_index()[1])
        assert (m.X is None) == (xa is Xd)                 # device points never come to the host
        _compare_packed(m, ref, what)
        _compare_fits(m, ref, S34, SIGMA2, what)
    print("numpy / torch device / mixed inputs: identical")


# ------------------------------------------------------------------------------------ 3. the global setters
@pytest.fixture(scope="module")
def pair():
    """one tree model and its host-route twin on overlapping eps-sets, shared by the setter tests"""
    X = _points(1500, 2, 11)
    y = _targets(X)
    root, _, _ = pmk.setuppartition(X, 3)
    sets = _sets(root, 3, X, 0.3)
    return dict(X=X, y=y, root=root, sets=sets, tree=pmk.DeviceModel.from_tree(root, X, y, eps=0.3),
                host=_host_model(root, X, y, sets))


def _compare_scores(a, b, what):
    a.loo()
    b.loo()
    for va, vb in zip(a.loo_values(), b.loo_values()):
        for pa, pb in zip(va, vb):
            assert same_bits(pa, pb), what
    for ea, eb in zip(a.evidence(), b.evidence()):
        assert same_bits(ea, eb), what


def test_set_targets_global_equals_set_targets(pair):
    import torch
    a, b, sets = pair["tree"], pair["host"], pair["sets"]
    for what in ("host", "device"):
        y2 = _targets(pair["X"], shift=1.1 if what == "host" else 2.3)
        arr = y2 if what == "host" else torch.from_numpy(y2).cuda()
        torch.cuda.synchronize()
        a.set_targets_global(arr)
        b.set_targets([y2[s] for s in sets])
        _compare_packed(a, b, what, buffers=(1,))
        _compare_fits(a, b, S34, SIGMA2, what)
        _compare_scores(a, b, what)
    print("set_targets_global (host, device): weights, factors, leave-one-out, evidence identical")


@pytest.mark.parametrize("R", [1, 3, 16])
def test_set_targets_multi_global_equals_set_targets_multi(pair, R):
    import torch
    a, b, sets, X = pair["tree"], pair["host"], pair["sets"], pair["X"]
    N = len(X)
    big = np.full((N + 5, R), np.nan, order="F")          # ldy = N + 5; the five spare rows must never be read
    big[:N] = np.stack([_targets(X, shift=0.4 * j) + 0.1 * j for j in range(R)], 1)
    Y = big[:N]
    a.fit(S34, SIGMA2)
    b.fit(S34, SIGMA2)
    tb = torch.from_numpy(big).cuda()
    torch.cuda.synchronize()
    assert tb.stride() == (1, N + 5)
    for what, arr in (("host", Y), ("device", tb[:N])):
        a.set_targets_multi_global(arr)
        b.set_targets_multi([Y[s] for s in sets])
        _compare_packed(a, b, (what, R), buffers=(3,))
        a.solve_multi()
        b.solve_multi()
        for ca, cb in zip(a.weights_multi(), b.weights_multi()):
            assert ca.shape[1] == R and same_bits(ca, cb), (what, R)
        a.loo()
        b.loo()
        (ra, va), (rb, vb) = a.loo_values_multi(), b.loo_values_multi()
        for pa, pb in zip(ra + va, rb + vb):
            assert same_bits(pa, pb), (what, R)
        for ea, eb in zip(a.evidence_multi(), b.evidence_multi()):
            assert same_bits(ea, eb), (what, R)
    print("set_targets_multi_global R=%d, ldy=N+5 (host, device): identical" % R)


def test_set_diag_global_equals_set_diag(pair):
    import torch
    a, b, sets, X = pair["tree"], pair["host"], pair["sets"], pair["X"]
    a.set_targets_global(pair["y"])
    b.set_targets([pair["y"][s] for s in sets])
    _compare_fits(a, b, S34, SIGMA2, "before")
    L0 = [a.get(r, M.GET_L) for r in range(a.P)]
    g = 0.5 + 0.25 * np.cos(X[:, 0]) ** 2
    for what, arr in (("host", g), ("device", torch.from_numpy(g).cuda())):
        torch.cuda.synchronize()
        a.set_diag_global(arr)
        b.set_diag([g[s] for s in sets])
        _compare_packed(a, b, what, buffers=(2,))
        _compare_fits(a, b, S34, SIGMA2, what)
        assert not same_bits(a.get(0, M.GET_L), L0[0])     # the addend is really in the factor
        _compare_scores(a, b, what)
    a.set_diag_global(None)
    b.set_diag(None)
    _compare_fits(a, b, S34, SIGMA2, "cleared")
    for r in range(a.P):
        assert same_bits(a.get(r, M.GET_L), L0[r])
    print("set_diag_global (host, device, cleared): identical")


# ------------------------------------------------------------------------------------ 4. a shard
def test_a_shard_equals_its_patches_of_the_whole_model():
    import torch
    X = _points(1500, 2, 13)
    y = _targets(X)
    root, _, _ = pmk.setuppartition(X, 3)
    whole = pmk.DeviceModel.from_tree(root, X, y, eps=0.3)
    shard = pmk.DeviceModel.from_tree(root, X, y, eps=0.3, leaf_base=2, P=2)
    assert shard.P == 2 and np.array_equal(shard.n, whole.n[2:])
    ow, iw = whole.patch_index()
    os_, is_ = shard.patch_index()
    assert np.array_equal(os_, ow[2:] - ow[2]) and np.array_equal(is_, iw[ow[2]:])
    whole.fit(S34, SIGMA2)
    shard.fit(S34, SIGMA2)
    assert np.all(whole.info() == 0) and np.all(shard.info() == 0)
    cw, cs = whole.weights(), shard.weights()
    for r in range(2):
        assert same_bits(cs[r], cw[2 + r])
        assert same_bits(shard.get(r, M.GET_L), whole.get(2 + r, M.GET_L))
    # explicit (point, region) items on points of the shard's leaves, through both models
    leaf = np.array([pmk.findpartition(x, root) for x in X[:400]])
    keep = leaf >= 2
    xs, reg = np.ascontiguousarray(X[:400][keep]), np.ascontiguousarray(leaf[keep], dtype=np.int32)
    assert len(reg) > 50 and set(reg.tolist()) == {2, 3}
    out = []
    for m in (whole, shard):
        q = pmk.DeviceQuery.from_items(m, len(reg), xs.ctypes.data, reg.ctypes.data)
        q.items(S34)
        u = torch.empty(len(reg), dtype=torch.float64, device="cuda")
        v = torch.empty(len(reg), dtype=torch.float64, device="cuda")
        q.export_results(u.data_ptr(), v.data_ptr())
        m.ctx.synchronize()
        out.append((u.cpu().numpy(), v.cpu().numpy()))
    assert same_bits(out[0][0], out[1][0]) and same_bits(out[0][1], out[1][1])
    # a leaf range outside the tree is refused
    with pytest.raises(pmk.PmkError):
        pmk.DeviceModel.from_tree(root, X, y, eps=0.3, leaf_base=3, P=2)
    print("shard [2, 4): fit and %d explicit items identical" % len(reg))


# ------------------------------------------------------------------------------------ 5. predict end to end
SENTINEL = -12345.678


@pytest.fixture(scope="module")
def predict_pair():
    X = _points(3000, 2, 17)
    y = _targets(X)
    root, _, _ = pmk.setuppartition(X, 3)
    sets = _sets(root, 3, X, 0.3)
    tree, host = pmk.DeviceModel.from_tree(root, X, y, eps=0.3), _host_model(root, X, y, sets)
    tree.fit(S34, SIGMA2)
    host.fit(S34, SIGMA2)
    Xq = np.random.default_rng(18).uniform(-4, 4, (513, 2))
    return dict(X=X, sets=sets, tree=tree, host=host, Xq=Xq)


def test_predict_into_device_tensors(predict_pair):
    import torch
    p = predict_pair
    Nq = len(p["Xq"])
    qh = pmk.DeviceQuery(p["host"], p["Xq"])
    qh.plan(0.5, 1e-5)
    qh.items(S34)
    qh.mix(WTH)
    Yh, Vh = qh.fetch()
    Xqd = torch.from_numpy(p["Xq"]).cuda()
    buf = torch.full((2, Nq + 8), SENTINEL, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    qt = pmk.DeviceQuery(p["tree"], Xqd)                   # device Xq: no host copy
    assert qt.Xq is None and qt.Nq == Nq
    qt.plan(0.5, 1e-5)
    qt.items(S34)
    qt.mix(WTH)
    qt.fetch_into(buf[0, :Nq], buf[1, :Nq])
    p["tree"].ctx.synchronize()
    got = buf.cpu().numpy()
    assert same_bits(got[0, :Nq], Yh) and same_bits(got[1, :Nq], Vh)
    assert np.all(got[:, Nq:] == SENTINEL)                 # nothing past the outputs
    Yt, Vt = qt.fetch()
    assert same_bits(Yt, Yh) and same_bits(Vt, Vh)
    print("fetch_into: Yq, Vq of %d queries identical with the host route's fetch()" % Nq)


@pytest.mark.parametrize("variance", [True, False])
def test_predict_multi_into_device_tensors(predict_pair, variance):
    import torch
    p = predict_pair
    X, sets, Nq, R = p["X"], p["sets"], len(p["Xq"]), 3
    Y = np.asfortranarray(np.stack([_targets(X, shift=0.4 * j) for j in range(R)], 1))
    p["host"].set_targets_multi([Y[s] for s in sets])
    p["tree"].set_targets_multi_global(Y)
    for m in (p["host"], p["tree"]):
        m.solve_multi()
    qh = pmk.DeviceQuery(p["host"], p["Xq"])
    qh.plan(0.5, 1e-5)
    qh.items_multi(S34, variance)
    qh.mix_multi(WTH)
    Yh, Vh = qh.fetch_multi(R)
    assert (Vh is None) == (not variance)
    ld = Nq + 3
    ybuf = torch.full((R + 1, ld), SENTINEL, dtype=torch.float64, device="cuda")      # column-major (ld, R + 1)
    vbuf = torch.full((Nq + 8,), SENTINEL, dtype=torch.float64, device="cuda")
    Xqd = torch.from_numpy(p["Xq"]).cuda()
    torch.cuda.synchronize()
    qt = pmk.DeviceQuery(p["tree"], Xqd)
    qt.plan(0.5, 1e-5)
    qt.items_multi(S34, variance)
    qt.mix_multi(WTH)
    Yview = ybuf.T[:Nq, :R]
    assert Yview.stride() == (1, ld)
    if not variance:
        with pytest.raises(ValueError):
            qt.fetch_multi_into(Yview, vbuf[:Nq])
        rc = qt.L.pmk_query_fetch_multi_dev(qt.h, Yview.data_ptr(), ld, vbuf.data_ptr())     # the library says so too
        assert rc == -3 and "want_var" in qt.L.pmk_last_error().decode()
    qt.fetch_multi_into(Yview, vbuf[:Nq] if variance else None)
    p["tree"].ctx.synchronize()
    got, gv = ybuf.cpu().numpy(), vbuf.cpu().numpy()
    assert same_bits(got[:R, :Nq].T, Yh)
    assert np.all(got[:R, Nq:] == SENTINEL) and np.all(got[R] == SENTINEL)
    if variance:
        assert same_bits(gv[:Nq], Vh)
        assert np.all(gv[Nq:] == SENTINEL)
    else:
        assert np.all(gv == SENTINEL)
    print("fetch_multi_into R=3 variance=%s: identical, sentinels intact" % variance)


# ------------------------------------------------------------------------------------ 6. ordering on a shared stream
def test_a_target_produced_on_the_stream_needs_no_host_synchronisation(predict_pair):
    import torch
    p = predict_pair
    tree, ctx = p["tree"], p["tree"].ctx
    Xd, Xqd = torch.from_numpy(p["X"]).cuda(), torch.from_numpy(p["Xq"]).cuda()
    Nq = len(p["Xq"])

    def produce(shift):
        # a few milliseconds of device work that the targets depend on: the library's calls below are enqueued while it
        # is still running, so only the stream orders them
        z = torch.ones(1 << 25, dtype=torch.float64, device="cuda")
        for _ in range(20):
            z = torch.sin(z) + 1.0
        return torch.sin(0.7 * Xd[:, 0] + shift) * torch.cos(0.3 * Xd[:, 1]) + 0.05 * Xd[:, 0] + 0.0 * z[0]

    def run(shift, synchronise):
        out = torch.empty((2, Nq), dtype=torch.float64, device="cuda")
        yd = produce(shift)                                # a torch op, enqueued immediately before the library's calls
        if synchronise:
            torch.cuda.synchronize()
        tree.set_targets_global(yd)
        tree.fit(S34, SIGMA2)
        q = pmk.DeviceQuery(tree, Xqd)
        q.plan(0.5, 1e-5)                                  # the plan blocks for its sizes; the targets are not its input
        q.items(S34)
        q.mix(WTH)
        q.fetch_into(out[0], out[1])
        if synchronise:
            torch.cuda.synchronize()
        return out, yd

    pd.use_torch_stream(ctx)
    try:
        free, y_free = run(0.9, False)
        res_free = free.cpu().numpy()                      # torch's own copy, ordered on the shared stream
        sync, y_sync = run(0.9, True)
        res_sync = sync.cpu().numpy()
        torch.cuda.synchronize()
        assert same_bits(y_free.cpu().numpy(), y_sync.cpu().numpy())
        assert same_bits(res_free, res_sync)
        assert np.all(np.isfinite(res_sync)) and np.all(tree.info() == 0)
    finally:
        torch.cuda.synchronize()
        ctx.set_stream(None)
        ctx.shares_torch_stream = False
    print("shared stream: no-sync sequence equals the synchronised one on %d queries" % Nq)


# ------------------------------------------------------------------------------------ 7. refusals
def _one_good_fit(root, X, y):
    m = pmk.DeviceModel.from_tree(root, X, y)
    m.fit(S34, SIGMA2)
    assert np.all(m.info() == 0)
    m.ctx.synchronize()


def test_refusals_return_their_status_and_leave_the_context_usable():
    X = _points(600, 2, 23)
    y = _targets(X)
    root, _, inds = pmk.setuppartition(X, 3)
    L, ctx = pmk.lib(), pmk.default_context()
    tree = M._native(root).h
    h = C.c_void_p()

    def create(Xa, eps):
        return L.pmk_model_create_from_bsp(ctx.h, tree, len(Xa), Xa.ctypes.data, None, eps, 0, 0, 0, C.byref(h))

    # the tree's own leaves need the tree's own points
    assert create(X[:-1].copy(), -1.0) == -3 and h.value is None
    assert "600" in L.pmk_last_error().decode()
    # N at 2^31 is refused before anything is read
    assert L.pmk_model_create_from_bsp(ctx.h, tree, 1 << 31, X.ctypes.data, None, 0.1, 0, 0, 0, C.byref(h)) == -5
    _one_good_fit(root, X, y)
    # a point set in one half of the tree's box leaves the other half's leaves empty
    half = np.ascontiguousarray(X[np.concatenate([inds[0], inds[1]])])
    assert create(half, 0.0) == -4 and h.value is None
    assert "patch 2" in L.pmk_last_error().decode()
    with pytest.raises(pmk.PmkError, match="patch 2"):
        pmk.DeviceModel.from_tree(root, half, eps=0.0)
    _one_good_fit(root, X, y)
    # the global calls belong to models made by pmk_model_create_from_bsp
    lists = pmk.DeviceModel([X[i] for i in inds], [y[i] for i in inds])
    assert L.pmk_model_set_targets_global(lists.h, y.ctypes.data) == -3
    assert L.pmk_model_set_targets_multi_global(lists.h, 1, y.ctypes.data, len(y)) == -3
    assert L.pmk_model_set_diag_global(lists.h, y.ctypes.data) == -3
    assert L.pmk_model_set_diag_global(lists.h, None) == -3
    assert L.pmk_model_patch_index(lists.h, None, None, None) == -3
    assert "pmk_model_create_from_bsp" in L.pmk_last_error().decode()
    lists.fit(S34, SIGMA2)                                  # untouched by the refused calls
    assert np.all(lists.info() == 0)
    # argument checks of the setters on a tree model
    m = pmk.DeviceModel.from_tree(root, X, y)
    assert L.pmk_model_set_targets_multi_global(m.h, 0, y.ctypes.data, len(y)) == -2
    assert L.pmk_model_set_targets_multi_global(m.h, 17, y.ctypes.data, len(y)) == -2
    assert L.pmk_model_set_targets_multi_global(m.h, 1, y.ctypes.data, len(y) - 1) == -3
    assert L.pmk_model_set_targets_global(m.h, None) == -1
    _one_good_fit(root, X, y)
    print("refusals: -3 (N), -4 (empty leaf, named), -3 (list-built model); a good fit after each")


# ------------------------------------------------------------------------------------ 8. the reference-named route
def test_the_reference_named_calls_take_the_tree_route(golden):
    g, m = golden("bsp_2d.npz"), golden("mixgp_2d.npz")
    X, levels, y = np.ascontiguousarray(g["X"]), int(g["levels"]), np.ascontiguousarray(m["y"])
    eps, radius, delta, sigma2 = float(g["eps"]), float(g["radius"]), float(g["delta"]), float(m["sigma2"])
    th, wth = pmk.Spline34KernelType(float(m["a"])), pmk.Spline34KernelType(1 / radius)
    root, _, _ = pmk.setuppartition(X, levels)
    X_set, X_set_inds, _, _ = pmk.organizetrainingsets(root, levels, X, eps)
    ref = pmk.MixtureGPType(X_set, pmk.fetchhyperplanes(root))
    eta = pmk.MixtureGPType.from_tree(root, X, eps=eps, hps=pmk.fetchhyperplanes(root))
    handle = eta._model.h.value
    for k, yk in enumerate((y, y[::-1].copy() + 0.5)):     # a second fit with new targets refits the resident model
        pmk.fitmixtureGP_(ref, [yk[i] for i in X_set_inds], th, sigma2)
        pmk.fitmixtureGP_(eta, yk, th, sigma2)
        assert eta._model.h.value == handle
        assert len(eta.c_set) == len(ref.c_set)
        for ca, cb in zip(eta.c_set, ref.c_set):
            assert same_bits(ca, cb), k
        assert eta.sigma2_set == ref.sigma2_set
        assert same_bits(eta.L_set[0], ref.L_set[0])
        Yr, Vr, _ = pmk.querymixtureGP(g["Xq"], ref, root, levels, radius, delta, th, sigma2, wth)
        Yt, Vt, _ = pmk.querymixtureGP(g["Xq"], eta, root, levels, radius, delta, th, sigma2, wth)
        assert same_bits(Yt, Yr) and same_bits(Vt, Vr), k
    for xa, xb in zip(eta.X_parts, X_set):
        assert same_bits(xa, xb)
    assert np.linalg.norm(np.concatenate(ref.c_set) - np.concatenate(eta.c_set)) == 0
    # the multi-output and the per-patch fits take the global targets on such an eta as well
    Y = np.asfortranarray(np.stack([y, 0.5 * y + 1.0], 1))
    pmk.fitmixtureGP_multi_(ref, [Y[i] for i in X_set_inds], th, sigma2)
    pmk.fitmixtureGP_multi_(eta, Y, th, sigma2)
    for ca, cb in zip(eta.C_set, ref.C_set):
        assert same_bits(ca, cb)
    P = len(X_set)
    ths, s2s = [pmk.Spline34KernelType(float(m["a"]) * (1 + 0.1 * r)) for r in range(P)], [sigma2 * (1 + r) for r in range(P)]
    pmk.fitmixtureGP_patches_(ref, [y[i] for i in X_set_inds], ths, s2s)
    pmk.fitmixtureGP_patches_(eta, y, ths, s2s)
    assert eta._model.h.value == handle
    for ca, cb in zip(eta.c_set, ref.c_set):
        assert same_bits(ca, cb)
    print("MixtureGPType.from_tree: c_set, Yq, Vq identical with the list route; one model handle for every fit")

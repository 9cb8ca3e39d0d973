"""GPU tests of the predict path (plan kernel K5, prefix scan, counting sort, strip tasks, strip kernel K4, mix K6, the
multi-output item means) at the sizes where it changes code path, which the benchmark-shaped tests elsewhere do not
reach:

  A. deep trees: plan_kernel<D, *, LDS = false> (P - 1 > PLAN_LDS_NODES), the largest LDS sort (P = SORT_LDS_BINS,
     blocks of more than 1024 items), the global-histogram sort (P > SORT_LDS_BINS), a one-hyperplane tree (P = 2),
     and thousands of strip tasks over many rounds;
  B. D = 4 through plan, sort, strips, mix and item_means_kernel<4, *>, with the largest LDS tree (2047 nodes);
  C. the plan's distance decision sqrt(s) < radius inside and outside its +-2^-50 band around radius^2, and the
     radius <= 0, NaN and >= 1e150 branches (which also make the fill pass re-walk instead of copying its staged hits);
  D. scan_offsets_kernel's carry across its 256-entry passes (more than 256 blocks of SCAN_BLOCK offsets);
  E. the strip kernel on one region: idle waves, last_pairs 1..4 for the Spline34 and the generic instantiation, a
     one-task last round, and bits that do not depend on the strip, round or lock-step group an item lands in.

Every test first asserts that it reached its branch: the thresholds are read from the HIP sources, and the host rules
that pick a branch are restated in tests/_query_refs.py, which asserts that the restated device code is unchanged.

References: the CPU oracle (oracle/oracle.py), numpy and scipy, in fp64.  Integer outputs (home leaf, item offsets, item
regions, t) are bit-exact.  fp64 values against the oracle's own fits use the SURVEY section 8(d) bounds of
tests/test_gpu_parity.py; per-item values against queryinner! on the device's own factors use the bounds of
tests/test_gpu_family_parity.py::test_predict_strip_parity_matrix, with kappa(U) eps32 <= 1e-3 asserted per patch in fp32.
"""
import math

import numpy as np
import pytest
import torch

import patchmixturekriging_amd as pmk
from patchmixturekriging_amd import mixture as M
from oracle import oracle as O

import _query_refs as R

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)


def _num_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _targets(X):
    return np.sin(3 * X[:, 0]) * np.cos(2 * X[:, 1]) + 0.5 * X[:, -1] ** 2


# ------------------------------------------------------------------------------------ A. deep trees
A_LEVELS = [2, 13, 14, 15]
A_SIGMA2, A_DELTA, A_NQ = 1e-3, 1e-7, 20000
A_TH, A_OTH = pmk.Spline34KernelType(4.0), O.kernel(O.SPLINE34, 4.0)
_A = {}


def _deep_case(levels):
    """24 points per leaf, uniform in [-1, 1]^2; the weight kernel's radius is 0.3 x the leaf width 2 / sqrt(P)"""
    if levels in _A:
        return _A[levels]
    P = 2 ** (levels - 1)
    rng = np.random.Generator(np.random.PCG64(400 + levels))
    X = rng.uniform(-1, 1, (24 * P, 2))
    y = _targets(X)
    root, X_parts, inds = pmk.setuppartition(X, levels)
    assert len(X_parts) == P and all(len(x) == 24 for x in X_parts)
    Xq = rng.uniform(-1, 1, (A_NQ, 2))
    _A[levels] = dict(P=P, X=X, root=root, X_parts=X_parts, ys=[y[i] for i in inds], Xq=Xq, radius=0.6 / math.sqrt(P))
    return _A[levels]


@pytest.mark.timeout(600)
@pytest.mark.parametrize("levels", A_LEVELS)
def test_deep_tree_every_query_against_oracle(levels):
    """levels 2, 13, 14, 15 (P = 2, 4096, 8192, 16384): the one-hyperplane tree, the global-memory plan kernel, the
    largest LDS sort and the global-histogram sort.  Home, item offsets, regions and t of EVERY query bit for bit
    against the oracle's querymixtureGP!, and Yq / Vq at the fp64 bounds on the oracle's own fits"""
    c = _deep_case(levels)
    P, radius = c["P"], c["radius"]
    if levels == 2:
        assert P - 1 == 1                                           # one hyperplane
    else:
        assert P - 1 > R.PLAN_LDS_NODES                             # plan_kernel<2, *, LDS = false>
    if levels == 14:
        assert P == R.SORT_LDS_BINS and R.sort_block_items(P) > 1024    # sort_hist_lds_kernel at its largest
    if levels == 15:
        assert P > R.SORT_LDS_BINS                                  # sort_hist_kernel + memset
    ob = O.BSP(c["X"], levels)
    assert ob.P == P
    wth, owth = pmk.Spline34KernelType(1 / radius), O.kernel(O.SPLINE34, 1 / radius)
    m = pmk.DeviceModel(c["X_parts"], c["ys"]); m.fit(A_TH, A_SIGMA2); m.set_bsp(c["root"], 0)
    assert np.all(m.info() == 0)
    q = pmk.DeviceQuery(m, c["Xq"]); total = q.plan(radius, A_DELTA); q.items(A_TH); q.mix(wth)
    Yq, Vq = q.fetch()
    dbg = q.debug()
    counts = np.diff(q.region_offsets(P))
    assert counts.sum() == total
    tasks = R.strip_tasks(counts)
    if levels > 2:                                                  # small strip tasks over many rounds
        assert len(tasks) > 8 * _num_cu() and max(tasks) < R.TQ // 2, (len(tasks), max(tasks))
    fits = R.oracle_fits(A_OTH, c["X_parts"], c["ys"], A_SIGMA2)
    oY, oV, ohome, ooff, oreg, ots = R.oracle_mixture(ob, A_OTH, owth, c["X_parts"], fits, c["Xq"], radius, A_DELTA)
    print("levels %d: %d items (%.2f per query), %d strip tasks (%d of <= 3 columns), max |dY| %.2e"
          % (levels, total, total / A_NQ, len(tasks), sum(1 for t in tasks if t <= 3), np.abs(Yq - oY).max()))
    R.assert_plan_matches(dbg, ohome, ooff, oreg, ots, "levels %d" % levels)
    R.assert_fp64_values(Yq, Vq, oY, oV, "levels %d" % levels)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("levels", [14, 15])
def test_item_sort_is_stable_on_deep_trees(levels):
    """the counting sort at P = SORT_LDS_BINS (LDS histograms, blocks of 2P items) and above it (global histograms):
    explicit items with random regions and x = the item's own index come back in np.argsort(kind="stable") order"""
    c = _deep_case(levels)
    P = c["P"]
    assert (P == R.SORT_LDS_BINS) if levels == 14 else (P > R.SORT_LDS_BINS)
    m = pmk.DeviceModel(c["X_parts"], c["ys"]); m.fit(pmk.Spline34KernelType(2.0), 1e-3); m.set_bsp(c["root"], 0)
    rng = np.random.Generator(np.random.PCG64(99 + levels))
    n = 100003
    assert n > 2 * R.sort_block_items(P)                            # several blocks of the sort
    reg = rng.integers(0, P, n).astype(np.int32)
    xs = np.stack([np.arange(n, dtype=np.float64), np.zeros(n)], axis=1)
    q = pmk.DeviceQuery.from_items(m, n, xs.ctypes.data, reg.ctypes.data)
    off = q.region_offsets(P)
    assert np.array_equal(np.diff(off), np.bincount(reg, minlength=P))
    xo = torch.empty((n, 2), dtype=torch.float64, device="cuda")
    ro = torch.empty(n, dtype=torch.int32, device="cuda")
    q.export_requests(0, n, xo.data_ptr(), ro.data_ptr())
    pmk.default_context().synchronize()
    order = xo[:, 0].cpu().numpy().astype(np.int64)
    assert np.array_equal(order, np.argsort(reg, kind="stable"))
    assert np.array_equal(ro.cpu().numpy(), reg[order])


# ------------------------------------------------------------------------------------ B. D = 4
# name -> (N, levels, eps, radius, queries)
B_CASES = {"ragged": (8000, 6, 0.3, 0.4, 3000), "lds2047": (40960, 12, 0.0, 0.15, 3000)}
B_KERNELS = {"spline34": (pmk.Spline34KernelType(1.0), O.kernel(O.SPLINE34, 1.0)),
             "spline32": (pmk.Spline32KernelType(1.0), O.kernel(O.SPLINE32, 1.0))}
B_SIGMA2, B_DELTA = 0.05, 1e-7
_B, _BF = {}, {}


def _d4_case(case, dot_mode):
    key = (case, dot_mode)
    if key in _B:
        return _B[key]
    N, levels, eps, radius, nq = B_CASES[case]
    rng = np.random.Generator(np.random.PCG64(500 + levels))
    X = rng.uniform(-2, 2, (N, 4))
    y = _targets(X)
    root, _, _ = pmk.setuppartition(X, levels, dot_mode=dot_mode)
    X_set, inds, _, _ = pmk.organizetrainingsets(root, levels, X, eps)
    Xq = rng.uniform(-2, 2, (nq, 4))
    Xq[:5] = X_set[0][:5]                                           # at training points: variance at the floor
    _B[key] = dict(X=X, levels=levels, radius=radius, root=root, X_set=X_set, inds=inds, ys=[y[i] for i in inds], Xq=Xq,
                   ob=O.BSP(X, levels, dot_mode=dot_mode))
    return _B[key]


def _d4_oracle(case, dot_mode, kern):
    """the oracle's fits and querymixtureGP! of one (case, dot mode, fit kernel)"""
    key = (case, dot_mode, kern)
    if key not in _BF:
        c = _d4_case(case, dot_mode)
        oth, radius = B_KERNELS[kern][1], c["radius"]
        fits = R.oracle_fits(oth, c["X_set"], c["ys"], B_SIGMA2)
        _BF[key] = R.oracle_mixture(c["ob"], oth, O.kernel(O.SPLINE34, 1 / radius), c["X_set"], fits, c["Xq"], radius,
                                    B_DELTA)
    return _BF[key]


def _d4_preconditions(case, c):
    P = len(c["X_set"])
    if case == "lds2047":
        assert P - 1 == R.PLAN_LDS_NODES                            # plan_kernel<4, *, true>: the largest LDS tree
    else:
        nts = {-(-len(x) // R.TILE) for x in c["X_set"]}
        assert len(nts) >= 3 and min(nts) >= 4, nts                 # ragged patches of several block rows
        assert len({R.last_pairs(len(x)) for x in c["X_set"]}) >= 3


@pytest.mark.timeout(300)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("dot_mode", [0, 1])
@pytest.mark.parametrize("kern", list(B_KERNELS))
@pytest.mark.parametrize("case", list(B_CASES))
def test_d4_mixture_against_oracle(case, kern, dot_mode, dtype):
    """D = 4, both strip instantiations (Spline34 and generic), both dot modes: integer outputs bit for bit against the
    oracle in both dtypes; fp64 Yq / Vq against the oracle's own fits; fp32 items against queryinner! on the device's own
    fp32 factors, blended with the device's weights (the weights themselves against the Spline34 profile)"""
    c = _d4_case(case, dot_mode)
    _d4_preconditions(case, c)
    th, oth = B_KERNELS[kern]
    radius, X_set = c["radius"], c["X_set"]
    owth = O.kernel(O.SPLINE34, 1 / radius)
    m = pmk.DeviceModel(X_set, c["ys"], dtype=dtype); m.fit(th, B_SIGMA2); m.set_bsp(c["root"], 0)
    assert np.all(m.info() == 0)
    q = pmk.DeviceQuery(m, c["Xq"]); q.plan(radius, B_DELTA); q.items(th); q.mix(pmk.Spline34KernelType(1 / radius))
    Yq, Vq = q.fetch()
    dbg = q.debug()
    oY, oV, ohome, ooff, oreg, ots = _d4_oracle(case, dot_mode, kern)
    R.assert_plan_matches(dbg, ohome, ooff, oreg, ots, "%s %s dot %d %s" % (case, kern, dot_mode, dtype))
    off = dbg["item_offsets"]
    nb = np.ones(off[-1], bool); nb[off[1:] - 1] = False
    wref = np.array([1.0 if not b else O.profile(owth, abs(t)) for b, t in zip(nb, dbg["item_t"])])
    assert np.abs(dbg["item_w"] - wref).max() <= 1e-15
    if dtype == "f64":
        R.assert_fp64_values(Yq, Vq, oY, oV, "%s %s dot %d" % (case, kern, dot_mode))
        return
    u_ref, v_ref = np.empty(off[-1]), np.empty(off[-1])
    kmax = 0.0
    for r in np.unique(dbg["item_region"]):
        idx = np.nonzero(dbg["item_region"] == r)[0]
        qj = np.searchsorted(off, idx, side="right") - 1
        k = R.kappa(O.kernel_matrix(oth, X_set[r]) + B_SIGMA2 * np.eye(len(X_set[r])))
        assert k * EPS32 <= 1e-3, (r, k)
        kmax = max(kmax, k)
        cr, L = m.get(int(r), M.GET_C), m.get(int(r), M.GET_L)
        mu, var, msc, vsc = R.queryinner_reference(oth, X_set[r], cr, L, c["Xq"][qj])
        u_ref[idx], v_ref[idx] = mu, var
        du, dv = np.abs(dbg["item_u"][idx] - mu), np.abs(dbg["item_v"][idx] - var)
        assert np.all(du <= 50 * np.sqrt(k) * EPS32 * (msc + 1)), (r, du.max())
        assert np.all(dv <= 50 * k * EPS32 * (vsc + 1)), (r, dv.max())
    Y, V = R.blend_reference(dbg, u_ref, v_ref)
    assert np.all(np.abs(Yq - Y) <= 50 * kmax * EPS32 * np.maximum(1, np.abs(Y)))
    assert np.all(np.abs(Vq - V) <= 50 * kmax * EPS32 * (V + 1e-3))
    print("%s %s dot %d f32: max kappa eps32 %.2e" % (case, kern, dot_mode, kmax * EPS32))


@pytest.mark.timeout(300)
@pytest.mark.parametrize("dot_mode", [0, 1])
@pytest.mark.parametrize("kern", list(B_KERNELS))
@pytest.mark.parametrize("case", list(B_CASES))
def test_d4_multi_output_means_against_oracle(case, kern, dot_mode):
    """R = 3 target columns, mean only (item_means_kernel<4, *>): every column against the oracle's querymixtureGP! on
    the oracle's fits of that column, at 1e-7 max(1, |Yq|)"""
    c = _d4_case(case, dot_mode)
    _d4_preconditions(case, c)
    th, oth = B_KERNELS[kern]
    radius, X_set, X = c["radius"], c["X_set"], c["X"]
    Y = np.stack([_targets(X), np.cos(X[:, 1] - X[:, 2]), 0.3 * X[:, 3] - 0.1], 1)
    Ys = [Y[i] for i in c["inds"]]
    eta = pmk.MixtureGPType(X_set, pmk.fetchhyperplanes(c["root"]))
    pmk.fitmixtureGP_multi_(eta, Ys, th, B_SIGMA2)
    Yq, Vq = pmk.querymixtureGP_multi(c["Xq"], eta, c["root"], c["levels"], radius, B_DELTA, th, B_SIGMA2,
                                      pmk.Spline34KernelType(1 / radius), variance=False)
    assert Vq is None and Yq.shape == (len(c["Xq"]), 3)
    for j in range(3):
        fits = R.oracle_fits(oth, X_set, [y[:, j].copy() for y in Ys], B_SIGMA2)
        oY = R.oracle_mixture(c["ob"], oth, O.kernel(O.SPLINE34, 1 / radius), X_set, fits, c["Xq"], radius, B_DELTA)[0]
        bad = np.nonzero(~(np.abs(Yq[:, j] - oY) <= 1e-7 * np.maximum(1, np.abs(oY))))[0]      # NaN is out of bounds
        assert len(bad) == 0, "column %d: %d queries, first %d: %r vs oracle %r" % (j, len(bad), bad[0], Yq[bad[0], j],
                                                                                    oY[bad[0]])


# ------------------------------------------------------------------------------------ C. the distance decision
C_CASES = [(2, 0), (2, 1), (3, 0), (3, 1)]
C_LEVELS, C_DELTA, C_NQ, C_DESIGNATED = 6, 1e-7, 2000, 16


def _step(x, k):
    for _ in range(abs(k)):
        x = np.nextafter(x, np.inf if k > 0 else -np.inf)
    return float(x)


def _designated(ob, Xq):
    """queries whose nearest accepted plane lies at d = sqrt(s) (s: the oracle's sequential sum of squares); the radii
    nextafter^k(d), k = -6..6, cross both edges of the plan's band r^2 (1 -+ 2^-50).  Half of them are queries where
    fl(r r) > s at some k <= 0: sqrt(s) >= r there, yet the shortcut s < r^2 would accept the plane"""
    ks = list(range(-6, 7))
    picked = {True: [], False: []}
    for j in range(len(Xq)):
        h = ob.findpartition(Xq[j])
        _, _, zs, keep = ob.neighbours(Xq[j], 1e300, C_DELTA, h)
        if not keep.any():
            continue
        s = min(R.seq_sumsq(zs[i], Xq[j]) for i in np.nonzero(keep)[0])
        d = math.sqrt(s)
        radii = [_step(d, k) for k in ks]
        misjudged = any(r * r > s for r, k in zip(radii, ks) if k <= 0)
        if len(picked[misjudged]) >= C_DESIGNATED // 2:
            continue
        cnt = [len(ob.neighbours(Xq[j], r, C_DELTA, h)[0]) for r in radii]
        # precondition: this query's neighbour count changes exactly between k = 0 and k = 1
        assert len(set(cnt[:7])) == 1 and len(set(cnt[7:])) == 1 and cnt[7] > cnt[6], (j, cnt)
        picked[misjudged].append((j, radii))
        if all(len(v) >= C_DESIGNATED // 2 for v in picked.values()):
            break
    return picked


@pytest.mark.timeout(300)
@pytest.mark.parametrize("D,dot_mode", C_CASES)
def test_plan_distance_decision_at_the_band_and_the_extremes(D, dot_mode):
    """radius = nextafter^k(d) around the distance d of designated queries to their nearest accepted plane, then
    radius in {0, -1, NaN, inf, 1e151}: home, offsets, regions and t of ALL queries bit for bit against the oracle.  The
    last two send every plane through the across test; in 3-D some query then has more than PLAN_STAGE neighbours, and
    the fill pass re-walks the planes instead of copying its staged hits"""
    rng = np.random.Generator(np.random.PCG64(600 + 10 * D + dot_mode))
    X = rng.uniform(-1, 1, (32 * 40, D))
    root, X_parts, inds = pmk.setuppartition(X, C_LEVELS, dot_mode=dot_mode)
    ob = O.BSP(X, C_LEVELS, dot_mode=dot_mode)
    y = np.sin(3 * X.sum(1))
    m = pmk.DeviceModel(X_parts, [y[i] for i in inds]); m.fit(pmk.Spline34KernelType(2.0), 1e-3); m.set_bsp(root, 0)
    assert np.all(m.info() == 0)
    Xq = rng.uniform(-1, 1, (C_NQ, D))
    picked = _designated(ob, Xq)
    assert len(picked[True]) >= 4 and len(picked[True]) + len(picked[False]) >= C_DESIGNATED, \
        {k: len(v) for k, v in picked.items()}
    q = pmk.DeviceQuery(m, Xq)
    for j, radii in picked[True] + picked[False]:
        for k, r in zip(range(-6, 7), radii):
            q.plan(r, C_DELTA)
            R.assert_plan_matches(q.debug(), *R.oracle_plan(ob, Xq, r, C_DELTA), what="query %d k %d radius %r" % (j, k, r))
    widest = q.plan(max(max(radii) for _, radii in picked[True] + picked[False]), C_DELTA)
    for r in (0.0, -1.0, float("nan"), float("inf"), 1e151):
        total = q.plan(r, C_DELTA)
        dbg = q.debug()
        R.assert_plan_matches(dbg, *R.oracle_plan(ob, Xq, r, C_DELTA), what="radius %r" % r)
        cnt = np.diff(dbg["item_offsets"]) - 1
        if not r > 0:
            assert total == C_NQ and np.all(cnt == 0)                      # home-only items
        else:
            assert total > widest                                          # every plane passes the distance test
            if D == 3:                                                     # a query with more hits than the stage
                assert cnt.max() > R.PLAN_STAGE, cnt.max()                 # holds: the fill pass re-walks the planes


# ------------------------------------------------------------------------------------ D. the prefix scan
@pytest.mark.timeout(600)
def test_prefix_scan_carries_across_its_passes():
    """Nq = 524287, 524288, 1100000 at levels 6: 256, 257 and 538 blocks of the scan, i.e. one full pass of
    scan_offsets_kernel, one carry, two carries.  Item offsets of EVERY query exactly, homes and regions bit for bit,
    Yq / Vq at the fp64 bounds"""
    NQS = [524287, 524288, 1100000]
    nbs = [R.scan_blocks(n) for n in NQS]
    assert nbs[0] == R.SCAN_PASS and nbs[1] == R.SCAN_PASS + 1 and nbs[2] > 2 * R.SCAN_PASS, nbs
    levels, sigma2, delta = 6, 1e-3, 1e-7
    P = 2 ** (levels - 1)
    radius = 0.6 / math.sqrt(P)
    rng = np.random.Generator(np.random.PCG64(700))
    X = rng.uniform(-1, 1, (64 * P, 2))
    y = _targets(X)
    root, X_parts, inds = pmk.setuppartition(X, levels)
    ys = [y[i] for i in inds]
    Xq = rng.uniform(-1, 1, (NQS[-1], 2))
    ob = O.BSP(X, levels)
    wth, owth = pmk.Spline34KernelType(1 / radius), O.kernel(O.SPLINE34, 1 / radius)
    fits = R.oracle_fits(A_OTH, X_parts, ys, sigma2)
    oY, oV, ohome, ooff, oreg, ots = R.oracle_mixture(ob, A_OTH, owth, X_parts, fits, Xq, radius, delta)
    m = pmk.DeviceModel(X_parts, ys); m.fit(A_TH, sigma2); m.set_bsp(root, 0)
    assert np.all(m.info() == 0)
    for n in NQS:                                # a query's oracle outputs do not depend on the batch: prefixes
        q = pmk.DeviceQuery(m, Xq[:n]); q.plan(radius, delta); q.items(A_TH); q.mix(wth)
        Yq, Vq = q.fetch()
        e = ooff[n]
        R.assert_plan_matches(q.debug(), ohome[:n], ooff[:n + 1], oreg[:e], ots[:e], "Nq %d" % n)
        R.assert_fp64_values(Yq, Vq, oY[:n], oV[:n], "Nq %d" % n)
        del q


# ------------------------------------------------------------------------------------ E. strips on one region
E_SIZES = [1, 128, 200, 230, 700]
E_NQ = [1, 31, 32, 33, 63, 64, 65, 224, 225, 255, 256, 257, 511, 512, 513, 769]
E_FAMS = {"spline34": (pmk.Spline34KernelType(1.0), O.kernel(O.SPLINE34, 1.0)),
          "gaussian": (pmk.GaussianKernel1DType(4.0), O.kernel(O.GAUSSIAN, 4.0))}
E_SIGMA2 = 0.05


def _check_items(dtype, k, mu, var, ref, what):
    mref, vref, msc, vsc = ref
    if dtype == "f64":
        assert np.all(np.abs(mu - mref) <= 1e-9 * np.maximum(1, np.abs(mref))), (what, np.abs(mu - mref).max())
        assert np.all(np.abs(var - vref) <= 1e-9 + 1e-5 * vref), (what, np.abs(var - vref).max())
    else:
        assert np.all(np.abs(mu - mref) <= 50 * np.sqrt(k) * EPS32 * (msc + 1)), (what, np.abs(mu - mref).max())
        assert np.all(np.abs(var - vref) <= 50 * k * EPS32 * (vsc + 1)), (what, np.abs(var - vref).max())


@pytest.mark.timeout(600)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("fam", list(E_FAMS))
def test_strip_scheduling_on_one_region(fam, dtype):
    """DeviceModel.queryinner on patches whose last block row has 1, 4, 3, 4 and 2 live 32-row pairs, with query counts
    around the WCOLS-column wave and the TQ-column strip (partly and wholly idle waves, evenly dealt strips), and
    TQ num_cu + 1 queries (num_cu full strips and a one-column task alone in a second round): every item against
    queryinner! on the device's own factors.  Then the bits of an item must not depend on the strip, round or lock-step
    group it lands in: the big batch queried again as single points and odd-sized chunks"""
    th, oth = E_FAMS[fam]
    ncu = _num_cu()
    assert [R.last_pairs(n) for n in E_SIZES] == [1, 4, 3, 4, 2]
    tasks = [R.strip_counts(nq) for nq in E_NQ]
    assert any(t % R.WCOLS != 0 for ts in tasks for t in ts)               # a partly idle wave
    assert any(t <= R.TQ - 2 * R.WCOLS for ts in tasks for t in ts)        # wholly idle waves
    assert any(len(ts) > 1 for ts in tasks)                                 # a region dealt over several strips
    big = R.TQ * ncu + 1
    bt = R.strip_counts(big)
    assert len(bt) == ncu + 1 and bt[-1] == 1, (len(bt), bt[-1])            # one 1-column task in a round of its own
    rng = np.random.Generator(np.random.PCG64(800 + len(fam)))
    Xs = [rng.uniform(-2, 2, (n, 2)) for n in E_SIZES]
    ys = [_targets(x) for x in Xs]
    m = pmk.DeviceModel(Xs, ys, dtype=dtype); m.fit(th, E_SIGMA2)
    assert np.all(m.info() == 0)
    for r, X in enumerate(Xs):
        k = R.kappa(O.kernel_matrix(oth, X) + E_SIGMA2 * np.eye(len(X)))
        assert k * EPS32 <= 1e-3, k
        c, L = m.get(r, M.GET_C), m.get(r, M.GET_L)
        for nq in E_NQ:
            Xq = rng.uniform(-2, 2, (nq, 2))
            Xq[0] = X[0]                                                    # at a training point: variance at the floor
            mu, var = m.queryinner(r, th, Xq)
            _check_items(dtype, k, mu, var, R.queryinner_reference(oth, X, c, L, Xq), (len(X), nq))
        if len(X) != 230:
            continue
        Xq = rng.uniform(-2, 2, (big, 2))
        mu, var = m.queryinner(r, th, Xq)
        _check_items(dtype, k, mu, var, R.queryinner_reference(oth, X, c, L, Xq), (len(X), big))
        at = 0
        for size in [1, 1, 1, 7, 31, 33, 65, 255, 257, 513, 1, 2049]:
            mu1, var1 = m.queryinner(r, th, Xq[at:at + size])
            assert np.array_equal(mu1, mu[at:at + size]) and np.array_equal(var1, var[at:at + size]), (at, size)
            at += size
        mu1, var1 = m.queryinner(r, th, Xq[-1:])                           # the item of the one-column last round
        assert np.array_equal(mu1, mu[-1:]) and np.array_equal(var1, var[-1:])

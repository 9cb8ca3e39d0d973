"""GPU tests of the model-selection path at its SCHEDULING and GEOMETRY edges (csrc/pmk_loo.hip): the (patch, strip) tasks
of loo_strip_kernel and their eight queues, the strip workspace a workgroup reuses for its next task, the second half of
a strip that starts one block row later, the 128-column last strip of an odd tile count, the 32-row pairs of the last
block row, evidence_kernel<16> and loo_values_kernel<16> at their 16-row stride, and the state selectmixtureGP_ carries
from one candidate to the next.

  A. Exact factors through DeviceModel.from_factors (fp64): L whose inverse has small integer entries, so that
     d = diag((L L^T)^-1) is known EXACTLY whatever the summation order -- no reference computation at all.
       dense: L = the all-ones lower triangle, L^-1 = I - S (S the down-shift), d = 2, 2, .., 2, 1
       shift: L = I - S, L^-1 = the all-ones lower triangle, d_j = n - j (every column names itself)
     var = 1 / d and res = c / d are compared bit for bit with numpy's IEEE division.
  B. Fitted pools, fp64 and fp32: column j of L^-1 is computed by one wave in a fixed order, so a patch's scores are
     bit-identical whatever batch it sits in, whatever queue its tasks land in and whichever workgroup runs them; and every
     patch of the pool meets max_i |d_i - d*_i| / d*_i <= n u against LAPACK trtri on the device's own factor.
  C. evidence_multi and loo_values_multi for every R = 1..16 at n = 1, 15, 16, 17, 255, 256, 257, 300.
  D. selectmixtureGP_: every row of its scores against a fresh model fitted at that candidate alone, with a candidate in
     the middle that fails on one patch.

tests/_loo_schedule.py mirrors build_loo_tasks; it holds the inputs of this file and says which branch each of them drives
(proved on the CPU by tests/test_loo_schedule_model.py for 256 CUs, recomputed here for the device at hand).  Every
figure is printed as a `measured {json}` line before it is asserted.
"""
import json
import time

import numpy as np
import pytest
import torch

import patchmixturekriging_amd as pmk
from patchmixturekriging_amd import mixture as M

import _loo_refs as LR
import _loo_schedule as S
from test_gpu_fit_schedule import A_COMBOS

pytestmark = pytest.mark.gpu

LD = LR.LD


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    t0 = time.perf_counter()
    yield
    print("\ntests/test_gpu_loo_schedule.py: %.1f s wall" % (time.perf_counter() - t0))


def _record(**kw):
    print("measured " + json.dumps(kw))


def _num_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _targets(X):
    return np.sin(3 * X[:, 0]) + X[:, -1] ** 2


# ======================================================================================== A. exact factors
PATTERNS = ("dense", "shift")
_FACTORS = {}


def _factor(n, pattern):
    """(L, d): every intermediate of the sweep is an integer of magnitude <= n, so d is exact in any order"""
    if (n, pattern) not in _FACTORS:
        if pattern == "dense":
            L = np.asfortranarray(np.tril(np.ones((n, n))))
            d = np.full(n, 2.0)
            d[-1] = 1.0
        else:
            L = np.asfortranarray(np.eye(n) - np.eye(n, k=-1))
            d = (n - np.arange(n)).astype(np.float64)
        _FACTORS[(n, pattern)] = (L, d)
    return _FACTORS[(n, pattern)]


def _load(patches, seed):
    """a model from the exact factors of `patches`, a list of (n, pattern), with random weights -> (model, weights)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    cs = [rng.standard_normal(n) for n, _ in patches]
    model = M.DeviceModel.from_factors([np.zeros((n, 2)) for n, _ in patches], cs, [_factor(n, p)[0] for n, p in patches])
    return model, cs


def _check_exact(name, model, patches, cs):
    """var == 1 / d and res == c / d bit for bit for every patch; returns the number of columns checked"""
    res, var = model.loo_values()
    wrong, first = 0, None
    for r, (n, pattern) in enumerate(patches):
        d = _factor(n, pattern)[1]
        bad = np.nonzero(~((var[r] == 1.0 / d) & (res[r] == cs[r] / d)))[0]
        wrong += len(bad)
        if len(bad) and first is None:
            with np.errstate(divide="ignore"):
                first = dict(patch=r, n=n, pattern=pattern, columns=bad[:8].tolist(), d_got=(1.0 / var[r][bad[:8]]).tolist(),
                             d_want=d[bad[:8]].tolist(), bad_columns_of_patch=len(bad))
    sizes = [n for n, _ in patches]
    _record(test="exact", batch=name, patches=len(patches), tasks=len(S.tasks(sizes)[0]), slots=S.slots(sizes, _num_cu()),
            columns=int(sum(sizes)), wrong_columns=wrong, first_wrong=first)
    assert wrong == 0, (name, first)
    for r, (n, pattern) in enumerate(patches):          # the same as whole arrays (1 / var is NOT compared: 1 / (1 / k) != k)
        d = _factor(n, pattern)[1]
        assert np.array_equal(var[r], 1.0 / d) and np.array_equal(res[r], cs[r] / d), (name, r, n, pattern)
    return int(sum(sizes))


A_BATCHES = ["pool", "reversed", "permuted", "prefix7", "prefix8", "prefix9", "deep12_alone", "deep13_alone",
             "deep12_and_seven_small"]


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("batch", A_BATCHES)
def test_exact_factors(batch, pattern):
    sizes = S.exact_batches(_num_cu())[batch]
    print("\n%s: %d patches, branches %s" % (batch, len(sizes), sorted(S.branches(sizes, _num_cu()))))
    patches = [(n, pattern) for n in sizes]
    model, cs = _load(patches, 4100 + len(sizes))
    model.loo()
    _check_exact("%s-%s" % (batch, pattern), model, patches, cs)


def test_exact_factors_with_more_tasks_than_workgroups_and_both_patterns_interleaved():
    """the pool repeated until its tasks are more than 1.5 times the CUs: every workgroup runs a second, shorter task of
    another patch in the strip workspace of its first, and since dense and shift patches alternate (and swap from one
    repeat to the next) the rows it finds there are often the other pattern's"""
    num_cu = _num_cu()
    sizes = S.exact_batches(num_cu)["repeated"]
    npool = len(S.pool_sizes())
    patches = [(n, PATTERNS[(k + k // npool) % 2]) for k, n in enumerate(sizes)]
    ntasks, slots = len(S.tasks(sizes)[0]), S.slots(sizes, num_cu)
    hit = S.branches(sizes, num_cu)
    print("\nrepeated: %d patches, %d tasks on %d workgroups, branches %s" % (len(sizes), ntasks, slots, sorted(hit)))
    assert ntasks >= 1.5 * num_cu and slots == num_cu and "tasks_gt_slots" in hit
    model, cs = _load(patches, 4200)
    model.loo()
    _check_exact("repeated-interleaved", model, patches, cs)


@pytest.mark.parametrize("pattern", PATTERNS)
def test_a_second_pass_over_the_same_model_gives_the_same_bits(pattern):
    """model.loo() twice: the queue counters are reset and the task list, the strip workspace and d are reused"""
    sizes = S.exact_batches(_num_cu())["pool"] + S.deep_sizes()
    patches = [(n, pattern) for n in sizes]
    model, cs = _load(patches, 4300)
    model.loo()
    _check_exact("first-pass-" + pattern, model, patches, cs)
    first = model.loo_values()
    model.loo()
    _check_exact("second-pass-" + pattern, model, patches, cs)
    second = model.loo_values()
    for a, b in zip(first[0] + first[1], second[0] + second[1]):
        assert np.array_equal(a, b)


def test_exact_batches_cover_the_branches_on_this_device():
    """the coverage assertion of tests/test_loo_schedule_model.py with the device's own CU count"""
    num_cu = _num_cu()
    cov = S.coverage(num_cu)
    print("\nnum_cu = %d" % num_cu)
    for b in S.BRANCHES:
        print("    %-36s %d batches, e.g. %s" % (b, len(cov.get(b, [])), cov.get(b, ["-"])[0]))
    assert sorted(cov) == sorted(S.BRANCHES)


# ======================================================================================== B. fitted pools
# a second (theta, sigma2) per precision for the refit: another kernel matrix on the same points
B_SECOND = {"f64": (lambda: pmk.Spline34KernelType(2.0), 1e-4), "f32": (lambda: pmk.Spline34KernelType(0.8), 0.1)}


def _scores(m):
    m.loo()
    res, var = m.loo_values()
    logdet, quad = m.evidence()
    return res, var, logdet, quad


@pytest.mark.timeout(600)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_scores_of_a_patch_do_not_depend_on_its_batch(dtype):
    """Spline34 in 2-D (the fused kernel-matrix path) at the settings of A_COMBOS["spline34-2d"], batched mode forced.
    Bit identity of var, res, logdet and quad of every patch with its solo run in every arrangement, after a refit, and
    beside a patch that cannot be factorised; accuracy of d for every patch of the pool against LAPACK trtri in double on
    the downloaded factor, bound n u (4 u at n = 1).
    Measured on an MI355X: worst ratio to the bound 0.25 in fp64, 0.075 in fp32."""
    (lo, hi), th, _, sigma2, _ = A_COMBOS["spline34-2d"][1][dtype]
    th = th()
    u = LR.unit_roundoff(dtype)
    num_cu = _num_cu()
    sizes = S.fitted_pool_sizes()
    P = len(sizes)
    rng = np.random.Generator(np.random.PCG64(7300))
    Xs = [rng.uniform(lo, hi, (n, 2)) for n in sizes]
    ys = [_targets(x) for x in Xs]
    lib = pmk.default_context().L

    def model_of(idx, X=None):
        m = pmk.DeviceModel([(X or Xs)[i] for i in idx], [ys[i] for i in idx], dtype=dtype)
        assert lib.pmk_test_model_set_split(m.h, 0) == 0
        return m

    guard = (0, P // 2, P - 1)
    solo, solo_L = [], {}
    for i in range(P):
        m = model_of([i])
        m.fit(th, sigma2)
        assert m.info()[0] == 0, (i, sizes[i])
        res, var, logdet, quad = _scores(m)
        solo.append((res[0], var[0], logdet[0], quad[0]))
        if i in guard:
            solo_L[i] = m.get(0, M.GET_L)
    compared = 0

    def compare(name, m, idx, want=None, skip=()):
        nonlocal compared
        want = want or solo
        res, var, logdet, quad = _scores(m)
        for j, i in enumerate(idx):
            if i in skip:
                continue
            for what, got, ref in (("var", var[j], want[i][1]), ("res", res[j], want[i][0]),
                                   ("logdet", logdet[j], want[i][2]), ("quad", quad[j], want[i][3])):
                assert np.array_equal(got, ref), "%s %s: %s of patch %d (n = %d, slot %d of %d) differs from the patch alone" \
                    % (name, dtype, what, i, sizes[i], j, len(idx))
            compared += 1
        return res, var, logdet, quad

    worst = 0.0
    for name, idx in S.fitted_batches(num_cu).items():
        sz = [sizes[i] for i in idx]
        ntasks = len(S.tasks(sz)[0])
        if name == "repeated":
            assert ntasks >= 1.5 * num_cu and "tasks_gt_slots" in S.branches(sz, num_cu)
        m = model_of(idx)
        m.fit(th, sigma2)
        assert np.all(m.info() == 0), name
        _, var, _, _ = compare(name, m, idx)
        _record(test="batch_independence", dtype=dtype, batch=name, patches=len(idx), tasks=ntasks,
                slots=S.slots(sz, num_cu), identical=True)
        if name == "pool":
            for i in guard:                             # the guard of this test: the factor itself is batch-independent
                assert np.array_equal(m.get(i, M.GET_L), solo_L[i]), (i, sizes[i])
            for r, n in enumerate(sizes):
                d = 1.0 / var[r]
                dstar = LR.trtri_colnorms(m.get(r, M.GET_L))
                ratio = float((np.abs(d - dstar) / dstar).max()) / (max(n, 4) * u)
                _record(test="pool_d_vs_trtri", dtype=dtype, patch=r, n=n, ratio_to_max_n_4_u=ratio)
                worst = max(worst, ratio)
                assert ratio <= 1.0, (dtype, r, n, ratio)
    # fit(th1), loo(), fit(th2), loo() on one model against a fresh model at th2
    th2, sigma2_2 = B_SECOND[dtype][0](), B_SECOND[dtype][1]
    everyone = list(range(P))
    fresh = model_of(everyone)
    fresh.fit(th2, sigma2_2)
    assert np.all(fresh.info() == 0)
    fr = _scores(fresh)
    want2 = [(fr[0][i], fr[1][i], fr[2][i], fr[3][i]) for i in range(P)]
    assert not np.array_equal(want2[P - 1][1], solo[P - 1][1])
    m = model_of(everyone)
    m.fit(th, sigma2)
    compare("first fit", m, everyone)
    m.fit(th2, sigma2_2)
    compare("second fit", m, everyone, want=want2)
    # one patch that cannot be factorised (points 0 and 1 coincide, sigma2 = 0 for that patch: pivot 2 is 1 - 1 * 1 = 0 in
    # any precision) at the first, a middle and the last position: NaN in its four outputs, every other patch keeps its bits
    for where, bad in (("first", 0), ("middle", P // 2), ("last", P - 1)):
        assert sizes[bad] >= 2
        Xb = list(Xs)
        Xb[bad] = Xs[bad].copy()
        Xb[bad][1] = Xb[bad][0]
        s2 = [sigma2] * P
        s2[bad] = 0.0
        m = model_of(everyone, Xb)
        m.fit_patches([th] * P, s2)
        info = m.info()
        assert info[bad] == 2 and np.all(np.delete(info, bad) == 0), (where, info)
        res, var, logdet, quad = compare("bad patch " + where, m, everyone, skip=(bad,))
        assert np.all(np.isnan(res[bad])) and np.all(np.isnan(var[bad])) and np.isnan(logdet[bad]) and np.isnan(quad[bad])
        assert len(res[bad]) == len(var[bad]) == sizes[bad]
    _record(test="batch_independence_total", dtype=dtype, patch_scores_compared=compared, worst_d_ratio=worst)
    print("\n%s: %d patch scorings bit-identical to the patch alone; worst d ratio to max(n, 4) u %.3f" % (dtype, compared, worst))


# ======================================================================================== C. evidence and values, R = 1..16
def _ulps(a, b):
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_evidence_and_values_for_every_R_at_row_edges(dtype):
    """one batch of n = 1, 15, 16, 17, 255, 256, 257, 300; R = 16 first, then every R down from 15 on the same model.
    quad against the long-double sum over the device's own Y and C (summation bound); logdet and var bit-identical to the
    single-output calls; RES within 2 ulp of C * var; column j of a run with R columns bit-identical to column j of the
    run with 16.
    Measured on an MI355X: worst quad error / summation bound 0.068 in fp64, 0.025 in fp32; RES at most 1 ulp from C * var."""
    (lo, hi), th, _, sigma2, _ = A_COMBOS["spline34-2d"][1][dtype]
    sizes = S.EVIDENCE_SIZES
    rng = np.random.Generator(np.random.PCG64(7400))
    Xs = [rng.uniform(lo, hi, (n, 2)) for n in sizes]
    Y16 = [np.stack([np.sin((1 + 0.37 * j) * X[:, 0] + 0.2 * j) + (0.1 * j - 0.5) * X[:, 1] for j in range(16)], 1) for X in Xs]
    model = pmk.DeviceModel(Xs, [Y[:, 0].copy() for Y in Y16], dtype=dtype)
    model.fit(th(), sigma2)
    assert np.all(model.info() == 0)
    model.loo()
    _, var1 = model.loo_values()
    logdet1, _ = model.evidence()
    full, worst = None, 0.0
    for R in [16] + list(range(1, 16)):
        model.set_targets_multi([Y[:, :R] for Y in Y16])
        model.solve_multi()
        logdet, quad = model.evidence_multi()
        RES, var = model.loo_values_multi()
        Cs = model.weights_multi()
        assert quad.shape == (len(sizes), R)
        assert np.array_equal(logdet, logdet1), R
        worst_R, ulp_R = 0.0, 0.0
        for r, n in enumerate(sizes):
            assert RES[r].shape == (n, R) and Cs[r].shape == (n, R)
            assert np.array_equal(var[r], var1[r]), (R, n)
            Yd = Y16[r][:, :R].astype(np.float32).astype(np.float64) if dtype == "f32" else Y16[r][:, :R]
            for j in range(R):
                err, bound = LR.summation_error_and_bound(n, quad[r, j], Yd[:, j].astype(LD) * Cs[r][:, j].astype(LD))
                worst_R = max(worst_R, err / bound)
                assert err <= bound, (dtype, R, n, j, err, bound)
                ul = float(_ulps(RES[r][:, j], Cs[r][:, j] * var1[r]).max())
                ulp_R = max(ulp_R, ul)
                assert ul <= 2.0, (dtype, R, n, j, ul)
        _record(test="evidence_values_R", dtype=dtype, R=R, worst_quad_err_over_bound=worst_R, worst_res_ulps=ulp_R)
        worst = max(worst, worst_R)
        if R == 16:
            full = (quad.copy(), [a.copy() for a in RES], [c.copy() for c in Cs])
        else:
            assert np.array_equal(quad, full[0][:, :R]), R
            for r in range(len(sizes)):
                assert np.array_equal(RES[r], full[1][r][:, :R]), (R, sizes[r])
                assert np.array_equal(Cs[r], full[2][r][:, :R]), (R, sizes[r])
    print("\n%s: worst quad error / summation bound %.4f" % (dtype, worst))


# ======================================================================================== D. the selection loop
def _selection_inputs():
    sizes = [300, 130, 257, 1, 200, 128, 97, 33, 256, 65]
    rng = np.random.Generator(np.random.PCG64(7500))
    Xs = [rng.uniform(0, 1, (n, 2)) for n in sizes]
    bad = 4
    Xs[bad][1] = Xs[bad][0]                            # with sigma2 = 0 pivot 2 of this patch is 1 - 1 * 1 = 0
    ys = [_targets(x) for x in Xs]
    cands = [(pmk.Spline34KernelType(3.0), 1e-3), (pmk.Spline32KernelType(3.0), 1e-4), (pmk.Spline34KernelType(6.0), 0.0),
             (pmk.RationalQuadraticKernelType(0.5), 1e-2), (pmk.Spline12KernelType(2.0), 1e-3)]
    return sizes, Xs, ys, cands, bad


@pytest.mark.parametrize("score", ["evidence", "loo"])
def test_selection_loop_scores_each_candidate_as_a_fresh_model_does(score):
    """five candidates of four families on ten ragged patches; the third has sigma2 = 0 and fails on the patch with a
    duplicated point.  One model is fitted five times by selectmixtureGP_ and reuses its task list, queue counters, strip
    workspace and d: every row of the scores must be what a fresh model gives, NaN at (candidate 3, that patch) only."""
    sizes, Xs, ys, cands, bad = _selection_inputs()
    P = len(sizes)
    want = np.empty((len(cands), P))
    for g, (th, s2) in enumerate(cands):
        m = pmk.DeviceModel(Xs, ys)
        m.fit(th, s2)
        info = m.info()
        assert np.all(np.delete(info, bad) == 0) and (info[bad] == 2 if g == 2 else info[bad] == 0), (g, info)
        if score == "evidence":
            logdet, quad = m.evidence()
            want[g] = -0.5 * quad - 0.5 * logdet - 0.5 * m.n * np.log(2.0 * np.pi)
        else:
            m.loo()
            res, var = m.loo_values()
            with np.errstate(invalid="ignore", divide="ignore"):
                want[g] = [M.loo_log_pseudo_likelihood(a, b) for a, b in zip(res, var)]
    nan = np.isnan(want)
    assert nan[2, bad] and nan.sum() == 1, np.argwhere(nan).tolist()
    eta = pmk.MixtureGPType(Xs, None)
    _, winners, scores = pmk.selectmixtureGP_(eta, ys, cands, score=score)
    differ = np.argwhere(~((scores == want) | (np.isnan(scores) & nan))).tolist()
    _record(test="selection_loop", score=score, candidates=len(cands), patches=P, cells_that_differ=differ,
            nan_cells=np.argwhere(np.isnan(scores)).tolist())
    assert np.array_equal(scores, want, equal_nan=True), differ
    assert np.array_equal(np.argwhere(np.isnan(scores)), [[2, bad]])
    assert np.all(np.isfinite(scores[3:, bad]))
    assert np.array_equal(winners, pmk.select_candidates(want))
    assert winners[bad] != 2

"""GPU tests of the fit path's SCHEDULING (launch_cholesky and launch_split_solves in csrc/pmk_chol.hip): end-aligned
block columns, the active prefix of the sorted patches, step_slot's deal over the XCDs and its padded grid, the split
path's chunk counts, the pending diagonal tile and the buffer half it is read from, the fold workgroups, and the choice
between chained and block-by-block solves.

  A. Batched path: a patch's factor, inverted diagonal blocks, weights and status word do not depend on which other
     patches share its batch -- bit for bit, over a pool of 40 ragged patches fitted alone, together, reversed, permuted,
     in prefixes on both sides of 8 and 16 slots and beside the largest patch only; with a non-positive-definite patch
     planted at the first, the middle and the last slot.  This is what "the sharded result is bit-identical to the
     single-model result"  rests on.  Every patch of the full pool is also held to the project's fit bounds.
  B. Split path: the same comparison.  Among batches of EQUAL max_nt the factor is bit-identical (a patch of nt tiles
     runs its block column k at launch l = k + max_nt - nt, and the chunk count is a function of l); across different
     max_nt the chunks, hence the summation order, differ and the factors agree to the bound the project already uses for
     "same tiles, other summation order".
  C. Split-scheduling edges against LAPACK and against the batched path, in all four modes of pmk_test_model_set_split.

tests/_fit_schedule.py mirrors the host schedule; it holds the inputs of this file and says which branch each of them
drives (proved on the CPU by tests/test_fit_schedule_model.py for 256 CUs, recomputed here for the device at hand).

References: LAPACK (scipy) in fp64 on the oracle's kernel matrix.  Bounds: A -- those of test_gpu_parity.py::_check_fit
 in fp64 and of test_gpu_family_parity.py::test_fit_parity_matrix in fp32; B and C -- those of
test_split_path_matches_batched_path_and_lapack and test_split_path_fp32_matches_batched_path_and_lapack, on their
data recipe.  Every figure is printed before it is asserted.
"""
import time

import numpy as np
import pytest
import scipy.linalg as sla
import torch
from scipy.linalg import lapack

import patchmixturekriging_amd as pmk
from patchmixturekriging_amd import mixture as M
from oracle import oracle as O

import _fit_schedule as F

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    t0 = time.perf_counter()
    yield
    print("\ntests/test_gpu_fit_schedule.py: %.1f s wall" % (time.perf_counter() - t0))


def _num_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _targets(X):
    return np.sin(3 * X[:, 0]) + X[:, -1] ** 2


def _fit(Xs, ys, dtype, mode, th, sigma2, diag=None, fits=1):
    m = pmk.DeviceModel(Xs, ys, dtype=dtype)
    assert pmk.default_context().L.pmk_test_model_set_split(m.h, mode) == 0
    if diag is not None:
        m.set_diag(diag)
    for _ in range(fits):
        m.fit(th, sigma2)
    return m


def _state(m, r):
    return m.get(r, M.GET_L), m.get(r, M.GET_LINV_DIAG), m.get(r, M.GET_C)


def _same(a, b):
    return all(np.array_equal(u, v) for u, v in zip(a, b))


def _residual(U, c, y):
    return np.linalg.norm(U @ c - y) / (np.linalg.norm(U) * np.linalg.norm(c) + np.linalg.norm(y))


def _kappa(U):
    ev = np.linalg.eigvalsh(U)
    assert ev[0] > 0, ev[0]
    return float(ev[-1] / ev[0])


def _ulps(a, b):
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


# ======================================================================================== A. batched path
# name -> D, {dtype: (domain, product kernel, oracle kernel, sigma2, L_tol)}.  fp64: the recipe of the split-path tests
# (uniform in the unit box, compact kernels; L_tol as _check_fit is called for the family).  fp32: the recipe of the family
# parity matrix, which keeps kappa(U) eps32 <= 1e-3 (asserted per patch).
A_COMBOS = {
    # Spline34 in 2 and 3 dimensions: the step launches evaluate the kernel themselves (fused kernel-matrix build)
    "spline34-2d": (2, {"f64": ((0, 1), lambda: pmk.Spline34KernelType(3.0), lambda: O.kernel(O.SPLINE34, 3.0), 1e-5, 1e-8),
                        "f32": ((-2, 2), lambda: pmk.Spline34KernelType(1.0), lambda: O.kernel(O.SPLINE34, 1.0), 0.05, None)}),
    "spline34-3d": (3, {"f64": ((0, 1), lambda: pmk.Spline34KernelType(6.0), lambda: O.kernel(O.SPLINE34, 6.0), 1e-4, 1e-8),
                        "f32": ((-2, 2), lambda: pmk.Spline34KernelType(1.0), lambda: O.kernel(O.SPLINE34, 1.0), 0.05, None)}),
    # another family: the tiles are read from the slab
    "spline32-2d": (2, {"f64": ((0, 1), lambda: pmk.Spline32KernelType(3.0), lambda: O.kernel(O.SPLINE32, 3.0), 1e-4, 1e-7),
                        "f32": ((-2, 2), lambda: pmk.Spline32KernelType(1.0), lambda: O.kernel(O.SPLINE32, 1.0), 0.05, None)}),
}


def _check_pool_patch(m, r, X, y, oth, sigma2, dtype, L_tol, st):
    """_check_fit of test_gpu_parity.py (fp64) / the fp32 branch of test_fit_parity_matrix, against LAPACK on the
    oracle's kernel matrix; returns the figures"""
    n = len(y)
    L, Ni, c = st
    K = O.kernel_matrix(oth, X)
    U = K + sigma2 * np.eye(n)
    Lref = sla.cholesky(U, lower=True, check_finite=False)
    cref = sla.cho_solve((Lref, True), y, check_finite=False)
    res = _residual(U, c, y)
    back = np.linalg.norm(L @ L.T - U) / np.linalg.norm(U)
    dL = np.abs(L - Lref).max()
    dc = np.linalg.norm(c - cref) / np.linalg.norm(cref)
    assert np.all(np.triu(L, 1) == 0)
    if dtype == "f64":
        assert res <= 1e-13, (r, n, res)
        assert back <= 1e-14, (r, n, back)
        assert dL <= L_tol, (r, n, dL)
        assert dc <= 1e-6, (r, n, dc)
        Kd = m.get(r, M.GET_K)
        assert np.array_equal(Kd, Kd.T) and (n == 0 or _ulps(Kd[K != 0], K[K != 0]).max() <= 4)
        ni_tol = 1e-9
        fig = (res, back, dL, dc)
    else:
        k = _kappa(U)
        assert k * EPS32 <= 1e-3, (r, n, k)
        relL = np.linalg.norm(L - Lref) / np.linalg.norm(Lref)
        assert back <= 200 * EPS32, (r, n, back / EPS32)
        assert res <= 200 * EPS32, (r, n, res / EPS32)
        assert relL <= 10 * k * EPS32, (r, n, relL / (k * EPS32))
        assert dc <= 10 * k * EPS32, (r, n, dc / (k * EPS32))
        ni_tol = 64 * np.sqrt(k) * EPS32
        fig = (res / EPS32, back / EPS32, relL / (k * EPS32), dc / (k * EPS32))
    for b in range(Ni.shape[0]):                         # the negated inverted 32 x 32 diagonal blocks invert L's blocks
        lo, hi = 32 * b, min(32 * (b + 1), n)
        if lo >= n:
            assert np.array_equal(Ni[b], -np.eye(32))    # identity padding
            continue
        assert np.abs(-Ni[b][:hi - lo, :hi - lo] @ L[lo:hi, lo:hi] - np.eye(hi - lo)).max() <= ni_tol, (r, b)
        assert np.all(np.triu(Ni[b], 1) == 0)
    return fig


@pytest.mark.timeout(1200)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("combo", sorted(A_COMBOS))
def test_batched_fit_of_a_patch_does_not_depend_on_its_batch(combo, dtype):
    D, by_dtype = A_COMBOS[combo]
    (lo, hi), th, oth, sigma2, L_tol = by_dtype[dtype]
    th, oth = th(), oth()
    sizes = F.pool_sizes()
    P = len(sizes)
    # a condition on the inputs: over the pool's launches the number of active patches visits every residue mod 8
    # (step_slot deals slots over 8 XCDs and pads the grid to a multiple of 8 slots)
    sched = F.schedule(sizes, _num_cu(), 0)
    assert {L.nactive % 8 for L in sched.launches} == set(range(8))
    rng = np.random.Generator(np.random.PCG64(7000 + 10 * D + len(combo)))
    Xs = [rng.uniform(lo, hi, (n, D)) for n in sizes]
    ys = [_targets(x) for x in Xs]

    def fit(idx, diag=None):
        m = _fit([Xs[i] for i in idx], [ys[i] for i in idx], dtype, 0, th, sigma2,
                 None if diag is None else [diag[i] for i in idx])
        return m, m.info()

    alone = []
    for i in range(P):
        m, info = fit([i])
        assert info[0] == 0, (i, info)
        alone.append(_state(m, 0))
    compared = 0

    def compare(name, idx, skip=(), diag=None):
        nonlocal compared
        m, info = fit(idx, diag)
        for j, i in enumerate(idx):
            if i in skip:
                continue
            assert info[j] == 0, (name, i, sizes[i], info[j])
            st = _state(m, j)
            for what, u, v in zip(("L", "LINV_DIAG", "C"), st, alone[i]):
                assert np.array_equal(u, v), "%s: %s of patch %d (n = %d, slot %d of %d) differs from the patch fitted alone" \
                    % (name, what, i, sizes[i], j, len(idx))
            compared += 1
        return m, info

    comps = F.pool_compositions(P)
    worst = None
    for name, idx in comps.items():
        m, _ = compare(name, idx)
        if name == "pool":
            # every patch of the full pool against LAPACK, with the project's fit bounds
            figs = [_check_pool_patch(m, r, Xs[r], ys[r], oth, sigma2, dtype, L_tol, alone[r]) for r in range(P)]
            worst = np.max(np.array(figs), axis=0)
    big = sched.order[0]
    for i in range(P):
        if i != big:
            compare("beside the largest", [i, big] if i % 2 else [big, i])
    # one non-positive-definite patch (diagonal addend -3 at one point: pivot <= -2 in any precision) at the first, the
    # middle and the last slot of the sorted order: every other patch keeps its bits (v + 0.0 == v for the zero addends),
    # the bad one reports what it reports alone, which is what LAPACK reports
    for where, bad in (("first", sched.order[0]), ("middle", sched.order[P // 2]), ("last", sched.order[-1])):
        diag = [np.zeros(n) for n in sizes]
        j = (2 * sizes[bad]) // 3
        diag[bad][j] = -3.0
        _, info_alone = fit([bad], diag)
        _, want = lapack.dpotrf(O.kernel_matrix(oth, Xs[bad]) + np.diag(sigma2 + diag[bad]), lower=1)
        assert info_alone[0] == want == j + 1, (where, bad, info_alone, want)
        _, info = compare("bad patch " + where, list(range(P)), skip=(bad,), diag=diag)
        assert info[bad] == want, (where, bad, info[bad], want)
    unit = "" if dtype == "f64" else " (eps32, eps32, kappa eps32, kappa eps32)"
    print("\n%s %s: %d patch fits in %d batches bit-identical to the patch alone; pool worst residual %.2e  backward %.2e  "
          "dL %.2e  dc %.2e%s" % ((combo, dtype, compared, len(comps) + P - 1 + 3) + tuple(worst) + (unit,)))


# ======================================================================================== B and C: the split path
# the data recipe of test_split_path_matches_batched_path_and_lapack (D = 2) and of its fp32 twin
S_TH, S_OTH = pmk.Spline34KernelType(3.0), O.kernel(O.SPLINE34, 3.0)
S_SIGMA2 = {"f64": 1e-5, "f32": 5e-2}


def _split_data(seed, sizes):
    rng = np.random.Generator(np.random.PCG64(seed))
    Xs = [rng.uniform(0, 1, (n, 2)) for n in sizes]
    return Xs, [_targets(x) for x in Xs]


def _refs(Xs, ys, sigma2, dtype):
    out = []
    for X, y in zip(Xs, ys):
        U = O.kernel_matrix(S_OTH, X) + sigma2 * np.eye(len(y))
        Lref = sla.cholesky(U, lower=True, check_finite=False)
        cref = sla.cho_solve((Lref, True), y, check_finite=False)
        k = None
        if dtype == "f32":
            k = _kappa(U)
            assert k * EPS32 <= 1e-3, k
        out.append((U, Lref, cref, k))
    return out


def _other_order(dtype, L1, c1, L0, c0, k, tag):
    """the bound for 'same tiles, other summation order': test_split_path_matches_batched_path_and_lapack in fp64, its
    fp32 twin in fp32; returns max |dL|"""
    dL = float(np.abs(L1 - L0).max())
    relc = np.linalg.norm(c1 - c0) / np.linalg.norm(c0)
    if dtype == "f64":
        assert dL < 1e-11, (tag, dL)
        assert relc < 1e-7, (tag, relc)
    else:
        assert np.linalg.norm(L1 - L0) / np.linalg.norm(L0) <= 10 * k * EPS32, tag
        assert relc <= 10 * k * EPS32, tag
    return dL


@pytest.mark.timeout(900)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_split_factor_of_a_patch_across_batches(dtype):
    """mode 2 (split path, block-by-block solves: their chunking is a function of the block alone).  Patches a, b of 20
    tiles, c of 13, d of 40."""
    sizes = {"a": 2560, "b": 2500, "c": 1600, "d": 5120}
    Xs, ys = _split_data(8100, list(sizes.values()))
    X, y = dict(zip(sizes, Xs)), dict(zip(sizes, ys))
    sigma2 = S_SIGMA2[dtype]
    kap = dict(zip(sizes, (r[3] for r in _refs(Xs[:3], ys[:3], sigma2, dtype)))) if dtype == "f32" else {}

    def fit(names):
        m = _fit([X[s] for s in names], [y[s] for s in names], dtype, 2, S_TH, sigma2)
        assert np.all(m.info() == 0)
        return {s: _state(m, j) for j, s in enumerate(names)}

    def c_close(c1, c0, s, tag):                        # the weights: by the bound for another summation order only
        relc = np.linalg.norm(c1 - c0) / np.linalg.norm(c0)
        assert relc < (1e-7 if dtype == "f64" else 10 * kap[s] * EPS32), (tag, s, relc)

    alone_a, alone_c = fit("a")["a"], fit("c")["c"]
    # equal max_nt = 20: bit-identical, alone or not, in any order
    abc, cba, ba = fit("abc"), fit("cba"), fit("ba")
    for name, got in (("a+b+c", abc), ("c+b+a", cba), ("b+a", ba)):
        assert _same(got["a"][:2], alone_a[:2]), name
        c_close(got["a"][2], alone_a[2], "a", name)
        for s in got:
            assert _same(got[s][:2], abc[s][:2]), (name, s)
            c_close(got[s][2], abc[s][2], s, name)
    # different max_nt: a alone (max_nt = 20) against a beside d (max_nt = 40), c alone (13) against c beside a and b (20).
    # The patch runs the same block columns at later launches and nsplit_of(l, G) grows with l: other chunks, another
    # summation order.  Measured on an MI355X: the factors are NOT bit-identical (figures in the output), as the
    # nsplit_of comment and DESIGN.md say; they agree to the bound for "same tiles, other summation order".  Both are
    # asserted, so those two texts say what holds: a change that makes the bits equal has to restate them.
    ad = fit("ad")
    for tag, one, other, s in (("20 tiles alone vs beside 40 tiles", alone_a, ad["a"], "a"),
                               ("13 tiles alone vs beside 20 + 20 tiles", alone_c, abc["c"], "c")):
        same_L, same_N = np.array_equal(one[0], other[0]), np.array_equal(one[1], other[1])
        print("\nsplit path %s, %s: L bit-identical %s, inverted blocks bit-identical %s, max |dL| %.3e"
              % (dtype, tag, same_L, same_N, float(np.abs(other[0] - one[0]).max())))
        assert not same_L, tag
        _other_order(dtype, other[0], other[2], one[0], one[2], kap.get(s), tag)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("mode", [1, 2, 3])
def test_split_failing_patch_reports_for_itself_and_leaves_its_neighbours_alone(mode, dtype):
    """tiles 12, 7, 6, 12, 9 in the caller's order, so a patch's slot in `order` is not its index (7 tiles: patch 1, slot 3;
    6 tiles: patch 2, slot 4).  Both enter after splitting has begun, so every diagonal tile of theirs from the second on
    is factorised by the first workgroups of a partial launch (the pending potrf) or by the final flush.  One failing
    pivot in each, in turn: the status word is the failing patch's own, and every other patch keeps the bits of the
    healthy fit of the same batch."""
    sizes = [1536, 800, 641, 1500, 1100]
    Xs, ys = _split_data(8300, sizes)
    sigma2 = S_SIGMA2[dtype]
    sched = F.schedule(sizes, _num_cu(), mode)
    assert sched.order == [0, 3, 4, 1, 2]
    healthy = _fit(Xs, ys, dtype, mode, S_TH, sigma2)
    assert np.all(healthy.info() == 0)
    ref = [_state(healthy, r) for r in range(len(sizes))]
    # patch 1 (7 tiles, 800 points): its last tile (final potrf-only flush), its sixth and its second (pending potrf);
    # patch 2 (6 tiles, 641 points): its one-row last tile (final flush) and its third tile (pending potrf)
    for bad, j in ((1, 790), (1, 700), (1, 130), (2, 640), (2, 300)):
        diag = [np.zeros(n) for n in sizes]
        diag[bad][j] = -3.0
        _, want = lapack.dpotrf(O.kernel_matrix(S_OTH, Xs[bad]) + np.diag(sigma2 + diag[bad]), lower=1)
        assert want == j + 1
        m = _fit(Xs, ys, dtype, mode, S_TH, sigma2, diag)
        info = m.info()
        print("\nsplit mode %d %s, patch %d fails at pivot %d: info %s" % (mode, dtype, bad, j + 1, info.tolist()))
        assert info.tolist() == [want if r == bad else 0 for r in range(len(sizes))]
        for r in range(len(sizes)):
            if r != bad:
                assert _same(_state(m, r), ref[r]), (mode, bad, j, r)


def _figures(dtype, L, c, U, Lref, cref, y, k, tag, same_L=False):
    """a fit against LAPACK: the bounds of the two split-path tests; returns (|L - Lref|, residual).  same_L: this L has
    been held to them already (the caller asserts it bit-identical to one that was), only c is new"""
    dL = float(np.abs(L - Lref).max())
    res = _residual(U, c, y)
    if dtype == "f64":
        assert dL < 1e-9, (tag, dL)
        assert res <= 1e-13, (tag, res)
    else:
        if not same_L:
            back = np.linalg.norm(L @ L.T - U) / np.linalg.norm(U)
            assert back <= 200 * EPS32, (tag, back / EPS32)
            assert np.linalg.norm(L - Lref) / np.linalg.norm(Lref) <= 10 * k * EPS32, tag
        assert res <= 200 * EPS32, (tag, res / EPS32)
        assert np.linalg.norm(c - cref) / np.linalg.norm(cref) <= 10 * k * EPS32, tag
    return dL, res


C_CASES = F.edge_cases()


@pytest.mark.timeout(1200)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("case", list(C_CASES))
def test_split_schedule_edges_vs_lapack_and_batched_path(case, dtype):
    sizes = C_CASES[case]
    P = len(sizes)
    Xs, ys = _split_data(8200 + sum(sizes) % 1000, sizes)
    sigma2 = S_SIGMA2[dtype]
    refs = _refs(Xs, ys, sigma2, dtype)
    hit = sorted(F.branches(F.schedule(sizes, _num_cu(), 1), auto_solves=True))
    worst = {"L": 0.0, "res": 0.0, "split": 0.0}
    base = None
    L_split = None
    for mode in (0, 1, 2, 3):
        # three fits in a row with the chained solves: their flags carry an epoch, nothing is cleared in between
        m = _fit(Xs, ys, dtype, mode, S_TH, sigma2, fits=3 if mode == 3 else 1)
        assert np.all(m.info() == 0), (case, mode, m.info())
        st = [_state(m, r) for r in range(P)]
        for r in range(P):
            U, Lref, cref, k = refs[r]
            L, Ni, c = st[r]
            tag = (case, dtype, mode, r, sizes[r])
            if mode > 1:
                # the factor does not depend on how the solves that follow it are scheduled
                assert np.array_equal(L, L_split[r][0]) and np.array_equal(Ni, L_split[r][1]), tag
            dL, res = _figures(dtype, L, c, U, Lref, cref, ys[r], k, tag, same_L=mode > 1)
            worst["L"], worst["res"] = max(worst["L"], dL), max(worst["res"], res)
            if mode > 0:
                worst["split"] = max(worst["split"], _other_order(dtype, L, c, base[r][0], base[r][2], k, tag))
        if mode == 0:
            base = st
        if mode == 1:
            L_split = st
    print("\n%s %s sizes %s\n    branches %s\n    worst |L - Lref| %.2e  residual %.2e  |L_split - L_batched| %.2e"
          % (case, dtype, sizes if P <= 8 else "%d patches of %d..%d" % (P, min(sizes), max(sizes)), hit,
             worst["L"], worst["res"], worst["split"]))


def test_edge_cases_cover_the_schedule_branches_on_this_device():
    """the coverage assertions of tests/test_fit_schedule_model.py with the device's own CU count; on a device that is not
    256 CUs wide the coverage is printed and not asserted (the numerical tests above run regardless)"""
    num_cu = _num_cu()
    cov = F.coverage(num_cu)
    print("\nnum_cu = %d" % num_cu)
    for b in sorted(cov):
        print("    %-48s %d cases, e.g. %s" % (b, len(cov[b]), cov[b][0]))
    if num_cu == 256:
        for b in F.REQUIRED_BRANCHES:
            assert cov.get(b), b

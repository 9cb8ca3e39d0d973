"""The multi-output solve and item means at their column and chunk edges (csrc/pmk_multi.hip: multi_solve_kernel,
item_means_kernel, mix_multi_kernel; the host packing loops of pmk_api.cpp behind them).

A. the solve: every R, a column's bits whatever R and whatever the other columns hold, a patch's bits whatever its batch,
   padded leading dimensions through the raw C calls, the split and loaded-factor routes at small n, and the R-column
   block after a history of target and trend changes against a model taken straight to the same state.
B. the items: chunk and workgroup edges of item_means_kernel (tests/_multi_refs.py restates the rules), an item's bits
   wherever it lands, mean-only against variance, pmk_query_mix_multi on pieces of the query range, a failed neighbour.

Workload: points uniform(-4, 4), Spline34 at the settings of tests/test_gpu_multi_output.py (fp64 a = 1/3, sigma2 = 1e-3;
fp32 a = 1, sigma2 = 0.05, where kappa(U) eps32 <= 1e-3 is asserted first).  Per-item values come from explicit
(point, region) items, one per query, whose mixture with weight 1 is the item itself (tests/test_gpu_trend.py).

Bounds.  Weights: those of tests/test_gpu_multi_output.py.  Items in fp64, derived: the device's kernel values are within
4 ulp of the oracle's or both below 1e-18 (tests/test_gpu_parity.py), a dot product of n terms adds gamma_n, so to first
order |d| <= (n + 4) u S_j + 1e-18 sum_i |C_ij| with S_j = sum_i |k_i| |C_ij| and u = eps of the element type; the
bound is twice that.  With a trend mu also takes the q terms of h . beta: they join S_j and n.  Items in fp32: the bound
of tests/test_gpu_query_edges.py for the same quantity, 50 sqrt(kappa) eps32 (S_j + 1).  Every measured ratio to its
bound is printed ("MULTI {json}") and a run of the whole module writes them to profiles/multi_output_edges.json.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
from scipy.sparse.csgraph import connected_components

import patchmixturekriging_amd as pmk
from patchmixturekriging_amd import _lib
from patchmixturekriging_amd import mixture as M
from oracle import oracle as O
import _multi_refs as R_
import _trend_refs as T
from test_gpu_multi_output import _mixgp_case, _targets

pytestmark = pytest.mark.gpu

EPS = {"f64": float(np.finfo(np.float64).eps), "f32": float(np.finfo(np.float32).eps)}
SETTING = {"f64": (1 / 3.0, 1e-3), "f32": (1.0, 0.05)}
RMAX = R_.PMK_MAX_OUTPUTS
SOLVE_SIZES = [1, 2, 31, 32, 33, 127, 128, 129, 255, 256, 257, 384, 385]     # nt = 1 .. 4, both sides of every edge
ITEM_SIZES = [1, 7, 8, 9, 63, 128, 129, 700]
COUNT_SETS = [(0, 1, 15, 16, 17, 0, 64, 65), (65, 64, 0, 17, 16, 15, 1, 0), (0, 0, 0, 0, 0, 0, 0, 33), (33, 0, 0, 0, 0, 0, 0, 0)]
SENTINEL = -7.25e300

_RECORDS = []
EDGES_JSON = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "multi_output_edges.json")


def _record(**kw):
    _RECORDS.append(kw)
    print("MULTI " + json.dumps(kw, sort_keys=True))


@pytest.fixture(scope="module", autouse=True)
def _write_edges_file():
    """after the module's last test: every figure of this run -> profiles/multi_output_edges.json.  Only a run of the
    whole module replaces the file"""
    yield
    cases = {(r["test"], r.get("case"), r["dtype"]) for r in _RECORDS}
    want = {("items", c, d) for c, d, _, _, _ in ITEM_CASES} | {("weights", None, d) for d in EPS} | \
           {("split_and_loaded", c, "f64") for c in ("split", "loaded")} | {("split_and_loaded", "split", "f32")}
    if want <= cases:
        with open(EDGES_JSON, "w") as f:
            f.write("[\n" + ",\n".join(" " + json.dumps(r, sort_keys=True) for r in _RECORDS) + "\n]\n")


# ------------------------------------------------------------------------------------------ helpers
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def _kernels(dtype):
    a = SETTING[dtype][0]
    return pmk.Spline34KernelType(a), O.kernel(O.SPLINE34, a)


def _fitted(Xs, dtype, split=0):
    """a fitted model; split = 0 pins the batched factorisation, so that the factor does not depend on the batch"""
    model = M.DeviceModel(Xs, [np.ascontiguousarray(X[:, 0]) for X in Xs], dtype=dtype)
    assert pmk.default_context().L.pmk_test_model_set_split(model.h, split) == 0
    model.fit(_kernels(dtype)[0], SETTING[dtype][1])
    return model


def _solve(model, Ys, trend=None):
    model.set_targets_multi(Ys)
    model.set_trend(trend)
    model.solve_multi()
    return model.weights_multi()


_BATCH = {}


def _solve_batch(dtype):
    """the 13 patches of part A, 16 target vectors each, U and kappa(U) from the oracle, the LAPACK weights: once"""
    if dtype not in _BATCH:
        rng = np.random.default_rng(9100)
        Xs = [rng.uniform(-4, 4, (n, 2)) for n in SOLVE_SIZES]
        Ys = [np.asfortranarray(_targets(X, RMAX)) for X in Xs]
        oth, sigma2 = _kernels(dtype)[1], SETTING[dtype][1]
        Us = [O.kernel_matrix(oth, X) + sigma2 * np.eye(len(X)) for X in Xs]
        ks = [R_.kappa(U) for U in Us]
        _BATCH[dtype] = (Xs, Ys, Us, ks, [R_.lapack_weights(U, Y) for U, Y in zip(Us, Ys)])
    return _BATCH[dtype]


def _check_weights(dtype, U, k, Cm, Y, ref, what):
    """the bounds of test_weights_vs_oracle_per_column / test_weights_f32 -> (residual, worst forward error) over bound"""
    if dtype == "f32":
        assert k * EPS["f32"] <= 1e-3, (what, k)
    rb, fb = (1e-14, 1e-6) if dtype == "f64" else (200 * EPS["f32"], 10 * k * EPS["f32"])
    res = R_.rel_residual(U, Cm, Y)
    fwd = max(np.linalg.norm(Cm[:, j] - ref[:, j]) / np.linalg.norm(ref[:, j]) for j in range(Cm.shape[1]))
    assert res <= rb, (what, "residual", res / rb)
    assert fwd <= fb, (what, "forward error", fwd / fb)
    return res / rb, fwd / fb


# ------------------------------------------------------------------------------------------ A1. every R
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_every_R_and_a_column_does_not_depend_on_R(dtype):
    Xs, Ys, Us, ks, refs = _solve_batch(dtype)
    model = _fitted(Xs, dtype)
    assert np.all(model.info() == 0)
    Cs = {R: _solve(model, [Y[:, :R] for Y in Ys]) for R in range(1, RMAX + 1)}
    for r, n in enumerate(SOLVE_SIZES):
        full = Cs[RMAX][r]
        for R in range(1, RMAX + 1):
            Cm = Cs[R][r]
            assert Cm.shape == (n, R)
            for j in range(R):
                assert same_bits(Cm[:, j], full[:, j]), "n = %d: column %d at R = %d differs from R = %d" % (n, j, R, RMAX)
            res, fwd = _check_weights(dtype, Us[r], ks[r], Cm, Ys[r][:, :R], refs[r], (n, R))
        _record(test="weights", dtype=dtype, n=n, R=RMAX, residual=res, forward=fwd)


# ------------------------------------------------------------------------------------------ A2. isolation, linearity
def scaling_is_exact(U, y, dtype):
    """a condition on the inputs, checked on the host: the solves of 2^20 y and 2^-20 y round as the solve of y does.
    A power-of-two scale commutes with every rounding unless a result overflows or falls below the smallest normal
    number.  Every intermediate of the substitutions is a sum of at most n products of an entry of L (or of an inverted
    32 x 32 diagonal block) with an entry of y, z = L^-1 y or c:
      - overflow: n max|L, inverted blocks| max|y, z, c| 2^20 is finite;
      - underflow: every nonzero entry of y, z and c, times 2^-20, is at least 2^30 times the smallest normal number.
    The second cannot be asked of every partial sum: fill-in entries of L are products of kernel values near the edge of
    the support and as small as 1e-30, so the first terms of a sum may fall below the smallest normal number in the
    2^-20 column.  What is lost there is at most that number, 2^-30 of the smallest value the sum is added to or stored
    as (2^-7 of its last bit): it can change a result only by breaking an exact rounding tie."""
    fi = np.finfo(np.float64 if dtype == "f64" else np.float32)
    big, tiny = float(fi.max), float(fi.tiny)
    n = len(y)
    L = np.linalg.cholesky(U)
    z = np.linalg.solve(L, y)
    c = np.linalg.solve(L.T, z)
    mats = [L] + [np.linalg.inv(L[s:s + 32, s:s + 32]) for s in range(0, n, 32)]
    mmax = max(float(np.abs(m).max()) for m in mats)
    vv = np.abs(np.concatenate([y, z, c]))
    vv = vv[vv > 0]
    assert 2.0 ** 20 * n * mmax * vv.max() < big, (n, mmax, vv.max())
    assert 2.0 ** -20 * vv.min() >= 2.0 ** 30 * tiny, (n, vv.min())


def reach_of_row0(U):
    """rows i with (U^-1)[i, 0] != 0 for a generic U of this sparsity: the connected component of row 0"""
    _, lab = connected_components(U != 0, directed=False)
    return lab == lab[0]


def isolation_columns(y):
    inf0 = y.copy()
    inf0[0] = np.inf
    return np.asfortranarray(np.stack([y, 2.0 ** 20 * y, 2.0 ** -20 * y, np.zeros_like(y), np.full_like(y, np.nan), inf0], 1))


@pytest.mark.parametrize("trend", [None, "constant"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_columns_are_isolated_and_the_solve_is_linear(dtype, trend):
    Xs, Ys, Us, ks, _ = _solve_batch(dtype)
    for U, Y in zip(Us, Ys):
        scaling_is_exact(U, Y[:, 0], dtype)
    model = _fitted(Xs, dtype)
    alone = _solve(model, [Y[:, :1] for Y in Ys], trend)
    beta_alone = model.trend()[0]
    six = _solve(model, [isolation_columns(Y[:, 0].copy()) for Y in Ys], trend)
    beta = model.trend()[0]
    assert np.all(model.trend_info() == 0)
    for r, n in enumerate(SOLVE_SIZES):
        Cm = six[r]
        assert np.all(np.isfinite(Cm[:, :4])), n
        assert same_bits(Cm[:, 0], alone[r][:, 0]), "n = %d: y beside other columns differs from y alone" % n
        assert np.array_equal(Cm[:, 1], 2.0 ** 20 * Cm[:, 0]), "n = %d: 2^20 y" % n
        assert np.array_equal(Cm[:, 2], 2.0 ** -20 * Cm[:, 0]), "n = %d: 2^-20 y" % n
        assert np.all(Cm[:, 3] == 0.0), "n = %d: the zero column" % n
        if trend is None:
            assert not np.any(np.isfinite(Cm[:, 4])), "n = %d: the NaN column" % n
            reach = reach_of_row0(Us[r])
            assert reach[0] and not np.any(np.isfinite(Cm[reach, 5])), "n = %d: the column with +inf in row 0" % n
        else:
            b = beta[r]
            assert same_bits(b[:, 0], beta_alone[r][:, 0]), n
            assert np.array_equal(b[:, 1], 2.0 ** 20 * b[:, 0]) and np.array_equal(b[:, 2], 2.0 ** -20 * b[:, 0]), n
            assert np.all(b[:, 3] == 0.0), n


# ------------------------------------------------------------------------------------------ A3. batch position
def _probe_state(model, j):
    return model.get(j, M.GET_L), model.get(j, M.GET_LINV_DIAG)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_solve_of_a_patch_does_not_depend_on_its_batch(dtype):
    Xs, Ys, _, _, _ = _solve_batch(dtype)
    probes = [SOLVE_SIZES.index(n) for n in (33, 129, 385)]
    others = [i for i in range(len(SOLVE_SIZES)) if i not in probes]
    rng = np.random.default_rng(9300)
    small = [rng.uniform(-4, 4, (5, 2)) for _ in range(300)]
    crowd = [(X, np.asfortranarray(_targets(X, RMAX))) for X in small]
    assert len(crowd) > _num_cu()                   # more workgroups than the chip holds at one per CU

    def run(entries):
        """entries: indices of the 13-patch batch, or (X, Y) pairs -> the model and the weights"""
        pairs = [(Xs[e], Ys[e]) if isinstance(e, int) else e for e in entries]
        model = _fitted([p[0] for p in pairs], dtype)
        return model, _solve(model, [p[1] for p in pairs])

    want = {}
    for p in probes:
        model, Cs = run([p])
        want[p] = (_probe_state(model, 0), Cs[0])
    arrangements = {}
    for k in range(3):                              # each probe first, in the middle and last of the 13
        first, mid, last = probes[k], probes[(k + 1) % 3], probes[(k + 2) % 3]
        arrangements["batch %d" % k] = [first] + others[:5] + [mid] + others[5:] + [last]
        assert len(arrangements["batch %d" % k]) == len(SOLVE_SIZES)
    arrangements["crowd"] = [probes[0]] + crowd[:150] + [probes[1]] + crowd[150:] + [probes[2]]
    compared = 0
    for name, entries in arrangements.items():
        model, Cs = run(entries)
        for j, e in enumerate(entries):
            if isinstance(e, int) and e in probes:
                # the factor first (tests/test_gpu_fit_schedule.py's property), so that only the solve is left to differ
                assert same_bits(_probe_state(model, j), want[e][0]), "%s: the FACTOR of n = %d differs" % (name, SOLVE_SIZES[e])
                assert same_bits(Cs[j], want[e][1]), "%s: the weights of n = %d at position %d of %d differ from the patch " \
                    "solved alone" % (name, SOLVE_SIZES[e], j, len(entries))
                compared += 1
    assert compared == 12


def _num_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


# ------------------------------------------------------------------------------------------ B. the item batch
_TREE = {}


def _tree8(D):
    """any 8-leaf tree: explicit items name their regions"""
    if D not in _TREE:
        _TREE[D] = pmk.setuppartition(np.random.default_rng(5).uniform(-4, 4, (64, D)), 4)[0]
    return _TREE[D]


def _item_patches(D):
    rng = np.random.default_rng(9400 + D)
    return [rng.uniform(-4, 4, (n, D)) for n in ITEM_SIZES]


def item_set(counts, Xs, seed):
    """explicit items with the given per-region counts, in shuffled order: inside the data, one at a training point and
    two far outside every support (in the region with the most items)"""
    D = Xs[0].shape[1]
    rng = np.random.default_rng(seed)
    xq = [rng.uniform(-4, 4, (c, D)) for c in counts]
    big = int(np.argmax(counts))
    assert counts[big] >= 3
    xq[big][0] = Xs[big][len(Xs[big]) // 2]
    xq[big][1], xq[big][2] = 0.0, 0.0
    xq[big][1, :2], xq[big][2, :2] = [40.0, -25.0], [-300.0, 7.0]
    xq, region = np.vstack(xq), np.repeat(np.arange(len(counts)), counts)
    order = rng.permutation(len(region))
    return np.ascontiguousarray(xq[order]), np.ascontiguousarray(region[order], dtype=np.int32)


def chunk_coverage():
    """conditions on COUNT_SETS, checked with the restated rules: what the four item sets place on purpose"""
    seen = set()
    for counts in COUNT_SETS:
        chunks = R_.chunks_of(counts)
        assert len(chunks) == sum(-(-c // R_.CHUNK) for c in counts) and sum(c for _, c in chunks) == sum(counts)
        if counts[0] == 0:
            seen.add("empty first region")
        if counts[-1] == 0:
            seen.add("empty last region")
        if any(c == 0 for c in counts[1:-1]):
            seen.add("empty region in the middle")
        last_of = {r: c for r, c in chunks}                       # the last chunk of every region
        if 1 in last_of.values():
            seen.add("one-item chunk")
        if R_.CHUNK in last_of.values():
            seen.add("full last chunk")
        wg = {}
        for g, (r, _) in enumerate(chunks):
            wg.setdefault(R_.workgroup_of(g), []).append(r)
        if any(len({w for w, rs in wg.items() if r in rs}) >= 2 for r in range(len(counts))):
            seen.add("region in two workgroups")
        if any(len(rs) == R_.WAVES and len(set(rs)) >= 3 for rs in wg.values()):
            seen.add("workgroup serving three regions")
        if len(chunks) % R_.WAVES:
            seen.add("idle waves in the last workgroup")
    assert seen == {"empty first region", "empty last region", "empty region in the middle", "one-item chunk", "full last chunk",
                    "region in two workgroups", "workgroup serving three regions", "idle waves in the last workgroup"}, seen
    # the k-steps of 8 rows: a patch below one step, exact steps, one row into the next step
    assert any(n < R_.KSTEP for n in ITEM_SIZES) and any(n % R_.KSTEP == 0 for n in ITEM_SIZES)
    assert sum(n % R_.KSTEP == 1 for n in ITEM_SIZES) >= 3 and any(n % R_.KSTEP == R_.KSTEP - 1 for n in ITEM_SIZES)


def _explicit(model, xq, region, variance=True, fitted=False):
    """(mu [m, R], v [m] or None) of explicit (point, region) items: items_multi -> mix_multi -> fetch_multi"""
    model.set_bsp(_tree8(xq.shape[1]), 0)
    q = M.DeviceQuery.from_items(model, len(xq), xq.ctypes.data_as(C.c_void_p), region.ctypes.data_as(C.c_void_p))
    if fitted:
        q.items_multi_fitted(variance)
    else:
        q.items_multi(_kernels(model.dtype)[0], variance)
    q.mix_multi(pmk.Spline34KernelType(1.0))
    return q.fetch_multi(model.R)


# case, dtype, D, R, trend
ITEM_CASES = [("R1", "f64", 2, 1, None), ("R1", "f32", 2, 1, None), ("R16", "f64", 2, RMAX, None), ("R16", "f32", 2, RMAX, None),
              ("D4 linear R11", "f64", 4, 11, "linear")]
_ITEM_MODELS = {}


def _item_model(dtype, D, R, trend):
    """the fitted and solved model of an item case, shared by the B tests"""
    key = (dtype, D, R, trend)
    if key not in _ITEM_MODELS:
        Xs = _item_patches(D)
        model = _fitted(Xs, dtype)
        assert np.all(model.info() == 0)
        Cs = _solve(model, [_targets(X, R) for X in Xs], trend)
        _ITEM_MODELS[key] = (Xs, model, Cs)
    return _ITEM_MODELS[key]


@pytest.mark.parametrize("case,dtype,D,R,trend", ITEM_CASES)
def test_item_means_at_chunk_edges(case, dtype, D, R, trend):
    chunk_coverage()
    Xs, model, Cs = _item_model(dtype, D, R, trend)
    th, oth = _kernels(dtype)
    sigma2, u = SETTING[dtype][1], EPS[dtype]
    q = 0 if trend is None else 1 + D
    assert R + q == RMAX or trend is None
    betas, flags = model.trend()[0], model.trend_info()
    kappas = [R_.kappa(O.kernel_matrix(oth, X) + sigma2 * np.eye(len(X))) for X in Xs] if dtype == "f32" else [None] * len(Xs)
    failures = []
    for s, counts in enumerate(COUNT_SETS):
        xq, region = item_set(counts, Xs, 9500 + s)
        mu, v = _explicit(model, xq, region)
        assert mu.shape == (sum(counts), R) and v.shape == (sum(counts),)
        for r, n in enumerate(ITEM_SIZES):
            sel = np.nonzero(region == r)[0]
            if len(sel) == 0:
                continue
            if flags[r] != 0:                        # fewer points than basis functions: NaN, as include/pmk.h promises
                assert n < q and flags[r] == n + 1 and np.all(np.isnan(mu[sel])), (case, s, r)
                continue
            ref, S, _ = R_.item_means_reference(oth, Xs[r], Cs[r], xq[sel])
            terms = n + 4
            if q:
                Hq = T.basis(xq[sel], trend)
                ref = ref + np.asarray(Hq, dtype=R_.LD) @ np.asarray(betas[r], dtype=R_.LD)
                S = S + np.abs(Hq) @ np.abs(betas[r])
                terms += q
            if dtype == "f64":
                bound = 2 * terms * u * S + 1e-18 * np.abs(Cs[r]).sum(0)[None, :]
            else:
                assert kappas[r] * EPS["f32"] <= 1e-3, kappas[r]
                bound = 50 * np.sqrt(kappas[r]) * EPS["f32"] * (S + 1)
            err = np.abs(np.asarray(np.asarray(mu[sel], dtype=R_.LD) - ref, dtype=np.float64))
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.where(err == 0, 0.0, err / bound)         # 0 / 0: a far query, every kernel value exactly zero
            worst = float(np.max(ratio))
            _record(test="items", case=case, dtype=dtype, counts=list(counts), region=r, n=n, items=len(sel), ratio=worst)
            if not worst <= 1.0:
                failures.append((s, r, n, worst))
    assert not failures, failures


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_an_items_bits_do_not_depend_on_where_it_lands(dtype):
    Xs, model, _ = _item_model(dtype, 2, RMAX, None)
    xq, region = item_set(COUNT_SETS[0], Xs, 9500)
    m = len(region)
    want, _ = _explicit(model, xq, region, variance=False)
    got, _ = _explicit(model, np.ascontiguousarray(xq[::-1]), np.ascontiguousarray(region[::-1]), variance=False)
    assert same_bits(got[::-1], want), "reversed"
    for size in (1, 7, 15, 16, 17, 33):
        got = np.vstack([_explicit(model, np.ascontiguousarray(xq[f:f + size]), np.ascontiguousarray(region[f:f + size]),
                                   variance=False)[0] for f in range(0, m, size)])
        bad = np.nonzero(np.any(bits(got) != bits(want), axis=1))[0]
        assert len(bad) == 0, "slices of %d: %d items differ, first %d (region %d)" % (size, len(bad), bad[0], region[bad[0]])


def test_mean_only_against_variance():
    wth = pmk.Spline34KernelType(1.0)
    # without a trend: the means whatever the variance pass, and the variance of the single-output path
    Xs, model, _ = _item_model("f64", 2, RMAX, None)
    xq, region = item_set(COUNT_SETS[0], Xs, 9500)
    Ym, none = _explicit(model, xq, region, variance=False)
    Yv, Vv = _explicit(model, xq, region, variance=True)
    assert none is None and same_bits(Ym, Yv)
    q = M.DeviceQuery.from_items(model, len(xq), xq.ctypes.data_as(C.c_void_p), region.ctypes.data_as(C.c_void_p))
    q.items(_kernels("f64")[0])
    q.mix(wth)
    y1, v1 = q.fetch()
    assert same_bits(Vv, v1)
    # with a trend: the means again; the variance is that of the one-column model with the same trend (the single-output
    # case of kriging with a trend), and the drift's uncertainty only adds to the plain variance
    Xs4, trended, _ = _item_model("f64", 4, 11, "linear")
    xq4, region4 = item_set(COUNT_SETS[0], Xs4, 9500)
    Ym, none = _explicit(trended, xq4, region4, variance=False)
    Yv, Vv = _explicit(trended, xq4, region4, variance=True)
    assert none is None and same_bits(Ym, Yv)
    one = _fitted(Xs4, "f64")
    _solve(one, [_targets(X, 1) for X in Xs4], "linear")
    Y1, V1 = _explicit(one, xq4, region4, variance=True)
    assert same_bits(Vv, V1) and same_bits(Yv[:, 0], Y1[:, 0])
    q = M.DeviceQuery.from_items(trended, len(xq4), xq4.ctypes.data_as(C.c_void_p), region4.ctypes.data_as(C.c_void_p))
    q.items(_kernels("f64")[0])
    q.mix(wth)
    _, v_plain = q.fetch()
    live = trended.trend_info()[region4] == 0
    assert np.all(Vv[live] >= v_plain[live]) and np.all(np.isnan(Vv[~live]))


# ------------------------------------------------------------------------------------------ A4. leading dimensions
def test_leading_dimensions_through_the_raw_calls():
    L = pmk.lib()
    R = 3
    Xs = _item_patches(2)
    P = len(Xs)
    model = _fitted(Xs, "f64")
    Ys = [np.asfortranarray(_targets(X, R)) for X in Xs]
    xq, region = item_set(COUNT_SETS[0], Xs, 9500)
    Nq = len(xq)
    PA = M._dp * P

    def everything():
        model.solve_multi()
        model.loo()
        return model.weights_multi(), model.loo_values_multi(), _explicit(model, xq, region)

    model.set_targets_multi(Ys)
    C0, (RES0, var0), (Yq0, Vq0) = everything()
    # ldy = n + 3: the padding rows are NaN and must not be read
    Yp = [np.full((len(X) + 3, R), np.nan, order="F") for X in Xs]
    for yp, y in zip(Yp, Ys):
        yp[:len(y)] = y
    ldy = np.array([len(yp) for yp in Yp], dtype=np.int64)
    assert L.pmk_model_set_targets_multi(model.h, R, PA(*[M._d(y) for y in Yp]), M._i(ldy)) == 0, L.pmk_last_error()
    model.R, model._multi_solved = R, False
    C1, (RES1, var1), (Yq1, Vq1) = everything()
    assert same_bits(C1, C0) and same_bits(RES1, RES0) and same_bits(var1, var0) and same_bits(Yq1, Yq0) and same_bits(Vq1, Vq0)
    # ldc = n + 5, ldres = n + 2, ldyq = Nq + 3: the padding of the outputs is untouched
    Cp = [np.full((len(X) + 5, R), SENTINEL, order="F") for X in Xs]
    ldc = np.array([len(c) for c in Cp], dtype=np.int64)
    assert L.pmk_model_get_weights_multi(model.h, PA(*[M._d(c) for c in Cp]), M._i(ldc)) == 0, L.pmk_last_error()
    Rp = [np.full((len(X) + 2, R), SENTINEL, order="F") for X in Xs]
    vp = [np.full(len(X), SENTINEL) for X in Xs]
    ldres = np.array([len(a) for a in Rp], dtype=np.int64)
    assert L.pmk_model_get_loo_multi(model.h, PA(*[M._d(a) for a in Rp]), M._i(ldres), PA(*[M._d(a) for a in vp])) == 0
    for r, X in enumerate(Xs):
        n = len(X)
        assert same_bits(Cp[r][:n], C0[r]) and np.all(Cp[r][n:] == SENTINEL), r
        assert same_bits(Rp[r][:n], RES0[r]) and np.all(Rp[r][n:] == SENTINEL) and same_bits(vp[r], var0[r]), r
    q = M.DeviceQuery.from_items(model, Nq, xq.ctypes.data_as(C.c_void_p), region.ctypes.data_as(C.c_void_p))
    q.items_multi(_kernels("f64")[0], True)
    q.mix_multi(pmk.Spline34KernelType(1.0))
    Yqp = np.full((Nq + 3, R), SENTINEL, order="F")
    assert L.pmk_query_fetch_multi(q.h, M._d(Yqp), Nq + 3, None) == 0, L.pmk_last_error()
    assert same_bits(Yqp[:Nq], Yq0) and np.all(Yqp[Nq:] == SENTINEL)
    # ld = n - 1 is refused, with the status and text of today, and changes nothing
    short = np.array([len(X) - 1 for X in Xs], dtype=np.int64)
    assert L.pmk_model_set_targets_multi(model.h, R, PA(*[M._d(y) for y in Ys]), M._i(short)) == -3
    assert b"ldy[0] = 0 < n = 1" in L.pmk_last_error()
    assert L.pmk_model_get_weights_multi(model.h, PA(*[M._d(c) for c in Cp]), M._i(short)) == -2
    assert b"bad output of patch 0" in L.pmk_last_error()
    assert L.pmk_model_get_loo_multi(model.h, PA(*[M._d(a) for a in Rp]), M._i(short), PA(*[M._d(a) for a in vp])) == -4
    assert b"bad output of patch 0" in L.pmk_last_error()
    assert L.pmk_query_fetch_multi(q.h, M._d(Yqp), Nq - 1, None) == -4
    assert b"ldyq = %d < Nq = %d" % (Nq - 1, Nq) in L.pmk_last_error()
    assert same_bits(model.weights_multi(), C0)
    for r, X in enumerate(Xs):
        assert np.all(Cp[r][len(X):] == SENTINEL) and np.all(Rp[r][len(X):] == SENTINEL), r
    assert np.all(Yqp[Nq:] == SENTINEL)


# ------------------------------------------------------------------------------------------ A5. split, loaded factors
def test_forced_split_and_loaded_factors_at_small_n():
    for dtype in ("f64", "f32"):
        Xs, Ys, Us, ks, refs = _solve_batch(dtype)
        idx = [SOLVE_SIZES.index(n) for n in (257, 385)]
        sub = [Xs[i] for i in idx]
        split = _fitted(sub, dtype, split=1)
        assert np.all(split.info() == 0)
        models = [("split", split)]
        if dtype == "f64":                           # pmk_model_load takes fp64 factors
            regular = _fitted(sub, dtype)
            models.append(("loaded", M.DeviceModel.from_factors(sub, regular.weights(),
                                                               [regular.get(r, M.GET_L) for r in range(len(sub))])))
        for name, model in models:
            Cs = _solve(model, [Ys[i] for i in idx])
            for j, i in enumerate(idx):
                res, fwd = _check_weights(dtype, Us[i], ks[i], Cs[j], Ys[i], refs[i], (name, SOLVE_SIZES[i]))
                _record(test="split_and_loaded", case=name, dtype=dtype, n=SOLVE_SIZES[i], R=RMAX, residual=res, forward=fwd)


# ------------------------------------------------------------------------------------------ A6. history
def _packed_block(model, r):
    L = model.ctx.L
    ld = C.c_int64()
    _lib.check(L.pmk_test_model_packed(model.h, r, 3, C.byref(ld), None), "pmk_test_model_packed")
    out = np.empty(ld.value * RMAX)
    _lib.check(L.pmk_test_model_packed(model.h, r, 3, C.byref(ld), M._d(out)), "pmk_test_model_packed")
    return out.reshape(ld.value, RMAX)


def _expected_block(X, Y, trend, ld, dtype):
    """targets in columns < R, H in columns R .. R + q - 1 of the live rows, zero everywhere else"""
    real = np.float64 if dtype == "f64" else np.float32
    n, R = Y.shape
    want = np.zeros((ld, RMAX))
    want[:n, :R] = Y.astype(real)
    if trend is not None:
        H = T.basis(X, trend).astype(real)
        want[:n, R:R + H.shape[1]] = H
    return want


def _state(model):
    beta, G = model.trend()
    return dict(C=model.weights_multi(), beta=beta, G=G, ev=list(model.evidence_multi()), tinfo=model.trend_info())


def _assert_state(model, fresh, what):
    a, b = _state(model), _state(fresh)
    for key in a:
        assert same_bits(a[key], b[key]), "%s: %s differs from a model taken straight to this state" % (what, key)


HISTORY = [(RMAX, None), (2, None), (2, "linear"), (2, None), (RMAX, "constant"), (RMAX - 1, "constant"), (RMAX - 1, None)]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_history_independence(dtype):
    L = pmk.lib()
    sizes = [1, 2, 33, 129, 385]
    Xs, Ys, _, _, _ = _solve_batch(dtype)
    Xs, Ys = [Xs[SOLVE_SIZES.index(n)] for n in sizes], [Ys[SOLVE_SIZES.index(n)] for n in sizes]
    model = _fitted(Xs, dtype)
    for step, (R, trend) in enumerate(HISTORY):
        what = "step %d (R = %d, trend %s)" % (step, R, trend)
        q = M.trend_degree(trend) + 1 if trend != "linear" else 3
        Yr = [Y[:, :R] for Y in Ys]
        if R + q > RMAX:
            model.set_targets_multi(Yr)
            model.set_trend(trend)
            assert L.pmk_model_solve_multi(model.h) == -3, what
            msg = L.pmk_last_error()
            assert b"R=%d" % R in msg and b"q=%d" % q in msg, msg
            # nothing was written: the block holds the new targets alone, and there are no weights to read
            for r, (X, Y) in enumerate(zip(Xs, Yr)):
                blk = _packed_block(model, r)
                assert np.array_equal(blk, _expected_block(X, Y, None, len(blk), dtype)), (what, r)
            PA = M._dp * len(Xs)
            out = [np.empty((len(X), R), order="F") for X in Xs]
            assert L.pmk_model_get_weights_multi(model.h, PA(*[M._d(c) for c in out]), M._i(np.array(sizes, dtype=np.int64))) == -3
            continue
        if [Rt for Rt, _ in HISTORY[:step]][-1:] != [R]:
            model.set_targets_multi(Yr)              # same R as the step before: only the trend changes
        model.set_trend(trend)
        model.solve_multi()
        for r, (X, Y) in enumerate(zip(Xs, Yr)):
            blk = _packed_block(model, r)
            assert blk.shape[0] % R_.TILE == 0 and blk.shape[0] >= len(X)
            want = _expected_block(X, Y, trend, len(blk), dtype)
            bad = np.argwhere(bits(blk) != bits(want))
            assert len(bad) == 0, "%s, n = %d: the block differs at (row, column) %s: %r, want %r" % (
                what, len(X), tuple(bad[0]), blk[tuple(bad[0])], want[tuple(bad[0])])
        fresh = _fitted(Xs, dtype)
        _solve(fresh, Yr, trend)
        _assert_state(model, fresh, what)


def test_history_independence_on_the_tree_route():
    import torch
    levels, eps = 4, 0.6
    X, _, root, X_set, X_set_inds = _mixgp_case(700, levels, eps, 0.5, 10, 31)
    N = len(X)
    Yall = np.asfortranarray(_targets(X, RMAX) + 1.0 + 0.25 * X[:, :1])
    th, sigma2 = _kernels("f64")[0], SETTING["f64"][1]

    def tree_model():
        m = M.DeviceModel.from_tree(root, X, np.ascontiguousarray(Yall[:, 0]), eps=eps)
        m.fit(th, sigma2)
        return m

    model = tree_model()
    off, inds = model.patch_index()
    rows = [inds[off[r]:off[r + 1]] for r in range(model.P)]
    held, sets = None, 0
    for step, (R, trend) in enumerate(HISTORY):
        if R + (M.trend_degree(trend) + 1 if trend != "linear" else 3) > RMAX:
            continue                                 # the refusal is the list route's to test
        what = "tree step %d (R = %d, trend %s)" % (step, R, trend)
        Y = np.asfortranarray(Yall[:, :R])
        if held == R:
            pass                                     # only the trend changes
        elif sets % 2 == 0:
            model.set_targets_multi_global(Y)
        else:
            big = np.asfortranarray(np.full((N + 5, R), np.nan))
            big[:N] = Y
            dev = torch.from_numpy(big).cuda()
            torch.cuda.synchronize()
            model.set_targets_multi_global(dev[:N])
        sets, held = sets + (held != R), R
        model.set_trend(trend)
        model.solve_multi()
        for r in range(model.P):
            blk = _packed_block(model, r)
            want = _expected_block(X[rows[r]], Y[rows[r]], trend, len(blk), "f64")
            assert np.array_equal(bits(blk), bits(want)), (what, r)
        fresh = tree_model()
        fresh.set_targets_multi_global(Y)
        fresh.set_trend(trend)
        fresh.solve_multi()
        _assert_state(model, fresh, what)


# ------------------------------------------------------------------------------------------ B4. mix_multi ranges
@pytest.mark.parametrize("variance", [True, False])
def test_mix_multi_on_pieces_of_the_range(variance):
    L = pmk.lib()
    levels, eps, radius, delta, R, Nq = 4, 0.6, 0.5, 1e-5, 5, 600
    X, Xq, root, X_set, X_set_inds = _mixgp_case(1500, levels, eps, radius, Nq, 28)
    th, sigma2 = _kernels("f64")[0], SETTING["f64"][1]
    wth, other = pmk.Spline34KernelType(1 / radius), pmk.Spline34KernelType(0.7 / radius)
    Yall = _targets(X, R)
    model = M.DeviceModel(X_set, [np.ascontiguousarray(Yall[i, 0]) for i in X_set_inds])
    model.fit(th, sigma2)
    _solve(model, [Yall[i] for i in X_set_inds])
    model.set_bsp(root, 0)
    q = M.DeviceQuery(model, Xq)
    assert q.plan(radius, delta) > Nq                # some queries blend neighbours: the profile matters
    q.items_multi(th, variance)
    q.mix_multi(wth)
    Y0, V0 = q.fetch_multi(R)
    q.mix_multi(other)                               # every entry now holds another profile's result
    Yo, Vo = q.fetch_multi(R)
    assert not np.array_equal(Yo, Y0) and (not variance or not np.array_equal(Vo, V0))
    pieces = [(0, 1), (1, 255), (255, 256), (256, 257), (257, Nq)]
    for k in np.random.default_rng(9600).permutation(len(pieces)):
        q.mix_multi(wth, *pieces[k])
    Y1, V1 = q.fetch_multi(R)
    assert same_bits(Y1, Y0) and (V0 is None) == (not variance) and (not variance or same_bits(V1, V0))
    d = other.desc()
    for at in (0, 255, Nq):                          # [q, q) is a no-op
        assert L.pmk_query_mix_multi(q.h, C.byref(d), at, at) == 0
    for q0, q1 in ((0, Nq + 1), (5, 4), (-1, 3)):
        assert L.pmk_query_mix_multi(q.h, C.byref(d), q0, q1) == -3, (q0, q1)
        assert b"bad query range" in L.pmk_last_error()
    Y2, V2 = q.fetch_multi(R)
    assert same_bits(Y2, Y0) and (not variance or same_bits(V2, V0))


# ------------------------------------------------------------------------------------------ B5. a failed neighbour
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_a_failed_neighbour(dtype):
    """patch 3: points 0 and 1 coincide and sigma2_3 = 0, so pivot 2 is 1 - 1 * 1 = 0 in any precision and any order
    (tests/test_gpu_patches.py::test_a_failed_patch_stays_local)"""
    bad, R = 3, 4
    Xs = _item_patches(2)
    Ys = [_targets(X, R) for X in Xs]
    th, sigma2 = _kernels(dtype)[0], SETTING[dtype][1]
    xq, region = item_set(COUNT_SETS[0], Xs, 9500)
    assert np.any(region == bad)

    def run(Xp, s2, trend):
        m = M.DeviceModel(Xp, [np.ascontiguousarray(X[:, 0]) for X in Xp], dtype=dtype)
        m.fit_patches([th] * len(Xp), s2)
        Cs = _solve(m, Ys, trend)
        m.loo()
        return dict(info=m.info(), C=Cs, beta=m.trend()[0], ev=m.evidence_multi(), loo=m.loo_values_multi(),
                    items=_explicit(m, xq, region, fitted=True))

    Xb = [X.copy() for X in Xs]
    Xb[bad][1] = Xb[bad][0]
    s2b = [sigma2] * len(Xs)
    s2b[bad] = 0.0
    others = [r for r in range(len(Xs)) if r != bad]
    for trend in (None, "constant"):
        sound, broken = run(Xs, [sigma2] * len(Xs), trend), run(Xb, s2b, trend)
        assert np.all(sound["info"] == 0) and broken["info"][bad] == 2 and np.all(np.delete(broken["info"], bad) == 0)
        for r in others:
            assert same_bits(broken["C"][r], sound["C"][r]) and same_bits(broken["beta"][r], sound["beta"][r]), (trend, r)
            assert broken["ev"][0][r] == sound["ev"][0][r] and same_bits(broken["ev"][1][r], sound["ev"][1][r]), (trend, r)
            assert same_bits(broken["loo"][0][r], sound["loo"][0][r]) and same_bits(broken["loo"][1][r], sound["loo"][1][r])
        keep = region != bad
        assert same_bits(broken["items"][0][keep], sound["items"][0][keep]), trend
        assert same_bits(broken["items"][1][keep], sound["items"][1][keep]), trend
        # the failed patch: only what include/pmk.h promises
        assert np.isnan(broken["ev"][0][bad]) and np.all(np.isnan(broken["ev"][1][bad]))
        assert np.all(np.isnan(broken["loo"][0][bad])) and np.all(np.isnan(broken["loo"][1][bad]))
        if trend is not None:
            assert np.all(np.isnan(broken["C"][bad])) and np.all(np.isnan(broken["beta"][bad]))

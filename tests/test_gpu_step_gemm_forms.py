"""The loop forms of the factorisation steps' GEMMs (pmk_mfma.h: gemm_nt, the pointer form, and gemm_nt_buf, the
buffer-load form; PMK_STEP_GEMM=ptr|buf|auto) issue the same MFMAs in the same order, so a fit must not depend on the
form by a single bit.  Three fresh child processes (tests/_step_gemm_worker.py), one per setting, fit the same cases;
every comparison here is np.array_equal on L, c, the -D^-1 blocks and info.

The two pure functions behind the choice -- the 32-bit extent predicate and the per-launch rule -- are checked without a
device."""
import os
import subprocess
import sys

import numpy as np
import pytest

import patchmixturekriging_amd as pmk

import _step_gemm_worker as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fits(tmp_path_factory):
    """form -> the worker's arrays; the three children run one after the other, once per module"""
    d = tmp_path_factory.mktemp("step_gemm")
    out = {}
    for form in ("ptr", "buf", "auto"):
        path = str(d / (form + ".npz"))
        env = dict(os.environ, PMK_STEP_GEMM=form)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_step_gemm_worker.py"), path], env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        with np.load(path) as z:
            out[form] = {k: z[k] for k in z.files}
    return out


def _same(fits, a, b, name, skip_patch=None):
    sizes = W.CASES[name][0]
    assert np.array_equal(fits[a][name + "/info"], fits[b][name + "/info"]), (name, a, b)
    for r in range(len(sizes)):
        if r == skip_patch:
            continue
        for what in ("L", "c", "ninv"):
            key = "%s/%d/%s" % (name, r, what)
            assert fits[a][key].shape == fits[b][key].shape and np.array_equal(fits[a][key], fits[b][key]), (key, a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n", W.TILE_SIZES)
def test_tile_counts_and_padded_waves(fits, n, dtype):
    """nt = 2, 3 and 5 with a ragged last tile; a last block row with waves entirely (n = 296) and partly (n = 328) in
    the identity padding"""
    name = "tiles-%d-%s" % (n, dtype)
    assert np.all(fits["ptr"][name + "/info"] == 0)
    _same(fits, "buf", "ptr", name)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("D", [1, 2, 3])
def test_ragged_batch_fused_and_unfused(fits, D, dtype):
    """P = 11 patches of 2, 3 and 5 tiles in one batch (end-aligned schedule, a remainder in the dealing over the XCDs);
    D = 2 and 3 evaluate the tiles below the diagonal inside the step kernel, D = 1 loads them"""
    name = "ragged-D%d-%s" % (D, dtype)
    assert np.all(fits["ptr"][name + "/info"] == 0)
    _same(fits, "buf", "ptr", name)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_not_positive_definite_patch(fits, dtype):
    """one patch of the batch fails at a pivot of its fourth tile: the same info under both forms, and every other
    patch's bits unchanged"""
    name = "notpd-%s" % dtype
    bad = W.CASES[name][3]
    info = fits["ptr"][name + "/info"]
    assert info[bad[0]] == bad[1] + 1 and np.all(np.delete(info, bad[0]) == 0), info
    _same(fits, "buf", "ptr", name, skip_patch=bad[0])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("D", [1, 2, 3])
def test_auto_equals_both_forced_forms(fits, D, dtype):
    """the default: by step_gemm_rule the buffer form in every launch of the fused fits (D = 2, 3) and the pointer form in
    the unfused ones (D = 1) -- test_launch_rule_... pins that down -- so each case differs in kernels from one of the two
    forced fits"""
    name = "ragged-D%d-%s" % (D, dtype)
    _same(fits, "auto", "ptr", name)
    _same(fits, "auto", "buf", name)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [16, 128, 1920])
def test_selftest_four_loop_forms_agree(K):
    """the library's self-test: gemm_nt, gemm_nt_indexed, gemm_nt_sbase and gemm_nt_buf bit for bit (a disagreement
    comes back as NaN; K = 128 and 1920 also run the buffer form with a J ring twice as deep as the I ring), and the
    common value against the exact integer product"""
    import ctypes as C
    ctx = pmk.default_context()
    rng = np.random.default_rng(K)
    MI = rng.integers(-8, 9, (K, 128)).astype(np.float64)        # MI[I + 128 k]
    MJ = rng.integers(-8, 9, (K, 32)).astype(np.float64)         # MJ[J + 32 k]
    Cout = np.empty((128, 32))
    dp = C.POINTER(C.c_double)
    rc = ctx.L.pmk_selftest_gemm(ctx.h, K, MI.ctypes.data_as(dp), MJ.ctypes.data_as(dp), Cout.ctypes.data_as(dp))
    assert rc == 0
    assert not np.isnan(Cout).any()
    assert np.array_equal(Cout, MI.T @ MJ)                       # integers: exact in fp64


# ------------------------------------------------------------------------------------------------ without a device
def test_extent_predicate_at_its_boundary():
    """(K + 4 pfj) ld elem_size < 2^31, on both sides of the bound, for both element sizes"""
    L = pmk.lib()
    ok = L.pmk_test_gemm_buf_extent_ok
    for es in (8, 4):
        for pfj in (4, 8):
            ld = 16384
            kmax = (2 ** 31 - 1) // (ld * es) - 4 * pfj          # the largest K that fits
            assert (kmax + 4 * pfj) * ld * es < 2 ** 31 <= (kmax + 1 + 4 * pfj) * ld * es
            assert ok(kmax, ld, pfj, es) == 1 and ok(kmax + 1, ld, pfj, es) == 0
    # the product exactly 2^31 is out, one element less is in
    assert ok(2 ** 14 - 16, 2 ** 14, 4, 8) == 0 and ok(2 ** 14 - 17, 2 ** 14, 4, 8) == 1
    # the workload (2000-point patches: K <= 1920, ld = 2048) is far inside; a 2 GiB slab is not
    assert ok(1920, 2048, 4, 8) == 1 and ok(16384, 16384, 4, 8) == 0 and ok(16384, 16384, 4, 4) == 1
    # 64-bit arguments do not wrap
    assert ok(2 ** 40, 2 ** 20, 4, 8) == 0 and ok(0, 128, 4, 8) == 0 and ok(128, 0, 4, 8) == 0


def test_launch_rule_is_a_function_of_its_four_arguments():
    """the rule has no other input (no patch count, no model): a pure C function of (G, k, dtype, fused) whose values
    are the same on every call, in whatever order the calls come (no state between them).  Its content: the buffer form
    (1) for the fused build, the pointer form (0) for the unfused one, at every (G, k) and element type -- tile counts
    that nobody measured included"""
    L = pmk.lib()
    rule = L.pmk_test_step_gemm_rule
    assert len(rule.argtypes) == 4
    args = [(G, k, f32, fused) for G in range(1, 40) for k in range(0, 40) for f32 in (0, 1) for fused in (0, 1)]
    first = [rule(*a) for a in args]
    assert first == [fused for (_, _, _, fused) in args]
    order = np.random.default_rng(1).permutation(len(args))
    for i in order:
        assert rule(*args[i]) == first[i]


@pytest.mark.gpu
def test_unknown_form_is_refused(monkeypatch):
    """a misspelt PMK_STEP_GEMM must not quietly run the default"""
    rng = np.random.default_rng(3)
    X = [rng.uniform(-4, 4, (300, 2))]
    y = [np.sin(X[0][:, 0])]
    monkeypatch.setenv("PMK_STEP_GEMM", "buff")
    with pytest.raises(pmk.PmkError, match="PMK_STEP_GEMM"):
        pmk.fit_patches(X, y, pmk.Spline34KernelType(1 / 3.0), 5e-2)
    monkeypatch.setenv("PMK_STEP_GEMM", "buf")
    _, _, info = pmk.fit_patches(X, y, pmk.Spline34KernelType(1 / 3.0), 5e-2)
    assert np.all(info == 0)

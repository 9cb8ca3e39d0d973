"""What tests/test_gpu_dispatch_stages.py relies on, asserted on the CPU of every input of tests/_dispatch_stage_cases.py, so
that the GPU bounds are the existing ones and nothing is tuned on the device:

  * kappa2(L) <= 10^3 for every patch and sigma2;
  * a plain numpy / LAPACK evaluation in the model's precision stays below one unit of each stage's reference;
  * no item is clamped, and every block aggregate lies 100 units above its floor (tests/test_block_refs.py);
  * every region holds items;
  * the kernels can be told apart: per (D, stage, precision) and region, the Spline34 and the Spline32 reference differ by
    more than 100 of the stage's units in at least one output, and so does either from the same stage evaluated with the
    other family on its own factor (what a launcher with the wrong FAM computes); for the DISTINCT lists every patch r >= 1
    differs by as much from the stage evaluated with patch 0's theta (what th_arg[0] in place of th_arg[region] computes;
    patch 0 is the uniform one by construction: a_0 = a, sigma2_0 = sigma2).
    These are conditions on the inputs, not tolerances.

Three inputs did not meet them as first drawn and were changed, no bound was: the header of tests/_dispatch_stage_cases.py
says which and why (DISTINCT ranges at D = 4; sigma2 of the covariance and of block kriging at D = 1 in fp32).

And the two-kernel reference (TwoKernel: a stage evaluated with theta_eval on a patch factored with theta_fit) is pinned to the
single-kernel references at theta_eval = theta_fit.
"""
import numpy as np
import pytest

import _block_refs as BR
import _dispatch_stage_cases as DC
import _vgrad_refs as VR
from _loo_refs import LD

P = DC.P
LISTS = DC.FAMS + ("distinct34", "distinct32", "mixed")
OTHER = {"spline34": "spline32", "spline32": "spline34"}
TWO_KERNEL_CASES = sorted(DC.TWO_KERNEL)                     # (d) of the GPU file: Spline32 on the Spline34 factor


@pytest.mark.parametrize("dtype", DC.DTYPES)
@pytest.mark.parametrize("D", DC.DIMS)
def test_every_input_meets_the_preconditions_of_its_units(D, dtype):
    w = DC.workload(D, dtype)
    assert all(len(w.sel[r]) > 0 for r in range(P))                                    # every region holds items
    assert len(w.Xq) == 257 and np.diff(w.items[0]).max() >= 2                          # and the blend has neighbours
    assert np.all(np.diff(w.group) >= 0) and np.any(w.a < 0) and np.any(w.a > 0)
    assert list(np.bincount(w.group)[:5]) == [1, 2, 3, 4, 5]
    for stage in DC.STAGES:
        for key in LISTS:
            hs = DC.hypers(w, key, stage)
            kappa = max(DC.region_ref(w, r, hs[r]).kappa for r in range(P))
            clamped = sum(DC.stage_outputs(w, key, stage, r)[2] for r in range(P))
            plain = DC.plain(w, key, stage)
            print("DISPATCHREF D=%d %s %-5s %-10s kappa2(L) %.3g plain / unit %.3g" % (D, dtype, stage, key, kappa, plain))
            assert kappa <= DC.KAPPA_MAX, (stage, key, kappa)
            assert clamped == 0, (stage, key, clamped)           # block: aggregates less than 100 units above their floor
            assert plain < 1.0, (stage, key, plain)
        if stage == "block":
            worst = min(x["margin"] for key in LISTS for x in DC.block_out(w, key)["aggs"])
            print("DISPATCHREF D=%d %s least margin in units %.3g" % (D, dtype, worst))
            assert worst >= DC.MARGIN_MIN


@pytest.mark.parametrize("dtype", DC.DTYPES)
@pytest.mark.parametrize("D", DC.DIMS)
def test_the_kernels_can_be_told_apart(D, dtype):
    w = DC.workload(D, dtype)
    for stage in DC.STAGES + ("block:kappa", "block:vn2"):       # the two pieces come from two kernels: each on its own
        for r in range(P):
            a, ua, _ = DC.stage_outputs(w, "spline34", stage, r)
            b, ub, _ = DC.stage_outputs(w, "spline32", stage, r)
            if stage != "grad":                              # the gradient of the mean is taken on each fit's own weights
                assert DC.ratio(np.abs(a - b), np.maximum(ua, ub)) > DC.APART_MIN, (stage, r)
            figs = [DC.apart(w, fam, stage, r, (OTHER[fam], DC.A)) for fam in DC.FAMS]
            if r >= 1:
                for key in ("distinct34", "distinct32"):
                    figs.append(DC.apart(w, key, stage, r, DC.hypers(w, key, stage[:5])[0][:2]))
            print("DISPATCHREF apart D=%d %s %-5s region %d: %s" % (D, dtype, stage, r, " ".join("%.3g" % f for f in figs)))
            assert min(figs) > DC.APART_MIN, (stage, r, figs)


@pytest.mark.parametrize("D,dtype", TWO_KERNEL_CASES)
def test_the_explicit_theta_cases_are_not_clamped(D, dtype):
    """Spline32 on the factor of a Spline34 fit is no posterior: k_eval(x, x) - |V|^2 need not be positive.  On these
    inputs (sigma2 of DC.TWO_KERNEL) it is, for every item and, by 100 units, for every block aggregate; and the result
    lies more than 100 units from the stage on the model's own kernel."""
    w = DC.workload(D, dtype)
    ev = ("spline32", DC.A)
    for stage in DC.STAGES:
        key = ("spline34", DC.TWO_KERNEL[(D, dtype)][stage])
        assert max(DC.region_ref(w, r, DC.hypers(w, key, stage)[r]).kappa for r in range(P)) <= DC.KAPPA_MAX
        assert sum(DC.stage_outputs(w, key, stage, r, ev)[2] for r in range(P)) == 0, stage
        assert DC.plain(w, key, stage) < 1.0
        figs = [DC.apart(w, key, stage, r, ev) for r in range(P)]
        print("DISPATCHREF two kernels D=%d %s %-5s apart %s" % (D, dtype, stage, " ".join("%.3g" % f for f in figs)))
        assert min(figs) > DC.APART_MIN, (stage, figs)
    worst = min(x["margin"] for x in DC.block_out(w, ("spline34", DC.TWO_KERNEL[(D, dtype)]["block"]), ev)["aggs"])
    print("DISPATCHREF two kernels D=%d %s least margin in units %.3g" % (D, dtype, worst))
    assert worst >= DC.MARGIN_MIN


def test_the_brownian_bridge_input_at_two_dimensions():
    for dtype in DC.BB_DTYPES:
        w = DC.workload(2, dtype, unit_square=True)
        assert all(len(w.sel[r]) > 0 for r in range(P)) and np.diff(w.items[0]).max() >= 2
        assert 0.05 < min(x.min() for x in w.Xs + [w.Xq]) and max(x.max() for x in w.Xs + [w.Xq]) < 0.95
        for stage in ("cov", "block"):
            hs = DC.hypers(w, "bb", stage)
            assert [h[0] for h in hs] == DC.BB_NAMES
            kappa = max(DC.region_ref(w, r, hs[r]).kappa for r in range(P))
            plain = DC.plain(w, "bb", stage)
            print("DISPATCHREF bb %s %-5s kappa2(L) %.3g plain / unit %.3g" % (dtype, stage, kappa, plain))
            assert kappa <= DC.KAPPA_MAX and plain < 1.0, (stage, kappa, plain)
            assert sum(DC.stage_outputs(w, "bb", stage, r)[2] for r in range(P)) == 0
        # the product over the coordinates is not the one-dimensional kernel of the first coordinate, nor of the distance
        ref = DC.region_ref(w, 1, DC.hypers(w, "bb", "cov")[1])
        x = np.asarray(w.Xs[1], dtype=LD)
        k1 = np.minimum(x[:, None, 0], x[None, :, 0]) - x[:, None, 0] * x[None, :, 0]
        k2 = np.minimum(x[:, None, 1], x[None, :, 1]) - x[:, None, 1] * x[None, :, 1]
        K = ref.U - LD(DC.hypers(w, "bb", "cov")[1][2]) * np.eye(ref.n, dtype=LD)
        assert np.abs(np.asarray(K - k1 * k2, dtype=np.float64)).max() <= 1e-18 and np.abs(np.asarray(K - k1, dtype=np.float64)).max() > 0.01


def test_two_kernels_are_the_single_kernel_references_at_the_same_theta():
    """on its own Cholesky (patch 1: 100 points) and on the shared factor"""
    w = DC.workload(2, "f64")
    h = DC.hypers(w, "distinct32", "cov")[1]
    oth = DC.kernel(*h[:2])[1]
    ref, xq = DC.region_ref(w, 1, h), w.points(1)
    addend = np.random.default_rng(1).uniform(0, 0.5, len(xq))
    for two in (DC.TwoKernel(oth, w.Xs[1], h[2], oth), DC.TwoKernel.on(ref, oth)):
        assert abs(two.kappa - ref.kappa) <= 1e-12 * ref.kappa
        for ad in (None, addend):
            got, want = two.cov(xq, ad), ref.cov(xq, ad)
            assert np.abs(np.asarray(got["S"] - want["S"], dtype=np.float64)).max() <= 1e-18
            assert np.allclose(got["unit"], want["unit"], rtol=1e-12, atol=0) and not got["clamped"].any()
        got, want = two.items(xq), VR.PatchRef(oth, w.Xs[1], h[2]).items(xq)
        assert np.abs(np.asarray(got["grad"] - want["grad"], dtype=np.float64)).max() <= 1e-17
        assert np.abs(np.asarray(got["v"] - want["v"], dtype=np.float64)).max() <= 1e-18
        assert np.allclose(got["unit"], want["unit"], rtol=1e-12, atol=0)
    # block kriging takes a TwoKernel as a region's reference
    refs = DC.refs_of(w, "distinct32", "block")
    same = {r: DC.TwoKernel.on(refs[r], refs[r].th) for r in refs}
    a = BR.block_ref(w.items[:2], w.items[2], w.owth, w.group, w.a, w.F, same, w.Xq, DC.U_OF["f64"])
    b = DC.block_out(w, "distinct32")
    assert np.abs(np.asarray(a["Var"] - b["Var"], dtype=np.float64)).max() <= 1e-18 and np.allclose(a["unit"], b["unit"], rtol=1e-12)
    # and with another theta it is another number: a larger range of the evaluated kernel leaves the factor alone
    other = DC.TwoKernel.on(ref, DC.kernel("spline32", 1.0)[1]).cov(xq)
    assert np.abs(np.asarray(other["S"] - ref.cov(xq)["S"], dtype=np.float64)).max() > 1e-3
    assert np.array_equal(DC.with_theta(ref, DC.kernel("spline32", 1.0)[1]).cov(xq, addend)["S"],
                          DC.TwoKernel.on(ref, DC.kernel("spline32", 1.0)[1]).cov(xq, addend)["S"])
    # the gradients of the item means, all items at once, are GR.item_grad_ref
    import _grad_refs as GR
    Cw = DC.lapack_weights(ref, w.Ys[1], "f64")
    G = DC.item_grads(oth, w.Xs[1], Cw, xq[:5])
    for i in range(5):
        assert np.abs(np.asarray(G[i] - GR.item_grad_ref(oth, w.Xs[1], Cw, xq[i]).T, dtype=np.float64)).max() <= 1e-17
    # the PatchRef on a shared factor is the PatchRef
    got, want = DC.patch_ref(w, 1, h).items(xq), VR.PatchRef(oth, w.Xs[1], h[2]).items(xq)
    assert np.array_equal(got["grad"], want["grad"]) and np.array_equal(got["unit"], want["unit"])
    # and the trend reference on a shared factor is the TrendRegionRef
    import _cov_multi_refs as CMR
    got, want = DC.region_ref(w, 1, h, DC.TREND).cov(xq), CMR.TrendRegionRef(oth, w.Xs[1], h[2], DC.TREND).cov(xq)
    assert np.array_equal(got["S"], want["S"]) and np.array_equal(got["unit"], want["unit"])
    # the PatchRef on the factor, C_H and L_G of a TrendRegionRef is the PatchRef under that trend
    got, want = DC.patch_ref(w, 1, h, DC.TREND).items(xq), VR.PatchRef(oth, w.Xs[1], h[2], DC.TREND).items(xq)
    for k in ("grad", "trend"):
        assert np.abs(np.asarray(got[k] - want[k], dtype=np.float64)).max() <= 1e-15 * np.abs(np.asarray(want[k], dtype=np.float64)).max()
    assert np.allclose(got["unit"], want["unit"], rtol=1e-9, atol=0) and np.allclose(got["tunit"], want["tunit"], rtol=1e-9, atol=0)
    # and with another kernel it is TwoKernel where there is no trend
    o32 = DC.kernel("spline32", 1.0)[1]
    got, want = DC.patch_ref(w, 1, h, None, ("spline32", 1.0)).items(xq), DC.TwoKernel.on(ref, o32).items(xq)
    assert np.abs(np.asarray(got["grad"] - want["grad"], dtype=np.float64)).max() <= 1e-17 and np.allclose(got["unit"], want["unit"], rtol=1e-12)

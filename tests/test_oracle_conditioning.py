"""The conditioning-ladder fixtures (tests/golden/conditioning_p{1,2}.npz, long double) against the CPU references that
tests/test_gpu_breakdown.py holds the device to: the oracle's fit_patch + queryinner stay within ONE QUARTER of every
bound asserted for the device, on every rung -- the standing proof that the bounds leave a correct fp64 solver room --
and the emulated plain fp32 pipeline stays inside the fp32 bounds."""
import numpy as np
import pytest

from _conditioning import BWD_F32, U32, U64, backward_error, fp32_pipeline, load, residual
from oracle import oracle as O


@pytest.mark.parametrize("name,D,n", [("p1", 2, 640), ("p2", 3, 1111)])
def test_fixture_layout(name, D, n):
    g = load(name)
    assert g["X"].shape == (n, D) and g["y"].shape == (n,) and g["y2"].shape == (n,) and g["Xq"].shape == (60, D)
    assert g["Xc"].shape == (257, D) and g["yc"].shape == (257,)
    assert g["sigma2_f64"].tolist() == [1e-4, 1e-6, 1e-8, 1e-10] and g["sigma2_f32"].tolist() == [1e-1, 1e-2, 1e-3]
    for tag, k in (("f64", 4), ("f32", 3)):
        assert g["c_" + tag].shape == (k, n) and g["mu_" + tag].shape == (k, 60) and g["var_" + tag].shape == (k, 60)
        assert np.all(np.diff(g["cond_" + tag]) > 0)
    assert g["c2_hard"].shape == (n,)
    assert 5e6 < g["cond_f64"][0] < 2e7 and 5e12 < g["cond_f64"][-1] < 1e13          # the ladder really is one
    # the last ten queries are training points (full cancellation in 1 - ||V||^2), the ten before them nearly are
    d = np.abs(g["Xq"][:, None, :] - g["X"][None, :, :]).max(2).min(1)
    assert np.all(d[50:] == 0) and np.all(d[40:50] < 1.001e-3) and np.all(d[40:50] > 0)
    assert g["var_f64"][-1][50:].max() < 2e-10 and g["var_f64"].min() > 0


@pytest.mark.parametrize("name", ["p1", "p2"])
def test_oracle_stays_within_a_quarter_of_every_bound(name):
    g = load(name)
    X, y, Xq = g["X"], g["y"], g["Xq"]
    oth = O.kernel(O.SPLINE34, float(g["theta"]))
    K = O.kernel_matrix(oth, X)
    for tag in ("f64", "f32"):
        for i, sigma2 in enumerate(g["sigma2_" + tag]):
            sigma2, cond = float(sigma2), float(g["cond_" + tag][i])
            c_ref, mu_ref, v_ref = g["c_" + tag][i], g["mu_" + tag][i], g["var_" + tag][i]
            U = K + sigma2 * np.eye(len(y))
            f = O.fit_patch(oth, X, y, sigma2)
            assert f["info"] == 0
            mv = np.array([O.queryinner(oth, X, f["c_lu"], f["L"], xq) for xq in Xq])
            figures = dict(
                bwd=backward_error(f["L"], U) / 1e-14,
                res=max(residual(U, f["c_lu"], y), residual(U, f["c_chol"], y)) / 1e-13,
                fwd=max(np.linalg.norm(f[k] - c_ref) / np.linalg.norm(c_ref) for k in ("c_lu", "c_chol")) / (cond * U64),
                dY=(np.abs(mv[:, 0] - mu_ref) / (1e-7 * np.maximum(1, np.abs(mu_ref)))).max(),
                dV=(np.abs(mv[:, 1] - np.maximum(v_ref, 1e-12)) / (1e-9 + 1e-5 * v_ref)).max())
            print(name, "sigma2 %.0e cond2 %.2e" % (sigma2, cond), {k: "%.2e" % v for k, v in figures.items()})
            assert all(v <= 0.25 for v in figures.values()), (name, sigma2, figures)


@pytest.mark.parametrize("name", ["p1", "p2"])
def test_plain_fp32_pipeline_stays_inside_the_fp32_bounds_but_not_inside_the_flat_mean_bound(name):
    g = load(name)
    X, y, Xq = g["X"], g["y"], g["Xq"]
    oth = O.kernel(O.SPLINE34, float(g["theta"]))
    K, Kq = O.kernel_matrix(oth, X), O.cross_kernel_matrix(oth, X, Xq)
    dmus = []
    for i, sigma2 in enumerate(g["sigma2_f32"]):
        sigma2, cond = float(sigma2), float(g["cond_f32"][i])
        c_ref, mu_ref, v_ref = g["c_f32"][i], g["mu_f32"][i], g["var_f32"][i]
        U = K + sigma2 * np.eye(len(y))
        info, L, c, mu, var = fp32_pipeline(U, y, Kq)
        bwd = backward_error(L, U)
        fwd = np.linalg.norm(c - c_ref) / np.linalg.norm(c_ref)
        dv = (np.abs(var - np.maximum(v_ref, 1e-12)) / (5e-5 + 2e-3 * v_ref)).max()
        dmus.append(np.abs(mu - mu_ref).max())
        print(name, "sigma2 %.0e cond2 %.2e bwd %.2e fwd/(cond u32) %.2f dV/tol %.3f max|dmu| %.2e"
              % (sigma2, cond, bwd, fwd / (cond * U32), dv, dmus[-1]))
        assert info == 0 and bwd <= BWD_F32 / 4 and fwd <= cond * U32 / 2 and dv <= 0.25
    # the finding behind the fp32 mean bound of the GPU test: a flat 1e-4 is a statement about well-conditioned fits
    assert max(dmus) > 1e-4

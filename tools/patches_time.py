"""Per-patch kernels and noise at config C (256 patches x 2000 points, 2-D Spline34(1/15), sigma2 = 1e-5, 2^20 queries):
stage times on HIP events (pmk_ctx_timer_ms), median of --reps after one warm-up, all in one process, of

  (a) pmk_model_fit, fused kernel-matrix build (as shipped)
  (b) pmk_model_fit with PMK_FUSE_K1=0 (the whole lower triangle is built, then factorised): what a per-patch fit runs
  (c) pmk_model_fit_patches with 256 copies of one theta and sigma2
  (d) pmk_model_fit_patches with 256 distinct a_r (1/15 +- 10 %) and sigma2_r (1e-5 .. 1e-4)
  (e) pmk_query_items(theta) against pmk_query_items_fitted on the same plan of --nq queries
  (f) the same for the mean-only multi-output path at R = 1 (pmk_query_items_multi / _multi_fitted, want_var = 0)

The per-patch kernels run the instruction stream of the unfused uniform ones plus one descriptor load per workgroup or
task, so (c) and (d) are expected at (b), and the *_fitted items at the explicit-theta items, within 3 %.  The weights
of (c) are compared with those of (b), bit for bit.

Writes the JSON to --out (default profiles/patches_time_C.json) and prints it.  --fit-only times (a) alone (for a library
that does not have the per-patch entry points).
Usage: python tools/patches_time.py [--reps 5] [--nq 1048576] [--out FILE] [--fit-only]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import patchmixturekriging_amd as pmk                      # noqa: E402
from patchmixturekriging_amd import mixture as M           # noqa: E402


def med(v):
    return float(np.median(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nq", type=int, default=1 << 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "patches_time_C.json"))
    ap.add_argument("--fit-only", action="store_true")
    args = ap.parse_args()
    P, levels, a, sigma2, delta = 256, 9, 1 / 15, 1e-5, 1e-5
    rng = np.random.Generator(np.random.PCG64(25))
    N = 512000
    X = np.stack([rng.uniform(-5, 5, N), rng.uniform(-10, 10, N)], 1)
    Xq = np.stack([rng.uniform(-5, 5, args.nq), rng.uniform(-10, 10, args.nq)], 1)
    y = np.sin(X[:, 0]) * np.cos(0.5 * X[:, 1])
    radius = 0.1 * np.sqrt(200.0 / P)
    root, X_parts, X_inds = pmk.setuppartition(X, levels, device=True)
    ys = [y[i] for i in X_inds]
    th, wth = pmk.Spline34KernelType(a), pmk.Spline34KernelType(1 / radius)
    ctx = pmk.default_context()
    ctx.enable_timers(True)
    model = M.DeviceModel(X_parts, ys)

    def time_fit(run):
        fit, k1, chol = [], [], []
        for _ in range(args.reps + 1):
            run()
            assert np.all(model.info() == 0)
            fit.append(ctx.timer_ms("fit"))
            k1.append(ctx.timer_ms("kernel_matrix"))
            chol.append(ctx.timer_ms("cholesky"))
        return {"fit_ms": med(fit[1:]), "kernel_matrix_ms": med(k1[1:]), "cholesky_ms": med(chol[1:]), "fit_ms_all": fit[1:]}

    out = {"tool": "patches_time", "config": "C", "patches": P, "reps": args.reps,
           "n": [int(min(len(x) for x in X_parts)), int(max(len(x) for x in X_parts))], "queries": args.nq}
    os.environ.pop("PMK_FUSE_K1", None)
    out["a_fit_fused"] = time_fit(lambda: model.fit(th, sigma2))
    if not args.fit_only:
        os.environ["PMK_FUSE_K1"] = "0"
        out["b_fit_unfused"] = time_fit(lambda: model.fit(th, sigma2))
        wb = model.weights()
        os.environ.pop("PMK_FUSE_K1", None)
        out["c_fit_patches_copies"] = time_fit(lambda: model.fit_patches([th] * P, [sigma2] * P))
        # faster and different is not faster: at the size that is timed, the weights of all patches, bit for bit
        out["c_weights_bit_identical_to_b"] = bool(all(np.array_equal(u, v) for u, v in zip(wb, model.weights())))
        prng = np.random.Generator(np.random.PCG64(26))
        ths = [pmk.Spline34KernelType(a * f) for f in prng.uniform(0.9, 1.1, P)]
        s2s = (1e-5 * 10 ** prng.uniform(0.0, 1.0, P)).tolist()
        out["d_fit_patches_distinct"] = time_fit(lambda: model.fit_patches(ths, s2s))
        b = out["b_fit_unfused"]["fit_ms"]
        out["c_over_b"] = out["c_fit_patches_copies"]["fit_ms"] / b
        out["d_over_b"] = out["d_fit_patches_distinct"]["fit_ms"] / b
        # predict on the model of (d): explicit theta against the model's own kernels, same plan
        model.set_bsp(root, 0)
        q = M.DeviceQuery(model, Xq)
        q.plan(radius, delta)
        t_exp, t_fit = [], []
        for _ in range(args.reps + 1):
            q.items(th)
            q.mix(wth)
            q.fetch()
            t_exp.append(ctx.timer_ms("items"))
            q.items_fitted()
            q.mix(wth)
            Yq, Vq = q.fetch()
            t_fit.append(ctx.timer_ms("items"))
        out["e_items_ms"] = med(t_exp[1:])
        out["e_items_fitted_ms"] = med(t_fit[1:])
        out["e_fitted_over_explicit"] = out["e_items_fitted_ms"] / out["e_items_ms"]
        out["items"] = int(q.total)
        model.set_targets_multi(ys)
        model.solve_multi()
        t_exp, t_fit = [], []
        for _ in range(args.reps + 1):
            q.items_multi(th, False)
            q.mix_multi(wth)
            q.fetch_multi(1)
            t_exp.append(ctx.timer_ms("items_multi"))
            q.items_multi_fitted(False)
            q.mix_multi(wth)
            Ym, _ = q.fetch_multi(1)
            t_fit.append(ctx.timer_ms("items_multi"))
        out["f_items_multi_mean_ms"] = med(t_exp[1:])
        out["f_items_multi_fitted_mean_ms"] = med(t_fit[1:])
        out["f_fitted_over_explicit"] = out["f_items_multi_fitted_mean_ms"] / out["f_items_multi_mean_ms"]
        out["finite"] = bool(np.all(np.isfinite(Yq)) and np.all(np.isfinite(Vq)) and np.all(np.isfinite(Ym)))
    out["fit_shader_clock_ghz"] = ctx.shader_clock(0)
    text = json.dumps(out, indent=1)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""Multi-output targets at config C (256 patches x 2000 points, 2-D Spline34(1/15), sigma2 = 1e-5, 2^20 queries): stage
times on HIP events (pmk_ctx_timer_ms) of

  - the fit (kernel matrix + Cholesky + solve) once, then pmk_model_solve_multi for R = 1, 4, 16 from the resident factor,
    against R separate fits (R x the measured fit);
  - the multi-output prediction for R = 1, 4, 16 with and without the variance: plan, items_multi, mix_multi, and the
    single-output pmk_query_items (strip kernel) for reference.

Prints one JSON line.  Usage: python tools/multi_output_time.py [--reps 5] [--nq 1048576]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import patchmixturekriging_amd as pmk                      # noqa: E402
from patchmixturekriging_amd import mixture as M           # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nq", type=int, default=1 << 20)
    args = ap.parse_args()
    P, levels, a, sigma2, delta = 256, 9, 1 / 15, 1e-5, 1e-5
    rng = np.random.Generator(np.random.PCG64(25))
    N = 512000
    X = np.stack([rng.uniform(-5, 5, N), rng.uniform(-10, 10, N)], 1)
    Xq = np.stack([rng.uniform(-5, 5, args.nq), rng.uniform(-10, 10, args.nq)], 1)
    radius = 0.1 * np.sqrt(200.0 / P)
    root, X_parts, X_inds = pmk.setuppartition(X, levels, device=True)
    Yall = np.stack([np.sin((0.5 + 0.1 * j) * X[:, 0]) * np.cos(0.3 * X[:, 1]) for j in range(16)], 1)
    Ys = [np.asfortranarray(Yall[i]) for i in X_inds]
    th, wth = pmk.Spline34KernelType(a), pmk.Spline34KernelType(1 / radius)
    ctx = pmk.default_context()
    ctx.enable_timers(True)
    model = M.DeviceModel(X_parts, [y[:, 0].copy() for y in Ys])

    def med(v):
        return float(np.median(v))

    fit = []
    for _ in range(args.reps + 1):
        model.fit(th, sigma2)
        assert np.all(model.info() == 0)
        fit.append(ctx.timer_ms("fit"))
    fit_ms = med(fit[1:])
    out = {"tool": "multi_output_time", "config": "C", "patches": P, "n": [int(min(len(x) for x in X_parts)),
                                                                           int(max(len(x) for x in X_parts))],
           "queries": args.nq, "fit_ms": fit_ms, "solve_multi_ms": {}, "separate_fits_ms": {}, "predict": {}}
    model.set_bsp(root, 0)
    for R in (1, 4, 16):
        model.set_targets_multi([y[:, :R] for y in Ys])
        t = []
        for _ in range(args.reps + 1):
            model.solve_multi()
            t.append(ctx.timer_ms("solve_multi"))
        out["solve_multi_ms"][str(R)] = med(t[1:])
        out["separate_fits_ms"][str(R)] = R * fit_ms
        q = M.DeviceQuery(model, Xq)
        for var in (False, True):
            tp, ti, tm = [], [], []
            for _ in range(max(2, args.reps // 2) + 1):
                q.plan(radius, delta)
                tp.append(ctx.timer_ms("plan"))
                q.items_multi(th, var)
                q.mix_multi(wth)
                Yq, Vq = q.fetch_multi(R)
                ti.append(ctx.timer_ms("items_multi"))
                tm.append(ctx.timer_ms("mix_multi"))
            out["predict"]["R%d_%s" % (R, "var" if var else "mean")] = {
                "plan_ms": med(tp[1:]), "items_multi_ms": med(ti[1:]), "mix_multi_ms": med(tm[1:]),
                "total_ms": med(tp[1:]) + med(ti[1:]) + med(tm[1:]), "items": int(q.total),
                "finite": bool(np.all(np.isfinite(Yq)))}
        del q
    q = M.DeviceQuery(model, Xq)
    q.plan(radius, delta)
    ts = []
    for _ in range(3):
        q.items(th)
        q.mix(wth)
        q.fetch()
        ts.append(ctx.timer_ms("items"))
    out["single_output_items_ms"] = med(ts[1:])
    print(json.dumps(out))


if __name__ == "__main__":
    main()

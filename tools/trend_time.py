"""Kriging with a trend at config C (256 patches x 2000 points, 2-D Spline34(1/15), sigma2 = 1e-5, 2^20 queries), R = 1:
what the trend adds to pmk_model_solve_multi and to a prediction with variance, for trend none / constant / linear.

Stage times on HIP events (pmk_ctx_timer_ms), the median of --reps runs after one warm-up, all in one process:

  solve     "solve_multi" (with a trend: the fill of H and the solve of R + q columns) + "trend_gls"
  predict   "items_multi" (means of R + q columns, then the variance strips) + "trend_items" + "mix_multi" on one plan

The trend is expected to add only the fill, the GLS and the epilogue launches: the solve kernel's time does not depend on
the number of columns, and the items kernel always runs 16.

--no-trend measures the trend-free figures only and never calls pmk_model_set_trend.  The parent's figures are taken by
copying this file into a checkout of the parent commit and running it there with --no-trend (the Python package of this
commit refuses to load a library that lacks the trend symbols, so PMK_LIB alone does not do); --parent then folds that
JSON into the output.

Writes one JSON object to --out (default profiles/trend_time_C.json) and prints it.
Usage: python tools/trend_time.py [--reps 5] [--nq 1048576] [--no-trend] [--parent parent.json] [--out FILE]
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


def timer(ctx, name):
    try:
        return ctx.timer_ms(name)
    except pmk.PmkError:
        return 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nq", type=int, default=1 << 20)
    ap.add_argument("--no-trend", action="store_true")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trend_time_C.json"))
    args = ap.parse_args()
    P, levels, a, sigma2, delta = 256, 9, 1 / 15, 1e-5, 1e-5
    rng = np.random.Generator(np.random.PCG64(25))
    N = 512000
    X = np.stack([rng.uniform(-5, 5, N), rng.uniform(-10, 10, N)], 1)
    Xq = np.stack([rng.uniform(-5, 5, args.nq), rng.uniform(-10, 10, args.nq)], 1)
    radius = 0.1 * np.sqrt(200.0 / P)
    root, X_parts, X_inds = pmk.setuppartition(X, levels, device=True)
    y = np.sin(0.5 * X[:, 0]) * np.cos(0.3 * X[:, 1]) + 2.0 + 0.3 * X[:, 0]
    ys = [y[i].copy() for i in X_inds]
    th, wth = pmk.Spline34KernelType(a), pmk.Spline34KernelType(1 / radius)
    ctx = pmk.default_context()
    ctx.enable_timers(True)
    model = M.DeviceModel(X_parts, ys)
    model.fit(th, sigma2)
    assert np.all(model.info() == 0)
    model.set_targets_multi(ys)
    model.set_bsp(root, 0)
    out = {"tool": "trend_time", "config": "C", "patches": P, "R": 1, "queries": args.nq, "reps": args.reps,
           "n": [int(min(len(x) for x in X_parts)), int(max(len(x) for x in X_parts))], "trend": {}}
    q = M.DeviceQuery(model, Xq)
    q.plan(radius, delta)
    out["items"] = int(q.total)
    for trend in (["none"] if args.no_trend else ["none", "constant", "linear"]):
        if not args.no_trend:
            model.set_trend(trend)
        ts, tg = [], []
        for _ in range(args.reps + 1):
            model.solve_multi()
            ctx.synchronize()
            ts.append(timer(ctx, "solve_multi"))
            tg.append(timer(ctx, "trend_gls") if trend != "none" else 0.0)
        ti, te, tm = [], [], []
        for _ in range(args.reps + 1):
            q.items_multi(th, True)
            q.mix_multi(wth)
            Yq, Vq = q.fetch_multi(1)
            ti.append(timer(ctx, "items_multi"))
            te.append(timer(ctx, "trend_items") if trend != "none" else 0.0)
            tm.append(timer(ctx, "mix_multi"))
        out["trend"][trend] = {
            "solve_multi_ms": med(ts[1:]), "trend_gls_ms": med(tg[1:]), "solve_total_ms": med(np.add(ts, tg)[1:]),
            "items_multi_ms": med(ti[1:]), "trend_items_ms": med(te[1:]), "mix_multi_ms": med(tm[1:]),
            "predict_total_ms": med((np.add(ti, te) + tm)[1:]),
            "finite": bool(np.all(np.isfinite(Yq)) and np.all(np.isfinite(Vq)))}
    if args.parent:
        parent = json.load(open(args.parent))["trend"]["none"]
        mine = out["trend"]["none"]
        out["parent_none"] = parent
        out["none_over_parent"] = {k: mine[k] / parent[k] for k in ("solve_total_ms", "predict_total_ms")}
    txt = json.dumps(out, indent=1, sort_keys=True)
    with open(args.out, "w") as f:
        f.write(txt + "\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()

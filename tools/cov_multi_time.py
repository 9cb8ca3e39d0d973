"""Joint covariance on the multi-output path under a linear trend at config C (256 patches x 2000 points, 2-D
Spline34(1/15), sigma2 = 1e-5, fp64, R = 1) for Nq = 1024, 4096 and 16384 queries: what the trend's term costs beside the
covariance sweep it follows.

Stage times on HIP events (pmk_ctx_timer_ms), the median of --reps runs after one warm-up, all in one process and on one
plan per Nq:

  items_cov        pmk_query_items_cov: the covariance sweep, the Gram and the region blocks (no trend's term)
  items_cov_multi  pmk_query_items_cov_multi: the same three kernels, then z per item and z_a . z_b per block entry
  cov_trend        the trend's stage alone (its timer lies inside "items_cov")
  mix_cov          the gather-form blend into the Nq x Nq result, after pmk_query_items_cov_multi

The two items_cov figures come from alternating calls on the same plan in the same run.  extra_bytes is what the query owns
on top of pmk_query_items_cov's arenas: 40 bytes per item (z, TQ_MAX = 5 doubles) and 4 bytes per patch (the marks).

Writes one JSON object to --out (default profiles/cov_multi_time_C.json) and prints it.
Usage: python tools/cov_multi_time.py [--reps 5] [--nq 1024,4096,16384] [--out FILE]
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

TQ_MAX = 5


def med(v):
    return float(np.median(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nq", default="1024,4096,16384")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cov_multi_time_C.json"))
    args = ap.parse_args()
    P, levels, a, sigma2, delta, D = 256, 9, 1 / 15, 1e-5, 1e-5, 2
    rng = np.random.Generator(np.random.PCG64(25))
    N = 512000
    X = np.stack([rng.uniform(-5, 5, N), rng.uniform(-10, 10, N)], 1)
    radius = 0.1 * np.sqrt(200.0 / P)
    root, X_parts, X_inds = pmk.setuppartition(X, levels, device=True)
    y = np.sin(0.5 * X[:, 0]) * np.cos(0.3 * X[:, 1]) + 2.0 + 0.3 * X[:, 0]
    th, wth = pmk.Spline34KernelType(a), pmk.Spline34KernelType(1 / radius)
    ctx = pmk.default_context()
    ctx.enable_timers(True)
    ys = [y[i].copy() for i in X_inds]
    model = M.DeviceModel(X_parts, ys)
    model.set_bsp(root, 0)
    model.fit(th, sigma2)
    assert np.all(model.info() == 0)
    model.set_targets_multi(ys)
    model.set_trend("linear")
    model.solve_multi()
    assert np.all(model.trend_info() == 0)
    out = {"tool": "cov_multi_time", "config": "C", "patches": P, "D": D, "R": 1, "trend": "linear", "reps": args.reps,
           "dtype": "f64", "n": [int(min(len(x) for x in X_parts)), int(max(len(x) for x in X_parts))], "Nq": {}}
    for Nq in [int(v) for v in args.nq.split(",")]:
        Xq = np.stack([rng.uniform(-5, 5, Nq), rng.uniform(-10, 10, Nq)], 1)
        q = M.DeviceQuery(model, Xq)
        q.plan(radius, delta)
        t = {k: [] for k in ("items_cov", "items_cov_multi", "cov_trend", "mix_cov")}
        for _ in range(args.reps + 1):
            q.items_multi_fitted(True)
            q.mix_multi(wth)
            q.items_cov()
            ctx.synchronize()
            t["items_cov"].append(ctx.timer_ms("items_cov"))
            q.items_cov_multi()
            q.mix_cov(wth)
            Yq, Vq = q.fetch_multi(1)                   # blocks: the stages above have run
            t["items_cov_multi"].append(ctx.timer_ms("items_cov"))
            t["cov_trend"].append(ctx.timer_ms("cov_trend"))
            t["mix_cov"].append(ctx.timer_ms("mix_cov"))
        r = {k + "_ms": med(v[1:]) for k, v in t.items()}
        r.update({k + "_runs_ms": v[1:] for k, v in t.items()})
        r["items_cov_multi_over_items_cov"] = r["items_cov_multi_ms"] / r["items_cov_ms"]
        r["items"] = int(q.total)
        r["extra_bytes"] = {"z": int(8 * TQ_MAX * q.total), "marks": int(4 * P), "total": int(8 * TQ_MAX * q.total + 4 * P)}
        r["finite"] = bool(np.all(np.isfinite(Yq)) and np.all(np.isfinite(Vq)))
        if Nq <= 4096:
            Cov = q.fetch_cov()
            r["finite"] = r["finite"] and bool(np.all(np.isfinite(Cov)))
            r["max_abs_diag_minus_vq"] = float(np.abs(np.diag(Cov) - Vq).max())
        out["Nq"][str(Nq)] = r
        del q
    txt = json.dumps(out, indent=1, sort_keys=True)
    with open(args.out, "w") as f:
        f.write(txt + "\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()

"""Joint covariance of a query batch at config C (256 patches x 2000 points, 2-D Spline34(1/15), sigma2 = 1e-5, fp64) for
Nq = 1024, 4096 and 16384 queries: what the covariance stages cost beside the prediction sweep over the same items.

Stage times on HIP events (pmk_ctx_timer_ms), the median of --reps runs after one warm-up, all in one process and on one
plan per Nq:

  items      pmk_query_items_fitted: the existing strip sweep over the plan's items (means and variances)
  items_cov  the covariance sweep (the same triangular solves, every block row stored to the V arena), the Gram of the
             arena's columns on the MFMA and the region blocks
  mix_cov    the gather-form blend into the Nq x Nq result

items_cov_over_items is the figure the covariance sweep is measured against.  The arena bytes are those the library
allocates for the plan: sum over strips of ld x 256 x 8, 8 sum m_r^2 of region blocks and 8 Nq^2 of result.

Writes one JSON object to --out (default profiles/cov_time_C.json) and prints it.
Usage: python tools/cov_time.py [--reps 5] [--nq 1024,4096,16384] [--out FILE]
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

TQ, TILE = 256, 128


def med(v):
    return float(np.median(v))


def arena_bytes(counts, n, Nq):
    """(V arena, region blocks, result) in bytes for the items per region `counts` and the patch sizes n (fp64)"""
    ld = TILE * ((np.asarray(n) + TILE - 1) // TILE)
    strips = (np.asarray(counts) + TQ - 1) // TQ
    return int((strips * ld * TQ * 8).sum()), int(8 * (np.asarray(counts) ** 2).sum()), int(8 * Nq * Nq)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nq", default="1024,4096,16384")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cov_time_C.json"))
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
    model = M.DeviceModel(X_parts, [y[i].copy() for i in X_inds])
    model.set_bsp(root, 0)
    model.fit(th, sigma2)
    assert np.all(model.info() == 0)
    out = {"tool": "cov_time", "config": "C", "patches": P, "D": D, "reps": args.reps, "dtype": "f64",
           "n": [int(min(len(x) for x in X_parts)), int(max(len(x) for x in X_parts))], "Nq": {}}
    stages = ["items", "items_cov", "mix_cov"]
    for Nq in [int(v) for v in args.nq.split(",")]:
        Xq = np.stack([rng.uniform(-5, 5, Nq), rng.uniform(-10, 10, Nq)], 1)
        q = M.DeviceQuery(model, Xq)
        q.plan(radius, delta)
        counts = np.diff(q.region_offsets(P))
        t = {k: [] for k in stages}
        for _ in range(args.reps + 1):
            q.items_fitted()
            q.mix(wth)
            q.items_cov()
            q.mix_cov(wth)
            Yq, Vq = q.fetch()                          # blocks: the stages above have run
            for k in t:
                t[k].append(ctx.timer_ms(k))
        r = {k + "_ms": med(v[1:]) for k, v in t.items()}
        r.update({k + "_runs_ms": v[1:] for k, v in t.items()})
        r["items_cov_over_items"] = r["items_cov_ms"] / r["items_ms"]
        r["items"] = int(q.total)
        r["strips"] = int(((counts + TQ - 1) // TQ).sum())
        va, sb, cb = arena_bytes(counts, model.n, Nq)
        r["arena_bytes"] = {"V": va, "blocks": sb, "result": cb, "total": va + sb + cb}
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

"""Appending observations in place at config C (256 patches x 2000 points, 2-D Spline34(1/15), sigma2 = 1e-5, fp64; a
patch of 2000 points has ld = 2048, so 48 free rows) against building and fitting a fresh model of the extended sets.

Variants: 1, 16 and 48 new points to every patch, and 8 new points to 4 patches.  Per variant and repetition a model of the
original sets is created and fitted, the append runs once, and a fresh model of the extended sets is created and fitted,
all in one process; the median of --reps repetitions after one warm-up.

  append_sweep   the covariance sweep over the appended items (strip kernel, Gram, blocks): V and S
  append_border  append_border_kernel, one workgroup per receiving patch
  append_solve   the back substitution over all patches
      on HIP events (pmk_ctx_timer_ms)
  append_call    host clock around DeviceModel.append up to a synchronise: the three stages plus the staging of the items
                 (host grouping, uploads, one stream synchronise) and the info read-back
  fresh_fit      the "fit" timer of the fresh model (kernel matrix, factorisation, solves), HIP events
  fresh_call     host clock around DeviceModel(...) + fit + info of the fresh model

Writes one JSON object to --out (default profiles/append_time_C.json) and prints it.
Usage: python tools/append_time.py [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import patchmixturekriging_amd as pmk                      # noqa: E402
from patchmixturekriging_amd import mixture as M           # noqa: E402

STAGES = ["append_sweep", "append_border", "append_solve"]


def med(v):
    return float(np.median(v))


def target(X):
    return np.sin(0.5 * X[:, 0]) * np.cos(0.3 * X[:, 1]) + 2.0 + 0.3 * X[:, 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "append_time_C.json"))
    args = ap.parse_args()
    P, levels, a, sigma2 = 256, 9, 1 / 15, 1e-5
    rng = np.random.Generator(np.random.PCG64(25))
    N = 512000
    X = np.stack([rng.uniform(-5, 5, N), rng.uniform(-10, 10, N)], 1)
    root, X_parts, X_inds = pmk.setuppartition(X, levels, device=True)
    y_parts = [target(x) for x in X_parts]
    th = pmk.Spline34KernelType(a)
    ctx = pmk.default_context()
    ctx.enable_timers(True)
    lo, hi = [x.min(0) for x in X_parts], [x.max(0) for x in X_parts]
    variants = [("1_to_every_patch", 1, P), ("16_to_every_patch", 16, P), ("48_to_every_patch", 48, P),
                ("8_to_4_patches", 8, 4)]
    out = {"tool": "append_time", "config": "C", "patches": P, "D": 2, "reps": args.reps, "dtype": "f64",
           "n": [int(min(len(x) for x in X_parts)), int(max(len(x) for x in X_parts))], "variants": {}}
    for name, m, npatch in variants:
        # new points inside the bounding box of their patch
        Xn = [rng.uniform(lo[r], hi[r], (m if r < npatch else 0, 2)) for r in range(P)]
        yn = [target(x) for x in Xn]
        Xe = [np.ascontiguousarray(np.vstack([x, xn])) for x, xn in zip(X_parts, Xn)]
        ye = [np.concatenate([y, v]) for y, v in zip(y_parts, yn)]
        t = {k: [] for k in STAGES + ["append_call", "fit", "fresh_fit", "fresh_call"]}
        worst = 0.0
        for _ in range(args.reps + 1):
            model = M.DeviceModel(X_parts, y_parts)
            model.fit(th, sigma2)
            assert np.all(model.info() == 0)
            t["fit"].append(ctx.timer_ms("fit"))
            assert int(model.capacity().min()) >= m
            ctx.synchronize()
            t0 = time.perf_counter()
            info = model.append(Xn, yn)
            ctx.synchronize()
            t["append_call"].append(1e3 * (time.perf_counter() - t0))
            assert np.all(info == 0)
            for k in STAGES:
                t[k].append(ctx.timer_ms(k))
            c_app = model.weights()
            del model
            ctx.synchronize()
            t0 = time.perf_counter()
            fresh = M.DeviceModel(Xe, ye)
            fresh.fit(th, sigma2)
            assert np.all(fresh.info() == 0)
            t["fresh_call"].append(1e3 * (time.perf_counter() - t0))
            t["fresh_fit"].append(ctx.timer_ms("fit"))
            c_new = fresh.weights()
            del fresh
            # the two sets of weights agree as two evaluations of one ill-conditioned solve do (sigma2 = 1e-5)
            worst = max(worst, max(float(np.abs(u - v).max() / np.abs(v).max()) for u, v in zip(c_app, c_new)))
        r = {k + "_ms": med(v[1:]) for k, v in t.items()}
        r.update({k + "_runs_ms": v[1:] for k, v in t.items()})
        r["append_stages_ms"] = sum(r[k + "_ms"] for k in STAGES)
        r["fresh_fit_over_append_stages"] = r["fresh_fit_ms"] / r["append_stages_ms"]
        r["items"] = int(m * npatch)
        r["max_rel_weight_difference"] = worst
        out["variants"][name] = r
    txt = json.dumps(out, indent=1, sort_keys=True)
    with open(args.out, "w") as f:
        f.write(txt + "\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()

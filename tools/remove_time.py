"""Removing observations in place at config C (256 patches x 2000 points, 2-D Spline34(1/15), sigma2 = 1e-5, fp64; a
patch of 2000 points has nt = 16 and can lose 79 rows) against building and fitting a fresh model of the reduced sets.

Variants: one row of every patch at k0 = 0 (the first row: everything is transformed, the worst case), at a random row and
at k0 = n - 1 (the last row: nothing is), 8 and 32 random rows of every patch (32 is PMK_REMOVE_MAX_ROWS), and 8 random
rows of 4 patches.  Per variant and repetition a model of the original sets is created and fitted, the removal runs once,
and a fresh model of the reduced sets is created and fitted, all in one process; the median of --reps repetitions after
one warm-up.

  remove_rows    remove_rows_kernel, one workgroup per patch that loses rows: compaction, reflector sweep, padding, -D^-1
  remove_solve   the back substitution over all patches
      on HIP events (pmk_ctx_timer_ms)
  remove_call    host clock around DeviceModel.remove up to a synchronise: the two stages plus the staging of the row list
                 (host grouping, uploads, one stream synchronise) and the info read-back
  fresh_fit      the "fit" timer of the fresh model (kernel matrix, factorisation, solves), HIP events
  fresh_call     host clock around DeviceModel(...) + fit + info of the fresh model

Writes one JSON object to --out (default profiles/remove_time_C.json) and prints it.
Usage: python tools/remove_time.py [--reps 5] [--out FILE]
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

STAGES = ["remove_rows", "remove_solve"]


def med(v):
    return float(np.median(v))


def target(X):
    return np.sin(0.5 * X[:, 0]) * np.cos(0.3 * X[:, 1]) + 2.0 + 0.3 * X[:, 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "remove_time_C.json"))
    args = ap.parse_args()
    P, levels, a, sigma2 = 256, 9, 1 / 15, 1e-5
    rng = np.random.Generator(np.random.PCG64(25))
    N = 512000
    X = np.stack([rng.uniform(-5, 5, N), rng.uniform(-10, 10, N)], 1)
    root, X_parts, X_inds = pmk.setuppartition(X, levels, device=True)
    y_parts = [target(x) for x in X_parts]
    n = [len(x) for x in X_parts]
    th = pmk.Spline34KernelType(a)
    ctx = pmk.default_context()
    ctx.enable_timers(True)
    none = np.zeros(0, dtype=np.int64)
    pick = lambda m, npatch: [np.sort(rng.choice(n[r], m, replace=False)) if r < npatch else none for r in range(P)]
    variants = [("1_first_row_of_every_patch", [np.array([0])] * P), ("1_random_row_of_every_patch", pick(1, P)),
                ("1_last_row_of_every_patch", [np.array([k - 1]) for k in n]), ("8_of_every_patch", pick(8, P)),
                ("32_of_every_patch", pick(M.MAX_REMOVE_ROWS, P)), ("8_of_4_patches", pick(8, 4))]
    out = {"tool": "remove_time", "config": "C", "patches": P, "D": 2, "reps": args.reps, "dtype": "f64",
           "n": [int(min(n)), int(max(n))], "variants": {}}
    for name, rows in variants:
        Xr = [np.ascontiguousarray(np.delete(x, r, axis=0)) for x, r in zip(X_parts, rows)]
        yr = [np.delete(y, r) for y, r in zip(y_parts, rows)]
        t = {k: [] for k in STAGES + ["remove_call", "fit", "fresh_fit", "fresh_call"]}
        worst = 0.0
        for _ in range(args.reps + 1):
            model = M.DeviceModel(X_parts, y_parts)
            model.fit(th, sigma2)
            assert np.all(model.info() == 0)
            t["fit"].append(ctx.timer_ms("fit"))
            ctx.synchronize()
            t0 = time.perf_counter()
            info = model.remove(rows)
            ctx.synchronize()
            t["remove_call"].append(1e3 * (time.perf_counter() - t0))
            assert np.all(info == 0)
            for k in STAGES:
                t[k].append(ctx.timer_ms(k))
            c_rem = model.weights()
            del model
            ctx.synchronize()
            t0 = time.perf_counter()
            fresh = M.DeviceModel(Xr, yr)
            fresh.fit(th, sigma2)
            assert np.all(fresh.info() == 0)
            t["fresh_call"].append(1e3 * (time.perf_counter() - t0))
            t["fresh_fit"].append(ctx.timer_ms("fit"))
            c_new = fresh.weights()
            del fresh
            # the two sets of weights agree as two evaluations of one ill-conditioned solve do (sigma2 = 1e-5)
            assert all(np.all(np.isfinite(u)) and np.all(np.isfinite(v)) for u, v in zip(c_rem, c_new))
            worst = max(worst, max(float(np.abs(u - v).max() / np.abs(v).max()) for u, v in zip(c_rem, c_new)))
        r = {k + "_ms": med(v[1:]) for k, v in t.items()}
        r.update({k + "_runs_ms": v[1:] for k, v in t.items()})
        r["remove_stages_ms"] = sum(r[k + "_ms"] for k in STAGES)
        r["fresh_fit_over_remove_stages"] = r["fresh_fit_ms"] / r["remove_stages_ms"]
        r["items"] = int(sum(len(v) for v in rows))
        r["max_rel_weight_difference"] = worst
        out["variants"][name] = r
    txt = json.dumps(out, indent=1, sort_keys=True)
    with open(args.out, "w") as f:
        f.write(txt + "\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()

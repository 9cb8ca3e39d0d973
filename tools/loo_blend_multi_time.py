"""Blended leave-one-out of the multi-output path at config C on the tree route (256 leaves x 2000 points, 2-D
Spline34(1/15), sigma2 = 1e-5, eps-sets of about 2000 points, eps = 1e-3): stage times on HIP events (pmk_ctx_timer_ms),
medians of --reps after one warm-up, all in one process, for R = 1, 4 and 16 - q target columns, trend none and linear,
with and without the variance, of

  plan -> loo_items_multi -> mix_multi   with the 512 000 training points as the queries (pmk_query_items_loo_multi), for
                                         radius = eps (every item is a lookup: nothing runs after the scan of the marks)
                                         and radius = 0.088 > eps (the non-member items go through item_means_kernel and,
                                         with the variance, the strips), each with n_member and n_other
  plan -> items_multi -> mix_multi       pmk_query_items_multi_fitted at the same X and the larger radius: what could be run
                                         before.  It is NOT a leave-one-out (every patch has seen its points); it is the
                                         cost of the same blend with every item on the means kernel and the strips.

"trend_items_ms" is the stage of that name as last recorded: inside loo_items_multi it covers the non-members only.

Writes the JSON to --out (default profiles/loo_blend_multi_time_C.json) and prints it.
Usage: python tools/loo_blend_multi_time.py [--reps 5] [--out FILE]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loo_blend_multi_time_C.json"))
    args = ap.parse_args()
    P, levels, a, sigma2, delta, eps = 256, 9, 1 / 15, 1e-5, 1e-5, 1e-3
    rng = np.random.Generator(np.random.PCG64(25))
    N, D = 512000, 2
    X = np.stack([rng.uniform(-5, 5, N), rng.uniform(-10, 10, N)], 1)
    Yall = np.empty((N, 16), order="F")
    for c in range(16):
        Yall[:, c] = np.sin((1.0 + 0.1 * c) * X[:, 0]) * np.cos(0.5 * X[:, 1]) + 0.05 * c * X[:, 0]
    r_small, r_large = eps, 0.1 * np.sqrt(200.0 / P)
    th = pmk.Spline34KernelType(a)
    ctx = pmk.default_context()
    ctx.enable_timers(True)
    root, _, _ = pmk.setuppartition(X, levels, device=True)
    model = M.DeviceModel.from_tree(root, X, np.ascontiguousarray(Yall[:, 0]), eps=eps)
    model.fit(th, sigma2)
    assert np.all(model.info() == 0)
    model.loo()
    ctx.synchronize()
    out = {"tool": "loo_blend_multi_time", "config": "C", "patches": P, "points": N, "eps": eps, "reps": args.reps,
           "n": [int(model.n.min()), int(model.n.max())], "loo_ms": ctx.timer_ms("loo"), "radius_small": r_small,
           "radius_large": r_large,
           "how": "HIP-event ms per stage, medians of reps after one warm-up, one process", "runs": []}
    q = M.DeviceQuery(model, X)

    def staged(radius, loo, variance, trend):
        wth = pmk.Spline34KernelType(1 / radius)
        stage = "loo_items_multi" if loo else "items_multi"
        t = {"plan": [], stage: [], "mix_multi": []}
        inner = {"trend_items": []} if trend is not None else {}
        for _ in range(args.reps + 1):
            total = q.plan(radius, delta)
            counts = q.items_loo_multi(False, variance) if loo else q.items_multi_fitted(variance)
            q.mix_multi(wth)
            MU, V = q.fetch_multi(model.R)
            for k in t:
                t[k].append(ctx.timer_ms(k))
            for k in inner:
                if not loo or counts[1] > 0:
                    inner[k].append(ctx.timer_ms(k))
        r = {"radius": radius, "items": int(total), "variance": variance,
             "finite": bool(np.all(np.isfinite(MU)) and (V is None or np.all(np.isfinite(V))))}
        if loo:
            r["n_member"], r["n_other"] = int(counts[0]), int(counts[1])
        for k in t:
            r[k + "_ms"] = med(t[k][1:])
        for k in inner:
            if inner[k]:
                r[k + "_ms"] = med(inner[k][1:])
        r["stages_ms"] = sum(r[k + "_ms"] for k in t) + (r.get("trend_items_ms", 0.0) if not loo else 0.0)
        return r

    for trend in (None, "linear"):
        qt = 0 if trend is None else 1 + D
        for R in (1, 4, 16 - qt):
            model.set_targets_multi_global(np.asfortranarray(Yall[:, :R]))
            model.set_trend(trend)
            model.solve_multi()
            assert np.all(model.trend_info() == 0)
            run = {"R": R, "trend": trend or "none", "solve_multi_ms": ctx.timer_ms("solve_multi")}
            for variance in (True, False):
                key = "var" if variance else "mean_only"
                run["loo_radius_le_eps_" + key] = staged(r_small, True, variance, trend)
                assert run["loo_radius_le_eps_" + key]["n_other"] == 0
                run["loo_radius_gt_eps_" + key] = staged(r_large, True, variance, trend)
                assert run["loo_radius_gt_eps_" + key]["n_other"] > 0
                run["predict_multi_fitted_same_X_" + key] = staged(r_large, False, variance, trend)
            out["runs"].append(run)
    text = json.dumps(out, indent=1)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""Blended leave-one-out at config C on the tree route (256 leaves x 2000 points, 2-D Spline34(1/15), sigma2 = 1e-5,
eps-sets of about 2000 points): stage times on HIP events (pmk_ctx_timer_ms), medians of --reps after one warm-up, all in
one process, of

  plan -> loo_items -> mix   with the 512 000 training points as the queries (pmk_query_items_loo), for one radius <= eps
                             (every item is a lookup: no strip kernel, no inner query) and one radius > eps (the
                             non-member items go through the strips), each with n_member and n_strip
  plan -> items -> mix       pmk_query_items_fitted at the same X and the larger radius: what a user would do today with
                             the training points.  It is NOT a leave-one-out (every patch has seen its points); it is the
                             cost of the same blend with every item on the strips.
  wall clock                 of the one-shot calls pmk_predict_mixture_loo and pmk_predict_mixture_fitted (host arrays in
                             and out), and pmk_model_loo once (the pass the lookups read from)

The one timing condition is asserted: after the radius <= eps run, which comes first on a fresh context, no stage "items"
has been recorded.

Writes the JSON to --out (default profiles/loo_blend_time_C.json) and prints it.
Usage: python tools/loo_blend_time.py [--reps 5] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import patchmixturekriging_amd as pmk                      # noqa: E402
from patchmixturekriging_amd import _lib                   # noqa: E402
from patchmixturekriging_amd import mixture as M           # noqa: E402

_dp = C.POINTER(C.c_double)


def med(v):
    return float(np.median(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loo_blend_time_C.json"))
    args = ap.parse_args()
    P, levels, a, sigma2, delta, eps = 256, 9, 1 / 15, 1e-5, 1e-5, 1e-3
    rng = np.random.Generator(np.random.PCG64(25))
    N = 512000
    X = np.stack([rng.uniform(-5, 5, N), rng.uniform(-10, 10, N)], 1)
    y = np.sin(X[:, 0]) * np.cos(0.5 * X[:, 1])
    r_small, r_large = eps, 0.1 * np.sqrt(200.0 / P)
    th = pmk.Spline34KernelType(a)
    ctx = pmk.default_context()
    ctx.enable_timers(True)
    root, _, _ = pmk.setuppartition(X, levels, device=True)
    model = M.DeviceModel.from_tree(root, X, y, eps=eps)
    model.fit(th, sigma2)
    assert np.all(model.info() == 0)
    model.loo()
    ctx.synchronize()
    out = {"tool": "loo_blend_time", "config": "C", "patches": P, "points": N, "eps": eps, "reps": args.reps,
           "n": [int(model.n.min()), int(model.n.max())], "loo_ms": ctx.timer_ms("loo"),
           "how": "HIP-event ms per stage, medians of reps after one warm-up, one process"}
    L = ctx.L
    Y, V = np.empty(N), np.empty(N)

    def staged(radius, loo):
        wth = pmk.Spline34KernelType(1 / radius)
        q = M.DeviceQuery(model, X)
        t = {"plan": [], "loo_items" if loo else "items": [], "mix": []}
        for _ in range(args.reps + 1):
            total = q.plan(radius, delta)
            if loo:
                counts = q.items_loo()
            else:
                q.items_fitted()
            q.mix(wth)
            res = q.fetch()
            for k in t:
                t[k].append(ctx.timer_ms(k))
        r = {"radius": radius, "items": int(total), "finite": bool(np.all(np.isfinite(res[0])) and np.all(np.isfinite(res[1])))}
        if loo:
            r["n_member"], r["n_strip"] = int(counts[0]), int(counts[1])
        for k in t:
            r[k + "_ms"] = med(t[k][1:])
            r[k + "_ms_all"] = t[k][1:]
        r["stages_ms"] = sum(r[k + "_ms"] for k in t)
        return r

    def wall(call, radius):
        wd = pmk.Spline34KernelType(1 / radius).desc()
        ts = []
        for _ in range(args.reps + 1):
            t0 = time.perf_counter()
            _lib.check(call(wd, radius), "one-shot call")
            ts.append(1e3 * (time.perf_counter() - t0))
        return med(ts[1:])

    out["loo_radius_le_eps"] = staged(r_small, True)
    assert out["loo_radius_le_eps"]["n_strip"] == 0
    try:                                                    # no strip kernel has run on this context so far
        ctx.timer_ms("items")
        raise AssertionError("stage 'items' was recorded although n_strip == 0")
    except pmk.PmkError:
        out["items_stage_recorded_with_n_strip_0"] = False
    out["loo_radius_gt_eps"] = staged(r_large, True)
    assert out["loo_radius_gt_eps"]["n_strip"] > 0
    out["predict_fitted_same_X"] = staged(r_large, False)
    out["wall_predict_mixture_loo_ms"] = wall(lambda wd, r: L.pmk_predict_mixture_loo(
        model.h, C.byref(wd), X.ctypes.data_as(_dp), r, delta, 0, Y.ctypes.data_as(_dp), V.ctypes.data_as(_dp)), r_large)
    out["wall_predict_mixture_fitted_ms"] = wall(lambda wd, r: L.pmk_predict_mixture_fitted(
        model.h, C.byref(wd), N, X.ctypes.data_as(_dp), r, delta, Y.ctypes.data_as(_dp), V.ctypes.data_as(_dp)), r_large)
    text = json.dumps(out, indent=1)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""Gradient of the blended mean at config C (256 patches x 2000 points, 2-D Spline34(1/15), sigma2 = 1e-5, 2^20 queries),
R = 1, 4 and 16: what the gradient costs beside the mean-only prediction it differentiates.

Stage times on HIP events (pmk_ctx_timer_ms), the median of --reps runs after one warm-up, all in one process:

  plan         "plan" (the plan kernel records the hyperplane of every item; it does not depend on R)
  items_multi  the mean-only item means (one MFMA per k-step)          items_grad  their gradients (D MFMAs per k-step)
  mix_multi    the blend of the means                                  mix_grad    the gradient of the blend

items_grad evaluates one distance and one psi where items_multi evaluates one distance and one phi, and issues D MFMAs
for its one: between 1 x and (1 + D) x of items_multi is expected.

--plan-only measures the plan alone and uses no symbol of the gradient: copy this file into a checkout of the parent commit
and run it there with --plan-only to take the parent's figure on the same box; --parent-plan folds that JSON into the output.

Writes one JSON object to --out (default profiles/grad_time_C.json) and prints it.
Usage: python tools/grad_time.py [--reps 5] [--nq 1048576] [--plan-only] [--parent-plan parent.json] [--out FILE]
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
    ap.add_argument("--plan-only", action="store_true")
    ap.add_argument("--parent-plan", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_time_C.json"))
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
    model.set_bsp(root, 0)
    out = {"tool": "grad_time", "config": "C", "patches": P, "D": 2, "queries": args.nq, "reps": args.reps,
           "n": [int(min(len(x) for x in X_parts)), int(max(len(x) for x in X_parts))]}
    q = M.DeviceQuery(model, Xq)
    tp = []
    for _ in range(args.reps + 1):
        q.plan(radius, delta)
        ctx.synchronize()
        tp.append(ctx.timer_ms("plan"))
    out["items"] = int(q.total)
    out["plan_ms"] = med(tp[1:])
    out["plan_runs_ms"] = tp[1:]
    if not args.plan_only:
        model.fit(th, sigma2)
        assert np.all(model.info() == 0)
        out["R"] = {}
        for R in (1, 4, 16):
            Ys = [np.stack([v * (1.0 + 0.1 * j) + 0.05 * j for j in range(R)], 1) for v in ys]
            model.set_targets_multi(Ys)
            model.solve_multi()
            t = {k: [] for k in ("items_multi", "items_grad", "mix_multi", "mix_grad")}
            for _ in range(args.reps + 1):
                q.items_multi(th, False)
                q.items_grad(th)
                q.mix_multi(wth)
                q.mix_grad(wth)
                Yq, _ = q.fetch_multi(R)
                dYq = q.fetch_grad()
                for k in t:
                    t[k].append(ctx.timer_ms(k))
            r = {k + "_ms": med(v[1:]) for k, v in t.items()}
            r["items_grad_over_items_multi"] = r["items_grad_ms"] / r["items_multi_ms"]
            r["mix_grad_over_mix_multi"] = r["mix_grad_ms"] / r["mix_multi_ms"]
            r["finite"] = bool(np.all(np.isfinite(Yq)) and np.all(np.isfinite(dYq)))
            out["R"][str(R)] = r
    if args.parent_plan:
        parent = json.load(open(args.parent_plan))
        out["parent_plan_ms"] = parent["plan_ms"]
        out["parent_plan_runs_ms"] = parent.get("plan_runs_ms")
        out["plan_over_parent"] = out["plan_ms"] / parent["plan_ms"]
    txt = json.dumps(out, indent=1, sort_keys=True)
    with open(args.out, "w") as f:
        f.write(txt + "\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()

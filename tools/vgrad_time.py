"""Gradient of the blended variance at config C (256 patches x 2000 points, 2-D Spline34(1/15), sigma2 = 1e-5, 2^20
queries), R = 1 and 4: what the variance gradient costs beside the prediction with variance it differentiates, and beside
the 2 D finite-difference predict passes it replaces.

Stage times on HIP events (pmk_ctx_timer_ms), the median of --reps runs after one warm-up, all in one process:

  plan         "plan"
  items_multi  the item means and, with the variance, the prediction strip sweep (one right-hand side per item)
  items_grad   the gradients of the item means              items_vgrad  the strip sweep with D + 1 right-hand sides per item
  mix_multi    the blend of means and variance              mix_grad, mix_vgrad  the gradients of the blend

items_vgrad carries D + 1 columns per item through the sweep that items_multi carries one through: about (D + 1) x of it
is expected.  fd_passes_ms is 2 D x (plan + items_multi + mix_multi): the central differences of Vq that a caller runs
without this stage, each a full predict pass with the variance.

--items-only measures plan and items_multi with the variance alone and uses no symbol of the variance gradient: copy this
file into a checkout of the parent commit and run it there with --items-only to take the parent's figures on the same
box; --parent folds that JSON into the output.

Writes one JSON object to --out (default profiles/vgrad_time_C.json) and prints it.
Usage: python tools/vgrad_time.py [--reps 5] [--nq 1048576] [--items-only] [--parent parent.json] [--out FILE]
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
    ap.add_argument("--items-only", action="store_true")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vgrad_time_C.json"))
    args = ap.parse_args()
    P, levels, a, sigma2, delta, D = 256, 9, 1 / 15, 1e-5, 1e-5, 2
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
    model.fit(th, sigma2)
    assert np.all(model.info() == 0)
    out = {"tool": "vgrad_time", "config": "C", "patches": P, "D": D, "queries": args.nq, "reps": args.reps,
           "n": [int(min(len(x) for x in X_parts)), int(max(len(x) for x in X_parts))], "R": {}}
    q = M.DeviceQuery(model, Xq)
    stages = ["plan", "items_multi", "mix_multi"] + ([] if args.items_only else ["items_grad", "items_vgrad", "mix_grad", "mix_vgrad"])
    for R in (1, 4):
        Ys = [np.stack([v * (1.0 + 0.1 * j) + 0.05 * j for j in range(R)], 1) for v in ys]
        model.set_targets_multi(Ys)
        model.solve_multi()
        t = {k: [] for k in stages}
        for _ in range(args.reps + 1):
            q.plan(radius, delta)
            q.items_multi(th, True)
            if not args.items_only:
                q.items_grad(th)
                q.items_vgrad(th)
            q.mix_multi(wth)
            if not args.items_only:
                q.mix_grad(wth)
                q.mix_vgrad(wth)
            Yq, Vq = q.fetch_multi(R)
            finite = bool(np.all(np.isfinite(Yq)) and np.all(np.isfinite(Vq)))
            if not args.items_only:
                finite = finite and bool(np.all(np.isfinite(q.fetch_vgrad())))
            for k in t:
                t[k].append(ctx.timer_ms(k))
        r = {k + "_ms": med(v[1:]) for k, v in t.items()}
        r["items_multi_runs_ms"] = t["items_multi"][1:]
        r["finite"] = finite
        if not args.items_only:
            r["items_vgrad_over_items_multi"] = r["items_vgrad_ms"] / r["items_multi_ms"]
            r["fd_passes_ms"] = 2 * D * (r["plan_ms"] + r["items_multi_ms"] + r["mix_multi_ms"])
            r["fd_passes_over_vgrad"] = r["fd_passes_ms"] / (r["items_vgrad_ms"] + r["mix_vgrad_ms"])
        out["R"][str(R)] = r
    out["items"] = int(q.total)
    if args.parent:
        parent = json.load(open(args.parent))
        for R in out["R"]:
            p = parent["R"][R]
            out["R"][R]["parent_items_multi_ms"] = p["items_multi_ms"]
            out["R"][R]["parent_items_multi_runs_ms"] = p.get("items_multi_runs_ms")
            out["R"][R]["items_multi_over_parent"] = out["R"][R]["items_multi_ms"] / p["items_multi_ms"]
    txt = json.dumps(out, indent=1, sort_keys=True)
    with open(args.out, "w") as f:
        f.write(txt + "\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()

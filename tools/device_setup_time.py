"""Set-up between the tree and the model at config C (256 patches x ~2000 points, 2-D Spline34(1/15), sigma2 = 1e-5, fp64):
the host route (lists of per-patch arrays) against the tree route (one global array, assigned, gathered and packed on
the GPU).  Wall-clock ms (time.perf_counter around calls that end synchronised), median of --reps after one warm-up, all
in one process on one box:

  (a) host route: organizetrainingsets(device=True) + MixtureGPType + fitmixtureGP_
  (b) MixtureGPType.from_tree + fitmixtureGP_, X and y numpy arrays
  (c) the same with torch tensors on the device
  (d) a refit on new targets only: host fitmixtureGP_ (a new model per call) against set_targets_global + fit on the
      resident model with a device y (info() ends both)
  (e) prediction of --nq queries on a fitted model: host Xq + fetch() against device Xq + fetch_into()
  (f) pmk_ctx_timer_ms("fit") of the plain fit on the tree-built model (HIP events), to set beside other commits

The weights of (b) and (c) are compared with those of (a) bit for bit, and the predictions of both forms of (e).
Writes the JSON to --out (default profiles/device_setup_time_C.json) and prints it.
Usage: python tools/device_setup_time.py [--reps 10] [--nq 1048576] [--out FILE]
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


def timed(fn, reps):
    """ms of every call after one warm-up -> (median, all)"""
    ms = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ms[1:])), ms[1:]


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--nq", type=int, default=1 << 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_setup_time_C.json"))
    args = ap.parse_args()
    P, levels, a, sigma2, delta, eps = 256, 9, 1 / 15, 1e-5, 1e-5, 1e-3
    rng = np.random.Generator(np.random.PCG64(25))
    N = 512000
    X = np.stack([rng.uniform(-5, 5, N), rng.uniform(-10, 10, N)], 1)
    Xq = np.stack([rng.uniform(-5, 5, args.nq), rng.uniform(-10, 10, args.nq)], 1)
    y = np.sin(X[:, 0]) * np.cos(0.5 * X[:, 1])
    y2 = np.cos(X[:, 0]) * np.sin(0.5 * X[:, 1])
    radius = 0.1 * np.sqrt(200.0 / P)
    th, wth = pmk.Spline34KernelType(a), pmk.Spline34KernelType(1 / radius)
    ctx = pmk.default_context()
    ctx.enable_timers(True)
    root, _, _ = pmk.setuppartition(X, levels, device=True)
    hps = pmk.fetchhyperplanes(root)
    Xd, yd, y2d, Xqd = (torch.from_numpy(v).cuda() for v in (X, y, y2, Xq))
    torch.cuda.synchronize()
    keep = {}

    def host_route():
        X_set, inds, _, _ = pmk.organizetrainingsets(root, levels, X, eps, device=True)
        eta = pmk.MixtureGPType(X_set, hps)
        pmk.fitmixtureGP_(eta, [y[i] for i in inds], th, sigma2)
        keep["host"], keep["inds"] = eta, inds

    def tree_route(Xa, ya, name):
        def run():
            eta = pmk.MixtureGPType.from_tree(root, Xa, eps=eps, hps=hps)
            pmk.fitmixtureGP_(eta, ya, th, sigma2)
            keep[name] = eta
        return run

    out = {"tool": "device_setup_time", "config": "C", "patches": P, "reps": args.reps, "eps": eps, "queries": args.nq,
           "how": "wall-clock ms, median of reps after one warm-up, one process"}
    out["a_host_route_ms"], out["a_all"] = timed(host_route, args.reps)
    out["b_from_tree_host_arrays_ms"], out["b_all"] = timed(tree_route(X, y, "b"), args.reps)
    out["c_from_tree_device_tensors_ms"], out["c_all"] = timed(tree_route(Xd, yd, "c"), args.reps)
    sizes = [len(i) for i in keep["inds"]]
    out["n"] = [int(min(sizes)), int(max(sizes))]
    for k in ("b", "c"):
        out["%s_weights_bit_identical_to_a" % k] = bool(all(
            np.array_equal(u.view(np.uint64), v.view(np.uint64)) for u, v in zip(keep["host"].c_set, keep[k].c_set)))
    out["b_over_a"] = out["b_from_tree_host_arrays_ms"] / out["a_host_route_ms"]
    out["c_over_a"] = out["c_from_tree_device_tensors_ms"] / out["a_host_route_ms"]

    # (d) new targets only
    eta_h, inds, model = keep["host"], keep["inds"], keep["c"]._model

    def refit_host():
        pmk.fitmixtureGP_(eta_h, [y2[i] for i in inds], th, sigma2)

    def refit_tree():
        model.set_targets_global(y2d)
        model.fit(th, sigma2)
        assert np.all(model.info() == 0)

    out["d_refit_host_ms"], out["d_host_all"] = timed(refit_host, args.reps)
    out["d_refit_global_ms"], out["d_global_all"] = timed(refit_tree, args.reps)
    out["d_weights_bit_identical"] = bool(all(np.array_equal(u.view(np.uint64), v.view(np.uint64))
                                               for u, v in zip(eta_h.c_set, model.weights())))
    out["d_global_over_host"] = out["d_refit_global_ms"] / out["d_refit_host_ms"]

    # (e) prediction in and out
    res = {}
    Yd, Vd = (torch.empty(args.nq, dtype=torch.float64, device="cuda") for _ in range(2))

    def predict(Xq_in, into):
        def run():
            q = pmk.DeviceQuery(model, Xq_in)
            q.plan(radius, delta)
            q.items(th)
            q.mix(wth)
            if into:
                q.fetch_into(Yd, Vd)
                ctx.synchronize()
            else:
                res["host"] = q.fetch()
        return run

    out["e_predict_host_in_out_ms"], out["e_host_all"] = timed(predict(Xq, False), args.reps)
    out["e_predict_device_in_out_ms"], out["e_device_all"] = timed(predict(Xqd, True), args.reps)
    out["e_bit_identical"] = bool(np.array_equal(Yd.cpu().numpy().view(np.uint64), res["host"][0].view(np.uint64)) and
                                  np.array_equal(Vd.cpu().numpy().view(np.uint64), res["host"][1].view(np.uint64)))
    out["e_device_over_host"] = out["e_predict_device_in_out_ms"] / out["e_predict_host_in_out_ms"]

    # (f) the fit itself, on HIP events
    fit = []
    for _ in range(args.reps + 1):
        model.fit(th, sigma2)
        assert np.all(model.info() == 0)
        fit.append(ctx.timer_ms("fit"))
    out["f_fit_ms"], out["f_all"] = float(np.median(fit[1:])), fit[1:]
    out["fit_shader_clock_ghz"] = ctx.shader_clock(0)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""Leave-one-out and evidence scores at config C (256 patches x 2000 points, 2-D Spline34(1/15), sigma2 = 1e-5): stage times
on HIP events (pmk_ctx_timer_ms), median of --reps after one warm-up, of

  - the fit (kernel matrix + Cholesky + solve),
  - pmk_model_loo (d = diag((L L^T)^-1) of every patch from the resident factor) with the flop count the kernel executes
    (from the shapes: pmk_loo.hip) and the rate that gives,
  - pmk_model_evidence (log det and y^T c),

and, for context, the host route on 3 patches: pmk_model_get(PMK_GET_L) + LAPACK dpotri, wall time.  The shader clock is
the one the factorisation's step launches of the same run saw (pmk_ctx_shader_clock).

Prints one JSON line.  Usage: python tools/loo_time.py [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.linalg as sla

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import patchmixturekriging_amd as pmk                      # noqa: E402
from patchmixturekriging_amd import mixture as M           # noqa: E402


def loo_flop(n):
    """executed by loo_strip_kernel on a patch of n points: the two halves of strip s run m = nt - 2 s - h block rows with
    K = 128 k, k < m, so m runs over 1 .. nt; a substitution is counted as 128^2 flop per column"""
    nt = (n + 127) // 128
    gemm = sum(2 * 128 * 128 * 128 * k for m in range(1, nt + 1) for k in range(m))
    return gemm, nt * (nt + 1) // 2 * 128 * 128 * 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    P, levels, a, sigma2 = 256, 9, 1 / 15, 1e-5
    rng = np.random.Generator(np.random.PCG64(25))
    N = 512000
    X = np.stack([rng.uniform(-5, 5, N), rng.uniform(-10, 10, N)], 1)
    y = np.sin(X[:, 0]) * np.cos(0.5 * X[:, 1])
    root, X_parts, X_inds = pmk.setuppartition(X, levels, device=True)
    th = pmk.Spline34KernelType(a)
    ctx = pmk.default_context()
    ctx.enable_timers(True)
    model = M.DeviceModel(X_parts, [y[i] for i in X_inds])

    def med(v):
        return float(np.median(v))

    fit, loo, ev = [], [], []
    for _ in range(args.reps + 1):
        model.fit(th, sigma2)
        assert np.all(model.info() == 0)
        fit.append(ctx.timer_ms("fit"))
        model.loo()
        res, var = model.loo_values()
        loo.append(ctx.timer_ms("loo"))
        logdet, quad = model.evidence()
        ev.append(ctx.timer_ms("evidence"))
    clock = ctx.shader_clock(0)
    gemm, subst = (sum(v) for v in zip(*[loo_flop(len(x)) for x in X_parts]))
    loo_ms = med(loo[1:])
    out = {"tool": "loo_time", "config": "C", "patches": P, "n": [int(min(len(x) for x in X_parts)), int(max(len(x) for x in X_parts))],
           "fit_ms": med(fit[1:]), "loo_ms": loo_ms, "loo_ms_all": loo[1:], "evidence_ms": med(ev[1:]),
           "loo_over_fit": loo_ms / med(fit[1:]),
           "loo_flop_gemm": gemm, "loo_flop_substitution": subst, "loo_flop": gemm + subst,
           "loo_flop_over_n3_3": (gemm + subst) / sum(len(x) ** 3 / 3 for x in X_parts),
           "loo_tflops": (gemm + subst) / (loo_ms * 1e-3) / 1e12, "fit_shader_clock_ghz": clock,
           "finite": bool(np.all(np.isfinite(np.stack(var))) and np.all(np.isfinite(logdet)) and np.all(np.isfinite(quad)))}
    # the host route: pull L (32 MB per patch), LAPACK dpotri, take the diagonal
    t0 = time.perf_counter()
    worst = 0.0
    for r in (0, 101, 255):
        Lr = model.get(r, M.GET_L)
        inv, info = sla.lapack.dpotri(Lr, lower=1)
        assert info == 0
        worst = max(worst, float(np.abs(1.0 / var[r] - np.diag(inv)).max() / np.diag(inv).max()))
    host_s = time.perf_counter() - t0
    out["host_route_3_patches_ms"] = 1e3 * host_s
    out["host_route_256_patches_ms_extrapolated"] = 1e3 * host_s * P / 3
    out["d_vs_dpotri_max_rel"] = worst
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generate the conditioning-ladder fixtures conditioning_p1.npz / conditioning_p2.npz under tests/golden/.

Per patch fit + predict of src/RKHS/mixtureGP.jl:92-115,296-316 restated in numpy.longdouble (x87 extended, 64-bit
mantissa): a plain column Cholesky and plain substitutions, nothing blocked, nothing inverted.  The kernel matrix K and
the cross kernel K_q come from the C oracle (<= 4 ulp of the device's by tests/test_gpu_parity.py) and are widened to
long double, so the fixtures are the exact-to-19-digits answer for the matrix every fp64 solver under test sees.

Two problems, each with a ladder of noise levels sigma2 (the conditioning of U = K + sigma2 I grows as sigma2 falls):

  problem 1: D = 2, n = 640,  X uniform in [-4, 4]^2, y = sin(x0) cos(x1 / 2), Spline34 theta = 1/40
  problem 2: D = 3, n = 1111, X uniform in [0, 1]^3,  y = (sum x)^2,           Spline34 theta = 0.1

  fp64 rungs sigma2 = 1e-4, 1e-6, 1e-8, 1e-10;   fp32 rungs sigma2 = 1e-1, 1e-2, 1e-3

60 queries per problem: 40 uniform, 10 training points shifted by 1e-3 in every coordinate, 10 exact training points
(the predictive variance 1 - ||L^-1 k_q||^2 cancels fully there).  Stored per rung: the weights c, the predictive mean
mu and variance var (unclamped) rounded to double, and cond_2(U); on the hardest fp64 rung also the weights c2 of a
second smooth target y2.  Xc, yc: a 257-point companion patch from the same distribution (no reference values; it makes
the device's batch ragged).

Run:  python tests/golden/make_conditioning.py   (deterministic: fixed PCG64 seeds, fixed zip time stamps; the output
is reproduced bit for bit)
"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import oracle as O  # noqa: E402

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "numpy.longdouble is not the x87 extended type here"

RUNGS_F64 = [1e-4, 1e-6, 1e-8, 1e-10]
RUNGS_F32 = [1e-1, 1e-2, 1e-3]

PROBLEMS = {
    "p1": dict(D=2, n=640, lo=-4.0, hi=4.0, theta=1 / 40.0, seed=9101,
               f=lambda X: np.sin(X[:, 0]) * np.cos(0.5 * X[:, 1]),
               f2=lambda X: np.cos(0.5 * X[:, 0]) + 0.1 * X[:, 1]),
    "p2": dict(D=3, n=1111, lo=0.0, hi=1.0, theta=0.1, seed=9102,
               f=lambda X: X.sum(1) ** 2,
               f2=lambda X: np.sin(3 * X[:, 0]) + X[:, 2] ** 2),
}


def cholesky_ld(U):
    """plain left-looking column Cholesky in long double; raises if a pivot is not positive"""
    n = U.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        col = U[j:, j] - L[j:, :j] @ L[j, :j]
        assert col[0] > 0, "pivot %d is not positive" % j
        d = np.sqrt(col[0])
        L[j, j] = d
        L[j + 1:, j] = col[1:] / d
    return L


def forward_ld(L, B):
    """L^-1 B, row by row"""
    Z = np.array(B, dtype=LD, copy=True)
    for i in range(L.shape[0]):
        Z[i] = (Z[i] - L[i, :i] @ Z[:i]) / L[i, i]
    return Z


def backward_ld(L, B):
    """L^-T B, row by row from the last"""
    n = L.shape[0]
    Z = np.array(B, dtype=LD, copy=True)
    for i in range(n - 1, -1, -1):
        Z[i] = (Z[i] - L[i + 1:, i] @ Z[i + 1:]) / L[i, i]
    return Z


def solve_rung(K, Kq, Y, sigma2):
    """(C = U^-1 Y, mu = Kq^T C[:, 0], var = 1 - ||L^-1 Kq||^2 per query, cond_2(U)), everything but cond in long double"""
    n = K.shape[0]
    U = K.astype(LD)
    U[np.diag_indices(n)] += LD(sigma2)
    L = cholesky_ld(U)
    Cw = backward_ld(L, forward_ld(L, Y.astype(LD)))
    V = forward_ld(L, Kq.astype(LD))
    mu = Kq.astype(LD).T @ Cw[:, 0]
    var = LD(1) - (V * V).sum(0)                     # Spline34: k(x, x) = 1
    ev = np.linalg.eigvalsh(K + sigma2 * np.eye(n))
    return Cw, mu, var, ev[-1] / ev[0]


def save_npz(path, **arrays):
    """np.savez with fixed member time stamps: the file is a function of the arrays alone"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(a), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())


def make(name):
    p = PROBLEMS[name]
    rng = np.random.Generator(np.random.PCG64(p["seed"]))
    D, n = p["D"], p["n"]
    X = rng.uniform(p["lo"], p["hi"], (n, D))
    Xc = rng.uniform(p["lo"], p["hi"], (257, D))
    Xu = rng.uniform(p["lo"], p["hi"], (40, D))
    pick = rng.permutation(n)[:20]
    Xq = np.concatenate([Xu, X[pick[:10]] + 1e-3, X[pick[10:]]])
    y, y2, yc = p["f"](X), p["f2"](X), p["f"](Xc)
    th = O.kernel(O.SPLINE34, p["theta"])
    K = O.kernel_matrix(th, X)
    Kq = O.cross_kernel_matrix(th, X, Xq)
    out = dict(X=X, y=y, y2=y2, Xq=Xq, Xc=Xc, yc=yc, theta=np.float64(p["theta"]),
               sigma2_f64=np.array(RUNGS_F64), sigma2_f32=np.array(RUNGS_F32))
    for tag, rungs in (("f64", RUNGS_F64), ("f32", RUNGS_F32)):
        cs, mus, vs, conds = [], [], [], []
        for s2 in rungs:
            Cw, mu, var, cond = solve_rung(K, Kq, np.stack([y, y2], 1), s2)
            cs.append(Cw[:, 0].astype(np.float64))
            mus.append(mu.astype(np.float64))
            vs.append(var.astype(np.float64))
            conds.append(cond)
            if tag == "f64" and s2 == RUNGS_F64[-1]:
                out["c2_hard"] = Cw[:, 1].astype(np.float64)
            print("%s %s sigma2 %.0e: cond2 %.3g, min var %.3g, max |c| %.3g" % (name, tag, s2, cond, float(var.min()),
                                                                              float(np.abs(Cw[:, 0]).max())), flush=True)
        out["c_" + tag], out["mu_" + tag], out["var_" + tag] = np.array(cs), np.array(mus), np.array(vs)
        out["cond_" + tag] = np.array(conds)
    save_npz(os.path.join(HERE, "conditioning_%s.npz" % name), **out)


if __name__ == "__main__":
    for name in (sys.argv[1:] or sorted(PROBLEMS)):
        make(name)

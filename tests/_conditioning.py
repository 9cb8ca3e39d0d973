"""Shared by tests/test_oracle_conditioning.py (CPU) and tests/test_gpu_breakdown.py (GPU): the conditioning-ladder
fixtures, the error measures, and the two emulated reference solvers (program text of this project: numpy + LAPACK)."""
import os

import numpy as np
import scipy.linalg as sla
from scipy.linalg import lapack

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U64, U32 = 2.0 ** -53, 2.0 ** -24
# fp32 bounds on the factor's backward error and on the residual of the weights: the project's fp64 bounds (DESIGN
# section 2) in units of roundoff, 1e-14 = 90 u and 1e-13 = 900 u, carried to fp32
BWD_F32 = 1e-14 / U64 * U32
RES_F32 = 1e-13 / U64 * U32


def load(name):
    return np.load(os.path.join(GOLDEN, "conditioning_%s.npz" % name))


def backward_error(L, U):
    return np.linalg.norm(L @ L.T - U) / np.linalg.norm(U)


def residual(U, c, y):
    return np.linalg.norm(U @ c - y) / (np.linalg.norm(U) * np.linalg.norm(c) + np.linalg.norm(y))


def block_inverse_emulation(U, y, dt):
    """LAPACK's factor, then substitutions that MULTIPLY by explicitly inverted 32 x 32 diagonal blocks (the device's
    construction, in numpy, on the same U): a reference for what that construction costs, not the device"""
    n = len(y)
    L = sla.cholesky(U.astype(dt), lower=True, check_finite=False)
    inv = [sla.solve_triangular(L[b:b + 32, b:b + 32], np.eye(min(32, n - b), dtype=dt), lower=True, check_finite=False)
           for b in range(0, n, 32)]
    z = np.array(y, dtype=dt)
    for i, b in enumerate(range(0, n, 32)):
        z[b:b + 32] = inv[i] @ (z[b:b + 32] - L[b:b + 32, :b] @ z[:b])
    c = z.copy()
    for i, b in reversed(list(enumerate(range(0, n, 32)))):
        c[b:b + 32] = inv[i].T @ (c[b:b + 32] - L[b + 32:, b:b + 32].T @ c[b + 32:])
    return L.astype(np.float64), c.astype(np.float64)


def fp32_pipeline(U, y, Kq):
    """a plain fp32 solver: fp32-rounded U, LAPACK spotrf, fp32 substitutions, fp32 Kq^T c and 1 - ||V||^2
    -> info, L, c, mu, var (widened to double)"""
    f = np.float32
    L, info = lapack.spotrf(U.astype(f), lower=1, clean=1)
    z = sla.solve_triangular(L, y.astype(f), lower=True, check_finite=False)
    c = sla.solve_triangular(L, z, lower=True, trans="T", check_finite=False)
    V = sla.solve_triangular(L, Kq.astype(f), lower=True, check_finite=False)
    mu = Kq.astype(f).T @ c
    var = f(1) - (V * V).sum(0, dtype=f)
    assert L.dtype == f and c.dtype == f and mu.dtype == f and var.dtype == f
    return int(info), L.astype(np.float64), c.astype(np.float64), mu.astype(np.float64), var.astype(np.float64)

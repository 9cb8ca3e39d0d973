"""Long-double references for the model-selection scores (tests/test_model_selection_abi.py,
tests/test_gpu_model_selection.py, tests/test_gpu_loo_schedule.py): leave-one-out residuals and variances in closed form (Rasmussen & Williams, Gaussian
Processes for Machine Learning, eq. 5.10-5.12) and the two terms of the log marginal likelihood (eq. 5.8).

numpy.longdouble (x87 extended, 64-bit mantissa), a plain column Cholesky and plain row substitutions -- nothing blocked,
nothing inverted -- in the manner of tests/golden/make_conditioning.py, whose routines are used here.  The kernel matrix
comes from the CPU oracle and is widened, so the references are exact to ~19 digits for the matrix the device sees.

    U = K + sigma2 I = L L^T,   d = diag(U^-1) = squared column norms of L^-1,   c = U^-1 y
    res_i = y_i - mu_-i = c_i / d_i,    var_i = 1 / d_i  (variance of y_i given the others, noise included)
    logdet = 2 sum log L_ii,            quad = y^T c
"""
import os
import sys

import numpy as np

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
if _GOLDEN not in sys.path:
    sys.path.insert(0, _GOLDEN)

from make_conditioning import LD, backward_ld, cholesky_ld, forward_ld  # noqa: E402

U64 = 2.0 ** -53          # unit roundoff of fp64 models
U32 = 2.0 ** -24          # unit roundoff of fp32 models


def unit_roundoff(dtype):
    return {"f64": U64, "f32": U32}[dtype]


def linv_colnorms_ld(L):
    """squared column norms of L^-1 in long double, L lower triangular (any float type): row i of Z = L^-1 by forward
    substitution on the identity, only its nonzero part Z[i, :i + 1]"""
    L = np.asarray(L, dtype=LD)
    n = L.shape[0]
    Z = np.zeros((n, n), dtype=LD)
    for i in range(n):
        row = -(L[i, :i] @ Z[:i, :i + 1])
        row[i] += LD(1)
        Z[i, :i + 1] = row / L[i, i]
    return (Z * Z).sum(0)


def loo_reference(K, sigma2, Y):
    """dict(d, C, res, var, logdet, quad, L) in long double for U = K + sigma2 I and the target columns Y (n or n x R)"""
    K = np.asarray(K)
    n = K.shape[0]
    Y = np.asarray(Y, dtype=LD)
    vec = Y.ndim == 1
    if vec:
        Y = Y[:, None]
    U = K.astype(LD)
    U[np.diag_indices(n)] += LD(sigma2)
    L = cholesky_ld(U)
    d = linv_colnorms_ld(L)
    C = backward_ld(L, forward_ld(L, Y))
    res = C / d[:, None]
    out = dict(d=d, C=C, res=res, var=LD(1) / d, logdet=LD(2) * np.log(np.diag(L)).sum(), quad=(Y * C).sum(0), L=L)
    if vec:
        out["C"], out["res"], out["quad"] = C[:, 0], res[:, 0], out["quad"][0]
    return out


def trtri_colnorms(L):
    """squared column norms of L^-1 in double by LAPACK dtrtri, where long double would take too long"""
    import scipy.linalg as sla
    Li, info = sla.lapack.dtrtri(np.asfortranarray(L), lower=1)
    assert info == 0
    return (Li * Li).sum(0)


def sum_ld(terms):
    """(sum, sum of magnitudes) of the terms in long double"""
    t = np.asarray(terms, dtype=LD)
    return t.sum(), np.abs(t).sum()


def summation_error_and_bound(n, got, terms):
    """|got - sum terms| <= 2 (n + 4) 2^-53 sum |terms|: worst-case recursive summation plus two roundoffs per term (the
    device accumulates in double in both precisions)"""
    s, mag = sum_ld(terms)
    bound = 2 * (n + 4) * U64 * float(mag)
    err = abs(float(LD(got) - s))
    return err, bound

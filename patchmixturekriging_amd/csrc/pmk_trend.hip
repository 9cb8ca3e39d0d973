// Kriging with a trend (ordinary / universal kriging) on the multi-output path: one generalised-least-squares drift per
// patch, computed from the resident factor through the multi-output solve.
//
// With H the n x q basis of a patch (q = 1: h = [1]; q = 1 + D: h(x) = [1, x_1 .. x_D] in the RAW coordinates the model
// stores) and U = K + sigma2 I = L L^T:
//
//   [C_Y | C_H] = U^-1 [Y | H]                one multi_solve_kernel launch over R + q <= 16 columns (pmk_multi.hip)
//   G = H^T C_H (q x q), B = H^T C_Y,  G = L_G L_G^T,  beta = G^-1 B,  C <- C_Y - C_H beta        (trend_gls_kernel)
//   query x*:  a = kq^T C_H,  mu_j = kq^T C[:, j] + h(x*)^T beta_j,  rho = h(x*) - a,  v = v_sk + |L_G^-1 rho|^2
//   leave-one-out:  Q_ii = d_i - |L_G^-1 C_H[i, :]^T|^2,  res_ij = C_ij / Q_ii,  var_i = 1 / Q_ii
//
//   trend_fill_kernel        H into columns R .. R + q - 1 of the row-major x 16 target block (pmk_multi.hip), zero in
//                            columns >= R + q and in the padding rows: q = 0 restores "columns >= R are zero"
//   trend_gls_kernel         one workgroup per patch: the q x (R + q) products H^T [C_Y | C_H] (of G only the lower
//                            triangle is used), the Cholesky of G, beta, and the update of C
//   trend_loo_values_kernel  the trend-aware leave-one-out values, next to loo_values_kernel (pmk_loo.hip)
//   trend_items_kernel       per (query, region) item: mu += h^T beta, v += |L_G^-1 rho|^2 (double only)
//
// Per-patch trend state on the device, always double, TQ_MAX = 5 = 1 + MAX_D:
//   beta[(r * 16 + j) * 5 + a]   coefficient a of column j      G, L_G [r * 25 + a + 5 b]   column-major 5 x 5
// Status per patch (tinfo): 0 ok; a in 1..q: pivot a of the Cholesky of G is <= 0 or NaN; n + 1: the patch has n < q
// points (nothing is computed).  A flagged patch, and a patch whose factorisation failed (info != 0, tinfo stays 0), gets
// NaN in beta, L_G and the R weight columns of its rows i < n; the padding rows stay zero (the items kernel multiplies
// them by masked zeros, and 0 * NaN is NaN).  A nearly singular G is not flagged: G is kept for the caller to judge.
//
// Every sum over the n rows is taken in double in both precisions with a fixed reduction tree (as evidence_kernel), the
// small solves run in double in a fixed order, and C is rounded once to the element type.
#include "pmk_items.h"
#include "pmk_real.h"

namespace pmk {

// TQ_MAX and TR_RP: pmk_internal.h
constexpr int TR_BETA = TQ_MAX * TR_RP;       // doubles of beta per patch
constexpr int TR_G = TQ_MAX * TQ_MAX;         // doubles of G and of L_G per patch

namespace PMK_NS {

constexpr int TF_THREADS = 256;

// grid: chunks x P workgroups, flattened; chunk c of patch r covers the slab rows [256 c, 256 c + 256)
__global__ __launch_bounds__(TF_THREADS) void trend_fill_kernel(const PatchDesc *__restrict__ descs, const real *__restrict__ x,
                                                                int chunks, int R, int q, real *__restrict__ Y)
{
    const int r = (int)(blockIdx.x / (unsigned)chunks);
    const PatchDesc pd = descs[r];
    const int i = (int)(blockIdx.x % (unsigned)chunks) * TF_THREADS + (int)threadIdx.x;
    if (i >= pd.ld) return;
    real *row = Y + (pd.yoff + i) * TR_RP;
    const real *xs = x + pd.xoff + i;
    const bool live = i < pd.n;                  // the padding coordinates are huge on purpose: never copy them
    for (int j = R; j < TR_RP; ++j) {
        const int a = j - R;
        real v = (real)0;
        if (live && a < q) v = a == 0 ? (real)1 : xs[(int64_t)(a - 1) * pd.ld];
        row[j] = v;
    }
}

int launch_trend_fill(const pmk_model *m, int R, int q, hipStream_t s)
{
    const int chunks = (m->max_nt * TILE + TF_THREADS - 1) / TF_THREADS;
    hipLaunchKernelGGL(trend_fill_kernel, dim3((unsigned)(m->P * chunks)), dim3(TF_THREADS), 0, s, m->d_desc,
                       (const real *)m->d_x, chunks, R, q, (real *)m->d_ym);
    PMK_HIP(hipGetLastError());
    return 0;
}

// One workgroup per patch.  Thread t sums column t % 16 of [C_Y | C_H] against the q columns of H over the rows
// t / 16, t / 16 + 16, ..; the tree then adds t and t + st (the same column) for st = 128 .. 16, as evidence_kernel does.
constexpr int TG_THREADS = 256;

__global__ __launch_bounds__(TG_THREADS) void trend_gls_kernel(const PatchDesc *__restrict__ descs, const int32_t *__restrict__ info,
                                                               const real *__restrict__ Y, real *Cm, int R, int q,
                                                               double *__restrict__ beta, double *__restrict__ Lg,
                                                               double *__restrict__ G, int32_t *__restrict__ tinfo)
{
    const int r = blockIdx.x, tid = threadIdx.x;
    const PatchDesc pd = descs[r];
    const bool failed = info[r] != 0;
    const double nan = __builtin_nan("");
    __shared__ double red[TQ_MAX][TG_THREADS];
    __shared__ double sG[TR_G], sL[TR_G], sbeta[TR_BETA];
    __shared__ int sflag;
    const int j = tid % TR_RP;
    const bool few = pd.n < q;                   // workgroup-uniform, as is `failed`
    int flag = few ? pd.n + 1 : 0;
    if (tid < TR_G) sG[tid] = sL[tid] = nan;
    if (tid < TR_BETA) sbeta[tid] = nan;
    __syncthreads();
    if (!failed && !few) {
        double acc[TQ_MAX];
#pragma unroll
        for (int a = 0; a < TQ_MAX; ++a) acc[a] = 0.0;
        for (int i = tid / TR_RP; i < pd.n; i += TG_THREADS / TR_RP) {
            const int64_t row = (pd.yoff + i) * TR_RP;
            const double cj = (double)Cm[row + j];
#pragma unroll
            for (int a = 0; a < TQ_MAX; ++a)
                if (a < q) acc[a] = __builtin_fma((double)Y[row + R + a], cj, acc[a]);
        }
#pragma unroll
        for (int a = 0; a < TQ_MAX; ++a) red[a][tid] = acc[a];
        __syncthreads();
        for (int st = TG_THREADS / 2; st >= TR_RP; st >>= 1) {
            if (tid < st)
#pragma unroll
                for (int a = 0; a < TQ_MAX; ++a) red[a][tid] += red[a][tid + st];
            __syncthreads();
        }
        // red[a][j] = H[:, a]^T [C_Y | C_H][:, j].  G from its lower triangle, then G = L L^T by rows
        if (tid == 0) {
            for (int a = 0; a < q; ++a)
                for (int b = 0; b <= a; ++b) sG[a + TQ_MAX * b] = sG[b + TQ_MAX * a] = red[a][R + b];
            int f = 0;
            for (int a = 0; a < q && !f; ++a)
                for (int b = 0; b <= a; ++b) {
                    double t = sG[a + TQ_MAX * b];
                    for (int k = 0; k < b; ++k) t = __builtin_fma(-sL[a + TQ_MAX * k], sL[b + TQ_MAX * k], t);
                    if (b < a) {
                        sL[a + TQ_MAX * b] = t / sL[b + TQ_MAX * b];
                    } else {
                        if (!(t > 0.0)) { f = a + 1; break; }
                        sL[a + TQ_MAX * a] = sqrt(t);
                    }
                }
            sflag = f;
        }
        __syncthreads();
        flag = sflag;
        // beta[:, j] = L^-T L^-1 B[:, j], B[a][j] = red[a][j]: thread j < R, forward then backward, in index order
        if (!flag && tid < R) {
            double z[TQ_MAX];
            trend_forward(sL, q, [&](int a) { return red[a][tid]; }, z);
            for (int a = q - 1; a >= 0; --a) {
                double t = z[a];
                for (int k = a + 1; k < q; ++k) t = __builtin_fma(-sL[k + TQ_MAX * a], z[k], t);
                z[a] = t / sL[a + TQ_MAX * a];
            }
            for (int a = 0; a < q; ++a) sbeta[a + TQ_MAX * tid] = z[a];
        }
        __syncthreads();
    }
    const bool bad = failed || flag != 0;
    if (tid == 0) tinfo[r] = failed ? 0 : flag;
    if (tid < TR_G) {
        const int a = tid % TQ_MAX, b = tid / TQ_MAX;
        const bool in = a < q && b < q;
        G[(int64_t)r * TR_G + tid] = in ? sG[tid] : 0.0;
        Lg[(int64_t)r * TR_G + tid] = !in ? 0.0 : bad ? nan : (b <= a ? sL[tid] : 0.0);
    }
    if (tid < TR_BETA) {
        const int a = tid % TQ_MAX, jj = tid / TQ_MAX;
        beta[(int64_t)r * TR_BETA + tid] = (a < q && jj < R) ? (bad ? nan : sbeta[tid]) : 0.0;
    }
    // C[:, j] <- C_Y[:, j] - C_H beta[:, j] for j < R in double, rounded once; the columns of C_H are read only
    if (j < R)
        for (int i = tid / TR_RP; i < pd.n; i += TG_THREADS / TR_RP) {
            const int64_t row = (pd.yoff + i) * TR_RP;
            double t = (double)Cm[row + j];
            for (int a = 0; a < q; ++a) t = __builtin_fma(-(double)Cm[row + R + a], sbeta[a + TQ_MAX * j], t);
            Cm[row + j] = bad ? (real)nan : (real)t;
        }
}

int launch_trend_gls(pmk_model *m, int R, int q, hipStream_t s)
{
    hipLaunchKernelGGL(trend_gls_kernel, dim3((unsigned)m->P), dim3(TG_THREADS), 0, s, m->d_desc, m->d_info,
                       (const real *)m->d_ym, (real *)m->d_cm, R, q, m->d_tbeta, m->d_tL, m->d_tG, m->d_tinfo);
    PMK_HIP(hipGetLastError());
    return 0;
}

// loo_values_kernel (pmk_loo.hip) with a trend: one thread per row, Q_ii = d_i - |L_G^-1 C_H[i, :]^T|^2 by forward
// substitution in index order, then res[i][j] = C[i][j] / Q_ii and var[i] = 1 / Q_ii (IEEE division, double)
__global__ __launch_bounds__(256) void trend_loo_values_kernel(const PatchDesc *__restrict__ descs, const int32_t *__restrict__ info,
                                                               const int32_t *__restrict__ tinfo, const double *__restrict__ d,
                                                               const real *__restrict__ Cw, const double *__restrict__ Lg, int R,
                                                               int q, double *__restrict__ res, double *__restrict__ var)
{
    const int r = blockIdx.x;
    const PatchDesc pd = descs[r];
    const bool bad = patch_is_bad_loo(info, tinfo, r, q, pd.n);
    const double nan = __builtin_nan("");
    const double *L = Lg + (int64_t)r * TR_G;
    for (int i = threadIdx.x; i < pd.n; i += 256) {
        const int64_t row = (pd.yoff + i) * TR_RP;
        const double Q = d[pd.yoff + i] - trend_leverage(L, q, [&](int a) { return (double)Cw[row + R + a]; });
        if (res)
            for (int jj = 0; jj < R; ++jj) res[row + jj] = bad ? nan : (double)Cw[row + jj] / Q;
        if (var) var[pd.yoff + i] = bad ? nan : 1.0 / Q;
    }
}

int launch_trend_loo_values(const pmk_model *m, int R, int q, double *d_res, double *d_var, hipStream_t s)
{
    hipLaunchKernelGGL(trend_loo_values_kernel, dim3((unsigned)m->P), dim3(256), 0, s, m->d_desc, m->d_info, m->d_tinfo,
                       m->d_dloo, (const real *)m->d_cm, m->d_tL, R, q, d_res, d_var);
    PMK_HIP(hipGetLastError());
    return 0;
}

}  // namespace PMK_NS

#ifndef PMK_REAL_F32
// One thread per sorted item p (row p of U, ld columns: R means, then a = kq^T C_H in columns R .. R + q - 1).
// Operation order, fixed: rho_a = h_a - a_a for a = 0 .. q - 1; mu_j = fma(h_a, beta[a][j], mu_j) for a = 0 .. q - 1;
// add = |L_G^-1 rho|^2 (trend_leverage, pmk_items.h); v <- v + add (v has been clamped at min_v before).
__global__ __launch_bounds__(256) void trend_items_kernel(int64_t total, const int32_t *__restrict__ sorted_item,
                                                          const int32_t *__restrict__ item_region,
                                                          const int32_t *__restrict__ item_query, const double *__restrict__ xq,
                                                          int D, int R, int q, int ld, const double *__restrict__ beta,
                                                          const double *__restrict__ Lg, double *__restrict__ U,
                                                          double *__restrict__ v)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= total) return;
    const int32_t it = sorted_item[p];
    const int64_t r = item_region[it], qi = item_query[it];
    double h[TQ_MAX], rho[TQ_MAX];
    h[0] = 1.0;
    for (int a = 1; a < q; ++a) h[a] = xq[qi * D + (a - 1)];
    double *row = U + p * ld;
    for (int a = 0; a < q; ++a) rho[a] = h[a] - row[R + a];
    const double *b = beta + r * TR_BETA;
    for (int j = 0; j < R; ++j) {
        double t = row[j];
        for (int a = 0; a < q; ++a) t = __builtin_fma(h[a], b[a + TQ_MAX * j], t);
        row[j] = t;
    }
    if (v) {
        const double s = trend_leverage(Lg + r * TR_G, q, [&](int a) { return rho[a]; });
        v[p] = v[p] + s;
    }
}

int launch_trend_items(pmk_query *q, int R, int qt, bool want_var, hipStream_t s)
{
    const pmk_model *m = q->m;
    if (q->total == 0) return 0;
    hipLaunchKernelGGL(trend_items_kernel, grid256(q->total), dim3(256), 0, s, q->total, q->d_sorted_item,
                       q->d_item_region, q->d_item_query, q->d_xq, m->D, R, qt, q->um_ld, m->d_tbeta, m->d_tL, q->d_um,
                       want_var ? q->d_v : nullptr);
    PMK_HIP(hipGetLastError());
    return 0;
}
#endif

}  // namespace pmk

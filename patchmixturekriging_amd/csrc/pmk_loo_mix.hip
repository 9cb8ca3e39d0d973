// Blended leave-one-out (pmk_query_items_loo, pmk_query_items_loo_multi): stage 2 of a query whose points ARE the
// training points of a tree-built model, query j = global point j.  Leaving point j out removes it from every patch that
// holds it and changes nothing else (the patches are independent GPs, the tree is held fixed), so an item (point j,
// region r) is one of two things:
//
//   member      patch r holds j as row i.  The prediction at x_j from the other n - 1 rows is the Schur complement of row i
//               of U = K + sigma2 I:  mu = y_i - c_i / d_i, noisy variance 1 / d_i, latent variance 1 / d_i - sigma2_r, with
//               d = diag(U^-1) from pmk_model_loo.  A lookup: no strip runs.
//   non-member  patch r never saw j (a neighbour reached with radius > eps): the ordinary queryinner! of x_j, done by an
//               inner query of explicit items on the untouched item kernels.
//
//   loo_member_kernel    one thread per sorted item: binary search of j in the patch's ascending index list, the member
//                        formula, and a 0 / 1 non-member mark
//   loo_compact_kernel   points, regions and addends of the non-members, in sorted order, at the positions an exclusive scan
//                        of the marks gives (the order is kept, so the inner query's stable sort leaves it as it is)
//   loo_scatter_kernel   the inner query's (u, v) back to the sorted positions; the noisy form adds sigma2_r here, one add
//                        after the strip kernel's clamp; NaN for a patch whose factorisation failed
//
// The R-column form (the multi-output path, with or without the per-patch trend of pmk_trend.hip) keeps all of this and
// changes the member formula alone: d_i becomes Q_ii = d_i - |L_G^-1 C_H[i, :]^T|^2 (Q_ii = d_i without a trend), by the
// forward substitution of trend_loo_values_kernel, and every column c < R gets mu_c = Y[i, c] - C[i, c] / Q_ii from the
// resident weight block (with a trend the universal-kriging weights C_Y - C_H beta).  A non-member is the item of
// pmk_query_items_multi_fitted for that (point, region).  loo_member_multi_kernel writes the R means into row k of U;
// loo_scatter_multi_kernel copies the inner query's row and v (the noisy add comes after the trend term; NaN also for a
// flagged patch).  Both also write u[k] (the single-output item mean buffer), which the unchanged mix_kernel reads next
// to v when pmk_query_mix_multi blends Vq: column 0's mean, never used.
//
// All arithmetic of the member formulas is double with IEEE division; y and c are cast from the element type exactly as
// the values kernels (pmk_loo.hip, pmk_trend.hip) cast them, so u and v are the values numpy computes from
// pmk_model_get_loo's res and var (pmk_model_get_loo_multi's RES and var).  The traffic is a few bytes per item: nothing
// here is tuned.
#include "pmk_dispatch.h"
#include "pmk_items.h"
#include "pmk_real.h"

// the member formulas promise bits: no contraction, whatever the compiler's default becomes
#pragma clang fp contract(off)

namespace pmk {
namespace PMK_NS {

__global__ __launch_bounds__(256) void loo_member_kernel(int64_t total, const int32_t *__restrict__ sorted_item,
                                                         const int32_t *__restrict__ item_query,
                                                         const int32_t *__restrict__ item_region, int32_t leaf_base,
                                                         const PatchDesc *__restrict__ descs, const int64_t *__restrict__ pidx_off,
                                                         const int32_t *__restrict__ pidx, const int32_t *__restrict__ info,
                                                         const real *__restrict__ Y, const real *__restrict__ Cw,
                                                         const double *__restrict__ dloo, const double *__restrict__ sigma2s,
                                                         double sigma2, int noisy, double min_v, double *__restrict__ u_out,
                                                         double *__restrict__ v_out, int32_t *__restrict__ mark)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= total) return;
    const int32_t it = sorted_item[k];
    const int32_t j = item_query[it];
    const int32_t p = item_region[it] - leaf_base;
    int64_t i;
    const bool member = patch_holds(pidx_off, pidx, p, j, i);
    mark[k] = !member;
    if (!member) return;
    const int64_t e = descs[p].yoff + i;
    double u = __builtin_nan(""), v = __builtin_nan("");
    if (info[p] == 0) {
        const double d = dloo[e];
        const double var = 1.0 / d;
        u = (double)Y[e] - (double)Cw[e] / d;
        v = noisy ? var : latent_variance(var, patch_noise(sigma2s, sigma2, p), min_v);
    }
    u_out[k] = u;
    v_out[k] = v;
}

// TR_RP (columns of a row of the target / weight block) and TQ_MAX (leading dimension of L_G) are pmk_internal.h's.
// ld: row length of U (R + q).  tinfo, Lg: null without a trend (q == 0).  v_out: null for a mean-only run.
__global__ __launch_bounds__(256) void loo_member_multi_kernel(int64_t total, const int32_t *__restrict__ sorted_item,
                                                               const int32_t *__restrict__ item_query,
                                                               const int32_t *__restrict__ item_region, int32_t leaf_base,
                                                               const PatchDesc *__restrict__ descs,
                                                               const int64_t *__restrict__ pidx_off, const int32_t *__restrict__ pidx,
                                                               const int32_t *__restrict__ info, const int32_t *__restrict__ tinfo,
                                                               const real *__restrict__ Y, const real *__restrict__ Cw,
                                                               const double *__restrict__ dloo, const double *__restrict__ Lg,
                                                               int R, int q, int ld, const double *__restrict__ sigma2s,
                                                               double sigma2, int noisy, double min_v, double *__restrict__ U,
                                                               double *__restrict__ u_out, double *__restrict__ v_out,
                                                               int32_t *__restrict__ mark)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= total) return;
    const int32_t it = sorted_item[k];
    const int32_t j = item_query[it];
    const int32_t p = item_region[it] - leaf_base;
    int64_t i;
    const bool member = patch_holds(pidx_off, pidx, p, j, i);
    mark[k] = !member;
    if (!member) return;
    const int64_t e = descs[p].yoff + i;
    const int64_t row = e * TR_RP;
    const bool bad = patch_is_bad_loo(info, tinfo, p, q, descs[p].n);
    const double nan = __builtin_nan("");
    const double *L = Lg ? Lg + (int64_t)p * (TQ_MAX * TQ_MAX) : nullptr;      // null exactly when q == 0
    const double s = trend_leverage(L, q, [&](int a) { return (double)Cw[row + R + a]; });
    const double Q = dloo[e] - s;
    double *out = U + k * ld;
    for (int c = 0; c < R; ++c) out[c] = bad ? nan : (double)Y[row + c] - (double)Cw[row + c] / Q;
    for (int c = R; c < ld; ++c) out[c] = 0.0;
    u_out[k] = out[0];
    if (v_out) {
        const double var = 1.0 / Q;
        const double v = noisy ? var : latent_variance(var, patch_noise(sigma2s, sigma2, p), min_v);
        v_out[k] = bad ? nan : v;
    }
}

template <int D>
__global__ __launch_bounds__(256) void loo_compact_kernel(int64_t total, const int32_t *__restrict__ mark,
                                                          const int64_t *__restrict__ off, const int32_t *__restrict__ sorted_item,
                                                          const int32_t *__restrict__ item_query,
                                                          const int32_t *__restrict__ item_region, const double *__restrict__ xq,
                                                          const double *__restrict__ qdiag, double *__restrict__ x_out,
                                                          int32_t *__restrict__ region_out, double *__restrict__ diag_out)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= total || !mark[k]) return;
    const int64_t o = off[k];
    const int32_t it = sorted_item[k];
    const int64_t j = item_query[it];
#pragma unroll
    for (int d = 0; d < D; ++d) x_out[o * D + d] = xq[j * D + d];
    region_out[o] = item_region[it];
    if (qdiag) diag_out[o] = qdiag[j];
}

__global__ __launch_bounds__(256) void loo_scatter_kernel(int64_t total, const int32_t *__restrict__ mark,
                                                          const int64_t *__restrict__ off, const int32_t *__restrict__ sorted_item,
                                                          const int32_t *__restrict__ item_region, int32_t leaf_base,
                                                          const int32_t *__restrict__ info, const double *__restrict__ ru,
                                                          const double *__restrict__ rv, const double *__restrict__ sigma2s,
                                                          double sigma2, int noisy, double *__restrict__ u_out,
                                                          double *__restrict__ v_out)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= total || !mark[k]) return;
    const int64_t o = off[k];
    const int32_t p = item_region[sorted_item[k]] - leaf_base;
    double u = ru[o], v = rv[o];
    if (noisy) v = v + patch_noise(sigma2s, sigma2, p);
    // a failed patch answers NaN on both routes (the strips ran on whatever its factorisation left behind)
    if (patch_is_bad(info, nullptr, p)) u = v = __builtin_nan("");
    u_out[k] = u;
    v_out[k] = v;
}

int launch_loo_member(pmk_query *q, int noisy, int32_t *d_mark, hipStream_t s)
{
    const pmk_model *m = q->m;
    if (q->total == 0) return 0;
    hipLaunchKernelGGL(loo_member_kernel, grid256(q->total), dim3(256), 0, s, q->total, q->d_sorted_item, q->d_item_query,
                       q->d_item_region, (int32_t)m->leaf_base, m->d_desc, m->d_pidx_off, m->d_pidx, m->d_info,
                       (const real *)m->d_y, (const real *)m->d_c, m->d_dloo, patch_sigma2s(m), m->sigma2, noisy, q->min_v,
                       q->d_u, q->d_v, d_mark);
    PMK_HIP(hipGetLastError());
    return 0;
}

int launch_loo_member_multi(pmk_query *q, int noisy, int want_var, int32_t *d_mark, hipStream_t s)
{
    const pmk_model *m = q->m;
    if (q->total == 0) return 0;
    const int qt = m->trend_q;
    hipLaunchKernelGGL(loo_member_multi_kernel, grid256(q->total), dim3(256), 0, s, q->total, q->d_sorted_item,
                       q->d_item_query, q->d_item_region, (int32_t)m->leaf_base, m->d_desc, m->d_pidx_off, m->d_pidx,
                       m->d_info, qt > 0 ? m->d_tinfo : nullptr, (const real *)m->d_ym, (const real *)m->d_cm, m->d_dloo,
                       qt > 0 ? m->d_tL : nullptr, q->R_items, qt, q->um_ld, patch_sigma2s(m), m->sigma2, noisy, q->min_v,
                       q->d_um, q->d_u, want_var ? q->d_v : nullptr, d_mark);
    PMK_HIP(hipGetLastError());
    return 0;
}

int launch_loo_compact(pmk_query *q, const int32_t *d_mark, const int64_t *d_off, double *x_out, int32_t *region_out,
                       double *diag_out, hipStream_t s)
{
    if (q->total == 0) return 0;
    const dim3 grid = grid256(q->total), block(256);
    const int rc = dispatch_dim(q->m->D, [&](auto dd) {
        hipLaunchKernelGGL(loo_compact_kernel<dd()>, grid, block, 0, s, q->total, d_mark, d_off, q->d_sorted_item, q->d_item_query,
                           q->d_item_region, q->d_xq, q->d_qdiag, x_out, region_out, diag_out);
        return 0;
    });
    if (rc) return rc;
    PMK_HIP(hipGetLastError());
    return 0;
}

int launch_loo_scatter(pmk_query *q, int noisy, const int32_t *d_mark, const int64_t *d_off, const double *d_ru,
                       const double *d_rv, hipStream_t s)
{
    const pmk_model *m = q->m;
    if (q->total == 0) return 0;
    hipLaunchKernelGGL(loo_scatter_kernel, grid256(q->total), dim3(256), 0, s, q->total, d_mark, d_off, q->d_sorted_item,
                       q->d_item_region, (int32_t)m->leaf_base, m->d_info, d_ru, d_rv, patch_sigma2s(m), m->sigma2, noisy,
                       q->d_u, q->d_v);
    PMK_HIP(hipGetLastError());
    return 0;
}

}  // namespace PMK_NS

#ifndef PMK_REAL_F32
// in_pos: the inner query's item -> sorted position (its item o is request o); in_U, in_v: its results, sorted order.
// R columns are copied; the columns R .. ld - 1 of the outer row (kq . C_H of the inner run) are not needed again: zero.
__global__ __launch_bounds__(256) void loo_scatter_multi_kernel(int64_t total, const int32_t *__restrict__ mark,
                                                                const int64_t *__restrict__ off,
                                                                const int32_t *__restrict__ sorted_item,
                                                                const int32_t *__restrict__ item_region, int32_t leaf_base,
                                                                const int32_t *__restrict__ info, const int32_t *__restrict__ tinfo,
                                                                const int32_t *__restrict__ in_pos, const double *__restrict__ in_U,
                                                                int in_ld, const double *__restrict__ in_v,
                                                                const double *__restrict__ sigma2s, double sigma2, int noisy, int R,
                                                                int ld, double *__restrict__ U, double *__restrict__ u_out,
                                                                double *__restrict__ v_out)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= total || !mark[k]) return;
    const int64_t src = in_pos[off[k]];
    const int32_t p = item_region[sorted_item[k]] - leaf_base;
    // a failed or flagged patch answers NaN on both routes
    const bool bad = patch_is_bad(info, tinfo, p);
    const double nan = __builtin_nan("");
    const double *in = in_U + src * in_ld;
    double *out = U + k * ld;
    for (int c = 0; c < R; ++c) out[c] = bad ? nan : in[c];
    for (int c = R; c < ld; ++c) out[c] = 0.0;
    u_out[k] = out[0];
    if (v_out) {
        double v = in_v[src];
        if (noisy) v = v + patch_noise(sigma2s, sigma2, p);
        v_out[k] = bad ? nan : v;
    }
}

int launch_loo_scatter_multi(pmk_query *q, const pmk_query *in, int noisy, int want_var, const int32_t *d_mark,
                             const int64_t *d_off, hipStream_t s)
{
    const pmk_model *m = q->m;
    if (q->total == 0) return 0;
    const int qt = m->trend_q;
    hipLaunchKernelGGL(loo_scatter_multi_kernel, grid256(q->total), dim3(256), 0, s, q->total, d_mark, d_off,
                       q->d_sorted_item, q->d_item_region, (int32_t)m->leaf_base, m->d_info,
                       qt > 0 ? m->d_tinfo : nullptr, in->d_item_pos, in->d_um, in->um_ld, want_var ? in->d_v : nullptr,
                       patch_sigma2s(m), m->sigma2, noisy, q->R_items, q->um_ld, q->d_um, q->d_u,
                       want_var ? q->d_v : nullptr);
    PMK_HIP(hipGetLastError());
    return 0;
}
#endif

}  // namespace pmk

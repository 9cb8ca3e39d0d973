// Blended leave-one-out on the multi-output path (pmk_query_items_loo_multi): pmk_loo_mix.hip for R target columns and
// the per-patch trend of pmk_trend.hip.  Query j = global point j; an item (point j, region r) is
//
//   member      patch r holds j as row i.  Q_ii = d_i - |L_G^-1 C_H[i, :]^T|^2 (Q_ii = d_i without a trend), and for every
//               column c < R:  mu_c = Y[i, c] - C[i, c] / Q_ii; noisy variance 1 / Q_ii, latent max(1 / Q_ii - sigma2_r, min_v).
//               C is the resident weight block: with a trend the universal-kriging weights C_Y - C_H beta.
//   non-member  the item of pmk_query_items_multi_fitted for that (point, region), run by the inner query of explicit
//               items as pmk_query_items_loo does; untouched kernels.
//
//   loo_member_multi_kernel    one thread per sorted item: the binary search of loo_member_kernel, Q_ii by the forward
//                              substitution of trend_loo_values_kernel (same index order, same fma chain: the same bits),
//                              the R means into row k of U, v, and the 0 / 1 non-member mark
//   loo_scatter_multi_kernel   the inner query's row (R means) and v back to the sorted position; the noisy form adds
//                              sigma2_r here, one add after the trend term; NaN for a failed or flagged patch
//
// Both also write u[k] (the single-output item mean buffer), which the unchanged mix_kernel reads next to v when
// pmk_query_mix_multi blends Vq: column 0's mean, never used.
// All arithmetic is double with IEEE division; Y and C are cast from the element type as the values kernels cast them, so
// a member item is what numpy computes from pmk_model_get_loo_multi's RES and var.
#include "pmk_dispatch.h"
#include "pmk_real.h"

// the member formula promises bits: no contraction, whatever the compiler's default becomes
#pragma clang fp contract(off)

namespace pmk {

// TR_RP (columns of a row of the target / weight block) and TQ_MAX (leading dimension of L_G, column-major
// TQ_MAX x TQ_MAX per patch) are pmk_trend.hip's, from pmk_internal.h

namespace PMK_NS {

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
    // the first entry of the patch's list that is >= j
    int64_t lo = pidx_off[p], hi = pidx_off[p + 1];
    const int64_t base = lo, end = hi;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (pidx[mid] < j) lo = mid + 1;
        else hi = mid;
    }
    if (lo == end || pidx[lo] != j) {
        mark[k] = 1;
        return;
    }
    mark[k] = 0;
    const int64_t e = descs[p].yoff + (lo - base);
    const int64_t row = e * TR_RP;
    // n <= q: the point left out, fewer points remain than basis functions (trend_loo_values_kernel's rule)
    const bool bad = info[p] != 0 || (tinfo && tinfo[p] != 0) || (q > 0 && descs[p].n <= q);
    const double nan = __builtin_nan("");
    double z[TQ_MAX], s = 0.0;
    const double *L = Lg ? Lg + (int64_t)p * (TQ_MAX * TQ_MAX) : nullptr;      // null exactly when q == 0
    for (int a = 0; a < q; ++a) {
        double t = (double)Cw[row + R + a];
        for (int kk = 0; kk < a; ++kk) t = __builtin_fma(-L[a + TQ_MAX * kk], z[kk], t);
        z[a] = t / L[a + TQ_MAX * a];
        s = __builtin_fma(z[a], z[a], s);
    }
    const double Q = dloo[e] - s;
    double *out = U + k * ld;
    for (int c = 0; c < R; ++c) out[c] = bad ? nan : (double)Y[row + c] - (double)Cw[row + c] / Q;
    for (int c = R; c < ld; ++c) out[c] = 0.0;
    u_out[k] = out[0];
    if (v_out) {
        const double var = 1.0 / Q;
        double v = var;
        if (!noisy) {
            const double lat = var - (sigma2s ? sigma2s[p] : sigma2);
            v = lat < min_v ? min_v : lat;
        }
        v_out[k] = bad ? nan : v;
    }
}

int launch_loo_member_multi(pmk_query *q, int noisy, int want_var, int32_t *d_mark, hipStream_t s)
{
    const pmk_model *m = q->m;
    if (q->total == 0) return 0;
    const int qt = m->trend_q;
    hipLaunchKernelGGL(loo_member_multi_kernel, dim3((unsigned)((q->total + 255) / 256)), dim3(256), 0, s, q->total,
                       q->d_sorted_item, q->d_item_query, q->d_item_region, (int32_t)m->leaf_base, m->d_desc, m->d_pidx_off,
                       m->d_pidx, m->d_info, qt > 0 ? m->d_tinfo : nullptr, (const real *)m->d_ym, (const real *)m->d_cm,
                       m->d_dloo, qt > 0 ? m->d_tL : nullptr, q->R_items, qt, q->um_ld, patch_sigma2s(m), m->sigma2, noisy,
                       q->min_v, q->d_um, q->d_u, want_var ? q->d_v : nullptr, d_mark);
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
    const bool bad = info[p] != 0 || (tinfo && tinfo[p] != 0);
    const double nan = __builtin_nan("");
    const double *in = in_U + src * in_ld;
    double *out = U + k * ld;
    for (int c = 0; c < R; ++c) out[c] = bad ? nan : in[c];
    for (int c = R; c < ld; ++c) out[c] = 0.0;
    u_out[k] = out[0];
    if (v_out) {
        double v = in_v[src];
        if (noisy) v = v + (sigma2s ? sigma2s[p] : sigma2);
        v_out[k] = bad ? nan : v;
    }
}

int launch_loo_scatter_multi(pmk_query *q, const pmk_query *in, int noisy, int want_var, const int32_t *d_mark,
                             const int64_t *d_off, hipStream_t s)
{
    const pmk_model *m = q->m;
    if (q->total == 0) return 0;
    const int qt = m->trend_q;
    hipLaunchKernelGGL(loo_scatter_multi_kernel, dim3((unsigned)((q->total + 255) / 256)), dim3(256), 0, s, q->total, d_mark,
                       d_off, q->d_sorted_item, q->d_item_region, (int32_t)m->leaf_base, m->d_info,
                       qt > 0 ? m->d_tinfo : nullptr, in->d_item_pos, in->d_um, in->um_ld, want_var ? in->d_v : nullptr,
                       patch_sigma2s(m), m->sigma2, noisy, q->R_items, q->um_ld, q->d_um, q->d_u,
                       want_var ? q->d_v : nullptr);
    PMK_HIP(hipGetLastError());
    return 0;
}
#endif

}  // namespace pmk

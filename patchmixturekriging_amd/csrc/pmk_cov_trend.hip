// The trend's term of the joint covariance on the multi-output path (pmk_query_items_cov_multi): under a trend with q
// basis functions the universal-kriging covariance of a region's items is
//
//   S[a, b] = k(x_a, x_b) - V_a . V_b + z_a . z_b,   z = L_G^-1 rho,   rho = h(x) - C_H^T k(X, x),
//
// the first two terms being the block that cov_block_kernel (pmk_cov.hip) leaves.  Everything else is resident: L_G and
// tinfo per patch after pmk_model_solve_multi, a = kq^T C_H in columns R .. R + q - 1 of the item rows after
// pmk_query_items_multi (trend_items_kernel, pmk_trend.hip, reads them and does not overwrite them).
//
//   cov_trend_items_kernel   one thread per sorted item p: z_p = L_G^-1 rho_p into row p of Z (sorted items x TQ_MAX)
//   cov_trend_block_kernel   on the launch geometry of cov_block_kernel, after it: S[a, b] <- S[a, b] + z_a . z_b
//   cov_trend_flags_kernel   per patch: info != 0 or tinfo != 0, the mark mix_cov_kernel reads in place of info
//
// Bits.  rho and z are taken as trend_items_kernel takes them (trend_forward, pmk_items.h), t = z_a . z_b is one chain of
// fused multiply-adds from 0 in ascending a and joins the block with one addition: on the diagonal t is the leverage
// |z|^2 of trend_forward, added after the clamp at min_v, as the item variance has it.  An entry depends on its two items
// only, the lower triangle is a copy of the upper one, nothing is accumulated across threads.  All double: the file is
// compiled once and serves the models of both element types.
#include "pmk_items.h"

namespace pmk {

constexpr int CT_G = TQ_MAX * TQ_MAX;         // doubles of L_G per patch (pmk_trend.hip)
constexpr int CT_SLICES = 16;                 // BLOCK_SLICES of pmk_cov.hip: workgroups that share one pair's entries

// Row p of U holds a = kq^T C_H in columns R .. R + q - 1 (ld columns a row).  Operation order, fixed: rho_a = h_a - a_a
// for a = 0 .. q - 1 with h = [1, x_1 .. x_D], z = L_G^-1 rho by trend_forward; the entries a >= q of the row are zero.
__global__ __launch_bounds__(256) void cov_trend_items_kernel(int64_t total, const int32_t *__restrict__ sorted_item,
                                                              const int32_t *__restrict__ item_region,
                                                              const int32_t *__restrict__ item_query,
                                                              const double *__restrict__ xq, int D, int R, int q, int ld,
                                                              const double *__restrict__ Lg, const double *__restrict__ U,
                                                              double *__restrict__ Z)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= total) return;
    const int32_t it = sorted_item[p];
    const int64_t r = item_region[it], qi = item_query[it];
    const double *row = U + p * ld;
    double z[TQ_MAX];
    for (int a = 0; a < TQ_MAX; ++a) z[a] = 0.0;
    trend_forward(Lg + r * CT_G, q, [&](int a) { return (a == 0 ? 1.0 : xq[qi * D + (a - 1)]) - row[R + a]; }, z);
    for (int a = 0; a < TQ_MAX; ++a) Z[p * TQ_MAX + a] = z[a];
}

// blockIdx.x: a pair of strips of one region, its entries (a, b) with a <= b in the region's order dealt over gridDim.y
// workgroups exactly as cov_block_kernel deals them.  The items of a strip are the sorted items first .. first + count - 1.
__global__ __launch_bounds__(256) void cov_trend_block_kernel(const CovTask *__restrict__ tasks,
                                                              const CovPair *__restrict__ pairs,
                                                              const double *__restrict__ Z, int q,
                                                              const int32_t *__restrict__ info,
                                                              const int32_t *__restrict__ tinfo, double *__restrict__ G)
{
    const CovPair pr = pairs[blockIdx.x];
    const CovTask ta = tasks[pr.ta], tb = tasks[pr.tb];
    const bool bad = patch_is_bad(info, tinfo, ta.region);
    double *Gr = G + ta.goff;
    const int64_t m = ta.m;
    const int total = ta.count * tb.count;
    for (int e = (int)blockIdx.y * 256 + (int)threadIdx.x; e < total; e += (int)gridDim.y * 256) {
        const int a = e % ta.count, b = e / ta.count;
        const int64_t ra = ta.a0 + a, rb = tb.a0 + b;
        if (ra > rb) continue;
        const double *za = Z + (ta.first + a) * TQ_MAX, *zb = Z + (tb.first + b) * TQ_MAX;
        double t = 0.0;
        for (int k = 0; k < q; ++k) t = __builtin_fma(za[k], zb[k], t);
        double s = Gr[ra + m * rb] + t;
        if (bad) s = __builtin_nan("");
        Gr[ra + m * rb] = s;
        Gr[rb + m * ra] = s;
    }
}

__global__ __launch_bounds__(256) void cov_trend_flags_kernel(int64_t P, const int32_t *__restrict__ info,
                                                              const int32_t *__restrict__ tinfo, int32_t *__restrict__ flags)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r < P) flags[r] = patch_is_bad(info, tinfo, r) ? 1 : 0;
}

// Z alone, for the callers that need no block (pmk_query_items_block): the same kernel on the same arguments
int launch_cov_trend_items(pmk_query *q, hipStream_t s)
{
    const pmk_model *m = q->m;
    if (q->total == 0) return 0;
    hipLaunchKernelGGL(cov_trend_items_kernel, grid256(q->total), dim3(256), 0, s, q->total, q->d_sorted_item,
                       q->d_item_region, q->d_item_query, q->d_xq, m->D, q->R_items, m->trend_q, q->um_ld, m->d_tL, q->d_um,
                       q->d_cov_z);
    PMK_HIP(hipGetLastError());
    return 0;
}

// after launch_items_cov on the same stream; the tasks, the pairs, Z and the flags are the caller's
// (pmk_query_items_cov_multi)
int launch_cov_trend(pmk_query *q, hipStream_t s)
{
    const pmk_model *m = q->m;
    const int qt = m->trend_q;
    hipLaunchKernelGGL(cov_trend_flags_kernel, grid256(m->P), dim3(256), 0, s, m->P, (const int32_t *)m->d_info,
                       (const int32_t *)m->d_tinfo, q->d_cov_flags);
    PMK_HIP(hipGetLastError());
    if (q->total == 0 || q->cov_npairs == 0) return 0;
    hipLaunchKernelGGL(cov_trend_items_kernel, grid256(q->total), dim3(256), 0, s, q->total, q->d_sorted_item,
                       q->d_item_region, q->d_item_query, q->d_xq, m->D, q->R_items, qt, q->um_ld, m->d_tL, q->d_um, q->d_cov_z);
    PMK_HIP(hipGetLastError());
    hipLaunchKernelGGL(cov_trend_block_kernel, dim3((unsigned)q->cov_npairs, CT_SLICES), dim3(256), 0, s, q->d_cov_tasks,
                       q->d_cov_pairs, q->d_cov_z, qt, (const int32_t *)m->d_info, (const int32_t *)m->d_tinfo, q->d_cov_s);
    PMK_HIP(hipGetLastError());
    return 0;
}

}  // namespace pmk

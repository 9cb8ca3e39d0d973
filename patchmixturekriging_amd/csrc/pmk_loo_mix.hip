// Blended leave-one-out (pmk_query_items_loo): stage 2 of a query whose points ARE the training points of a tree-built
// model, query j = global point j.  Leaving point j out removes it from every patch that holds it and changes nothing
// else (the patches are independent GPs, the tree is held fixed), so an item (point j, region r) is one of two things:
//
//   member      patch r holds j as row i.  The prediction at x_j from the other n - 1 rows is the Schur complement of row i
//               of U = K + sigma2 I:  mu = y_i - c_i / d_i, noisy variance 1 / d_i, latent variance 1 / d_i - sigma2_r, with
//               d = diag(U^-1) from pmk_model_loo.  A lookup: no strip runs.
//   non-member  patch r never saw j (a neighbour reached with radius > eps): the ordinary queryinner! of x_j, done by an
//               inner query of explicit items on the strip kernel, untouched.
//
//   loo_member_kernel    one thread per sorted item: binary search of j in the patch's ascending index list, the member
//                        formula, and a 0 / 1 non-member mark
//   loo_compact_kernel   points, regions and addends of the non-members, in sorted order, at the positions an exclusive scan
//                        of the marks gives (the order is kept, so the inner query's stable sort leaves it as it is)
//   loo_scatter_kernel   the inner query's (u, v) back to the sorted positions; the noisy form adds sigma2_r here, one add
//                        after the strip kernel's clamp; NaN for a patch whose factorisation failed
//
// All arithmetic of the member formula is double with IEEE division; y and c are cast from the element type exactly as
// loo_values_kernel (pmk_loo.hip) casts c, so u and v are the values numpy computes from pmk_model_get_loo's res and var.
// The traffic is a few bytes per item: nothing here is tuned.
#include "pmk_dispatch.h"
#include "pmk_real.h"

// the member formula promises bits: no contraction, whatever the compiler's default becomes
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
    double u = __builtin_nan(""), v = __builtin_nan("");
    if (info[p] == 0) {
        const double d = dloo[e];
        const double var = 1.0 / d;
        u = (double)Y[e] - (double)Cw[e] / d;
        if (noisy) v = var;
        else {
            const double lat = var - (sigma2s ? sigma2s[p] : sigma2);
            v = lat < min_v ? min_v : lat;
        }
    }
    u_out[k] = u;
    v_out[k] = v;
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
    if (noisy) v = v + (sigma2s ? sigma2s[p] : sigma2);
    // a failed patch answers NaN on both routes (the strips ran on whatever its factorisation left behind)
    if (info[p] != 0) u = v = __builtin_nan("");
    u_out[k] = u;
    v_out[k] = v;
}

int launch_loo_member(pmk_query *q, int noisy, int32_t *d_mark, hipStream_t s)
{
    const pmk_model *m = q->m;
    if (q->total == 0) return 0;
    hipLaunchKernelGGL(loo_member_kernel, dim3((unsigned)((q->total + 255) / 256)), dim3(256), 0, s, q->total, q->d_sorted_item,
                       q->d_item_query, q->d_item_region, (int32_t)m->leaf_base, m->d_desc, m->d_pidx_off, m->d_pidx, m->d_info,
                       (const real *)m->d_y, (const real *)m->d_c, m->d_dloo, patch_sigma2s(m), m->sigma2, noisy, q->min_v,
                       q->d_u, q->d_v, d_mark);
    PMK_HIP(hipGetLastError());
    return 0;
}

int launch_loo_compact(pmk_query *q, const int32_t *d_mark, const int64_t *d_off, double *x_out, int32_t *region_out,
                       double *diag_out, hipStream_t s)
{
    if (q->total == 0) return 0;
    const dim3 grid((unsigned)((q->total + 255) / 256)), block(256);
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
    hipLaunchKernelGGL(loo_scatter_kernel, dim3((unsigned)((q->total + 255) / 256)), dim3(256), 0, s, q->total, d_mark, d_off,
                       q->d_sorted_item, q->d_item_region, (int32_t)m->leaf_base, m->d_info, d_ru, d_rv, patch_sigma2s(m), m->sigma2,
                       noisy, q->d_u, q->d_v);
    PMK_HIP(hipGetLastError());
    return 0;
}

}  // namespace PMK_NS
}  // namespace pmk

// The device rules of the (query, region) items and of their blend, each stated once: the kernels of pmk_multi.hip,
// pmk_grad.hip, pmk_loo_mix.hip, pmk_trend.hip and mix_kernel (pmk_kernels.hip) promise each other bits, and sharing
// these functions is how they keep the promise.  No `#pragma clang fp contract` here and no expression a contraction
// could change (every fused multiply-add is spelled __builtin_fma): a call site keeps the mode of its own file.
#pragma once

#include "pmk_device.h"

namespace pmk {

// ---- chunks of 16 sorted items (item_means_kernel, item_grads_kernel) ----
// Chunk g of the whole list lies in the region r with cpre[r] <= g < cpre[r + 1] (chunks per region, host prefix, P
// regions).  The kernels take its items [first, first + count) from roff themselves: tests/_multi_refs.py restates that
// rule from the text of pmk_multi.hip.
__device__ __forceinline__ int chunk_region(const int64_t *cpre, int P, int64_t g)
{
    int lo = 0, hi = P;                                      // cpre[lo] <= g < cpre[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (cpre[mid] <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}

// the query point of item li of the chunk [first, first + count), rounded to the element type; zero for the lanes past
// the chunk's end
template <int D, typename R>
__device__ __forceinline__ void chunk_query_point(int64_t first, int count, int li, const int32_t *sorted_item,
                                                  const int32_t *item_query, const double *xq, R (&q)[D])
{
    if (li < count) {
        const int64_t qi = item_query[sorted_item[first + li]];
#pragma unroll
        for (int d = 0; d < D; ++d) q[d] = (R)xq[qi * D + d];
    } else {
#pragma unroll
        for (int d = 0; d < D; ++d) q[d] = (R)0;
    }
}

// ---- the blend (mixtureGP.jl:224-272): items [b, e) of a query, neighbours in hyperplane order, home last ----
// weight of item it: phi_w(|t|) for a neighbour, 1 for the home item
__device__ __forceinline__ double blend_weight(const pmk_kernel_desc &wth, const double *item_t, int64_t it, int64_t e)
{
    return (it == e - 1) ? 1.0 : profile(wth, fabs(item_t[it]));
}
// the sum of the weights in item order, the first weight taken as it is; keep(it, w) sees every weight on the way
template <class Keep>
__device__ __forceinline__ double blend_weight_sum(const pmk_kernel_desc &wth, const double *item_t, int64_t b, int64_t e,
                                                   Keep keep)
{
    double sw = 0.0;
    for (int64_t it = b; it < e; ++it) {
        const double w = blend_weight(wth, item_t, it, e);
        keep(it, w);
        sw = (it == b) ? w : sw + w;
    }
    return sw;
}
__device__ __forceinline__ double blend_weight_sum(const pmk_kernel_desc &wth, const double *item_t, int64_t b, int64_t e)
{
    return blend_weight_sum(wth, item_t, b, e, [](int64_t, double) {});
}

// patch p holds the global point j; row: the first entry >= j of its ascending index list pidx[pidx_off[p] .. pidx_off[p + 1])
__device__ __forceinline__ bool patch_holds(const int64_t *pidx_off, const int32_t *pidx, int32_t p, int32_t j, int64_t &row)
{
    int64_t lo = pidx_off[p], hi = pidx_off[p + 1];
    const int64_t base = lo, end = hi;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (pidx[mid] < j) lo = mid + 1;
        else hi = mid;
    }
    row = lo - base;
    return lo != end && pidx[lo] == j;
}

// sigma2 of patch p: the model's device array after a per-patch fit, one value otherwise (patch_sigma2s, pmk_internal.h)
__device__ __forceinline__ double patch_noise(const double *sigma2s, double sigma2, int32_t p)
{
    return sigma2s ? sigma2s[p] : sigma2;
}
// latent variance from the noisy one, clamped below as the strip kernel clamps it
__device__ __forceinline__ double latent_variance(double var, double noise, double min_v)
{
    const double lat = var - noise;
    return lat < min_v ? min_v : lat;
}

// patch p answers NaN: its factorisation failed, or its trend is flagged (tinfo null: the model has no trend)
__device__ __forceinline__ bool patch_is_bad(const int32_t *info, const int32_t *tinfo, int64_t p)
{
    return info[p] != 0 || (tinfo && tinfo[p] != 0);
}
// the same for leave-one-out with q basis functions: n <= q, the point left out, fewer points remain than basis
// functions, no such prediction (Q_ii is rounding noise)
__device__ __forceinline__ bool patch_is_bad_loo(const int32_t *info, const int32_t *tinfo, int64_t p, int q, int n)
{
    return patch_is_bad(info, tinfo, p) || (q > 0 && n <= q);
}

// ---- the trend's q x q factor L_G, column-major with leading dimension TQ_MAX ----
// z = L_G^-1 rhs, rhs(a) the right-hand side: z_a = (rhs_a - sum_{k < a} L[a][k] z_k) / L[a][a], the sum as an fma chain
// in k order, IEEE division.  Returns the leverage |z|^2 as an fma chain in a order (it does not feed the solve).
template <class Rhs>
__device__ __forceinline__ double trend_forward(const double *L, int q, Rhs rhs, double *z)
{
    double s = 0.0;
    for (int a = 0; a < q; ++a) {
        double t = rhs(a);
        for (int k = 0; k < a; ++k) t = __builtin_fma(-L[a + TQ_MAX * k], z[k], t);
        z[a] = t / L[a + TQ_MAX * a];
        s = __builtin_fma(z[a], z[a], s);
    }
    return s;
}
template <class Rhs>
__device__ __forceinline__ double trend_leverage(const double *L, int q, Rhs rhs)
{
    double z[TQ_MAX];
    return trend_forward(L, q, rhs, z);
}

}  // namespace pmk

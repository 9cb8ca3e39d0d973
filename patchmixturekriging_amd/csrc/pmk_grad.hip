// Gradient of the blended mean of the multi-output path (R <= 16 columns, with or without a trend).
//
//   item_grads_kernel   G[item][d + D c] = d/dx_d of the item mean of column c at the item's query point:
//                       sum_k psi(tau_k) (x_d - z_{k,d}) C_r[k, c]  (+ beta_r[1 + d, c] with a linear trend), the MFMA of
//                       item_means_kernel (pmk_multi.hip) with D different A operands sharing one B operand
//   mix_grad_kernel     the gradient of the mixture of mix_multi_kernel, one thread per query (double only)
//
// For every stationary family grad_x k(x, z) = psi(tau) (x - z) with psi = phi'(tau) / tau (profile_dpsi, pmk_device.h),
// finite at tau = 0: no division by the distance, and a training point that coincides with the query contributes 0.
// The mixture weights depend on x only through t_i = c - v . x of the hyperplane the item was accepted at (item_plane,
// recorded by plan_kernel), whose gradient is -v.  With w_i = phi_w(|t_i|), S = sum_i w_i, Y_c = sum_i w_i u_{i,c} / S:
//
//   dY_c/dx_d = (1 / S) sum_i [ w_i G_{i,d,c} + (u_{i,c} - Y_c) dw_i/dx_d ],
//   dw_i/dx_d = -psi_w(|t_i|) t_i v_{plane(i),d} for a neighbour, 0 for the home item (w = 1).
//
// This is the derivative with the item list held fixed.  Where the list changes the blend itself jumps -- at the radius
// cut-off unless phi_w vanishes there, at a delta test, and where the home leaf changes -- and no derivative exists.
//
// A patch whose factorisation failed (info != 0), or whose trend is flagged (tinfo != 0), gives NaN in all D R values of
// its items, and through the blend in every query that uses one of them.  The q trend columns of C are not differentiated.
#include "pmk_device.h"
#include "pmk_dispatch.h"
#include "pmk_items.h"
#include "pmk_mfma.h"

namespace pmk {
namespace PMK_NS {

constexpr int IG_THREADS = 256;
constexpr int IG_RP = PMK_MAX_OUTPUTS;

// The chunking (chunk_region, pmk_items.h), XCD remap and operand layout of item_means_kernel: one wave per chunk of (up
// to) 16 items of one region.  Lane l evaluates tau once for (item l & 15, point k0 + (l >> 4)), forms the D operands
// psi (q_d - x_d) and issues D MFMAs against the same row of C_r.  R: target columns emitted (c < R only).
// beta: the model's trend coefficients when the trend is linear (beta[(r 16 + c) 5 + 1 + d]), else null.
// Operation order of the store, fixed: g = (double)(acc0 + acc1), then g + beta[1 + d][c] (one double addition).
template <int D, int FAM, bool PP = false>
__global__ __launch_bounds__(IG_THREADS) void item_grads_kernel(const PatchDesc *__restrict__ descs, const real *__restrict__ x,
                                                                const real *__restrict__ Cm, const int64_t *__restrict__ roff,
                                                                const int64_t *__restrict__ cpre, int P, int64_t nchunks,
                                                                const int32_t *__restrict__ sorted_item,
                                                                const int32_t *__restrict__ item_query,
                                                                const double *__restrict__ xq,
                                                                typename HyperArgs<PP>::th_t th_arg, int R,
                                                                const int32_t *__restrict__ info,
                                                                const int32_t *__restrict__ tinfo,
                                                                const double *__restrict__ beta, double *__restrict__ G)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t g = (int64_t)xcd_remap((int)blockIdx.x, (int)gridDim.x) * (IG_THREADS / 64) + wave;
    if (g >= nchunks) return;
    const int r = chunk_region(cpre, P, g);
    const int64_t first = roff[r] + (g - cpre[r]) * 16;
    const int count = (int)min((int64_t)16, roff[r + 1] - first);
    const PatchDesc pd = descs[r];
    pmk_kernel_desc th;
    if constexpr (PP) th = th_arg[__builtin_amdgcn_readfirstlane(r)];
    else th = th_arg;
    const int li = lane & 15, lg = lane >> 4;
    real q[D];
    chunk_query_point(first, count, li, sorted_item, item_query, xq, q);
    const real *xs = x + pd.xoff;
    const real *Cb = Cm + pd.yoff * IG_RP + li;
    const int ld = pd.ld, n = pd.n;
    real4_t acc0[D], acc1[D];
#pragma unroll
    for (int d = 0; d < D; ++d)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc0[d][e] = acc1[d][e] = (real)0;
    // k0 < n <= ld and ld is a multiple of 128: k0 + 7 < ld, every load stays inside the patch's padded rows
    for (int k0 = 0; k0 < n; k0 += 8) {
        const int ka = k0 + lg, kb = k0 + 4 + lg;
        real da[D], db[D];
        real sa = (real)0, sb = (real)0;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            da[d] = q[d] - xs[d * ld + ka];
            db[d] = q[d] - xs[d * ld + kb];
            sa += da[d] * da[d];
            sb += db[d] * db[d];
        }
        const real ba = Cb[(int64_t)ka * IG_RP], bb = Cb[(int64_t)kb * IG_RP];
        real ta, tb;
        if constexpr (sizeof(real) == 8) { ta = sqrt_dist(sa); tb = sqrt_dist(sb); }
        else { ta = sqrt(sa); tb = sqrt(sb); }
        // the padding rows (coordinates far away on purpose) are masked to exact zeros
        const real pa = ka < n ? profile_dpsi<FAM, real>(th, ta) : (real)0;
        const real pb = kb < n ? profile_dpsi<FAM, real>(th, tb) : (real)0;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            acc0[d] = mfma_real(ka < n ? pa * da[d] : (real)0, ba, acc0[d]);
            acc1[d] = mfma_real(kb < n ? pb * db[d] : (real)0, bb, acc1[d]);
        }
    }
    if (li >= R) return;
    const bool bad = patch_is_bad(info, tinfo, r);
    const double nan = __builtin_nan("");
    const double *b = beta ? beta + ((int64_t)r * TR_RP + li) * TQ_MAX + 1 : nullptr;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const real4_t acc = acc0[d] + acc1[d];
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
            const int i = frag_irow(lg, qq);
            if (i < count) {
                double v = (double)acc[qq];
                if (b) v = v + b[d];
                G[(first + i) * (int64_t)(D * R) + d + D * li] = bad ? nan : v;
            }
        }
    }
}

// th null: the model's per-patch kernels (the convention of pmk_dispatch.h)
int launch_items_grad(pmk_query *q, const pmk_kernel_desc *th, hipStream_t s)
{
    pmk_model *m = q->m;
    if (q->mchunks == 0) return 0;
    const unsigned grid = (unsigned)((q->mchunks + IG_THREADS / 64 - 1) / (IG_THREADS / 64));
    const bool trend = m->trend_q > 0;
    const double *beta = m->trend_q > 1 ? m->d_tbeta : nullptr;         // q = 1 + D: the linear trend
    const int rc = dispatch_hyper(m, th, [&](auto dd, auto fam, auto pp) {
        hipLaunchKernelGGL((item_grads_kernel<dd(), fam(), pp()>), dim3(grid), dim3(IG_THREADS), 0, s, m->d_desc,
                           (const real *)m->d_x, (const real *)m->d_cm, q->d_roff, q->d_mcpre, (int)m->P, q->mchunks,
                           q->d_sorted_item, q->d_item_query, q->d_xq, hyper_th<pp()>(m, th), q->R_items,
                           (const int32_t *)m->d_info, trend ? (const int32_t *)m->d_tinfo : nullptr, beta, q->d_gm);
        return 0;
    });
    if (rc) return rc;
    PMK_HIP(hipGetLastError());
    return 0;
}

}  // namespace PMK_NS

#ifndef PMK_REAL_F32
// One thread per query; the items in the order of mix_multi_kernel (neighbours in hyperplane order, home last with
// w = 1, t = 0, no plane).  S is mix_multi_kernel's (blend_weight_sum); then, per (c, d), the sum over the items of
// w_i G_{i,d,c} + (u_{i,c} - Y_c) dw_i/dx_d in item order (the home item adds its G alone), divided by S.  u_i - Y_c is
// taken as sum_k w_k (u_i - u_k) / S and never as a difference against the rounded blend: where the patches agree
// (u_i close to Y_c, both far from zero) that difference would carry the rounding of Y_c, not of u_i - Y_c.
// hv, pre: the tree's normals in heap order and the pre-order -> heap permutation (item_plane is a pre-order index).
__global__ __launch_bounds__(256) void mix_grad_kernel(int64_t q0, int64_t q1, int64_t Nq, const int64_t *__restrict__ qoff,
                                                       const double *__restrict__ item_t, const int32_t *__restrict__ item_pos,
                                                       const int32_t *__restrict__ item_plane, const double *__restrict__ U,
                                                       int ldu, int R, int D, const double *__restrict__ G,
                                                       const double *__restrict__ hv, const int32_t *__restrict__ pre,
                                                       pmk_kernel_desc wth, double *__restrict__ dyq)
{
    const int64_t j = q0 + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= q1) return;
    const int64_t b = qoff[j], e = qoff[j + 1];
    const double sw = blend_weight_sum(wth, item_t, b, e);
    for (int col = 0; col < R; ++col) {
        double acc[MAX_D];
        for (int64_t it = b; it < e; ++it) {
            const int64_t pos = item_pos[it];
            const double *gi = G + pos * (int64_t)(D * R) + D * col;
            if (it == e - 1) {                                           // home: w = 1, dw = 0
                for (int d = 0; d < D; ++d) acc[d] = (it == b) ? gi[d] : acc[d] + gi[d];
                break;
            }
            const double t = item_t[it], ui = U[pos * ldu + col];
            const double w = profile(wth, fabs(t));
            const double c = -(profile_dpsi(wth, fabs(t)) * t);          // dw_i/dx_d = c v_d
            double dev = 0.0;                                            // S (u_i - Y) = sum_k w_k (u_i - u_k), k in item order
            for (int64_t k = b; k < e; ++k) {
                const double wk = blend_weight(wth, item_t, k, e);
                dev += wk * (ui - U[(int64_t)item_pos[k] * ldu + col]);
            }
            const double uy = dev / sw;
            const double *v = hv + (int64_t)pre[item_plane[it]] * D;
            for (int d = 0; d < D; ++d) {
                const double term = w * gi[d] + uy * (c * v[d]);
                acc[d] = (it == b) ? term : acc[d] + term;
            }
        }
        for (int d = 0; d < D; ++d) dyq[j + Nq * (d + (int64_t)D * col)] = acc[d] / sw;
    }
}

int launch_mix_grad(pmk_query *q, const pmk_kernel_desc &wth, int64_t q0, int64_t q1, hipStream_t s)
{
    if (q1 <= q0) return 0;
    const pmk_model *m = q->m;
    hipLaunchKernelGGL(mix_grad_kernel, grid256(q1 - q0), dim3(256), 0, s, q0, q1, q->Nq, q->d_qoff,
                       q->d_item_t, q->d_item_pos, q->d_item_plane, q->d_um, q->um_ld, q->R_items, m->D, q->d_gm, m->d_hv,
                       m->d_pre, wth, q->d_dyq);
    PMK_HIP(hipGetLastError());
    return 0;
}
#endif

}  // namespace pmk

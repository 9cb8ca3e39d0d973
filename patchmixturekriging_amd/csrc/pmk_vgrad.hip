// Gradient of the blended variance of the multi-output path (with or without a trend).
//
//   vgrad_strip_kernel      GV[item][d] = d/dx_d of the simple-kriging variance of the item at its query point:
//                           -2 V . W_d with V = L^-1 kq, W_d = L^-1 g_d, g_{d,k} = psi(tau_k) (x_d - z_{k,d}); exactly 0
//                           where the variance is clamped at min_v.  The strip sweep of pmk_predict.hip with D + 1
//                           right-hand sides per item, run through strip_block_row (pmk_strip.h) as pmk_loo.hip does.
//   item_trend_grads_kernel GH[item][a + q d] = (g_d^T C_H)_a: the MFMA of item_grads_kernel (pmk_grad.hip) on the q trend
//                           columns R .. R + q - 1 of the weight block, which that kernel computes and does not store
//   trend_vgrad_kernel      GV[item][d] += 2 z . (L_G^-1 d_d rho), one thread per item (double only)
//   mix_vgrad_kernel        the gradient of Vq = sum_i (w_i / S)^2 v_i, one thread per query (double only)
//
// Layout of a strip.  A wave owns 32 columns, a lane two of them (2 (lane & 15) + c).  Lane (lane & 15) = (D + 1) g + k
// owns component k (0: kq, 1 + d: g_d) of the items 2 g and 2 g + 1 of its wave, so the D + 1 columns of an item lie in
// D + 1 neighbouring lanes of every 16-lane row and an item takes 16 / 10 / 8 / 6 places of a wave at D = 1 / 2 / 3 / 4
// (128 / 80 / 64 / 48 items a strip).  Lanes past the last whole group, and places past the strip's last item, repeat a
// valid item and are never written out.  After the substitution of a block row every lane multiplies its 64 values with
// those of the base lane (k = 0) of its group, fetched by shuffle inside the 16-lane row: the base lane so accumulates
// b = |V|^2, lane k >= 1 accumulates V . W_{k-1}.  The alternative, one pass over the stored strip after the sweep, would
// store the last block row too and read the whole strip once more; the shuffles are 128 a lane and block row beside
// 512 i MFMAs, and no memory traffic.
//
// Bits.  The columns of an MFMA product do not meet, the sums of a column run in block-row, register and lane-group
// order, and nothing passes between waves: the D values of an item do not depend on what shares its strip or on where
// in the strip it sits.  A patch with info != 0, or tinfo != 0 under a trend, gives NaN in all D values of its items.
#include <algorithm>

#include "pmk_dispatch.h"
#include "pmk_items.h"
#include "pmk_strip.h"

namespace pmk {
namespace PMK_NS {

template <int D> struct VgShape {
    static constexpr int COMP = D + 1;                          // columns of an item
    static constexpr int GROUPS = 16 / COMP;                    // lane groups of a 16-lane row
    static constexpr int WITEMS = STRIP_NC * GROUPS;            // items of a wave
    static constexpr int SITEMS = STRIP_WAVES * WITEMS;         // items of a strip
};

// The right-hand-side tile of one block row: eval_tile of pmk_predict.hip (a rolled loop whose results pass through a
// lane-private LDS slot) with phi(tau) in the lanes of component 0 and psi(tau) (q_d - x_d) in those of component 1 + d.
// Rows past the patch's n are exact zeros.
template <int D, int FAM>
__device__ __forceinline__ void vgrad_eval_tile(WaveTile<4, 1> &acc, const real *pt, real2_t *mine, const real *pk,
                                                const pmk_kernel_desc &th, int row0, int n, int k, int lane)
{
    real q[STRIP_NC][D];
#pragma unroll
    for (int c = 0; c < STRIP_NC; ++c)
#pragma unroll
        for (int d = 0; d < D; ++d) q[c][d] = pk[(c * D + d) * STRIP_THREADS];
#pragma unroll
    for (int pi = 0; pi < 4; ++pi) {
#pragma clang loop unroll_count(2)
        for (int sl = 0; sl < 8; ++sl) {
            const int r = 32 * pi + 2 * frag_irow(lane >> 4, sl >> 1) + (sl & 1);     // row within the block row
            real xr[D];
#pragma unroll
            for (int d = 0; d < D; ++d) xr[d] = pt[d * TILE + r];
            const bool inside = row0 + r < n;
            real2_t kv;
#pragma unroll
            for (int c = 0; c < STRIP_NC; ++c) {
                real dd[D], s = (real)0;
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    dd[d] = q[c][d] - xr[d];
                    s += dd[d] * dd[d];
                }
                real dk = dd[0];
#pragma unroll
                for (int d = 1; d < D; ++d) dk = (k == d + 1) ? dd[d] : dk;
                real tau;
                if constexpr (sizeof(real) == 8) tau = sqrt_dist(s);
                else tau = sqrt(s);
                const real val = (k == 0) ? profile<FAM, real>(th, tau) : profile_dpsi<FAM, real>(th, tau) * dk;
                kv[c] = inside ? val : (real)0;
            }
            mine[sl * 64] = kv;
        }
#pragma unroll
        for (int sl = 0; sl < 8; ++sl) {
            const real2_t kv = mine[sl * 64];
#pragma unroll
            for (int c = 0; c < STRIP_NC; ++c) acc.f[2 * pi + (sl & 1)][c][sl >> 1] = kv[c];
        }
    }
}

// Strip g of the launch lies in the region r with spre[r] <= g < spre[r + 1] (strips per region, host prefix) and holds
// the sorted items [first, first + count), first = roff[r] + SITEMS (g - spre[r]).  One barrier per block row: it keeps
// the waves on the same block row of L and publishes the training points of the next one (a ring of two).
template <int D, int FAM, bool PP = false>
__global__ __launch_bounds__(STRIP_THREADS, 2) void vgrad_strip_kernel(const PatchDesc *__restrict__ descs, const real *__restrict__ x,
                                                                     const real *__restrict__ A, const real *__restrict__ inv,
                                                                     const int64_t *__restrict__ roff,
                                                                     const int64_t *__restrict__ spre, int P, int64_t nstrips,
                                                                     const int32_t *__restrict__ sorted_item,
                                                                     const int32_t *__restrict__ item_query,
                                                                     const double *__restrict__ xq, real *__restrict__ strips,
                                                                     int64_t strip_stride, typename HyperArgs<PP>::th_t th_arg,
                                                                     double min_v, const int32_t *__restrict__ info,
                                                                     const int32_t *__restrict__ tinfo, double *__restrict__ GV)
{
    using S = VgShape<D>;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    real *V = strips + (int64_t)blockIdx.x * strip_stride + STRIP_WCOLS * wave;   // this wave's columns, ld = TQ
    constexpr int PTS = MAX_D * TILE;
    __shared__ real pts[2 * PTS];                                   // training points (SoA) of two consecutive block rows
    __shared__ real priv[STRIP_WAVES * 8 * 64 * STRIP_NC];          // lane-private staging of the evaluations
    real2_t *mine = reinterpret_cast<real2_t *>(priv) + (wave * 8) * 64 + lane;
    // the lane's two query points and running products are parked in LDS between the MFMA phases, as in prediction
    __shared__ real park[(STRIP_NC * D + STRIP_NC) * STRIP_THREADS];
    real *pk = park + threadIdx.x;
    const int li = lane & 15;
    const bool used = li < S::GROUPS * S::COMP;
    const int grp = used ? li / S::COMP : 0;
    const int k = used ? li - grp * S::COMP : 0;                    // component of this lane's columns
    const int base = (lane & 48) | (grp * S::COMP);                 // the lane that holds V of the same items

    for (int64_t g = blockIdx.x; g < nstrips; g += gridDim.x) {
        const int r = chunk_region(spre, P, g);
        const int64_t first = roff[r] + (g - spre[r]) * S::SITEMS;
        const int count = (int)min((int64_t)S::SITEMS, roff[r + 1] - first);
        const bool active = S::WITEMS * wave < count;               // wave-uniform
        const PatchDesc pd = descs[r];
        pmk_kernel_desc th;
        if constexpr (PP) th = th_arg[r];
        else th = th_arg;
        const real *Sl = A + pd.aoff;
        const real *xs = x + pd.xoff;
        const int64_t ld = pd.ld;
        auto stage_points = [&](int br, int t) {
            real *dst = pts + (br & 1) * PTS;
#pragma unroll
            for (int d = 0; d < D; ++d) dst[d * TILE + t] = xs[(int64_t)d * ld + br * TILE + t];
        };
#pragma unroll
        for (int c = 0; c < STRIP_NC; ++c) {
            const int e = S::WITEMS * wave + STRIP_NC * grp + c;
            const int64_t qi = item_query[sorted_item[first + (e < count ? e : 0)]];
#pragma unroll
            for (int d = 0; d < D; ++d) pk[(c * D + d) * STRIP_THREADS] = (real)xq[qi * D + d];
            pk[(STRIP_NC * D + c) * STRIP_THREADS] = (real)0;
        }
        // rows of the last block row that are not identity padding, in 32-row pairs
        const int last_pairs = (pd.n - (pd.nt - 1) * TILE + 31) >> 5;

        __syncthreads();                              // every wave is done with the previous task's points
        if (threadIdx.x < TILE) stage_points(0, threadIdx.x);
        for (int i = 0; i < pd.nt; ++i) {
            __syncthreads();                          // block row i - 1 is complete in every wave; points of row i visible
            if (threadIdx.x < TILE && i + 1 < pd.nt) stage_points(i + 1, threadIdx.x);
            if (!active) continue;
            WaveTile<4, 1> acc;
            vgrad_eval_tile<D, FAM>(acc, pts + (i & 1) * PTS, mine, pk, th, i * TILE, pd.n, k, lane);
            // ---- acc -= L[i, 0:i] V_0:i  (the strip holds -V), then acc <- -V_i = -L[ii]^-1 acc
            const real *Li = Sl + (int64_t)i * TILE;
            const real *Lii = Li + (int64_t)i * TILE * ld;
            const real *ninv_i = inv + pd.ioff + (int64_t)i * 4096;
            if (i + 1 == pd.nt && last_pairs == 3) strip_block_row<3>(acc, Li, ld, V, i, Lii, ninv_i, lane);
            else if (i + 1 == pd.nt && last_pairs == 2) strip_block_row<2>(acc, Li, ld, V, i, Lii, ninv_i, lane);
            else if (i + 1 == pd.nt && last_pairs == 1) strip_block_row<1>(acc, Li, ld, V, i, Lii, ninv_i, lane);
            else strip_block_row<4>(acc, Li, ld, V, i, Lii, ninv_i, lane);
            {
                // both factors are negated: the products are those of V and W
                real vs[STRIP_NC];
#pragma unroll
                for (int c = 0; c < STRIP_NC; ++c) vs[c] = pk[(STRIP_NC * D + c) * STRIP_THREADS];
#pragma unroll
                for (int fi = 0; fi < 8; ++fi)
#pragma unroll
                    for (int qq = 0; qq < 4; ++qq)
#pragma unroll
                        for (int c = 0; c < STRIP_NC; ++c) vs[c] += __shfl(acc.f[fi][c][qq], base) * acc.f[fi][c][qq];
#pragma unroll
                for (int c = 0; c < STRIP_NC; ++c) pk[(STRIP_NC * D + c) * STRIP_THREADS] = vs[c];
            }
            if (i + 1 < pd.nt) {
                int srow = tile_i(0, lane, 0);
                asm volatile("" : "+v"(srow));
#pragma unroll
                for (int fi = 0; fi < 8; ++fi)
#pragma unroll
                    for (int qq = 0; qq < 4; ++qq) {
                        const int row = i * TILE + srow + (tile_i(fi, 0, qq) - tile_i(0, 0, 0));
                        real2_t o;
                        o[0] = acc.f[fi][0][qq];
                        o[1] = acc.f[fi][1][qq];
                        __builtin_nontemporal_store(o, reinterpret_cast<real2_t *>(V + (int64_t)row * TQ + 2 * li));
                    }
            }
        }
        // ---- reduce over the four lane groups that share a column; the base lane's sum is b = |V|^2
        const bool bad = patch_is_bad(info, tinfo, r);
#pragma unroll
        for (int c = 0; c < STRIP_NC && active; ++c) {
            real s = pk[(STRIP_NC * D + c) * STRIP_THREADS];
            s += __shfl_xor(s, 16);
            s += __shfl_xor(s, 32);
            const real b = __shfl(s, base);
            const int e = S::WITEMS * wave + STRIP_NC * grp + c;
            if ((lane >> 4) == 0 && used && k >= 1 && e < count) {
                real qe[D];
#pragma unroll
                for (int d = 0; d < D; ++d) qe[d] = pk[(c * D + d) * STRIP_THREADS];
                const real kself = kern_eval<D, FAM, real>(th, qe, qe);
                const double var = (double)kself - (double)b;         // as predict_strip_kernel takes it
                // clamped at min_v: the variance is constant there.  + 0.0: no negative zero
                const double gv = var < min_v ? 0.0 : -2.0 * (double)s + 0.0;
                GV[(first + e) * D + (k - 1)] = bad ? __builtin_nan("") : gv;
            }
        }
        // the next task reuses the strip: order its first stores after this task's last loads
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    }
}

constexpr int IH_THREADS = 256;

// item_grads_kernel (pmk_grad.hip) with another store: the same chunks, operands and MFMAs, and of the 16 columns of
// the weight block the q trend columns C_H (R <= column < R + q) are kept: GH[p][a + q d] = sum_k g_{d,k} C_H[k, a].
template <int D, int FAM, bool PP = false>
__global__ __launch_bounds__(IH_THREADS) void item_trend_grads_kernel(const PatchDesc *__restrict__ descs, const real *__restrict__ x,
                                                                        const real *__restrict__ Cm, const int64_t *__restrict__ roff,
                                                                        const int64_t *__restrict__ cpre, int P, int64_t nchunks,
                                                                        const int32_t *__restrict__ sorted_item,
                                                                        const int32_t *__restrict__ item_query,
                                                                        const double *__restrict__ xq,
                                                                        typename HyperArgs<PP>::th_t th_arg, int R, int qt,
                                                                        double *__restrict__ GH)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t g = (int64_t)xcd_remap((int)blockIdx.x, (int)gridDim.x) * (IH_THREADS / 64) + wave;
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
    const real *Cb = Cm + pd.yoff * TR_RP + li;
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
        const real ba = Cb[(int64_t)ka * TR_RP], bb = Cb[(int64_t)kb * TR_RP];
        real ta, tb;
        if constexpr (sizeof(real) == 8) { ta = sqrt_dist(sa); tb = sqrt_dist(sb); }
        else { ta = sqrt(sa); tb = sqrt(sb); }
        const real pa = ka < n ? profile_dpsi<FAM, real>(th, ta) : (real)0;
        const real pb = kb < n ? profile_dpsi<FAM, real>(th, tb) : (real)0;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            acc0[d] = mfma_real(ka < n ? pa * da[d] : (real)0, ba, acc0[d]);
            acc1[d] = mfma_real(kb < n ? pb * db[d] : (real)0, bb, acc1[d]);
        }
    }
    if (li < R || li >= R + qt) return;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const real4_t acc = acc0[d] + acc1[d];
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
            const int i = frag_irow(lg, qq);
            if (i < count) GH[(first + i) * (int64_t)(D * qt) + (li - R) + qt * d] = (double)acc[qq];
        }
    }
}

// th null: the model's per-patch kernels (the convention of pmk_dispatch.h).  GV: sorted items x D; GH: sorted items x
// (D q), written only under a trend.
int launch_items_vgrad(pmk_query *q, const pmk_kernel_desc *th, hipStream_t s)
{
    pmk_model *m = q->m;
    if (q->vstrips == 0) return 0;
    const int64_t slots = std::min<int64_t>(q->vstrips, (int64_t)m->ctx->num_cu);     // one 8-wave workgroup per CU
    if (int rc = reserve_strips(m, slots)) return rc;
    const bool trend = m->trend_q > 0;
    const int32_t *tinfo = trend ? (const int32_t *)m->d_tinfo : nullptr;
    int rc = dispatch_hyper(m, th, [&](auto dd, auto fam, auto pp) {
        static_assert(VgShape<dd()>::SITEMS == vgrad_strip_items(dd()), "the strip prefix of the host (pmk_internal.h)");
        hipLaunchKernelGGL((vgrad_strip_kernel<dd(), fam(), pp()>), dim3((unsigned)slots), dim3(STRIP_THREADS), 0, s,
                           m->d_desc, (const real *)m->d_x, (const real *)m->d_a, (const real *)m->d_inv, q->d_roff,
                           q->d_vgpre, (int)m->P, q->vstrips, q->d_sorted_item, q->d_item_query, q->d_xq,
                           (real *)m->d_strip, (int64_t)m->max_nt * TILE * TQ, hyper_th<pp()>(m, th), q->min_v,
                           (const int32_t *)m->d_info, tinfo, q->d_gv);
        return 0;
    });
    if (rc) return rc;
    PMK_HIP(hipGetLastError());
    if (!trend) return 0;
    const unsigned grid = (unsigned)((q->mchunks + IH_THREADS / 64 - 1) / (IH_THREADS / 64));
    rc = dispatch_hyper(m, th, [&](auto dd, auto fam, auto pp) {
        hipLaunchKernelGGL((item_trend_grads_kernel<dd(), fam(), pp()>), dim3(grid), dim3(IH_THREADS), 0, s, m->d_desc,
                           (const real *)m->d_x, (const real *)m->d_cm, q->d_roff, q->d_mcpre, (int)m->P, q->mchunks,
                           q->d_sorted_item, q->d_item_query, q->d_xq, hyper_th<pp()>(m, th), q->R_items, m->trend_q,
                           q->d_gh);
        return 0;
    });
    if (rc) return rc;
    PMK_HIP(hipGetLastError());
    return 0;
}

}  // namespace PMK_NS

#ifndef PMK_REAL_F32
// One thread per sorted item p.  Row p of U holds a = kq^T C_H in columns R .. R + q - 1 (item_means_kernel), GH the
// products g_d^T C_H.  Operation order, fixed: rho_a = h_a - a_a and z = L_G^-1 rho as trend_items_kernel takes them;
// per d: (d_d rho)_a = [a == 1 + d] - GH[a + q d] (the constant basis function and a constant trend have no slope),
// y = L_G^-1 d_d rho, t = z . y as an fma chain in a order, GV[d] <- GV[d] + 2 t.
__global__ __launch_bounds__(256) void trend_vgrad_kernel(int64_t total, const int32_t *__restrict__ sorted_item,
                                                          const int32_t *__restrict__ item_region,
                                                          const int32_t *__restrict__ item_query, const double *__restrict__ xq,
                                                          int D, int R, int q, int ld, const double *__restrict__ Lg,
                                                          const double *__restrict__ U, const double *__restrict__ GH,
                                                          double *__restrict__ GV)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= total) return;
    const int32_t it = sorted_item[p];
    const int64_t r = item_region[it], qi = item_query[it];
    const double *row = U + p * ld;
    const double *L = Lg + r * (int64_t)(TQ_MAX * TQ_MAX);
    double z[TQ_MAX], y[TQ_MAX];
    trend_forward(L, q, [&](int a) { return (a == 0 ? 1.0 : xq[qi * D + (a - 1)]) - row[R + a]; }, z);
    const double *gh = GH + p * (int64_t)(D * q);
    for (int d = 0; d < D; ++d) {
        trend_forward(L, q, [&](int a) { return (a == 1 + d ? 1.0 : 0.0) - gh[a + q * d]; }, y);
        double t = 0.0;
        for (int a = 0; a < q; ++a) t = __builtin_fma(z[a], y[a], t);
        GV[p * D + d] = GV[p * D + d] + 2.0 * t;
    }
}

int launch_trend_vgrad(pmk_query *q, hipStream_t s)
{
    const pmk_model *m = q->m;
    if (q->total == 0 || m->trend_q == 0) return 0;
    hipLaunchKernelGGL(trend_vgrad_kernel, grid256(q->total), dim3(256), 0, s, q->total, q->d_sorted_item, q->d_item_region,
                       q->d_item_query, q->d_xq, m->D, q->R_items, m->trend_q, q->um_ld, m->d_tL, q->d_um, q->d_gh, q->d_gv);
    PMK_HIP(hipGetLastError());
    return 0;
}

// One thread per query; items, weights and S as in mix_grad_kernel (pmk_grad.hip).  With wn_i = w_i / S:
//   dVq/dx_d = sum_i [ wn_i^2 GV_{i,d} + 2 wn_i v_i dwn_i ],  dwn_i = (dw_i - wn_i sum_j dw_j) / S,
//   dw_i = c_i v_{plane(i),d}, c_i = -psi_w(|t_i|) t_i for a neighbour, 0 for the home item,
// every sum in item order, the first term taken as it is.
__global__ __launch_bounds__(256) void mix_vgrad_kernel(int64_t q0, int64_t q1, int64_t Nq, const int64_t *__restrict__ qoff,
                                                        const double *__restrict__ item_t, const int32_t *__restrict__ item_pos,
                                                        const int32_t *__restrict__ item_plane, const double *__restrict__ vi,
                                                        int D, const double *__restrict__ GV, const double *__restrict__ hv,
                                                        const int32_t *__restrict__ pre, pmk_kernel_desc wth,
                                                        double *__restrict__ dvq)
{
    const int64_t j = q0 + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= q1) return;
    const int64_t b = qoff[j], e = qoff[j + 1];
    const double sw = blend_weight_sum(wth, item_t, b, e);
    double sdw[MAX_D], acc[MAX_D];
    for (int d = 0; d < D; ++d) sdw[d] = acc[d] = 0.0;
    for (int64_t it = b; it < e - 1; ++it) {                             // the home item (last) has dw = 0
        const double t = item_t[it];
        const double c = -(profile_dpsi(wth, fabs(t)) * t);
        const double *v = hv + (int64_t)pre[item_plane[it]] * D;
        for (int d = 0; d < D; ++d) sdw[d] = (it == b) ? c * v[d] : sdw[d] + c * v[d];
    }
    for (int64_t it = b; it < e; ++it) {
        const int64_t pos = item_pos[it];
        const double wn = blend_weight(wth, item_t, it, e) / sw;
        const double var = vi[pos];
        const double *gv = GV + pos * D;
        double c = 0.0;
        const double *v = nullptr;
        if (it < e - 1) {
            const double t = item_t[it];
            c = -(profile_dpsi(wth, fabs(t)) * t);
            v = hv + (int64_t)pre[item_plane[it]] * D;
        }
        for (int d = 0; d < D; ++d) {
            const double dw = v ? c * v[d] : 0.0;
            const double dwn = (dw - wn * sdw[d]) / sw;
            const double term = (wn * wn) * gv[d] + (2.0 * wn) * (var * dwn);
            acc[d] = (it == b) ? term : acc[d] + term;
        }
    }
    for (int d = 0; d < D; ++d) dvq[j + Nq * d] = acc[d];
}

int launch_mix_vgrad(pmk_query *q, const pmk_kernel_desc &wth, int64_t q0, int64_t q1, hipStream_t s)
{
    if (q1 <= q0) return 0;
    const pmk_model *m = q->m;
    hipLaunchKernelGGL(mix_vgrad_kernel, grid256(q1 - q0), dim3(256), 0, s, q0, q1, q->Nq, q->d_qoff, q->d_item_t,
                       q->d_item_pos, q->d_item_plane, q->d_v, m->D, q->d_gv, m->d_hv, m->d_pre, wth, q->d_dvq);
    PMK_HIP(hipGetLastError());
    return 0;
}
#endif

}  // namespace pmk

// Block kriging (change of support): mean and kriging variance of weighted sums of the blended field over groups of
// queries, on the multi-output path (pmk_query_items_block).
//
// Query j belongs to group[j] (non-decreasing in j) and carries the coefficient a[j].  With w_i = a_{j(i)} wn_i, wn the
// normalised blend weights of pmk_query_mix, the items of one (region r, group f) pair -- an AGGREGATE, a run of the
// sorted item list -- collapse to one right-hand side:
//
//   kbar = sum_i w_i k_r(X_r, x_i)             Vbar = L_r^-1 kbar            (one column of the strip sweep)
//   kappa = sum_{i, i'} w_i w_i' k_r(x_i, x_i') + sum_i w_i^2 addend_{j(i)}  (the addend of pmk_query_set_diag)
//   zbar = sum_i w_i z_i                       (z_i the rows of cov_trend_items_kernel, pmk_cov_trend.hip)
//   s = max(kappa - |Vbar|^2, min_v sum_i w_i^2) + |zbar|^2
//   Var_f = sum_r s_{r, f}                     Mean_f[c] = sum_{items i of f} w_i u_{i, c}
//
// which is a^T Cov a of pmk_query_items_cov_multi + pmk_query_mix_cov by bilinearity, without a buffer of size Nq^2 or
// m_r^2 and with one swept column per aggregate instead of one per item.
//
//   block_weights_kernel    one thread per query: w at each item's sorted position (blend_weight of pmk_items.h)
//   block_heads_kernel      one thread per sorted item: 1 where (region, group) differs from the predecessor's
//   block_compact_kernel    after the scan of the heads: {region, group, first} per aggregate, the aggregate of every item
//   block_counts_kernel     one thread per aggregate: its member count; the first aggregate above the member cap
//   block_region_kernel     one thread per region: its first aggregate (the scan at the region's first item)
//   block_strip_kernel      cov_strip_kernel's task loop and barriers; column c of a strip is an aggregate, the
//                           workspace is the workgroup's strip of reserve_strips, the output |Vbar|^2 per column
//   block_self_kernel       kappa and sum w^2, one wave per aggregate
//   block_reduce_kernel     one thread per group: the R means, and the variance from the pieces of its aggregates
//
// Bits.  An entry of the right-hand-side tile is ONE chain of fused multiply-adds from 0 over the aggregate's members in
// ascending sorted-item order, a lane past its own count adds nothing: a column has the same bits whatever shares its
// wave or strip.  |Vbar|^2 is summed as predict_strip_kernel sums |V|^2.  kappa: lane l of the wave takes the columns
// i' = l, l + 64, .. and in each the rows i = 0 .. i', one chain of fused multiply-adds; the 64 partial sums meet in a
// fixed butterfly.  Everything a group's results depend on is the group's own.
#include <algorithm>

#include "pmk_dispatch.h"
#include "pmk_items.h"
#include "pmk_strip.h"

namespace pmk {
namespace PMK_NS {

// The right-hand-side tile of one block row.  The lane's two columns are the aggregates [first, first + cnt) of sorted
// items with the weights w; mc is the largest count among the wave's columns.  32 rows at a time the partial sums live in
// the lane-private LDS slots of cov_eval_tile (eight slots a lane), so that the member loop is rolled and a member's
// point is fetched four times a block row.  Rows past the patch's n are exact zeros.
template <int D, int FAM>
__device__ __forceinline__ void block_eval_tile(WaveTile<4, 1> &acc, const real *pt, real2_t *mine, const int *ip, int mc,
                                                const int32_t *__restrict__ sorted_item,
                                                const int32_t *__restrict__ item_query, const double *__restrict__ xq,
                                                const double *__restrict__ w, const pmk_kernel_desc &th, int row0, int n,
                                                int lane)
{
    int64_t first[STRIP_NC];
    int cnt[STRIP_NC];
#pragma unroll
    for (int c = 0; c < STRIP_NC; ++c) {
        first[c] = (int64_t)(uint32_t)ip[(2 * c) * STRIP_THREADS];
        cnt[c] = ip[(2 * c + 1) * STRIP_THREADS];
    }
#pragma unroll
    for (int pi = 0; pi < 4; ++pi) {
        const real2_t zero = {(real)0, (real)0};
#pragma unroll
        for (int sl = 0; sl < 8; ++sl) mine[sl * 64] = zero;
        for (int mm = 0; mm < mc; ++mm) {
            real xm[STRIP_NC][D], wm[STRIP_NC];
            bool on[STRIP_NC];
#pragma unroll
            for (int c = 0; c < STRIP_NC; ++c) {
                on[c] = mm < cnt[c];
                const int64_t p = first[c] + (on[c] ? mm : 0);
                const int64_t qi = item_query[sorted_item[p]];
#pragma unroll
                for (int d = 0; d < D; ++d) xm[c][d] = (real)xq[qi * D + d];
                wm[c] = (real)w[p];
            }
#pragma clang loop unroll_count(2)
            for (int sl = 0; sl < 8; ++sl) {
                const int r = 32 * pi + 2 * frag_irow(lane >> 4, sl >> 1) + (sl & 1);     // row within the block row
                real xr[D];
#pragma unroll
                for (int d = 0; d < D; ++d) xr[d] = pt[d * TILE + r];
                const bool inside = row0 + r < n;
                real2_t kv = mine[sl * 64];
#pragma unroll
                for (int c = 0; c < STRIP_NC; ++c)
                    if (inside && on[c]) kv[c] = __builtin_fma(wm[c], kern_eval<D, FAM, real>(th, xm[c], xr), kv[c]);
                mine[sl * 64] = kv;
            }
        }
#pragma unroll
        for (int sl = 0; sl < 8; ++sl) {
            const real2_t kv = mine[sl * 64];
#pragma unroll
            for (int c = 0; c < STRIP_NC; ++c) acc.f[2 * pi + (sl & 1)][c][sl >> 1] = kv[c];
        }
    }
}

// One barrier per block row, as in cov_strip_kernel: it keeps the waves on the same block row of L and publishes the
// training points of the next one (a ring of two).  A wave reads back only the columns it stored itself; the strip is the
// workgroup's own (blockIdx.x), reused by its next task.
template <int D, int FAM, bool PP = false>
__global__ __launch_bounds__(STRIP_THREADS, 2) void block_strip_kernel(const PatchDesc *__restrict__ descs, const real *__restrict__ x,
                                                                     const real *__restrict__ A, const real *__restrict__ inv,
                                                                     const BlockTask *__restrict__ tasks, int64_t ntasks,
                                                                     const BlockAgg *__restrict__ aggs,
                                                                     const int32_t *__restrict__ sorted_item,
                                                                     const int32_t *__restrict__ item_query,
                                                                     const double *__restrict__ xq, const double *__restrict__ w,
                                                                     real *__restrict__ strips, int64_t strip_stride,
                                                                     typename HyperArgs<PP>::th_t th_arg,
                                                                     double *__restrict__ vnorm2)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int PTS = MAX_D * TILE;
    __shared__ real pts[2 * PTS];                                   // training points (SoA) of two consecutive block rows
    __shared__ real priv[STRIP_WAVES * 8 * 64 * STRIP_NC];          // lane-private partial sums of the evaluations
    real2_t *mine = reinterpret_cast<real2_t *>(priv) + (wave * 8) * 64 + lane;
    __shared__ int ipark[2 * STRIP_NC * STRIP_THREADS];             // first member and count of the lane's two columns
    __shared__ real vpark[STRIP_NC * STRIP_THREADS];                // their running |Vbar|^2
    int *ip = ipark + threadIdx.x;
    real *vp = vpark + threadIdx.x;
    real *V = strips + (int64_t)blockIdx.x * strip_stride + STRIP_WCOLS * wave;   // this wave's columns, ld = TQ
    const int li = lane & 15;

    for (int64_t g = blockIdx.x; g < ntasks; g += gridDim.x) {
        const BlockTask tk = tasks[g];
        const bool active = STRIP_WCOLS * wave < tk.count;          // wave-uniform
        const PatchDesc pd = descs[tk.region];
        pmk_kernel_desc th;
        if constexpr (PP) th = th_arg[tk.region];
        else th = th_arg;
        const real *Sl = A + pd.aoff;
        const real *xs = x + pd.xoff;
        const int64_t ld = pd.ld;
        auto stage_points = [&](int br, int t) {
            real *dst = pts + (br & 1) * PTS;
#pragma unroll
            for (int d = 0; d < D; ++d) dst[d * TILE + t] = xs[(int64_t)d * ld + br * TILE + t];
        };
        // the lane's columns: 2 (lane & 15) + c of the wave's; a column past the strip's last aggregate has no member
        int mc = 0;
#pragma unroll
        for (int c = 0; c < STRIP_NC; ++c) {
            const int col = STRIP_WCOLS * wave + 2 * li + c;
            int first = 0, cnt = 0;
            if (col < tk.count) {
                const BlockAgg ag = aggs[tk.first + col];
                first = (int)ag.first;
                cnt = ag.count;
            }
            ip[(2 * c) * STRIP_THREADS] = first;
            ip[(2 * c + 1) * STRIP_THREADS] = cnt;
            vp[c * STRIP_THREADS] = (real)0;
            mc = cnt > mc ? cnt : mc;
        }
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
            const int other = __shfl_xor(mc, o);
            mc = other > mc ? other : mc;
        }
        mc = __builtin_amdgcn_readfirstlane(mc);                    // the same in all 64 lanes: the four row groups share the columns
        // rows of the last block row that are not identity padding, in 32-row pairs
        const int last_pairs = (pd.n - (pd.nt - 1) * TILE + 31) >> 5;

        __syncthreads();                              // every wave is done with the previous task's points
        if (threadIdx.x < TILE) stage_points(0, threadIdx.x);
        for (int i = 0; i < pd.nt; ++i) {
            __syncthreads();                          // block row i - 1 is complete in every wave; points of row i visible
            if (threadIdx.x < TILE && i + 1 < pd.nt) stage_points(i + 1, threadIdx.x);
            if (!active) continue;
            WaveTile<4, 1> acc;
            block_eval_tile<D, FAM>(acc, pts + (i & 1) * PTS, mine, ip, mc, sorted_item, item_query, xq, w, th, i * TILE, pd.n,
                                    lane);
            // ---- acc -= L[i, 0:i] V_0:i  (the strip holds -V), then acc <- -V_i = -L[ii]^-1 acc
            const real *Li = Sl + (int64_t)i * TILE;
            const real *Lii = Li + (int64_t)i * TILE * ld;
            const real *ninv_i = inv + pd.ioff + (int64_t)i * 4096;
            if (i + 1 == pd.nt && last_pairs == 3) strip_block_row<3>(acc, Li, ld, V, i, Lii, ninv_i, lane);
            else if (i + 1 == pd.nt && last_pairs == 2) strip_block_row<2>(acc, Li, ld, V, i, Lii, ninv_i, lane);
            else if (i + 1 == pd.nt && last_pairs == 1) strip_block_row<1>(acc, Li, ld, V, i, Lii, ninv_i, lane);
            else strip_block_row<4>(acc, Li, ld, V, i, Lii, ninv_i, lane);
            {
                real vs[STRIP_NC];
#pragma unroll
                for (int c = 0; c < STRIP_NC; ++c) vs[c] = vp[c * STRIP_THREADS];
#pragma unroll
                for (int fi = 0; fi < 8; ++fi)
#pragma unroll
                    for (int qq = 0; qq < 4; ++qq)
#pragma unroll
                        for (int c = 0; c < STRIP_NC; ++c) vs[c] += acc.f[fi][c][qq] * acc.f[fi][c][qq];
#pragma unroll
                for (int c = 0; c < STRIP_NC; ++c) vp[c * STRIP_THREADS] = vs[c];
            }
            if (i + 1 < pd.nt) {                      // nothing is kept but the block rows a later one reads
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
        // ---- reduce over the four lane groups that share a column, then write |Vbar|^2
#pragma unroll
        for (int c = 0; c < STRIP_NC && active; ++c) {
            real b = vp[c * STRIP_THREADS];
            b += __shfl_xor(b, 16);
            b += __shfl_xor(b, 32);
            const int col = STRIP_WCOLS * wave + 2 * li + c;
            if ((lane >> 4) == 0 && col < tk.count) vnorm2[tk.first + col] = (double)b;
        }
        // the next task reuses the strip: order its first stores after this task's last loads
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    }
}

constexpr int SELF_WAVES = 4;       // aggregates of a workgroup of block_self_kernel

// One wave per aggregate.  kappa = sum over the pairs i <= i' of the members of (i == i' ? 1 : 2) w_i w_i' k(x_i, x_i'),
// plus w_i^2 addend on the diagonal; sw2 = sum w_i^2.  Lane l takes i' = l, l + 64, ...
template <int D, int FAM, bool PP = false>
__global__ __launch_bounds__(64 * SELF_WAVES) void block_self_kernel(const BlockAgg *__restrict__ aggs, int64_t naggs,
                                                                   const int32_t *__restrict__ sorted_item,
                                                                   const int32_t *__restrict__ item_query,
                                                                   const double *__restrict__ xq, const double *__restrict__ w,
                                                                   const double *__restrict__ qdiag,
                                                                   typename HyperArgs<PP>::th_t th_arg,
                                                                   double *__restrict__ kappa, double *__restrict__ sw2)
{
    const int lane = threadIdx.x & 63;
    const int64_t k = (int64_t)blockIdx.x * SELF_WAVES + (threadIdx.x >> 6);
    if (k >= naggs) return;
    const BlockAgg ag = aggs[k];
    pmk_kernel_desc th;
    if constexpr (PP) th = th_arg[ag.region];
    else th = th_arg;
    double s = 0.0, s2 = 0.0;
    for (int b = lane; b < ag.count; b += 64) {
        const int64_t jb = item_query[sorted_item[ag.first + b]];
        const double wb = w[ag.first + b];
        real xb[D];
#pragma unroll
        for (int d = 0; d < D; ++d) xb[d] = (real)xq[jb * D + d];
        for (int a = 0; a <= b; ++a) {
            const int64_t ja = item_query[sorted_item[ag.first + a]];
            real xa[D];
#pragma unroll
            for (int d = 0; d < D; ++d) xa[d] = (real)xq[ja * D + d];
            const double kab = (double)kern_eval<D, FAM, real>(th, xa, xb);
            const double ww = w[ag.first + a] * wb;
            s = __builtin_fma(a == b ? ww : 2.0 * ww, kab, s);
        }
        if (qdiag) s = __builtin_fma(wb * wb, qdiag[jb], s);
        s2 = __builtin_fma(wb, wb, s2);
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        s += __shfl_xor(s, o);
        s2 += __shfl_xor(s2, o);
    }
    if (lane == 0) {
        kappa[k] = s;
        sw2[k] = s2;
    }
}

// th null: the model's per-patch kernels (the convention of pmk_dispatch.h).  The tasks, the aggregates, the weights and
// the pieces are the caller's (pmk_query_items_block); the strips are the model's (reserve_strips).
int launch_items_block(pmk_query *q, const pmk_kernel_desc *th, hipStream_t s)
{
    pmk_model *m = q->m;
    if (q->blk_naggs == 0) return 0;
    const int64_t stride = (int64_t)m->max_nt * TILE * TQ;
    double *kappa = q->d_blk_piece, *vn2 = kappa + q->blk_agg_cap, *sw2 = kappa + 3 * q->blk_agg_cap;
    int rc = dispatch_hyper(m, th, [&](auto dd, auto fam, auto pp) {
        hipLaunchKernelGGL((block_strip_kernel<dd(), fam(), pp()>), dim3((unsigned)q->blk_grid), dim3(STRIP_THREADS), 0, s,
                           m->d_desc, (const real *)m->d_x, (const real *)m->d_a, (const real *)m->d_inv, q->d_blk_tasks,
                           q->blk_ntasks, q->d_blk_aggs, q->d_sorted_item, q->d_item_query, q->d_xq, q->d_blk_w,
                           (real *)m->d_strip, stride, hyper_th<pp()>(m, th), vn2);
        return 0;
    });
    if (rc) return rc;
    PMK_HIP(hipGetLastError());
    rc = dispatch_hyper(m, th, [&](auto dd, auto fam, auto pp) {
        hipLaunchKernelGGL((block_self_kernel<dd(), fam(), pp()>), dim3((unsigned)((q->blk_naggs + SELF_WAVES - 1) / SELF_WAVES)),
                           dim3(64 * SELF_WAVES), 0, s, q->d_blk_aggs, q->blk_naggs, q->d_sorted_item, q->d_item_query, q->d_xq,
                           q->d_blk_w, q->d_qdiag, hyper_th<pp()>(m, th), kappa, sw2);
        return 0;
    });
    if (rc) return rc;
    PMK_HIP(hipGetLastError());
    return 0;
}

}  // namespace PMK_NS

#ifndef PMK_REAL_F32
// w_i = a_j (blend_weight / blend_weight_sum) at the item's sorted position: for a_j = 1 the weight of mix_kernel
__global__ __launch_bounds__(256) void block_weights_kernel(int64_t Nq, const int64_t *__restrict__ qoff,
                                                            const double *__restrict__ item_t,
                                                            const int32_t *__restrict__ item_pos,
                                                            const double *__restrict__ a, pmk_kernel_desc wth,
                                                            double *__restrict__ w)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= Nq) return;
    const int64_t b = qoff[j], e = qoff[j + 1];
    const double sw = blend_weight_sum(wth, item_t, b, e);
    const double aj = a[j];
    for (int64_t it = b; it < e; ++it) w[item_pos[it]] = aj * (blend_weight(wth, item_t, it, e) / sw);
}

__global__ __launch_bounds__(256) void block_heads_kernel(int64_t total, const int32_t *__restrict__ sorted_item,
                                                          const int32_t *__restrict__ item_region,
                                                          const int32_t *__restrict__ item_query,
                                                          const int32_t *__restrict__ group, int32_t *__restrict__ head)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= total) return;
    const int32_t it = sorted_item[p];
    int32_t h = 1;
    if (p > 0) {
        const int32_t pr = sorted_item[p - 1];
        h = item_region[it] != item_region[pr] || group[item_query[it]] != group[item_query[pr]];
    }
    head[p] = h;
}

// scan: the exclusive scan of the heads (total + 1 entries): the aggregate of sorted item p is scan[p + 1] - 1
__global__ __launch_bounds__(256) void block_compact_kernel(int64_t total, const int32_t *__restrict__ sorted_item,
                                                            const int32_t *__restrict__ item_region,
                                                            const int32_t *__restrict__ item_query,
                                                            const int32_t *__restrict__ group, const int32_t *__restrict__ head,
                                                            const int64_t *__restrict__ scan, int32_t region_base,
                                                            BlockAgg *__restrict__ aggs, int32_t *__restrict__ agg_of)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= total) return;
    const int64_t k = scan[p + 1] - 1;
    agg_of[p] = (int32_t)k;
    if (!head[p]) return;
    const int32_t it = sorted_item[p];
    aggs[k].region = item_region[it] - region_base;
    aggs[k].group = group[item_query[it]];
    aggs[k].first = p;
}

// the member counts; *over: the first aggregate with more than cap members (initialised to naggs)
__global__ __launch_bounds__(256) void block_counts_kernel(int64_t naggs, int64_t total, int cap, BlockAgg *__restrict__ aggs,
                                                           unsigned long long *__restrict__ over)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= naggs) return;
    const int64_t cnt = (k + 1 < naggs ? aggs[k + 1].first : total) - aggs[k].first;
    aggs[k].count = (int32_t)cnt;
    aggs[k].pad_ = 0;
    if (cnt > cap) atomicMin(over, (unsigned long long)k);
}

// first aggregate of every region (P + 1 entries): the scan at the region's first sorted item
__global__ __launch_bounds__(256) void block_region_kernel(int64_t P, const int64_t *__restrict__ roff,
                                                           const int64_t *__restrict__ scan, int64_t *__restrict__ aoff)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r <= P) aoff[r] = scan[roff[r]];
}

// One thread per group f: its queries are gq[f] .. gq[f + 1] - 1, its items qoff[gq[f]] .. qoff[gq[f + 1]] - 1 in item
// order.  Mean[c] is a chain of fused multiply-adds of w_i u_{i, c} from 0; Var adds s of an aggregate at the item that is
// its head.  zbar_k is a chain over the aggregate's members in sorted order, |zbar|^2 a chain over k.  Vb null: the
// variance is not wanted and no piece is read.
__global__ __launch_bounds__(256) void block_reduce_kernel(int64_t F, const int64_t *__restrict__ gq,
                                                           const int64_t *__restrict__ qoff,
                                                           const int32_t *__restrict__ item_pos,
                                                           const int32_t *__restrict__ item_region, int32_t region_base,
                                                           const double *__restrict__ w, const double *__restrict__ U, int ldu,
                                                           int R, const int32_t *__restrict__ head,
                                                           const int32_t *__restrict__ agg_of, const BlockAgg *__restrict__ aggs,
                                                           const double *__restrict__ kappa, const double *__restrict__ vn2,
                                                           double *__restrict__ zn2, const double *__restrict__ sw2,
                                                           const double *__restrict__ Z, int q, double min_v,
                                                           const int32_t *__restrict__ info, const int32_t *__restrict__ tinfo,
                                                           double *__restrict__ Yb, double *__restrict__ Vb)
{
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const int64_t b = qoff[gq[f]], e = qoff[gq[f + 1]];
    double mean[TR_RP];
#pragma unroll
    for (int c = 0; c < TR_RP; ++c) mean[c] = 0.0;
    double var = 0.0;
    bool bad = false;
    for (int64_t it = b; it < e; ++it) {
        const int64_t pos = item_pos[it];
        const double wi = w[pos];
        bad = bad || patch_is_bad(info, tinfo, item_region[it] - region_base);
        const double *row = U + pos * ldu;
#pragma unroll
        for (int c = 0; c < TR_RP; ++c)
            if (c < R) mean[c] = __builtin_fma(wi, row[c], mean[c]);
        if (!Vb || !head[pos]) continue;
        const int64_t k = agg_of[pos];
        double t = 0.0;
        if (q > 0) {
            const BlockAgg ag = aggs[k];
            double zb[TQ_MAX];
#pragma unroll
            for (int a = 0; a < TQ_MAX; ++a) zb[a] = 0.0;
            for (int mm = 0; mm < ag.count; ++mm) {
                const double wm = w[ag.first + mm];
                const double *z = Z + (ag.first + mm) * TQ_MAX;
#pragma unroll
                for (int a = 0; a < TQ_MAX; ++a)
                    if (a < q) zb[a] = __builtin_fma(wm, z[a], zb[a]);
            }
#pragma unroll
            for (int a = 0; a < TQ_MAX; ++a)
                if (a < q) t = __builtin_fma(zb[a], zb[a], t);
        }
        zn2[k] = t;
        double s = kappa[k] - vn2[k];
        const double floor_ = min_v * sw2[k];
        s = s < floor_ ? floor_ : s;
        var += s + t;
    }
#pragma unroll
    for (int c = 0; c < TR_RP; ++c)
        if (c < R) Yb[c * F + f] = bad ? __builtin_nan("") : mean[c];
    if (Vb) Vb[f] = bad ? __builtin_nan("") : var;
}

int launch_block_weights(pmk_query *q, const pmk_kernel_desc &wth, hipStream_t s)
{
    if (q->Nq == 0) return 0;
    hipLaunchKernelGGL(block_weights_kernel, grid256(q->Nq), dim3(256), 0, s, q->Nq, q->d_qoff, q->d_item_t, q->d_item_pos,
                       q->d_blk_a, wth, q->d_blk_w);
    PMK_HIP(hipGetLastError());
    return 0;
}

// heads and their scan; the number of aggregates is then scan[total]
int launch_block_heads(pmk_query *q, hipStream_t s)
{
    hipLaunchKernelGGL(block_heads_kernel, grid256(q->total), dim3(256), 0, s, q->total, q->d_sorted_item, q->d_item_region,
                       q->d_item_query, q->d_blk_group, q->d_blk_head);
    PMK_HIP(hipGetLastError());
    if (exclusive_scan_i32_to_i64(q->d_blk_head, q->d_blk_scan, q->total, &q->d_tmp, &q->tmp_bytes, s)) {
        set_error("pmk_query_items_block: prefix scan failed");
        return -100;
    }
    return 0;
}

// after the aggregates' count is known and d_blk_aggs holds that many: the list, the counts (d_over: see
// block_counts_kernel) and the regions' first aggregates
int launch_block_aggregates(pmk_query *q, int cap, unsigned long long *d_over, int64_t *d_aoff, hipStream_t s)
{
    const pmk_model *m = q->m;
    hipLaunchKernelGGL(block_compact_kernel, grid256(q->total), dim3(256), 0, s, q->total, q->d_sorted_item, q->d_item_region,
                       q->d_item_query, q->d_blk_group, q->d_blk_head, q->d_blk_scan, (int32_t)m->leaf_base, q->d_blk_aggs,
                       q->d_blk_agg_of);
    PMK_HIP(hipGetLastError());
    hipLaunchKernelGGL(block_counts_kernel, grid256(q->blk_naggs), dim3(256), 0, s, q->blk_naggs, q->total, cap, q->d_blk_aggs,
                       d_over);
    PMK_HIP(hipGetLastError());
    hipLaunchKernelGGL(block_region_kernel, grid256(m->P + 1), dim3(256), 0, s, m->P, q->d_roff + m->leaf_base, q->d_blk_scan,
                       d_aoff);
    PMK_HIP(hipGetLastError());
    return 0;
}

int launch_block_reduce(pmk_query *q, bool want_var, int qt, hipStream_t s)
{
    if (q->blk_F == 0) return 0;
    const pmk_model *m = q->m;
    double *kappa = q->d_blk_piece, *vn2 = kappa + q->blk_agg_cap, *zn2 = kappa + 2 * q->blk_agg_cap,
           *sw2 = kappa + 3 * q->blk_agg_cap;
    hipLaunchKernelGGL(block_reduce_kernel, grid256(q->blk_F), dim3(256), 0, s, q->blk_F, q->d_blk_gq, q->d_qoff, q->d_item_pos,
                       q->d_item_region, (int32_t)m->leaf_base, q->d_blk_w, q->d_um, q->um_ld, q->R_items, q->d_blk_head,
                       q->d_blk_agg_of, q->d_blk_aggs, kappa, vn2, zn2, sw2, q->d_cov_z, qt, q->min_v,
                       (const int32_t *)m->d_info, qt > 0 ? (const int32_t *)m->d_tinfo : nullptr, q->d_blk_y,
                       want_var ? q->d_blk_v : nullptr);
    PMK_HIP(hipGetLastError());
    return 0;
}
#endif

}  // namespace pmk

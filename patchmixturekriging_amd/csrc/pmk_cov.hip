// Joint posterior covariance of a query batch under the blend (single-output path, no trend).
//
//   Cov[j, j'] = sum over the regions r that hold an item of both j and j':
//                wn_{r,j} wn_{r,j'} ( k_r(x_j, x_j') - V_{r,j} . V_{r,j'} ),   V_{r,j} = L_r^-1 k_r(X_r, x_j),
//   wn the normalised weights of pmk_query_mix.  For j = j' this is Vq = sum wn^2 v.
//
//   cov_strip_kernel   the strip sweep of pmk_predict.hip through strip_block_row (pmk_strip.h), one right-hand side per
//                      item, that keeps -V: every block row, the last one included, goes to the V ARENA, which has one
//                      strip per task (ld x TQ elements, leading dimension TQ, at CovTask::voff), not one per workgroup
//   cov_gram_kernel    G_r[a, b] = sum_rows V_a[row] V_b[row] for every pair of strips of a region, on the MFMA, into the
//                      region's m_r x m_r block of doubles (the two negations cancel)
//   cov_block_kernel   S_r = k_r(x_a, x_b) - G_r in place; the diagonal takes the addend of pmk_query_set_diag and the
//                      clamp at min_v as predict_strip_kernel applies them, off-diagonal entries are not clamped
//   mix_cov_kernel     the blend in gather form: one thread per entry (j, j'), j <= j', no atomics (double only)
//
// The arena.  A task's strip has all ld = 128 nt rows of its patch.  The waves that hold items store all 128 rows of
// every block row: rows past n are exact zeros (the right-hand side is zero there and the factor's padding is the
// identity), so nothing of an earlier plan survives in a column that the Gram reads for a result.  The columns of the
// waves past a strip's last item are never written and those past the last item of a written wave repeat item 0: the
// Gram multiplies them (the columns of an MFMA product do not meet) and stores none of them.
//
// Bits.  Entry (a, b) of G_r is one chain of 16x16x4 MFMAs over the rows 0 .. ld - 1 in steps of four, whatever the
// columns' places in their strips and whatever shares the tiles; the lower triangle is a copy of the upper one.  The
// blend sums over the shared regions in ascending region index, whichever query comes first.  Nothing is accumulated
// across threads.
#include <algorithm>

#include "pmk_dispatch.h"
#include "pmk_items.h"
#include "pmk_strip.h"

namespace pmk {
namespace PMK_NS {

// The right-hand-side tile of one block row: eval_tile of pmk_predict.hip (a rolled loop whose results pass through a
// lane-private LDS slot) without the mean.  Rows past the patch's n are exact zeros for every family.
template <int D, int FAM>
__device__ __forceinline__ void cov_eval_tile(WaveTile<4, 1> &acc, const real *pt, real2_t *mine, const real *pk,
                                              const pmk_kernel_desc &th, int row0, int n, int lane)
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
            for (int c = 0; c < STRIP_NC; ++c) kv[c] = inside ? kern_eval<D, FAM, real>(th, q[c], xr) : (real)0;
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

// One barrier per block row: it keeps the waves on the same block row of L and publishes the training points of the
// next one (a ring of two), as in vgrad_strip_kernel.  A wave reads back only the columns it stored itself.
template <int D, int FAM, bool PP = false>
__global__ __launch_bounds__(STRIP_THREADS, 2) void cov_strip_kernel(const PatchDesc *__restrict__ descs, const real *__restrict__ x,
                                                                   const real *__restrict__ A, const real *__restrict__ inv,
                                                                   const CovTask *__restrict__ tasks, int64_t ntasks,
                                                                   const int32_t *__restrict__ sorted_item,
                                                                   const int32_t *__restrict__ item_query,
                                                                   const double *__restrict__ xq, real *__restrict__ arena,
                                                                   typename HyperArgs<PP>::th_t th_arg)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int PTS = MAX_D * TILE;
    __shared__ real pts[2 * PTS];                                   // training points (SoA) of two consecutive block rows
    __shared__ real priv[STRIP_WAVES * 8 * 64 * STRIP_NC];          // lane-private staging of the evaluations
    real2_t *mine = reinterpret_cast<real2_t *>(priv) + (wave * 8) * 64 + lane;
    __shared__ real park[STRIP_NC * D * STRIP_THREADS];             // the lane's two query points
    real *pk = park + threadIdx.x;
    const int li = lane & 15;

    for (int64_t g = blockIdx.x; g < ntasks; g += gridDim.x) {
        const CovTask tk = tasks[g];
        real *V = arena + tk.voff + STRIP_WCOLS * wave;             // this wave's columns of the task's strip, ld = TQ
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
        // the lane's columns: 2 (lane & 15) + c of the wave's; columns past the strip's last item repeat item 0
#pragma unroll
        for (int c = 0; c < STRIP_NC; ++c) {
            const int col = STRIP_WCOLS * wave + 2 * li + c;
            const int64_t qi = item_query[sorted_item[tk.first + (col < tk.count ? col : 0)]];
#pragma unroll
            for (int d = 0; d < D; ++d) pk[(c * D + d) * STRIP_THREADS] = (real)xq[qi * D + d];
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
            cov_eval_tile<D, FAM>(acc, pts + (i & 1) * PTS, mine, pk, th, i * TILE, pd.n, lane);
            // ---- acc -= L[i, 0:i] V_0:i  (the strip holds -V), then acc <- -V_i = -L[ii]^-1 acc
            const real *Li = Sl + (int64_t)i * TILE;
            const real *Lii = Li + (int64_t)i * TILE * ld;
            const real *ninv_i = inv + pd.ioff + (int64_t)i * 4096;
            if (i + 1 == pd.nt && last_pairs == 3) strip_block_row<3>(acc, Li, ld, V, i, Lii, ninv_i, lane);
            else if (i + 1 == pd.nt && last_pairs == 2) strip_block_row<2>(acc, Li, ld, V, i, Lii, ninv_i, lane);
            else if (i + 1 == pd.nt && last_pairs == 1) strip_block_row<1>(acc, Li, ld, V, i, Lii, ninv_i, lane);
            else strip_block_row<4>(acc, Li, ld, V, i, Lii, ninv_i, lane);
            // every block row is kept, the last one too: the Gram reads all ld rows
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
}

constexpr int GRAM_THREADS = 256;   // four waves, each a 32 x 32 piece of a 64 x 64 piece of the pair's 256 x 256 tile
constexpr int GRAM_PIECES = (TQ / 64) * (TQ / 64);

// blockIdx.x: a pair (ta <= tb) of strips of one region, blockIdx.y: a 64 x 64 piece of its tile.  A wave multiplies the
// columns [a0, a0 + 32) of strip ta with the columns [b0, b0 + 32) of strip tb: lane l supplies V[row k0 + (l >> 4)] of
// column (l & 15) of each 16-column fragment, straight from the arena (16 consecutive elements per row and fragment).
// Entry (a, b) is ONE accumulator register, updated by the MFMAs of k0 = 0, 4, ..., ld - 4 in that order.
__global__ __launch_bounds__(GRAM_THREADS) void cov_gram_kernel(const PatchDesc *__restrict__ descs,
                                                                const CovTask *__restrict__ tasks,
                                                                const CovPair *__restrict__ pairs,
                                                                const real *__restrict__ arena, double *__restrict__ G)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const CovPair pr = pairs[blockIdx.x];
    const CovTask ta = tasks[pr.ta], tb = tasks[pr.tb];
    const int a0 = 64 * ((int)blockIdx.y / (TQ / 64)) + 32 * (wave >> 1);
    const int b0 = 64 * ((int)blockIdx.y % (TQ / 64)) + 32 * (wave & 1);
    if (a0 >= ta.count || b0 >= tb.count) return;
    if (pr.ta == pr.tb && b0 + 32 <= a0) return;           // strictly below the diagonal: mirrored from above
    const int li = lane & 15, lg = lane >> 4;
    const int rows = descs[ta.region].nt * TILE;           // the rows the strip kernel wrote: the active block rows
    const real *pa = arena + ta.voff + (int64_t)lg * TQ + a0 + li;
    const real *pb = arena + tb.voff + (int64_t)lg * TQ + b0 + li;
    real4_t acc[2][2];
#pragma unroll
    for (int ia = 0; ia < 2; ++ia)
#pragma unroll
        for (int ib = 0; ib < 2; ++ib) acc[ia][ib] = real4_t{0, 0, 0, 0};
    // rows is a multiple of 128: four k-steps a pass, their sixteen loads issued ahead of the MFMAs
    for (int k0 = 0; k0 < rows; k0 += 16) {
        real va[4][2], vb[4][2];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int f = 0; f < 2; ++f) {
                va[u][f] = pa[(int64_t)(k0 + 4 * u) * TQ + 16 * f];
                vb[u][f] = pb[(int64_t)(k0 + 4 * u) * TQ + 16 * f];
            }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int ia = 0; ia < 2; ++ia)
#pragma unroll
                for (int ib = 0; ib < 2; ++ib) acc[ia][ib] = mfma_real(va[u][ia], vb[u][ib], acc[ia][ib]);
    }
    double *Gr = G + ta.goff;
    const int64_t m = ta.m;
#pragma unroll
    for (int ia = 0; ia < 2; ++ia)
#pragma unroll
        for (int ib = 0; ib < 2; ++ib)
#pragma unroll
            for (int qq = 0; qq < 4; ++qq) {
                const int a = a0 + 16 * ia + frag_irow(lg, qq), b = b0 + 16 * ib + li;
                if (a >= ta.count || b >= tb.count) continue;
                const int64_t ra = ta.a0 + a, rb = tb.a0 + b;       // places in the region's sorted segment
                if (ra > rb) continue;
                const double v = (double)acc[ia][ib][qq];
                Gr[ra + m * rb] = v;
                Gr[rb + m * ra] = v;
            }
}

constexpr int BLOCK_SLICES = 16;    // workgroups that share the entries of one pair's tile

// blockIdx.x: a pair of strips, as in the Gram; its entries (a, b) with a <= b in the region's order are dealt over
// gridDim.y workgroups.  The kernel value of (a, b) is evaluated once and stored on both sides of the diagonal.
template <int D, int FAM, bool PP = false>
__global__ __launch_bounds__(256) void cov_block_kernel(const CovTask *__restrict__ tasks, const CovPair *__restrict__ pairs,
                                                        const int32_t *__restrict__ sorted_item,
                                                        const int32_t *__restrict__ item_query,
                                                        const double *__restrict__ xq, const double *__restrict__ qdiag,
                                                        typename HyperArgs<PP>::th_t th_arg, double min_v,
                                                        const int32_t *__restrict__ info, double *__restrict__ G)
{
    const CovPair pr = pairs[blockIdx.x];
    const CovTask ta = tasks[pr.ta], tb = tasks[pr.tb];
    pmk_kernel_desc th;
    if constexpr (PP) th = th_arg[ta.region];
    else th = th_arg;
    const bool bad = patch_is_bad(info, nullptr, ta.region);
    double *Gr = G + ta.goff;
    const int64_t m = ta.m;
    const int total = ta.count * tb.count;
    for (int e = (int)blockIdx.y * 256 + (int)threadIdx.x; e < total; e += (int)gridDim.y * 256) {
        const int a = e % ta.count, b = e / ta.count;
        const int64_t ra = ta.a0 + a, rb = tb.a0 + b;
        if (ra > rb) continue;
        const int64_t ja = item_query[sorted_item[ta.first + a]], jb = item_query[sorted_item[tb.first + b]];
        real xa[D], xb[D];
#pragma unroll
        for (int d = 0; d < D; ++d) {
            xa[d] = (real)xq[ja * D + d];
            xb[d] = (real)xq[jb * D + d];
        }
        const double kab = (double)kern_eval<D, FAM, real>(th, xa, xb);
        double s;
        if (ra == rb) {
            // as predict_strip_kernel takes the variance
            s = kab - Gr[ra + m * ra];
            if (qdiag) s = (kab + qdiag[ja]) - Gr[ra + m * ra];
            s = s < min_v ? min_v : s;
        } else {
            s = kab - Gr[ra + m * rb];
        }
        if (bad) s = __builtin_nan("");
        Gr[ra + m * rb] = s;
        Gr[rb + m * ra] = s;
    }
}

// th null: the model's per-patch kernels (the convention of pmk_dispatch.h).  The tasks, the pairs and the buffers are
// the caller's (pmk_query_items_cov).
int launch_items_cov(pmk_query *q, const pmk_kernel_desc *th, hipStream_t s)
{
    pmk_model *m = q->m;
    if (q->cov_ntasks == 0) return 0;
    const int64_t slots = std::min<int64_t>(q->cov_ntasks, (int64_t)m->ctx->num_cu);   // one 8-wave workgroup per CU
    int rc = dispatch_hyper(m, th, [&](auto dd, auto fam, auto pp) {
        hipLaunchKernelGGL((cov_strip_kernel<dd(), fam(), pp()>), dim3((unsigned)slots), dim3(STRIP_THREADS), 0, s, m->d_desc,
                           (const real *)m->d_x, (const real *)m->d_a, (const real *)m->d_inv, q->d_cov_tasks, q->cov_ntasks,
                           q->d_sorted_item, q->d_item_query, q->d_xq, (real *)q->d_cov_v, hyper_th<pp()>(m, th));
        return 0;
    });
    if (rc) return rc;
    PMK_HIP(hipGetLastError());
    hipLaunchKernelGGL(cov_gram_kernel, dim3((unsigned)q->cov_npairs, GRAM_PIECES), dim3(GRAM_THREADS), 0, s, m->d_desc,
                       q->d_cov_tasks, q->d_cov_pairs, (const real *)q->d_cov_v, q->d_cov_s);
    PMK_HIP(hipGetLastError());
    rc = dispatch_hyper(m, th, [&](auto dd, auto fam, auto pp) {
        hipLaunchKernelGGL((cov_block_kernel<dd(), fam(), pp()>), dim3((unsigned)q->cov_npairs, BLOCK_SLICES), dim3(256), 0, s,
                           q->d_cov_tasks, q->d_cov_pairs, q->d_sorted_item, q->d_item_query, q->d_xq, q->d_qdiag,
                           hyper_th<pp()>(m, th), q->min_v, (const int32_t *)m->d_info, q->d_cov_s);
        return 0;
    });
    if (rc) return rc;
    PMK_HIP(hipGetLastError());
    return 0;
}

}  // namespace PMK_NS

#ifndef PMK_REAL_F32
constexpr int MIXC = 16;    // a workgroup blends a 16 x 16 tile of the result

// Workgroup (bx, by), bx <= by, computes the entries (j, j') of the tile rows 16 bx .. and columns 16 by .. with j <= j'
// and writes the tile and its mirror image, both with j along the lanes (the result is column-major).  For every region
// of j, in ascending region index, the items of j and of j' in that region are looked for in their order (item lists
// are short); an item's place in the region's sorted segment is item_pos - roff[region].  The neighbour search can accept one
// leaf through two hyperplanes, so a query may hold two items of a region: every pair of items of the two queries that
// share a region is a term, which is the covariance of the two blends as they are.  A query that blends an item of a
// failed patch is NaN in its whole row and column, also where the two queries share no region; other entries without a
// shared region are +0.
__global__ __launch_bounds__(MIXC *MIXC) void mix_cov_kernel(int64_t Nq, const int64_t *__restrict__ qoff,
                                                             const double *__restrict__ item_t,
                                                             const int32_t *__restrict__ item_region,
                                                             const int32_t *__restrict__ item_pos,
                                                             const int64_t *__restrict__ roff,
                                                             const int64_t *__restrict__ goff, const double *__restrict__ S,
                                                             const int32_t *__restrict__ info, pmk_kernel_desc wth,
                                                             double *__restrict__ cov)
{
    if (blockIdx.x > blockIdx.y) return;
    __shared__ double tile[MIXC][MIXC + 1];
    const int tx = threadIdx.x & (MIXC - 1), ty = threadIdx.x / MIXC;
    const int64_t j = (int64_t)blockIdx.x * MIXC + tx, jp = (int64_t)blockIdx.y * MIXC + ty;
    double acc = 0.0;
    if (j < Nq && jp < Nq && j <= jp) {
        const int64_t b = qoff[j], e = qoff[j + 1], bp = qoff[jp], ep = qoff[jp + 1];
        const double sw = blend_weight_sum(wth, item_t, b, e), swp = blend_weight_sum(wth, item_t, bp, ep);
        bool bad = false;
        for (int64_t it = bp; it < ep; ++it) bad = bad || patch_is_bad(info, nullptr, item_region[it]);
        // one term: the pair (it, ip) of items of j and j' in region r, added to the chain a (n: terms before it)
        auto add_term = [&](int64_t it, int64_t ip, int32_t r, double a, int n) {
            const double wn = blend_weight(wth, item_t, it, e) / sw, wnp = blend_weight(wth, item_t, ip, ep) / swp;
            const int64_t m = roff[r + 1] - roff[r];
            const double s = S[goff[r] + (item_pos[it] - roff[r]) + m * (item_pos[ip] - roff[r])];
            return n == 0 ? (wn * wnp) * s : __builtin_fma(wn * wnp, s, a);
        };
        // The sum of an entry is a chain of fused multiply-adds over its terms in ASCENDING region index, so that it does
        // not depend on which of its two queries has the lower index: two queries at one point have equal rows, and a
        // sub-batch in any order keeps the bits of its entries.  The items of j are walked in their own order first;
        // nearly every entry has at most one term or meets its regions in ascending order, and is done.
        int nterm = 0;
        int32_t last = -1;
        bool ascending = true;
        for (int64_t it = b; it < e; ++it) {
            const int32_t r = item_region[it];
            bad = bad || patch_is_bad(info, nullptr, r);
            for (int64_t ip = bp; ip < ep; ++ip) {
                if (item_region[ip] != r) continue;
                acc = add_term(it, ip, r, acc, nterm);
                ++nterm;
                ascending = ascending && r >= last;
                last = r;
            }
        }
        if (nterm >= 2 && !ascending) {
            nterm = 0;
            for (int32_t prev = -1;;) {
                int32_t r = INT32_MAX;
                for (int64_t it = b; it < e; ++it) {
                    const int32_t rr = item_region[it];
                    if (rr > prev && rr < r) r = rr;
                }
                if (r == INT32_MAX) break;
                prev = r;
                for (int64_t it = b; it < e; ++it) {
                    if (item_region[it] != r) continue;
                    for (int64_t ip = bp; ip < ep; ++ip)
                        if (item_region[ip] == r) acc = add_term(it, ip, r, acc, nterm++);
                }
            }
        }
        if (bad) acc = __builtin_nan("");
    }
    tile[ty][tx] = acc;
    __syncthreads();
    if (blockIdx.x == blockIdx.y) {
        if (j < Nq && jp < Nq) cov[j + Nq * jp] = tx <= ty ? tile[ty][tx] : tile[tx][ty];
        return;
    }
    if (j < Nq && jp < Nq) cov[j + Nq * jp] = tile[ty][tx];
    // the mirror image: row jm of the tile's columns, column jc of its rows
    const int64_t jm = (int64_t)blockIdx.y * MIXC + tx, jc = (int64_t)blockIdx.x * MIXC + ty;
    if (jm < Nq && jc < Nq) cov[jm + Nq * jc] = tile[tx][ty];
}

int launch_mix_cov(pmk_query *q, const pmk_kernel_desc &wth, hipStream_t s)
{
    if (q->Nq == 0) return 0;
    const pmk_model *m = q->m;
    const unsigned nt = (unsigned)((q->Nq + MIXC - 1) / MIXC);
    // blocks with a trend's term: a patch whose trend is flagged marks its queries as one whose factorisation failed does
    const int32_t *info = q->cov_trend_q > 0 ? q->d_cov_flags : (const int32_t *)m->d_info;
    hipLaunchKernelGGL(mix_cov_kernel, dim3(nt, nt), dim3(MIXC * MIXC), 0, s, q->Nq, q->d_qoff, q->d_item_t, q->d_item_region,
                       q->d_item_pos, q->d_roff, q->d_cov_goff, q->d_cov_s, info, wth, q->d_cov);
    PMK_HIP(hipGetLastError());
    return 0;
}
#endif

}  // namespace pmk

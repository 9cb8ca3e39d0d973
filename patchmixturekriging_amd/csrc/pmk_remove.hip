// Row deletion from the Cholesky factor: m points removed from a fitted patch in place (pmk_model_remove).
//
// The rows r_1 < ... < r_m leave, k0 = r_1, n' = n - m, t = n' - k0.  L~ = L[keep, :] (n' x n) satisfies L~ L~^T = U[keep, keep]
// and L~ z = y[keep]; its first k0 rows are those of L.  New row k0 + j of the trailing block B = L[keep >= k0, k0 : n] is the
// old row k0 + j + s_j, s_j = #{removed rows before it} (1 <= s_j <= m, non-decreasing), and ends at column j + s_j.  One
// Householder reflector per new column j, of length s_j + 1 on the columns j .. j + s_j, made from row j (v = x + sign(x_0)|x| e_0,
// then the column's sign flipped: the diagonal is +|x|), zeroes that row right of its diagonal; it is applied to every row
// below and to z^T[k0:], which is indexed by COLUMNS and therefore does not move with the rows: B Q = [L'_22 0] and
// z' = (Q^T z)[:t].  The fill of a lower row stays inside its own span because s does not decrease.
//
// remove_rows_kernel, one workgroup per patch that loses rows:
//   1. moves the rows >= k0 of the slab (columns < n), of the coordinates, of y and of the addends up by s: top to bottom in
//      chunks of 64 rows, a chunk read completely, then a barrier, then written (a row is read at a + s_a and written at a);
//   2. sweeps the trailing block in blocks of RM_NB new columns.  A row's segment of RM_NB + m columns is staged once per
//      block in LDS, one thread per row (the row z^T is the last one).  The block's own rows make their reflectors one after
//      another, a barrier per reflector, each applied at once to the staged rows below; every later chunk of 256 rows takes
//      the block's reflectors from LDS without a barrier;
//   3. a new diagonal that is <= 0 or NaN is replaced by 1 and recorded once: info = k0 + j + 1 if info was 0 (an info
//      that was set stays set, lowered to n' if it named a row past it);
//   4. restores the padding of the rows and columns n' .. n - 1 (identity in the slab, 1e300 in x, zeros in y, z, c and the
//      addends) and inverts anew the 32 x 32 diagonal blocks k0 / 32 .. (n - 1) / 32 (the arithmetic of ninv_from_slab_kernel);
//   5. writes n' into the device PatchDesc last.
// Rows and columns < k0 of the slab, z below k0 and the -D^-1 blocks before k0 / 32 are not written.  c = L'^-T z' is the
// caller's launch_backsolve.  No trip count depends on the data; NaN only propagates.
#include "pmk_real.h"

namespace pmk {
namespace PMK_NS {

constexpr int RM_THREADS = 256;
constexpr int RM_NB = 32;                           // new columns (reflectors) per block
constexpr int RM_MAXM = PMK_REMOVE_MAX_ROWS;        // rows one patch can lose in one call: a reflector has at most RM_MAXM + 1 entries
constexpr int RM_W = RM_NB + RM_MAXM;               // columns of a staged row segment
constexpr int RM_LDI = RM_W + 1;                    // its leading dimension (odd: a thread walks its own row)
constexpr int RM_LDV = RM_MAXM + 1;                 // leading dimension of the block's reflectors
constexpr int RM_SB = 32;                           // edge of a -D^-1 block
constexpr int RM_RC = 64, RM_CU = 8;                // compaction: rows of a chunk, columns in flight per thread
// the image (256 rows x 65), the reflectors (32 x 33), their beta and sign: 139.5 KiB in fp64
constexpr size_t RM_LDS_BYTES = sizeof(real) * (size_t)(RM_THREADS * RM_LDI + RM_NB * RM_LDV + 2 * RM_NB);

#ifdef PMK_REAL_F32
__device__ __forceinline__ real rm_sqrt(real v) { return sqrtf(v); }
#else
__device__ __forceinline__ real rm_sqrt(real v) { return sqrt(v); }
#endif

// s of the new row a (patch index): the removed rows before it.  rem ascends, so rem[i] - i (the kept rows before rem[i])
// does not decrease
__device__ __forceinline__ int rm_shift(const int *rem, int m, int a)
{
    int s = 0;
    for (int i = 0; i < m; ++i) s += (rem[i] - i <= a) ? 1 : 0;
    return s;
}

// new row a of [k0, n1) takes the old row a + s_a in `ncols` columns (column c at base + c * stride).  Columns are
// independent of each other; within one, a chunk reads rows <= a0 + 63 + m and writes rows <= a0 + 63, the next chunk reads
// only rows above that, and its own writes come after its barrier.  lower: the columns right of every source row of the
// chunk hold nothing of L and are skipped.
__device__ void rm_compact(real *base, int ncols, int64_t stride, int k0, int n1, int m, const int *rem, bool lower)
{
    const int rl = threadIdx.x & (RM_RC - 1), cl = threadIdx.x / RM_RC;
    constexpr int CG = RM_THREADS / RM_RC;
    for (int a0 = k0; a0 < n1; a0 += RM_RC) {
        const int a = a0 + rl;
        const int p = a + rm_shift(rem, m, a);
        const int cend = lower ? min(ncols, a0 + RM_RC + m) : ncols;
        for (int cb = 0; cb < cend; cb += CG * RM_CU) {
            real v[RM_CU];
#pragma unroll
            for (int u = 0; u < RM_CU; ++u) {
                const int c = cb + CG * u + cl;
                v[u] = (a < n1 && c < cend) ? base[p + (int64_t)c * stride] : (real)0;
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < RM_CU; ++u) {
                const int c = cb + CG * u + cl;
                if (a < n1 && c < cend) base[a + (int64_t)c * stride] = v[u];
            }
        }
    }
}

__global__ __launch_bounds__(RM_THREADS) void remove_rows_kernel(PatchDesc *descs, real *A, real *__restrict__ ninv, real *x,
                                                                 real *y, real *diag, real *z, real *__restrict__ cvec,
                                                                 int32_t *__restrict__ info,
                                                                 const RemoveTask *__restrict__ tasks,
                                                                 const int32_t *__restrict__ rows, int D)
{
    extern __shared__ double rm_raw[];
    real *img = reinterpret_cast<real *>(rm_raw);       // row segments, one per thread
    real *V = img + RM_THREADS * RM_LDI;                // reflectors of the block
    real *Vb = V + RM_NB * RM_LDV;                      // 2 / v^T v
    real *Vf = Vb + RM_NB;                              // the sign the column is multiplied by
    __shared__ int rem[RM_MAXM];
    __shared__ int Vs[RM_NB];                           // s of the block's reflectors
    __shared__ int sbad;                                // first failed diagonal, 1-based in the trailing block, 0: none
    const RemoveTask tk = tasks[blockIdx.x];
    const PatchDesc pd = descs[tk.region];
    const int m = tk.count, n = pd.n, tid = threadIdx.x;
    const int64_t ld = pd.ld;
    real *Sg = A + pd.aoff;
    real *zp = z + pd.yoff;
    if (tid < m) rem[tid] = rows[tk.first + tid];
    if (tid == 0) sbad = 0;
    __syncthreads();
    const int k0 = rem[0], n1 = n - m, t = n1 - k0;

    // ---- 1. the rows move up
    rm_compact(Sg, n, ld, k0, n1, m, rem, true);
    rm_compact(x + pd.xoff, D, ld, k0, n1, m, rem, false);
    rm_compact(y + pd.yoff, 1, ld, k0, n1, m, rem, false);
    if (diag) rm_compact(diag + pd.yoff, 1, ld, k0, n1, m, rem, false);
    __threadfence_block();
    __syncthreads();

    // ---- 2. the banded reflector sweep, RM_NB new columns at a time; rows j0 .. t of the trailing block, row t is z^T
    real *row = img + tid * RM_LDI;
    for (int j0 = 0; j0 < t; j0 += RM_NB) {
        const int nb = min(RM_NB, t - j0);
        const int wcols = min(RM_W, nb + m);
        for (int i0 = j0; i0 <= t; i0 += RM_THREADS) {
            const int i = i0 + tid;
            const bool live = i <= t, isz = i == t;
            // last column of the row's span, in the trailing block's columns
            const int send = !live ? j0 - 1 : isz ? t + m - 1 : i + rm_shift(rem, m, k0 + i);
            const int wlen = min(wcols, send - j0 + 1);
            const real *src = isz ? zp + k0 + j0 : Sg + (k0 + i) + (int64_t)(k0 + j0) * ld;
            const int64_t cs = isz ? 1 : ld;
#pragma unroll 8
            for (int c = 0; c < wcols; ++c) row[c] = (c < wlen) ? src[c * cs] : (real)0;
            if (i0 == j0) {
                // the block's own rows: thread jj makes reflector jj from its row, which it alone has updated so far
                for (int jj = 0; jj < nb; ++jj) {
                    if (tid == jj) {
                        const int s = send - (j0 + jj);
                        real *xr = row + jj, *v = V + jj * RM_LDV;
                        real nrm2 = 0;
                        for (int k = 0; k <= s; ++k) nrm2 += xr[k] * xr[k];
                        const real nrm = rm_sqrt(nrm2);
                        const bool ok = nrm > (real)0;                  // false for NaN too
                        if (!ok && sbad == 0) sbad = j0 + jj + 1;
                        const real x0 = xr[0], sg = x0 < (real)0 ? (real)-1 : (real)1;
                        v[0] = x0 + sg * nrm;                           // no cancellation
                        for (int k = 1; k <= s; ++k) { v[k] = xr[k]; xr[k] = 0; }
                        Vb[jj] = ok ? (real)1 / (nrm * (nrm + sg * x0)) : (real)0;
                        Vf[jj] = -sg;
                        Vs[jj] = s;
                        xr[0] = ok ? nrm : (real)1;
                    }
                    __syncthreads();
                    if (live && tid > jj) {
                        const int s = Vs[jj];
                        const real *v = V + jj * RM_LDV;
                        real *r = row + jj;
                        real dot = 0;
                        for (int k = 0; k <= s; ++k) dot += v[k] * r[k];
                        const real w = Vb[jj] * dot;
                        for (int k = 0; k <= s; ++k) r[k] -= w * v[k];
                        r[0] *= Vf[jj];
                    }
                }
            } else if (live) {
                for (int jj = 0; jj < nb; ++jj) {
                    const int s = Vs[jj];
                    const real *v = V + jj * RM_LDV;
                    real *r = row + jj;
                    real dot = 0;
                    for (int k = 0; k <= s; ++k) dot += v[k] * r[k];
                    const real w = Vb[jj] * dot;
                    for (int k = 0; k <= s; ++k) r[k] -= w * v[k];
                    r[0] *= Vf[jj];
                }
            }
            real *dst = isz ? zp + k0 + j0 : Sg + (k0 + i) + (int64_t)(k0 + j0) * ld;
#pragma unroll 8
            for (int c = 0; c < wlen; ++c) dst[c * cs] = row[c];
            __syncthreads();                            // the next block's reflectors replace these
        }
        __threadfence_block();
        __syncthreads();                                // the next block reads what this one wrote, by other threads
    }
    if (tid == 0) {
        // a patch that had failed stays failed; its leading minor is named inside the rows that are left
        const int32_t was = info[tk.region];
        if (was > n1) info[tk.region] = n1;
        else if (was == 0 && sbad != 0) info[tk.region] = k0 + sbad;
    }

    // ---- 4. the padding of the rows and columns n1 .. n - 1, as a fit of the reduced set leaves it
    {
        const int tail = n - k0;                        // rows k0 .. n - 1 of the columns n1 .. n - 1
        for (int e = tid; e < tail * m; e += RM_THREADS) {
            const int a = k0 + e % tail, c = n1 + e / tail;
            Sg[a + (int64_t)c * ld] = (a == c) ? (real)1 : (real)0;
        }
        for (int e = tid; e < m * n1; e += RM_THREADS) {        // rows n1 .. n - 1 of the columns < n1
            const int a = n1 + e % m, c = e / m;
            Sg[a + (int64_t)c * ld] = 0;
        }
        if (tid < m) {
            const int a = n1 + tid;
            for (int d = 0; d < D; ++d) x[pd.xoff + (int64_t)d * ld + a] = (real)1e300;
            y[pd.yoff + a] = 0;
            zp[a] = 0;
            cvec[pd.yoff + a] = 0;
            if (diag) diag[pd.yoff + a] = 0;
        }
    }
    __threadfence_block();
    __syncthreads();                                    // the slab as it now stands is visible to every wave
    // -(L[ss])^-1 of the diagonal blocks from k0 / 32 on: a wave per block, one thread per column
    {
        const int lane = tid & 63;
        for (int blk = k0 / RM_SB + (tid >> 6); blk <= (n - 1) / RM_SB; blk += RM_THREADS / 64) {
            if (lane >= RM_SB) continue;
            const int c = lane;
            const real *Dg = Sg + (int64_t)RM_SB * blk + (int64_t)RM_SB * blk * ld;
            real xc[RM_SB];
#pragma unroll
            for (int i = 0; i < RM_SB; ++i) {
                real sacc = (i == c) ? 1.0 : 0.0;
#pragma unroll
                for (int l = 0; l < i; ++l) sacc -= Dg[i + (int64_t)l * ld] * xc[l];
                xc[i] = sacc / Dg[i + (int64_t)i * ld];
            }
            real *out = ninv + pd.ioff + (int64_t)blk * (RM_SB * RM_SB);
#pragma unroll
            for (int i = 0; i < RM_SB; ++i) out[i + RM_SB * c] = (i >= c) ? -xc[i] : 0.0;
        }
    }
    if (tid == 0) descs[tk.region].n = n1;
}

// per-device kernel attribute (called by pmk_ctx_create beside set_append_attributes): the image of the row segments
// needs more than the default 64 KB of dynamic LDS in fp64
int set_remove_attributes()
{
    PMK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(remove_rows_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)RM_LDS_BYTES));
    return 0;
}

// tasks: one per patch that loses rows (count = m_r <= PMK_REMOVE_MAX_ROWS, first = its first entry of `rows`, ascending
// and inside the patch: checked by the caller)
int launch_remove_rows(pmk_model *m, const RemoveTask *d_tasks, int64_t ntasks, const int32_t *d_rows, hipStream_t s)
{
    if (ntasks == 0) return 0;
    hipLaunchKernelGGL(remove_rows_kernel, dim3((unsigned)ntasks), dim3(RM_THREADS), RM_LDS_BYTES, s, m->d_desc,
                       (real *)m->d_a, (real *)m->d_inv, (real *)m->d_x, (real *)m->d_y, (real *)m->d_diag, (real *)m->d_z,
                       (real *)m->d_c, m->d_info, d_tasks, d_rows, m->D);
    PMK_HIP(hipGetLastError());
    return 0;
}

}  // namespace PMK_NS
}  // namespace pmk

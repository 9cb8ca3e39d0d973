// The border of the Cholesky factor: m new points appended to a fitted patch in place (pmk_model_append).
//
//   L' = [ L    0   ]    L21^T = V = L^-1 k(X, Xn)                                  (n x m)
//        [ L21  L22 ]    L22 L22^T = S = k(Xn, Xn) + sigma2 I (+ addends) - V^T V
//   z' = [ z ; L22^-1 (yn - L21 z) ]
//
// The covariance sweep (pmk_cov.hip, its kernels as they are) has left -V in the patch's strip of the arena (ld x TQ,
// column a = new point a, rows past n exact zeros) and S, without a floor on its diagonal, in the patch's m x m block of
// doubles.  append_border_kernel, one workgroup per receiving patch, then
//   copies -(-V) into the rows n .. n + m - 1 of the slab and forms t = yn - L21 z on the way,
//   factors S in LDS (right-looking, the pivot's reciprocal square root as tile_potrf takes it, a failed pivot replaced
//   by 1 and recorded once) with t as one more row, which the elimination turns into the new entries of z,
//   writes L22 into the diagonal tile (both triangles: zeros above the diagonal), the new coordinates over the 1e300
//   padding of x, the targets, the addends and z,
//   inverts anew the 32 x 32 diagonal blocks that meet the rows [n, n + m) (the arithmetic of ninv_from_slab_kernel),
//   and with them the rest of a block row the new rows enter, and
//   writes nt' = ceil((n + m) / 128) and n + m into the device PatchDesc last.
// Rows and columns < n of the slab, z below n and every other -D^-1 block are not written.  The new rows start in the
// patch's last block row, n > 128 (nt - 1), and may run on into the block rows that pmk_model_reserve has laid out past
// it: m <= 128 and n + m <= ld.  Everything from 128 nt up to ld is identity padding before the call (the invariant of
// DESIGN.md section 4), so entering a block row is the new entries plus a change of nt.  c = L'^-T z' is the caller's
// launch_backsolve.
#include "pmk_real.h"

namespace pmk {
namespace PMK_NS {

constexpr int AB_THREADS = 256;
constexpr int AB_LD = TILE + 1;         // leading dimension of the LDS image of S (column-major; row m holds t)
constexpr int AB_SB = 32;               // edge of a -D^-1 block
constexpr size_t AB_LDS_BYTES = sizeof(real) * (size_t)(TILE * AB_LD + TILE + AB_THREADS);

__global__ __launch_bounds__(AB_THREADS) void append_border_kernel(PatchDesc *descs, real *__restrict__ A,
                                                                   real *__restrict__ ninv, real *__restrict__ x,
                                                                   real *__restrict__ y, real *__restrict__ diag,
                                                                   real *__restrict__ z, int32_t *__restrict__ info,
                                                                   const CovTask *__restrict__ tasks,
                                                                   const real *__restrict__ arena,
                                                                   const double *__restrict__ S,
                                                                   const double *__restrict__ xn,
                                                                   const double *__restrict__ yn,
                                                                   const double *__restrict__ dn, int D)
{
    extern __shared__ double ab_raw[];
    real *Sl = reinterpret_cast<real *>(ab_raw);        // S, then L22 (strictly lower) and z' (row m)
    real *Ld = Sl + TILE * AB_LD;                       // diagonal of L22
    real *part = Ld + TILE;                             // partial sums of t
    __shared__ int sbad;                                // first failed pivot, 1-based, 0: none
    const CovTask tk = tasks[blockIdx.x];
    const PatchDesc pd = descs[tk.region];
    const int m = tk.count, n = pd.n, tid = threadIdx.x;
    const int64_t ld = pd.ld;
    real *Sg = A + pd.aoff;

    {   // S: the lower triangle
        const double *Sr = S + tk.goff;
        for (int e = tid; e < m * m; e += AB_THREADS) {
            const int i = e % m, k = e / m;
            if (i >= k) Sl[i + AB_LD * k] = (real)Sr[i + (int64_t)m * k];
        }
        if (tid == 0) sbad = 0;
    }
    {   // L21 = V^T into the slab (coalesced along the new rows), t = yn - L21 z; the strip holds -V
        int cw = 16;
        while (cw < m) cw <<= 1;
        const int groups = AB_THREADS / cw, col = tid & (cw - 1), grp = tid / cw;
        const real *V = arena + tk.voff + col;
        const real *zp = z + pd.yoff;
        real *dst = Sg + n + col;
        real acc = 0;
        if (col < m) {
#pragma unroll 4
            for (int j = grp; j < n; j += groups) {
                const real v = V[(int64_t)j * TQ];
                dst[(int64_t)j * ld] = -v;
                acc += v * zp[j];
            }
        }
        part[tid] = acc;
        __syncthreads();
        if (tid < m) {
            real t = (real)yn[tk.first + tid];
            for (int g = 0; g < groups; ++g) t += part[g * cw + tid];
            Sl[m + AB_LD * tid] = t;
        }
    }
    // right-looking factorisation of S with t as row m; thread (tx, ty) of a 16 x 16 grid takes the rows k + tx + 16 u
    // of the columns j + 1 + ty + 16 v
    const int tx = tid & 15, ty = tid >> 4;
    for (int j = 0; j < m; ++j) {
        __syncthreads();
        real d = Sl[j + AB_LD * j];
        if (!(d > (real)0)) {                           // not positive definite (or NaN): record, keep going
            if (tid == 0 && sbad == 0) sbad = j + 1;
            d = 1;
        }
        const real rs = rsqrt_real(d);
        if (tid == 0) Ld[j] = d * rs;
        for (int i = j + 1 + tid; i <= m; i += AB_THREADS) Sl[i + AB_LD * j] *= rs;
        __syncthreads();
        for (int k = j + 1 + ty; k < m; k += 16) {
            const real lk = Sl[k + AB_LD * j];
            for (int i = k + tx; i <= m; i += 16) Sl[i + AB_LD * k] -= Sl[i + AB_LD * j] * lk;
        }
    }
    __syncthreads();
    // the diagonal tile keeps both of its triangles in the slab: zeros above the diagonal of L22
    for (int e = tid; e < m * m; e += AB_THREADS) {
        const int a = e % m, b = e / m;
        const real v = a > b ? Sl[a + AB_LD * b] : (a == b ? Ld[a] : (real)0);
        Sg[(n + a) + (int64_t)(n + b) * ld] = v;
    }
    if (tid < m) {
        const int64_t it = tk.first + tid;
        for (int d = 0; d < D; ++d) x[pd.xoff + (int64_t)d * ld + n + tid] = (real)xn[it * D + d];
        y[pd.yoff + n + tid] = (real)yn[it];
        if (diag) diag[pd.yoff + n + tid] = dn ? (real)dn[it] : (real)0;
        z[pd.yoff + n + tid] = Sl[m + AB_LD * tid];
    }
    if (tid == 0 && sbad != 0 && info[tk.region] == 0) info[tk.region] = n + sbad;
    __threadfence_block();
    __syncthreads();                                    // the new rows of the slab are visible to every wave
    // -(L[ss])^-1 of the diagonal blocks that meet the new rows: wave w takes the blocks n / 32 + w, + 4, ..., one thread
    // per column.  Rows that enter a new block row (nt2 > nt) take every block up to the end of the last block row
    // entered: those past the new rows are identity padding and get the blocks a loaded factor has there.  Up to eight
    // blocks (128 rows meet five, three more in padding).
    const int nt2 = (n + m + TILE - 1) / TILE;
    const int last_blk = nt2 > pd.nt ? 4 * nt2 - 1 : (n + m - 1) / AB_SB;
    for (int blk = n / AB_SB + (tid >> 6); blk <= last_blk; blk += AB_THREADS / 64) {
        const int lane = tid & 63;
        if (lane < AB_SB) {
            const int c = lane;
            const real *Dg = Sg + (int64_t)AB_SB * blk + (int64_t)AB_SB * blk * ld;
            real xc[AB_SB];
#pragma unroll
            for (int i = 0; i < AB_SB; ++i) {
                real sacc = (i == c) ? 1.0 : 0.0;
#pragma unroll
                for (int l = 0; l < i; ++l) sacc -= Dg[i + (int64_t)l * ld] * xc[l];
                xc[i] = sacc / Dg[i + (int64_t)i * ld];
            }
            real *out = ninv + pd.ioff + (int64_t)blk * (AB_SB * AB_SB);
#pragma unroll
            for (int i = 0; i < AB_SB; ++i) out[i + AB_SB * c] = (i >= c) ? -xc[i] : 0.0;
        }
    }
    if (tid == 0) {
        descs[tk.region].nt = nt2;
        descs[tk.region].n = n + m;
    }
}

// per-device kernel attribute (called by pmk_ctx_create beside set_device_attributes): the image of S needs more than
// the default 64 KB of dynamic LDS in both precisions
int set_append_attributes()
{
    PMK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(append_border_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)AB_LDS_BYTES));
    return 0;
}

// q carries the tasks (one per receiving patch: count = m_r, first = its first staged item), the arena and the blocks of
// the sweep that ran before; d_y, d_diag: targets and addends (or null) of the staged items
int launch_append_border(pmk_model *m, const pmk_query *q, const double *d_y, const double *d_diag, hipStream_t s)
{
    if (q->cov_ntasks == 0) return 0;
    hipLaunchKernelGGL(append_border_kernel, dim3((unsigned)q->cov_ntasks), dim3(AB_THREADS), AB_LDS_BYTES, s, m->d_desc,
                       (real *)m->d_a, (real *)m->d_inv, (real *)m->d_x, (real *)m->d_y, (real *)m->d_diag, (real *)m->d_z,
                       m->d_info, q->d_cov_tasks, (const real *)q->d_cov_v, q->d_cov_s, q->d_xq, d_y, d_diag, m->D);
    PMK_HIP(hipGetLastError());
    return 0;
}

}  // namespace PMK_NS
}  // namespace pmk

// Model selection from the resident factor: the two per-patch scores of a fit at (theta, sigma2) that need nothing but
// L, y and c (Rasmussen & Williams, Gaussian Processes for Machine Learning, eq. 5.8 and 5.10-5.12).
//
//   loo_strip_kernel    d = diag((L L^T)^-1) = squared column norms of L^-1, for every patch.  The leave-one-out
//                       prediction of training point i from the other n - 1 has residual c_i / d_i and variance 1 / d_i.
//   evidence_kernel     log det (K + sigma2 I) = 2 sum log L_ii and y^T c (R columns in the multi-output form)
//   loo_values_kernel   res = c / d, var = 1 / d, NaN where the factorisation failed
//
// loo_strip_kernel is the prediction strip sweep (pmk_predict.hip) with identity columns as right-hand sides.  A task
// is (patch, strip s): the 256 columns 256 s .. 256 s + 255 of L^-1.  Column j of L^-1 is zero above row j, so the strip
// starts at block row i0 = 2 s, and the second half of its columns (waves 4..7) one block row later:
//     block row i:  acc(128 x 32) = E_i - L[i, 128 w0 : 128 i] V[128 w0 : 128 i]     (w0: first block row of the wave;
//                                                                                      E_i: identity slice, nonzero at i = w0)
//                   -V_i = -L[ii]^-1 acc ; column sums of squares += V_i^2
// with strip_block_row (pmk_strip.h) doing the product and the block substitution exactly as in prediction.  There is
// no kernel evaluation, no mean and no query point; nothing passes between the waves of a workgroup.
//
// Work.  Wave group h (0: columns 0..127, 1: columns 128..255 of strip s) runs nt - 2 s - h block rows with K = 128 k,
// k = 0 .. nt - 2 s - h - 1: the m = nt - 2 s - h of a patch run over 1 .. nt, so a patch executes
// 2 * 128^3 * C(nt + 1, 3) flop of GEMM and nt (nt + 1) / 2 substitutions of 128^2 * 128.  At nt = 16 that is 2.85e9 +
// 0.29e9 = 3.14e9 = 1.18 n^3 / 3 (n = 2000); starting every column of a strip at block row 2 s would make it 1.28.
//
// Tasks differ in length, so they are handed out longest first from queues, one per XCD: a workgroup draws from the queue
// of its own XCD (blockIdx.x & 7) and, when that is empty, from the others.  With at least 8 patches all strips of a
// patch sit in one queue, so the workgroups that stream one factor do so through one L2.  Locality only: any workgroup
// may run any task.
#include <algorithm>
#include <numeric>

#include "pmk_strip.h"

namespace pmk {
namespace PMK_NS {

struct LooTask {
    int32_t patch;     // local patch index
    int32_t strip;     // columns 256 strip .. 256 strip + 255 of the patch
};
struct LooQueues {
    int32_t off[9];    // queue x holds tasks [off[x], off[x + 1])
};

__global__ __launch_bounds__(STRIP_THREADS, 2) void loo_strip_kernel(const PatchDesc *__restrict__ descs, const real *__restrict__ A,
                                                                   const real *__restrict__ inv, const LooTask *__restrict__ tasks,
                                                                   LooQueues qs, uint32_t *__restrict__ heads,
                                                                   real *__restrict__ strips, int64_t strip_stride,
                                                                   double *__restrict__ d_out)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    real *V = strips + (int64_t)blockIdx.x * strip_stride + STRIP_WCOLS * wave;   // this wave's columns, ld = TQ
    // the running sums of squares are parked in LDS between the MFMA phases, as in prediction: around its GEMM the
    // block-row routine has no register to spare
    __shared__ real park[STRIP_NC * STRIP_THREADS];
    __shared__ int next_task;
    real *pk = park + threadIdx.x;
    // 0: columns 0..127 of the strip, 1: columns 128..255 (wave-uniform, and said so: the GEMM's trip count depends on it.
    // Saying the same of the whole wave index doubles the spills: 172 registers against 75)
    const int half = __builtin_amdgcn_readfirstlane(wave / (STRIP_WAVES / 2));
    int tried = 0;                                  // thread 0 only: queues found empty so far

    for (;;) {
        __syncthreads();                            // every wave has read the previous task's index
        if (threadIdx.x == 0) {
            int t = -1;
            while (tried < 8) {
                const int x = ((int)(blockIdx.x & 7) + tried) & 7;
                const uint32_t k = __hip_atomic_fetch_add(heads + x, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (k < (uint32_t)(qs.off[x + 1] - qs.off[x])) {
                    t = qs.off[x] + (int)k;
                    break;
                }
                ++tried;
            }
            next_task = t;
        }
        __syncthreads();
        const int task = next_task;
        if (task < 0) break;
        const LooTask tk = tasks[task];
        const PatchDesc pd = descs[tk.patch];
        const int i0 = 2 * tk.strip;
        const int count = min(TQ, pd.nt * TILE - TQ * tk.strip);   // 128 in the last strip of a patch with an odd tile count
        const bool active = STRIP_WCOLS * wave < count;            // wave-uniform
        const int w0 = i0 + half;                            // first block row in which this wave's columns are not zero
        const real *S = A + pd.aoff;
        const int64_t ld = pd.ld;
        // rows of the last block row that are not identity padding, in 32-row pairs
        const int last_pairs = (pd.n - (pd.nt - 1) * TILE + 31) >> 5;
#pragma unroll
        for (int c = 0; c < STRIP_NC; ++c) pk[c * STRIP_THREADS] = (real)0;

        for (int i = i0; i < pd.nt; ++i) {
            // No data passes between the waves.  The barrier keeps the eight waves on the same block row of L, the one
            // operand they all read, as the barrier of the prediction strip does; what it is worth here has not been
            // measured.
            __syncthreads();
            if (!active || i < w0) continue;
            WaveTile<4, 1> acc;
            acc.zero();
            if (i == w0) {
                // E_i: row r of the block row meets column 128 half + r of the strip
#pragma unroll
                for (int fi = 0; fi < 8; ++fi)
#pragma unroll
                    for (int qq = 0; qq < 4; ++qq)
#pragma unroll
                        for (int c = 0; c < STRIP_NC; ++c)
                            if (tile_i(fi, lane, qq) == STRIP_WCOLS * (wave % (STRIP_WAVES / 2)) + 2 * (lane & 15) + c)
                                acc.f[fi][c][qq] = (real)1;
            }
            // ---- acc -= L[i, 128 w0 : 128 i] V[128 w0 : 128 i]  (the strip holds -V), then acc <- -V_i = -L[ii]^-1 acc.
            //      Padding rows of the last block row are zero in every column that is written out: skip them.
            const real *Li = S + (int64_t)i * TILE + (int64_t)w0 * TILE * ld;
            const real *Lii = S + (int64_t)i * TILE + (int64_t)i * TILE * ld;
            const real *ninv_i = inv + pd.ioff + (int64_t)i * 4096;
            const real *Vw = V + (int64_t)w0 * TILE * TQ;
            const int nb = i - w0;
            if (i + 1 == pd.nt && last_pairs == 3) strip_block_row<3>(acc, Li, ld, Vw, nb, Lii, ninv_i, lane);
            else if (i + 1 == pd.nt && last_pairs == 2) strip_block_row<2>(acc, Li, ld, Vw, nb, Lii, ninv_i, lane);
            else if (i + 1 == pd.nt && last_pairs == 1) strip_block_row<1>(acc, Li, ld, Vw, nb, Lii, ninv_i, lane);
            else strip_block_row<4>(acc, Li, ld, Vw, nb, Lii, ninv_i, lane);
            {
                real vs[STRIP_NC];
#pragma unroll
                for (int c = 0; c < STRIP_NC; ++c) vs[c] = pk[c * STRIP_THREADS];
#pragma unroll
                for (int fi = 0; fi < 8; ++fi)
#pragma unroll
                    for (int qq = 0; qq < 4; ++qq)
#pragma unroll
                        for (int c = 0; c < STRIP_NC; ++c) vs[c] += acc.f[fi][c][qq] * acc.f[fi][c][qq];
#pragma unroll
                for (int c = 0; c < STRIP_NC; ++c) pk[c * STRIP_THREADS] = vs[c];
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
                        __builtin_nontemporal_store(o, reinterpret_cast<real2_t *>(V + (int64_t)row * TQ + 2 * (lane & 15)));
                    }
            }
        }
        // ---- reduce over the four lane groups that share a column, then write d once per column (never for padding)
#pragma unroll
        for (int c = 0; c < STRIP_NC && active; ++c) {
            real b = pk[c * STRIP_THREADS];
            b += __shfl_xor(b, 16);
            b += __shfl_xor(b, 32);
            const int col = TQ * tk.strip + STRIP_WCOLS * wave + 2 * (lane & 15) + c;
            if ((lane >> 4) == 0 && col < pd.n) d_out[pd.yoff + col] = (double)b;
        }
        // the next task reuses the strip: order its first stores after this task's last loads
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    }
}

// strip tasks of the model (they depend on the patch sizes only) and their queues.  Mirrored by tasks() in tests/_loo_schedule.py.
static int build_loo_tasks(pmk_model *m, hipStream_t s)
{
    std::vector<LooTask> all;
    std::vector<int64_t> cost;                       // block-row products of a task, ~ its run time
    std::vector<int> queue_of;
    int64_t load[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    auto lightest = [&]() { return (int)(std::min_element(load, load + 8) - load); };
    // whole patches go to the lightest queue, largest first; with fewer patches than queues single tasks do
    std::vector<int64_t> order((size_t)m->P);
    std::iota(order.begin(), order.end(), (int64_t)0);
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return m->desc[(size_t)a].nt > m->desc[(size_t)b].nt; });
    for (int64_t r : order) {
        const int nt = m->desc[(size_t)r].nt;
        int x = lightest();
        for (int st = 0; 2 * st < nt; ++st) {
            const int64_t len = nt - 2 * st;
            if (m->P < 8) x = lightest();
            all.push_back(LooTask{(int32_t)r, (int32_t)st});
            cost.push_back(len * len);
            queue_of.push_back(x);
            load[x] += len * len;
        }
    }
    // grouped by queue, longest first inside a queue
    std::vector<size_t> idx(all.size());
    std::iota(idx.begin(), idx.end(), (size_t)0);
    std::stable_sort(idx.begin(), idx.end(), [&](size_t a, size_t b) {
        return queue_of[a] != queue_of[b] ? queue_of[a] < queue_of[b] : cost[a] > cost[b];
    });
    std::vector<LooTask> tasks(all.size());
    for (int x = 0; x <= 8; ++x) m->loo_qoff[x] = 0;
    for (size_t k = 0; k < idx.size(); ++k) {
        tasks[k] = all[idx[k]];
        ++m->loo_qoff[queue_of[idx[k]] + 1];
    }
    for (int x = 0; x < 8; ++x) m->loo_qoff[x + 1] += m->loo_qoff[x];
    // loo_ntasks is set last: a call that failed half way is repeated and keeps what it had allocated
    if (!m->d_loo_tasks) PMK_HIP(hipMalloc(&m->d_loo_tasks, sizeof(LooTask) * tasks.size()));
    if (!m->d_loo_cnt) PMK_HIP(hipMalloc((void **)&m->d_loo_cnt, sizeof(uint32_t) * 8));
    if (!m->d_dloo) PMK_HIP(hipMalloc((void **)&m->d_dloo, sizeof(double) * (size_t)std::max<int64_t>(m->tot_y, 1)));
    PMK_HIP(hipMemcpyAsync(m->d_loo_tasks, tasks.data(), sizeof(LooTask) * tasks.size(), hipMemcpyHostToDevice, s));
    PMK_HIP(hipStreamSynchronize(s));            // `tasks` is a local
    m->loo_ntasks = (int64_t)tasks.size();
    return 0;
}

int launch_loo(pmk_model *m, hipStream_t s)
{
    if (m->loo_ntasks == 0)
        if (int rc = build_loo_tasks(m, s)) return rc;
    const int64_t slots = std::min<int64_t>(m->loo_ntasks, (int64_t)m->ctx->num_cu);     // one 8-wave workgroup per CU
    if (int rc = reserve_strips(m, slots)) return rc;
    LooQueues qs;
    for (int x = 0; x <= 8; ++x) qs.off[x] = m->loo_qoff[x];
    PMK_HIP(hipMemsetAsync(m->d_loo_cnt, 0, sizeof(uint32_t) * 8, s));
    hipLaunchKernelGGL(loo_strip_kernel, dim3((unsigned)slots), dim3(STRIP_THREADS), 0, s, m->d_desc, (const real *)m->d_a,
                       (const real *)m->d_inv, (const LooTask *)m->d_loo_tasks, qs, m->d_loo_cnt, (real *)m->d_strip,
                       (int64_t)m->max_nt * TILE * TQ, m->d_dloo);
    PMK_HIP(hipGetLastError());
    return 0;
}

// One workgroup per patch.  Sums in double in both precisions; a fixed reduction tree, so the result does not depend on
// scheduling.  RP = 1: y and c are the model's vectors; RP = PMK_MAX_OUTPUTS: the row-major R-column blocks of
// pmk_multi.hip, thread t sums column t % RP.  quad[r + P j] = Y[:, j]^T C[:, j].
constexpr int EV_THREADS = 256;

template <int RP>
__global__ __launch_bounds__(EV_THREADS) void evidence_kernel(const PatchDesc *__restrict__ descs, const real *__restrict__ A,
                                                              const int32_t *__restrict__ info, const real *__restrict__ Y,
                                                              const real *__restrict__ Cw, int R, int P,
                                                              double *__restrict__ logdet, double *__restrict__ quad)
{
    const int r = blockIdx.x, tid = threadIdx.x;
    const PatchDesc pd = descs[r];
    const bool failed = info[r] != 0;
    const double nan = __builtin_nan("");
    __shared__ double red[EV_THREADS];
    if (logdet) {
        const real *S = A + pd.aoff;
        double a = 0.0;
        for (int i = tid; i < pd.n; i += EV_THREADS) a += 2.0 * log((double)S[i + (int64_t)i * pd.ld]);
        red[tid] = a;
        __syncthreads();
        for (int st = EV_THREADS / 2; st >= 1; st >>= 1) {
            if (tid < st) red[tid] += red[tid + st];
            __syncthreads();
        }
        if (tid == 0) logdet[r] = failed ? nan : red[0];
        __syncthreads();
    }
    if (quad) {
        const int j = tid % RP;
        double a = 0.0;
        for (int i = tid / RP; i < pd.n; i += EV_THREADS / RP) {
            const int64_t e = (pd.yoff + i) * RP + j;
            a += (double)Y[e] * (double)Cw[e];
        }
        red[tid] = a;
        __syncthreads();
        for (int st = EV_THREADS / 2; st >= RP; st >>= 1) {      // t and t + st sum the same column
            if (tid < st) red[tid] += red[tid + st];
            __syncthreads();
        }
        if (tid < R) quad[r + (int64_t)P * tid] = failed ? nan : red[tid];
    }
}

int launch_evidence(const pmk_model *m, int R, double *d_logdet, double *d_quad, hipStream_t s)
{
    if (R == 0)
        hipLaunchKernelGGL(evidence_kernel<1>, dim3((unsigned)m->P), dim3(EV_THREADS), 0, s, m->d_desc, (const real *)m->d_a,
                           m->d_info, (const real *)m->d_y, (const real *)m->d_c, 1, (int)m->P, d_logdet, d_quad);
    else
        hipLaunchKernelGGL(evidence_kernel<PMK_MAX_OUTPUTS>, dim3((unsigned)m->P), dim3(EV_THREADS), 0, s, m->d_desc,
                           (const real *)m->d_a, m->d_info, (const real *)m->d_ym, (const real *)m->d_cm, R, (int)m->P, d_logdet,
                           d_quad);
    PMK_HIP(hipGetLastError());
    return 0;
}

// res = c / d and var = 1 / d in double (IEEE division), one workgroup per patch.  RP as in evidence_kernel: res has the
// layout of the weights it is computed from.
template <int RP>
__global__ __launch_bounds__(256) void loo_values_kernel(const PatchDesc *__restrict__ descs, const int32_t *__restrict__ info,
                                                         const double *__restrict__ d, const real *__restrict__ Cw,
                                                         double *__restrict__ res, double *__restrict__ var)
{
    const PatchDesc pd = descs[blockIdx.x];
    const bool failed = info[blockIdx.x] != 0;
    const double nan = __builtin_nan("");
    for (int i = threadIdx.x / RP; i < pd.n; i += 256 / RP) {
        const int j = threadIdx.x % RP;
        const double di = d[pd.yoff + i];
        const int64_t e = (pd.yoff + i) * RP + j;
        if (res) res[e] = failed ? nan : (double)Cw[e] / di;
        if (var && j == 0) var[pd.yoff + i] = failed ? nan : 1.0 / di;
    }
}

int launch_loo_values(const pmk_model *m, int R, double *d_res, double *d_var, hipStream_t s)
{
    if (R == 0)
        hipLaunchKernelGGL(loo_values_kernel<1>, dim3((unsigned)m->P), dim3(256), 0, s, m->d_desc, m->d_info, m->d_dloo,
                           (const real *)m->d_c, d_res, d_var);
    else
        hipLaunchKernelGGL(loo_values_kernel<PMK_MAX_OUTPUTS>, dim3((unsigned)m->P), dim3(256), 0, s, m->d_desc, m->d_info,
                           m->d_dloo, (const real *)m->d_cm, d_res, d_var);
    PMK_HIP(hipGetLastError());
    return 0;
}

}  // namespace PMK_NS
}  // namespace pmk

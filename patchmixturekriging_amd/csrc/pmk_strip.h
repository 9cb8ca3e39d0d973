// The block-row routine of a 256-column strip of right-hand sides swept down a resident factor L, shared by the two
// kernels that run such strips: prediction (pmk_predict.hip: the columns are cross-kernel vectors k_q) and leave-one-out
// (pmk_loo.hip: the columns are identity columns, i.e. the strip is a block column of L^-1).
//
// A workgroup owns TQ = 256 columns (8 waves x 32 columns: one workgroup per CU, two waves per SIMD); a wave owns a
// 128 x 32 tile of the current block row in registers and keeps the finished block rows of its columns, NEGATED, in the
// workgroup's strip workspace in global memory (leading dimension TQ), so that the MFMA accumulates the subtraction.
#pragma once

#include "pmk_mfma.h"

namespace pmk {
namespace PMK_NS {

constexpr int PF_PRED = 4;          // I-operand (factor, from L2) prefetch depth in k-steps
constexpr int PFJ_PRED = 4;         // J-operand (the wave's own strip columns, HBM) prefetch depth
// a wave owns a 128 x 32 tile of the strip (WaveTile<4, 1>): eight waves, two per SIMD (256 registers each)
constexpr int STRIP_WCOLS = 32;     // strip columns of a wave
constexpr int STRIP_WAVES = TQ / STRIP_WCOLS;
constexpr int STRIP_THREADS = 64 * STRIP_WAVES;
constexpr int STRIP_NC = 2;         // strip columns of a lane

// one block row of the strip: acc = right-hand side of the block row (in) -> -V_i (out).  Li: the block row of the factor
// from the first column the strip's earlier block rows cover, V: those block rows of the wave's columns, i: how many
// 128-column blocks that is (prediction: all i blocks left of the diagonal).
template <int NACT>
__device__ __forceinline__ void strip_block_row(WaveTile<4, 1> &acc, const real *Li, int64_t ld, const real *V, int i,
                                                const real *Lii, const real *ninv_i, int lane, bool traced = false)
{
    if (i > 0) {
        // order this wave's earlier strip stores before its loads of them
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        gemm_nt_indexed<4, 1, PF_PRED, PFJ_PRED, NACT>(acc, Li, ld, V, TQ, i * TILE, lane);
    }
#if defined(PMK_TRACE) && defined(PMK_STRIP_STAMPS)
    if (traced && i == PMK_TRACE_ROW && lane == 0 && blockIdx.x < 64) {
        g_row_stamp[(blockIdx.x * 8 + (threadIdx.x >> 6)) * 8 + 3] = __builtin_amdgcn_s_memrealtime();
        g_row_stamp[(blockIdx.x * 8 + (threadIdx.x >> 6)) * 8 + 7] = __builtin_amdgcn_s_memtime();      // shader clock
    }
#endif
    // the TRSM operands come straight from the factor (prefetched block by block into registers): no LDS copy, no
    // barrier around staging one
    tri_solve_global<1>(acc, Lii, ld, ninv_i, lane);
}

}  // namespace PMK_NS
}  // namespace pmk

/*
 * pmk_test.h -- self-test entry points of libpmk_hip.so (used by tests/ only).
 * They exercise the fp64 MFMA tile routines on caller-supplied data so the fragment layout
 * (cdna_hip_programming.md section 3: v_mfma_f64_16x16x4_f64 does NOT use the f32 C/D map)
 * is checked with asymmetric integer data on the real device.
 */
#ifndef PMK_TEST_H
#define PMK_TEST_H

#include <stdint.h>

#include "pmk.h"

#ifdef __cplusplus
extern "C" {
#endif

/* C[I][J] (128 x 32, J contiguous: C[J + 32*I]) = sum_k MI[I + 128 k] MJ[J + 32 k],
 * k < K (K a multiple of 16), through the four forms of the wave-tile GEMM loop (gemm_nt, gemm_nt_indexed,
 * gemm_nt_sbase, gemm_nt_buf -- the last also with a J ring of 8 k-steps where K is a multiple of 32) of one wave;
 * elements on which they disagree come back as NaN.  Host buffers. */
int pmk_selftest_gemm(pmk_ctx *ctx, int K, const double *MI, const double *MJ, double *C);
/* T (128 x 32, T[J + 32*I]) <- -L^-1 T through tri_solve_inplace (operands staged in LDS) AND tri_solve_global (operands
 * prefetched from global memory); elements on which the two disagree come back as NaN.  L is 128 x 128 column-major
 * lower, ninv its four negated inverted 32 x 32 diagonal blocks (column-major, ld 32) */
int pmk_selftest_trisolve(pmk_ctx *ctx, const double *L, const double *ninv, const double *T_in, double *T_out);
/* sustained fp64 MFMA rate of the device in TFLOP/s (register-resident loop, all CUs) */
int pmk_selftest_mfma_peak(pmk_ctx *ctx, double *tflops);

/* make pmk_query_predict_sharded run its whole request / response exchange even when the communicator has one rank
 * (the rank then sends to itself through RCCL): the only way to drive that path on a one-GPU box */
int pmk_test_comm_force_exchange(pmk_comm *comm, int on);

/* choose the factorisation path of a model by hand: 0 = one workgroup per block row (batched), 1 = split path (deep
 * products cut along K; the triangular solves as one chained launch each where the blocks nearly fit on the chip, block
 * by block otherwise), 2 = split path with the block-by-block solves, 3 = split path with the chained solves whatever
 * the size; pmk_model_create picks by itself from P and the tile counts */
int pmk_test_model_set_split(pmk_model *model, int on);

/* the packed device buffers of one patch WITH their padding rows, as doubles (tests compare what the host route and the
 * device route of the model set-up leave there): what = 0 the SoA coordinates (D rows of ld), 1 the targets (ld), 2 the
 * diagonal addend (ld; -3 if none is set), 3 the multi-output targets (ld rows of PMK_MAX_OUTPUTS; -3 if none).  *ld
 * receives the padded row count; out == NULL only reports it.  Blocks. */
int pmk_test_model_packed(pmk_model *model, int64_t patch, int what, int64_t *ld, double *out);

/* the device addresses of the model's slabs, coordinates and weights as integers (tests of pmk_model_reserve: a call
 * with nothing to grow must not move the model, one that grows a patch moves all of it); never dereferenced */
int pmk_test_model_buffers(pmk_model *model, int64_t *slabs, int64_t *points, int64_t *weights);

/* 1 if the buffer-load form of the wave-tile GEMM can address an operand of K columns with leading dimension ld
 * (elements of elem_size bytes, J ring of pfj k-steps) with its 32-bit offsets: (K + 4 pfj) ld elem_size < 2^31; else 0.
 * Pure: needs no device. */
int pmk_test_gemm_buf_extent_ok(int64_t K, int64_t ld, int pfj, int elem_size);

/* the loop forms that PMK_STEP_GEMM=auto gives the factorisation step launch with G block rows below the diagonal at
 * block column k: 0 = pointer form (gemm_nt), 1 = buffer-load form (gemm_nt_buf).  A function of its four arguments
 * alone.  Pure: needs no device. */
int pmk_test_step_gemm_rule(int G, int k, int f32, int fused);

#ifdef __cplusplus
}
#endif
#endif

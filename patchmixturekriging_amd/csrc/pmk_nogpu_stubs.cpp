// Stand-ins for every device-side launcher of libpmk_hip.so, for the HOST sanitizer build only (make asan): the host
// code of the C ABI (pmk_api.cpp, pmk_comm.cpp, pmk_bsp.cpp) is compiled with g++ -fsanitize=address,undefined and linked
// against these instead of the .hip objects, so that the CPU test-suite can run the argument checks, the exact host
// BSP, the sharding arithmetic and every error path under ASan / UBSan in a container without a GPU.  Never part of
// libpmk_hip.so: a product call that reaches one of these fails loudly.
#include "pmk_internal.h"

namespace pmk {

static int no_gpu(const char *what)
{
    set_error("%s: this is the host sanitizer build (no device code)", what);
    return -100;
}

#define PMK_STUB_REAL(NS)                                                                                          \
    namespace NS {                                                                                                  \
    int launch_kernel_matrix_slabs(const pmk_model *, const pmk_kernel_desc *, double, hipStream_t, int64_t, int64_t, bool) { return no_gpu("launch_kernel_matrix_slabs"); } \
    int launch_cholesky(pmk_model *, hipStream_t, int64_t, int64_t) { return no_gpu("launch_cholesky"); }         \
    int launch_backsolve(pmk_model *, hipStream_t, int64_t, int64_t) { return no_gpu("launch_backsolve"); }       \
    int launch_ninv_from_slabs(pmk_model *, hipStream_t) { return no_gpu("launch_ninv_from_slabs"); }             \
    int set_device_attributes() { return 0; }                                                                       \
    int build_strip_tasks(pmk_query *, hipStream_t) { return no_gpu("build_strip_tasks"); }                        \
    int launch_items(pmk_query *, const pmk_kernel_desc *, hipStream_t) { return no_gpu("launch_items"); }         \
    int launch_solve_multi(pmk_model *, hipStream_t) { return no_gpu("launch_solve_multi"); }                       \
    int launch_items_multi(pmk_query *, const pmk_kernel_desc *, hipStream_t) { return no_gpu("launch_items_multi"); } \
    int launch_loo(pmk_model *, hipStream_t) { return no_gpu("launch_loo"); }                                       \
    int launch_evidence(const pmk_model *, int, double *, double *, hipStream_t) { return no_gpu("launch_evidence"); } \
    int launch_loo_values(const pmk_model *, int, double *, double *, hipStream_t) { return no_gpu("launch_loo_values"); } \
    int launch_gather_points(const pmk_model *, const double *, const double *, hipStream_t) { return no_gpu("launch_gather_points"); } \
    int launch_gather_vector(const pmk_model *, const double *, void *, hipStream_t) { return no_gpu("launch_gather_vector"); } \
    int launch_gather_multi(const pmk_model *, int, const double *, int64_t, hipStream_t) { return no_gpu("launch_gather_multi"); } \
    int launch_trend_fill(const pmk_model *, int, int, hipStream_t) { return no_gpu("launch_trend_fill"); }         \
    int launch_trend_gls(pmk_model *, int, int, hipStream_t) { return no_gpu("launch_trend_gls"); }                 \
    int launch_trend_loo_values(const pmk_model *, int, int, double *, double *, hipStream_t) { return no_gpu("launch_trend_loo_values"); } \
    int launch_loo_member(pmk_query *, int, int32_t *, hipStream_t) { return no_gpu("launch_loo_member"); }         \
    int launch_loo_compact(pmk_query *, const int32_t *, const int64_t *, double *, int32_t *, double *, hipStream_t) { return no_gpu("launch_loo_compact"); } \
    int launch_loo_scatter(pmk_query *, int, const int32_t *, const int64_t *, const double *, const double *, hipStream_t) { return no_gpu("launch_loo_scatter"); } \
    int launch_loo_member_multi(pmk_query *, int, int, int32_t *, hipStream_t) { return no_gpu("launch_loo_member_multi"); } \
    int launch_items_grad(pmk_query *, const pmk_kernel_desc *, hipStream_t) { return no_gpu("launch_items_grad"); } \
    int launch_items_vgrad(pmk_query *, const pmk_kernel_desc *, hipStream_t) { return no_gpu("launch_items_vgrad"); } \
    int launch_items_cov(pmk_query *, const pmk_kernel_desc *, hipStream_t) { return no_gpu("launch_items_cov"); }  \
    int launch_items_block(pmk_query *, const pmk_kernel_desc *, hipStream_t) { return no_gpu("launch_items_block"); } \
    int launch_append_border(pmk_model *, const pmk_query *, const double *, const double *, hipStream_t) { return no_gpu("launch_append_border"); } \
    int set_append_attributes() { return 0; }                                                                       \
    int launch_remove_rows(pmk_model *, const RemoveTask *, int64_t, const int32_t *, hipStream_t) { return no_gpu("launch_remove_rows"); } \
    int set_remove_attributes() { return 0; }                                                                       \
    int launch_reserve(const pmk_model *, const PatchDesc *, void *, void *, void *, void *, void *, void *, void *, int64_t, hipStream_t) { return no_gpu("launch_reserve"); } \
    }
PMK_STUB_REAL(f64)
PMK_STUB_REAL(f32)

int launch_kernel_matrix_dense(const pmk_kernel_desc &, int, int64_t, const double *, int64_t, int64_t, const double *, int64_t,
                               double *, int64_t, bool, hipStream_t) { return no_gpu("launch_kernel_matrix_dense"); }
int set_plan_attributes() { return 0; }
int launch_iota(int32_t *, int64_t, hipStream_t) { return no_gpu("launch_iota"); }
int launch_plan_count(pmk_query *, double, double, hipStream_t) { return no_gpu("launch_plan_count"); }
int launch_plan_fill(pmk_query *, double, double, hipStream_t) { return no_gpu("launch_plan_fill"); }
int launch_sort_items(pmk_query *, hipStream_t) { return no_gpu("launch_sort_items"); }
int launch_mix(pmk_query *, const pmk_kernel_desc &, int64_t, int64_t, hipStream_t) { return no_gpu("launch_mix"); }
int launch_mix_multi(pmk_query *, const pmk_kernel_desc &, int64_t, int64_t, hipStream_t) { return no_gpu("launch_mix_multi"); }
int launch_trend_items(pmk_query *, int, int, bool, hipStream_t) { return no_gpu("launch_trend_items"); }
int launch_mix_grad(pmk_query *, const pmk_kernel_desc &, int64_t, int64_t, hipStream_t) { return no_gpu("launch_mix_grad"); }
int launch_trend_vgrad(pmk_query *, hipStream_t) { return no_gpu("launch_trend_vgrad"); }
int launch_mix_vgrad(pmk_query *, const pmk_kernel_desc &, int64_t, int64_t, hipStream_t) { return no_gpu("launch_mix_vgrad"); }
int launch_mix_cov(pmk_query *, const pmk_kernel_desc &, hipStream_t) { return no_gpu("launch_mix_cov"); }
int launch_cov_trend(pmk_query *, hipStream_t) { return no_gpu("launch_cov_trend"); }
int launch_cov_trend_items(pmk_query *, hipStream_t) { return no_gpu("launch_cov_trend_items"); }
int launch_block_weights(pmk_query *, const pmk_kernel_desc &, hipStream_t) { return no_gpu("launch_block_weights"); }
int launch_block_heads(pmk_query *, hipStream_t) { return no_gpu("launch_block_heads"); }
int launch_block_aggregates(pmk_query *, int, unsigned long long *, int64_t *, hipStream_t) { return no_gpu("launch_block_aggregates"); }
int launch_block_reduce(pmk_query *, bool, int, hipStream_t) { return no_gpu("launch_block_reduce"); }
int launch_factor_cov(pmk_query *, int, hipStream_t) { return no_gpu("launch_factor_cov"); }
int launch_draw(pmk_query *, const pmk_kernel_desc &, const double *, int64_t, int64_t, double *, int64_t, hipStream_t)
{
    return no_gpu("launch_draw");
}
int launch_loo_scatter_multi(pmk_query *, const pmk_query *, int, int, const int32_t *, const int64_t *, hipStream_t)
{
    return no_gpu("launch_loo_scatter_multi");
}
int launch_export_requests(pmk_query *, int64_t, int64_t, double *, int32_t *, hipStream_t) { return no_gpu("launch_export_requests"); }
int launch_export_request_diag(pmk_query *, int64_t, int64_t, double *, hipStream_t) { return no_gpu("launch_export_request_diag"); }
int launch_export_results(pmk_query *, double *, double *, hipStream_t) { return no_gpu("launch_export_results"); }
int launch_explicit_items(pmk_query *, int *, hipStream_t) { return no_gpu("launch_explicit_items"); }
int launch_query_mean(const pmk_kernel_desc *, int, int, int64_t, const double *, int64_t, const double *, int64_t, const double *,
                      double *, hipStream_t) { return no_gpu("launch_query_mean"); }
int64_t exclusive_scan_i32_to_i64(const int32_t *, int64_t *, int64_t, void **, size_t *, hipStream_t) { return no_gpu("exclusive_scan"); }
int bsp_build_device(pmk_ctx *, int, int64_t, const double *, int, int, int, BspArrays &) { return no_gpu("bsp_build_device"); }
int bsp_assign_device(pmk_ctx *, const BspArrays &, int64_t, const double *, double, int64_t *, int64_t *, int64_t *, int64_t *)
{
    return no_gpu("bsp_assign_device");
}
int bsp_patch_index_device(pmk_ctx *, const BspArrays &, int64_t, const double *, double, int64_t *, int32_t **, double **)
{
    return no_gpu("bsp_patch_index_device");
}

}  // namespace pmk

extern "C" {
int pmk_selftest_gemm(pmk_ctx *, int, const double *, const double *, double *) { return pmk::no_gpu("pmk_selftest_gemm"); }
int pmk_selftest_trisolve(pmk_ctx *, const double *, const double *, const double *, double *) { return pmk::no_gpu("pmk_selftest_trisolve"); }
int pmk_selftest_mfma_peak(pmk_ctx *, double *) { return pmk::no_gpu("pmk_selftest_mfma_peak"); }
}

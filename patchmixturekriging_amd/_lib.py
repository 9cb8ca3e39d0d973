"""ctypes loader of libpmk_hip.so (the C ABI of include/pmk.h).

The library is the product: there is no CPU fallback.  If it cannot be built or loaded the import
of this module's `lib()` raises, and every operator of the package fails loudly.
"""
import ctypes as C
import os
import subprocess
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
SO_PATH = os.path.join(CSRC, "libpmk_hip.so")
_LIB = None


class PmkError(RuntimeError):
    pass


class KernelDesc(C.Structure):
    """pmk_kernel_desc of include/pmk.h"""
    _fields_ = [("family", C.c_int32), ("flags", C.c_int32), ("p", C.c_double * 4)]


def _build_jobs():
    """parallel compiles: MAX_JOBS if set, else the CPUs this process may run on, at most 16"""
    env = os.environ.get("MAX_JOBS", "")
    if env.isdigit() and int(env) > 0:
        return int(env)
    try:
        ncpu = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        ncpu = os.cpu_count() or 1
    return max(1, min(16, ncpu))


def build(force=False, jobs=None):
    """compile the HIP kernels for gfx950 in-tree (hipcc cross-compiles without a GPU); a failed build raises with the
    end of the compiler output"""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC)
            if f.endswith((".hip", ".cpp", ".h"))] + [
        os.path.join(_HERE, "..", "include", "pmk.h"), os.path.join(_HERE, "..", "include", "pmk_test.h")]
    stale = force or not os.path.exists(SO_PATH) or any(
        os.path.getmtime(s) > os.path.getmtime(SO_PATH) for s in srcs if os.path.exists(s))
    if stale:
        if not os.path.exists("/opt/rocm/bin/hipcc"):
            raise PmkError("libpmk_hip.so is missing or stale and hipcc is not available to build it")
        cmd = ["make", "-C", CSRC, "-j%d" % (jobs or _build_jobs()), "libpmk_hip.so"]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        out = r.stdout.decode(errors="replace")
        if r.returncode != 0:
            sys.stderr.write(out[-8000:])
            raise PmkError("building libpmk_hip.so failed (%s, exit %d):\n%s" % (" ".join(cmd), r.returncode, out[-4000:]))
    return SO_PATH


_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int64)
_i32p = C.POINTER(C.c_int32)
_bp = C.POINTER(C.c_uint8)
_kp = C.POINTER(KernelDesc)
_vp = C.c_void_p
_vpp = C.POINTER(C.c_void_p)
_dpp = C.POINTER(_dp)

# name -> (restype, argtypes): exactly the symbols declared in include/pmk.h and include/pmk_test.h
SIGNATURES = {
    "pmk_version": (C.c_int, []),
    "pmk_last_error": (C.c_char_p, []),
    "pmk_ctx_create": (C.c_int, [C.c_int, _vpp]),
    "pmk_ctx_set_stream": (C.c_int, [_vp, _vp]),
    "pmk_ctx_set_stream_null": (C.c_int, [_vp]),
    "pmk_ctx_synchronize": (C.c_int, [_vp]),
    "pmk_ctx_destroy": (None, [_vp]),
    "pmk_ctx_enable_timers": (C.c_int, [_vp, C.c_int]),
    "pmk_ctx_shader_clock": (C.c_int, [_vp, C.c_int, _dp]),
    "pmk_ctx_timer_ms": (C.c_int, [_vp, C.c_char_p, _dp]),
    "pmk_bsp_build": (C.c_int, [C.c_int, C.c_int64, _dp, C.c_int, C.c_int, C.c_int, _vpp]),
    "pmk_bsp_build_device": (C.c_int, [_vp, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_int, _vpp]),
    "pmk_bsp_from_hyperplanes": (C.c_int, [C.c_int, C.c_int, _dp, _dp, C.c_int, _vpp]),
    "pmk_bsp_destroy": (None, [_vp]),
    "pmk_bsp_dim": (C.c_int, [_vp]),
    "pmk_bsp_levels": (C.c_int, [_vp]),
    "pmk_bsp_dot_mode": (C.c_int, [_vp]),
    "pmk_bsp_num_leaves": (C.c_int64, [_vp]),
    "pmk_bsp_num_points": (C.c_int64, [_vp]),
    "pmk_bsp_arrays": (C.c_int, [_vp, _dp, _dp, _ip, _ip]),
    "pmk_bsp_assign": (C.c_int, [_vp, C.c_int64, _dp, C.c_double, _ip, _ip, _ip, _ip]),
    "pmk_bsp_assign_device": (C.c_int, [_vp, _vp, C.c_int64, C.c_void_p, C.c_double, _ip, _ip, _ip, _ip]),
    "pmk_bsp_findpartition": (C.c_int64, [_vp, _dp]),
    "pmk_bsp_neighbours": (C.c_int64, [_vp, _dp, C.c_double, C.c_double, C.c_int64, _ip, _dp, _dp, _bp]),
    "pmk_kernel_matrix": (C.c_int, [_vp, _kp, C.c_int, C.c_int64, _dp, C.c_int64, _dp, _dp, C.c_int64]),
    "pmk_model_create": (C.c_int, [_vp, C.c_int, C.c_int64, _ip, _dpp, _dpp, _vpp]),
    "pmk_model_create_ex": (C.c_int, [_vp, C.c_int, C.c_int64, _ip, _dpp, _dpp, C.c_int, _vpp]),
    "pmk_model_fit": (C.c_int, [_vp, _kp, C.c_double]),
    "pmk_model_info": (C.c_int, [_vp, _i32p]),
    "pmk_model_set_targets": (C.c_int, [_vp, _dpp]),
    "pmk_model_set_diag": (C.c_int, [_vp, C.c_void_p]),
    "pmk_query_set_diag": (C.c_int, [_vp, _dp]),
    "pmk_model_get": (C.c_int, [_vp, C.c_int64, C.c_int, _dp, C.c_int64]),
    "pmk_model_num_patches": (C.c_int64, [_vp]),
    "pmk_model_destroy": (None, [_vp]),
    "pmk_fit_batched": (C.c_int, [_vp, _kp, C.c_double, C.c_int, C.c_int64, _ip, _dpp, _dpp, _vpp, _dpp, _i32p]),
    "pmk_model_load": (C.c_int, [_vp, C.c_int, C.c_int64, _ip, _dpp, _dpp, _dpp, _ip, _vpp]),
    "pmk_model_queryinner": (C.c_int, [_vp, C.c_int64, _kp, C.c_int64, _dp, _dp, _dp]),
    "pmk_model_queryinner_ex": (C.c_int, [_vp, C.c_int64, _kp, C.c_int64, _dp, C.c_double, _dp, _dp]),
    "pmk_model_set_weights": (C.c_int, [_vp, _dpp]),
    "pmk_model_get_weights": (C.c_int, [_vp, _dpp]),
    "pmk_model_set_bsp": (C.c_int, [_vp, _vp, C.c_int64]),
    "pmk_query_create": (C.c_int, [_vp, C.c_int64, _dp, _vpp]),
    "pmk_query_create_items": (C.c_int, [_vp, C.c_int64, C.c_void_p, C.c_void_p, _vpp]),
    "pmk_query_export_requests": (C.c_int, [_vp, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    "pmk_query_export_results": (C.c_int, [_vp, C.c_void_p, C.c_void_p]),
    "pmk_query_export_request_diag": (C.c_int, [_vp, C.c_int64, C.c_int64, C.c_void_p]),
    "pmk_query_plan": (C.c_int, [_vp, C.c_double, C.c_double]),
    "pmk_query_counts": (C.c_int, [_vp, _ip, _ip, _ip]),
    "pmk_query_region_offsets": (C.c_int, [_vp, _ip]),
    "pmk_query_items": (C.c_int, [_vp, _kp]),
    "pmk_query_item_buffers": (C.c_int, [_vp, _vpp, _vpp]),
    "pmk_query_mix": (C.c_int, [_vp, _kp, C.c_int64, C.c_int64]),
    "pmk_comm_unique_id": (C.c_int, [C.c_void_p]),
    "pmk_comm_create": (C.c_int, [_vp, C.c_int, C.c_int, C.c_void_p, _vpp]),
    "pmk_comm_rank": (C.c_int, [_vp]),
    "pmk_comm_size": (C.c_int, [_vp]),
    "pmk_comm_destroy": (None, [_vp]),
    "pmk_shard_segments": (C.c_int, [_ip, C.c_int64, C.c_int, _ip, _ip]),
    "pmk_query_predict_sharded": (C.c_int, [_vp, _vp, _kp, _kp, C.c_double, C.c_double, _ip]),
    "pmk_query_predict_allgather": (C.c_int, [_vp, _vp, _kp, _kp, C.c_double, C.c_double, _ip]),
    "pmk_comm_last_bytes": (C.c_int, [_vp, _ip, _ip]),
    "pmk_query_fetch": (C.c_int, [_vp, _dp, _dp]),
    "pmk_query_debug": (C.c_int, [_vp, _ip, _ip, _ip, _dp, _dp, _dp, _dp]),
    "pmk_query_destroy": (None, [_vp]),
    "pmk_predict_mixture": (C.c_int, [_vp, _kp, _kp, C.c_int64, _dp, C.c_double, C.c_double, _dp, _dp]),
    "pmk_query_mean": (C.c_int, [_vp, _kp, C.c_int, C.c_int64, _dp, _dp, C.c_int64, _dp, _dp]),
    "pmk_query_mean_multi": (C.c_int, [_vp, _kp, C.c_int, C.c_int64, _dp, _dp, C.c_int64, _dp, _dp]),
    "pmk_model_set_targets_multi": (C.c_int, [_vp, C.c_int, _dpp, _ip]),
    "pmk_model_solve_multi": (C.c_int, [_vp]),
    "pmk_model_get_weights_multi": (C.c_int, [_vp, _dpp, _ip]),
    "pmk_query_items_multi": (C.c_int, [_vp, _kp, C.c_int]),
    "pmk_query_mix_multi": (C.c_int, [_vp, _kp, C.c_int64, C.c_int64]),
    "pmk_query_fetch_multi": (C.c_int, [_vp, _dp, C.c_int64, _dp]),
    "pmk_predict_mixture_multi": (C.c_int, [_vp, _kp, _kp, C.c_int64, _dp, C.c_double, C.c_double, _dp, C.c_int64, _dp]),
    "pmk_model_evidence": (C.c_int, [_vp, _dp, _dp]),
    "pmk_model_evidence_multi": (C.c_int, [_vp, _dp, _dp]),
    "pmk_model_loo": (C.c_int, [_vp]),
    "pmk_model_get_loo": (C.c_int, [_vp, _dpp, _dpp]),
    "pmk_model_get_loo_multi": (C.c_int, [_vp, _dpp, _ip, _dpp]),
    "pmk_query_items_loo": (C.c_int, [_vp, C.c_int, _ip, _ip]),
    "pmk_predict_mixture_loo": (C.c_int, [_vp, _kp, _dp, C.c_double, C.c_double, C.c_int, _dp, _dp]),
    "pmk_query_items_loo_multi": (C.c_int, [_vp, C.c_int, C.c_int, _ip, _ip]),
    "pmk_predict_mixture_loo_multi": (C.c_int, [_vp, _kp, _dp, C.c_double, C.c_double, C.c_int, _dp, C.c_int64, _dp]),
    "pmk_query_get_items_multi": (C.c_int, [_vp, _dp, C.c_int64, _dp]),
    "pmk_model_set_trend": (C.c_int, [_vp, C.c_int]),
    "pmk_model_get_trend": (C.c_int, [_vp, C.POINTER(C.c_int), _dp, _dp]),
    "pmk_model_trend_info": (C.c_int, [_vp, _i32p]),
    "pmk_model_fit_patches": (C.c_int, [_vp, _kp, _dp]),
    "pmk_model_set_kernels": (C.c_int, [_vp, _kp]),
    "pmk_model_get_hyper": (C.c_int, [_vp, _kp, _dp]),
    "pmk_query_items_fitted": (C.c_int, [_vp]),
    "pmk_query_items_multi_fitted": (C.c_int, [_vp, C.c_int]),
    "pmk_predict_mixture_fitted": (C.c_int, [_vp, _kp, C.c_int64, _dp, C.c_double, C.c_double, _dp, _dp]),
    "pmk_predict_mixture_multi_fitted": (C.c_int, [_vp, _kp, C.c_int64, _dp, C.c_double, C.c_double, _dp, C.c_int64, _dp]),
    "pmk_model_create_from_bsp": (C.c_int, [_vp, _vp, C.c_int64, C.c_void_p, C.c_void_p, C.c_double, C.c_int64, C.c_int64,
                                            C.c_int, _vpp]),
    "pmk_model_patch_index": (C.c_int, [_vp, _ip, _ip, _ip]),
    "pmk_model_set_targets_global": (C.c_int, [_vp, C.c_void_p]),
    "pmk_model_set_targets_multi_global": (C.c_int, [_vp, C.c_int, C.c_void_p, C.c_int64]),
    "pmk_model_set_diag_global": (C.c_int, [_vp, C.c_void_p]),
    "pmk_query_fetch_dev": (C.c_int, [_vp, C.c_void_p, C.c_void_p]),
    "pmk_query_fetch_multi_dev": (C.c_int, [_vp, C.c_void_p, C.c_int64, C.c_void_p]),
    "pmk_query_items_grad": (C.c_int, [_vp, _kp]),
    "pmk_query_mix_grad": (C.c_int, [_vp, _kp, C.c_int64, C.c_int64]),
    "pmk_query_fetch_grad": (C.c_int, [_vp, _dp, C.c_int64]),
    "pmk_query_fetch_grad_dev": (C.c_int, [_vp, C.c_void_p, C.c_int64]),
    "pmk_query_get_items_grad": (C.c_int, [_vp, _dp, C.c_int64, _i32p]),
    "pmk_predict_mixture_grad_fitted": (C.c_int, [_vp, _kp, C.c_int64, _dp, C.c_double, C.c_double, _dp, C.c_int64, _dp,
                                                  C.c_int64]),
    "pmk_query_items_vgrad": (C.c_int, [_vp, _kp]),
    "pmk_query_mix_vgrad": (C.c_int, [_vp, _kp, C.c_int64, C.c_int64]),
    "pmk_query_fetch_vgrad": (C.c_int, [_vp, _dp, C.c_int64]),
    "pmk_query_fetch_vgrad_dev": (C.c_int, [_vp, C.c_void_p, C.c_int64]),
    "pmk_query_get_items_vgrad": (C.c_int, [_vp, _dp, C.c_int64]),
    "pmk_predict_mixture_vgrad_fitted": (C.c_int, [_vp, _kp, C.c_int64, _dp, C.c_double, C.c_double, _dp, C.c_int64, _dp,
                                                   _dp, C.c_int64, _dp, C.c_int64]),
    "pmk_query_items_cov": (C.c_int, [_vp, _kp]),
    "pmk_query_mix_cov": (C.c_int, [_vp, _kp]),
    "pmk_query_fetch_cov": (C.c_int, [_vp, _dp, C.c_int64]),
    "pmk_query_fetch_cov_dev": (C.c_int, [_vp, C.c_void_p, C.c_int64]),
    "pmk_query_get_items_cov": (C.c_int, [_vp, C.c_int64, _ip, _i32p, _dp, C.c_int64]),
    "pmk_predict_mixture_cov_fitted": (C.c_int, [_vp, _kp, C.c_int64, _dp, C.c_double, C.c_double, _dp, _dp, _dp,
                                                 C.c_int64]),
    "pmk_query_items_cov_multi": (C.c_int, [_vp, _kp]),
    "pmk_query_items_cov_blocks": (C.c_int, [_vp, _kp, C.c_int]),
    "pmk_query_factor_cov": (C.c_int, [_vp, _dp]),
    "pmk_query_factor_info": (C.c_int, [_vp, _i32p, _dp]),
    "pmk_query_get_items_cov_factor": (C.c_int, [_vp, C.c_int64, _ip, _dp, C.c_int64]),
    "pmk_query_draw": (C.c_int, [_vp, _kp, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]),
    "pmk_predict_mixture_cov_multi_fitted": (C.c_int, [_vp, _kp, C.c_int64, _dp, C.c_double, C.c_double, _dp, C.c_int64,
                                                       _dp, _dp, C.c_int64]),
    "pmk_query_items_block": (C.c_int, [_vp, _kp, _kp, C.c_int64, _i32p, _dp, C.c_int]),
    "pmk_query_fetch_block": (C.c_int, [_vp, _dp, C.c_int64, _dp]),
    "pmk_query_fetch_block_dev": (C.c_int, [_vp, C.c_void_p, C.c_int64, C.c_void_p]),
    "pmk_query_get_items_block": (C.c_int, [_vp, _ip, _i32p, _i32p, _ip, _i32p, _dp, _dp, _dp, _dp]),
    "pmk_predict_mixture_block_fitted": (C.c_int, [_vp, _kp, C.c_int64, _dp, C.c_double, C.c_double, C.c_int64, _i32p, _dp,
                                                   _dp, C.c_int64, _dp]),
    "pmk_model_capacity": (C.c_int, [_vp, _ip]),
    "pmk_model_append": (C.c_int, [_vp, C.c_int64, _dp, _dp, _dp, _i32p, _ip]),
    "pmk_model_removable": (C.c_int, [_vp, _ip]),
    "pmk_model_remove": (C.c_int, [_vp, C.c_int64, _i32p, _ip]),
    "pmk_model_reserve": (C.c_int, [_vp, _ip]),
    # include/pmk_test.h
    "pmk_selftest_gemm": (C.c_int, [_vp, C.c_int, _dp, _dp, _dp]),
    "pmk_selftest_trisolve": (C.c_int, [_vp, _dp, _dp, _dp, _dp]),
    "pmk_selftest_mfma_peak": (C.c_int, [_vp, _dp]),
    "pmk_test_comm_force_exchange": (C.c_int, [_vp, C.c_int]),
    "pmk_test_model_set_split": (C.c_int, [_vp, C.c_int]),
    "pmk_test_model_packed": (C.c_int, [_vp, C.c_int64, C.c_int, _ip, _dp]),
    "pmk_test_model_buffers": (C.c_int, [_vp, _ip, _ip, _ip]),
    "pmk_test_gemm_buf_extent_ok": (C.c_int, [C.c_int64, C.c_int64, C.c_int, C.c_int]),
    "pmk_test_step_gemm_rule": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
}


def lib():
    """load (building if needed) libpmk_hip.so; raises PmkError when that is impossible"""
    global _LIB
    if _LIB is not None:
        return _LIB
    try:
        # share torch's HIP runtime when torch is (or will be) in the process: both must use one
        # libamdhip64 for streams and device pointers to be interchangeable
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch is plumbing, not a requirement
        pass
    path = os.environ.get("PMK_LIB") or build()       # PMK_LIB: load an A/B variant build instead
    try:
        L = C.CDLL(path, mode=C.RTLD_GLOBAL)
    except OSError as e:
        raise PmkError("cannot load %s: %s" % (path, e))
    for name, (res, args) in SIGNATURES.items():
        try:
            f = getattr(L, name)
        except AttributeError:
            raise PmkError("libpmk_hip.so does not export %s" % name)
        f.restype = res
        f.argtypes = args
    _LIB = L
    return L


def check(rc, what="pmk call"):
    """negative status -> exception with the library's message"""
    if rc < 0:
        raise PmkError("%s failed (%d): %s" % (what, rc, lib().pmk_last_error().decode()))
    return rc

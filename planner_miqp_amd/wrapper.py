"""Python mirror of miqp::planner::cplex::CplexWrapper (src/cplex_wrapper.hpp:61-275) over libmiqp_gpu.so.

Method names, argument meaning and error behaviour follow the reference class so that parity tests read
like test/cplex_wrapper_test.cc.  All solving happens in the HIP library; this file only marshals."""
import ctypes as C
import enum
import os
import subprocess

import numpy as np

# (four concurrent launches per round + the null stream: see miqp_gpu.hip - effective when set before the process's first HIP call)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

from .ctypes_types import (AsNodeC, Certificate, CertificateC, FixedResultC, ModelParameters, ModelParamsC, PoolCarryC, PoolExploreC, PoolImproveC, RawResults, RawResultsC, SolutionPropertiesC, SolverOptsC,
                           c_double_p)

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None
# miqp_exchange_fn (include/miqp_gpu.h): int (*)(void* user, int op, void* buf, int count, int root)
EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int)


def library_path():
    return os.environ.get("MIQP_GPU_LIB", os.path.join(_HERE, "libmiqp_gpu.so"))


def build_library(force=False):
    """hipcc --offload-arch=gfx950 build of the in-tree shared library (cross-compiles without a GPU)."""
    src = os.path.join(_HERE, "csrc", "miqp_gpu.hip")
    out = library_path()
    deps = [os.path.join(_HERE, "csrc", f) for f in os.listdir(os.path.join(_HERE, "csrc"))]
    deps += [os.path.join(_HERE, "..", "include", f) for f in ("miqp_gpu.h", "miqp_types.h")]
    if not force and os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps):
        return out
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    # the value-changing fast-math switches apply to the DEVICE code only: the host side of the translation unit holds the
    # restatement of RoundWithPrecision (host_inst.hpp::round_dec), which has to divide exactly as the reference does
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-fno-math-errno", "-fno-trapping-math",
           "-Xarch_device", "-freciprocal-math", "-Xarch_device", "-fno-signed-zeros",
           "-fPIC", "-shared", "-std=c++17", "-o", out, src]
    subprocess.check_call(cmd)
    return out


def load_library():
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise RuntimeError("libmiqp_gpu.so is not built (run __graft_entry__.build()); the solver has no CPU fallback")
    L = C.CDLL(path)
    vp = C.c_void_p
    L.miqp_solver_create.restype = vp; L.miqp_solver_create.argtypes = [C.POINTER(SolverOptsC)]
    L.miqp_solver_destroy.restype = None; L.miqp_solver_destroy.argtypes = [vp]
    L.miqp_solver_set_params.restype = C.c_int; L.miqp_solver_set_params.argtypes = [vp, C.POINTER(ModelParamsC)]
    L.miqp_solver_load_dat.restype = C.c_int; L.miqp_solver_load_dat.argtypes = [vp, C.c_char_p]
    L.miqp_solver_override_settings.restype = C.c_int; L.miqp_solver_override_settings.argtypes = [vp, C.c_double, C.c_double]
    L.miqp_solver_set_warmstart.restype = C.c_int; L.miqp_solver_set_warmstart.argtypes = [vp, C.POINTER(RawResultsC), C.c_int]
    L.miqp_solver_solve.restype = C.c_int; L.miqp_solver_solve.argtypes = [vp, C.c_double]
    L.miqp_solver_solve_batch.restype = C.c_int; L.miqp_solver_solve_batch.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(C.c_int)]
    L.miqp_solver_solve_stream.restype = C.c_int; L.miqp_solver_solve_stream.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.miqp_solver_solve_batch_multi.restype = C.c_int; L.miqp_solver_solve_batch_multi.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.miqp_solver_raw_sizes.restype = C.c_int; L.miqp_solver_raw_sizes.argtypes = [vp, C.POINTER(C.c_int)]
    L.miqp_solver_lift_tables.restype = C.c_int; L.miqp_solver_lift_tables.argtypes = [vp, c_double_p, C.c_int]
    L.miqp_solver_solve_split.restype = C.c_int; L.miqp_solver_solve_split.argtypes = [vp, C.c_double, C.c_int, C.c_int, EXCHANGE_FN, vp]
    L.miqp_solver_solve_split_rccl.restype = C.c_int; L.miqp_solver_solve_split_rccl.argtypes = [vp, C.c_double]
    L.miqp_solver_split_roots.restype = C.c_int
    L.miqp_solver_split_roots.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.miqp_comm_unique_id.restype = C.c_int; L.miqp_comm_unique_id.argtypes = [C.c_char_p]
    L.miqp_comm_init.restype = C.c_int; L.miqp_comm_init.argtypes = [C.c_int, C.c_int, C.c_char_p, C.c_int]
    L.miqp_comm_finalize.restype = C.c_int; L.miqp_comm_finalize.argtypes = []
    L.miqp_comm_selftest.restype = C.c_int; L.miqp_comm_selftest.argtypes = [EXCHANGE_FN, vp, C.c_int, C.c_int]
    L.miqp_solver_get_results.restype = C.c_int; L.miqp_solver_get_results.argtypes = [vp, C.POINTER(RawResultsC)]
    L.miqp_solver_materialize_results.restype = C.c_int; L.miqp_solver_materialize_results.argtypes = [C.POINTER(vp), C.c_int, C.c_int]
    L.miqp_solver_get_properties.restype = C.c_int; L.miqp_solver_get_properties.argtypes = [vp, C.POINTER(SolutionPropertiesC)]
    L.miqp_solver_get_dims.restype = C.c_int; L.miqp_solver_get_dims.argtypes = [vp, C.POINTER(C.c_int)]
    L.miqp_solver_export_lp.restype = C.c_int; L.miqp_solver_export_lp.argtypes = [vp, C.c_char_p]
    for fn in (L.miqp_solver_write_dat, L.miqp_solver_write_solution, L.miqp_solver_write_mst, L.miqp_solver_read_mst):
        fn.restype = C.c_int; fn.argtypes = [vp, C.c_char_p]
    L.miqp_solver_solve_fixed.restype = C.c_int
    L.miqp_solver_solve_fixed.argtypes = [vp, C.POINTER(RawResultsC), C.POINTER(RawResultsC), C.POINTER(C.c_double), C.POINTER(C.c_int)]
    L.miqp_solver_last_timing.restype = C.c_int; L.miqp_solver_last_timing.argtypes = [vp, C.POINTER(C.c_double)]
    L.miqp_solver_last_setup.restype = C.c_int; L.miqp_solver_last_setup.argtypes = [vp, C.POINTER(C.c_double)]
    L.miqp_solver_last_active_set.restype = C.c_int; L.miqp_solver_last_active_set.argtypes = [vp, C.POINTER(C.c_double)]
    L.miqp_solver_last_fixed_route.restype = C.c_int; L.miqp_solver_last_fixed_route.argtypes = [vp]
    L.miqp_solver_last_error.restype = C.c_char_p; L.miqp_solver_last_error.argtypes = [vp]
    L.miqp_solver_last_admission.restype = C.c_int; L.miqp_solver_last_admission.argtypes = [vp, C.POINTER(C.c_double)]
    L.miqp_solver_certify.restype = C.c_int; L.miqp_solver_certify.argtypes = [vp, C.POINTER(RawResultsC), C.POINTER(CertificateC)]
    L.miqp_solver_certify_batch.restype = C.c_int; L.miqp_solver_certify_batch.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(CertificateC)]
    L.miqp_gpu_certificate_size.restype = C.c_int; L.miqp_gpu_certificate_size.argtypes = []
    L.miqp_gpu_certify_last_timing.restype = C.c_int; L.miqp_gpu_certify_last_timing.argtypes = [C.POINTER(C.c_double)]
    L.miqp_gpu_has_active_set.restype = C.c_int; L.miqp_gpu_has_active_set.argtypes = [C.c_int, C.c_int]
    L.miqp_solver_launch_plan.restype = C.c_int
    L.miqp_solver_launch_plan.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_double, C.c_int, C.POINTER(C.c_int), C.c_int]
    L.miqp_solver_solve_fixed_batch.restype = C.c_int
    L.miqp_solver_solve_fixed_batch.argtypes = [vp, C.POINTER(C.POINTER(RawResultsC)), C.c_int, C.POINTER(FixedResultC), C.POINTER(C.c_int)]
    L.miqp_solver_fixed_batch_record.restype = C.c_int; L.miqp_solver_fixed_batch_record.argtypes = [vp, C.c_int, C.POINTER(RawResultsC)]
    L.miqp_gpu_fixed_result_size.restype = C.c_int; L.miqp_gpu_fixed_result_size.argtypes = []
    L.miqp_gpu_fixed_batch_chunk.restype = C.c_int; L.miqp_gpu_fixed_batch_chunk.argtypes = []
    L.miqp_solver_solve_fixed_as.restype = C.c_int
    L.miqp_solver_solve_fixed_as.argtypes = [vp, C.POINTER(C.POINTER(RawResultsC)), C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_double), C.POINTER(AsNodeC), C.POINTER(C.c_ulonglong)]
    L.miqp_solver_fixed_as_record.restype = C.c_int; L.miqp_solver_fixed_as_record.argtypes = [vp, C.c_int, C.POINTER(RawResultsC)]
    L.miqp_gpu_as_node_size.restype = C.c_int; L.miqp_gpu_as_node_size.argtypes = []
    L.miqp_solver_set_pool.restype = C.c_int; L.miqp_solver_set_pool.argtypes = [vp, C.c_int]
    L.miqp_solver_pool_count.restype = C.c_int; L.miqp_solver_pool_count.argtypes = [vp]
    L.miqp_solver_pool_found.restype = C.c_int; L.miqp_solver_pool_found.argtypes = [vp, c_double_p, C.c_int]
    L.miqp_solver_pool_solve.restype = C.c_int; L.miqp_solver_pool_solve.argtypes = [vp, C.POINTER(FixedResultC), C.c_int]
    L.miqp_solver_pool_record.restype = C.c_int; L.miqp_solver_pool_record.argtypes = [vp, C.c_int, C.POINTER(RawResultsC)]
    L.miqp_gpu_pool_max.restype = C.c_int; L.miqp_gpu_pool_max.argtypes = []
    L.miqp_solver_set_pool_filter.restype = C.c_int; L.miqp_solver_set_pool_filter.argtypes = [vp, C.c_int]
    L.miqp_gpu_pool_signature.restype = C.c_int
    L.miqp_gpu_pool_signature.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_byte), C.POINTER(C.c_byte), C.c_int]
    L.miqp_solver_pool_signature.restype = C.c_int; L.miqp_solver_pool_signature.argtypes = [vp, C.POINTER(RawResultsC), C.c_int, C.POINTER(C.c_byte), C.c_int]
    L.miqp_solver_pool_found_decisions.restype = C.c_int; L.miqp_solver_pool_found_decisions.argtypes = [vp, C.c_int, C.POINTER(C.c_byte), C.c_int]
    L.miqp_gpu_pool_moves.restype = C.c_int
    L.miqp_gpu_pool_moves.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_byte), C.POINTER(C.c_int), C.c_int]
    L.miqp_gpu_pool_moves_max.restype = C.c_int; L.miqp_gpu_pool_moves_max.argtypes = []
    L.miqp_gpu_pool_improve_size.restype = C.c_int; L.miqp_gpu_pool_improve_size.argtypes = []
    L.miqp_solver_solve_decisions.restype = C.c_int
    L.miqp_solver_solve_decisions.argtypes = [vp, C.POINTER(C.c_byte), C.c_int, C.POINTER(FixedResultC), C.POINTER(C.c_int)]
    L.miqp_solver_pool_improve.restype = C.c_int; L.miqp_solver_pool_improve.argtypes = [vp, C.c_int, C.POINTER(PoolImproveC), C.c_int]
    L.miqp_solver_pool_improve_multi.restype = C.c_int
    L.miqp_solver_pool_improve_multi.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.POINTER(PoolImproveC), C.c_int, C.POINTER(C.c_int)]
    L.miqp_gpu_pool_improve_plan.restype = C.c_int
    L.miqp_gpu_pool_improve_plan.argtypes = [C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), C.c_int]
    L.miqp_gpu_pool_jumps.restype = C.c_int
    L.miqp_gpu_pool_jumps.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_byte), C.POINTER(C.c_int), C.c_int]
    L.miqp_gpu_pool_explore_size.restype = C.c_int; L.miqp_gpu_pool_explore_size.argtypes = []
    L.miqp_solver_pool_explore.restype = C.c_int; L.miqp_solver_pool_explore.argtypes = [vp, C.c_int, C.c_double, C.POINTER(PoolExploreC), C.c_int]
    L.miqp_solver_pool_explore_distinct.restype = C.c_int; L.miqp_solver_pool_explore_distinct.argtypes = [vp, C.c_int, C.c_double, C.POINTER(PoolExploreC), C.c_int]
    L.miqp_solver_canonical_decisions.restype = C.c_int
    L.miqp_solver_canonical_decisions.argtypes = [vp, C.POINTER(C.c_byte), C.c_int, C.POINTER(FixedResultC), C.POINTER(C.c_byte), C.POINTER(C.c_int)]
    L.miqp_solver_settle_decisions.restype = C.c_int
    L.miqp_solver_settle_decisions.argtypes = [vp, C.POINTER(C.c_byte), C.c_int, C.POINTER(FixedResultC), C.POINTER(C.c_byte), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.miqp_solver_pool_explore_settled.restype = C.c_int; L.miqp_solver_pool_explore_settled.argtypes = [vp, C.c_int, C.c_double, C.POINTER(PoolExploreC), C.c_int]
    L.miqp_solver_pool_explore_multi.restype = C.c_int
    L.miqp_solver_pool_explore_multi.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_double, C.POINTER(PoolExploreC), C.c_int, C.POINTER(C.c_int)]
    L.miqp_gpu_pool_explore_plan.restype = C.c_int
    L.miqp_gpu_pool_explore_plan.argtypes = [C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), C.c_int]
    L.miqp_gpu_pool_explore_multi_last.restype = None; L.miqp_gpu_pool_explore_multi_last.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.miqp_gpu_pool_settle_passes.restype = C.c_int; L.miqp_gpu_pool_settle_passes.argtypes = []
    L.miqp_solver_canonical_labels.restype = C.c_int
    L.miqp_solver_canonical_labels.argtypes = [vp, C.POINTER(C.c_byte), c_double_p, C.c_int, C.c_int, C.POINTER(C.c_byte)]
    L.miqp_solver_solve_fixed_multi.restype = C.c_int
    L.miqp_solver_solve_fixed_multi.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(C.POINTER(RawResultsC)), C.POINTER(C.c_int), C.POINTER(FixedResultC), C.POINTER(C.c_int)]
    L.miqp_solver_pool_solve_multi.restype = C.c_int
    L.miqp_solver_pool_solve_multi.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(FixedResultC), C.c_int, C.POINTER(C.c_int)]
    L.miqp_gpu_pool_shift.restype = C.c_int
    L.miqp_gpu_pool_shift.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_byte), C.POINTER(C.c_byte), C.c_int]
    L.miqp_solver_pool_carry_maps.restype = C.c_int; L.miqp_solver_pool_carry_maps.argtypes = [vp, vp, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), C.c_int]
    L.miqp_solver_pool_carry.restype = C.c_int; L.miqp_solver_pool_carry.argtypes = [vp, vp, C.c_int, C.c_double, C.POINTER(PoolCarryC), C.c_int]
    L.miqp_gpu_pool_carry_size.restype = C.c_int; L.miqp_gpu_pool_carry_size.argtypes = []
    L.miqp_gpu_pool_carry_last.restype = None; L.miqp_gpu_pool_carry_last.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.miqp_solver_pool_carry_multi.restype = C.c_int
    L.miqp_solver_pool_carry_multi.argtypes = [C.POINTER(vp), C.POINTER(vp), C.c_int, C.c_int, C.c_double, C.POINTER(PoolCarryC), C.c_int, C.POINTER(C.c_int)]
    L.miqp_gpu_pool_carry_multi_last.restype = None; L.miqp_gpu_pool_carry_multi_last.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.miqp_solver_set_pool_starts.restype = C.c_int; L.miqp_solver_set_pool_starts.argtypes = [vp, C.c_int]
    L.miqp_solver_pool_starts_last.restype = C.c_int; L.miqp_solver_pool_starts_last.argtypes = [vp, C.POINTER(C.c_int), C.c_int]
    L.miqp_solver_get_pool_starts.restype = C.c_int; L.miqp_solver_get_pool_starts.argtypes = [vp]
    if L.miqp_gpu_pool_carry_size() != C.sizeof(PoolCarryC):
        raise RuntimeError("libmiqp_gpu.so and ctypes_types.PoolCarryC disagree on miqp_pool_carry_c (%d / %d bytes): rebuild the library"
                           % (L.miqp_gpu_pool_carry_size(), C.sizeof(PoolCarryC)))
    if L.miqp_gpu_as_node_size() != C.sizeof(AsNodeC):
        raise RuntimeError("libmiqp_gpu.so and ctypes_types.AsNodeC disagree on miqp_as_node_c (%d / %d bytes): rebuild the library"
                           % (L.miqp_gpu_as_node_size(), C.sizeof(AsNodeC)))
    if L.miqp_gpu_fixed_result_size() != C.sizeof(FixedResultC):
        raise RuntimeError("libmiqp_gpu.so and ctypes_types.FixedResultC disagree on miqp_fixed_result_c (%d / %d bytes): rebuild the library"
                           % (L.miqp_gpu_fixed_result_size(), C.sizeof(FixedResultC)))
    if L.miqp_gpu_pool_improve_size() != C.sizeof(PoolImproveC):
        raise RuntimeError("libmiqp_gpu.so and ctypes_types.PoolImproveC disagree on miqp_pool_improve_c (%d / %d bytes): rebuild the library"
                           % (L.miqp_gpu_pool_improve_size(), C.sizeof(PoolImproveC)))
    if L.miqp_gpu_pool_explore_size() != C.sizeof(PoolExploreC):
        raise RuntimeError("libmiqp_gpu.so and ctypes_types.PoolExploreC disagree on miqp_pool_explore_c (%d / %d bytes): rebuild the library"
                           % (L.miqp_gpu_pool_explore_size(), C.sizeof(PoolExploreC)))
    L.miqp_gpu_version.restype = C.c_char_p
    _LIB = L
    return L


EXPORTED_SYMBOLS = ["miqp_solver_create", "miqp_solver_destroy", "miqp_solver_set_params", "miqp_solver_load_dat",
                    "miqp_solver_override_settings", "miqp_solver_set_warmstart", "miqp_solver_solve",
                    "miqp_solver_solve_batch", "miqp_solver_get_results", "miqp_solver_get_properties",
                    "miqp_solver_get_dims", "miqp_solver_export_lp", "miqp_solver_solve_fixed",
                    "miqp_solver_last_timing", "miqp_solver_last_active_set", "miqp_solver_last_setup", "miqp_solver_last_error", "miqp_solver_last_admission", "miqp_gpu_version", "miqp_solver_write_dat", "miqp_solver_write_solution",
                    "miqp_solver_write_mst", "miqp_solver_read_mst", "miqp_fraction_parameters", "miqp_mean_angles",
                    "miqp_limits_per_region", "miqp_calculate_region_idx", "miqp_reserve_neighbor_regions",
                    "miqp_calculate_possible_regions", "miqp_calculate_warmstart", "miqp_plan",
                    "miqp_solver_solve_batch_multi", "miqp_solver_raw_sizes", "miqp_solver_lift_tables", "miqp_reference_trajectory", "miqp_update_car", "miqp_fitting_polynomial_parameters",
                    "miqp_solver_solve_split", "miqp_solver_solve_split_rccl", "miqp_solver_split_roots", "miqp_comm_unique_id",
                    "miqp_comm_init", "miqp_comm_finalize", "miqp_comm_selftest", "miqp_solver_solve_stream", "miqp_solver_materialize_results",
                    "miqp_initial_pose_check", "miqp_select_environment", "miqp_obstacle_intersects_environment", "miqp_obstacles_roi", "miqp_bark_trajectory", "miqp_obstacle_intersects_environment_roi", "miqp_environment_warmstart",
                    "miqp_solver_certify", "miqp_solver_certify_batch", "miqp_gpu_certificate_size", "miqp_gpu_certify_last_timing",
                    "miqp_gpu_has_active_set", "miqp_solver_last_fixed_route", "miqp_solver_launch_plan",
                    "miqp_solver_solve_fixed_batch", "miqp_solver_fixed_batch_record", "miqp_gpu_fixed_result_size", "miqp_gpu_fixed_batch_chunk",
                    "miqp_solver_solve_fixed_as", "miqp_solver_fixed_as_record", "miqp_gpu_as_node_size",
                    "miqp_solver_set_pool", "miqp_solver_pool_count", "miqp_solver_pool_found", "miqp_solver_pool_solve", "miqp_solver_pool_record", "miqp_gpu_pool_max",
                    "miqp_solver_solve_fixed_multi", "miqp_solver_pool_solve_multi",
                    "miqp_solver_set_pool_filter", "miqp_gpu_pool_signature", "miqp_solver_pool_signature", "miqp_solver_pool_found_decisions",
                    "miqp_gpu_pool_moves", "miqp_gpu_pool_moves_max", "miqp_gpu_pool_improve_size", "miqp_solver_solve_decisions", "miqp_solver_pool_improve",
                    "miqp_solver_pool_improve_multi", "miqp_gpu_pool_improve_plan",
                    "miqp_gpu_pool_jumps", "miqp_gpu_pool_explore_size", "miqp_solver_pool_explore",
                    "miqp_solver_canonical_decisions", "miqp_solver_canonical_labels", "miqp_solver_pool_explore_distinct",
                    "miqp_solver_settle_decisions", "miqp_solver_pool_explore_settled", "miqp_gpu_pool_settle_passes",
                    "miqp_solver_pool_explore_multi", "miqp_gpu_pool_explore_plan", "miqp_gpu_pool_explore_multi_last",
                    "miqp_gpu_pool_shift", "miqp_solver_pool_carry_maps", "miqp_solver_pool_carry", "miqp_gpu_pool_carry_size", "miqp_gpu_pool_carry_last",
                    "miqp_solver_pool_carry_multi", "miqp_gpu_pool_carry_multi_last",
                    "miqp_solver_set_pool_starts", "miqp_solver_pool_starts_last", "miqp_solver_get_pool_starts"]


# a row of CplexWrapper.launchPlan (NodeLaunch in csrc/miqp_gpu.hip)
LAUNCH_PLAN_FIELDS = ("kernel", "stream", "grid", "lds", "ovf_mode", "cls_take", "as_split", "skip_probes", "bounce", "work", "from_ovf2", "bufs", "zero")


# miqp_fixed_result_c as a numpy record
_FIXED_RESULT_DTYPE = np.dtype([("status", "<i4"), ("route", "<i4"), ("iterations", "<i4"), ("reserved", "<i4"), ("objective", "<f8"), ("violation", "<f8")])


# the families of CplexWrapper.setSolutionPoolFilter (MIQP_POOL_BY_* of include/miqp_types.h): a bit set
POOL_BY_REGION, POOL_BY_ENVIRONMENT, POOL_BY_OBSTACLE, POOL_BY_CAR_CAR, POOL_EXACT_TIMING = 1, 2, 4, 8, 16


def _decision_len(cars, steps, obstacles):
    """D: the decision bytes of a fix record (regions, environment pieces, obstacle edges, car/car alternatives)"""
    return cars * steps * 6 + cars * obstacles * steps * 5 + cars * (cars - 1) // 2 * steps * 4


def pool_signature(cars, steps, obstacles, families, decisions):
    """the signature of a record's D decision bytes under ``families`` (miqp_gpu_pool_signature; int8 array of D bytes): two records are the same
    entry of a filtered pool when their signatures are equal.  A pure function on bytes: needs no wrapper and no device.  Raises ValueError
    where the library refuses the arguments."""
    d = np.ascontiguousarray(decisions, dtype=np.int8)
    D = _decision_len(int(cars), int(steps), int(obstacles))
    if d.ndim != 1 or d.size < D or D <= 0:
        raise ValueError("%d decision bytes given, the shape has %d" % (d.size, D))
    out = np.empty(D, dtype=np.int8)
    bp = C.POINTER(C.c_byte)
    rc = load_library().miqp_gpu_pool_signature(int(cars), int(steps), int(obstacles), int(families), d.ctypes.data_as(bp), out.ctypes.data_as(bp), D)
    if rc != D:
        raise ValueError("miqp_gpu_pool_signature refused the arguments (%d)" % rc)
    return out


def pool_moves_max():
    """most moves pool_moves and CplexWrapper.improveSolutionPool take of one record (a constant of the built library; needs no device)"""
    return int(load_library().miqp_gpu_pool_moves_max())


def pool_moves(cars, steps, obstacles, families, decisions):
    """the timing moves of a record's D decision bytes that keep its signature under ``families`` (miqp_gpu_pool_moves): an int32 array [n, 4] of
    (first, stride, count, value) - the bytes decisions[first + k * stride], k < count, take value - in the order site, change point, later by one,
    later by two, earlier by one, earlier by two; at most pool_moves_max().  A pure function on bytes: needs no wrapper and no device.  Raises
    ValueError where the library refuses the arguments (families outside 1 .. 15)."""
    d = np.ascontiguousarray(decisions, dtype=np.int8)
    D = _decision_len(int(cars), int(steps), int(obstacles))
    if d.ndim != 1 or d.size < D or D <= 0:
        raise ValueError("%d decision bytes given, the shape has %d" % (d.size, D))
    cap = pool_moves_max()
    out = np.empty((cap, 4), dtype=np.int32)
    n = load_library().miqp_gpu_pool_moves(int(cars), int(steps), int(obstacles), int(families), d.ctypes.data_as(C.POINTER(C.c_byte)),
                                           out.ctypes.data_as(C.POINTER(C.c_int)), cap)
    if n < 0:
        raise ValueError("miqp_gpu_pool_moves refused the arguments (%d)" % n)
    return out[:n].copy()


def pool_jumps(cars, steps, obstacles, max_lines, families, decisions):
    """the jumps of a record's D decision bytes to neighbouring manoeuvre classes under ``families`` (miqp_gpu_pool_jumps): an int32 array [n, 4]
    of (first, stride, count, value) as pool_moves returns them - group jumps (all five points of a (car, obstacle), all four group-sites of a car
    pair, over a run of steps with constant decided bytes) in front of the jumps of single sites, every alternative 0 .. max_lines - 1 of an
    obstacle edge or 0 .. 3 of a car/car byte; every one changes pool_signature; at most pool_moves_max().  A pure function on bytes: needs no
    wrapper and no device.  Raises ValueError where the library refuses the arguments (families outside 1 .. 15, or without POOL_BY_OBSTACLE and
    POOL_BY_CAR_CAR)."""
    d = np.ascontiguousarray(decisions, dtype=np.int8)
    D = _decision_len(int(cars), int(steps), int(obstacles))
    if d.ndim != 1 or d.size < D or D <= 0:
        raise ValueError("%d decision bytes given, the shape has %d" % (d.size, D))
    cap = pool_moves_max()
    out = np.empty((cap, 4), dtype=np.int32)
    n = load_library().miqp_gpu_pool_jumps(int(cars), int(steps), int(obstacles), int(max_lines), int(families), d.ctypes.data_as(C.POINTER(C.c_byte)),
                                           out.ctypes.data_as(C.POINTER(C.c_int)), cap)
    if n < 0:
        raise ValueError("miqp_gpu_pool_jumps refused the arguments (%d)" % n)
    return out[:n].copy()


def pool_shift(cars, steps, obstacles, shift, decisions, region_map=None, env_map=None):
    """a record's D decision bytes shifted by ``shift`` steps and re-expressed for the next cycle's instance (miqp_gpu_pool_shift): byte i of every
    site is the source byte of step min(i + shift, steps - 1); a region byte q * 4 + h becomes region_map[c, q] * 4 + h, an environment byte e
    becomes env_map[e]; obstacle and car/car bytes stay; negative bytes and step 0 are -1.  ``region_map`` is an int array [cars, p_src] (None: the
    identity), ``env_map`` an int vector (None: the identity), as CplexWrapper.poolCarryMaps returns them.  Returns (mappable, int8 array of D bytes):
    mappable is False when a region byte has no target - those bytes are -1.  A pure function on bytes: needs no wrapper and no device.  Raises
    ValueError where the library refuses the arguments (shift outside 1 .. steps - 2)."""
    d = np.ascontiguousarray(decisions, dtype=np.int8)
    D = _decision_len(int(cars), int(steps), int(obstacles))
    if d.ndim != 1 or d.size < D or D <= 0:
        raise ValueError("%d decision bytes given, the shape has %d" % (d.size, D))
    ip = C.POINTER(C.c_int)
    rm = em = None
    if region_map is not None:
        rm = np.ascontiguousarray(region_map, dtype=np.int32)
        if rm.ndim != 2 or rm.shape[0] != int(cars) or rm.shape[1] < 1:
            raise ValueError("a region map of shape [cars, p_src] expected, got %s" % (rm.shape,))
    if env_map is not None:
        em = np.ascontiguousarray(env_map, dtype=np.int32)
        if em.ndim != 1:
            raise ValueError("an environment map is a vector")
    out = np.empty(D, dtype=np.int8)
    bp = C.POINTER(C.c_byte)
    rc = load_library().miqp_gpu_pool_shift(int(cars), int(steps), int(obstacles), int(shift), rm.ctypes.data_as(ip) if rm is not None else None,
                                            rm.shape[1] if rm is not None else 0, em.ctypes.data_as(ip) if em is not None and em.size else None,
                                            em.size if em is not None else 0, d.ctypes.data_as(bp), out.ctypes.data_as(bp), D)
    if rc != D and rc != -4:
        raise ValueError("miqp_gpu_pool_shift refused the arguments (%d)" % rc)
    return rc == D, out


def pool_carry_last():
    """(seconds in pool_shift_kernel, seconds in pool_carry_admit_kernel) of the calling thread's last carrySolutionPool, from the call's own device
    events (miqp_gpu_pool_carry_last)"""
    a, b = C.c_double(0.0), C.c_double(0.0)
    load_library().miqp_gpu_pool_carry_last(C.byref(a), C.byref(b))
    return a.value, b.value


def pool_max():
    """largest capacity CplexWrapper.setSolutionPool accepts (a constant of the built library; needs no device)"""
    return int(load_library().miqp_gpu_pool_max())


def pool_settle_passes():
    """the number of solves after which settleDecisions and the refinement of solveSolutionPool stop (miqp_gpu_pool_settle_passes)"""
    return int(load_library().miqp_gpu_pool_settle_passes())


def fixed_batch_chunk():
    """nodes per launch group of CplexWrapper.solveFixedBatch (a constant of the built library; needs no device)"""
    return int(load_library().miqp_gpu_fixed_batch_chunk())


def has_active_set(cars, steps):
    """1 when instances of `cars` cars and `steps` steps have the dual active-set launches for their node relaxations (one or two
    cars, up to 20 steps), else 0: those shapes stay with the interior point.  Host code of the library; needs no device."""
    return int(load_library().miqp_gpu_has_active_set(int(cars), int(steps)))


class OptimizationStatus(enum.IntEnum):  # src/cplex_wrapper.hpp:54-59
    SUCCESS = 0
    FAILED_NO_SOLUT = 1
    FAILED_SEG_FAULT = 2
    FAILED_TIMEOUT = 3


class WarmstartType(enum.IntEnum):  # src/miqp_planner_settings.h:13-18
    NO_WARMSTART = 0
    RECEDING_HORIZON_WARMSTART = 1
    LAST_SOLUTION_WARMSTART = 2
    BOTH_WARMSTART_STRATEGIES = 3


class ParameterSource(enum.IntEnum):  # src/cplex_wrapper.hpp:63
    DATFILE = 0
    CPPINPUTS = 1
    MIXED = 2


class SolutionProperties:  # src/cplex_wrapper.hpp:41-52
    def __init__(self, c=None):
        for n, _ in SolutionPropertiesC._fields_:
            setattr(self, n, getattr(c, n) if c is not None else 0)

    def __repr__(self):
        return "SolutionProperties(" + ", ".join("%s=%r" % (n, getattr(self, n)) for n, _ in SolutionPropertiesC._fields_) + ")"


class CplexWrapper:
    """Same public surface as the reference class; ``modfile`` is accepted and ignored (the OPL model is
    built into the device solver)."""

    def __init__(self, modfile="cplexmodel.mod", parameterSource=ParameterSource.CPPINPUTS, precision=12, modpath="cplexmodel/",
                 nodes_per_round=0, max_open_nodes=0, gap_override=-1.0, verbose=0, device=-1):
        self._L = load_library()
        self._opts = SolverOptsC(int(precision), int(device), int(nodes_per_round), int(max_open_nodes), float(gap_override), int(verbose))
        self._h = self._L.miqp_solver_create(C.byref(self._opts))
        self.parameterSource_ = ParameterSource(parameterSource)
        self.modfile_ = modpath + modfile
        self.datfile_ = ""
        self._params = None
        self._keep = None
        self._results = None
        self._warm = None
        self._starts = 0           # setSolutionPoolStarts
        self._solved = False       # a solve stands behind the loaded instance
        self._keep_loaded = False  # the handle's pool is a carried one that the next solve may start from: that solve does not load the parameters again
        self.useSpecialOrderedSets_ = False
        self.useBranchingPriorities_ = False
        self.doWarmstart_ = WarmstartType.NO_WARMSTART
        self.debugOutputFilePath_ = ""
        self.debugOutputFilePrefix_ = ""
        self.print_debug_outputs_ = False
        self.debugOutputParameterFilePath_ = ""
        self.tmpWarmstartFile_ = "/tmp/warmstart_debug_res.mst"   # src/cplex_wrapper.hpp:104 (shared by all instances)

    def __del__(self):
        try:
            if self._h:
                self._L.miqp_solver_destroy(self._h)
                self._h = None
        except Exception:
            pass

    # ---- parameters
    def setParameterDatFileRelative(self, datfile):
        self.datfile_ = "cplexmodel/" + datfile
        self._keep_loaded = False

    def setParameterDatFileAbsolute(self, datfile):
        self.datfile_ = datfile
        self._keep_loaded = False

    def resetParameters(self, parameters: ModelParameters):
        self._params = parameters  # shared with the caller, re-read on every callCplex (cplex_wrapper.cpp:661-664)
        self._keep_loaded = False  # (new parameters: the next solve loads them, which empties a carried pool)

    def overrideSolverSettingsDataSource(self, parameters: ModelParameters):
        if self._params is not None:
            for n in ["max_solution_time", "relative_mip_gap_tolerance", "mipdisplay", "mipemphasis", "relobjdif", "cutpass",
                      "probe", "repairtries", "rinsheur", "varsel", "mircuts", "parallelmode"]:
                setattr(self._params, n, getattr(parameters, n))

    # ---- options that only steer CPLEX's search (accepted, no effect on the result: K7)
    def setSpecialOrderedSets(self, v):
        self.useSpecialOrderedSets_ = bool(v)

    def setUseBranchingPriorities(self, v):
        self.useBranchingPriorities_ = bool(v)

    def setBranchingPriorityValueExtent(self, value, extent):
        self.branchingPriority_ = (value, extent)

    def setBufferCplexOutputsToStream(self, v):
        pass

    def setDebugOutputPrint(self, v):
        self.print_debug_outputs_ = bool(v)

    def setDebugOutputFilePath(self, p):
        self.debugOutputFilePath_ = p

    def setDebugOutputFilePrefix(self, p):
        self.debugOutputFilePrefix_ = p

    # ---- warm start
    def addRecedingHorizonWarmstart(self, warmstart: RawResults, wt=WarmstartType.RECEDING_HORIZON_WARMSTART):
        self.doWarmstart_ = wt if wt == WarmstartType.RECEDING_HORIZON_WARMSTART else WarmstartType.BOTH_WARMSTART_STRATEGIES
        self._warm = warmstart

    def setLastSolutionWarmstart(self, wt=WarmstartType.LAST_SOLUTION_WARMSTART):
        self.doWarmstart_ = wt if wt == WarmstartType.LAST_SOLUTION_WARMSTART else WarmstartType.BOTH_WARMSTART_STRATEGIES

    def deleteLastSolutionWarmstartFile(self):
        """src/cplex_wrapper.cpp:482-488"""
        self._last = None
        if os.path.exists(self.tmpWarmstartFile_):
            os.remove(self.tmpWarmstartFile_)

    # ---- solve
    def _push_inputs(self):
        keep, self._keep_loaded = self._keep_loaded and self._starts > 0, False
        if keep:
            # starts from the carried pool (setSolutionPoolStarts): the instance stays the one carrySolutionPool settled its records on - loading
            # the parameters again would empty the carried pool before the solve can start from it.  resetParameters loads afresh
            rc = 0
        elif self.parameterSource_ == ParameterSource.DATFILE:
            rc = self._L.miqp_solver_load_dat(self._h, self.datfile_.encode())
        elif self.parameterSource_ == ParameterSource.MIXED and self._params is None:
            rc = self._L.miqp_solver_load_dat(self._h, self.datfile_.encode())   # MIXED: the C++ inputs when given, else the file
        else:
            if self._params is None:
                return -1
            s, self._keep = self._params.to_c()
            rc = self._L.miqp_solver_set_params(self._h, C.byref(s))
        if rc != 0:
            return rc
        if not keep:
            self._solved = False
        # MIP starts (src/cplex_wrapper.cpp:121-138): the receding-horizon start and, independently of it, the .mst
        # file of the last solution - with BOTH_WARMSTART_STRATEGIES the reference applies both
        self._L.miqp_solver_set_warmstart(self._h, None, int(WarmstartType.NO_WARMSTART))
        if self.doWarmstart_ in (WarmstartType.RECEDING_HORIZON_WARMSTART, WarmstartType.BOTH_WARMSTART_STRATEGIES) and self._warm is not None:
            wc = self._warm.to_c()
            self._L.miqp_solver_set_warmstart(self._h, C.byref(wc), int(WarmstartType.RECEDING_HORIZON_WARMSTART))
        if self.doWarmstart_ in (WarmstartType.LAST_SOLUTION_WARMSTART, WarmstartType.BOTH_WARMSTART_STRATEGIES):
            # cplex.readMIPStarts(tmpWarmstartFile_) when the file exists (src/cplex_wrapper.cpp:128-138)
            if os.path.exists(self.tmpWarmstartFile_):
                self._L.miqp_solver_read_mst(self._h, self.tmpWarmstartFile_.encode())
        return 0

    def _stamp(self, timestamp):
        return "%.15g" % float(timestamp)

    def _debug_before(self, timestamp):
        """parameters_<t>.txt (OPL external data) and lpexport_<t>.lp (src/cplex_wrapper.cpp:141-155)"""
        if not self.print_debug_outputs_:
            return
        base = os.path.join(self.debugOutputFilePath_, self.debugOutputFilePrefix_)
        self.debugOutputParameterFilePath_ = base + "parameters_" + self._stamp(timestamp) + ".txt"
        self._L.miqp_solver_write_dat(self._h, self.debugOutputParameterFilePath_.encode())
        self._L.miqp_solver_export_lp(self._h, (base + "lpexport_" + self._stamp(timestamp) + ".lp").encode())

    def _debug_after(self, timestamp, status):
        """MIP start of the last solution and solution_<t>.txt / warmstartsolution_<t>.mst (src/cplex_wrapper.cpp:206-229)"""
        if status != OptimizationStatus.SUCCESS:
            return
        last = self.doWarmstart_ in (WarmstartType.LAST_SOLUTION_WARMSTART, WarmstartType.BOTH_WARMSTART_STRATEGIES)
        if last:
            self._L.miqp_solver_write_mst(self._h, self.tmpWarmstartFile_.encode())
        if self.print_debug_outputs_:
            base = os.path.join(self.debugOutputFilePath_, self.debugOutputFilePrefix_)
            self._L.miqp_solver_write_solution(self._h, (base + "solution_" + self._stamp(timestamp) + ".txt").encode())
            if last:
                self._L.miqp_solver_write_mst(self._h, (base + "warmstartsolution_" + self._stamp(timestamp) + ".mst").encode())

    def _collect(self, status, lazy=False):
        """takes the result record over from the library; lazy (batch entry points): on the first getRawResults()"""
        self._stale = status == OptimizationStatus.SUCCESS
        self._solved, self._keep_loaded = True, False
        if not self._stale:
            return OptimizationStatus(status)
        if not lazy:
            self._fetch()
        return OptimizationStatus(status)

    def _fetch(self):
        if getattr(self, "_stale", False):
            d = (C.c_int * 6)()
            self._L.miqp_solver_get_dims(self._h, d)
            res = RawResults(*list(d))
            rc = res.to_c()
            if self._L.miqp_solver_get_results(self._h, C.byref(rc)) != 0:
                raise RuntimeError("miqp_solver_get_results failed: the library holds no solution for this handle")
            self._results = res
            self._last = res
            self._stale = False

    def callCplex(self, timestamp=0.0):
        if self._push_inputs() != 0:
            return OptimizationStatus.FAILED_SEG_FAULT
        self._debug_before(timestamp)
        st = self._collect(self._L.miqp_solver_solve(self._h, float(timestamp)))
        self._debug_after(timestamp, st)
        return st

    def callCplexSplit(self, world, rank, exchange=None, timestamp=0.0):
        """one instance whose branch-and-bound tree is split over the ranks of a job (miqp_solver_solve_split): every rank
        calls this with the same parameters; ``exchange`` is an EXCHANGE_FN (e.g. sharding.torch_exchange()), None = the RCCL
        communicator of sharding.init_rccl_comm().  Every rank returns the same status and holds the full result."""
        if self._push_inputs() != 0:
            return OptimizationStatus.FAILED_SEG_FAULT
        if exchange is None:
            st = self._L.miqp_solver_solve_split_rccl(self._h, float(timestamp))
        else:
            st = self._L.miqp_solver_solve_split(self._h, float(timestamp), int(world), int(rank), exchange, None)
        return self._collect(st)

    def splitRoots(self, world, rank):
        """the roots of rank ``rank`` in a tree split over ``world`` ranks: (list of roots, each a list of (record index,
        alternative) fixings; size of the partition).  No device needed."""
        if self._push_inputs() != 0:
            return None
        cap = 4096
        ro, ix, va = (C.c_int * cap)(), (C.c_int * cap)(), (C.c_int * cap)()
        nr, nc = C.c_int(0), C.c_int(0)
        n = self._L.miqp_solver_split_roots(self._h, int(world), int(rank), ro, ix, va, cap, C.byref(nr), C.byref(nc))
        if n < 0:
            return None
        roots = [[] for _ in range(nr.value)]
        for k in range(min(n, cap)):
            roots[ro[k]].append((ix[k], va[k]))
        return roots, nc.value

    def getRawResults(self):
        self._fetch()
        return self._results

    def getSolutionProperties(self):
        p = SolutionPropertiesC()
        self._L.miqp_solver_get_properties(self._h, C.byref(p))
        return SolutionProperties(p)

    def getTmpWarmstartFile(self):
        return self.tmpWarmstartFile_

    def getDebugOutputParameterFilePath(self):
        return self.debugOutputParameterFilePath_

    def writeDat(self, path):
        """the parameters of the next solve as OPL external data (no device needed)"""
        if self._push_inputs() != 0:
            return -1
        return self._L.miqp_solver_write_dat(self._h, path.encode())

    # ---- extras of this implementation
    def solveFixed(self, fixed: RawResults):
        """continuous QP with the binaries of ``fixed`` asserted (device interior point kernel)"""
        if self._push_inputs() != 0:
            return None
        d = (C.c_int * 6)()
        self._L.miqp_solver_get_dims(self._h, d)
        out = RawResults(*list(d))
        oc = out.to_c()
        fc = fixed.to_c()
        obj = C.c_double(0)
        it = C.c_int(0)
        rc = self._L.miqp_solver_solve_fixed(self._h, C.byref(fc), C.byref(oc), C.byref(obj), C.byref(it))
        return rc, out, obj.value, it.value

    def lastFixedRoute(self):
        """which launch solved the node of the last solveFixed(): 0 the standard on-chip kernel, 1 its larger variant, 2 the
        memory-backed kernel behind them, 3 the memory-backed kernel of a shape without an on-chip kernel; -1 before any"""
        return int(self._L.miqp_solver_last_fixed_route(self._h))

    def launchPlan(self, bc, overlap=0, par=-1, cls_n=(-1, -1, -1), cus=256, free_gb=256.0, as_on=1, concurrent=True):
        """the node launches of a round of ``bc`` nodes (``overlap`` 1, ``par`` the round's parity) or of the serial chain (``overlap`` 0), one tuple
        of LAUNCH_PLAN_FIELDS per launch in the order of issue (miqp_solver_launch_plan, include/miqp_gpu.h).  Host code; needs no device."""
        if self._push_inputs() != 0:
            return None
        out = (C.c_int * (5 * len(LAUNCH_PLAN_FIELDS)))()
        n = self._L.miqp_solver_launch_plan(self._h, int(bc), int(overlap), int(par), (C.c_int * 3)(*cls_n), int(cus), float(free_gb),
                                            (1 if as_on else 0) | (0 if concurrent else 2), out, len(out))
        if n < 0:
            raise RuntimeError("miqp_solver_launch_plan failed (%d)" % n)
        k = len(LAUNCH_PLAN_FIELDS)
        return [tuple(out[i * k:(i + 1) * k]) for i in range(n)]

    def solveFixedBatch(self, records):
        """the continuous QPs of many records of this wrapper's instance in one device call (miqp_solver_solve_fixed_batch): each entry is
        answered as solveFixed answers it alone.  Returns (status, objective, violation, iterations, route, best): numpy arrays of
        len(records) - status 0 feasible, 1 infeasible, 2 entry refused (None, or a record of another shape) - and the index of the feasible
        entry with the lowest objective (-1: none).  Raises RuntimeError where the library refuses the call (no device: there is no host solve)."""
        if self._push_inputs() != 0:
            raise RuntimeError("invalid parameters")
        n = len(records)
        keep = [r.to_c() if r is not None else None for r in records]
        ptrs = (C.POINTER(RawResultsC) * max(n, 1))(*[C.pointer(c) if c is not None else None for c in keep])
        out = (FixedResultC * max(n, 1))()
        best = C.c_int(-1)
        rc = self._L.miqp_solver_solve_fixed_batch(self._h, ptrs, n, out, C.byref(best))
        if rc != 0:
            raise RuntimeError("miqp_solver_solve_fixed_batch failed (%d)" % rc)
        a = np.frombuffer(out, dtype=np.dtype([("status", "<i4"), ("route", "<i4"), ("iterations", "<i4"), ("reserved", "<i4"),
                                               ("objective", "<f8"), ("violation", "<f8")]), count=n)
        return (a["status"].copy(), a["objective"].copy(), a["violation"].copy(), a["iterations"].copy(), a["route"].copy(), best.value)

    def fixedBatchRecord(self, k):
        """(rc, RawResults) of entry ``k`` of the last solveFixedBatch of this wrapper: rc 0 and the record solveFixed would have returned
        for it; rc 1 (entry not feasible), -1 (no such entry, no batch held: new parameters drop it) with None"""
        d = (C.c_int * 6)()
        if self._L.miqp_solver_get_dims(self._h, d) != 0:
            return -1, None
        out = RawResults(*list(d))
        oc = out.to_c()
        rc = self._L.miqp_solver_fixed_batch_record(self._h, int(k), C.byref(oc))
        return rc, (out if rc == 0 else None)

    def solveFixedActiveSet(self, records, start=None, block=0, cutoff=None):
        """DIAGNOSTIC (miqp_solver_solve_fixed_as): the records as nodes of the dual active-set launches, each read back as the kernel left it.
        start[k]: -1 cold, p < k from node p's final active set and its M, -(p + 2) the same with M rebuilt; block 0 the standard block, 1 the
        larger one; cutoff[k] in the units of the objective (nan: none).  Returns (nodes, info32): a numpy record array with the fields of
        miqp_as_node_c - status 0 solved, 1 infeasible, 2 cut off, 3 the block does not hold the rows, 4 the method could not finish - and the
        32 counters of the launches.  Raises RuntimeError with the library's code and text where the call is refused."""
        if self._push_inputs() != 0:
            raise RuntimeError("invalid parameters")
        n = len(records)
        keep = [r.to_c() if r is not None else None for r in records]
        ptrs = (C.POINTER(RawResultsC) * max(n, 1))(*[C.pointer(c) if c is not None else None for c in keep])
        out = (AsNodeC * max(n, 1))()
        info = (C.c_ulonglong * 32)()
        st = None if start is None else (C.c_int * max(n, 1))(*[int(v) for v in start])
        cu = None if cutoff is None else (C.c_double * max(n, 1))(*[float(v) for v in cutoff])
        rc = self._L.miqp_solver_solve_fixed_as(self._h, ptrs, n, st, int(block), cu, out, info)
        if rc != 0:
            raise RuntimeError("miqp_solver_solve_fixed_as failed (%d): %s" % (rc, self.lastError()))
        a = np.frombuffer(out, dtype=np.dtype([("status", "<i4"), ("steps", "<i4"), ("active", "<i4"), ("reserved", "<i4"),
                                               ("objective", "<f8"), ("bound", "<f8"), ("violation", "<f8")]), count=n).copy()
        return a, np.array(list(info), dtype=np.uint64)

    def fixedActiveSetRecord(self, k):
        """(rc, RawResults) of node ``k`` of the last solveFixedActiveSet of this wrapper, as fixedBatchRecord: rc 0 with the record, 1 (the
        node was not solved) or -1 (no such node, nothing held) with None"""
        d = (C.c_int * 6)()
        if self._L.miqp_solver_get_dims(self._h, d) != 0:
            return -1, None
        out = RawResults(*list(d))
        oc = out.to_c()
        rc = self._L.miqp_solver_fixed_as_record(self._h, int(k), C.byref(oc))
        return rc, (out if rc == 0 else None)

    # ---- solution pool (IloCplex::getSolnPoolNsolns / getObjValue(i) / getValues(x, i) for a CPLEX user)
    def setSolutionPool(self, capacity):
        """the next solves of this wrapper keep their ``capacity`` best distinct integer solutions (0: off, the default; at most pool_max()).
        Returns the library's code: 0, < 0 when the capacity is refused (the previous setting stays)"""
        return int(self._L.miqp_solver_set_pool(self._h, int(capacity)))

    def setSolutionPoolFilter(self, families):
        """which leaves are ONE entry of the pool of the next solves: a bit set of POOL_BY_REGION, POOL_BY_ENVIRONMENT, POOL_BY_OBSTACLE,
        POOL_BY_CAR_CAR and POOL_EXACT_TIMING (0: off, the default - entries differ in any decision byte).  POOL_BY_OBSTACLE | POOL_BY_CAR_CAR keeps
        one entry per manoeuvre: which side of each obstacle, which order of the cars, not at which step.  Returns the library's code: 0, < 0 when
        the value is refused (the previous setting stays)"""
        return int(self._L.miqp_solver_set_pool_filter(self._h, int(families)))

    def solutionPoolFoundDecisions(self, k):
        """the decision bytes of entry ``k`` as the search kept it (int8 array; before any refinement), None when there is no such entry; needs no device"""
        d = (C.c_int * 6)()
        if self._L.miqp_solver_get_dims(self._h, d) != 0:
            return None
        out = np.empty(_decision_len(d[0], d[1], d[4]), dtype=np.int8)
        rc = self._L.miqp_solver_pool_found_decisions(self._h, int(k), out.ctypes.data_as(C.POINTER(C.c_byte)), out.size)
        return out if rc == out.size else None

    def poolSignature(self, record, families):
        """the signature of a RawResults record of this wrapper's instance under ``families`` (int8 array): the record's fix record, then
        pool_signature.  Needs no device.  Raises ValueError where the library refuses the arguments."""
        d = (C.c_int * 6)()
        if self._L.miqp_solver_get_dims(self._h, d) != 0 and (self._push_inputs() != 0 or self._L.miqp_solver_get_dims(self._h, d) != 0):   # (a loaded instance is kept: loading drops its pool)
            raise ValueError("invalid parameters")
        out = np.empty(_decision_len(d[0], d[1], d[4]), dtype=np.int8)
        rc = self._L.miqp_solver_pool_signature(self._h, C.byref(record.to_c()), int(families), out.ctypes.data_as(C.POINTER(C.c_byte)), out.size)
        if rc != out.size:
            raise ValueError("miqp_solver_pool_signature refused the arguments (%d)" % rc)
        return out

    def solutionPoolCount(self):
        """entries the last solve kept (0 with the pool off, before a solve, without a solution, after new parameters); needs no device.  Behind
        solveSolutionPool: the entries that call left (it merges records that are one solution), before it an upper bound"""
        return int(self._L.miqp_solver_pool_count(self._h))

    def solutionPoolFound(self):
        """the objectives of the kept entries as the search found them (node tolerance), best first; needs no device"""
        n = self.solutionPoolCount()
        o = np.zeros(max(n, 1))
        m = self._L.miqp_solver_pool_found(self._h, o.ctypes.data_as(c_double_p), n)
        return o[:max(m, 0)].copy()

    def solveSolutionPool(self):
        """the kept entries refined at the tight tolerance in one device call (miqp_solver_pool_solve): (status, objective, violation, iterations,
        route) as numpy arrays in pool order, like solveFixedBatch - each entry as solveFixed answers its solutionPoolRecord.  Records that turn out
        to be one solution (the same binaries) are merged, so the arrays can be shorter than solutionPoolCount() was before the call.  Raises RuntimeError
        where the library refuses the call (no device: there is no host solve)."""
        n = max(self.solutionPoolCount(), 1)
        out = (FixedResultC * n)()
        m = self._L.miqp_solver_pool_solve(self._h, out, n)
        if m < 0:
            raise RuntimeError("miqp_solver_pool_solve failed (%d)" % m)
        a = np.frombuffer(out, dtype=np.dtype([("status", "<i4"), ("route", "<i4"), ("iterations", "<i4"), ("reserved", "<i4"),
                                               ("objective", "<f8"), ("violation", "<f8")]), count=m)
        return (a["status"].copy(), a["objective"].copy(), a["violation"].copy(), a["iterations"].copy(), a["route"].copy())

    def improveSolutionPool(self, max_passes=8):
        """every kept entry of a FILTERED pool hill-climbed inside its own class in one device-resident loop (miqp_solver_pool_improve): per pass
        all timing moves of pool_moves of every entry that still moves are solved at the tight tolerance and the best improving one is applied.
        Returns (rc, before, after, moves, status): rc the number of entries that moved - or the library's code < 0: -2 the filter is not in
        1 .. 15 or max_passes not in 1 .. 64, -3 no device; the pool is untouched then - and numpy arrays in pool order (empty for rc < 0).
        Behind it solutionPoolFoundDecisions / solutionPoolFound report the improved records and their tight-tolerance objectives; entries keep
        their places.  A refined pool is dropped: call solveSolutionPool afterwards."""
        n = max(self.solutionPoolCount(), 1)
        out = (PoolImproveC * n)()
        rc = int(self._L.miqp_solver_pool_improve(self._h, int(max_passes), out, n))
        m = min(self.solutionPoolCount(), n) if rc >= 0 else 0
        a = np.frombuffer(out, dtype=np.dtype([("before", "<f8"), ("after", "<f8"), ("moves", "<i4"), ("status", "<i4")]), count=m)
        return rc, a["before"].copy(), a["after"].copy(), a["moves"].copy(), a["status"].copy()

    def exploreSolutionPool(self, max_passes=4, max_rel=-1.0, distinct=False, settled=False):
        """the free places of a FILTERED pool filled with neighbouring manoeuvre classes in one device-resident loop (miqp_solver_pool_explore;
        IloCplex::populate for a CPLEX user): pass 1 solves every jump of pool_jumps of every kept entry at the tight tolerance, pass p > 1 those of
        the entries pass p - 1 added; the best feasible neighbour of every class the pool does not hold yet is appended while a place is free.
        ``max_rel`` >= 0 admits only objectives within max_rel * |objective of entry 0| above entry 0's.  Returns (rc, added): rc the number of
        entries added - or the library's code < 0: -2 the filter is not in 1 .. 15 or has neither POOL_BY_OBSTACLE nor POOL_BY_CAR_CAR, or
        max_passes not in 1 .. 64; -3 no device; the pool is untouched then - and one dict per added entry, in pool order behind the old entries
        (parent, pass, first, stride, count, value, iterations, objective; empty for rc <= 0).  Old entries keep their bytes and places.  A
        refined pool is dropped: call solveSolutionPool afterwards.
        ``distinct`` (miqp_solver_pool_explore_distinct): a neighbour is admitted only when the canonical labels of its own solution have a new
        signature as well, so an entry's solution under other labels takes no place; the timing then counts pass 0, the kept entries' own solves.
        ``settled`` (miqp_solver_pool_explore_settled): every candidate is solved and re-labelled until its labels stay, as solveSolutionPool
        does, and admitted by the signature of those settled labels, so solveSolutionPool behind the call merges away nothing it added; the
        dicts then carry ``solves``, the solves the entry's settling took, and the timing counts every solve.  Not together with ``distinct``."""
        if distinct and settled:
            raise ValueError("distinct and settled are two admissions: choose one")
        n = pool_max()
        out = (PoolExploreC * n)()
        call = self._L.miqp_solver_pool_explore_settled if settled else self._L.miqp_solver_pool_explore_distinct if distinct else self._L.miqp_solver_pool_explore
        rc = int(call(self._h, int(max_passes), float(max_rel), out, n))
        return rc, _explore_dicts(out[:max(rc, 0)], settled)

    def _loaded(self):
        """the instance is in the library (a loaded instance is kept: loading drops its pool); False: invalid parameters"""
        d = (C.c_int * 6)()
        return self._L.miqp_solver_get_dims(self._h, d) == 0 or (self._push_inputs() == 0 and self._L.miqp_solver_get_dims(self._h, d) == 0)

    def poolCarryMaps(self, src):
        """the two maps of a carry from ``src`` (last cycle's wrapper) into this wrapper's instance (miqp_solver_pool_carry_maps): (region_map,
        env_map) - region_map[c, q] this instance's possible-region index of the region number that is src's q-th possible region of car c, or
        -1; env_map[e] this instance's environment piece of the same edges as src's piece e, or -1.  Needs no device.  Raises ValueError, with
        lastError(), where the library refuses the pair (instances of different shape, obstacle soft flags or region tables)."""
        if not self._loaded() or not src._loaded():
            raise ValueError("invalid parameters")
        d = (C.c_int * 6)()
        self._L.miqp_solver_get_dims(src._h, d)
        rm = np.full(d[0] * d[2], -1, dtype=np.int32); em = np.full(max(d[3], 1), -1, dtype=np.int32)
        ip = C.POINTER(C.c_int)
        p = int(self._L.miqp_solver_pool_carry_maps(src._h, self._h, rm.ctypes.data_as(ip), rm.size, em.ctypes.data_as(ip), d[3]))
        if p < 1:
            raise ValueError("miqp_solver_pool_carry_maps refused the pair (%d)%s" % (p, ": " + self.lastError() if self.lastError() else ""))
        return rm[:d[0] * p].reshape(d[0], p).copy(), em[:d[3]].copy()

    def carrySolutionPool(self, src, shift=1, max_rel=-1.0):
        """the kept entries of ``src`` - the wrapper of the cycle ``shift`` steps ago, its pool as it stands (explored entries included) - carried
        into the free places of this wrapper's pool in one device-resident call (miqp_solver_pool_carry): every record shifted by ``shift`` steps
        and re-expressed in this instance's alternatives (pool_shift with poolCarryMaps), settled on this instance, and admitted under this
        wrapper's filter when its class is new - by its own signature and by that of its settled labels, so solveSolutionPool behind the call
        merges away nothing it added - within ``max_rel`` (as exploreSolutionPool; an empty pool admits its first record whatever the cap).
        Returns (added, records): added the number of entries appended - or the library's code < 0: -2 the shift is outside 1 .. NumSteps - 2, no
        capacity, a filter outside 1 .. 15, instances the maps refuse; -3 no device; both pools are untouched then - and one dict per SOURCE
        entry (status, place, solves, iterations, objective; empty for a code < 0): status 0 admitted, 1 not feasible here, 2 unmappable, 3
        signature in the pool, 4 no settled labels or settled signature in the pool, 5 beyond the cost cap, 6 no place free.  ``src`` is only
        read; old entries keep bytes and places; a refined pool is dropped: call solveSolutionPool afterwards."""
        if not self._loaded() or not src._loaded():
            return -1, []
        n = pool_max()
        out = (PoolCarryC * n)(*[PoolCarryC(-1, -1, 0, 0, 0, 0, float("nan")) for _ in range(n)])   # (a call that touches no device writes nothing)
        ns = min(src.solutionPoolCount(), n)
        rc = int(self._L.miqp_solver_pool_carry(self._h, src._h, int(shift), float(max_rel), out, n))
        if rc < 0:
            return rc, []
        self._carried_into(rc)
        return rc, [dict(status=o.status, place=o.place, solves=o.solves, iterations=o.iterations, objective=float(o.objective)) for o in out[:ns] if o.status >= 0]

    def _carried_into(self, added):
        """behind a carry: a pool without a solve behind it is one the next solve may start from (setSolutionPoolStarts)"""
        if added > 0 and not self._solved:
            self._keep_loaded = True

    def setSolutionPoolStarts(self, max_starts):
        """the next solves of this wrapper START THEIR SEARCH from the carried manoeuvres (miqp_solver_set_pool_starts; for a CPLEX user: the old
        pool's members re-added as MIP starts): a solve behind carrySolutionPool into this wrapper's EMPTY pool - parameters loaded, capacity
        and filter set, no solve yet - takes the first min(max_starts, entries) carried records as additional roots of its first round.  A
        feasible one is the first incumbent, and the capture merges every feasible start into the pool of the solve, so the fallback that was
        carried in survives the solve.  0: off, the default; at most pool_max().  Returns the library's code: 0, -1 when the value is refused
        (the previous setting stays).  The order is resetParameters, carrySolutionPool, callCplex (or solve_batch): with the setting on, that solve
        keeps the instance the carry settled its records on instead of loading the parameters again - which would empty the carried pool;
        resetParameters in between loads afresh and so drops the carried pool.  THAT ONE SOLVE THEREFORE DOES NOT RE-READ THE SHARED
        ModelParameters: an in-place edit of them between the carry and the solve, overrideSolverSettingsDataSource (gap, time limit)
        included, takes effect from the next load on - make such edits before carrySolutionPool, or call resetParameters and give up the
        starts.  A tree-split solve ignores the setting."""
        rc = int(self._L.miqp_solver_set_pool_starts(self._h, int(max_starts)))
        if rc == 0:
            self._starts = int(max_starts)
        return rc

    def solutionPoolStarts(self):
        """the setting of setSolutionPoolStarts as the library holds it (miqp_solver_get_pool_starts)"""
        return int(self._L.miqp_solver_get_pool_starts(self._h))

    def solutionPoolStartsLast(self):
        """the places of the start roots the last solve took from the carried pool (miqp_solver_pool_starts_last): one int per start, the entry of
        the pool after that solve that stands for the start - the entry of its signature under this wrapper's filter, without a filter the entry
        of the same decision bytes - or -1 when the pool holds none.  [] when the solve took no starts; needs no device"""
        n = pool_max()
        place = (C.c_int * n)()
        t = int(self._L.miqp_solver_pool_starts_last(self._h, place, n))
        return [int(place[k]) for k in range(max(0, min(t, n)))]

    def solveDecisions(self, decisions):
        """the continuous QPs of many DECISION records of this wrapper's instance in one device call (miqp_solver_solve_decisions): ``decisions`` is
        an int8 array [n, D] of records as solutionPoolFoundDecisions hands them out.  Returns (rc, status, objective, violation, iterations,
        route, best) as solveFixedBatch does, with the library's code in front instead of an exception: 0, -3 without a device (every status
        is 2 then).  A record with a byte outside its site's alternatives is status 2 of that entry.  fixedBatchRecord(k) works behind it."""
        d = np.ascontiguousarray(decisions, dtype=np.int8)
        dims = (C.c_int * 6)()
        if self._L.miqp_solver_get_dims(self._h, dims) != 0 and (self._push_inputs() != 0 or self._L.miqp_solver_get_dims(self._h, dims) != 0):   # (a loaded instance is kept: loading drops its pool)
            raise RuntimeError("invalid parameters")
        D = _decision_len(dims[0], dims[1], dims[4])
        if d.ndim != 2 or d.shape[1] != D:
            raise ValueError("decision records of %d bytes expected, got an array of shape %s" % (D, d.shape))
        n = d.shape[0]
        out = (FixedResultC * max(n, 1))()
        best = C.c_int(-1)
        rc = int(self._L.miqp_solver_solve_decisions(self._h, d.ctypes.data_as(C.POINTER(C.c_byte)), n, out, C.byref(best)))
        a = np.frombuffer(out, dtype=_FIXED_RESULT_DTYPE, count=n)
        return (rc, a["status"].copy(), a["objective"].copy(), a["violation"].copy(), a["iterations"].copy(), a["route"].copy(), best.value)

    def _decision_array(self, decisions):
        d = np.ascontiguousarray(decisions, dtype=np.int8)
        dims = (C.c_int * 6)()
        if self._L.miqp_solver_get_dims(self._h, dims) != 0 and (self._push_inputs() != 0 or self._L.miqp_solver_get_dims(self._h, dims) != 0):   # (a loaded instance is kept: loading drops its pool)
            raise RuntimeError("invalid parameters")
        D = _decision_len(dims[0], dims[1], dims[4])
        if d.ndim != 2 or d.shape[1] != D:
            raise ValueError("decision records of %d bytes expected, got an array of shape %s" % (D, d.shape))
        return d, dims

    def canonicalDecisions(self, decisions):
        """solveDecisions with the canonical labels of every solved record, written on the device (miqp_solver_canonical_decisions): returns the
        tuple of solveDecisions and an int8 array [n, D] - row k the first alternative of every disjunction that holds at record k's own solution,
        byte for byte poolSignature(fixedBatchRecord(k), 31); all -1 for an entry of status 1 or 2.  Rows that agree are one solution."""
        d, _ = self._decision_array(decisions)
        n = d.shape[0]
        out = (FixedResultC * max(n, 1))()
        canon = np.full((max(n, 1), d.shape[1]), -1, dtype=np.int8)
        best = C.c_int(-1)
        bp = C.POINTER(C.c_byte)
        rc = int(self._L.miqp_solver_canonical_decisions(self._h, d.ctypes.data_as(bp), n, out, canon.ctypes.data_as(bp), C.byref(best)))
        a = np.frombuffer(out, dtype=_FIXED_RESULT_DTYPE, count=n)
        return (rc, a["status"].copy(), a["objective"].copy(), a["violation"].copy(), a["iterations"].copy(), a["route"].copy(), best.value, canon[:n])

    def settleDecisions(self, decisions):
        """decision records solved and re-labelled on the device until their labels stay (miqp_solver_settle_decisions), at most
        pool_settle_passes() solves each: returns the tuple of solveDecisions - of every record's LAST solve - an int8 array [n, D] - row k the
        labels that solve ran with; all -1 for an entry of status 1 or 2 - and an int32 array [n], the solves of every record (0: refused,
        negative: still moving at the end).  fixedBatchRecord does not work behind it: send the settled rows through solveDecisions."""
        d, _ = self._decision_array(decisions)
        n = d.shape[0]
        out = (FixedResultC * max(n, 1))()
        settled = np.full((max(n, 1), d.shape[1]), -1, dtype=np.int8)
        solves = np.zeros(max(n, 1), dtype=np.int32)
        best = C.c_int(-1)
        bp = C.POINTER(C.c_byte)
        rc = int(self._L.miqp_solver_settle_decisions(self._h, d.ctypes.data_as(bp), n, out, settled.ctypes.data_as(bp), solves.ctypes.data_as(C.POINTER(C.c_int)), C.byref(best)))
        a = np.frombuffer(out, dtype=_FIXED_RESULT_DTYPE, count=n)
        return (rc, a["status"].copy(), a["objective"].copy(), a["violation"].copy(), a["iterations"].copy(), a["route"].copy(), best.value, settled[:n], solves[:n])

    def canonicalLabels(self, decisions, trajectories, via=0):
        """the canonical labels of decision records [n, D] at given trajectories [n, NumSteps * 8 * NumCars], on the host
        (miqp_solver_canonical_labels): via 0 the restatement the device kernel compiles, via 1 the host functions behind fixedBatchRecord.
        Returns (labelled, int8 array [n, D]).  Needs no device."""
        d, dims = self._decision_array(decisions)
        z = np.ascontiguousarray(trajectories, dtype=np.float64)
        if z.shape != (d.shape[0], dims[1] * 8 * dims[0]):
            raise ValueError("trajectories of shape %s expected, got %s" % ((d.shape[0], dims[1] * 8 * dims[0]), z.shape))
        canon = np.full(d.shape, -1, dtype=np.int8)
        bp = C.POINTER(C.c_byte)
        rc = int(self._L.miqp_solver_canonical_labels(self._h, d.ctypes.data_as(bp), z.ctypes.data_as(c_double_p), d.shape[0], int(via), canon.ctypes.data_as(bp)))
        return rc, canon

    def solutionPoolRecord(self, k):
        """(rc, RawResults) of entry ``k`` of the last solveSolutionPool: rc 0 and the record; rc 1 (the entry did not come out feasible at the
        tight tolerance), -1 (no such entry, no refined pool held) with None"""
        d = (C.c_int * 6)()
        if self._L.miqp_solver_get_dims(self._h, d) != 0:
            return -1, None
        out = RawResults(*list(d))
        oc = out.to_c()
        rc = self._L.miqp_solver_pool_record(self._h, int(k), C.byref(oc))
        return rc, (out if rc == 0 else None)

    def liftTables(self):
        """response tables of the bound lifting, array [car][axis][step][4][4] (diagnostic, no device needed)"""
        if self._push_inputs() != 0:
            raise RuntimeError("invalid parameters")
        p = self._params
        out = np.zeros((p.NumCars, 2, p.NumSteps, 4, 4))
        n = self._L.miqp_solver_lift_tables(self._h, out.ctypes.data_as(c_double_p), out.size)
        if n != out.size:
            raise RuntimeError("miqp_solver_lift_tables failed (%d)" % n)
        return out

    def rawSizes(self):
        """rows / binaries / continuous columns / non-zeros of the OPL model of the loaded parameters (no device needed)"""
        if self._push_inputs() != 0:
            return None
        o = (C.c_int * 4)()
        if self._L.miqp_solver_raw_sizes(self._h, o) != 0:
            return None
        return dict(rows=o[0], bin=o[1], cont=o[2], nnz=o[3])

    def certify(self, candidate: RawResults = None, use_real_slack=True):
        """Certificate of a record against the raw big-M model of this wrapper's instance, evaluated on the device
        (miqp_solver_certify).  ``candidate`` None: the last solution of the wrapper, with its real-valued car/car slacks;
        a RawResults: that record (``use_real_slack`` False: with its int-truncated ``slackvars`` instead of
        ``slackvars_real``), against the instance the handle holds (that of the last solve; a wrapper that has not
        solved yet loads its parameters first).  Raises RuntimeError where the library
        refuses (record of another shape, no device - there is no host evaluation)."""
        out = CertificateC()
        if candidate is None:
            rc = self._L.miqp_solver_certify(self._h, None, C.byref(out))
        else:
            d = (C.c_int * 6)()
            if self._L.miqp_solver_get_dims(self._h, d) != 0 and self._push_inputs() != 0:   # (a loaded instance is kept: loading drops its solution)
                raise RuntimeError("invalid parameters")
            cc = candidate.to_c()
            if not use_real_slack:
                cc.slackvars_real = None
            rc = self._L.miqp_solver_certify(self._h, C.byref(cc), C.byref(out))
        if rc != 0:
            raise RuntimeError("miqp_solver_certify failed (%d): %s" % (rc, self.lastError()))
        return Certificate(out)

    def lastAdmission(self):
        """seconds after the start of the last batch / stream call at which this instance was admitted to a slot"""
        o = (C.c_double * 1)()
        self._L.miqp_solver_last_admission(self._h, o)
        return o[0]

    def lastError(self):
        """why the last solve of this wrapper did not run or did not finish ("" when there is nothing to say)"""
        return (self._L.miqp_solver_last_error(self._h) or b"").decode()

    def lastTiming(self):
        t = (C.c_double * 6)()
        self._L.miqp_solver_last_timing(self._h, t)
        u = (C.c_double * 3)()
        self._L.miqp_solver_last_setup(self._h, u)
        v = (C.c_double * 8)()
        self._L.miqp_solver_last_active_set(self._h, v)
        return dict(solve_s=t[0], ipm_s=t[1], ipm_launches=int(t[2]), nodes=int(t[3]), ipm_iters=int(t[4]), row_iters=int(t[5]),
                    setup_s=u[0], context_s=u[1], context_built=bool(u[2]),
                    as_nodes=int(v[0]), as_steps=int(v[1]), as_unfinished=int(v[2]), as_drops=int(v[3]), as_rows_end=int(v[4]), as_rows_parent=int(v[5]),
                    std_launch_s=v[6], std_launches=int(v[7]))


def prepare_batch(wrappers):
    """hands the parameters (and MIP starts) of every wrapper to its solver handle - the marshalling part of a batch call, which
    a caller with many instances does while it builds them (bench.py: before the timed region)"""
    for w in wrappers:
        if w._push_inputs() != 0:
            raise RuntimeError("invalid parameters")


def solve_batch(wrappers, gpus=None, inflight=None, prepared=False):
    """Solves independent instances concurrently: on one device (miqp_solver_solve_batch), or with ``gpus`` given
    sharded b -> device b mod gpus inside the library (miqp_solver_solve_batch_multi; 0 = every visible device).
    ``inflight``: the call is a queue drained with that many instances in flight (miqp_solver_solve_stream);
    ``prepared``: prepare_batch(wrappers) has been called already.  Result records are fetched on the first getRawResults()."""
    L = load_library()
    if not prepared:
        prepare_batch(wrappers)
    n = len(wrappers)
    hs = (C.c_void_p * n)(*[w._h for w in wrappers])
    st = (C.c_int * n)(*([int(OptimizationStatus.FAILED_SEG_FAULT)] * n))   # (a status the library does not write must not read as SUCCESS = 0)
    if inflight is not None and gpus is None:
        rc = L.miqp_solver_solve_stream(hs, n, int(inflight), st)
    else:
        rc = L.miqp_solver_solve_batch(hs, n, st) if gpus is None else L.miqp_solver_solve_batch_multi(hs, n, int(gpus), st)
    if rc not in (0, -2):
        return [OptimizationStatus.FAILED_SEG_FAULT] * n
    # (-2: the call failed as a whole or in part - the library has set every status: FAILED_SEG_FAULT for the instances it did not run)
    return [w._collect(st[k], lazy=True) for k, w in enumerate(wrappers)]


def certify_batch(wrappers):
    """certificates of the last solutions of ``wrappers`` in one call (miqp_solver_certify_batch): a list of Certificate, entry k
    with status 1 when wrapper k holds no solution.  The wrappers may differ in shape."""
    L = load_library()
    n = len(wrappers)
    if n == 0:
        return []
    hs = (C.c_void_p * n)(*[w._h for w in wrappers])
    out = (CertificateC * n)()
    rc = L.miqp_solver_certify_batch(hs, n, out)
    if rc != 0:
        raise RuntimeError("miqp_solver_certify_batch failed (%d): %s" % (rc, wrappers[0].lastError()))
    return [Certificate(out[k]) for k in range(n)]


def solve_fixed_multi(wrappers, records_per_wrapper):
    """the fix records of many wrappers in one device call (miqp_solver_solve_fixed_multi): records_per_wrapper[h] is the list solveFixedBatch would
    get for wrappers[h] (it may be empty).  Returns, per wrapper, what its solveFixedBatch returns - (status, objective, violation, iterations, route,
    best), best counting inside the wrapper's own list - bit for bit; fixedBatchRecord works per wrapper afterwards.  A wrapper whose handle holds an
    instance already (it has solved, or answered a solveFixedBatch) keeps it, and with it what the handle holds - the queue that was drained is the
    queue that is asked; one that has not loaded its parameters yet loads them now.  Raises RuntimeError where the library refuses the call
    (wrappers of different shape, no device: there is no host solve); a refused call leaves what the handles keep alone."""
    L = load_library()
    n = len(wrappers)
    if n != len(records_per_wrapper):
        raise ValueError("one list of records per wrapper")
    d = (C.c_int * 6)()
    for w in wrappers:
        if L.miqp_solver_get_dims(w._h, d) != 0 and w._push_inputs() != 0:
            raise RuntimeError("invalid parameters")
    first = [0]
    for recs in records_per_wrapper:
        first.append(first[-1] + len(recs))
    total = first[-1]
    keep = [r.to_c() if r is not None else None for recs in records_per_wrapper for r in recs]
    ptrs = (C.POINTER(RawResultsC) * max(total, 1))(*[C.pointer(c) if c is not None else None for c in keep])
    out = (FixedResultC * max(total, 1))()
    best = (C.c_int * max(n, 1))(*([-1] * max(n, 1)))
    hs = (C.c_void_p * max(n, 1))(*[w._h for w in wrappers])
    rc = L.miqp_solver_solve_fixed_multi(hs, n, ptrs, (C.c_int * (n + 1))(*first), out, best)
    if rc != 0:
        raise RuntimeError("miqp_solver_solve_fixed_multi failed (%d)%s" % (rc, ": " + wrappers[0].lastError() if n and rc == -2 else ""))
    a = np.frombuffer(out, dtype=_FIXED_RESULT_DTYPE, count=total)
    return [(a["status"][first[h]:first[h + 1]].copy(), a["objective"][first[h]:first[h + 1]].copy(), a["violation"][first[h]:first[h + 1]].copy(),
             a["iterations"][first[h]:first[h + 1]].copy(), a["route"][first[h]:first[h + 1]].copy(), int(best[h])) for h in range(n)]


def solve_solution_pools(wrappers):
    """the solution pools of many wrappers refined in one device call (miqp_solver_pool_solve_multi): per wrapper what its solveSolutionPool
    returns - (status, objective, violation, iterations, route) in pool order, bit for bit; solutionPoolCount and solutionPoolRecord work per
    wrapper afterwards.  A wrapper without a pool gets empty arrays.  Raises RuntimeError where the library refuses the call."""
    L = load_library()
    n = len(wrappers)
    cap = max([w.solutionPoolCount() for w in wrappers] + [1])
    out = (FixedResultC * (max(n, 1) * cap))()
    counts = (C.c_int * max(n, 1))()
    hs = (C.c_void_p * max(n, 1))(*[w._h for w in wrappers])
    m = L.miqp_solver_pool_solve_multi(hs, n, out, cap, counts)
    if m < 0:
        raise RuntimeError("miqp_solver_pool_solve_multi failed (%d)%s" % (m, ": " + wrappers[0].lastError() if n and m == -2 else ""))
    a = np.frombuffer(out, dtype=_FIXED_RESULT_DTYPE, count=n * cap)
    res = []
    for h in range(n):
        b = a[h * cap:h * cap + counts[h]]
        res.append((b["status"].copy(), b["objective"].copy(), b["violation"].copy(), b["iterations"].copy(), b["route"].copy()))
    return res


def improve_solution_pools(wrappers, max_passes=8, cap=None):
    """the solution pools of many wrappers hill-climbed inside their manoeuvre classes in one device call (miqp_solver_pool_improve_multi): per
    wrapper (moved, before, after, moves, status) - the arrays its own improveSolutionPool(max_passes) returns, bit for bit, and ``moved`` what
    that call returns as rc: the wrapper's entries with moves > 0.  ``cap``: entries per wrapper that take part (None: the largest
    solutionPoolCount() among the wrappers).  The wrappers may differ in their filters; one without a pool gets empty arrays and is left alone.
    Behind it solutionPoolFoundDecisions / solutionPoolFound of every wrapper report the improved records; call solve_solution_pools afterwards.
    Raises RuntimeError where the library refuses the call (wrappers of different shape, a wrapper with entries and no filter, no device), on -2
    with the first non-empty lastError() among the wrappers; a refused call leaves every pool alone."""
    L = load_library()
    n = len(wrappers)
    cap = max([w.solutionPoolCount() for w in wrappers] + [1]) if cap is None else int(cap)
    out = (PoolImproveC * (max(n, 1) * max(cap, 1)))()
    counts = (C.c_int * max(n, 1))()
    hs = (C.c_void_p * max(n, 1))(*[w._h for w in wrappers])
    rc = L.miqp_solver_pool_improve_multi(hs, n, int(max_passes), out, cap, counts)
    if rc < 0:
        why = next((w.lastError() for w in wrappers if w.lastError()), "") if rc == -2 else ""   # (a filterless handle is named in ITS last error)
        raise RuntimeError("miqp_solver_pool_improve_multi failed (%d)%s" % (rc, ": " + why if why else ""))
    a = np.frombuffer(out, dtype=np.dtype([("before", "<f8"), ("after", "<f8"), ("moves", "<i4"), ("status", "<i4")]), count=n * cap)
    res = []
    for h in range(n):
        b = a[h * cap:h * cap + counts[h]]
        res.append((int((b["moves"] > 0).sum()), b["before"].copy(), b["after"].copy(), b["moves"].copy(), b["status"].copy()))
    return res


def pool_improve_plan(move_counts):
    """the slices of a pass of improve_solution_pools for these per-entry move counts (miqp_gpu_pool_improve_plan): the list slice_first, entry
    s the first entry of slice s and the last one len(move_counts) - runs of whole entries whose (clamped) moves fit 8192 results, formed greedily
    in entry order.  Needs no device."""
    c = np.ascontiguousarray(move_counts, dtype=np.int32)
    if c.ndim != 1 or c.size == 0:
        raise ValueError("a non-empty vector of move counts expected")
    first = np.zeros(c.size + 2, dtype=np.int32)
    ns = load_library().miqp_gpu_pool_improve_plan(c.ctypes.data_as(C.POINTER(C.c_int)), c.size, first.ctypes.data_as(C.POINTER(C.c_int)), first.size)
    if ns < 1:
        raise RuntimeError("miqp_gpu_pool_improve_plan failed (%d)" % ns)
    return [int(x) for x in first[:ns + 1]]


POOL_EXPLORE_PLAIN, POOL_EXPLORE_DISTINCT, POOL_EXPLORE_SETTLED = 0, 1, 2   # MIQP_POOL_EXPLORE_* (include/miqp_gpu.h): the admission of explore_solution_pools


def _explore_dicts(records, settled):
    return [dict(parent=o.parent, **{"pass": o.pass_}, first=o.first, stride=o.stride, count=o.count, value=o.value, iterations=o.iterations,
                 objective=float(o.objective), **({"solves": o.reserved} if settled else {})) for o in records]


def explore_solution_pools(wrappers, max_passes=4, max_rel=-1.0, distinct=False, settled=False):
    """the free places of the solution pools of many wrappers filled with neighbouring manoeuvre classes in one device call
    (miqp_solver_pool_explore_multi): per wrapper (added_count, [dicts]) - what its own exploreSolutionPool(max_passes, max_rel, distinct, settled)
    returns, bit for bit, pool, last timing [2 .. 5] and lastError() behind it included.  All wrappers start pass 1 together and the neighbours of
    a pass fill common launch groups.  The wrappers may differ in filter and capacity; one whose pool is empty or full takes no part whatever its
    filter and gets (0, []).  ``distinct`` and ``settled`` together raise ValueError.  Raises RuntimeError where the library refuses the call
    (wrappers of different shape, a wrapper with entries and free places under a filter the explore cannot jump under, no device), on -2 with the
    first non-empty lastError() among the wrappers; a refused call leaves every pool alone."""
    if distinct and settled:
        raise ValueError("distinct and settled are two admissions: choose one")
    L = load_library()
    n = len(wrappers)
    cap = pool_max()
    out = (PoolExploreC * (max(n, 1) * cap))()
    counts = (C.c_int * max(n, 1))()
    hs = (C.c_void_p * max(n, 1))(*[w._h for w in wrappers])
    mode = POOL_EXPLORE_SETTLED if settled else POOL_EXPLORE_DISTINCT if distinct else POOL_EXPLORE_PLAIN
    rc = L.miqp_solver_pool_explore_multi(hs, n, mode, int(max_passes), float(max_rel), out, cap, counts)
    if rc < 0:
        why = next((w.lastError() for w in wrappers if w.lastError()), "") if rc == -2 else ""   # (a handle with a filter without jumps is named in ITS last error)
        raise RuntimeError("miqp_solver_pool_explore_multi failed (%d)%s" % (rc, ": " + why if why else ""))
    return [(int(counts[h]), _explore_dicts(out[h * cap:h * cap + counts[h]], settled)) for h in range(n)]


def pool_explore_plan(handle_totals):
    """the slices of a pass of explore_solution_pools for these per-wrapper neighbour totals (miqp_gpu_pool_explore_plan): the list slice_first,
    entry s the first wrapper of slice s and the last one len(handle_totals) - runs of whole wrappers whose neighbours fit 8192 results, formed
    greedily in order; a wrapper without neighbours rides along.  Needs no device."""
    c = np.ascontiguousarray(handle_totals, dtype=np.int32)
    if c.ndim != 1 or c.size == 0:
        raise ValueError("a non-empty vector of neighbour totals expected")
    first = np.zeros(c.size + 2, dtype=np.int32)
    ns = load_library().miqp_gpu_pool_explore_plan(c.ctypes.data_as(C.POINTER(C.c_int)), c.size, first.ctypes.data_as(C.POINTER(C.c_int)), first.size)
    if ns < 1:
        raise RuntimeError("miqp_gpu_pool_explore_plan failed (%d)" % ns)
    return [int(x) for x in first[:ns + 1]]


def pool_explore_multi_last():
    """(passes, slices) the calling thread's last explore_solution_pools ran on the device (miqp_gpu_pool_explore_multi_last)"""
    p, s = C.c_int(0), C.c_int(0)
    load_library().miqp_gpu_pool_explore_multi_last(C.byref(p), C.byref(s))
    return p.value, s.value


def carry_solution_pools(dsts, srcs, shift=1, max_rel=-1.0):
    """the kept entries of many source wrappers carried into the pools of many destination wrappers in one device call
    (miqp_solver_pool_carry_multi): pair p carries ``srcs[p]`` into ``dsts[p]``.  Per pair (added, [dict per source entry]) - what
    ``dsts[p].carrySolutionPool(srcs[p], shift, max_rel)`` returns, bit for bit, pool, last timing [2 .. 5] and lastError() behind it included.
    The settle rounds of all pairs fill common launch groups.  Sources are only read and one may feed several destinations; a pair with nothing
    to carry or a full destination takes no part and gets (0, []).  Raises ValueError for lists of different lengths and RuntimeError where the
    library refuses the call (a destination named twice or also a source, destinations of different shape, a pair the single call refuses, no
    device), on -2 with the first non-empty lastError() among the destinations; a refused call leaves every pool alone."""
    if len(dsts) != len(srcs):
        raise ValueError("one source per destination")
    L = load_library()
    n = len(dsts)
    if any(not w._loaded() for w in list(dsts) + list(srcs)):
        raise RuntimeError("miqp_solver_pool_carry_multi failed (-1): invalid parameters")
    cap = pool_max()
    out = (PoolCarryC * (max(n, 1) * cap))(*[PoolCarryC(-1, -1, 0, 0, 0, 0, float("nan")) for _ in range(max(n, 1) * cap)])   # (a pair that takes no part is not written)
    counts = (C.c_int * max(n, 1))()
    hd = (C.c_void_p * max(n, 1))(*[w._h for w in dsts]); hs = (C.c_void_p * max(n, 1))(*[w._h for w in srcs])
    ns = [min(w.solutionPoolCount(), cap) for w in srcs]
    rc = L.miqp_solver_pool_carry_multi(hd, hs, n, int(shift), float(max_rel), out, cap, counts)
    if rc < 0:
        why = next((w.lastError() for w in dsts if w.lastError()), "") if rc == -2 else ""   # (a pair the single call refuses is named in ITS destination's last error)
        raise RuntimeError("miqp_solver_pool_carry_multi failed (%d)%s" % (rc, ": " + why if why else ""))
    for p in range(n):
        dsts[p]._carried_into(int(counts[p]))
    return [(int(counts[p]), [dict(status=o.status, place=o.place, solves=o.solves, iterations=o.iterations, objective=float(o.objective))
                              for o in out[p * cap:p * cap + ns[p]] if o.status >= 0]) for p in range(n)]


def pool_carry_multi_last():
    """(rounds, launch groups) the calling thread's last carry_solution_pools ran on the device (miqp_gpu_pool_carry_multi_last)"""
    r, g = C.c_int(0), C.c_int(0)
    load_library().miqp_gpu_pool_carry_multi_last(C.byref(r), C.byref(g))
    return r.value, g.value


def certify_last_timing():
    """seconds of the last certify call of the process: dict(pack_s, upload_s, kernel_s, call_s)"""
    t = (C.c_double * 4)()
    load_library().miqp_gpu_certify_last_timing(t)
    return dict(pack_s=t[0], upload_s=t[1], kernel_s=t[2], call_s=t[3])


def materialize_results(wrappers, threads=0):
    """builds the RawResults records of a solved batch on host threads inside the library (miqp_solver_materialize_results);
    getRawResults() of each wrapper then only copies.  Returns the number of records built."""
    L = load_library()
    n = len(wrappers)
    hs = (C.c_void_p * n)(*[w._h for w in wrappers])
    return L.miqp_solver_materialize_results(hs, n, int(threads))

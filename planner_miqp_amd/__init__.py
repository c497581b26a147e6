"""planner_miqp_amd - MI355X-native MIQP solve path behind planner-miqp's CplexWrapper boundary.

The product is libmiqp_gpu.so (hand-written HIP for gfx950, C ABI in include/miqp_gpu.h); this package is the
host-side mirror of the reference's operator interface for that path (CplexWrapper, ModelParameters,
RawResults, SolutionProperties) over that C ABI.  There is no CPU fallback: importing works anywhere,
solving requires the built library and a HIP device.
"""
from .ctypes_types import ModelParameters, RawResults, Certificate, CertificateC, FixedResultC, AsNodeC, PoolImproveC, PoolExploreC, PoolCarryC  # noqa: F401
from .wrapper import (CplexWrapper, OptimizationStatus, SolutionProperties, WarmstartType, ParameterSource,  # noqa: F401
                      solve_batch, prepare_batch, materialize_results, certify_batch, certify_last_timing, load_library, library_path, build_library,
                      has_active_set, fixed_batch_chunk, pool_max, solve_fixed_multi, solve_solution_pools, pool_signature, pool_moves, pool_moves_max,
                      improve_solution_pools, pool_improve_plan, pool_jumps, pool_settle_passes, pool_shift, pool_carry_last,
                      explore_solution_pools, pool_explore_plan, pool_explore_multi_last, carry_solution_pools, pool_carry_multi_last, POOL_EXPLORE_PLAIN, POOL_EXPLORE_DISTINCT, POOL_EXPLORE_SETTLED,
                      POOL_BY_REGION, POOL_BY_ENVIRONMENT, POOL_BY_OBSTACLE, POOL_BY_CAR_CAR, POOL_EXACT_TIMING)

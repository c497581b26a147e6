/*
 * miqp_types.h - plain-C mirrors of the reference's data contract for the MIQP solve path.
 *
 * Replaces (reference paths relative to the planner-miqp checkout):
 *   struct ModelParameters   src/miqp_planner_data.hpp:99-185   -> miqp_model_params_c
 *   struct RawResults        src/miqp_planner_data.hpp:46-97    -> miqp_raw_results_c
 *   struct SolutionProperties src/cplex_wrapper.hpp:41-52       -> miqp_solution_properties_c
 *   enum OptimizationStatus  src/cplex_wrapper.hpp:54-59        -> MIQP_STATUS_*
 *   enum MiqpPlannerWarmstartType src/miqp_planner_settings.h:13-18 -> MIQP_WARMSTART_*
 *
 * Layout rule: every array is flat, row-major in the logical index order of the reference
 * member (Eigen members are column-major; the C++ adapter include/cplex_wrapper.hpp converts).
 *   x_ref[c*N+i], min_acc_x[c*R+j], possible_region[c*R+j],
 *   fraction_parameters[j*4+k], POLY_*[j*3+k],
 *   obstacle vertices [((o*N+i)*L+k)*2+{0,1}]  (index order [obstacle][time], parameters.mod:114),
 *   environment polygons: ragged, env_offsets[E+1] vertex offsets into env_vertices[2*total].
 * Polygons are counter-clockwise vertex lists (common/geometry/geometry.cpp:126-139); the edge
 * tuples <k,x1,y1,x2,y2> of the OPL model are built with wrap-around of the last vertex exactly as
 * ModelInputDataSource::addLineSet does (src/model_input_data_source.cpp:167-178).
 */
#ifndef MIQP_TYPES_H
#define MIQP_TYPES_H

#ifdef __cplusplus
extern "C" {
#endif

enum {
  MIQP_STATUS_SUCCESS = 0,
  MIQP_STATUS_FAILED_NO_SOLUT = 1,
  MIQP_STATUS_FAILED_SEG_FAULT = 2,
  MIQP_STATUS_FAILED_TIMEOUT = 3
};

enum {
  MIQP_WARMSTART_NONE = 0,
  MIQP_WARMSTART_RECEDING_HORIZON = 1,
  MIQP_WARMSTART_LAST_SOLUTION = 2,
  MIQP_WARMSTART_BOTH = 3
};

/* families of miqp_solver_set_pool_filter and miqp_gpu_pool_signature (include/miqp_gpu.h): a bit set.  Which disjunctions tell two pool entries
 * apart - by the ORDER of their alternatives along the horizon; with MIQP_POOL_EXACT_TIMING by the alternative of every step */
enum {
  MIQP_POOL_BY_REGION = 1,
  MIQP_POOL_BY_ENVIRONMENT = 2,
  MIQP_POOL_BY_OBSTACLE = 4,
  MIQP_POOL_BY_CAR_CAR = 8,
  MIQP_POOL_EXACT_TIMING = 16
};

/* CPLEX status integers reported in SolutionProperties.status (src/cplex_wrapper.cpp:672-677) */
enum {
  MIQP_CPX_STAT_OPTIMAL = 101,
  MIQP_CPX_STAT_OPTIMAL_TOL = 102,
  MIQP_CPX_STAT_INFEASIBLE = 103,
  MIQP_CPX_STAT_TIME_LIM_FEAS = 107,
  MIQP_CPX_STAT_TIME_LIM_INFEAS = 108
};

typedef struct miqp_model_params_c {
  /* solver parameters (cplexmodel/cplexmodel.mod:8-21); the CPLEX-specific knobs are accepted and ignored */
  double max_solution_time;
  double relative_mip_gap_tolerance;
  int mipdisplay, mipemphasis;
  double relobjdif;
  int cutpass, probe, repairtries, rinsheur, varsel, mircuts, parallelmode;
  /* sizes */
  int NumSteps;            /* N */
  int nr_regions;          /* R */
  int NumCars;             /* C */
  int nr_obstacles;        /* O */
  int max_lines_obstacles; /* L, every obstacle polygon has exactly L vertices */
  int nr_environments;     /* E */
  /* scalars */
  double ts;
  double min_vel_x_y, max_vel_x_y;
  double total_min_acc, total_max_acc, total_min_jerk, total_max_jerk;
  double maximum_slack;
  double WEIGHTS_SLACK, WEIGHTS_SLACK_OBSTACLE;
  double minimum_region_change_speed;
  /* [N] */
  const double* agent_safety_distance;
  const double* agent_safety_distance_slack;
  /* [C] */
  const double* WEIGHTS_POS_X; const double* WEIGHTS_VEL_X; const double* WEIGHTS_ACC_X;
  const double* WEIGHTS_POS_Y; const double* WEIGHTS_VEL_Y; const double* WEIGHTS_ACC_Y;
  const double* WEIGHTS_JERK_X; const double* WEIGHTS_JERK_Y;
  const double* WheelBase; const double* CollisionRadius;
  /* [C*6]  x,vx,ax,y,vy,ay (InitialStateIndices, miqp_planner_data.hpp:34-42) */
  const double* IntitialState;
  /* [C*N] */
  const double* x_ref; const double* vx_ref; const double* y_ref; const double* vy_ref;
  /* [C*R] */
  const double* min_acc_x; const double* max_acc_x; const double* min_acc_y; const double* max_acc_y;
  const double* min_jerk_x; const double* max_jerk_x; const double* min_jerk_y; const double* max_jerk_y;
  const int* initial_region;  /* [C], 1-based (miqp_planner.cpp:696-700) */
  const int* possible_region; /* [C*R] 0/1 */
  /* obstacles */
  const double* obstacle_vertices; /* [O*N*L*2] */
  const int* obstacle_is_soft;     /* [O] */
  /* environments */
  const int* env_offsets;          /* [E+1] */
  const double* env_vertices;      /* [2*env_offsets[E]] */
  /* [R*4], [R*3] */
  const double* fraction_parameters;
  const double* POLY_SINT_UB; const double* POLY_SINT_LB;
  const double* POLY_COSS_UB; const double* POLY_COSS_LB;
  const double* POLY_KAPPA_AX_MAX; const double* POLY_KAPPA_AX_MIN;
} miqp_model_params_c;

/* Caller-allocated result record; index order identical to RawResults (row-major here).
 * K = NumCars-1.  Entries the model does not define keep the reference's fill value 9999999
 * (src/cplex_wrapper.cpp:259).  The continuous slacks are truncated to int exactly as the
 * reference does (miqp_planner_data.hpp:84-88); the untruncated values are in the *_real arrays
 * (optional, may be NULL). */
typedef struct miqp_raw_results_c {
  int N, NrEnvironments, NrRegions, NrObstacles, MaxLinesObstacles, NrCarToCarCollisions, NrCars;
  double* u_x; double* u_y; double* pos_x; double* vel_x; double* acc_x; double* pos_y; double* vel_y; double* acc_y;
  double* pos_x_front_UB; double* pos_x_front_LB; double* pos_y_front_UB; double* pos_y_front_LB; /* each [C*N] */
  int* notWithinEnvironmentRear; int* notWithinEnvironmentFrontUbUb; int* notWithinEnvironmentFrontLbUb;
  int* notWithinEnvironmentFrontUbLb; int* notWithinEnvironmentFrontLbLb;  /* each [C*E*N] */
  int* active_region;                                                       /* [C*N*R] */
  int* region_change_not_allowed_x_positive; int* region_change_not_allowed_y_positive;
  int* region_change_not_allowed_x_negative; int* region_change_not_allowed_y_negative;
  int* region_change_not_allowed_combined;                                  /* each [C*N] */
  int* deltacc;                 /* [C*O*N*L] */
  int* deltacc_front;           /* [C*O*N*L*4] */
  int* car2car_collision;       /* [K*K*N*16] */
  int* slackvars;               /* [K*K*N*4] */
  int* slackvarsObstacle;       /* [C*O*N] */
  int* slackvarsObstacle_front; /* [C*O*N*4] */
  double* slackvars_real;       /* [K*K*N*4] or NULL */
} miqp_raw_results_c;

typedef struct miqp_solution_properties_c {
  int status;        /* CPLEX-style status integer, MIQP_CPX_STAT_* */
  double gap;        /* |best - inc| / (1e-10 + |inc|), NaN on failure */
  double objective;  /* NaN on failure */
  double time;       /* seconds spent in the solve only (src/cplex_wrapper.cpp:158-185) */
  int NrConstraints, NrBinaryVariables, NrFloatVariables, NonZeroCoefficients; /* of the raw OPL model */
  int NrIterations;  /* interior-point iterations summed over all nodes */
  int NrSolutionPool; /* number of incumbents found */
  /* extras (not in the reference struct) */
  double best_bound;
  long long nodes;
} miqp_solution_properties_c;

/* A-posteriori certificate of one delivered RawResults record against the raw big-M model (miqp_solver_certify): primal
 * feasibility and objective of the record as the caller holds it.  Row families in the generation order of the cplexmodel .mod files
 * and of miqp_solver_export_lp: A1 initial conditions, A2 dynamics, A3 global limits, A4 region block, A5 minimum speed /
 * region change, A6 environment, A7 obstacles (with the soft-obstacle alternative), A8 car/car collision. */
typedef struct miqp_certificate_c {
  double max_violation;        /* worst violation over all raw rows: lhs-rhs for <=, rhs-lhs for >=, |lhs-rhs| for = ; >= 0 */
  double objective;            /* objective_function.mod recomputed from the record: tracking, acc, jerk, obstacle slack, car/car slack */
  double family_violation[8];  /* the same maximum per row family A1..A8 */
  double max_int_infeas;       /* distance of the binary members, as delivered, from {0, 1} (ints: 0 unless a member is outside {0, 1};
                                  members are read saturated to [-128, 127]) */
  int    worst_family;         /* 1..8, 0 when max_violation == 0 */
  int    worst_row;            /* 0-based index of the worst row in the raw model's generation order (row c<worst_row+1> of
                                  miqp_solver_export_lp); ties: lowest index; -1 when max_violation == 0 */
  int    rows;                 /* rows evaluated; equals out[0] of miqp_solver_raw_sizes */
  int    status;               /* 0 evaluated; 1 the handle holds no solution (doubles NaN, ints -1) */
} miqp_certificate_c;

/* Outcome of one entry of miqp_solver_solve_fixed_batch: the continuous QP under the integer decisions of one record. */
typedef struct miqp_fixed_result_c {
  int status;       /* 0 feasible, 1 infeasible (as miqp_solver_solve_fixed returns 1), 2 entry refused - NULL record, NULL array in it,
                       sizes that differ from the instance - or not run (the call failed before its launches) */
  int route;        /* as miqp_solver_last_fixed_route for that node: 0..3; -1 for a refused entry */
  int iterations;   /* interior point iterations of the node */
  int reserved;     /* 0 */
  double objective; /* with the constant cost of step 0, as the single call reports it; NaN for status 2 */
  double violation; /* worst elastic violation of the node's rows at its solution (feasible: <= 1e-6); NaN for status 2 */
} miqp_fixed_result_c;

/* Outcome of one node of miqp_solver_solve_fixed_as: what ONE launch of the dual active-set kernel decided on one fix record (a diagnostic). */
typedef struct miqp_as_node_c {
  int status;       /* 0 solved, 1 infeasible, 2 cut off (the dual value passed the cutoff), 3 returned unsolved because the block does not hold
                       the node's rows, 4 returned unsolved because the method could not finish (64 active rows, step cap, loss of precision);
                       -1 not run (the call failed before or in its launches) */
  int steps;        /* rows added + rows dropped (0 for status 3, 4) */
  int active;       /* rows of the final active set, as handed to the children (0 unless status 0) */
  int reserved;     /* 0 */
  double objective; /* status 0: primal value of the iterate; 1, 2: the dual value reached.  With the constant cost of step 0 and the price of
                       the ignored soft-obstacle points, as miqp_solver_solve_fixed reports them; NaN for status 3, 4, -1 */
  double bound;     /* objective minus the allowance the kernel states for it: a lower bound of the node's QP (weak duality); NaN as above */
  double violation; /* worst row at the iterate (status 0: at most 5e-7, the kernel's own acceptance; status 1: 1); NaN as above */
} miqp_as_node_c;

/* Outcome of one entry of miqp_solver_pool_improve: the entry's own QP at the tight tolerance before the climb and its objective behind it. */
typedef struct miqp_pool_improve_c {
  double before;    /* objective of the entry's record as found, solved at the tight tolerance (with the constant cost of step 0) */
  double after;     /* objective of the record the call leaves; the bits of `before` exactly when moves == 0 */
  int moves;        /* accepted moves, at most one per pass */
  int status;       /* 0; 1 the entry's own QP did not come out feasible at the tight tolerance: the entry is left as it was */
} miqp_pool_improve_c;

/* One entry ADDED by miqp_solver_pool_explore: the jump that led to it and its QP at the tight tolerance. */
typedef struct miqp_pool_explore_c {
  int parent;       /* the entry of the pool it jumped from (an old entry, or one an earlier pass added) */
  int pass;         /* the pass that added it, 1 .. max_passes */
  int first, stride, count, value;   /* the jump: the parent's decision bytes d[first + k * stride], k < count, took `value` */
  int iterations;   /* interior point iterations of its node */
  int reserved;     /* 0 */
  double objective; /* with the constant cost of step 0; what miqp_solver_pool_found reports for the entry */
} miqp_pool_explore_c;

/* What miqp_solver_pool_carry answers for one entry of the SOURCE pool: what became of its shifted record on the destination's instance. */
typedef struct miqp_pool_carry_c {
  int status;       /* 0 admitted; 1 its first solve on the destination's instance was not feasible; 2 unmappable (a region it uses is not possible on
                       the destination); 3 its signature under the destination's filter is in the pool; 4 no settled labels, or the signature of its
                       settled labels is in the pool; 5 beyond the cost cap; 6 new in every respect, but no place is free */
  int place;        /* the entry of the destination's pool it became; -1 unless status 0 */
  int solves;       /* the solves its settling took (0 for status 2) */
  int iterations;   /* interior point iterations of its first solve (0 for status 2) */
  int reserved;     /* 0 */
  int reserved1;    /* 0 */
  double objective; /* of its first solve, with the constant cost of step 0: what miqp_solver_pool_found reports for an admitted entry; NaN for status 2 */
} miqp_pool_carry_c;

#ifdef __cplusplus
}
#endif
#endif /* MIQP_TYPES_H */

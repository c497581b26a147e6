/*
 * miqp_gpu.h - C ABI of libmiqp_gpu.so, the MI355X-native replacement of the reference's
 * CPLEX/OPL solve path (L1+L2+L3 of SURVEY.md section 1).
 *
 * Each entry point names the reference interface it replaces (paths relative to the planner-miqp
 * checkout).  The Eigen-typed class with the reference's own name and methods is the header-only
 * adapter include/cplex_wrapper.hpp, which forwards to these functions.
 *
 * Threading: one caller thread per solver handle (src/cplex_wrapper.hpp:61-275 has the same contract: one IloEnv
 * per wrapper).  Handles are independent objects; the device buffers behind them are kept per HIP device and a solve
 * holds that device's lock, so threads with different handles may call concurrently (same device: the solves run one
 * after the other; different devices: in parallel).  No GPU context is touched before the first solve.
 */
#ifndef MIQP_GPU_H
#define MIQP_GPU_H

#include "miqp_types.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct miqp_solver miqp_solver_t;

typedef struct miqp_solver_opts {
  int precision;            /* CplexWrapper ctor `precision` (cplex_wrapper.hpp:81-115); inputs are rounded to
                               precision-2 decimals like ModelInputDataSource (hpp:88); <= 0 -> 12 */
  int device;               /* HIP device ordinal, -1: the calling thread's current device */
  int nodes_per_round;      /* B&B nodes solved per instance and round (0: default = 32768 / batch size, within 16..16384) */
  int max_open_nodes;       /* per-instance open-list capacity (0: default = 2^27 / batch size, within 32768..2^20, and at
                               most an eighth of the free device memory) */
  double gap_override;      /* < 0: use ModelParameters.relative_mip_gap_tolerance */
  int verbose;
} miqp_solver_opts;

/* CplexWrapper::CplexWrapper(...) / ~CplexWrapper()            src/cplex_wrapper.hpp:81-158 */
miqp_solver_t* miqp_solver_create(const miqp_solver_opts* opts);
void miqp_solver_destroy(miqp_solver_t* s);

/* CplexWrapper::resetParameters(shared_ptr<ModelParameters>)   src/cplex_wrapper.cpp:661-664
 * + ModelInputDataSource::read (rounding, edge tuples)         src/model_input_data_source.cpp:180-275
 * The arrays are copied; returns 0 on success, <0 on invalid sizes. */
int miqp_solver_set_params(miqp_solver_t* s, const miqp_model_params_c* p);

/* CplexWrapper::setParameterDatFileAbsolute + DATFILE source   src/cplex_wrapper.cpp:30-42
 * Reads the OPL .dat subset of the fixtures (no rounding, as OPL would). */
int miqp_solver_load_dat(miqp_solver_t* s, const char* path);

/* CplexWrapper::overrideSolverSettingsDataSource               src/cplex_wrapper.cpp:893-896 */
int miqp_solver_override_settings(miqp_solver_t* s, double max_solution_time, double relative_mip_gap_tolerance);

/* CplexWrapper::addRecedingHorizonWarmstart / setLastSolutionWarmstart   src/cplex_wrapper.cpp:459-483
 * + initializeWarmstart / addMIPStart / readMIPStarts                    src/cplex_wrapper.cpp:124-138, 494-639
 * The record is copied.  Two starts can be registered at once, as the reference does with
 * BOTH_WARMSTART_STRATEGIES: type MIQP_WARMSTART_LAST_SOLUTION fills the last-solution slot, every other type the
 * receding-horizon slot; MIQP_WARMSTART_NONE (or start == NULL) clears both.  Each start is tried as an initial
 * incumbent (CPLEX MIPStartSolveMIP: the binaries of the start are fixed, the continuous QP is solved on the device; an
 * infeasible start, or one whose seven sizes differ from the instance, is ignored).  Starts stay registered across
 * miqp_solver_set_params.  Returns 0, <0 when the record is refused. */
int miqp_solver_set_warmstart(miqp_solver_t* s, const miqp_raw_results_c* start, int warmstart_type);

/* CplexWrapper::callCplex(timestamp)                           src/cplex_wrapper.cpp:65-249
 * Returns OptimizationStatus (MIQP_STATUS_*); never throws.  Fails with MIQP_STATUS_FAILED_SEG_FAULT when
 * no HIP device / kernel image is available - there is no CPU fallback. */
int miqp_solver_solve(miqp_solver_t* s, double timestamp);

/* Batch of independent instances (receding-horizon steps / scenario seeds) solved concurrently on one
 * device; statuses[k] receives the OptimizationStatus of solver k.  All instances must share
 * NumCars, NumSteps, nr_regions, nr_environments, nr_obstacles, max_lines_obstacles and opts.device.
 * Returns 0 on success.  (MiqpPlanner issues one callCplex at a time, src/miqp_planner.cpp:731; the batch entry
 * is what a scenario-parallel caller binds.) */
int miqp_solver_solve_batch(miqp_solver_t* const* solvers, int n, int* statuses);

/* The same call as a QUEUE drained with at most `inflight` instances in flight on the device (<= 0 or >= n: all at once =
 * miqp_solver_solve_batch): an instance that is proven - or has used up its own max_solution_time, counted from its
 * admission - hands its slot (open lists in HBM) to the next instance of the queue at the following branch-and-bound
 * round, so the device never idles behind the hardest instances of a batch.  SolutionProperties.time of an instance is the
 * time from its admission to its proof.  (No reference counterpart: MiqpPlanner issues one callCplex at a time,
 * src/miqp_planner.cpp:731; this is the entry a scenario-parallel caller binds to keep one GPU saturated.)
 * The device context (node pool, lists) is kept between calls of the same shape - slots, model dimensions - whose queue is no
 * longer than the per-instance arrays of the context hold (64 x inflight at least); miqp_solver_last_setup says whether a call
 * had to build it.  A single solve (miqp_solver_solve) returns the same result bit for bit when repeated, as CPLEX's default
 * deterministic mode does; the instances of a queue influence each other's shares of a round, so their node counts move by a
 * few nodes between runs (every reported bound and solution is valid either way). */
int miqp_solver_solve_stream(miqp_solver_t* const* solvers, int n, int inflight, int* statuses);

/* The same batch sharded over the first `gpus` HIP devices of this process (<= 0: all visible): instance b runs on
 * device b mod gpus with one host thread per device and no exchange between the shards;
 * opts.device of every handle is set to the device it ran on. */
int miqp_solver_solve_batch_multi(miqp_solver_t* const* solvers, int n, int gpus, int* statuses);

/* ---- one hard instance split over the ranks of a job (the reference walks its alternative
 * start configurations one after the other on one CPU, src/miqp_planner.cpp:694-749) ----
 * Every rank loads the SAME instance into its own handle and calls miqp_solver_solve_split with its rank.  The alternatives
 * of one or two car/car disjunctions partition the branch-and-bound tree over the ranks; once per round the ranks run
 * `exchange(user, 0, words, 4, 0)` = in-place all-reduce(min) over `count` unsigned 64-bit words (incumbent | owner rank,
 * lower bound, done, time-up: the best incumbent prunes everywhere, every rank takes the same stop decision), and at the
 * end `exchange(user, 1, buf, nbytes, root)` = broadcast of the owner's solution.  The callback returns 0 on success.
 * Returns the OptimizationStatus, identical on every rank, and every rank holds the full result. */
typedef int (*miqp_exchange_fn)(void* user, int op, void* buf, int count, int root);
int miqp_solver_solve_split(miqp_solver_t* s, double timestamp, int world, int rank, miqp_exchange_fn exchange, void* user);

/* Built-in transport of that exchange: RCCL (librccl is loaded at run time) over xGMI, one communicator per process.
 * Rank 0 creates the 128-byte id (miqp_comm_unique_id) and hands it to the others by any means (e.g. the launcher's
 * store); every rank then calls miqp_comm_init with the device it solves on.  miqp_solver_solve_split_rccl = solve_split
 * with ncclAllReduce(ncclUint64, ncclMin) / ncclBroadcast on the solver's stream. */
int miqp_comm_unique_id(char* out128);
int miqp_comm_init(int world, int rank, const char* id128, int device);
int miqp_comm_finalize(void);
int miqp_solver_solve_split_rccl(miqp_solver_t* s, double timestamp);
/* checks a transport against the contract above (min over unsigned words incl. values with the top bit set, broadcast from
 * every root); exchange == NULL: the RCCL communicator of miqp_comm_init.  0 when it conforms. */
int miqp_comm_selftest(miqp_exchange_fn exchange, void* user, int world, int rank);

/* the roots rank `rank` of `world` starts from in a tree split of the loaded instance (no device needed): writes up to `cap`
 * entries of (record index, alternative) pairs flattened as root_of_pair[k], index[k], value[k]; returns the number of pairs,
 * *nroots_out = the number of roots of this rank, *ncombos_out = the size of the partition */
int miqp_solver_split_roots(const miqp_solver_t* s, int world, int rank, int* root_of_pair, int* index, int* value, int cap, int* nroots_out, int* ncombos_out);

/* cplex.getNrows / getNbinVars / getNcols - getNbinVars / getNNZs of the model OPL would generate for the loaded
 * instance (collectCplexStatistics, src/cplex_wrapper.cpp:679-690): out[0..3] = rows, binary columns, continuous
 * columns, non-zeros.  Needs no device. */
int miqp_solver_raw_sizes(const miqp_solver_t* s, int* out4);
/* Diagnostic (no reference counterpart, no device needed): the response tables behind the bound lifting of the branch and
   bound - for every (car, axis, step) the 4 x 4 matrix Zu H^-1 Zu' of the chain's (position, velocity,
   acceleration, jerk) at that step under the objective's Hessian; out[((car * 2 + axis) * N + step) * 16 + 4 a + b].
   Returns the number of doubles written, < 0 on error (-3: cap too small). */
int miqp_solver_lift_tables(const miqp_solver_t* s, double* out, int cap);

/* CplexWrapper::getRawResults()                                src/cplex_wrapper.hpp:204, cpp:311-448
 * Fills the caller-allocated record (sizes must match the instance). */
int miqp_solver_get_results(const miqp_solver_t* s, miqp_raw_results_c* out);

/* collectRawResults for a whole batch                           src/cplex_wrapper.cpp:186 (collectRawResults() runs inside callCplex, before it returns)
 * Builds the RawResults record of every handle that holds a solution, on `threads` host threads (0: up to 32 - more contend for the allocator), and
 * keeps it inside the handle; miqp_solver_get_results then only copies.  The reference produces the record inside callCplex;
 * the batch entry points leave it to this call so that a service can overlap it - bench.py calls it inside its timed region.
 * Returns the number of records built, < 0 on error. */
int miqp_solver_materialize_results(miqp_solver_t* const* solvers, int n, int threads);

/* CplexWrapper::getSolutionProperties()                        src/cplex_wrapper.hpp:206-208, cpp:672-690 */
int miqp_solver_get_properties(const miqp_solver_t* s, miqp_solution_properties_c* out);

/* sizes of the loaded instance: out[0..5] = NumCars, NumSteps, nr_regions, nr_environments,
 * nr_obstacles, max_lines_obstacles                            (collectRawResults, cpp:314-327) */
int miqp_solver_get_dims(const miqp_solver_t* s, int* out6);

/* cplex.exportModel(".lp") debug output                        src/cplex_wrapper.cpp:150-154 */
int miqp_solver_export_lp(const miqp_solver_t* s, const char* path);

/* opl.printExternalData(): the loaded parameters as OPL external data (.dat syntax, re-readable by
 * miqp_solver_load_dat and by OPL)                              src/cplex_wrapper.cpp:141-149
 * (test_hardcoded_data_versus_datfile, test/cplex_wrapper_test.cc:474-505) */
int miqp_solver_write_dat(const miqp_solver_t* s, const char* path);

/* opl.printSolution(): every decision variable of the last solution as `name = [...]` blocks
 * (layout of cplexmodel/modelRun.txt)                           src/cplex_wrapper.cpp:212-219 */
int miqp_solver_write_solution(const miqp_solver_t* s, const char* path);

/* cplex.writeMIPStarts(): the last solution as a CPLEX MIP start (.mst XML, variable names of the LP export)
 *                                                               src/cplex_wrapper.cpp:206-209, 221-228 */
int miqp_solver_write_mst(const miqp_solver_t* s, const char* path);

/* cplex.readMIPStarts(): loads an .mst written by miqp_solver_write_mst (or by CPLEX for the exported .lp) as the
 * MIP start of the next solve; returns 0 when the start was accepted  src/cplex_wrapper.cpp:128-138 */
int miqp_solver_read_mst(miqp_solver_t* s, const char* path);

/* continuous QP with the binaries of `fixed` asserted, solved by the device interior-point kernel
 * (used by the parity tests to compare the QP machinery with the CPU oracle and with K3);
 * returns 0 when feasible */
int miqp_solver_solve_fixed(miqp_solver_t* s, const miqp_raw_results_c* fixed, miqp_raw_results_c* out,
                            double* objective, int* iterations);

/* timing of the last solve / batch in seconds, measured with HIP events on the solver stream:
 * out[0] = whole solve, out[1] = interior-point kernel total, out[2] = number of IPM kernel launches,
 * out[3] = node relaxations solved, out[4] = IPM iterations (summed over nodes), out[5] = rows x iterations */
int miqp_solver_last_timing(const miqp_solver_t* s, double* out6);

/* the dual active-set launches of the last solve / batch (one and two cars of up to 20 steps, miqp_gpu_has_active_set: the node relaxations of a round; the reference's counterpart is CPLEX's dual
 * simplex re-solve of a child node inside cplex.solve(), src/cplex_wrapper.cpp:158-185): out[0] = node relaxations they solved,
 * out[1] = their steps (rows added + rows dropped; they are part of out[4] of miqp_solver_last_timing and of NrIterations),
 * out[2] = nodes they could not finish (returned unsolved, solved by the interior point a round later), out[3] = rows dropped,
 * out[4] = sum over the nodes of the active rows at the end, out[5] = sum of the rows taken over from the parents' active sets,
 * out[6] = seconds of the STANDARD active-set launches alone (HIP events on the solver stream: from the start of a round's launch group
 * to the end of that kernel; the other three launches of the group run beside it on their own streams), out[7] = number of those launches */
int miqp_solver_last_active_set(const miqp_solver_t* s, double* out8);

/* which launch of the interior-point chain solved the node of the last miqp_solver_solve_fixed call of this handle (read back from the
 * hand-over counters the chain keeps; a diagnostic for tests that pin each kernel): 0 = the standard on-chip kernel, 1 = its larger
 * variant (the node has more general rows than the standard block holds), 2 = the memory-backed kernel (more than the larger block
 * holds), 3 = the memory-backed kernel because the shape has no on-chip kernel (three or four cars, more than 20 steps);
 * -1 = the handle's last such call did not get through its launches (refused record, no device), or there was none */
int miqp_solver_last_fixed_route(const miqp_solver_t* s);

/* n fix records of the instance loaded in s, solved as nodes of common launches: what miqp_solver_solve_fixed answers for one record, for
 * many in one device call - one compilation of the instance, one upload of its tables, one device lock.  No reference counterpart: the
 * reference walks its alternative start configurations one after the other, a cplex.solve() each (src/miqp_planner.cpp:694-749).
 * The entries go through the serial interior point chain of the single call in launch groups of miqp_gpu_fixed_batch_chunk nodes, with its
 * settings, and every entry is answered bit for bit as the single call answers it alone, whatever its place and its neighbours.
 * out[n] receives one result each.  *best (may be NULL) = index of the feasible entry with the lowest objective, ties to the lower index,
 * -1 when none is feasible.  n is at most 65536.
 * Returns 0, -1 invalid arguments / no instance (n <= 0, NULL arrays), -2 shape refused (as the solve refuses it),
 * -3 no device / kernel image / HIP error (every entry then has status 2: not run), -5 n above 65536.
 * A refused ENTRY - NULL record, NULL array in it, sizes that differ from the instance - is status 2 of that entry and does not fail the call.
 * The handle keeps the trajectories and fix records of the call for miqp_solver_fixed_batch_record until its next such call or its next
 * parameters.  Needs a device context of its own sizes: it rebuilds the one a solve or a single call left, and they rebuild theirs after it.
 * miqp_solver_last_timing then reports out[0] = the whole call, out[1] = of which on the device (first launch group to last kernel),
 * out[2] = launch groups, out[3] = entries run, out[4] = their iterations. */
int miqp_solver_solve_fixed_batch(miqp_solver_t* s, const miqp_raw_results_c* const* fixed, int n, miqp_fixed_result_c* out, int* best);

/* the RawResults record of entry k of the handle's last miqp_solver_solve_fixed_batch call (no reference counterpart): built from the kept
 * trajectory and fix record with the canonical completion of the binaries, as the single call builds its `out`.
 * 0, 1 when entry k was not feasible (or refused), -1 bad k / no batch held, -2 sizes of out differ from the instance. */
int miqp_solver_fixed_batch_record(miqp_solver_t* s, int k, miqp_raw_results_c* out);

/* sizeof(miqp_fixed_result_c) of the built library (binding check; no reference counterpart) */
int miqp_gpu_fixed_result_size(void);
/* nodes per launch group of miqp_solver_solve_fixed_batch: a constant of the build (no reference counterpart; no device is needed or touched) */
int miqp_gpu_fixed_batch_chunk(void);

/* DIAGNOSTIC: n fix records of the instance loaded in s (at most miqp_gpu_fixed_batch_chunk) as nodes of the dual ACTIVE-SET launches, one
 * launch per generation and cutoff value, each node read back as the kernel left it.  No reference counterpart (the reference's node re-solves
 * are CPLEX's, src/cplex_wrapper.cpp:158-185); no solve runs this path - it exists so that the tests can hold the kernel against the oracle
 * node by node (tests/test_as_node_gpu.py).
 * start (NULL: every node cold): start[k] = -1 cold; p with 0 <= p < k: node k starts from node p's final active set and the M that belongs to
 * it, as a child starts from its parent in a search; -(p + 2): the same active set with the tag of M cleared, so that the kernel rebuilds M
 * column by column and inverts it.  Nodes run in generations: the cold ones, then their children, and so on.
 * block: 0 the standard block of the launches, 1 the larger one; kernel, LDS size and grid are the round planner's.
 * cutoff (NULL: none): per node, in the units of the returned objective; a NaN or a value of 1e299 and above is none.
 * out[n]: one miqp_as_node_c each.  info32 (may be NULL): the 32 counters of the launches' statistics summed over the call - [0] nodes
 * finished, [1] their steps, [2] nodes not finished, [3] rows dropped, [4] infeasible, [5] cut off, [6] active rows at the end, [7] rows taken
 * over from the parents, [8] nodes started from the parent's M, [9] starts that fell back to a cold one, [11] .. [15] why a node was not
 * finished (no free slot, step cap, curvature, pivot of a down-date, rows off their equalities), [16] .. [19] why M was rebuilt (no ring,
 * the parent left none, the ring has come round, another row count).
 * Returns 0, -1 invalid arguments / no instance / block not 0 or 1, -2 shape refused (as the solve refuses it), -3 no device / kernel image /
 * HIP error, -4 a record is refused (as miqp_solver_solve_fixed refuses it), -5 n above the chunk, -6 the shape has no active-set launches
 * (miqp_gpu_has_active_set), -7 the launches are switched off (MIQP_AS=0), -8 start[k] names node k or a later one, -9 the device context has
 * no launch of that block or keeps no active sets.  miqp_solver_last_error has the text.  Everything but -3 and -9 is decided without a device.
 * The handle keeps trajectories and fix records for miqp_solver_fixed_as_record, in place of those of a miqp_solver_solve_fixed_batch call. */
int miqp_solver_solve_fixed_as(miqp_solver_t* s, const miqp_raw_results_c* const* fixed, int n, const int* start, int block, const double* cutoff,
                               miqp_as_node_c* out, unsigned long long* info32);
/* the RawResults record of node k of the handle's last miqp_solver_solve_fixed_as call, as miqp_solver_fixed_batch_record builds its own:
 * 0, 1 when node k was not solved (any status but 0), -1 bad k / nothing held, -2 sizes of out differ from the instance. */
int miqp_solver_fixed_as_record(miqp_solver_t* s, int k, miqp_raw_results_c* out);
/* sizeof(miqp_as_node_c) of the built library (binding check) */
int miqp_gpu_as_node_size(void);

/* ---- solution pool: the K best distinct integer solutions of a solve.  Counterpart of the CPLEX solution pool - IloCplex::getSolnPoolNsolns,
 * getObjValue(i), getValues(x, i) - which a user of the reference reaches through the IloCplex its wrapper owns; the reference source has no call
 * site for it. ----
 * miqp_solver_set_pool: the next solves of the handle keep up to `capacity` solutions, 0 <= capacity <= miqp_gpu_pool_max(); 0 (the default) = off:
 * then nothing is allocated and no kernel is launched for it.  Returns 0, -1 NULL handle, -2 capacity out of range (the previous setting stays).
 * With a pool, every integer-feasible leaf the branch and bound evaluates is merged on the device into the pool of its instance, which keeps the
 * `capacity` smallest DISTINCT ones in the order (objective as found, hash of the record, bytes of the record) - a function of the set of leaves seen,
 * not of their arrival order, so the pool of a single solve is reproducible bit for bit like the solve itself.  Two leaves are the same entry when they
 * decide every disjunction alike.  The incumbent of the solve is entry 0, at every capacity.  (The search compares objectives to 44 bits and breaks
 * ties by a hash of its own; among records whose objectives agree to those 44 bits the incumbent's is put first whatever the order above says, so
 * the found objectives do not decrease up to that resolution, 2.4e-10 relative.)  The solve, its tree and its result are the same with and without a pool.
 * Works in miqp_solver_solve, _solve_batch, _solve_stream (per handle: handles with and without a pool may share a call) and _solve_batch_multi (each
 * device on its own).  A rank of miqp_solver_solve_split keeps the pool of its OWN search: pools are not exchanged.
 * Device memory: instances of the call x largest capacity among them x (record bytes + 12); a pool that does not fit fails the call like any other
 * allocation failure, and miqp_solver_last_error says so. */
int miqp_solver_set_pool(miqp_solver_t* s, int capacity);
/* number of entries the handle's last solve kept (getSolnPoolNsolns): 0 with the pool off, before a solve, without a solution and after
 * miqp_solver_set_params / _load_dat.  Needs no device.  Behind miqp_solver_pool_solve it is the number that call left: the search tells leaves apart
 * by what they decide, and two such records can be ONE solution - the optimum of one also holds the alternatives the other asserts, so both QPs have
 * the same minimiser and their RawResults carry the same binaries.  Only the refinement sees that; it merges them (the best found stays), and
 * the count, the found objectives and the entry numbers are from then on those of the merged pool.  Until then the count is an upper bound. */
int miqp_solver_pool_count(const miqp_solver_t* s);
/* the objectives of those entries as the search found them (node tolerance; constant cost included), best first: obj[0 .. min(count, cap) - 1];
 * returns how many were written, -1 on NULL arguments.  Needs no device. */
int miqp_solver_pool_found(const miqp_solver_t* s, double* obj, int cap);
/* refines the kept entries: their continuous QPs at the tight tolerance, as nodes of one fixed-batch call (miqp_solver_solve_fixed_batch: one context,
 * one upload of the tables, one device lock), out[k] in pool order for k < min(count, cap).  Every entry is answered as miqp_solver_solve_fixed
 * answers the entry's record (miqp_solver_pool_record), bit for bit: for that the call labels each record with the canonical binaries of its own
 * solution and solves again while labels move (a few launch groups; miqp_solver_last_timing out[2] = their number, out[0], out[1], out[3], out[4] as
 * for the fixed batch; out[5] = 1 when labels still moved after the last pass - the entries are then answers to the labels of that pass, and
 * miqp_solver_last_error says so - else 0).  Entries that come out with the same binaries are one solution and are merged (see miqp_solver_pool_count): the records of
 * miqp_solver_pool_record differ pairwise in at least one binary.  Returns the number of entries left, which out[] then holds and
 * miqp_solver_pool_count reports (0: nothing kept), -1 invalid arguments / no instance, -3 no device / kernel image / HIP error.
 * The handle keeps the trajectories for miqp_solver_pool_record until its next solve, pool_solve or parameters.  Like the fixed batch it needs a device
 * context of the batch call's sizes: it rebuilds the one the solve left, and the next solve rebuilds its own. */
int miqp_solver_pool_solve(miqp_solver_t* s, miqp_fixed_result_c* out, int cap);
/* the RawResults record of entry k of the handle's last miqp_solver_pool_solve (getValues(x, i)), built as miqp_solver_fixed_batch_record builds its own.
 * 0, 1 when entry k did not come out feasible at the tight tolerance, -1 bad k / no refined pool held, -2 sizes of out differ from the instance. */
int miqp_solver_pool_record(miqp_solver_t* s, int k, miqp_raw_results_c* out);
/* largest capacity miqp_solver_set_pool accepts: a constant of the build (no device is needed or touched) */
int miqp_gpu_pool_max(void);

/* ---- manoeuvre filter of the solution pool: which leaves are ONE entry.  Counterpart of the diversity filter of the CPLEX pool
 * (IloCplex::addDiversityFilter); the reference source has no call site for it. ----
 * Without a filter two leaves are the same entry when they agree in every decision byte, and the near-optimal leaves of one manoeuvre - the same
 * alternatives, changed a step earlier or later - fill the pool.  With a filter two leaves are the same entry when their SIGNATURES under `families`
 * are equal, and the pool keeps the smallest member (in the pool's order) of each class: the `capacity` smallest class minima of the set of leaves
 * seen, still a function of that set and reproducible bit for bit.
 * families: a bit set of MIQP_POOL_BY_REGION (1), _BY_ENVIRONMENT (2), _BY_OBSTACLE (4), _BY_CAR_CAR (8), MIQP_POOL_EXACT_TIMING (16); 0 (the
 * default) = off: then nothing is allocated, launched or changed.  MIQP_POOL_BY_OBSTACLE | MIQP_POOL_BY_CAR_CAR (12) is the setting for a planner
 * that wants fallbacks: one entry per side of each obstacle and order of the cars.  31 is by definition the unfiltered pool.
 * The signature of the D decision bytes d of a fix record (D = cars * steps * 6 + cars * obstacles * steps * 5 + pairs * steps * 4, pairs =
 * cars * (cars - 1) / 2; per step i the region code of car c at d[c * steps + i], the environment piece of point pt at d[cars * steps + (c * steps + i)
 * * 5 + pt], the obstacle edge at d[6 * cars * steps + ((c * obstacles + o) * steps + i) * 5 + pt], the car/car alternative of pair p, group g behind
 * those at [(p * steps + i) * 4 + g]): D bytes, -1 except on the positions of the selected families.  A SITE is one such disjunction followed over i.
 * Per site: the bytes of steps 1 .. steps - 1 that are not negative - of a region code its possible-region index, code >> 2 - with repeats of the
 * value before collapsed, written left-packed to the site's positions of steps 1, 2, ...: what is decided in which order, not at which step.  With
 * MIQP_POOL_EXACT_TIMING the site's bytes as they are, step 0 included.
 * The incumbent stays entry 0: when its record is not kept but an entry of its signature is, it takes that entry's place.  miqp_solver_pool_solve and
 * _pool_solve_multi also merge entries whose final labels have one signature.  Device memory: instances x largest capacity x record bytes more
 * (the signatures of the entries kept), only in a call that has a handle with a filter.
 * miqp_solver_set_pool_filter: 0, -1 NULL handle, -2 families outside 0 .. 31 (the previous setting stays).  The setting lasts like the capacity. */
int miqp_solver_set_pool_filter(miqp_solver_t* s, int families);
/* the signature of decisions[0 .. D) into out[0 .. D): a pure function on bytes, no handle, no device.  Returns D; -1 NULL pointers or a
 * non-positive dimension (obstacles may be 0), -2 families outside 1 .. 31, -3 len < D. */
int miqp_gpu_pool_signature(int cars, int steps, int obstacles, int families, const signed char* decisions, signed char* out, int len);
/* ... of a RawResults record of the handle's instance: its fix record (the first alternative that holds, as miqp_solver_solve_fixed reads it), then
 * the function above.  Returns D; -1 NULL arguments / no instance, -2 a record without its arrays or families outside 1 .. 31, -3 sizes of the
 * record differ from the instance, -4 cap < D.  Needs no device. */
int miqp_solver_pool_signature(const miqp_solver_t* s, const miqp_raw_results_c* rec, int families, signed char* out, int cap);
/* the D decision bytes of entry k of the handle's pool as the search kept it (miqp_solver_pool_solve does not change them; entries it merges away
 * leave).  Returns D; -1 NULL arguments, bad k or no pool, -3 cap < D.  Needs no device. */
int miqp_solver_pool_found_decisions(const miqp_solver_t* s, int k, signed char* out, int cap);

/* ---- fix records and solution pools of MANY handles in one device call: one device lock, one context, the n instances compiled on host threads and
 * their tables uploaded once, the nodes of all handles in common launch groups of miqp_gpu_fixed_batch_chunk nodes. ----
 * miqp_solver_solve_fixed_multi: entries first[h] .. first[h + 1] - 1 of fixed[] are fix records of the instance loaded in solvers[h] (first has n + 1
 * entries, ascending, first[0] == 0; an empty range is allowed).  For every handle the call answers what miqp_solver_solve_fixed_batch(solvers[h], ...)
 * answers for that handle's records alone, bit for bit: out[first[h] + k] per entry, best[h] (may be NULL) = index INSIDE the handle's range of its
 * feasible entry with the lowest objective, ties to the lower index, -1 when none is feasible; and every handle keeps what the single call leaves
 * for miqp_solver_fixed_batch_record (a handle with an empty range keeps nothing).  The context has the common Layout of the handles; a node gives
 * the same bits under it as under its own instance's.
 * Returns 0; -1 invalid arguments (NULL arrays, n <= 0, a handle without an instance, a handle named twice, a `first` that does not ascend from 0);
 * -2 handles that do not share a shape (as miqp_solver_solve_batch refuses them; miqp_solver_last_error says why) or name different devices;
 * -5 more than 65536 entries in all; -3 no device / kernel image / HIP error (every entry then has status 2: not run).  -1, -2 and -5 are found
 * before any device is touched and leave what the handles keep alone; a call with nothing to run returns 0 without touching a device.
 * A refused ENTRY - NULL record, NULL array in it, sizes that differ from its handle's instance - is status 2 of that entry and does not fail the call.
 * miqp_solver_last_timing of every handle of the call then reports out[0] = the whole call, out[1] = of which on the device, out[2] = launch groups
 * (all three of the CALL), out[3] = the handle's own entries run, out[4] = their iterations.  No reference counterpart. */
int miqp_solver_solve_fixed_multi(miqp_solver_t* const* solvers, int n, const miqp_raw_results_c* const* fixed, const int* first, miqp_fixed_result_c* out, int* best);
/* refines the pools of n handles as miqp_solver_pool_solve refines one - the re-labelling passes, the merge of entries that end with the same
 * binaries, miqp_solver_pool_count and what miqp_solver_pool_record hands out afterwards are those of the single call, bit for bit - with the entries
 * of all handles as nodes of common launch groups; a pass re-runs only the entries of handles whose labels moved.  out[h * cap + k], k < counts[h],
 * receives the entries left of handle h (at most min(count, cap) are refined, cap >= 1); a handle with an empty pool gets counts[h] = 0 and nothing written.
 * Returns the total number of entries left (0: no handle kept anything - no device is touched then), -1 / -2 / -5 / -3 as
 * miqp_solver_solve_fixed_multi.  miqp_solver_last_timing of every handle: out[0], out[1] of the call, out[2] = passes the handle's entries took,
 * out[3] = its entries left, out[4] = their iterations, out[5] = 1 when the handle's labels still moved after the last pass (miqp_solver_last_error of
 * that handle says so), else 0.  No reference counterpart. */
int miqp_solver_pool_solve_multi(miqp_solver_t* const* solvers, int n, miqp_fixed_result_c* out, int cap, int* counts);

/* ---- the kept entries of a FILTERED pool improved inside their manoeuvre classes.  The filter keeps, of each class, the smallest
 * leaf the search happened to evaluate; the best trajectory of the class usually changes its alternatives at other steps.  No reference counterpart. ----
 * A MOVE is (first, stride, count, value): the decision bytes d[first + k * stride], k < count, take `value`.  Of every site (one disjunction along
 * the horizon, bytes b[i]) and every change point i = 2 .. N - 1 (b[i] != b[i - 1], both decided): L1 b[i] := b[i - 1]; L2 b[i], b[i + 1] := b[i - 1]
 * when i + 1 < N; E1 b[i - 1] := b[i]; E2 b[i - 2], b[i - 1] := b[i] when i - 2 >= 1.  Step 0 is never written.  A move is kept when the site's
 * family is not in `families` or the site's signature under `families` is the same behind it.  Order: site, change point, L1 L2 E1 E2; at most
 * miqp_gpu_pool_moves_max() per record, the first ones in that order.
 * miqp_gpu_pool_moves: the kept moves of a record of D decision bytes, 4 ints each, into moves4[4 * cap].  Returns their number; -1 NULL pointers or
 * a non-positive dimension, -2 families outside 1 .. 15 (without a family, or with MIQP_POOL_EXACT_TIMING, every move changes the signature), -3 cap
 * too small.  Pure host code: no handle, no device. */
int miqp_gpu_pool_moves(int cars, int steps, int obstacles, int families, const signed char* decisions, int* moves4, int cap);
int miqp_gpu_pool_moves_max(void);
/* sizeof(miqp_pool_improve_c) of the built library (binding check) */
int miqp_gpu_pool_improve_size(void);
/* n decision records of D bytes each (the format of miqp_solver_pool_found_decisions), completed to fix records as the pool's are - every byte behind
 * D is "none" - and solved as the nodes of one fixed-batch call: contract, return codes and miqp_solver_last_timing are those of
 * miqp_solver_solve_fixed_batch, every entry is answered bit for bit whatever its place and its neighbours, and miqp_solver_fixed_batch_record hands
 * out the trajectories.  A record with a byte that is neither -1 (undecided) nor an alternative of its site - a possible region of the car and one of
 * its half-plane alternatives, an environment piece, an obstacle edge or, for a soft obstacle, max_lines_obstacles, a car/car alternative 0 .. 3 - is
 * status 2 of that entry and never reaches the device. */
int miqp_solver_solve_decisions(miqp_solver_t* s, const signed char* decisions, int n, miqp_fixed_result_c* out, int* best);
/* hill-climbs the first min(count, cap) entries of the handle's pool as found, each inside its own class under the handle's filter, in one
 * device-resident loop: pass 0 solves the entries' own records at the tight tolerance (out[k].before; an entry that is not feasible there gets
 * status 1 and is left as it is); every further pass solves all kept moves of every entry that moved in the pass before (all live entries in pass 1)
 * as nodes of the fixed-batch chain (an entry that did not move is not expanded again: its neighbours are the ones just rejected) and applies, per entry, the feasible neighbour of the lowest objective (ties: the lower move number) when it is
 * below the entry's objective by more than 1e-9 (1 + |objective|).  Ends when no entry moved or after max_passes passes; the objectives decrease
 * strictly, so it ends.  Results are a function of the records alone: the call is reproducible bit for bit.
 * Afterwards miqp_solver_pool_found_decisions reports the improved bytes and miqp_solver_pool_found out[k].after - TIGHT-tolerance objectives from
 * then on, for the live entries.  Entries keep their places (no re-sort: the found objectives need not ascend any more); entry 0 stays the
 * incumbent's class and may come out better than the solve's result.  A refined pool the handle held is dropped: run miqp_solver_pool_solve afterwards.
 * Returns the number of entries with moves > 0; 0 also for an empty pool (no device is touched); -1 invalid arguments / no instance; -2 the handle's
 * filter is not in 1 .. 15, or max_passes outside 1 .. 64; -3 no device / kernel image / HIP error, or a shape whose fix record does not fit the
 * LDS of a workgroup three times (3 x record bytes + 4 x sites > 160 KB: miqp_solver_last_error says so).  On every failure the pool is untouched.
 * miqp_solver_last_error is cleared at the start of the call.
 * miqp_solver_last_timing: out[0] the whole call, out[1] of which on the device, out[2] passes run (pass 0 not counted), out[3] neighbours solved,
 * out[4] their iterations, out[5] 1 when the last allowed pass still accepted a move (miqp_solver_last_error says so), else 0. */
int miqp_solver_pool_improve(miqp_solver_t* s, int max_passes, miqp_pool_improve_c* out, int cap);
/* the climb of miqp_solver_pool_improve over the pools of n handles in one device call: one device lock, one context of the handles'
 * common Layout, the instances compiled on host threads and their tables uploaded once.  One pass of the call is one pass of every handle that still
 * moves; the neighbours of all handles fill common launch groups of miqp_gpu_fixed_batch_chunk nodes, and the host waits for the device once per pass.
 * For every handle h the call answers what miqp_solver_pool_improve(solvers[h], max_passes, ., cap) answers for that handle alone, bit for bit:
 * counts[h] = min(miqp_solver_pool_count(solvers[h]), cap), out[h * cap + k], k < counts[h], the entry's before / after / moves / status, and
 * miqp_solver_pool_found_decisions, miqp_solver_pool_found and the dropped refined pool behind the call are those of the single call.  The handles
 * may differ in their filters.  A handle stops exactly when the single call's loop would stop for it (its move total of a pass is 0); a handle
 * whose entries have all stopped contributes no nodes to later passes.  The call ends when no handle moved or after max_passes passes.
 * DIFFERENCE from the single call: a handle that kept nothing (pool off, no solution) gets counts[h] = 0 and is left alone WHATEVER ITS FILTER -
 * the single call checks the filter first and answers -2 for such a handle without one; its miqp_solver_last_error and miqp_solver_last_timing
 * stay what they were.
 * Returns the number of entries with moves > 0, summed over the handles.  -1: NULL arrays, n <= 0, cap < 1, a NULL handle, a handle without an
 * instance, a handle named twice, or a kept pool whose record length differs from the common Layout's.  -2: max_passes outside 1 .. 64; handles that
 * do not share a shape or name different devices (as miqp_solver_solve_fixed_multi refuses them, with its text as the handles' last error); a handle
 * that kept entries and whose filter is outside 1 .. 15 (its miqp_solver_last_error names it).  -5: more than 65536 entries in all.  -3: no device /
 * kernel image / HIP error (an allocation that failed is one), or the LDS refusal of miqp_solver_pool_improve.  -1, -2 and -5 are found before any
 * device is touched; on EVERY failure out, counts and every pool of the call are untouched.  A call in which no handle kept anything returns 0
 * (counts all 0) without touching a device.
 * Device memory: entries x (record + miqp_gpu_pool_moves_max() x 16 bytes + a few words) beside the fixed buffers of the single call, whatever the
 * number of neighbours; cached per device, grown, not shrunk.
 * miqp_solver_last_timing of every handle that kept entries: out[0] the whole call, out[1] of which on the device (both of the CALL); out[2] passes in which the handle
 * had neighbours, out[3] the handle's neighbours solved, out[4] their iterations, out[5] 1 when an entry of the handle was still accepted in pass
 * max_passes (miqp_solver_last_error of that handle says so), else 0 - out[2 .. 5] are the single call's.  No reference counterpart. */
int miqp_solver_pool_improve_multi(miqp_solver_t* const* solvers, int n, int max_passes, miqp_pool_improve_c* out, int cap, int* counts);
/* the SLICES of a pass of the climb: the results of a pass are kept a slice at a time, a slice being a run of whole entries whose neighbours fit 8192
 * results (16 x miqp_gpu_pool_moves_max()).  move_counts[e], e < entries: the moves of entry e, clamped to 0 .. miqp_gpu_pool_moves_max() as the
 * kernels clamp them.  Slices are formed greedily in entry order: an entry opens a new slice when its moves do not fit what is left of the current
 * one.  slice_first[s] receives the first entry of slice s, slice_first[nslices] = entries.  Returns nslices (>= 1); -1 NULL pointers, entries <= 0
 * or cap < 0; -3 cap < nslices + 1 (nothing is written).  Pure host code - no handle, no device - and the function the host loop of
 * miqp_solver_pool_improve_multi itself calls. */
int miqp_gpu_pool_improve_plan(const int* move_counts, int entries, int* slice_first, int cap);

/* ---- the free places of a FILTERED pool filled with neighbouring manoeuvre classes (IloCplex::populate for a CPLEX user).  The pool
 * holds leaves the search evaluated, and the search prunes everything beyond its gap: a manoeuvre that is clearly worse than the optimum but valid -
 * the car passes the obstacle on the other side - usually never becomes a leaf.  Opt-in, behind the solve; nothing changes unless it is called. ----
 * A JUMP is a move (first, stride, count, value) of the families MIQP_POOL_BY_OBSTACLE and MIQP_POOL_BY_CAR_CAR that are in `families`; region and
 * environment sites have none.  A GROUP is the five point-sites of one (car, obstacle) or the four group-sites of one car pair: its bytes of one step
 * are contiguous.  A RUN of a group or of a single site is a maximal range [i0, i1] inside 1 .. N - 1 over which all its bytes are decided (>= 0) and
 * constant.  For every run and every alternative v - an obstacle edge 0 .. max_lines - 1 (never the soft alternative max_lines, which a run may hold
 * and be jumped from), a car/car alternative 0 .. 3 - all bytes of the group (stride 1, one contiguous range) or of the site (its own stride) over
 * the run take v.  A candidate is skipped when its bytes all hold v already, and when the signature under `families` is the same behind it: for
 * every site it writes, the nearest decided bytes before and behind the run are (a, v) or (v, a), a the site's byte in the run - the run then
 * only moves a change point, which is a move of the climb.  So every jump changes the signature.  Step 0 and undecided bytes are never written.
 * Order: obstacle groups by c * O + o, pairs, then the sites in the order of the signature's sites; inside each the runs by i0, then v ascending; at
 * most miqp_gpu_pool_moves_max() per record, the first ones in that order.
 * miqp_gpu_pool_jumps: the jumps of a record of D decision bytes, 4 ints each, into moves4[4 * cap].  Returns their number; -1 NULL pointers, a
 * non-positive dimension or max_lines < 0; -2 families outside 1 .. 15 or with neither the obstacle nor the car/car family; -3 cap too small.
 * Pure host code: no handle, no device. */
int miqp_gpu_pool_jumps(int cars, int steps, int obstacles, int max_lines, int families, const signed char* decisions, int* moves4, int cap);
/* sizeof(miqp_pool_explore_c) of the built library (binding check) */
int miqp_gpu_pool_explore_size(void);
/* one device-resident loop: pass 1 takes the jumps of every kept entry, pass p > 1 those of the entries pass p - 1 added.  All neighbours of a pass
 * are solved as nodes of the fixed-batch chain at the tight tolerance; then the feasible ones are visited in ascending (objective, neighbour number
 * - entry by entry, jump by jump), and one whose signature under the handle's filter is not in the pool yet - the entries admitted earlier in the
 * pass included - is appended while a place is free (the handle's capacity); the first neighbour of a new class is that class's best of the pass.
 * max_rel < 0: no cost cap; else a neighbour is admitted only when objective - obj0 <= max_rel * |obj0|, obj0 what miqp_solver_pool_found reports
 * for entry 0 (each operation rounded on its own).  Ends when the pool is full, a pass admitted nothing or had no jumps, or after max_passes passes.
 * No existing entry is changed or moved.  Results are a function of the records alone: the call is reproducible bit for bit.
 * Afterwards miqp_solver_pool_count, miqp_solver_pool_found (tight-tolerance objectives for the added entries) and
 * miqp_solver_pool_found_decisions include the added entries behind the old ones (no re-sort); out[k], k < return value, describes them in that
 * order.  A refined pool the handle held is dropped; miqp_solver_pool_improve and miqp_solver_pool_solve work on the larger pool as on any other.
 * Returns the number of entries added; 0 also for an empty or a full pool (no device is touched); -1 invalid arguments (NULL, cap < 0, max_rel NaN)
 * or no instance; -2 the handle's filter is not in 1 .. 15 or has neither the obstacle nor the car/car family, max_passes outside 1 .. 64, or cap
 * below the free places; -3 no device / kernel image / HIP error, or a shape whose fix record does not fit the LDS of a workgroup twice beside the
 * 8192 objectives of a pass (2 x record bytes + 64 KB > 160 KB: miqp_solver_last_error says so).  On every failure the pool is untouched.
 * miqp_solver_last_error is cleared at the start of the call.
 * miqp_solver_last_timing: out[0] the whole call, out[1] of which on the device, out[2] passes run, out[3] neighbours solved, out[4] their
 * iterations, out[5] 1 when the last allowed pass still admitted something (with places still free miqp_solver_last_error says so), else 0. */
int miqp_solver_pool_explore(miqp_solver_t* s, int max_passes, double max_rel, miqp_pool_explore_c* out, int cap);

/* ---- canonical labels on the device, and the explore that admits a manoeuvre only when its own labels are new.  Opt-in and new: the
 * calls above stay what they are. ----
 * The CANONICAL record of a solved node: per disjunction of the steps 1 .. N - 1 the first alternative that holds at the node's own solution - what
 * miqp_solver_fixed_batch_record hands out, read back as a fix record: byte for byte the D decision bytes of
 * miqp_solver_pool_signature(record, 31).  An undecided byte of the node's record counts as alternative 0 there, as in every record the library
 * hands out.  Step 0 is -1.  Two records with the same canonical record are one solution under two names.
 * miqp_solver_canonical_decisions is miqp_solver_solve_decisions - contract, return codes, miqp_solver_last_timing, out and best are that call's, bit
 * for bit: the same chain, the same chunks, the same state for miqp_solver_fixed_batch_record - with pool_label_kernel behind every chunk of the
 * chain: canon[k * D ..] receives the D canonical bytes of entry k, all -1 for an entry of status 1 or 2 and for a record with an undecided region
 * byte at a step >= 1 (its points have no region to be taken in).  A caller enumerating manoeuvres learns which of its records are one solution
 * without building n RawResults records.  Additional refusal: -3 with a text in miqp_solver_last_error (cleared at the start of the call) when two
 * fix records and a trajectory row exceed the LDS of a workgroup (160 KB).  No reference counterpart; the reference's collectRawResults is the host
 * analogue. */
int miqp_solver_canonical_decisions(miqp_solver_t* s, const signed char* decisions, int n, miqp_fixed_result_c* out, signed char* canon /* [n * D] */, int* best);
/* the same labels for trajectories the caller holds, on the host: trajectories[k] is the row of N * 8 * NrCars doubles of record k in the
 * library's column order per step (per car position, velocity, acceleration in x then y, then the inputs of all cars).  via 0: the restatement the
 * kernel compiles (every operation rounded on its own, in the host's order), via 1: the two host functions behind miqp_solver_fixed_batch_record -
 * the two agree byte for byte, which is what pins the kernel's arithmetic without a device.  canon[k * D ..] is all -1 for a record out of range or
 * with an undecided region byte at a step >= 1.  Returns the number of records labelled; -1 NULL arguments, no instance or n <= 0; -2 via not 0 or 1,
 * or a refused shape.  Pure host code: no device. */
int miqp_solver_canonical_labels(const miqp_solver_t* s, const signed char* decisions, const double* trajectories, int n, int via, signed char* canon /* [n * D] */);
/* miqp_solver_pool_explore with DISTINCT admission: arguments, return codes, refusals, timing slots, "the pool is untouched on every failure" and the
 * stored bytes - an added entry is its parent's bytes behind its jump - are that call's.  Differences:
 * pass 0, as in the climb: the kept entries' own records are solved at the tight tolerance and labelled; per place the call keeps, beside the
 * signature, the CANONICAL signature - the signature under the handle's filter of the entry's canonical record; of its as-found bytes for a kept
 * entry that is not feasible there.  Every pass labels its neighbours chunk by chunk, and a neighbour is admitted when its signature AND the
 * canonical signature of its own solution are not in the pool yet - the entries admitted earlier in the pass included; both are appended with it.
 * A neighbour that is an entry's solution under other labels is dropped and takes no place, so the places go to the manoeuvres behind it in the
 * visiting order.  Stopping rules, cap and order are unchanged.  Additional refusal (-3, with a text): 4 x record bytes + 64 KB, or 2 x record bytes
 * and a trajectory row, exceed 160 KB.
 * miqp_solver_last_timing: out[3] and out[4] include pass 0's nodes (one per kept entry) and their iterations; out[2] does not count pass 0. */
int miqp_solver_pool_explore_distinct(miqp_solver_t* s, int max_passes, double max_rel, miqp_pool_explore_c* out, int cap);

/* ---- settled labels on the device, and the explore that admits only manoeuvres the refinement will keep.  Opt-in and new: the calls
 * above stay what they are. ----
 * One labelling is not where miqp_solver_pool_solve ends: it labels and solves again, up to miqp_gpu_pool_settle_passes() times, until the labels
 * stay, and a record solved under the labels of its own solution can slide to another solution.  SETTLING a record is that iteration for one
 * record.  r0: its D decision bytes, completed to a fix record as miqp_solver_solve_decisions completes them.  For p = 1 .. passes: r(p - 1) is
 * solved through the fixed-batch chain at the tight tolerance; an answer of status != 0 ends it - the record has no settled labels; its solution is
 * labelled as miqp_solver_canonical_decisions labels it, to c(p); when c(p) is r(p - 1) byte for byte over the whole record, step 0 included, it is
 * SETTLED; else r(p) = c(p).  A record still moving behind the last solve keeps the labels that solve ran with (never seen on any instance).
 * miqp_solver_settle_decisions settles n records on the device, every round over the records that still move: contract, the refusals decided before
 * a device is touched and the return codes are those of miqp_solver_canonical_decisions.  out[k] is the LAST solve of record k; settled[k * D ..]
 * the D bytes of the labels that solve ran with - all -1 for an entry of status 1 or 2, and for a record with an undecided region byte at a step
 * >= 1, whose labels are all -1 after the first solve and stay so; solves[k] is 0 for a refused record, else the number of its solves, 1 ..
 * passes, and -passes for a record still moving at the end (miqp_solver_last_error then says so; it is cleared at the start of the call).  best as
 * in miqp_solver_solve_decisions, over the last results.  The call keeps NO state for miqp_solver_fixed_batch_record and drops what the handle held:
 * a caller who wants the trajectories sends `settled` through miqp_solver_solve_decisions and receives `out` again bit for bit.
 * miqp_solver_last_timing: out[0] the whole call, out[1] of which on the device, out[2] launch groups, out[3] solves in all, out[4] their
 * iterations, out[5] 1 when a record still moved at the end.  No reference counterpart. */
int miqp_solver_settle_decisions(miqp_solver_t* s, const signed char* decisions, int n, miqp_fixed_result_c* out, signed char* settled /* [n * D] */, int* solves /* [n] */, int* best);
/* the number of solves after which settling and the refinement of miqp_solver_pool_solve stop (6).  Pure host code: no device */
int miqp_gpu_pool_settle_passes(void);
/* miqp_solver_pool_explore with SETTLED admission: arguments, return codes, refusals (those of the distinct call included), stopping rules, cap,
 * visiting order, "the pool is untouched on every failure" and what is stored - an added entry is its parent's bytes behind its jump, objective and
 * iterations are its first solve's - are that call's.  Differences:
 * pass 0 settles the kept entries' own records; per place the call keeps, beside the signature, the SETTLED signature - the signature under the
 * handle's filter of the entry's settled labels; a kept entry without settled labels has none and matches nothing.  In every pass the neighbours
 * that are feasible, within the cost cap and of a signature that is new against the pool at the start of the pass are settled - those whose first
 * labels are their own record with that one solve - and a neighbour is admitted while a place is free when its signature is not in the pool, it has
 * a settled signature and that one is not among the settled signatures of the pool; the entries admitted earlier in the pass are included in both.
 * The canonical signature of the distinct call takes no part.  miqp_solver_pool_solve behind the call merges away nothing the call added.
 * out[k].reserved is the number of solves the entry's settling took (1 .. miqp_gpu_pool_settle_passes()); in the other two calls it stays 0.
 * miqp_solver_last_timing: out[3] and out[4] count every solve of the call - pass 0, the neighbours, the settle rounds - and their iterations;
 * out[2] does not count pass 0. */
int miqp_solver_pool_explore_settled(miqp_solver_t* s, int max_passes, double max_rel, miqp_pool_explore_c* out, int cap);

/* ---- the free places of MANY handles filled in one device call.  Opt-in and new: the three calls above stay what they are. ----
 * mode: the admission, one of the three the single calls have */
#define MIQP_POOL_EXPLORE_PLAIN 0     /* miqp_solver_pool_explore */
#define MIQP_POOL_EXPLORE_DISTINCT 1  /* miqp_solver_pool_explore_distinct */
#define MIQP_POOL_EXPLORE_SETTLED 2   /* miqp_solver_pool_explore_settled */
/* All handles start pass 1 together; one pass of the call is one pass of every handle that is still adding, and the neighbours of all of them
 * fill common launch groups.  max_passes and max_rel are common; obj0, the capacity, the filter and the edge count are each handle's own.
 * out[h * cap + k] is the k-th entry added to handle h, counts[h] their number.  PER HANDLE the call answers bit for bit what the single call of
 * that mode answers for the handle alone: the added records (parent, pass, jump, iterations, objective, reserved), the pool afterwards (old
 * entries untouched and in place), the dropped refined pool, miqp_solver_last_timing out[2 .. 5] (passes in which the handle had neighbours, its
 * solves, their iterations, "still adding") and miqp_solver_last_error, the "last of N passes still added" text included.  out[0] and out[1] of
 * miqp_solver_last_timing are the CALL's.
 * A handle whose pool is empty or full takes no part WHATEVER ITS FILTER: counts[h] = 0, its pool and last timing stay, its last error is
 * cleared.  This is the one difference to the single call, which checks the filter first and refuses such a handle with -2.
 * Returns the number of entries added in all.  -1: NULL arrays, n <= 0, cap < 0, max_rel a NaN, mode outside 0 .. 2, a NULL handle, a handle
 * without an instance, a handle named twice, or a kept pool whose record length is not the common Layout's.  -2: max_passes outside 1 .. 64;
 * handles that do not share a shape or name different devices (as miqp_solver_solve_fixed_multi refuses them, with its text as the handles' last
 * error); a handle that has entries and free places under a filter outside 1 .. 15 or with neither the obstacle nor the car/car family (its
 * miqp_solver_last_error names it); cap below the largest number of free places among the handles that take part.  -5: more than 4096 handles
 * (65536 / 16 places).  -3: no device / kernel image / HIP error, or the LDS refusals of the single call of that mode (the handles that take part
 * then carry its text).  All but -3 are found before a device is touched; on EVERY failure out, counts and every pool are untouched.  A call in
 * which no handle takes part returns 0 (counts all 0) without touching a device.  miqp_solver_last_error of every handle is cleared once nothing
 * of the above but -3 refuses the call.
 * Device memory: 16 places per handle x (3 records + miqp_gpu_pool_moves_max() x 16 bytes + a few words), and the records of pass 0 of the
 * settled mode (the kept entries of all handles), beside the fixed slice buffers of 8192 neighbours; it does not grow with the neighbours of a pass.
 * No reference counterpart. */
int miqp_solver_pool_explore_multi(miqp_solver_t* const* solvers, int n, int mode, int max_passes, double max_rel, miqp_pool_explore_c* out, int cap, int* counts);
/* the SLICES of a pass of that call: results, labels and settle words are kept a slice at a time, a slice being a run of WHOLE handles whose
 * neighbours of the pass fit 8192.  handle_totals[h], h < n: the neighbours of handle h in the pass, 0 .. 8192.  Slices are formed greedily in handle
 * order: a handle opens a new slice when its neighbours do not fit what is left of the current one; a handle without neighbours rides along.
 * slice_first[s] receives the first handle of slice s, slice_first[nslices] = n.  Returns nslices (>= 1); -1 NULL pointers, n <= 0 or cap < 0; -2 a
 * total outside 0 .. 8192; -3 cap < nslices + 1 (nothing is written).  Pure host code - no handle, no device - and the function the host loop of
 * miqp_solver_pool_explore_multi itself calls. */
int miqp_gpu_pool_explore_plan(const int* handle_totals, int n, int* slice_first, int cap);
/* diagnostic: the passes and the slices the calling thread's last successful miqp_solver_pool_explore_multi ran on the device (either may be NULL) */
void miqp_gpu_pool_explore_multi_last(int* passes, int* slices);

/* ---- the kept manoeuvres of one planning cycle CARRIED into the pool of the next.  Opt-in and new: nothing changes unless it is
 * called.  A receding-horizon caller solves a new instance every cycle and miqp_solver_set_params empties the pool; the carry is the pool's
 * counterpart of miqp_calculate_warmstart (a CPLEX user would re-add the members of the old pool as MIP starts of the new model). ----
 *
 * The SHIFT of a record of D decision bytes (the layout of miqp_solver_pool_found_decisions) by `shift` steps: for every site and every step
 * i = 1 .. steps - 1 the byte of `out` is the byte of `decisions` at step min(i + shift, steps - 1) - the last decided state is held -, re-expressed
 * for the destination instance: a region byte q * 4 + h becomes region_map[c * p_src + q] * 4 + h (c the car; h, the half-plane or slow alternative,
 * is kept); an environment byte e becomes env_map[e], -1 (undecided) where the map says so; obstacle and car/car bytes are kept - obstacle o of the
 * destination is obstacle o of the source `shift` steps later: the caller's contract.  Negative bytes stay -1, step 0 of every site is -1, bytes of
 * `out` behind D are -1.  A NULL map is the identity.  A region byte whose target is -1 makes the whole record UNMAPPABLE: the return value is -4 and
 * `out` is written all the same, with -1 at those bytes.  Returns D; -1 NULL pointers or non-positive dimensions, -2 shift outside 1 .. steps - 2,
 * -3 len < D.  Pure host code - no handle, no device - and the very function pool_shift_kernel compiles. */
int miqp_gpu_pool_shift(int cars, int steps, int obstacles, int shift, const int* region_map, int p_src, const int* env_map, int e_src, const signed char* decisions,
                        signed char* out, int len);
/* both maps of a carry from the instances loaded in src and dst.  region_map[c * p_src + q]: the destination's possible-region index of the region
 * NUMBER that is the source's q-th possible region of car c, or -1 (p_src: the most possible regions a car of the source has); env_map[e], e < the
 * source's environment pieces: the first piece of the destination whose rounded edge tuples equal those of the source's piece e, or -1.  Returns
 * p_src.  -1: NULL, src == dst, a handle without an instance.  -2, with the reason in miqp_solver_last_error(dst): the instances differ in cars,
 * steps, obstacles, max_lines_obstacles or the obstacles' soft flags, or do not carry the same region tables.  -3: cap_r < cars * p_src or cap_e
 * below the source's pieces.  Needs no device; miqp_solver_last_error(dst) is cleared at the start. */
int miqp_solver_pool_carry_maps(const miqp_solver_t* src, const miqp_solver_t* dst, int* region_map, int cap_r, int* env_map, int cap_e);
/* The carry.  The SOURCE entries are the first min(miqp_solver_pool_count(src), 16) entries of src's pool as found (improved and explored entries
 * included); src is only read.  Each is shifted (above, with the maps of the two instances), the mappable ones are settled on dst's instance in the
 * rounds of miqp_solver_settle_decisions - together with dst's own kept entries, whose settled signatures the admission needs -, and the feasible ones
 * are visited in ascending (objective of the first solve, source entry number).  A record is appended behind dst's pool when it is within the cost cap
 * (else status 5), its signature under dst's filter is not in the pool (3), it has settled labels whose signature is not among the settled signatures
 * of the pool (4) and a place is free (6), in that order of tests; entries admitted earlier in the call count in both signature tests.  Stored for an
 * admitted entry: the shifted bytes, objective and iterations of its FIRST solve - the settled explore's convention, so miqp_solver_pool_solve behind
 * the call merges away nothing it added.  No existing entry is changed or moved; a refined pool dst held is dropped.
 * Cost cap: max_rel < 0 none, else objective - obj0 <= max_rel * |obj0|, obj0 = dst's entry 0 as found, every operation rounded on its own.
 * dst may hold an EMPTY pool (capacity and filter set, instance loaded, no solve yet or a solve that found nothing): the first record admitted is
 * admitted whatever max_rel is, becomes entry 0, and its objective is obj0 from then on; miqp_solver_pool_count(dst) then counts the carried entries
 * until the next solve or the next parameters.
 * out[k], k < source entries: one record per SOURCE entry (miqp_pool_carry_c).  Returns the number admitted; 0 without touching a device when src
 * keeps nothing or dst is full.  -1: NULL, cap < 0, max_rel a NaN, src == dst, a handle without an instance.  -2: shift outside 1 .. steps - 2; dst's
 * capacity 0; dst's filter outside 1 .. 15 (no jump family is needed here); what miqp_solver_pool_carry_maps refuses with -2; cap below the source
 * entries.  -3: no device / kernel image / HIP error, or a shape whose fix record does not fit the LDS of the kernels (miqp_solver_last_error(dst)
 * says which).  All but -3 are decided before a device is touched; on every failure out and both pools are untouched.
 * miqp_solver_last_error(dst) is cleared at the start.  miqp_solver_last_timing(dst): out[0] the call, out[1] of which on the device, out[2] launch
 * groups of the settle rounds, out[3] solves (dst's own entries included), out[4] their iterations, out[5] 1 when a carried record still moved after
 * the last settle pass.  The call is a function of the two pools and the two instances alone: reproducible bit for bit.
 * Out of scope: obstacle re-numbering; replacing a kept entry by a better carried one of its class (the climb's job).  The carried records of an
 * EMPTY pool as MIP starts of the solve behind the carry: miqp_solver_set_pool_starts below.  Many (src, dst) pairs in one call:
 * miqp_solver_pool_carry_multi below.  No reference counterpart. */
int miqp_solver_pool_carry(miqp_solver_t* dst, const miqp_solver_t* src, int shift, double max_rel, miqp_pool_carry_c* out, int cap);
/* ---- the carry of many (src, dst) pairs in ONE device call: a scenario-parallel caller drains a queue of handles every
 * cycle.  The carry is almost only settle rounds, and a round costs the same for 30 records as for a thousand: the records of all pairs fill
 * common launch groups, behind one lock, one context and one upload. ----
 * Pair p carries the kept entries of srcs[p] into the free places of dsts[p].  shift and max_rel are common; both maps, the capacity, the filter,
 * obj0 and the entry counts are each pair's own.  out[p * cap + k] is the record of source entry k of pair p, counts[p] the number admitted to
 * dsts[p]; the return value is their sum.  PER PAIR the call answers bit for bit what miqp_solver_pool_carry(dsts[p], srcs[p], shift, max_rel, ..)
 * answers for the pair alone: the count, every out record, the destination's pool afterwards (old entries untouched and in place), the dropped
 * refined pool, miqp_solver_last_timing(dst) out[2 .. 5] (out[2]: the rounds in which the pair had a live record - its launch groups, a pair having
 * at most 32 records) and miqp_solver_last_error(dst), the "still moved" text included.  out[0] and out[1] of the last timing are the CALL's.
 * Sources are only read; one source may feed several destinations (one pool of last cycle branching into several scenarios of the next).
 * A pair with nothing to carry or a full destination takes no part: counts[p] = 0, its rows of out are not written, its pool and last timing
 * stay, its last error is cleared - as the single call leaves it.  A call in which no pair takes part returns 0 without touching a device.
 * -1: NULL arrays, n <= 0, cap < 0, max_rel a NaN; a NULL handle or one without an instance; srcs[p] == dsts[p]; a destination named twice; a handle
 * that is the destination of one pair and the source of another (the answer would depend on the order); a kept pool whose record length is not the
 * common Layout's.  -5: more than 2048 pairs (65536 / 32 records: a pair has at most 16 own and 16 carried ones) - decided on n alone, before
 * a handle is read.  -2: shift outside 1 .. steps - 2; what the single call refuses of a pair with -2 - capacity 0, a filter outside 1 .. 15, what
 * miqp_solver_pool_carry_maps refuses -: the pairs are checked in order, the first refusal decides and its reason is THAT destination's last error
 * (the last errors of the other destinations stay what they were); destinations that do not share a shape or a device (as
 * miqp_solver_solve_fixed_multi refuses them, with its text as every destination's last error); cap below the largest number of source entries
 * among the pairs.  -3: no device / kernel image / HIP error, or the LDS refusals of the single call (the destinations that take part then carry
 * its text).  All but -3 are decided before a device is touched; on EVERY failure out, counts and every pool are untouched.
 * miqp_solver_last_error of every destination is cleared once nothing of the above but -3 refuses the call.
 * Device memory: 16 places per pair x (5 records + a few words) and 32 records per pair of the settle rounds.  No reference counterpart. */
int miqp_solver_pool_carry_multi(miqp_solver_t* const* dsts, const miqp_solver_t* const* srcs, int n, int shift, double max_rel, miqp_pool_carry_c* out, int cap, int* counts);
/* diagnostic: the settle rounds and the launch groups the calling thread's last successful miqp_solver_pool_carry_multi ran on the device (either may
 * be NULL) */
void miqp_gpu_pool_carry_multi_last(int* rounds, int* groups);
/* sizeof(miqp_pool_carry_c) of the built library (binding check) */
int miqp_gpu_pool_carry_size(void);
/* diagnostic: the seconds the calling thread's last successful miqp_solver_pool_carry spent in pool_shift_kernel and in pool_carry_admit_kernel, from
 * the call's own device events (either may be NULL) */
void miqp_gpu_pool_carry_last(double* shift_s, double* admit_s);
/* ---- starts from the carried pool: the solve behind a carry into an EMPTY pool starts its search from the carried manoeuvres - with
 * this the carry is the whole counterpart of a CPLEX user re-adding the old pool's members as MIP starts of the new model. ----
 * miqp_solver_set_pool_starts: the most start roots a solve takes from the handle's pool; 0 is off and the default, 1 .. miqp_gpu_pool_max() are
 * accepted.  Returns 0; -1 for a NULL handle or a value out of range (the previous setting stays).  The setting belongs to the handle and survives
 * miqp_solver_set_params, as the capacity and the filter do.
 * A handle TAKES STARTS in a solve when max_starts > 0, its pool is one that miqp_solver_pool_carry (or _carry_multi) put there and that no solve
 * stands behind (so miqp_solver_set_params has not been called since: it empties the pool), the pool holds an entry whose record length is the
 * call's, and the first step of the instance is feasible.  Its start roots are the first min(max_starts, entries) entries in pool order, each
 * completed as miqp_solver_solve_decisions completes decision bytes, with depth word 0 and no repair root, appended behind the root and the roots of
 * the two slots of miqp_solver_set_warmstart.  They are nodes of round 1: a feasible start is a candidate, the best one is the first incumbent, and
 * the capture merges every feasible start into the pool of the solve with the leaves of the search - the fallback that was carried in survives the
 * solve unless `capacity` better classes push it out.  Every entry point that solves takes them - miqp_solver_solve, _solve_batch, _solve_stream,
 * _solve_batch_multi -, handle by handle; a tree-split call (miqp_solver_solve_split, _solve_split_rccl) IGNORES the setting.
 * The root records per instance are the call's: 5 in a call in which no handle takes starts - every buffer and every kernel argument then has the
 * value it has without this setting, and so has every result -, else 5 plus the largest max_starts SETTING among the handles of the call that take
 * starts (the setting, not the number taken: a receding horizon carries another number of records every cycle).  A device context is rebuilt when
 * that number changes, as for any other change of a call's shape (about a second for a single solve's context): between a call with starts and
 * one without, and when the setting changes - not because a loop with one setting carries another number of records every cycle.
 * No kernel is added or changed.  A start decides every disjunction, so
 * its relaxation is larger than the on-chip node kernels hold: its record begins with the size mark that sends it to the memory-backed kernel in
 * round 1 - unmarked it would be handed from kernel to kernel for two rounds and then meet the cutoff of the incumbent found meanwhile.
 * With fewer nodes per instance and round than root records (at most 21; a batch of thousands of instances in flight runs 16 wide) the roots
 * behind the first round meet the incumbent of round 1, and a start that is not better than it is dropped like any node: it is then no candidate. */
int miqp_solver_set_pool_starts(miqp_solver_t* s, int max_starts);
/* the handle's setting (0: off); -1 for a NULL handle */
int miqp_solver_get_pool_starts(const miqp_solver_t* s);
/* the number T of start roots the handle's last solve took from its pool (0: none); for k < min(T, cap) place[k] is the entry of the pool AFTER that
 * solve that stands for start k - under the handle's filter the entry of the start's plain signature, without a filter the entry of the same
 * decision bytes - or -1 when the pool holds no such entry.  Computed on the host behind the pool's read-back: needs no device.  New parameters
 * reset it to 0.  -1: NULL handle (place may be NULL with cap 0) */
int miqp_solver_pool_starts_last(const miqp_solver_t* s, int* place, int cap);

/* 1 when instances of this shape (NrCars, N) have the dual active-set launches - one or two cars, a horizon of up to 20 steps - else 0 (their node
 * relaxations are interior point solves).  Pure host code: no device is needed or touched.  A call switches the launches off with MIQP_AS=0 */
int miqp_gpu_has_active_set(int num_cars, int num_steps);

/* diagnostic: the node launches a solve of the handle's instance would issue for a round of bc nodes (overlap 1, par = the round's parity, or -1
 * for a round without the parity counter sets) or for the serial chain of the polish and of miqp_solver_solve_fixed (overlap 0, par -1), on a device of
 * `cus` compute units with `free_gb` GB free and all four streams.  cls_n3: the lengths of the round's three class lists, {-1, -1, -1}: not known.
 * flags: 1 = the call uses the active-set launches (MIQP_AS), 2 = a context without the concurrent round (the tuning switch MIQP_CONCURRENT_BIG=0, which
 * the shipped library does not read): the serial chain with its probe overlap.  Writes one row of 13 ints per launch, in the order of issue: kernel (0
 * memory-backed, 1 / 2 larger active-set / larger on-chip interior point, 3 / 4 standard active-set / standard on-chip interior point), stream (0 the solver's, 2 .. 4 the ones beside
 * it), workgroups, dynamic LDS bytes, ovf_mode, cls_take, as_split, skip_probes, bounce, work counter (> 0: word of the parity set, 0 the batch's, -1 the
 * second stream's), hand-over list read (0 the standard launch's, 1 the larger variant's), per-block buffers (0 the batch's, 1 the second stream's,
 * 2 those with the third gain buffer), memsets in front (1 work counter, 2 hand-over count, 4 the larger variant's hand-over count).  Returns the number
 * of launches; < 0: no instance (-1), shape refused (-2), cap too small (-3).  Pure host code: no device is needed or touched */
int miqp_solver_launch_plan(const miqp_solver_t* s, int bc, int overlap, int par, const int* cls_n3, int cus, double free_gb, int flags, int* out, int cap);

/* host set-up of the last solve / batch / stream call this handle took part in: out[0] = seconds from the entry of the call to
 * the first round, out[1] = of which building the device context (pools, lists: reused by a call of the same shape with no more
 * instances than its per-instance arrays hold), out[2] = 1 when the context was built or rebuilt by that call, else 0 */
int miqp_solver_last_setup(const miqp_solver_t* s, double* out3);

/* out[0] = when the last batch / stream call admitted this instance to a slot, in seconds after the call's first branch-and-bound round started
 * (0 for a single solve and for the instances in flight from the start).  Together with SolutionProperties.time (admission to proof) it places
 * every instance of a drained queue on the call's time axis - bench.py derives the drain rate of the queue while it still had a backlog from it. */
int miqp_solver_last_admission(const miqp_solver_t* s, double* out1);

/* why the last solve of this handle did not run or did not finish, as text ("" when there is nothing to say; the pointer is valid
 * until the next call on the handle).  The reference logs such conditions with LOG(ERROR) inside callCplex
 * (src/cplex_wrapper.cpp:97-109, 162-180); here the status code says WHAT (the four OptimizationStatus values), this says WHY:
 * malformed parameters, the queue abandoned before the instance was admitted, an instance retired because it made no progress
 * for 64 branch-and-bound rounds.  Such an instance reports FAILED_SEG_FAULT without an incumbent (never FAILED_TIMEOUT) and SUCCESS with
 * one; its props.status stays the CPLEX code of an unfinished solve (107 with, 108 without an incumbent - CPLEX has no code for "stalled"):
 * what tells it from an instance that really used up max_solution_time is this text and, without an incumbent, the status code. */
const char* miqp_solver_last_error(const miqp_solver_t* s);

/* ---- planner core: the host logic directly above the solve ---- */

/* ParameterPreparer::CalculateFractionParameters             common/parameter/parameter_preparer.cpp:37-52; out[R*4] */
int miqp_fraction_parameters(int nr_regions, float max_velocity_fitting, double* out);
/* FittingPolynomialParameters::GetPOLY_*()                    common/parameter/fitting_polynomial_parameters.hpp:28-168
 * out[6][R*3], row-major [region][3], order SINT_UB, SINT_LB, COSS_UB, COSS_LB, KAPPA_AX_MAX, KAPPA_AX_MIN; returns -2 for a
 * (nr_regions, max, min velocity) combination outside the seven the reference ships (it throws std::invalid_argument) */
int miqp_fitting_polynomial_parameters(int nr_regions, float max_velocity_fitting, float min_velocity_fitting, double* out);
/* ParameterPreparer::CalculateMeanAngleVector                 parameter_preparer.cpp:96-113; out[R] */
int miqp_mean_angles(const double* fraction_parameters, int nr_regions, double* out);
/* CalculateAccLimitsPerCar / CalculateJerkLimitsPerCar (RotateLimitVectors)   parameter_preparer.cpp:54-94, 115-143
 * acc: (acc_min, acc_max, -acc_lat, +acc_lat); jerk: (-jerk_max, jerk_max, -jerk_lat, +jerk_lat); four arrays of R */
int miqp_limits_per_region(const double* fraction_parameters, int nr_regions, float long_min, float long_max, float lat_min, float lat_max,
                           double* min_x, double* max_x, double* min_y, double* max_y);
/* CalculateRegionIdx                                          common/parameter/regions.cpp:16-33; returns the count */
int miqp_calculate_region_idx(const double* fraction_parameters, int nr_regions, float vx, float vy, int* out);
/* ReserveNeighborRegions on one row of nr_regions flags       regions.cpp:75-112 */
int miqp_reserve_neighbor_regions(int* row, int nr_regions, int expansions);
/* CalculatePossibleRegions                                    regions.cpp:114-127; flags[R] */
int miqp_calculate_possible_regions(const double* fraction_parameters, int nr_regions, const double* theta_ref, int n, int* flags);
/* MiqpPlanner::CalculateWarmstart: last solution shifted by one step (with its quirks)   src/miqp_planner.cpp:787-1051 */
/* ReferenceTrajectoryGenerator::GenerateTrajectory on a polyline (common/reference/reference_trajectory_generator.cpp:51-148;
   bark's spline smoothing of the centre line replaced by the polyline itself: identical on straight reference lines).
   ref_xy: n_ref points (x, y); state5 = (time, x, y, theta, v); out[num_points][5] in the same order. */
int miqp_reference_trajectory(const double* ref_xy, int n_ref, const double* state5, double dt, int num_points, double line_interp_inc, double vel_desired,
                              double delta_s_desired, double acc_lat_max, int vel_curve_dep, double* out);
/* MiqpPlanner::UpdateCar for one car (src/miqp_planner.cpp:284-390): reference rows, possible regions, weights.
   settings12 = nr_regions, nr_steps, nr_neighbouring_possible_regions, additionalStepsForReferenceLongerHorizon, ts,
   refLineInterpInc, straight lateral acceleration limit, lambda, positionWeight, velocityWeight, acclerationWeight, jerkWeight;
   initial_state6 = (x, vx, ax, y, vy, ay); ref4N = x_ref, y_ref, vx_ref, vy_ref rows; weights8 = POS_X, VEL_X, ACC_X, POS_Y,
   VEL_Y, ACC_Y, JERK_X, JERK_Y.  0 ok, 1 region expansion failed (the reference logs and goes on), < 0 invalid arguments. */
int miqp_update_car(const double* settings12, const double* fraction_parameters, const double* initial_state6, const double* ref_xy, int n_ref, double desired_velocity,
                    double delta_s_desired, double timestep, int track_reference_positions, int is_ego, int num_cars, double* ref4N, int* possible_region, double* weights8);
int miqp_calculate_warmstart(const miqp_raw_results_c* last, miqp_raw_results_c* out, double ts, double minimum_region_change_speed);
/* MiqpPlanner::Plan, region-combination retry loop            src/miqp_planner.cpp:634-645, 692-766
 * initial_region[C] / possible_region[C*R] are the caller's arrays (p is re-pointed to them) and are updated in place as
 * the reference updates its ModelParameters; returns 1 when a combination solved (Plan() == true),
 * *status_out = last OptimizationStatus */
int miqp_plan(miqp_solver_t* s, miqp_model_params_c* p, int* initial_region, int* possible_region, const miqp_raw_results_c* warmstart,
              int warmstart_type, double timestamp, int* status_out);

/* ---- environment and obstacles of MiqpPlanner, on convex counter-clockwise pieces given as vertex arrays (the convexification of a
 * bark map polygon, common/map/convexified_map.cpp, is out of scope).  pieces_xy: x0, y0, x1, y1, ... of all pieces, piece_off[n + 1]
 * vertex offsets ---- */
/* the initial-pose check of MiqpPlanner::Plan (src/miqp_planner.cpp:654-685): -1 when the rear and the front axle point of every car
 * lie within a piece of p's environment, else 2 * car + (1: front point, 0: rear point); -2 on invalid arguments.  miqp_plan runs it. */
int miqp_initial_pose_check(const miqp_model_params_c* p);
/* MiqpPlanner::ResetEnvironment (src/miqp_planner.cpp:490-537): selected[e] = 1 for the pieces that a reference trajectory (x, y
 * polylines, traj_off[n_traj + 1] point offsets) touches; returns their number */
int miqp_select_environment(const double* pieces_xy, const int* piece_off, int n_pieces, const double* traj_xy, const int* traj_off, int n_traj, int* selected);
/* MiqpPlanner::ObstacleIntersectsEnvironment (src/miqp_planner.cpp:1248-1306, without the region of interest): 1 when the obstacle
 * (n_steps x 4 vertices) intersects a piece - checked at step 0 only when it is static; an empty environment admits every obstacle */
int miqp_obstacle_intersects_environment(const double* pieces_xy, const int* piece_off, int n_pieces, const double* obstacle_xy, int n_steps, int is_static);
/* MiqpPlanner::GetBarkTrajectory (src/miqp_planner.cpp:1132-1170) on plain arrays: out_rows5 receives up to N rows (time, x, y, theta, v)
 * - bark's StateDefinition order - of car `car`; the trajectory is cut off at the first step whose |vx| and |vy| are both <= min_speed
 * (IsVxVyValid :1184-1187; the planner uses 0.7, :53-54).  Returns the number of rows, -1 on invalid arguments */
int miqp_bark_trajectory(const miqp_raw_results_c* results, int car, double start_time, double ts, double min_speed, double* out_rows5);
/* MiqpPlanner::UpdateObstaclesROI (src/miqp_planner.cpp:1308-1335): the region of interest around the ego car as 4 vertices (x, y pairs:
 * front upper, front lower, rear lower, rear upper), computed exactly as the reference writes it */
int miqp_obstacles_roi(double x, double y, double theta, double behind_distance, double front_distance, double side_distance, double* roi_xy);
/* MiqpPlanner::ObstacleIntersectsEnvironment with its region-of-interest filter (src/miqp_planner.cpp:1278-1288; settings
 * obstacle_roi_filter, src/miqp_planner_settings.h:74-77): as above, but a step at which the obstacle does not intersect roi_xy (4 vertices;
 * NULL = no filter) is skipped - a static obstacle is then irrelevant (0), a moving one is checked at its next step */
int miqp_obstacle_intersects_environment_roi(const double* pieces_xy, const int* piece_off, int n_pieces, const double* obstacle_xy, int n_steps, int is_static, const double* roi_xy);
/* MiqpPlanner::EnvironmentWarmstart (src/miqp_planner.cpp:1053-1115): the five environment arrays of `last` ([C][n_old][N]) re-indexed
 * into `out` ([C][n_new][N]) by piece id; new pieces and the last step start as 1 */
int miqp_environment_warmstart(const miqp_raw_results_c* last, miqp_raw_results_c* out, const int* ids_old, int n_old, const int* ids_new, int n_new);

/* Certificate of a delivered record against the raw big-M model of the instance loaded in s (no reference counterpart; what
 * IloCplex::getQuality(MaxPrimalInfeas / MaxIntInfeas) answers for a CPLEX user).  Every row of the cplexmodel .mod files is generated and
 * evaluated on the device, from the host instance and the record - not from the solver's incumbent - so the answer is independent of the
 * branch and bound.  `candidate` NULL: the last solution of the handle (its record is built, or taken when
 * miqp_solver_materialize_results ran, and kept in the handle).  The car/car slacks are slackvars_real when the record carries
 * them, else the truncated ints.  It proves primal feasibility and the objective of that record, not optimality or a bound.
 * Returns 0 (a handle without a solution gives status 1), -1 invalid arguments / no instance, -2 a NULL array in `candidate`,
 * -3 `candidate` has other sizes than the instance (as miqp_solver_set_warmstart), -4 no HIP device or no kernel image
 * (miqp_solver_last_error says which): there is no host evaluation.  Holds the device lock of opts.device like a solve;
 * uses buffers of its own (two staging and two device buffers of at most 48 MB each, cached per device) and leaves the
 * solver's device context untouched.  Deterministic: the same record gives the same bytes. */
int miqp_solver_certify(miqp_solver_t* s, const miqp_raw_results_c* candidate, miqp_certificate_c* out);
/* ... of the last solution of every handle (out[n]); handles may differ in shape.  Records are packed on at most 16 host threads
 * and uploaded in chunks beside the kernel of the previous chunk; runs on the device of solvers[0] */
int miqp_solver_certify_batch(miqp_solver_t* const* solvers, int n, miqp_certificate_c* out);
/* sizeof(miqp_certificate_c) of the built library (binding check) */
int miqp_gpu_certificate_size(void);
/* the last certify call of the process: out[0] = seconds of host packing, out[1] = of uploads, out[2] = of kernels (both from
 * device events, they overlap each other and the packing), out[3] = the whole call */
int miqp_gpu_certify_last_timing(double* out4);

const char* miqp_gpu_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MIQP_GPU_H */

// miqp_gpu.hip - host side of libmiqp_gpu.so: C ABI (include/miqp_gpu.h), device buffer management and the
// round loop  select -> interior point -> evaluate/branch  of the on-device branch and bound.
//
// There is no CPU solve path in this library: without a HIP device the solve entry points return
// MIQP_STATUS_FAILED_SEG_FAULT (the reference's code for "the solver could not run", cplex_wrapper.cpp:97-109).
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <atomic>
#include <mutex>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#include "../../include/miqp_gpu.h"
#include "kernels.hip"
#include "wire_formats.hpp"
#include "planner_core.hpp"
#include "lp_export.hpp"

// A round of two cars runs FOUR launches side by side on four streams (launch_ipm_batch), and the process has its null stream: with the HIP runtime's
// default of four hardware queues two of those streams share one, and the launch behind on the shared queue - the memory-backed kernel - started only
// when the larger active-set launch in front of it had ended, alone, for 1.7 ms of a 12 ms round (rocprofv3 trace of the driver's command,
// profiles/r06_*round_gaps*).  The runtime reads GPU_MAX_HW_QUEUES once, at its first call: the library asks for eight when it is loaded, unless the
// variable is set already; a process that initialised HIP before loading the library keeps its four queues (and that serial tail) - INTEGRATION.md 5.
__attribute__((constructor)) static void miqp_gpu_hw_queues() { setenv("GPU_MAX_HW_QUEUES", "8", 0); }

using namespace miqp;

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "[miqp_gpu] %s failed: %s (%s:%d)\n", #x, hipGetErrorString(e_), __FILE__, __LINE__); return false; } } while (0)

// A device array that grows and never shrinks: what the per-device caches of the calls (certify.hip, fixed_chain.hip, the pool files) are made of.
// need(n, floor): room for n elements - the capacity becomes floor doubled until it holds n, or exactly n without a floor; `tail` elements more are
// allocated behind the capacity (the end word of a scan).  The old contents go.  A failure leaves the array empty, and the next call takes it up
// again.  PINNED: the same in pinned host memory
template <class T, bool PINNED = false> struct DevArr {
  T* p = nullptr; size_t cap = 0;
  operator T*() const { return p; }
  bool need(size_t n, size_t floor = 0, size_t tail = 0) {
    if (n <= cap) return true;
    if (p) (void)(PINNED ? hipHostFree(p) : hipFree(p));
    p = nullptr; cap = 0;
    size_t want = floor ? floor : n;
    while (want < n) want <<= 1;
    if (PINNED) HIP_OK(hipHostMalloc((void**)&p, (want + tail) * sizeof(T), hipHostMallocDefault));
    else HIP_OK(hipMalloc((void**)&p, (want + tail) * sizeof(T)));
    cap = want;
    return true;
  }
};
// the cache of type D of a device (CertDev, FixedDev, Pool..Dev); the one table that holds them stands behind the includes of their files
template <class D> D& call_dev(int device);

// caller-independent RawResults record (deep copy target; MIP starts are kept in this form until the solve compiles them)
struct OwnedResults {
  miqp_raw_results_c r{}; std::vector<std::vector<double>> d; std::vector<std::vector<int>> i;
  OwnedResults(int C, int N, int R, int E, int O, int L) {
    const int K = C - 1;
    r.N = N; r.NrEnvironments = E; r.NrRegions = R; r.NrObstacles = O; r.MaxLinesObstacles = L; r.NrCarToCarCollisions = K; r.NrCars = C;
    auto D = [&](size_t n) { d.emplace_back(n ? n : 1, 9999999.0); return d.back().data(); };
    auto J = [&](size_t n) { i.emplace_back(n ? n : 1, 9999999); return i.back().data(); };
    d.reserve(16); i.reserve(24);
    const size_t cn = (size_t)C * N;
    r.u_x = D(cn); r.u_y = D(cn); r.pos_x = D(cn); r.vel_x = D(cn); r.acc_x = D(cn); r.pos_y = D(cn); r.vel_y = D(cn); r.acc_y = D(cn);
    r.pos_x_front_UB = D(cn); r.pos_x_front_LB = D(cn); r.pos_y_front_UB = D(cn); r.pos_y_front_LB = D(cn);
    r.notWithinEnvironmentRear = J(cn * E); r.notWithinEnvironmentFrontUbUb = J(cn * E); r.notWithinEnvironmentFrontLbUb = J(cn * E);
    r.notWithinEnvironmentFrontUbLb = J(cn * E); r.notWithinEnvironmentFrontLbLb = J(cn * E); r.active_region = J(cn * R);
    r.region_change_not_allowed_x_positive = J(cn); r.region_change_not_allowed_y_positive = J(cn); r.region_change_not_allowed_x_negative = J(cn);
    r.region_change_not_allowed_y_negative = J(cn); r.region_change_not_allowed_combined = J(cn);
    r.deltacc = J(cn * O * L); r.deltacc_front = J(cn * O * L * 4); r.car2car_collision = J((size_t)K * K * N * 16); r.slackvars = J((size_t)K * K * N * 4);
    r.slackvarsObstacle = J(cn * O); r.slackvarsObstacle_front = J(cn * O * 4); r.slackvars_real = D((size_t)K * K * N * 4);
  }
  explicit OwnedResults(const HostInst& I) : OwnedResults(I.C, I.N, I.R, I.E, I.O, I.L) {}
  // deep copy of a caller's record of the same seven sizes (null arrays keep the fill value)
  void copy_from(const miqp_raw_results_c& f) {
    const double* const sd[13] = {f.u_x, f.u_y, f.pos_x, f.vel_x, f.acc_x, f.pos_y, f.vel_y, f.acc_y, f.pos_x_front_UB, f.pos_x_front_LB, f.pos_y_front_UB, f.pos_y_front_LB, f.slackvars_real};
    for (int k = 0; k < 13; ++k) if (sd[k]) std::copy(sd[k], sd[k] + d[k].size(), d[k].begin());
    const int* const si[17] = {f.notWithinEnvironmentRear, f.notWithinEnvironmentFrontUbUb, f.notWithinEnvironmentFrontLbUb, f.notWithinEnvironmentFrontUbLb, f.notWithinEnvironmentFrontLbLb,
                               f.active_region, f.region_change_not_allowed_x_positive, f.region_change_not_allowed_y_positive, f.region_change_not_allowed_x_negative,
                               f.region_change_not_allowed_y_negative, f.region_change_not_allowed_combined, f.deltacc, f.deltacc_front, f.car2car_collision, f.slackvars,
                               f.slackvarsObstacle, f.slackvarsObstacle_front};
    for (int k = 0; k < 17; ++k) if (si[k]) std::copy(si[k], si[k] + i[k].size(), i[k].begin());
  }
  // ... and the other way: this record into a caller's record of the same seven sizes (null arrays are skipped)
  void copy_to(miqp_raw_results_c& f) const {
    double* const sd[13] = {f.u_x, f.u_y, f.pos_x, f.vel_x, f.acc_x, f.pos_y, f.vel_y, f.acc_y, f.pos_x_front_UB, f.pos_x_front_LB, f.pos_y_front_UB, f.pos_y_front_LB, f.slackvars_real};
    for (int k = 0; k < 13; ++k) if (sd[k]) std::copy(d[k].begin(), d[k].end(), sd[k]);
    int* const si[17] = {f.notWithinEnvironmentRear, f.notWithinEnvironmentFrontUbUb, f.notWithinEnvironmentFrontLbUb, f.notWithinEnvironmentFrontUbLb, f.notWithinEnvironmentFrontLbLb,
                         f.active_region, f.region_change_not_allowed_x_positive, f.region_change_not_allowed_y_positive, f.region_change_not_allowed_x_negative,
                         f.region_change_not_allowed_y_negative, f.region_change_not_allowed_combined, f.deltacc, f.deltacc_front, f.car2car_collision, f.slackvars,
                         f.slackvarsObstacle, f.slackvarsObstacle_front};
    for (int k = 0; k < 17; ++k) if (si[k]) std::copy(i[k].begin(), i[k].end(), si[k]);
  }
};

// the seven sizes of a RawResults record against the loaded instance (a record of another shape is never indexed)
static bool dims_match(const miqp_raw_results_c& r, const HostInst& I) {
  return r.N == I.N && r.NrCars == I.C && r.NrRegions == I.R && r.NrEnvironments == I.E && r.NrObstacles == I.O &&
         (I.O == 0 || r.MaxLinesObstacles == I.L) && r.NrCarToCarCollisions == I.C - 1;
}

struct miqp_solver {
  miqp_solver_opts opts{};
  HostInst inst; bool has_inst = false;
  // last solution
  int status = MIQP_STATUS_FAILED_NO_SOLUT;
  miqp_solution_properties_c props{};
  std::vector<double> Z; std::vector<signed char> comp; bool has_sol = false;
  Layout lay{};
  double timing[6] = {0, 0, 0, 0, 0, 0};
  double as_timing[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // active-set launches of the last call (miqp_solver_last_active_set)
  int fixed_route = -1;   // which launch of the serial chain solved the last miqp_solver_solve_fixed node (miqp_solver_last_fixed_route); -1: no such call yet
  double setup[3] = {0, 0, 0};   // host set-up of the last call: seconds, of which the device context, 1 when the context was (re)built
  double admit_s = 0.0;          // when the last batch / stream call admitted this instance, in seconds after the first round of that call started
  // MIP starts (each tried as an additional root: binaries fixed, QP solved, accepted as incumbent when feasible).
  // Slot 0: receding-horizon start (addRecedingHorizonWarmstart), slot 1: last-solution start (.mst file); with
  // BOTH_WARMSTART_STRATEGIES the reference applies both (src/cplex_wrapper.cpp:124-138)
  std::unique_ptr<OwnedResults> ws[2];
  // result record of the last solve, built by miqp_solver_materialize_results (host threads, inside a batch call's timing) and
  // handed out by miqp_solver_get_results; dropped whenever the solution or the instance changes
  std::unique_ptr<OwnedResults> rescache;
  // what the last miqp_solver_solve_fixed_batch call of the handle left for miqp_solver_fixed_batch_record (fixed_batch.hip): the trajectories and fix
  // records of its accepted entries, and for each of its fb_n entries where its pair lies (-1: refused or infeasible); dropped by the next such
  // call and whenever the instance changes
  int fb_n = 0; std::vector<int> fb_slot; std::vector<double> fb_Z; std::vector<signed char> fb_fix;
  void drop_fixed_batch() { fb_n = 0; std::vector<int>().swap(fb_slot); std::vector<double>().swap(fb_Z); std::vector<signed char>().swap(fb_fix); }
  // solution pool (solution_pool.hip).  pool_cap: what miqp_solver_set_pool asked for, 0 = off.  Of the last solve: the pool_n kept fix records (best first),
  // their objectives as found and the record length; of the last miqp_solver_pool_solve: per entry whether it came out feasible, the fix record it was
  // refined with and its trajectory.  Dropped by the next solve and whenever the instance changes
  int pool_cap = 0, pool_n = 0, pool_fixlen = 0; std::vector<signed char> pool_fix; std::vector<double> pool_obj;
  bool pool_carried = false;   // the pool holds carried entries and no solve stands behind it (miqp_solver_pool_carry into an empty pool): miqp_solver_pool_count counts them
  int pool_fam = 0;   // miqp_solver_set_pool_filter: the families whose signature says which leaves are one entry, 0 = off (a setting like pool_cap: it stays)
  int pr_n = 0; std::vector<char> pr_ok; std::vector<signed char> pr_fix; std::vector<double> pr_Z;
  void drop_pool() { pool_n = 0; pr_n = 0; pool_carried = false; std::vector<signed char>().swap(pool_fix); std::vector<double>().swap(pool_obj); std::vector<char>().swap(pr_ok); std::vector<signed char>().swap(pr_fix); std::vector<double>().swap(pr_Z); }
  // starts from the carried pool (miqp_solver_set_pool_starts).  pool_starts: the most entries of a carried pool a solve takes as MIP-start
  // roots, 0 = off (a setting like pool_cap: it stays).  A solve drops the handle's pool when it begins: st_fix holds the st_offer records (st_fixlen
  // bytes each) it took from a carried pool before that, for prepare_instances.  Of the last solve: st_n start roots, and st_place[k], the entry of the
  // pool behind the solve that stands for start k (-1: none)
  int pool_starts = 0, st_offer = 0, st_fixlen = 0, st_n = 0; std::vector<signed char> st_fix; std::vector<int> st_place;
  void drop_starts() { st_offer = 0; st_fixlen = 0; st_n = 0; std::vector<signed char>().swap(st_fix); std::vector<int>().swap(st_place); }
  std::string err;
};

// host copies of the corner tables (kernels.hip: the same initialisers as the device's constant memory)
static const int ENV_PT_H[5][2] = MIQP_ENV_PT;
static const int OBS_PT_H[5][2] = MIQP_OBS_PT;

namespace {

// ---------------------------------------------------------------- raw model sizes
// rows / binary / continuous columns / non-zeros of the model OPL generates from cplexmodel/*.mod for this instance
// (cplex.getNrows / getNbinVars / getNcols - bin / getNNZs, src/cplex_wrapper.cpp:679-690).  Counted per statement of
// the .mod files: every `==` fixing is a row, duplicated rows stay, structural zero coefficients are dropped.
void raw_sizes(const HostInst& I, int& rows, int& bin, int& cont, int& nnz_out) {
  long C = I.C, N = I.N, R = I.R, E = I.E, O = I.O, L = I.L, K = I.C - 1;
  bin = (int)(C * N * (5 * E + R + 5 + 5 * O * L) + K * K * N * 16);
  cont = (int)(C * N * (12 + 5 * O) + K * K * N * 4);
  auto nz = [](double v) { return v != 0.0 ? 1L : 0L; };
  long a4 = 0, nnz = 0;
  nnz += C * (17 + 9 * R);                      // A1 initial_conditions.mod:11-61
  nnz += 24 * (N - 1) * C;                      // A2 model_region_constraints.mod:11-19
  nnz += 12 * N * C;                            // A3 :22-39
  for (int c = 0; c < C; ++c) {                 // A4 :43-117
    long P = 0, per = R;                        // the sum row carries R entries
    for (int j = 0; j < R; ++j) {
      if (I.possible[c * R + j] != 1) { per += 1; continue; }
      P++;
      const double* F = &I.frac[j * 4];
      per += nz(F[0]) + nz(F[1]) + 2 + nz(F[2]) + nz(F[3]) + 2;
      const int pt[4] = {2, 3, 0, 1};
      for (int k = 0; k < 4; ++k) { const double* p = &I.poly[pt[k]][j * 3]; per += 2 * (3 + nz(I.wb[c] * p[1]) + nz(I.wb[c] * p[2])); }
      per += 16;                                // jerk and acceleration boxes: 8 rows of 2
      double rho = (F[1] + F[3]) / (F[0] + F[2]);
      const double* kx = &I.poly[4][j * 3]; const double* kn = &I.poly[5][j * 3];
      per += 3 + nz(kx[1]) + nz(kx[2]) + nz(rho) + 3 + nz(kn[1]) + nz(kn[2]) + nz(rho);
    }
    a4 += 20 * P + (R - P) + 1;
    nnz += (N - 1) * per;
  }
  nnz += 35 * R * (N - 1) * C;                  // A5 minimum_speed_constraints.mod:9-49
  long env_edges = E > 0 ? I.env_off[E] : 0;
  if (E > 0) {                                  // A6 obstacle_environment_constraints.mod:6-47
    long per = 5 * E;
    for (long k = 0; k < env_edges; ++k) { const double* e = &I.env_edges[(size_t)k * 4]; per += 5 * (1 + nz(e[2] - e[0]) + nz(e[3] - e[1])); }
    nnz += N * C * per;
  }
  if (O > 0) {                                  // A7 :52-109
    for (int o = 0; o < O; ++o) for (int i = 0; i < N; ++i) {
      long per = 5 * (L + (I.obs_soft[o] == 1 ? 1 : 0));
      for (int k = 0; k < L; ++k) { const double* e = &I.obs_edges[((size_t)(o * N + i) * L + k) * 4]; per += 5 * (1 + nz(e[2] - e[0]) + nz(e[3] - e[1])); }
      nnz += C * per;
    }
  }
  if (C > 1) {                                  // A8 agent_collision_constraints.mod:10-73
    long tri = 0; for (long c1 = 2; c1 <= K; ++c1) tri += c1 - 1;
    nnz += N * 20 * tri + 76 * N * C * (C - 1) / 2;
  }
  int base[9]; miqp::raw_row_bases(I.C, I.N, I.R, I.E, I.O, I.L, (int)env_edges, (int)a4, base);   // the rows: the walker's own count
  rows = base[8]; nnz_out = (int)nnz;
}

// ---------------------------------------------------------------- host geometry helpers (results, step-1 presolve)
struct HostGeo {
  const HostInst& I; const Layout& Y; const double* D; const int* T;
  void point(int c, int i, int q /*possible idx*/, const double* z, int tx, int ty, double& X, double& Yc) const {
    if (i == 0) {
      X = I.x0[c * 6 + 0]; Yc = I.x0[c * 6 + 3];
      if (tx != PT_R) X = D[Y.d_theta + c * 4 + 0];
      if (ty != PT_R) Yc = D[Y.d_theta + c * 4 + 1];
      return;
    }
    const double* rt = D + Y.d_reg + (c * Y.P + q) * REGSZ;
    double vx = z[6 * c + 1], vy = z[6 * c + 4];
    X = z[6 * c + 0]; Yc = z[6 * c + 3];
    if (tx != PT_R) { const double* p = rt + 19 + (tx == PT_U ? 0 : 3); X += p[0] + p[1] * vx + p[2] * vy; }
    if (ty != PT_R) { const double* p = rt + 25 + (ty == PT_U ? 0 : 3); Yc += p[0] + p[1] * vx + p[2] * vy; }
  }
  double env_viol(int e, double X, double Yc) const {
    double v = -1e300; for (int k = 0; k < T[Y.i_envn + e]; ++k) { const double* ed = D + Y.d_env + (e * Y.EL + k) * 3; v = std::max(v, ed[0] * X + ed[1] * Yc - ed[2]); }
    return v;
  }
  double obs_viol(int o, int i, int k, double X, double Yc) const { const double* ed = D + Y.d_obs + ((o * Y.N + i) * Y.L + k) * 3; return ed[0] * X + ed[1] * Yc - ed[2]; }
  // zero-slack violation of (pair, step, group, alt): lhs + sep
  double c2c_viol(int p, int c1, int c2, int i, int grp, int alt, int q1, int q2, const double* z) const {
    double Dsep = D[Y.d_dsep + p * Y.N + i], S = D[Y.d_ssl + i];
    bool isx = alt < 2, lo = (alt == 0 || alt == 2), soft = (grp == 0 || grp == 3);
    int ca, cb, ta, tb;
    if (grp == 0) { ta = tb = PT_R; ca = lo ? c1 : c2; cb = lo ? c2 : c1; }
    else if (grp == 1) { if (lo) { ca = c1; ta = PT_R; cb = c2; tb = PT_L; } else { ca = c2; ta = PT_U; cb = c1; tb = PT_R; } }
    else if (grp == 2) { if (lo) { ca = c2; ta = PT_R; cb = c1; tb = PT_L; } else { ca = c1; ta = PT_U; cb = c2; tb = PT_R; } }
    else { if (lo) { ca = c2; ta = PT_U; cb = c1; tb = PT_L; } else { ca = c1; ta = PT_U; cb = c2; tb = PT_L; } }
    double XA, YA, XB, YB;
    point(ca, i, ca == c1 ? q1 : q2, z, ta, ta, XA, YA); point(cb, i, cb == c1 ? q1 : q2, z, tb, tb, XB, YB);
    return (isx ? XA - XB : YA - YB) + (soft ? Dsep + S : Dsep);
  }
};

// step 1 of the horizon is fixed by initial_conditions.mod:11-24 -> every row of it is a constant
bool step0_check(const HostGeo& G, double& cobj) {
  const HostInst& I = G.I; const Layout& Y = G.Y; double tol = FEAS_TOL; cobj = 0;
  for (int c = 0; c < I.C; ++c) {
    if (I.E >= 1)
      for (int pt = 0; pt < 5; ++pt) {
        double X, Yc; G.point(c, 0, 0, nullptr, ENV_PT_H[pt][0], ENV_PT_H[pt][1], X, Yc);
        bool any = false; for (int e = 0; e < I.E && !any; ++e) any = G.env_viol(e, X, Yc) <= tol;
        if (!any) return false;
      }
    for (int o = 0; o < I.O; ++o)
      for (int pt = 0; pt < 5; ++pt) {
        double X, Yc; G.point(c, 0, 0, nullptr, OBS_PT_H[pt][0], OBS_PT_H[pt][1], X, Yc);
        bool any = false; for (int k = 0; k < I.L && !any; ++k) any = G.obs_viol(o, 0, k, X, Yc) <= tol;
        if (!any) { if (I.obs_soft[o]) cobj += I.w_slack_obs; else return false; }
      }
  }
  int p = 0;
  for (int c1 = 0; c1 < I.C; ++c1)
    for (int c2 = c1 + 1; c2 < I.C; ++c2, ++p)
      for (int g = 0; g < 4; ++g) {
        double best = 1e300; double smax = G.D[Y.d_smax + 0];
        for (int a = 0; a < 4; ++a) {
          double v = G.c2c_viol(p, c1, c2, 0, g, a, 0, 0, nullptr);
          bool soft = (g == 0 || g == 3);
          if (v - (soft ? smax : 0.0) > tol) continue;
          double need = soft ? std::max(0.0, v) : 0.0;
          best = std::min(best, I.w_slack * need * need);
        }
        if (best > 1e299) return false;
        cobj += best;
      }
  return true;
}

}  // namespace


// ================================================================================================
//  device context (buffers are cached between calls with the same shape)
// ================================================================================================
namespace {

// ---------------------------------------------------------------- environment switches, by WHEN they are read
// Each name is read in one place per lifetime:
//   process: once, at the first solve of the process (ProcessSwitches)
//   context: when a device context is built, and latched in it until the shape of the call changes (CtxSwitches; MIQP_OPEN_CAP, MIQP_NPR and
//            MIQP_LANES shape the context through plan_call's result)
//   call:    at the start of every solve (read_call_switches for what the host decides with, apply_call_switches for the search fields of DevBuf)
struct ProcessSwitches {
  int prep_threads;          // (the 51 200 instances of the driver's stream on a 2 x 64-core host: 0.38 / 0.44 / 0.57 / 0.76 s at 16 / 32 / 64 / 128 threads - allocator and first-touch contention, not arithmetic)
  bool round_log;            // diagnostic: the batch sizes of the rounds, printed after the solve (no extra synchronisation)
  bool launch_trace; int replay, replay_round;   // diagnostics of solve_diag.hpp
  int big_grid_cap; double big_w1, big_w2;       // launch_ipm_batch
};
const ProcessSwitches& process_switches() {
  static const ProcessSwitches p = {
      knob_int(KNOB_T("MIQP_PREP_THREADS"), 16), knob_set(KNOB_P("MIQP_ROUND_LOG")),
      knob_set(KNOB_T("MIQP_LAUNCH_TRACE")), knob_int(KNOB_T("MIQP_REPLAY"), 0), knob_int(KNOB_T("MIQP_REPLAY_ROUND"), 0),
      knob_int(KNOB_T("MIQP_BIG_GRID"), 1 << 30),
      knob_double(KNOB_T("MIQP_BIG_W1"), 6.0), knob_double(KNOB_T("MIQP_BIG_W2"), 28.0)};   // (driver's stream, launch group / standard launch: 9.10 / 8.41 ms at 5 / 20, 8.76 / 8.50 at 6 / 28, 8.87 / 8.53 at 8 / 36)
  return p;
}

struct CtxSwitches {
  bool ipm_v1; int oc_waves;              // (experiment: resident wavefronts of the on-chip kernel per CU; 0: what its LDS admits)
  bool concurrent_big, oc_big; int oc_oversub;   // 0: off
  long long far_cap;                      // < 0: from the free memory
  bool warm;                              // warm start of the node relaxations (MIQP_WARM=0: cold)
  int opt2; double ws_mu, ws_delta; int as_chunk, as_quota;
  bool probe_overlap, stats, nocut;
};
CtxSwitches read_ctx_switches() {
  CtxSwitches c;
  c.ipm_v1 = knob_set(KNOB_T("MIQP_IPM_V1")); c.oc_waves = knob_int(KNOB_T("MIQP_OC_WAVES"), 0);
  c.concurrent_big = !knob_off(KNOB_T("MIQP_CONCURRENT_BIG")); c.oc_big = !knob_off(KNOB_T("MIQP_OC_BIG"));
  { const char* e = KNOB_T("MIQP_OC_OVERSUB"); c.oc_oversub = e ? std::max(1, std::min(64, std::atoi(e))) : 0; }
  { const char* e = KNOB_P("MIQP_FAR_CAP"); c.far_cap = e ? std::max(0LL, std::atoll(e)) : -1; }
  c.warm = !knob_off(KNOB_T("MIQP_WARM"));
  c.opt2 = knob_int(KNOB_T("MIQP_OPT2"), 8 << 4);   // rounding probe at nodes with at most 8 violated sites (eval_kernel)
  c.ws_mu = knob_double(KNOB_T("MIQP_WS_MU"), 1.0); c.ws_delta = knob_double(KNOB_T("MIQP_WS_DELTA"), 1.0e-3);
  c.as_chunk = knob_int(KNOB_T("MIQP_AS_CHUNK"), 1); c.as_quota = knob_int(KNOB_T("MIQP_AS_QUOTA"), 0);   // (runs of 2 / 4 / 8 / 16: the standard launch 4.7 -> 5.2 / 6.6 / 7.9 / 10.3 ms - a wavefront solves ~14 nodes per launch, longer runs only lengthen its tail)
  c.probe_overlap = !knob_off(KNOB_T("MIQP_PROBE_OVERLAP"));
  c.stats = knob_set(KNOB_P("MIQP_STATS"));   // (here: whether the counters are allocated)
  c.nocut = knob_set(KNOB_T("MIQP_NOCUT"));   // diagnostic: every node relaxation runs to convergence (tells infeasible children from expensive ones)
  return c;
}

// what the host side of a call decides with; the loop, the diagnostics and launch_ipm_batch read this (DevCtx::sw), not the environment
struct CallSwitches {
  int npr = 0, open_cap = 0;   // MIQP_NPR / MIQP_OPEN_CAP; 0: not set
  int seq_kinds = 5 << 8;      // plain K-way children, branching order 5 (see eval_kernel)
  bool debug_sync = false, trace = false, stats = false;
  bool memsets = false, cls_lists = true, big_pad = true;
  bool polish_cold = false; double polish_mu = 1.0e-2, polish_delta = 1.0e-4;   // the polish of the incumbents (polish())
  const char* dump_open = nullptr; const char* wave_dump = nullptr;            // diagnostics that write a file: its path
};
CallSwitches read_call_switches() {
  CallSwitches w;
  if (const char* e = KNOB_P("MIQP_NPR")) w.npr = std::max(1, std::atoi(e));   // tuning knob
  if (const char* e = KNOB_P("MIQP_OPEN_CAP")) w.open_cap = std::max(64, std::atoi(e));
  w.seq_kinds = knob_bits(KNOB_P("MIQP_SEQ_KINDS"), 5 << 8);
  w.debug_sync = knob_set(KNOB_P("MIQP_DEBUG_SYNC")); w.trace = knob_set(KNOB_P("MIQP_TRACE")); w.stats = knob_set(KNOB_P("MIQP_STATS"));
  w.memsets = knob_set(KNOB_T("MIQP_MEMSETS")); w.cls_lists = !knob_off(KNOB_T("MIQP_CLS_LISTS")); w.big_pad = !knob_off(KNOB_T("MIQP_BIG_PAD"));
  w.polish_cold = knob_set(KNOB_T("MIQP_POLISH_COLD")); w.polish_mu = knob_double(KNOB_T("MIQP_POLISH_MU"), 1.0e-2); w.polish_delta = knob_double(KNOB_T("MIQP_POLISH_DELTA"), 1.0e-4);
  w.dump_open = KNOB_T("MIQP_DUMP_OPEN"); w.wave_dump = KNOB_T("MIQP_WAVE_DUMP");
  return w;
}

// device side of the solution pool (solution_pool.hip): allocated with the context when a call asks for a pool, freed with it
struct SolPoolDev {
  int* list = nullptr; int* count = nullptr;   // the round's candidates: batch slots, and their number (two words, by the parity of the capture)
  signed char* fix = nullptr; double* obj = nullptr; unsigned int* hash = nullptr; int* cnt = nullptr; int* cap = nullptr;   // [n_inst][stride] records, objectives, hashes; [n_inst] entries kept, capacity asked for
  signed char* sig = nullptr; int* fam = nullptr;   // manoeuvre filter, only once a call had a handle with one: [n_inst][stride] signatures of the records, [n_inst] family sets
  bool filt = false;   // a handle of the call that holds the context has a filter: the capture launches pool_filter_kernel
  int n_inst = 0, stride = 0, list_cap = 0;
  int captures = 0;   // capture launches of the call: a capture uses count[captures & 1] and zeroes the other word for the next one (NOT the round number: rounds without a batch launch no capture)
  bool on = false;   // the call that holds the context has a handle with a pool
};

struct DevCtx {
  std::mutex mu;   // held for the whole solve: one solve at a time per device, different devices run concurrently
  bool ready = false; int device = -1;
  hipStream_t stream = nullptr;
  Layout Y{}; int n_inst = 0, n_slots = 0, open_cap = 0, far_cap = 0, batch_cap = 0, batch_alloc = 0, pool_cap = 0, npr = 0, ipm_grid_max = 1024;
  int n_inst_cap = 0;      // instances the per-instance arrays hold: a call with fewer reuses the context as it is
  int open_cap_req = 0;    // near-list capacity the caller asked for (open_cap: what the free memory allowed when the context was built)
  int mem_div = 1;         // contexts that share the device (lanes of one stream call): each sizes its pools for its share of the free memory
  int lane = 0;
  int* d_pairs = nullptr;   // admissions of one round: (slot, instance) pairs
  // concurrent launch of the memory-backed kernel on the rounding probes of a batch (second stream, its own work counter and
  // per-block buffers): see launch_ipm_batch
  hipStream_t stream2 = nullptr; hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_sfork = nullptr, ev_sjoin = nullptr;
  hipStream_t stream3 = nullptr, stream4 = nullptr; hipEvent_t ev_join3 = nullptr, ev_join4 = nullptr; double* kgain3 = nullptr;   // the larger active-set launch beside the interior point chain of stream2
  hipEvent_t ev_mid = nullptr;   // MIQP_LAUNCH_TRACE
  int* work_counter2 = nullptr; double* rowstate2 = nullptr; double* rowcache2 = nullptr; double* kgain2 = nullptr; int probe_grid = 0;
  int oc_grid = 0;   // resident wavefronts of the on-chip interior point kernel (0: the shape does not qualify)
  int kg_blocks = 0; // blocks the gain buffer holds
  int* ctr = nullptr; // two parity sets of 8 counters for the launches of a round (batch count, work counters, hand-over counts): a round uses one set, roll_kernel zeroes the other
  bool concurrent_big = true;   // MIQP_CONCURRENT_BIG=0: the sequential chain standard -> larger -> memory-backed
  int ocb_grid = 0;  // resident wavefronts of its larger variant (OC_GCAP_BIG general rows, one wavefront per SIMD; 0: not in use)
  bool as_on = false, as_cap = false; unsigned long long* as_stats = nullptr;
  int* cls_list = nullptr; int cls_n[3] = {-1, -1, -1};   // the round's class lists and (read back with the batch count) their lengths; -1: not known, the launches scan the batch
  unsigned short* as_batch_A = nullptr; unsigned short* as_pool_A = nullptr;   // (kept here: a call with MIQP_AS=0 runs with the DevBuf pointers nulled)   // dual active-set launch in front of the standard interior point launch (the shapes of as_shape_ok; MIQP_AS=0: off)
  DevBuf B{};
  CallSwitches sw;   // of the call that holds the context (apply_call_switches)
  SolPoolDev pool;
  std::vector<void*> allocs;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  std::vector<hipEvent_t> ipm_ev;  // pairs
  std::vector<hipEvent_t> std_ev;  // per round: the end of the standard launch on the solver stream
  template <class Tp> bool alloc(Tp** p, size_t n) {
    void* q = nullptr;
    if (hipMalloc(&q, std::max<size_t>(n, 1) * sizeof(Tp)) != hipSuccess) { std::fprintf(stderr, "[miqp_gpu] hipMalloc of %zu bytes failed\n", n * sizeof(Tp)); return false; }
    allocs.push_back(q); *p = (Tp*)q; return true;
  }
  template <class Tp> void drop(Tp** p) {   // one allocation given back ahead of release()
    if (!*p) return;
    for (auto it = allocs.begin(); it != allocs.end(); ++it) if (*it == (void*)*p) { allocs.erase(it); break; }
    (void)hipFree(*p); *p = nullptr;
  }
  void release() {
    for (void* q : allocs) (void)hipFree(q);
    allocs.clear();
    for (auto e : ipm_ev) (void)hipEventDestroy(e);
    ipm_ev.clear();
    for (auto e : std_ev) (void)hipEventDestroy(e);
    std_ev.clear();
    pool = SolPoolDev{};
    ready = false;
  }
};

// one context per HIP device (the reference has one IloEnv per wrapper; here the device buffers are shared by the
// handles that solve on the same device and serialised by the context's mutex)
std::mutex g_ctx_table_mu;
std::map<int, std::unique_ptr<DevCtx>> g_ctx_table;

// resolves `device` (-1: the current device) and returns its context; nullptr without a HIP device
DevCtx* ctx_for_device(int device, int lane = 0) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { std::fprintf(stderr, "[miqp_gpu] no HIP device: the solver has no CPU path\n"); return nullptr; }
  if (device < 0) { if (hipGetDevice(&device) != hipSuccess) device = 0; }
  if (device >= ndev) { std::fprintf(stderr, "[miqp_gpu] device %d requested, %d visible\n", device, ndev); return nullptr; }
  std::lock_guard<std::mutex> lk(g_ctx_table_mu);
  auto& slot = g_ctx_table[device * 16 + (lane & 15)];   // lane 0: the context of the device; lanes 1..: the further contexts of a stream call that shares the device
  if (!slot) { slot.reset(new DevCtx()); slot->device = device; slot->lane = lane; }
  return slot.get();
}

size_t ipm_lds_bytes(const Layout& Y);

bool same_layout(const Layout& a, const Layout& b) { return std::memcmp(&a, &b, sizeof(Layout)) == 0; }

// caller holds X.mu; X.device is the resolved device ordinal
// n_inst instances in the call (the queue), n_slots of them in flight at a time (list storage per slot), roots_per_inst root records each
// `clamp_open`: the near-list capacity may be cut to what an eighth of the free memory holds (40 B per entry)
// A ready context of the same shape is reused as it is when the call has no more instances than its per-instance arrays hold
// (built for 64 queues' worth at least, within 4 GB): releasing and reallocating the pools - most of the device memory - costs
// seconds, and a service that drains one queue after the other must not pay them per call (measured: 4.3 s of a 17 s bench stream).
bool ctx_matches(const DevCtx& X, const Layout& Y, int n_inst, int n_slots, int open_cap, int npr, int roots_per_inst, int mem_div) {
  return X.ready && same_layout(X.Y, Y) && n_inst <= X.n_inst_cap && X.n_slots == n_slots && X.open_cap_req == open_cap && X.npr == npr && X.B.root_stride == roots_per_inst && X.mem_div == mem_div;
}

// Every capacity of a context: a pure function of the shape, the memory that is free on the device, its CU count and the context switches.
// ctx_alloc walks it; the footprint of a context is this value.
struct CtxSizes {
  int n_inst_cap, open_cap, far_cap, pool_cap, z_cap, batch_cap, batch_alloc;
  int ipm_grid_max, oc_grid, ocb_grid, kg_blocks, probe_grid;
  bool concurrent_big, as_cap, as_starts;   // as_starts: the parents' active sets are kept for the children's starts
  size_t ring_doubles, ring_margin;         // 0: no ring
};
CtxSizes ctx_sizes(const Layout& Y, int n_inst, int n_slots, int open_cap, int npr, int roots_per_inst, bool clamp_open, int mem_div, bool free_known, size_t free_b, int cus, const CtxSwitches& cs) {
  CtxSizes Z{};
  if (clamp_open && free_known) { const size_t lim = free_b / (size_t)mem_div / 8 / 40 / (size_t)n_slots; if ((size_t)open_cap > lim) open_cap = (int)std::max<size_t>(4096, lim); }
  Z.open_cap = open_cap;
  {   // capacity of the per-instance arrays (tables, incumbent records: dstride * 8 + istride * 4 + fix record + solution per instance)
    const size_t per = (size_t)Y.dstride * 8 + (size_t)Y.istride * 4 + (size_t)Y.fixlen * 2 + (size_t)Y.N * Y.nz * 16 + 256;
    size_t cap = std::min<size_t>((size_t)64 * (size_t)n_slots, ((size_t)4 << 30) / per);
    Z.n_inst_cap = (int)std::max<size_t>((size_t)n_inst, cap);
  }
  n_inst = Z.n_inst_cap;   // everything below is sized for the capacity
  Z.batch_cap = n_slots * npr;
  const int batch_alloc = Z.batch_alloc = std::max(Z.batch_cap, n_inst);   // the final polish solves one node per instance in one launch
  // resident workgroups of the memory-backed kernel per CU: what its LDS admits, and its wavefronts per SIMD (three and four cars: workgroups of four wavefronts)
  size_t l = ipm_lds_bytes(Y); int per = (int)std::max<size_t>(1, std::min<size_t>(Y.C <= 2 ? 4 * MIQP_IPM_WPE : (4 * MIQP_WIDE_WPE) / (MIQP_WIDE_NT / 64), (160 * 1024) / std::max<size_t>(l + 8, 1))); Z.ipm_grid_max = cus * per;
  // on-chip kernel: up to two cars, horizon within its register slots; 2 wavefronts per SIMD, as many as its LDS admits
  Z.concurrent_big = true;
  const OcLds ol = oc_lds_layout(Y.N, Y.fixlen);
  const size_t bitmap_b = (size_t)((Y.N * Y.NSLOT + 63) / 64) * 10 + 16;   // decode bitmap + prefix inside the scratch region
  if (Y.C <= 2 && Y.N <= 2 * OC_NSL && bitmap_b + 1024 <= (size_t)(ol.r - ol.u) && !cs.ipm_v1) {
    size_t lo = (size_t)ol.total + 16;
    int perc = (int)std::min<size_t>(8, (160 * 1024) / lo);
    if (cs.oc_waves) perc = std::max(1, std::min(perc, cs.oc_waves));
    if (perc >= 1) Z.oc_grid = cus * perc;
    Z.concurrent_big = cs.concurrent_big;
    if (Z.oc_grid > 0 && cs.oc_big) {
      const size_t lb = (size_t)oc_lds_layout(Y.N, Y.fixlen, OC_GCAP_BIG).total + 16;
      const int pb = (int)std::min<size_t>(4, (160 * 1024) / lb);
      if (pb >= 1) Z.ocb_grid = cus * pb;
    }
  }
  if (Z.oc_grid > Z.ipm_grid_max) Z.ipm_grid_max = Z.oc_grid;   // the per-block buffers are sized for the larger grid
  // Oversubscribed launches of the on-chip kernels (MIQP_OC_OVERSUB = F): F times the resident wavefronts, each working through 1 / F of the
  // nodes - a wavefront slot comes free F times as often, so the short kernels of ANOTHER lane of the same device (MIQP_LANES: its
  // evaluation and selection) are dispatched between them instead of waiting for the whole launch.  Only the gain buffer grows.
  Z.kg_blocks = Z.ipm_grid_max;
  if (const int f = cs.oc_oversub) { Z.oc_grid = std::min(batch_alloc, Z.oc_grid * f); Z.ocb_grid = std::min(batch_alloc, Z.ocb_grid * f); Z.kg_blocks = std::max(Z.kg_blocks, std::max(Z.oc_grid, Z.ocb_grid)); }
  // node pool: live nodes are bounded by the open lists plus one round of children; processed records are recycled
  if (!free_known) free_b = (size_t)16 << 30;
  free_b /= (size_t)mem_div;
  // far tier of the open lists (16 B per entry): up to 2^24 entries per instance within a tenth of the free memory
  // (256 instances: 4 M entries each, 16 GB); MIQP_FAR_CAP overrides, 0 switches the tier off
  { size_t fc = std::min<size_t>((size_t)1 << 24, free_b / 10 / 16 / (size_t)n_slots);
    if (cs.far_cap >= 0) fc = (size_t)cs.far_cap;
    Z.far_cap = fc < 4096 ? 0 : (int)fc; }
  size_t want = (size_t)n_slots * ((size_t)open_cap + (size_t)Z.far_cap + (size_t)npr * 64 + 64) + (size_t)n_inst * roots_per_inst;
  size_t maxrec = std::min<size_t>((size_t)64 << 30, free_b / 4) / (size_t)Y.fixlen;   // node records: up to 64 GB of the 288 GB, at most a quarter of what is free
  Z.pool_cap = (int)std::min<size_t>(std::min(want, maxrec), (size_t)0x7FFFFFF0);
  // the parents' solutions for the warm starts: for the first z_cap records (recycled records keep the live set at low
  // indices) - 16384 per instance in flight, at least 2 M, within an eighth of the free memory (42 GB at 1024 in flight, 5 GB
  // for a single solve: a large allocation costs seconds, and a context is rebuilt whenever the shape of the call changes)
  if (cs.warm) {
    const size_t zb = (size_t)Y.N * Y.nz * 8;
    size_t zc = std::max<size_t>((size_t)2 << 20, (size_t)n_slots * 16384);
    Z.z_cap = (int)std::min(zc, std::min<size_t>((size_t)Z.pool_cap, free_b / 8 / zb));
  }
  Z.as_cap = as_shape_ok(Y.C, Y.N) && Z.oc_grid > 0;   // the shape has the active-set launches (whether a call uses them: MIQP_AS, read per call)
  Z.as_starts = Z.as_cap && Z.z_cap > 0 && Y.N * Y.NSLOT + 1024 < 65535;   // the parents' active sets for the children's starts (128 B per record)
  if (Z.as_starts) {
    // ... and the ring their M travels through (4 KB per node on average, at most 12.8): a quarter of the free memory, at most 96 GB
    const size_t margin = (size_t)batch_alloc * AS_MSTR + ((size_t)1 << 20);   // what one round's launches can allocate, and more
    // two cars: 64 MB per instance in flight, at least 8 GB (a single solve: hundreds of its rounds; a large allocation costs seconds when the context is built).
    // One car - the single planning call, whose context should stay small: four times what a round of batch_alloc nodes can write if every one of them
    // left a full triangle (an M stays whole for three such rounds at the least; at the ~20 active rows of a node, 1.7 KB of the 16.6 KB, for tens)
    const size_t rd = Y.C == 1 ? std::min<size_t>(free_b / 4 / 8, 4 * margin)
                               : std::min<size_t>(std::min<size_t>((size_t)12 << 30, free_b / 4 / 8), std::max<size_t>((size_t)1 << 30, (size_t)n_slots * ((size_t)8 << 20)));   // doubles
    if (rd >= 2 * margin) { Z.ring_doubles = rd; Z.ring_margin = margin; }
  }
  // buffers of the concurrent probe launch (two cars and fewer, on-chip kernel in use): 1024 resident blocks
  if (Z.oc_grid > 0 && cs.probe_overlap) Z.probe_grid = std::min(batch_alloc, 1536);
  return Z;
}

// the allocations of a context, in the order that decides their addresses
bool ctx_alloc(DevCtx& X, const CtxSizes& Z, const CtxSwitches& cs, int n_call, int n_slots, int npr, int roots_per_inst) {
  const Layout& Y = X.Y;
  const int n_inst = Z.n_inst_cap, open_cap = Z.open_cap, batch_alloc = Z.batch_alloc;
  X.n_inst_cap = Z.n_inst_cap; X.open_cap = Z.open_cap; X.far_cap = Z.far_cap; X.pool_cap = Z.pool_cap; X.batch_cap = Z.batch_cap; X.batch_alloc = Z.batch_alloc;
  X.ipm_grid_max = Z.ipm_grid_max; X.oc_grid = Z.oc_grid; X.ocb_grid = Z.ocb_grid; X.kg_blocks = Z.kg_blocks; X.concurrent_big = Z.concurrent_big;
  DevBuf& B = X.B; std::memset(&B, 0, sizeof(B));
  // (cut_gate, seq_kinds and the other search fields: apply_call_switches, at every call)
  B.qp_tol = QP_TOL; B.use_cutoff = cs.nocut ? 0 : 1;
  B.opt2 = cs.opt2;
  B.Y = Y; B.pool_cap = X.pool_cap; B.open_cap = open_cap; B.batch_cap = Z.batch_cap; B.nodes_per_round = npr; B.n_inst = n_call; B.n_slots = n_slots; B.root_stride = roots_per_inst;
  double* dd; int* ii;
  if (!X.alloc(&dd, (size_t)n_inst * Y.dstride)) return false; B.inst_d = dd;
  if (!X.alloc(&ii, (size_t)n_inst * Y.istride)) return false; B.inst_i = ii;
  if (!X.alloc(&B.pool_fix, (size_t)X.pool_cap * Y.fixlen)) return false;
  if (cs.warm && !X.alloc(&B.pool_Z, (size_t)Z.z_cap * (size_t)Y.N * Y.nz)) return false;
  B.z_cap = Z.z_cap;
  B.ws_on = cs.warm ? 1 : 0; B.ws_mu = cs.ws_mu; B.ws_delta = cs.ws_delta;
  if (!X.alloc(&B.pool_count, 1)) return false;
  if (!X.alloc(&B.free_q, (size_t)X.pool_cap)) return false;
  if (!X.alloc(&B.free_head, 1)) return false;
  if (!X.alloc(&B.free_tail, 1)) return false;
  if (!X.alloc(&B.free_limit, 1)) return false;
  if (!X.alloc(&B.open_bound, (size_t)2 * n_slots * open_cap)) return false;
  if (!X.alloc(&B.open_node, (size_t)2 * n_slots * open_cap)) return false;
  if (!X.alloc(&B.open_depth, (size_t)2 * n_slots * open_cap)) return false;
  if (!X.alloc(&B.open_key, (size_t)n_slots * open_cap)) return false;
  if (!X.alloc(&B.inst_slot, n_inst)) return false;
  if (!X.alloc(&B.slot_inst, n_slots)) return false;
  if (!X.alloc(&B.inst_kill, n_inst)) return false;
  if (!X.alloc(&B.slot_demand, n_slots)) return false;
  if (!X.alloc(&B.slot_take, n_slots)) return false;
  { int* rc; int* rn; int* rd; if (!X.alloc(&rc, n_inst)) return false; if (!X.alloc(&rn, (size_t)n_inst * roots_per_inst)) return false; if (!X.alloc(&rd, (size_t)n_inst * roots_per_inst)) return false;
    B.root_cnt = rc; B.root_node = rn; B.root_depth = rd; }
  if (!X.alloc(&X.d_pairs, (size_t)2 * n_slots)) return false;
  if (!X.alloc(&B.open_count, n_inst)) return false;
  B.far_cap = X.far_cap;
  if (X.far_cap > 0) {
    if (!X.alloc(&B.far_bound, (size_t)n_slots * X.far_cap)) return false;
    if (!X.alloc(&B.far_node, (size_t)n_slots * X.far_cap)) return false;
    if (!X.alloc(&B.far_depth, (size_t)n_slots * X.far_cap)) return false;
  }
  if (!X.alloc(&B.far_count, n_inst)) return false;
  if (!X.alloc(&B.far_minkey, n_inst)) return false;
  if (!X.alloc(&B.near_thr, n_inst)) return false;
  if (!X.alloc(&B.inst_mode, n_inst)) return false;
  if (!X.alloc(&B.inc_key, n_inst)) return false;
  if (!X.alloc(&B.inc_seen, n_inst)) return false;
  if (!X.alloc(&B.inc_obj, n_inst)) return false;
  if (!X.alloc(&B.inc_ext, n_inst)) return false;
  if (!X.alloc(&B.inc_fix, (size_t)n_inst * Y.fixlen)) return false;
  if (!X.alloc(&B.inc_Z, (size_t)n_inst * Y.N * Y.nz)) return false;
  if (as_shape_ok(Y.C, Y.N)) { if (!X.alloc(&B.inc_A, (size_t)n_inst * 64) || !X.alloc(&B.inc_Mtag, (size_t)n_inst)) return false; } else { B.inc_A = nullptr; B.inc_Mtag = nullptr; }
  if (!X.alloc(&B.lower_bound, n_inst)) return false;
  if (!X.alloc(&B.inst_done, n_inst)) return false;
  if (!X.alloc(&B.inst_flags, n_inst)) return false;
  if (!X.alloc(&B.inst_gap, n_inst)) return false;
  if (!X.alloc(&B.inst_const, n_inst)) return false;
  if (!X.alloc(&B.inst_nodes, n_inst)) return false;
  if (!X.alloc(&B.inst_iters, n_inst)) return false;
  if (!X.alloc(&B.inst_ninc, n_inst)) return false;
  if (!X.alloc(&B.inst_lns, n_inst)) return false;
  if (!X.alloc(&B.inst_lns_obj, n_inst)) return false;
  if (!X.alloc(&B.batch_count, 1)) return false;
  if (!X.alloc(&B.batch_node, batch_alloc)) return false;
  if (!X.alloc(&B.batch_candkey, batch_alloc)) return false;
  HIP_OK(hipMemset(B.batch_candkey, 0xFF, (size_t)batch_alloc * 8));
  if (!X.alloc(&B.batch_candinst, batch_alloc)) return false;
  HIP_OK(hipMemset(B.batch_candinst, 0xFF, (size_t)batch_alloc * 4));
  if (!X.alloc(&B.batch_inst, batch_alloc)) return false;
  if (!X.alloc(&B.batch_large, batch_alloc)) return false;
  HIP_OK(hipMemset(B.batch_large, 0, (size_t)batch_alloc));
  if (!X.alloc(&B.batch_depth, batch_alloc)) return false;
  if (!X.alloc(&B.batch_Z, (size_t)batch_alloc * Y.N * Y.nz)) return false;
  if (!X.alloc(&B.batch_obj, batch_alloc)) return false;
  if (!X.alloc(&B.batch_viol, batch_alloc)) return false;
  if (!X.alloc(&B.batch_ok, batch_alloc)) return false;
  if (!X.alloc(&B.batch_it, batch_alloc)) return false;
  if (!X.alloc(&B.batch_bound, batch_alloc)) return false;
  if (!X.alloc(&B.batch_comp, (size_t)batch_alloc * Y.fixlen)) return false;
  if (!X.alloc(&B.rowstate, (size_t)std::min(batch_alloc, X.ipm_grid_max) * NFIELD * Y.ROWCAP)) return false;
  if (!X.alloc(&B.rowcache, (size_t)std::min(batch_alloc, X.ipm_grid_max) * NCACHE * Y.ROWCAP)) return false;
  if (!X.alloc(&B.kgain, (size_t)std::min(batch_alloc, X.kg_blocks) * std::max(Y.N * Y.nu * (Y.nx + 2), oc_gain_doubles(Y.N)))) return false;
  if (!X.alloc(&B.work_counter, 1)) return false;
  if (!X.alloc(&X.ctr, 2 * CTR_SET)) return false;
  HIP_OK(hipMemset(X.ctr, 0, 2 * CTR_SET * 4));
  X.as_cap = Z.as_cap;
  X.as_on = X.as_cap;
  if (X.as_cap && !X.alloc(&X.cls_list, (size_t)3 * Z.batch_cap)) return false;   // the class lists of a round (large_class 1 / 2 / 3)
  if (!X.alloc(&X.as_stats, 32)) return false;
  HIP_OK(hipMemset(X.as_stats, 0, 256));
  B.as_stats = X.as_stats; B.as_chunk = cs.as_chunk; B.as_quota = cs.as_quota;
  X.as_batch_A = nullptr; X.as_pool_A = nullptr;
  if (Z.as_starts) {
    if (!X.alloc(&B.batch_A, (size_t)batch_alloc * 64)) return false;
    if (!X.alloc(&B.pool_A, (size_t)B.z_cap * 64)) return false;
    // (pool_A / pool_Mtag need no initial value: a record's entries are written when the record is created - eval_kernel, lns_kernel - and roots start cold)
    HIP_OK(hipMemset(B.batch_A, 0xFF, (size_t)batch_alloc * 128));
    X.as_batch_A = B.batch_A; X.as_pool_A = B.pool_A;
    if (Z.ring_doubles) {
      if (!X.alloc(&B.ring_M, Z.ring_doubles)) return false;
      if (!X.alloc(&B.ring_head, 1)) return false;
      if (!X.alloc(&B.batch_Mtag, batch_alloc)) return false;
      if (!X.alloc(&B.pool_Mtag, (size_t)B.z_cap)) return false;
      { const unsigned long long h0 = 1024ull; HIP_OK(hipMemcpy(B.ring_head, &h0, 8, hipMemcpyHostToDevice)); }
      HIP_OK(hipMemset(B.batch_Mtag, 0, (size_t)batch_alloc * 8));
      B.ring_doubles = (unsigned long long)Z.ring_doubles; B.ring_margin = (unsigned long long)Z.ring_margin;
    }
  }
  X.probe_grid = Z.probe_grid;
  if (X.probe_grid > 0) {
    if (!X.alloc(&X.work_counter2, 1)) return false;
    if (!X.alloc(&X.rowstate2, (size_t)X.probe_grid * NFIELD * Y.ROWCAP)) return false;
    if (!X.alloc(&X.rowcache2, (size_t)X.probe_grid * NCACHE * Y.ROWCAP)) return false;
    if (!X.alloc(&X.kgain2, (size_t)X.probe_grid * std::max(Y.N * Y.nu * (Y.nx + 2), oc_gain_doubles(Y.N)))) return false;
    if (!X.stream2) { HIP_OK(hipStreamCreate(&X.stream2)); HIP_OK(hipEventCreate(&X.ev_fork)); HIP_OK(hipEventCreate(&X.ev_join)); HIP_OK(hipEventCreate(&X.ev_sfork)); HIP_OK(hipEventCreate(&X.ev_sjoin)); }
    if (!X.stream3) { HIP_OK(hipStreamCreate(&X.stream3)); HIP_OK(hipEventCreate(&X.ev_join3)); HIP_OK(hipStreamCreate(&X.stream4)); HIP_OK(hipEventCreate(&X.ev_join4)); }
    if (!X.alloc(&X.kgain3, (size_t)X.probe_grid * std::max(Y.N * Y.nu * (Y.nx + 2), oc_gain_doubles(Y.N)))) return false;
  }
  if (!X.alloc(&B.ovf_count, 1)) return false;
  if (!X.alloc(&B.ovf_list, batch_alloc)) return false;
  { if (!X.alloc(&B.pool_big, (size_t)X.pool_cap)) return false; HIP_OK(hipMemset(B.pool_big, 0, (size_t)X.pool_cap)); }   // (size mark of the on-chip variants; its high nibble counts the re-roundings of a probe, for every kernel)
  if (!X.alloc(&B.ovf2_count, 1)) return false;
  if (!X.alloc(&B.ovf2_list, batch_alloc)) return false;
  HIP_OK(hipMemset(B.ovf2_count, 0, 4));
  HIP_OK(hipMemset(B.ovf_count, 0, 4));
  if (cs.stats) {
    if (!X.alloc(&B.stats, 256)) return false; HIP_OK(hipMemset(B.stats, 0, 256 * 8));
    if (!X.alloc(&B.pool_origin, (size_t)X.pool_cap)) return false; HIP_OK(hipMemset(B.pool_origin, 0, (size_t)X.pool_cap));
  }
  if (!X.alloc(&B.prof, 160 + 5 * 4 * 4096)) return false;
  (void)hipMemset(B.prof, 0, (160 + 5 * 4 * 4096) * 8);
  if (!X.alloc(&B.active_insts, 1)) return false;
  if (!X.alloc(&B.stat_rowiters, 1)) return false;
#ifdef MIQP_PROFILE
  if (!B.pool_origin) { if (!X.alloc(&B.pool_origin, (size_t)X.pool_cap)) return false; HIP_OK(hipMemset(B.pool_origin, 0, (size_t)X.pool_cap)); }
#endif
  return true;
}

std::mutex g_ctx_build_mu;   // contexts are built one at a time: each sizes its pools from the memory that is free at that moment
// `rebuilt` (optional): whether the call found no matching context and built one
bool ctx_prepare(DevCtx& X, const Layout& Y, int n_inst, int n_slots, int open_cap, int npr, int roots_per_inst, bool clamp_open = false, int mem_div = 1, bool* rebuilt = nullptr) {
  HIP_OK(hipSetDevice(X.device));   // the calling thread's current device (threads of solve_batch_multi each set their own)
  const bool reuse = ctx_matches(X, Y, n_inst, n_slots, open_cap, npr, roots_per_inst, mem_div);
  if (rebuilt) *rebuilt = !reuse;
  if (reuse) { X.n_inst = n_inst; X.B.n_inst = n_inst; return true; }
  std::lock_guard<std::mutex> build_lock(g_ctx_build_mu);
  if (X.ready || !X.allocs.empty()) X.release();
  if (!X.stream) HIP_OK(hipStreamCreate(&X.stream));
  if (!X.ev0) { HIP_OK(hipEventCreate(&X.ev0)); HIP_OK(hipEventCreate(&X.ev1)); }
  X.open_cap_req = open_cap; X.mem_div = mem_div < 1 ? 1 : mem_div;
  // (the memory that is free and the CU count are read after the old context is released and before the first allocation of the new one)
  size_t free_b = 0, total_b = 0; const bool free_known = hipMemGetInfo(&free_b, &total_b) == hipSuccess;
  hipDeviceProp_t pr; int dv = 0; (void)hipGetDevice(&dv); int cus = 256; if (hipGetDeviceProperties(&pr, dv) == hipSuccess) cus = pr.multiProcessorCount;
  const CtxSwitches cs = read_ctx_switches();
  const CtxSizes Z = ctx_sizes(Y, n_inst, n_slots, open_cap, npr, roots_per_inst, clamp_open, X.mem_div, free_known, free_b, cus, cs);
  X.Y = Y; X.n_inst = n_inst; X.n_slots = n_slots; X.npr = npr;
  if (!ctx_alloc(X, Z, cs, n_inst, n_slots, npr, roots_per_inst)) return false;
  X.ready = true;
  return true;
}

constexpr int IPM_NT = 64;  // one wavefront per node in the interior point kernel ...
constexpr int IPM_NT_WIDE = MIQP_WIDE_NT;   // ... two (or four) for three and four cars (ipm_kernel: the four MFMA tiles of the 2 x 2-tiled stage algebra are shared out over the wavefronts)
constexpr int ipm_nt(int C) { return C >= 3 ? IPM_NT_WIDE : IPM_NT; }
size_t ipm_lds_bytes(const Layout& Y) {
  int NZ = Y.nz, N = Y.N;
  size_t d = (size_t)N * NZ + (size_t)ipm_scratch_doubles(N, Y.C) + NZ + 8 + 32 + 2 * ((N + 6) / 2 + 1);
  return d * 8 + (size_t)Y.fixlen + 16;
}
bool multi_row_lifting_on(int seq_kinds) { return ((unsigned)seq_kinds & 0x80000000u) != 0u; }
size_t eval_lds_bytes(const Layout& Y, int seq_kinds) {
  size_t d = (size_t)Y.N * Y.nz + (size_t)eval_shared_doubles(Y.C, Y.N, Y.P) + 2 * (size_t)Y.C * Y.N;   // (the slow-alternative table and the lifting's dense rows share one region)
  return d * 8 + (size_t)(2 * Y.C * Y.N + 64) * 4 + 64 * 8 + 3 * (size_t)Y.fixlen + 8 + 64
         + (multi_row_lifting_on(seq_kinds) ? (size_t)(LIFT_ROWS * (2 * Y.nz + 3) + Y.nz) * 8 : 0) + 64   // rows of the multi-row lifting (an experiment: MIQP_SEQ_KINDS bit 31)
         + (size_t)Y.fixlen + 16;                                  // ploose
}

// the node kernels of a round, by kind and car count: the launcher and set_kernel_lds take a kernel from here and nowhere else.  (The compiler emits the
// instantiations in the order they are named here: the rows keep the order the launches named them in, and with it the code object byte for byte.)
enum NodeKernel { NK_IPM, NK_AS_BIG, NK_OC_BIG, NK_AS, NK_OC, NK_KINDS };   // memory-backed ipm_kernel; larger active-set, larger on-chip interior point; standard active-set, standard on-chip interior point
using NodeKernelFn = void (*)(DevBuf);
const NodeKernelFn NODE_KERNEL[NK_KINDS][4] = {
    {ipm_kernel<1, ipm_nt(1)>, ipm_kernel<2, ipm_nt(2)>, ipm_kernel<3, ipm_nt(3)>, ipm_kernel<4, ipm_nt(4)>},
    {as_onchip_kernel<1, OC_NSL, OC_GCAP_BIG>, as_onchip_kernel<2, OC_NSL, OC_GCAP_BIG>, nullptr, nullptr},
    // the larger variant: works through the list of the standard one (ovf_mode 1) or through the rounding probes of the batch (ovf_mode 2, on its
    // own stream with its own work counter)
    {ipm_onchip_kernel<1, OC_NSL, 0, OC_GCAP_BIG>, ipm_onchip_kernel<2, OC_NSL, 0, OC_GCAP_BIG>, nullptr, nullptr},
    {as_onchip_kernel<1, OC_NSL>, as_onchip_kernel<2, OC_NSL>, nullptr, nullptr},
    {ipm_onchip_kernel<1, OC_NSL>, ipm_onchip_kernel<2, OC_NSL>, nullptr, nullptr}};
template <int C> void launch_eval(const DevBuf& B, int nblocks, size_t lds, hipStream_t st) { hipLaunchKernelGGL(eval_kernel<C>, dim3(nblocks), dim3(64), lds, st, B); }

// LDS of a larger launch's block beside the standard active-set launch: padded to TWO blocks of that launch (rounded to the allocation granule), as
// long as four of them still fit a CU.  A larger block leaves a hole behind when it ends; the unpadded 34 KB took one standard block of 19.6 KB and
// wasted the rest - no CU ever held more than seven of its eight standard blocks again (tools/wave_dump.py, tools/resident_lab.hip)
inline size_t oc_big_lds_beside_as(const Layout& Y) {
  const size_t lb = (size_t)oc_lds_layout(Y.N, Y.fixlen, OC_GCAP_BIG).total, la = (size_t)oc_lds_layout(Y.N, Y.fixlen, OC_GCAP, true).total;
  const size_t st_ = 8 + 256;   // static LDS of the active-set kernels: the hand-out word and the wavefront's statistics
  const size_t two = 2 * ((la + st_ + 1279) / 1280 * 1280) - st_;
  return (two >= lb && 4 * (two + st_) <= 160 * 1024) ? two : lb;
}

// ---------------------------------------------------------------- the node launches of a round: a plan (pure) and its launcher
// interior point solves of the first `bc` batch entries: the on-chip kernel where the shape qualifies, followed by the
// memory-backed kernel on the nodes it handed over (their count stays on the device: no host round trip); else the
// memory-backed kernel on everything.  plan_node_launches decides, run_node_launches issues, launch_ipm_batch is the two together.
// One launch of a round.  Every field is an int: a row of the plan is what miqp_solver_launch_plan writes out
enum { Z_WORK = 1, Z_OVF = 2, Z_OVF2 = 4 };           // NodeLaunch::zero: the launch's work counter and hand-over count, on its stream; the larger variant's hand-over count, on
                                                      // stream 0 ahead of the fork (the launches of every stream append to that list)
enum { BUF_PRIMARY, BUF_SECOND, BUF_KGAIN3 };         // NodeLaunch::bufs: the batch's per-block buffers, those of the second stream, those with the gain buffer of the fourth
struct NodeLaunch {
  int kind, stream, grid, lds;                        // NodeKernel; 0: the caller's stream, 2 .. 4: stream2 .. stream4; workgroups; dynamic LDS bytes
  int ovf_mode, cls_take, as_split, skip_probes, bounce;   // the DevBuf fields of these names
  int work;                                           // work counter: > 0 that word of the round's parity set, 0 the batch's own, -1 the second stream's (work_counter2)
  int from_ovf2;                                      // hand-over count and list it reads: 0 the standard launch's (ovf_count, ovf_list), 1 the larger variant's (ovf2_count, ovf2_list)
  int bufs, zero;
};
static_assert(sizeof(NodeLaunch) == 13 * sizeof(int), "a row of the plan is the 13 ints of include/miqp_gpu.h");
// the launches of a round in the order they are issued; rebuilt every round (no allocation).  A launch without a workgroup - an empty class list - is not in it
struct RoundPlan {
  int n = 0, par = -1;   // par >= 0: the counters of the launches are that parity set of DevCtx::ctr, zeroed one round ahead by roll_kernel (no memset in the stream)
  NodeLaunch l[5], none;
  NodeLaunch& add(int kind, int stream, int grid, size_t lds) { NodeLaunch& L = grid > 0 ? l[n++] : none; L = NodeLaunch{kind, stream, grid, (int)lds}; return L; }
};
struct PlanCaps { int oc_grid, ocb_grid, probe_grid, ipm_grid_max; bool concurrent_big, as_on, stream2, stream3, stream4, ctr; };   // of the context: capacities, and which streams and counter sets exist
struct PlanSwitches { int big_grid_cap; double big_w1, big_w2; bool big_pad; int as_chunk, as_quota; };

// Which node kernels run in a round, where and on what: a pure function (no HIP call, no environment).  cls_n: lengths of the round's class lists, [0] < 0: not known
RoundPlan plan_node_launches(const Layout& Y, const PlanCaps& X, const PlanSwitches& S, const int* cls_n, int bc, bool overlap, int par) {
  RoundPlan P;
  const size_t l_ipm = ipm_lds_bytes(Y);
  // ---- no on-chip kernel for the shape: the memory-backed kernel on everything
  if (X.oc_grid <= 0) { P.add(NK_IPM, 0, std::min(bc, X.ipm_grid_max), l_ipm).zero = Z_WORK; return P; }
  const size_t l_oc = (size_t)oc_lds_layout(Y.N, Y.fixlen).total, l_ocb = (size_t)oc_lds_layout(Y.N, Y.fixlen, OC_GCAP_BIG).total;
  const size_t l_ocb_as = as_shape_ok(Y.C, Y.N) && S.big_pad ? oc_big_lds_beside_as(Y) : l_ocb;
  const bool big = X.ocb_grid > 0, aside = overlap && X.probe_grid > 0 && X.stream2, conc = big && aside && X.concurrent_big, pc = par >= 0 && X.ctr && conc;
  if (pc) P.par = par;
  if (conc) {
    // ---- the concurrent round
    // Every round: the larger variant works beside the standard one, on its own stream, through the nodes known to be large
    // (rounding probes, marked records); behind it, on that stream, the memory-backed kernel takes what even it cannot hold.
    // Both kernels hand their nodes out dynamically, so the wavefronts of the standard launch that find no room at first start
    // as the large nodes finish: the tail of the large nodes (40+ iterations) hides behind the standard launch instead of
    // being a launch of its own.  A node the standard kernel finds too large at its decode is marked and returned unsolved
    // (bounce): no second launch behind the standard one.
    // Words of the parity set: [0] batch count, [1] standard launch, [2] its hand-over list, [3] the larger variant's list, [4] the larger variant, [5] the
    // memory-backed launch behind it, [6] the larger active-set launch.  Without the set (!pc) every launch has its counters zeroed by memsets; the
    // class lists come with the set, so a launch that takes a list never has one
    const int zw = pc ? 0 : Z_WORK;
    const int gb = std::min(std::min(bc, S.big_grid_cap), std::min(X.probe_grid, X.ocb_grid));
    const bool as2 = X.as_on && pc && X.stream3;   // (as_on: the shape has the launches - as_shape_ok - and the call has not switched them off)
    const bool lists = as2 && X.stream4 && cls_n[0] >= 0;
    // With the class lists the larger launches get the SHARE of the device their work is of the round's, not all of it: their wavefronts take a SIMD
    // each (450 / 424 registers) and are enqueued first - a full grid of them held every SIMD until the larger active-set launch was through
    // (5 of 16 ms, tools/wave_dump.py), the standard launch started behind them and never got its holes back.  Weights: SIMD time of a node of the
    // class in units of a standard node's (half a SIMD for ~0.19 ms)
    int g1s = gb, g2s = gb;
    if (lists && S.big_w1 > 0) {
      const double n1 = cls_n[0], n2 = cls_n[1], n0 = std::max(0, bc - cls_n[0] - cls_n[1] - cls_n[2]);
      const double den = S.big_w1 * n1 + S.big_w2 * n2 + n0 + 1.0;
      g1s = std::max(32, (int)(gb * S.big_w1 * n1 / den + 0.5)); g2s = std::max(32, (int)(gb * S.big_w2 * n2 / den + 0.5));
    }
    if (as2) {
      // the large nodes of the round that the active-set method takes (large_class 1): its larger block, on a third stream beside the interior
      // point chain, which keeps the rest of them.  (With the class lists: as many workgroups as the class has nodes, none when it is empty.)  Its
      // LDS is that of a block beside the standard active-set launch with and without the lists
      NodeLaunch& L = P.add(NK_AS_BIG, 3, lists ? std::min(std::min(gb, g1s), cls_n[0]) : gb, l_ocb_as);
      L.ovf_mode = 2; L.cls_take = lists ? 1 : 0; L.work = 6; L.bufs = BUF_SECOND;
    }
    { // the larger interior point variant, on the second stream; padded like the launch above only when it takes its class's list
      NodeLaunch& L = P.add(NK_OC_BIG, 2, lists ? std::min(std::min(gb, g2s), cls_n[1]) : gb, lists ? l_ocb_as : l_ocb);
      L.ovf_mode = 2; L.cls_take = lists ? 2 : 0; L.as_split = as2; L.work = pc ? 4 : -1; L.bufs = BUF_SECOND; L.zero = zw;
    }
    { // the memory-backed kernel on the larger variant's list: behind it on the second stream or, beside the larger active-set launch and where a
      // fourth stream exists, on that one - the records known to exceed the larger block, beside the three others (gain buffer of its own)
      const bool own = as2 && X.stream4;
      NodeLaunch& L = P.add(NK_IPM, own ? 4 : 2, lists ? std::min(X.probe_grid, cls_n[2]) : std::min(bc, X.probe_grid), l_ipm);
      L.ovf_mode = own ? 3 : 1; L.cls_take = lists ? 3 : 0; L.as_split = as2; L.from_ovf2 = 1; L.work = pc ? 5 : -1; L.bufs = own ? BUF_KGAIN3 : BUF_SECOND; L.zero = zw;
    }
    { // the ordinary nodes of the round: dual active-set solves (as_onchip.hip) in place of the standard interior point launch; a node that
      // launch cannot finish comes back marked, like a node that is too large, and the larger interior point variant takes it next round
      const bool as = X.as_on && pc; const int run = S.as_quota * std::max(1, S.as_chunk);   // (nodes a wavefront of the launch takes before it leaves; 0: it stays)
      NodeLaunch& L = as ? P.add(NK_AS, 0, run > 0 ? std::max(1, (bc + run - 1) / run) : std::min(bc, X.oc_grid), (size_t)oc_lds_layout(Y.N, Y.fixlen, OC_GCAP, true).total)
                         : P.add(NK_OC, 0, std::min(bc, X.oc_grid), l_oc);
      L.skip_probes = 1; L.bounce = 1; L.work = pc ? 1 : 0; L.zero = pc ? 0 : Z_WORK | Z_OVF;
    }
  } else {
    // ---- the serial chain (`overlap` false: the polish, solve_fixed, the fixed batch, the replays), with the probe overlap in front of it in a round
    // The rounding probes of the batch (every disjunction fixed: >= 480 general rows, always beyond the on-chip capacity) are known
    // before the launch - their depth word says so - and go to a launch of their own on a SECOND stream that runs
    // beside the on-chip kernel: that kernel waits on memory for most of its cycles (58 % in s_waitcnt), the on-chip kernel is bound
    // by VALU issue, and the probes no longer cost a generation of their own behind it.
    const bool ov = aside && bc <= 4096;   // (a full batch keeps the device busy on its own: measured no gain there, 5.4 against 5.1 s on a 2048-instance queue; single solves: median 6.0 instead of 7.0 ms)
    if (ov) {
      NodeLaunch& L = big ? P.add(NK_OC_BIG, 2, std::min(bc, std::min(X.probe_grid, X.ocb_grid)), l_ocb) : P.add(NK_IPM, 2, std::min(bc, X.probe_grid), l_ipm);
      L.ovf_mode = 2; L.work = -1; L.bufs = BUF_SECOND; L.zero = Z_WORK;
    }
    { NodeLaunch& L = P.add(NK_OC, 0, std::min(bc, X.oc_grid), l_oc); L.skip_probes = ov; L.zero = Z_WORK | Z_OVF; }
    // the nodes the standard variant could not hold go to the larger one (up to OC_GCAP_BIG general rows: the rounding probes
    // without their slack front-point rows, the other large nodes); what even that one cannot hold - the polish of an
    // incumbent, every row of it - to the memory-backed kernel
    if (big) { NodeLaunch& L = P.add(NK_OC_BIG, 0, std::min(bc, X.ocb_grid), l_ocb); L.ovf_mode = 1; L.zero = Z_WORK; }
    { NodeLaunch& L = P.add(NK_IPM, 0, std::min(bc, X.ipm_grid_max), l_ipm); L.ovf_mode = 1; L.from_ovf2 = big; L.zero = Z_WORK; }   // blocks without a node read the count and leave
  }
  if (big && !pc && P.n > 0) P.l[0].zero |= Z_OVF2;
  return P;
}

// Issues a plan: every launch starts from the caller's B and gets its own fields, nothing of another launch's.  A stream beside the caller's waits for the
// fork event before its first launch and records its join event behind its last one; the caller's stream waits for those behind the standard
// launch (the launches below it in a serial chain and the evaluation need the results)
void run_node_launches(DevCtx& X, const DevBuf& B, const RoundPlan& P, hipStream_t st, hipEvent_t ev_std_end) {
  const hipStream_t stream[5] = {st, nullptr, X.stream2, X.stream3, X.stream4};
  const hipEvent_t join[5] = {nullptr, nullptr, X.ev_join, X.ev_join3, X.ev_join4};
  int* const cs = P.par >= 0 ? X.ctr + CTR_SET * P.par : nullptr;
  int last[5] = {-1, -1, -1, -1, -1};
  for (int i = 0; i < P.n; ++i) { last[P.l[i].stream] = i; if (P.l[i].zero & Z_OVF2) (void)hipMemsetAsync(B.ovf2_count, 0, 4, st); }
  if (last[2] >= 0 || last[3] >= 0 || last[4] >= 0) (void)hipEventRecord(X.ev_fork, st);
  for (int k = 2; k < 5; ++k) if (last[k] >= 0) (void)hipStreamWaitEvent(stream[k], X.ev_fork, 0);
  for (int i = 0; i < P.n; ++i) {
    const NodeLaunch& L = P.l[i]; const hipStream_t s = stream[L.stream];
    DevBuf Bl = B;
    Bl.ovf_mode = L.ovf_mode; Bl.cls_take = L.cls_take; Bl.as_split = L.as_split; Bl.skip_probes = L.skip_probes; Bl.bounce = L.bounce;
    if (cs) { Bl.ovf_count = cs + 2; Bl.ovf2_count = cs + 3; }
    Bl.work_counter = L.work > 0 ? cs + L.work : L.work < 0 ? X.work_counter2 : B.work_counter;
    if (L.from_ovf2) { Bl.ovf_count = Bl.ovf2_count; Bl.ovf_list = B.ovf2_list; }
    if (L.bufs != BUF_PRIMARY) { Bl.rowstate = X.rowstate2; Bl.rowcache = X.rowcache2; Bl.kgain = L.bufs == BUF_KGAIN3 ? X.kgain3 : X.kgain2; }
    if (L.zero & Z_WORK) (void)hipMemsetAsync(Bl.work_counter, 0, 4, s);
    if (L.zero & Z_OVF) (void)hipMemsetAsync(Bl.ovf_count, 0, 4, s);
    hipLaunchKernelGGL(NODE_KERNEL[L.kind][X.Y.C - 1], dim3(L.grid), dim3(L.kind == NK_IPM ? ipm_nt(X.Y.C) : 64), (size_t)L.lds, s, Bl);
    if (L.stream != 0 && last[L.stream] == i) (void)hipEventRecord(join[L.stream], s);
    if (L.kind == NK_OC || L.kind == NK_AS) {
      if (X.ev_mid) (void)hipEventRecord(X.ev_mid, st);       // (diagnostic, MIQP_LAUNCH_TRACE: where the standard launch ends)
      if (ev_std_end) (void)hipEventRecord(ev_std_end, st);   // (where the standard launch of the round ends: the dominant kernel's own time)
      for (int k = 2; k < 5; ++k) if (last[k] >= 0) (void)hipStreamWaitEvent(st, join[k], 0);
    }
  }
}

void launch_ipm_batch(DevCtx& X, const DevBuf& B, int bc, hipStream_t st, bool overlap = false, int par = -1, hipEvent_t ev_std_end = nullptr) {
  static const int unknown[3] = {-1, -1, -1};
  const ProcessSwitches& ps = process_switches();
  const PlanCaps caps = {X.oc_grid, X.ocb_grid, X.probe_grid, X.ipm_grid_max, X.concurrent_big, X.as_on, X.stream2 != nullptr, X.stream3 != nullptr, X.stream4 != nullptr, X.ctr != nullptr};
  const PlanSwitches sw = {ps.big_grid_cap, ps.big_w1, ps.big_w2, X.sw.big_pad, B.as_chunk, B.as_quota};
  run_node_launches(X, B, plan_node_launches(X.Y, caps, sw, B.cls_list ? X.cls_n : unknown, bc, overlap, par), st, ev_std_end);
}

void launch_eval_c(int C, const DevBuf& B, int nblocks, size_t lds, hipStream_t st) {
  switch (C) { case 1: launch_eval<1>(B, nblocks, lds, st); break; case 2: launch_eval<2>(B, nblocks, lds, st); break;
               case 3: launch_eval<3>(B, nblocks, lds, st); break; default: launch_eval<4>(B, nblocks, lds, st); }
}

bool set_kernel_lds(const Layout& Y, size_t ipm_lds, size_t eval_lds) {
  const auto set = [](NodeKernelFn k, size_t lds) { HIP_OK(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); return true; };
  if (Y.C <= 2 && Y.N <= 2 * OC_NSL) {
    const size_t l = (size_t)oc_lds_layout(Y.N, Y.fixlen).total, lb = std::max((size_t)oc_lds_layout(Y.N, Y.fixlen, OC_GCAP_BIG).total, as_shape_ok(Y.C, Y.N) ? oc_big_lds_beside_as(Y) : (size_t)0);
    if (l <= 160 * 1024) for (int k = NK_AS_BIG; k <= NK_OC; ++k) if (!set(NODE_KERNEL[k][Y.C - 1], k == NK_OC_BIG || k == NK_AS_BIG ? lb : l)) return false;
  }
  const NodeKernelFn eval[4] = {eval_kernel<1>, eval_kernel<2>, eval_kernel<3>, eval_kernel<4>};
  return set(NODE_KERNEL[NK_IPM][std::min(Y.C, 4) - 1], ipm_lds) && set(eval[std::min(Y.C, 4) - 1], eval_lds);
}

// ---------------------------------------------------------------- results (collectRawResults, cplex_wrapper.cpp:311-448)
// canonical binaries: 0 wherever the asserted side holds for the returned continuous point
void fill_results(const HostInst& I, const Layout& Y, const double* D, const int* T, const signed char* comp, const double* Z,
                  miqp_raw_results_c* r) {
  HostGeo G{I, Y, D, T};
  const int C = I.C, N = I.N, R = I.R, E = I.E, O = I.O, L = I.L, K = I.C - 1, nz = Y.nz;
  const double tol = 10 * FEAS_TOL;
  r->N = N; r->NrEnvironments = E; r->NrRegions = R; r->NrObstacles = O; r->MaxLinesObstacles = L; r->NrCarToCarCollisions = K; r->NrCars = C;
  for (int c = 0; c < C; ++c)
    for (int i = 0; i < N; ++i) {
      const double* z = Z + (size_t)i * nz; int qi = c * N + i;
      r->pos_x[qi] = z[6 * c]; r->vel_x[qi] = z[6 * c + 1]; r->acc_x[qi] = z[6 * c + 2];
      r->pos_y[qi] = z[6 * c + 3]; r->vel_y[qi] = z[6 * c + 4]; r->acc_y[qi] = z[6 * c + 5];
      r->u_x[qi] = z[6 * C + 2 * c]; r->u_y[qi] = z[6 * C + 2 * c + 1];
      int code = i >= 1 ? (int)comp[Y.f_reg + c * N + i] : -1;
      int q = i >= 1 ? (code >> 2) : 0;
      int j = i >= 1 ? T[Y.i_regj + c * Y.P + q] : I.init_region[c] - 1;
      double X, Yc;
      G.point(c, i, q, z, PT_U, PT_U, X, Yc); r->pos_x_front_UB[qi] = X; r->pos_y_front_UB[qi] = Yc;
      G.point(c, i, q, z, PT_L, PT_L, X, Yc); r->pos_x_front_LB[qi] = X; r->pos_y_front_LB[qi] = Yc;
      for (int jj = 0; jj < R; ++jj) r->active_region[(c * N + i) * R + jj] = jj == j ? 1 : 0;
      int xp = 0, yp = 0, xn = 0, yn = 0, cb = 0;
      if (i >= 1) {
        double vx = z[6 * c + 1], vy = z[6 * c + 4];
        xp = vx <= I.vm; xn = vx >= -I.vm; yp = vy <= I.vm; yn = vy >= -I.vm;
        int h = code & 3;
        if (h == 3) { xp = xn = yp = yn = cb = 1; }
        else {
          const int* hs = T + Y.i_hs + ((c * Y.P + q) * 2 + h) * 2;
          if (hs[0] == 0 && hs[1] > 0) xp = 0;
          if (hs[0] == 0 && hs[1] < 0) xn = 0;
          if (hs[0] == 1 && hs[1] > 0) yp = 0;
          if (hs[0] == 1 && hs[1] < 0) yn = 0;
        }
      }
      r->region_change_not_allowed_x_positive[qi] = xp; r->region_change_not_allowed_y_positive[qi] = yp;
      r->region_change_not_allowed_x_negative[qi] = xn; r->region_change_not_allowed_y_negative[qi] = yn;
      r->region_change_not_allowed_combined[qi] = cb;
      int* nw[5] = {r->notWithinEnvironmentRear, r->notWithinEnvironmentFrontUbUb, r->notWithinEnvironmentFrontLbUb,
                    r->notWithinEnvironmentFrontUbLb, r->notWithinEnvironmentFrontLbLb};
      for (int pt = 0; pt < 5; ++pt) {
        G.point(c, i, q, z, ENV_PT_H[pt][0], ENV_PT_H[pt][1], X, Yc);
        for (int e = 0; e < E; ++e) nw[pt][(c * E + e) * N + i] = G.env_viol(e, X, Yc) <= tol ? 0 : 1;
      }
      for (int o = 0; o < O; ++o)
        for (int pt = 0; pt < 5; ++pt) {
          bool ignored = i >= 1 && comp[Y.f_obs + ((c * O + o) * N + i) * 5 + pt] >= L;
          G.point(c, i, q, z, OBS_PT_H[pt][0], OBS_PT_H[pt][1], X, Yc);
          // a point that STARTS inside a soft obstacle is ignored by the constant step 0: the record says so, or it breaks the cardinality row of the
          // raw model at step 0.  The predicate is step0_check's own (no edge holds within FEAS_TOL), so the slack entry is 1 exactly where that charged the price
          if (i == 0 && I.obs_soft[o]) {
            double X0, Y0; G.point(c, 0, 0, nullptr, OBS_PT_H[pt][0], OBS_PT_H[pt][1], X0, Y0);   // (the initial state, as step0_check reads it)
            bool any = false; for (int k = 0; k < L && !any; ++k) any = G.obs_viol(o, 0, k, X0, Y0) <= FEAS_TOL;
            ignored = !any;
          }
          for (int k = 0; k < L; ++k) {
            int d = (G.obs_viol(o, i, k, X, Yc) <= tol && !ignored) ? 0 : 1;
            if (pt == 0) r->deltacc[((c * O + o) * N + i) * L + k] = d; else r->deltacc_front[(((c * O + o) * N + i) * L + k) * 4 + pt - 1] = d;
          }
          if (pt == 0) r->slackvarsObstacle[(c * O + o) * N + i] = ignored ? 1 : 0; else r->slackvarsObstacle_front[((c * O + o) * N + i) * 4 + pt - 1] = ignored ? 1 : 0;
        }
    }
  for (int a = 0; a < K * K * N * 16; ++a) r->car2car_collision[a] = 0;
  for (int a = 0; a < K * K * N * 4; ++a) { r->slackvars[a] = 0; if (r->slackvars_real) r->slackvars_real[a] = 0; }
  int p = 0;
  for (int c1 = 0; c1 < C; ++c1)
    for (int c2 = c1 + 1; c2 < C; ++c2, ++p)
      for (int i = 0; i < N; ++i) {
        const double* z = Z + (size_t)i * nz;
        int q1 = i >= 1 ? (comp[Y.f_reg + c1 * N + i] >> 2) : 0, q2 = i >= 1 ? (comp[Y.f_reg + c2 * N + i] >> 2) : 0;
        for (int g = 0; g < 4; ++g) {
          double vals[4]; for (int a = 0; a < 4; ++a) vals[a] = G.c2c_viol(p, c1, c2, i, g, a, q1, q2, z);
          int chosen = i >= 1 ? (int)comp[Y.f_c2c + (p * N + i) * 4 + g] : -1;
          if (chosen < 0) { chosen = 0; for (int a = 1; a < 4; ++a) if (vals[a] < vals[chosen]) chosen = a; }
          double sl[2] = {0, 0};
          if ((g == 0 || g == 3) && vals[chosen] > 0) sl[chosen < 2 ? 0 : 1] = vals[chosen];
          for (int a = 0; a < 4; ++a) {
            double need = vals[a] - ((g == 0 || g == 3) ? sl[a < 2 ? 0 : 1] : 0.0);
            r->car2car_collision[((c1 * K + (c2 - 1)) * N + i) * 16 + 4 * g + a] = (a == chosen || need <= tol) ? 0 : 1;
          }
          if (g == 0 || g == 3)
            for (int s = 0; s < 2; ++s) {
              int idx = ((c1 * K + (c2 - 1)) * N + i) * 4 + (g == 0 ? 0 : 2) + s;
              r->slackvars[idx] = (int)sl[s];  // truncation to int as in RawResults (miqp_planner_data.hpp:84-88)
              if (r->slackvars_real) r->slackvars_real[idx] = sl[s];
            }
        }
      }
}

// fix record from a complete assignment (warm start / solve_fixed): first asserted alternative of each disjunction
bool fix_from_results(const HostInst& I, const Layout& Y, const int* T, const miqp_raw_results_c* f, std::vector<signed char>& fix) {
  const int C = I.C, N = I.N, R = I.R, E = I.E, O = I.O, L = I.L, K = I.C - 1;
  fix.assign(Y.fixlen, -1);
  for (int c = 0; c < C; ++c)
    for (int i = 1; i < N; ++i) {
      int j = -1; for (int jj = 0; jj < R; ++jj) if (f->active_region[(c * N + i) * R + jj] == 1) j = jj;
      int q = -1; for (int k = 0; k < T[Y.i_nposs + c]; ++k) if (T[Y.i_regj + c * Y.P + k] == j) q = k;
      // a step without a (possible) active region stays undecided: the start is then a partial assignment that the
      // search completes (CPLEX repairs / completes partial MIP starts; the shifted receding-horizon start has an
      // all-zero last region row, src/miqp_planner.cpp:982)
      if (q >= 0) {
        int h = 3;
        if (f->region_change_not_allowed_combined[c * N + i] != 1) {
          h = 0;
          for (int k = 0; k < T[Y.i_nhs + c * Y.P + q]; ++k) {
            const int* hs = T + Y.i_hs + ((c * Y.P + q) * 2 + k) * 2;
            int b = hs[0] == 0 ? (hs[1] > 0 ? f->region_change_not_allowed_x_positive[c * N + i] : f->region_change_not_allowed_x_negative[c * N + i])
                               : (hs[1] > 0 ? f->region_change_not_allowed_y_positive[c * N + i] : f->region_change_not_allowed_y_negative[c * N + i]);
            if (b == 0) { h = k; break; }
          }
        }
        fix[Y.f_reg + c * N + i] = (signed char)(q * 4 + h);
      }
      const int* nw[5] = {f->notWithinEnvironmentRear, f->notWithinEnvironmentFrontUbUb, f->notWithinEnvironmentFrontLbUb,
                          f->notWithinEnvironmentFrontUbLb, f->notWithinEnvironmentFrontLbLb};
      for (int pt = 0; pt < 5; ++pt) {
        for (int e = 0; e < E; ++e) if (nw[pt][(c * E + e) * N + i] == 0) { fix[Y.f_env + (c * N + i) * 5 + pt] = (signed char)e; break; }
        for (int o = 0; o < O; ++o) {
          int so = pt == 0 ? f->slackvarsObstacle[(c * O + o) * N + i] : f->slackvarsObstacle_front[((c * O + o) * N + i) * 4 + pt - 1];
          if (so >= 1 && I.obs_soft[o]) { fix[Y.f_obs + ((c * O + o) * N + i) * 5 + pt] = (signed char)L; continue; }
          for (int k = 0; k < L; ++k) {
            int d = pt == 0 ? f->deltacc[((c * O + o) * N + i) * L + k] : f->deltacc_front[(((c * O + o) * N + i) * L + k) * 4 + pt - 1];
            if (d == 0) { fix[Y.f_obs + ((c * O + o) * N + i) * 5 + pt] = (signed char)k; break; }
          }
        }
      }
    }
  int p = 0;
  for (int c1 = 0; c1 < C; ++c1)
    for (int c2 = c1 + 1; c2 < C; ++c2, ++p)
      for (int i = 1; i < N; ++i)
        for (int g = 0; g < 4; ++g)
          for (int a = 0; a < 4; ++a)
            if (f->car2car_collision[((c1 * K + (c2 - 1)) * N + i) * 16 + 4 * g + a] == 0) { fix[Y.f_c2c + (p * N + i) * 4 + g] = (signed char)a; break; }
  return true;
}

struct BatchShape { Layout Y; bool ok; std::string err; };

BatchShape batch_layout(miqp_solver_t* const* S, int n) {
  BatchShape bs; bs.ok = false;
  const HostInst& I0 = S[0]->inst;
  int P = 1, EL = 0;
  for (int k = 0; k < n; ++k) {
    if (!S[k] || !S[k]->has_inst) { bs.err = "solver without parameters"; return bs; }
    const HostInst& I = S[k]->inst;
    if (I.C != I0.C || I.N != I0.N || I.O != I0.O || I.L != I0.L || I.E != I0.E || I.R != I0.R) { bs.err = "instances of one batch must share NumCars, NumSteps, nr_regions, nr_environments, nr_obstacles, max_lines_obstacles"; return bs; }
    P = std::max(P, max_possible(I)); EL = std::max(EL, max_env_edges(I));
  }
  if (I0.C > MAXC) { bs.err = "NumCars > 4 is not supported by the device kernels"; return bs; }
  if (P > 15) { bs.err = "more than 15 possible regions per car"; return bs; }
  // one branching creates a child per alternative of the chosen disjunction, at most 63 per node (eval_kernel): a shape
  // with more alternatives is refused instead of searched incompletely
  if (I0.E > 62 || I0.L + 1 > 62) { bs.err = "more than 62 environment pieces / 61 obstacle edges"; return bs; }
  bs.Y = make_layout(I0.C, I0.N, I0.R, P, I0.E, EL, I0.O, I0.L); bs.ok = true;
  return bs;
}

unsigned long long host_d2key(double v) { unsigned long long u; std::memcpy(&u, &v, 8); return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull); }
double host_key2d(unsigned long long k) { unsigned long long u = (k & 0x8000000000000000ull) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k; double v; std::memcpy(&v, &u, 8); return v; }

double wall_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// ---------------------------------------------------------------- the batch solve
// Tree split of ONE instance over the ranks of a job.  The alternatives of one or two car/car
// disjunctions partition the tree (every rank starts from the roots it owns); once per round the ranks exchange
// {incumbent | owner rank, lower bound, done, time-up} by an all-reduce(min) of four 64-bit words - the best incumbent prunes
// on every rank - and at the end the owner broadcasts the solution.
struct SplitCtx { int world, rank; miqp_exchange_fn fn; void* user; };
constexpr int SPLIT_MAXROOTS = 64;

// root records of the split: the cartesian product of the allowed alternatives of the rear/rear group of every car pair at
// the last step, then at the middle step, until there are at least 4 combinations per rank (at most SPLIT_MAXROOTS)
void split_roots(const Layout& Y, const int* T, std::vector<std::vector<std::pair<int, int>>>& combos, int world) {
  combos.assign(1, {});
  if (Y.C < 2) return;   // a single car has no car/car disjunction: rank 0 keeps the whole tree
  const int steps[2] = {Y.N - 1, (Y.N - 1) / 2};
  for (int si = 0; si < 2; ++si) {
    const int i = steps[si];
    if (i < 1 || (si == 1 && i == steps[0])) continue;
    for (int p = 0; p < Y.NP; ++p) {
      if ((int)combos.size() >= 4 * world) return;
      const int am0 = T[Y.i_c2callow + p * Y.N + i] & 15, am = am0 ? am0 : 15;
      int na = 0; for (int a = 0; a < 4; ++a) na += (am >> a) & 1;
      if (na < 2 || (int)combos.size() * na > SPLIT_MAXROOTS) continue;
      std::vector<std::vector<std::pair<int, int>>> next;
      for (auto& c : combos) for (int a = 0; a < 4; ++a) if ((am >> a) & 1) { auto d = c; d.emplace_back(Y.f_c2c + (p * Y.N + i) * 4 + 0, a); next.push_back(std::move(d)); }
      combos.swap(next);
    }
  }
}

#include "solve_diag.hpp"

// solution pool (solution_pool.hip): the capture launches behind a round's evaluation, `bc` nodes wide
bool pool_capture(DevCtx& X, int bc);
// starts from the carried pool (pool_carry.hip, pool_improve.hip): the range check of a decision record
bool decisions_in_range(const HostInst& I, const Layout& Y, const int* T, const signed char* d);

// ---------------------------------------------------------------- the batch solve: shape of the call
// `inflight`: instances solved concurrently (<= 0 or >= n: all of them).  With fewer than n the call is a queue drained by
// streaming admission: an instance that is proven (or has used up its own max_solution_time, counted from its admission)
// hands its slot to the next one at the following round.
// `lane` / `lanes`: this call is one of `lanes` concurrent calls that share the device, each with its own context (miqp_solver_solve_stream)
struct CallShape {
  int n, NS, lanes;          // instances, slots = instances in flight, lanes that share the device
  int npr, open_cap, MAXR;   // nodes per instance and round, near-list capacity asked for, root records per instance
  int starts;                // of MAXR: the room for start roots from a carried pool - the largest max_starts setting (miqp_solver_set_pool_starts) among the handles that offer any, 0 in a call without such a handle
  bool adaptive_width; int width0, width_max;   // a single solve starts at width0 nodes per round and widens up to width_max
  bool queue_mode, clamp_open;
};
// pure: the layout, the options, the sizes of the call and the switches in, the shape out.  Precedence: opts.nodes_per_round > MIQP_NPR > the rules
CallShape plan_call(const Layout& Y, const miqp_solver_opts& O0, int n, int inflight, int lanes, bool split, const CallSwitches& sw, int starts = 0) {
  CallShape sh{};
  sh.n = n; sh.lanes = lanes;
  const int NS = sh.NS = (split || inflight <= 0 || inflight >= n) ? n : inflight;   // slots = instances in flight
  // nodes of a round, all instances together: 32768 for three and four cars (and one), 98304 for two - since the node relaxations of two cars are active-set
  // solves (round 6) a round of 32768 lasts 5-6 ms of which 1.1 ms are the serial kernels and the tail of the launch; the driver's stream at 32 k / 49 k / 65 k /
  // 97 k / 131 k / 164 k nodes per round: 1783 / 1849 / 1864 / 1911 / 1856 / 1826 solves/s (time to a proof p50 0.043 -> 0.106 s, p99 7.4 -> 4.3 s at 97 k)
  const int round_nodes = Y.C == 2 ? 98304 : 32768;
  const bool rules = O0.nodes_per_round <= 0;
  int npr = !rules ? O0.nodes_per_round : std::max(16, std::min(16384, round_nodes / (NS * lanes)));   // (the lanes of a call keep the round width of the undivided call)
  // three and four cars: a node relaxation costs ~15 x that of two cars (memory-backed kernel, stage vector 24 / 32), a round of 32768 nodes
  // lasts 0.13 s and an instance that shares the device gets 80 rounds in its 10 s - fewer than the levels of its first dive.  Rounds of
  // 5120 nodes (0.035 s) give the tree its depth back at a quarter less node throughput: cfg5, 16 in flight, 7 -> 11 of 16 proven in 10 s.
  // Since the re-rounding finds the first incumbents within a few rounds the depth matters less and the throughput more: 8192 nodes
  // (3072 / 5120 / 8192 / 10240 / 12288 / 16384: 14 / 14 / 15 / 14 / 14 / 14 of 16, the open gaps smallest at 8192 - 12288; profiles/r04b_heuristics_ab.txt)
  if (rules && Y.C >= 3 && NS > 1) npr = std::max(16, std::min(npr, 8192 / NS));
  // ... and a single solve of three or four cars takes 2048 nodes per round (16384 / 8192 / 4096 / 2048: the sixteen cfg5 seeds in 35.1 / 34.3 / 29.5 / 25.3 s, 15 proven each time;
  // seed 15 8.5 -> 4.5 s): its rounds are as long as their slowest node whatever their width (~25 ms), so what a narrower round gives up is node throughput it could not use for the proof anyway
  if (rules && Y.C >= 3 && NS == 1) npr = std::min(npr, 2048);
  // ... and so does a single solve of one or two cars (round 5): 2048 nodes are one per resident wavefront of the standard on-chip launch (256 CUs x 8) - a
  // wider round lasts longer (several nodes per wavefront) and solves nodes that the incumbents of a narrower round would have pruned.  Measured on seeds 0-95
  // (tools/single_latency.py, profiles/r05_single_latency.txt), 16384 -> 2048 nodes per round: p99 58 -> 47 ms at gap 0.1 (seed 62: 55 k -> 26 k node
  // relaxations), 92 -> 75 ms at 0.01; p50 / p90 unchanged (5 / 18 ms); 1024: 51 / 76 ms (too narrow: more rounds), 4096: 51 / 86, 8192: 58 / 90
  if (rules && Y.C <= 2 && NS == 1) npr = std::min(npr, 2048);
  if (rules && sw.npr > 0) npr = sw.npr;
  // A single solve starts narrow (above) and WIDENS its rounds once it is bound-limited: the incumbent has not moved for 32 rounds and the
  // near list offers eight rounds' worth of eligible nodes - then the tree needs node throughput, not fresher incumbents (cfg5 seed 11: 1.61 / 2.17 / 2.92 M relaxations in 10 s at
  // 1024 / 2048 / 4096 nodes per round).  The batch arrays are sized for the widest round, select_kernel caps at width_cap
  sh.adaptive_width = NS == 1 && !split && rules && sw.npr <= 0;
  sh.width0 = npr; sh.width_max = Y.C >= 3 ? 4096 : 16384;   // (three and four cars: 4096 - cfg5 seed 11 relaxes 2.57 / 3.21 / 3.09 / 2.96 M nodes in its 10 s at 2048 / 4096 / 8192 / 16384, its gap 2.1 / 1.8 / 3.4 / 45 %)
  if (sh.adaptive_width) npr = sh.width_max;
  int open_cap = O0.max_open_nodes > 0 ? O0.max_open_nodes : (sw.open_cap > 0 ? sw.open_cap : std::max(1 << 17, std::min(1 << 20, (1 << 28) / NS)));   // near lists: 1 M entries per instance up to n = 256 (10 GB of list entries), 262144 at n = 1024; records are shared
  if (open_cap < 64) open_cap = 64;
  if (split && open_cap < SPLIT_MAXROOTS + 4 + 64) open_cap = SPLIT_MAXROOTS + 4 + 64;   // the root records of a tree split are the head of the list
  // (list entries - 40 B per open node - must fit an eighth of the free device memory: ctx_prepare cuts the capacity when it builds the context)
  if ((size_t)NS * npr >= ((size_t)1 << 20)) npr = (int)((((size_t)1 << 20) - 1) / NS);
  sh.npr = npr; sh.open_cap = open_cap;
  sh.starts = split ? 0 : starts;
  sh.MAXR = (split ? SPLIT_MAXROOTS + 4 : 5) + sh.starts;   // root records per instance: the root (or this rank's roots of a tree split), the MIP starts and their repair roots, the starts from a carried pool
  sh.queue_mode = NS < n; sh.clamp_open = O0.max_open_nodes <= 0;
  return sh;
}

// ---------------------------------------------------------------- host tables, step-1 presolve, root records
struct HostTables {
  // (not value-initialised: compile_instance writes every word of an instance's slice, and zeroing 1.4 GB for the 51 200 instances of the driver's stream
  // on the calling thread came before the threads below could start)
  std::unique_ptr<double[]> D; std::unique_ptr<int[]> T; size_t nD = 0, nT = 0;
  std::vector<double> h_const, h_gap, h_tlim;
  std::vector<int> h_done;              // 1: never starts (infeasible first step, no root on this rank)
  std::vector<signed char> roots;       // fix records of all roots, in the order of their record numbers
  std::vector<int> on, od, oc; int nrec = 0;   // root records of every instance (record, depth word; count): the head of its open list at admission
  std::vector<unsigned char> big;       // size marks of the first big.size() root records (empty without starts from a carried pool: every root starts unmarked)
};

// per instance (independent, spread over host threads): tables, step-0 check, the fix records of its roots, the raw model sizes
void prepare_instances(miqp_solver_t* const* S, const Layout& Y, const CallShape& sh, const SplitCtx* split, HostTables& H) {
  const int n = sh.n, MAXR = sh.MAXR, WS_MAX = sh.MAXR - sh.starts;   // (the two warm-start slots and their repair roots share the records in front of the pool starts: today's 5)
  H.nD = (size_t)n * Y.dstride; H.nT = (size_t)n * Y.istride;
  H.D.reset(new double[H.nD]); H.T.reset(new int[H.nT]);
  double* const hD = H.D.get(); int* const hT = H.T.get();
  H.h_const.assign(n, 0.0); H.h_gap.resize(n); H.h_tlim.resize(n); H.h_done.assign(n, 0);
  H.on.assign((size_t)n * MAXR, 0); H.od.assign((size_t)n * MAXR, 0); H.oc.assign(n, 0);
  std::vector<std::vector<std::vector<signed char>>> inst_roots(n);
  std::vector<std::vector<int>> inst_root_depth(n);
  std::vector<char> h_feas0(n, 0);
  auto prepare_one = [&](int k) {
    miqp_solver* s = S[k]; s->lay = Y; s->has_sol = false; s->pool_carried = false; s->rescache.reset();
    compile_instance(s->inst, Y, &hD[(size_t)k * Y.dstride], &hT[(size_t)k * Y.istride]);
    HostGeo G{s->inst, Y, &hD[(size_t)k * Y.dstride], &hT[(size_t)k * Y.istride]};
    double cobj = 0; bool feas0 = step0_check(G, cobj);
    H.h_const[k] = cobj; H.h_gap[k] = s->opts.gap_override >= 0 ? s->opts.gap_override : s->inst.gap; H.h_tlim[k] = s->inst.tilim;
    h_feas0[k] = feas0 ? 1 : 0;
    auto& R = inst_roots[k];
    if (feas0 && !split) R.emplace_back(Y.fixlen, (signed char)-1);
    else if (feas0) {
      std::vector<std::vector<std::pair<int, int>>> combos; split_roots(Y, &hT[(size_t)k * Y.istride], combos, split->world);
      for (size_t q = 0; q < combos.size(); ++q) {
        if ((int)(q % (size_t)split->world) != split->rank) continue;
        std::vector<signed char> fx(Y.fixlen, (signed char)-1);
        for (auto& d : combos[q]) fx[d.first] = (signed char)d.second;
        R.push_back(std::move(fx));
      }
    }
    // MIP starts (initializeWarmstart + addMIPStart / readMIPStarts, src/cplex_wrapper.cpp:124-138, 494-639): the binaries
    // of each start become an additional root whose QP the first round solves; a feasible one is the first incumbent
    for (int w = 0; w < 2 && feas0; ++w) {
      if (!s->ws[w] || !dims_match(s->ws[w]->r, s->inst)) continue;
      std::vector<signed char> fx;
      if (!fix_from_results(s->inst, Y, &hT[(size_t)k * Y.istride], &s->ws[w]->r, fx)) continue;
      // repair root of the start (CPLEX: repairtries): its region binaries alone; the search completes the rest by rounding
      std::vector<signed char> rx(Y.fixlen, (signed char)-1);
      bool any_reg = false;
      for (int q = Y.f_reg; q < Y.f_reg + Y.C * Y.N; ++q) { rx[q] = fx[q]; any_reg = any_reg || fx[q] >= 0; }
      if ((int)R.size() < WS_MAX) R.push_back(std::move(fx));
      if (any_reg && (int)R.size() < WS_MAX) { R.push_back(std::move(rx)); inst_root_depth[k].resize(R.size(), 0); inst_root_depth[k].back() = REPAIR_ROOT; }
    }
    // starts from the carried pool (miqp_solver_set_pool_starts; the counterpart of a CPLEX user re-adding the old pool's members as MIP starts): the
    // records the call took from the handle's pool before it dropped it, each completed as miqp_solver_solve_decisions completes decision bytes - the
    // bytes behind them "none" -, depth word 0, no repair root.  Nodes of round 1 like the starts above: a feasible one is a candidate of the capture
    // and, the best of them, the first incumbent.  A record with a byte outside its site's alternatives (a carry never admits one) and the handle takes none
    s->st_n = 0;
    if (feas0 && !split && s->st_offer > 0 && s->st_fixlen == Y.fixlen) {
      bool ok = (int)R.size() + s->st_offer <= MAXR && s->st_fix.size() >= (size_t)s->st_offer * Y.fixlen;
      for (int q = 0; q < s->st_offer && ok; ++q) ok = decisions_in_range(s->inst, Y, &hT[(size_t)k * Y.istride], s->st_fix.data() + (size_t)q * Y.fixlen);
      for (int q = 0; q < s->st_offer && ok; ++q) {
        std::vector<signed char> fx(Y.fixlen, (signed char)-1);
        std::memcpy(fx.data(), s->st_fix.data() + (size_t)q * Y.fixlen, (size_t)Y.f_c2n);
        R.push_back(std::move(fx)); s->st_n++;
      }
    }
    inst_root_depth[k].resize(R.size(), 0);
    int rows, bin, cont, nnz; raw_sizes(s->inst, rows, bin, cont, nnz);
    s->props = miqp_solution_properties_c{}; s->props.NrConstraints = rows; s->props.NrBinaryVariables = bin; s->props.NrFloatVariables = cont;
    s->props.NonZeroCoefficients = nnz;
  };
  const int nth = std::max(1, std::min<int>({n / 8, (int)std::thread::hardware_concurrency(), process_switches().prep_threads}));
  if (nth <= 1) for (int k = 0; k < n; ++k) prepare_one(k);
  else {
    std::atomic<int> next{0}; std::vector<std::thread> th;
    for (int t = 0; t < nth; ++t) th.emplace_back([&] { for (int k = next.fetch_add(1); k < n; k = next.fetch_add(1)) prepare_one(k); });
    for (auto& t : th) t.join();
  }
  { size_t nroot = 0; for (int k = 0; k < n; ++k) nroot += inst_roots[k].size(); H.roots.reserve(nroot * Y.fixlen); }   // (by the counts: not MAXR records for each of a stream's 51 200 handles)
  for (int k = 0; k < n; ++k) {
    if (!h_feas0[k]) H.h_done[k] = 1;
    for (size_t q = 0; q < inst_roots[k].size(); ++q) {
      const auto& fx = inst_roots[k][q];
      // A start from the carried pool decides every disjunction: its relaxation has more general rows than either on-chip block holds (two cars, 20
      // steps: over 480 against the 270 - 290 of a tree node).  Unmarked, the standard block would hand it to the larger one and that one to the
      // memory-backed kernel, a round each - and from round 2 on a start meets the cutoff of round 1's incumbent and is dropped before it is a
      // candidate.  So its record starts with the size mark those two hand-overs would leave: round 1 relaxes it, without a cutoff
      if (q + (size_t)S[k]->st_n >= inst_roots[k].size()) { H.big.resize((size_t)H.nrec + 1, 0); H.big.back() = 2; }
      H.roots.insert(H.roots.end(), fx.begin(), fx.end()); H.on[(size_t)k * MAXR + H.oc[k]] = H.nrec++; H.od[(size_t)k * MAXR + H.oc[k]] = inst_root_depth[k][q]; H.oc[k]++;
    }
    if (H.oc[k] == 0) H.h_done[k] = 1;   // (a rank of a tree split may own no root)
  }
}

// every copy and reset that a call starts from: the tables and roots up, the per-instance and per-slot state of the context back to "nothing yet"
bool upload_and_reset(DevCtx& X, const HostTables& H, const CallShape& sh) {
  const DevBuf& B = X.B; const Layout& Y = X.Y; hipStream_t st = X.stream; const int n = sh.n, NS = sh.NS;
  HIP_OK(hipMemcpyAsync((void*)B.inst_d, H.D.get(), H.nD * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync((void*)B.inst_i, H.T.get(), H.nT * 4, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(B.pool_fix, H.roots.data(), H.roots.size(), hipMemcpyHostToDevice, st));
  const int pool0 = H.nrec;
  if (B.pool_big && H.nrec > 0) HIP_OK(hipMemsetAsync(B.pool_big, 0, (size_t)H.nrec, st));   // the root records start unmarked (children are marked or cleared when they are written)
  if (B.pool_big && !H.big.empty()) HIP_OK(hipMemcpyAsync(B.pool_big, H.big.data(), std::min(H.big.size(), (size_t)H.nrec), hipMemcpyHostToDevice, st));   // ... but the starts from a carried pool (prepare_instances)
  HIP_OK(hipMemcpyAsync(B.pool_count, &pool0, 4, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemsetAsync(B.free_head, 0, 4, st)); HIP_OK(hipMemsetAsync(B.free_tail, 0, 4, st)); HIP_OK(hipMemsetAsync(B.free_limit, 0, 4, st));
  HIP_OK(hipMemcpyAsync((void*)B.root_node, H.on.data(), H.on.size() * 4, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync((void*)B.root_depth, H.od.data(), H.od.size() * 4, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync((void*)B.root_cnt, H.oc.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemsetAsync(B.open_count, 0, (size_t)n * 4, st));
  HIP_OK(hipMemsetAsync(B.inst_slot, 0xFF, (size_t)n * 4, st)); HIP_OK(hipMemsetAsync(B.slot_inst, 0xFF, (size_t)NS * 4, st));
  HIP_OK(hipMemsetAsync(B.inst_kill, 0, (size_t)n * 4, st));
  HIP_OK(hipMemsetAsync(B.slot_demand, 0, (size_t)NS * 4, st));
  { std::vector<int> t0_(NS, sh.npr); HIP_OK(hipMemcpyAsync(B.slot_take, t0_.data(), (size_t)NS * 4, hipMemcpyHostToDevice, st)); HIP_OK(hipStreamSynchronize(st)); }
  HIP_OK(hipMemsetAsync(B.far_count, 0, (size_t)n * 4, st)); HIP_OK(hipMemsetAsync(B.far_minkey, 0xFF, (size_t)n * 8, st));
  HIP_OK(hipMemsetAsync(B.inst_mode, 0, (size_t)n * 4, st));
  HIP_OK(hipMemsetAsync(B.inc_key, 0xFF, (size_t)n * 8, st));
  HIP_OK(hipMemsetAsync(B.inc_seen, 0xFF, (size_t)n * 8, st));
  HIP_OK(hipMemsetAsync(B.inc_fix, 0xFF, (size_t)n * Y.fixlen, st));   // no incumbent yet: every disjunction undecided
  if (B.inc_Mtag) HIP_OK(hipMemsetAsync(B.inc_Mtag, 0, (size_t)n * 8, st));
  const std::vector<double> big(n, 1e300);
  HIP_OK(hipMemcpyAsync(B.inc_obj, big.data(), n * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(B.inc_ext, big.data(), n * 8, hipMemcpyHostToDevice, st)); HIP_OK(hipMemcpyAsync(B.near_thr, big.data(), n * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(B.lower_bound, big.data(), n * 8, hipMemcpyHostToDevice, st)); HIP_OK(hipStreamSynchronize(st));
  HIP_OK(hipMemcpyAsync(B.inst_done, H.h_done.data(), n * 4, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemsetAsync(B.inst_flags, 0, (size_t)n * 4, st));
  HIP_OK(hipMemcpyAsync(B.inst_gap, H.h_gap.data(), n * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(B.inst_const, H.h_const.data(), n * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemsetAsync(B.inst_nodes, 0, (size_t)n * 8, st));
  HIP_OK(hipMemsetAsync(B.inst_iters, 0, (size_t)n * 8, st));
  HIP_OK(hipMemsetAsync(B.inst_ninc, 0, (size_t)n * 4, st));
  HIP_OK(hipMemsetAsync(B.as_stats, 0, 256, st));
  HIP_OK(hipMemsetAsync(B.inst_lns, 0, (size_t)n * 4, st));
  HIP_OK(hipMemcpyAsync(B.inst_lns_obj, big.data(), (size_t)n * 8, hipMemcpyHostToDevice, st)); HIP_OK(hipStreamSynchronize(st));
  HIP_OK(hipMemsetAsync(B.active_insts, 0, 4, st));   // admit_kernel counts the instances in as they enter
  HIP_OK(hipMemsetAsync(B.stat_rowiters, 0, 8, st));
  HIP_OK(hipStreamSynchronize(st));
  return true;
}

// call lifetime: the search fields of DevBuf, read at every call (a context is reused by every later call of the same shape)
void apply_call_switches(DevCtx& X, const CallShape& sh, const CallSwitches& sw, const std::vector<double>& h_gap) {
  DevBuf& B = X.B; const Layout& Y = X.Y; const int NS = sh.NS;
  { double gmin = 1.0; for (double g : h_gap) gmin = std::min(gmin, g);
    const double ftol = knob_double(KNOB_T("MIQP_QPTOL_F"), 1e-4);   // (tuning knob)
    const double tolcap = knob_double(KNOB_T("MIQP_QPTOL"), QP_TOL);
    B.qp_tol = std::min(tolcap, std::max(1e-12, ftol * gmin)); }  // node relaxations: accurate to a small fraction of the MIP gap
  B.base_take = std::max(1, std::min(sh.npr, knob_int(KNOB_T("MIQP_BASE_TAKE"), 8)));
  // Batch shares (share_kernel).  A QUEUE (more instances than slots: admissions go on while the old instances run against their limits): half
  // of the batch is shared evenly as a floor, the rest goes by admission order up to 256 nodes per instance - an instance that waits for its
  // turn no longer crawls at 8 nodes per round (its tree then costs 3-4 x the nodes, tools/crowd_probe.py), and narrow shares cost the fewest
  // nodes in all; measured on the 12-step bench stream: 1010 -> 1160 solves/s, 99.57 -> 99.39 % proven, p95 6.9 -> 4.5 s (the whole curve:
  // profiles/r04_share_policy.txt).  ONE batch with every instance in flight from the start (cfg4's 256, cfg5's 16): all deadlines are the same and
  // serving a few instances to their end frees the device for the others - admission order up to 1024 each, no floor (cfg5: 11 of 16 proven against 5).
  B.share_cap = std::max(1, knob_int(KNOB_T("MIQP_SHARE_CAP"), sh.queue_mode ? 256 : 1024));
  B.floor_pct = std::max(0, std::min(100, knob_int(KNOB_T("MIQP_FLOOR_PCT"), sh.queue_mode ? 50 : 0)));
  B.lns_narrow = std::max(0, knob_int(KNOB_T("MIQP_LNS_NARROW"), 512));   // width of a round that carries local-search leaves (0: as wide as any)
  B.defer_cap = knob_int(KNOB_T("MIQP_DEFER"), Y.C >= 3 ? 24 : 0);   // (see ipm_kernel.  Measured on cfg5 at 0 / 16 / 20 / 24: seed 8 0.96 / 0.85 / 0.78 / 0.77 s, seed 14 0.75 / 0.67 / 0.65 / 0.66 s, seed 15 2.47 / 2.62 / 2.39 / 2.42 s, node relaxations in seed 11's 10 s 2.22 / 2.25 / 2.43 / 2.49 M, sixteen in flight 3.33 / 3.71 / 3.42 / 3.49 M.  Two cars (both on-chip variants have the same exit): OFF - the bench on 8 steps at 0 / 16 / 18 / 20 / 24 / 28: 1160 / 1174 / 1176-1182 / 1172 / 1156 / 1160 solves/s (the standard launch 10.0 -> 9.2 ms but 6 % more nodes per instance), single solves p99 46 -> 44 ms; and cfg3 seed 1913 - the pinned hard instance of test_local_search_changes_the_order_not_the_answer - 135 k -> 327 k nodes: a result that arrives a round late reorders the local search's chains)
  B.probe_itcap0 = knob_int(KNOB_T("MIQP_PROBE_ITCAP0"), Y.C >= 3 ? 0 : 40);   // (the cap while the instance has no incumbent)
  B.pump_max = std::max(0, std::min(15, knob_int(KNOB_P("MIQP_PUMP"), 6)));   // re-rounding of infeasible rounding probes (eval_kernel)
  B.pump_inc = knob_int(KNOB_T("MIQP_PUMP_INC"), Y.C >= 3 ? 1 : 0);   // re-rounding also with an incumbent (probes whose OBJECTIVE is below it): three and four cars - cfg5 seed 15 proven in 8 s, the gaps of the two seeds left at 10 s with 16 in flight 0.38 / 0.32 -> 0.09 / 0.03; two cars: the probes it lets converge are the critical path of a round (single-solve p99 62 -> 72 ms, queue -1 %)
  B.young_nodes = std::max(0, knob_int(KNOB_T("MIQP_YOUNG_NODES"), 0));
  B.probe_room = knob_double(KNOB_T("MIQP_PROBE_ROOM"), 0.0);
  B.live_inc = knob_int(KNOB_T("MIQP_LIVE_INC"), 0);
  B.probe_every = knob_int(KNOB_T("MIQP_PROBE_EVERY"), 1);
  B.probe_itcap = knob_int(KNOB_T("MIQP_PROBE_ITCAP"), Y.C >= 3 ? 0 : 24);   // (three and four cars: no cap - EVERY probe of the phase without incumbent hit it there, at 25 iterations: infeasible roundings take 36-48, and it is their least-violation solution that the re-rounding needs)   // (0: never; solved probes take 9-24 iterations; 40 until round 4: the heuristic nodes - probes, local-search leaves - are the critical path of a single solve's round: p99 99 -> 80 ms at 24)
  B.probe_margin = knob_double(KNOB_T("MIQP_PROBE_MARGIN"), 0.25);   // (0: every disjunction of a probe fixed, as in round 2)
  B.det_ties = knob_int(KNOB_T("MIQP_DET_TIES"), 1);
  B.window_pct = std::max(1, std::min(100, knob_int(KNOB_T("MIQP_WINDOW"), 100)));
  B.lns_warm = !knob_off(KNOB_T("MIQP_LNS_WARM"));
  B.lns_step = knob_double(KNOB_T("MIQP_LNS_STEP"), 0.0);
  B.cut_gate = knob_double(KNOB_P("MIQP_CUT_GATE"), 1.0e-5);
  B.seq_kinds = sw.seq_kinds;
  // a single solve sends its re-roundable rounding probes to the active-set launch first (the interior point - up to 40 iterations of 70 us on the
  // critical path of its round - only sees the ones that turn out infeasible, a round later): seeds 0-95 p50 5.0 -> 4.0 ms at gap 0.1, 5.7 -> 5.0 at
  // 0.01, p90 / p99 unchanged; a queue keeps the direct route (1898 against 1868 solves/s on the driver's stream)
  B.as_probe_first = knob_int(KNOB_T("MIQP_AS_PROBE_FIRST"), NS == 1 ? 1 : 0);
  X.as_on = X.as_cap && !knob_off(KNOB_P("MIQP_AS"));
  B.batch_A = X.as_on ? X.as_batch_A : nullptr; B.pool_A = X.as_on ? X.as_pool_A : nullptr;
  B.lns_mode = knob_int(KNOB_P("MIQP_LNS"), 45);
#ifndef MIQP_TUNING
  B.lns_mode &= 127;   // (bits 7-9: the neighbourhood sub-problems of round 4 - measured without effect, DESIGN.md 2b - exist in a tuning build only)
#endif
  B.lns_min_nodes = knob_int(KNOB_T("MIQP_LNS_MIN"), NS == 1 ? 500 : 2000);   // (a single solve: sooner - 90 % quantile of seeds 0-95 24 -> 19 ms; a queue at 500: 1 % slower)
  X.sw = sw;
}

// ---------------------------------------------------------------- the round loop
// Tree split of ONE instance: what the ranks agreed on at the last exchange
struct SplitState { double inc = 1e300, lb = -1e300; int owner = 0; bool timeup = false, finished = false; };

struct Rounds {
  DevCtx& X; const CallShape& sh; const HostTables& H; const SplitCtx* split; int verbose;
  DevBuf& B; hipStream_t st; const int n, NS;
  // streaming admission (host side): which instance holds which slot, when it entered, who is next
  std::vector<int> slot_inst, kill, pairs; std::vector<double> t_admit;
  std::vector<char> stalled;   // retired because it made no progress (not because its time was up)
  int next_q = 0, in_flight = 0, empty_rounds = 0;
  bool abandoned = false, stuck_once = false;   // abandoned: the loop was left with instances still queued or in flight (reported, never silent)
  std::vector<int> done_now; std::vector<double> t_done;   // inst_done as of this round; seconds from admission to proof (-1: not proven)
  SplitState sp;
  // the launches
  size_t nev = 0; int rounds = 0, prev_bc = 0; long long launched_nodes = 0;
  bool use_par = false, use_cls = false; size_t l_eval = 0;
  std::vector<int> round_bc;   // MIQP_ROUND_LOG
  // adaptive width of a single solve
  int width_now = 0, width_since = 0, demand_now = 0; unsigned long long width_key = ~0ull, kinc_now = ~0ull; double lb_now = -1e300;
  double t0 = 0, tlim = 0;

  Rounds(DevCtx& X_, const CallShape& sh_, const HostTables& H_, const SplitCtx* split_, int verbose_, size_t l_eval_)
      : X(X_), sh(sh_), H(H_), split(split_), verbose(verbose_), B(X_.B), st(X_.stream), n(sh_.n), NS(sh_.NS),
        slot_inst(sh_.NS, -1), kill(sh_.n, 0), t_admit(sh_.n, 0.0), stalled(sh_.n, 0), done_now(H_.h_done), t_done(sh_.n, -1.0), l_eval(l_eval_) {}

  // frees the slots of proven / retired instances and fills them from the queue; `sel`: the list buffer the next select reads
  bool admit(double now, int sel) {
    pairs.clear();
    for (int sl = 0; sl < NS; ++sl) {
      const int k = slot_inst[sl];
      if (k >= 0 && !done_now[k]) continue;   // busy
      if (k >= 0) { in_flight--; slot_inst[sl] = -1; }
      while (next_q < n && H.h_done[next_q]) next_q++;   // instances that never start (infeasible first step, no root on this rank)
      if (next_q < n) { pairs.push_back(sl); pairs.push_back(next_q); slot_inst[sl] = next_q; t_admit[next_q] = now; next_q++; in_flight++; }
      else if (k >= 0) { pairs.push_back(sl); pairs.push_back(-1); }
    }
    if (!pairs.empty()) {
      const int np_ = (int)pairs.size() / 2;
      HIP_OK(hipMemcpyAsync(X.d_pairs, pairs.data(), pairs.size() * 4, hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(admit_kernel, dim3((np_ + 63) / 64), dim3(64), 0, st, B, (const int*)X.d_pairs, np_, sel);
      // (no synchronisation: the copy from pageable memory is staged before the call returns, the device buffer is protected by the stream order)
    }
    return true;
  }

  // time limit per instance, counted from its admission: the instance is retired by the next select_kernel (its records
  // return to the pool) and reports TIME_LIM_* in report()
  bool kill_timed_out(double tnow) {
    bool any_kill = false;
    for (int sl = 0; sl < NS; ++sl) { const int k = slot_inst[sl]; if (k >= 0 && !done_now[k] && !kill[k] && tnow - t_admit[k] > H.h_tlim[k]) { kill[k] = 1; any_kill = true; } }
    if (any_kill) HIP_OK(hipMemcpyAsync(B.inst_kill, kill.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    return true;
  }

  // An empty round (one may come up while a list tier is being reorganised, or right after admissions).  64 of them in a row: the instances
  // in flight are stuck (none of them is done, none has an open node to offer).  They are retired like instances at their time limit - the
  // slots go to the rest of the queue, which is NOT abandoned; a second such streak with nothing admitted in between ends the call with an
  // error (`abandoned`)
  bool empty_round() {
    if (++empty_rounds <= 64) return true;
    if (stuck_once) { for (int sl = 0; sl < NS; ++sl) { const int k = slot_inst[sl]; if (k >= 0 && !done_now[k]) stalled[k] = 1; } abandoned = true; return true; }   // (the instances in flight did not run out of time either)
    stuck_once = true; empty_rounds = 0;
    for (int sl = 0; sl < NS; ++sl) { const int k = slot_inst[sl]; if (k >= 0 && !done_now[k]) { kill[k] = 1; stalled[k] = 1; } }
    HIP_OK(hipMemcpyAsync(B.inst_kill, kill.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    std::fprintf(stderr, "[miqp_gpu] %d instances in flight made no progress for 64 rounds: retired, the queue goes on\n", in_flight);
    return true;
  }

  // Tree split, once per round: the ranks agree on incumbent, bound and whether to go on (identical decisions everywhere).
  // `stop`: the job is over (sp.finished says whether with a proof); `local_done`: this rank has nothing left and only keeps taking part
  bool exchange(int bc, bool& stop, bool& local_done) {
    unsigned long long kinc = ~0ull; double lbl = 1e300;
    HIP_OK(hipMemcpy(&kinc, B.inc_key, 8, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(&lbl, B.lower_bound, 8, hipMemcpyDeviceToHost));
    local_done = bc <= 0;
    unsigned long long w[4];
    w[0] = kinc >= 0xFFF0000000000000ull ? ~0ull : ((kinc & ~0xFFFFFull) | (unsigned long long)split->rank);
    w[1] = host_d2key(local_done && kinc >= 0xFFF0000000000000ull ? 1e300 : (local_done ? std::min(lbl, 1e300) : lbl));
    w[2] = local_done ? ~0ull : 0ull;
    w[3] = (wall_s() - t0 > tlim) ? 0ull : ~0ull;
    if (split->fn(split->user, 0, w, 4, 0) != 0) { std::fprintf(stderr, "[miqp_gpu] incumbent exchange failed\n"); return false; }
    sp.inc = w[0] >= 0xFFF0000000000000ull ? 1e300 : host_key2d(w[0] & ~0xFFFFFull); sp.owner = (int)(w[0] & 0xFFFFFull);
    sp.lb = host_key2d(w[1]); sp.timeup = w[3] == 0ull;
    HIP_OK(hipMemcpyAsync(B.inc_ext, &sp.inc, 8, hipMemcpyHostToDevice, st));
    const bool all_done = w[2] == ~0ull;
    const bool gap_ok = sp.inc < 1e299 && (sp.inc - sp.lb) <= H.h_gap[0] * (1e-10 + std::fabs(sp.inc));
    stop = all_done || sp.timeup || gap_ok;
    if (stop) sp.finished = all_done || gap_ok;
    return true;
  }

  // A single solve widens its rounds once it is bound-limited (plan_call): the incumbent has not moved for 32 rounds, the near list offers
  // eight rounds' worth of eligible nodes ...
  void adapt_width() {
    if (kinc_now != width_key) { width_key = kinc_now; width_since = rounds; }
    else if (kinc_now < 0xFFF0000000000000ull && rounds - width_since >= 32 && demand_now >= 8 * width_now && width_now < sh.width_max) {
      // ... and the incumbent is already close to the bound (within 5 %): with a poor incumbent a wide round solves what a better one would have pruned
      // (cfg5 seed 11 widened on a stale incumbent alone ended at a gap of 45 % instead of 2 %)
      const double io_ = host_key2d(kinc_now & ~0xFFFFFull);
      if (lb_now > -1e299 && io_ - lb_now <= 0.05 * std::fabs(io_)) { width_now *= 2; width_since = rounds; }
    }
  }

  bool run() {
    const ProcessSwitches& ps = process_switches(); const CallSwitches& sw = X.sw; const Layout& Y = X.Y;
    t0 = wall_s();
    for (int k = 0; k < n; ++k) tlim = std::max(tlim, H.h_tlim[k]);
    HIP_OK(hipEventRecord(X.ev0, st));
    if (!admit(0.0, 0)) return false;
    // (Enqueueing the launches of a round before the host has read the selection's counters - "pipelined rounds" - was measured twice and
    // removed in round 5: no gain on queues (round 3: the time between the interior point launches is the selection and evaluation kernels, not
    // the host) and none on single solves (round 5: p99 58.3 -> 59.6 ms, profiles/r05_single_latency.txt))
    // the counters of a round's launches (batch count, work counters, hand-over counts) come in two parity sets: a round uses one, its
    // roll_kernel zeroes the other for the round after - six 4-byte memsets per round less in the stream (0.65 ms of the 1.4 ms round of a single solve)
    use_par = X.ctr && X.oc_grid > 0 && X.ocb_grid > 0 && X.concurrent_big && X.stream2 && X.probe_grid > 0 && !sw.memsets;
    if (use_par) HIP_OK(hipMemsetAsync(X.ctr, 0, 2 * CTR_SET * 4, st));
    use_cls = use_par && X.as_on && X.cls_list && sw.cls_lists;
    B.cls_list = use_cls ? X.cls_list : nullptr; B.cls_take = 0; X.cls_n[0] = X.cls_n[1] = X.cls_n[2] = -1;
    width_now = sh.adaptive_width ? sh.width0 : 0;
    // (share_kernel - one workgroup, 0.23 ms: the shares of the NEXT round from this selection's demands - beside lns_kernel, 0.22 ms, on the second stream:
    // neither reads what the other writes)
    const bool share_aside = B.lns_mode > 0 && NS >= 64 && X.stream2 && X.ev_sfork && !sw.debug_sync;
    for (;;) {
      // ---- select, local search, roll, shares
      const int par = rounds & 1;
      B.width_cap = width_now;
      if (use_par) { B.batch_count = X.ctr + CTR_SET * par; B.cls_count = B.batch_count + 8; } else HIP_OK(hipMemsetAsync(B.batch_count, 0, 4, st));
      B.open_sel = rounds & 1;
      B.prev_bc = prev_bc;
      hipLaunchKernelGGL(select_kernel, dim3(NS), dim3(SEL_THREADS), 0, st, B, rounds);
      if (share_aside) { (void)hipEventRecord(X.ev_sfork, st); (void)hipStreamWaitEvent(X.stream2, X.ev_sfork, 0); hipLaunchKernelGGL(share_kernel, dim3(1), dim3(1024), 0, X.stream2, B); (void)hipEventRecord(X.ev_sjoin, X.stream2); }
      if (B.lns_mode > 0) hipLaunchKernelGGL(lns_kernel, dim3(NS), dim3(64), 0, st, B);   // the neighbours of new incumbents join this round's batch
      if (sw.debug_sync) debug_sync(st, rounds, "select");
      hipLaunchKernelGGL(roll_kernel, dim3(1), dim3(CTR_SET), 0, st, B, use_par ? X.ctr + CTR_SET * (par ^ 1) : (int*)nullptr);
      if (share_aside) (void)hipStreamWaitEvent(st, X.ev_sjoin, 0); else hipLaunchKernelGGL(share_kernel, dim3(1), dim3(1024), 0, st, B);
      // ---- the round's counters
      int bc = 0; int hctr[CTR_SET] = {0};
      HIP_OK(hipMemcpyAsync(use_cls ? hctr : &bc, B.batch_count, use_cls ? CTR_SET * 4 : 4, hipMemcpyDeviceToHost, st));
      HIP_OK(hipMemcpyAsync(done_now.data(), B.inst_done, (size_t)n * 4, hipMemcpyDeviceToHost, st));
      if (sh.adaptive_width) { HIP_OK(hipMemcpyAsync(&kinc_now, B.inc_key, 8, hipMemcpyDeviceToHost, st)); HIP_OK(hipMemcpyAsync(&demand_now, B.slot_demand, 4, hipMemcpyDeviceToHost, st)); HIP_OK(hipMemcpyAsync(&lb_now, B.lower_bound, 8, hipMemcpyDeviceToHost, st)); }
      HIP_OK(hipStreamSynchronize(st));
      if (use_cls) { bc = hctr[0]; for (int q = 0; q < 3; ++q) X.cls_n[q] = std::min(hctr[8 + q], X.batch_cap); }
      if (sh.adaptive_width) adapt_width();
      const double tnow = wall_s() - t0;
      for (int sl = 0; sl < NS; ++sl) { const int k = slot_inst[sl]; if (k >= 0 && done_now[k] && t_done[k] < 0) t_done[k] = tnow - t_admit[k]; }   // time from admission to proof
      // ---- who goes on: the ranks of a tree split agree; a batch or queue retires, admits, and stops when it is drained
      if (split) {
        bool stop = false, local_done = false;
        if (!exchange(bc, stop, local_done)) return false;
        if (stop) break;
        if (local_done) { rounds++; continue; }   // nothing left here: keep taking part in the exchange
      } else {
        if (!kill_timed_out(tnow)) return false;
        if (!admit(tnow, 1 - (rounds & 1))) return false;
        if (in_flight == 0 && next_q >= n) break;   // the queue is drained
        if (tnow > tlim * (double)((n + NS - 1) / NS + 1) + 30.0) { abandoned = true; break; }   // (safety net: no instance can outlive its limit by more than a round)
        if (bc <= 0) {
          if (!empty_round()) return false;
          if (abandoned) break;
          rounds++; prev_bc = 0; continue;
        }
        stuck_once = false;
        empty_rounds = 0;
      }
      if (bc > X.batch_cap) bc = X.batch_cap;
      if (sw.trace && bc > 0 && bc <= 256 && !trace_selection(X, rounds, bc)) return false;
      // ---- the launch group of the round, between two events (and a third where the standard launch ends)
      if (X.ipm_ev.size() < nev + 2) { hipEvent_t a, b; HIP_OK(hipEventCreate(&a)); HIP_OK(hipEventCreate(&b)); X.ipm_ev.push_back(a); X.ipm_ev.push_back(b); }
      if (ps.launch_trace && !X.ev_mid) HIP_OK(hipEventCreate(&X.ev_mid));
      if (X.std_ev.size() < nev / 2 + 1) { hipEvent_t a_; HIP_OK(hipEventCreate(&a_)); X.std_ev.push_back(a_); }
      HIP_OK(hipEventRecord(X.ipm_ev[nev], st));
      launch_ipm_batch(X, B, bc, st, true, use_par ? par : -1, X.std_ev[nev / 2]);
      HIP_OK(hipEventRecord(X.ipm_ev[nev + 1], st));
      if (ps.launch_trace && !trace_launches(X, rounds, bc, nev)) return false;
      nev += 2;
      if (bc >= X.batch_cap / 2 && rounds >= ps.replay_round && !replay_batch(X, bc)) return false;
      if (sw.debug_sync) debug_sync(st, rounds, "ipm", bc);
      if (sw.trace && !trace_batch(X, rounds, bc)) return false;
      // ---- evaluation: incumbents, pruning, children into the list buffer the next select reads
      { DevBuf Be = B; Be.open_sel = 1 - (rounds & 1); launch_eval_c(Y.C, Be, bc, l_eval, st); }
      if (X.pool.on && !pool_capture(X, bc)) return false;   // (before the next evaluation overwrites the candidates)
      if (sw.debug_sync) debug_sync(st, rounds, "eval");
      launched_nodes += bc; rounds++; prev_bc = bc;
      if (ps.round_log) round_bc.push_back(bc);
      if (verbose > 1) std::fprintf(stderr, "[miqp_gpu] round %d: %d nodes\n", rounds, bc);
      if (verbose == 1 && rounds % 25 == 0 && !print_progress(X, wall_s() - t0, rounds, launched_nodes, H.h_const[0])) return false;
    }
    return true;
  }
};

// ---------------------------------------------------------------- behind the rounds: polish, read-back, the verdicts
// polish: the incumbent of every instance is re-solved (all disjunctions fixed as completed) to a tight tolerance; its objective and
// states are what the caller receives.  Ends the device work of the call: `ms_all` is the time between its first round and here
struct Polished { std::vector<double> obj, viol; std::vector<int> ok, it; };
bool polish(DevCtx& X, int n, Polished& P, float& ms_all) {
  const DevBuf& B = X.B; const Layout& Y = X.Y; hipStream_t st = X.stream;
  P.obj.assign(n, 0.0); P.viol.assign(n, 1.0); P.ok.assign(n, 0); P.it.assign(n, 0);
  HIP_OK(hipMemcpyAsync(B.pool_fix, B.inc_fix, (size_t)n * Y.fixlen, hipMemcpyDeviceToDevice, st));
  std::vector<int> ids(n); for (int k = 0; k < n; ++k) ids[k] = k;
  HIP_OK(hipMemcpyAsync(B.batch_node, ids.data(), n * 4, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(B.batch_inst, ids.data(), n * 4, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(B.batch_count, &n, 4, hipMemcpyHostToDevice, st));
  HIP_OK(hipStreamSynchronize(st));
  DevBuf Bp = B; Bp.qp_tol = QP_TOL_FINAL; Bp.use_cutoff = 0; Bp.batch_cap = X.batch_alloc;
  // the polish starts at the incumbent's own solution (integer feasible: every row of the completed record holds there), centred
  // at a small complementarity - a third of the iterations of a cold solve to 1e-13 (the last thing a single solve waits for)
  Bp.ws_on = (B.ws_on && !X.sw.polish_cold) ? 2 : 0; Bp.ws_mu = X.sw.polish_mu; Bp.ws_delta = X.sw.polish_delta;
  int nb = std::min(n, X.batch_alloc);
  launch_ipm_batch(X, Bp, nb, st);
  HIP_OK(hipMemcpyAsync(P.obj.data(), B.batch_obj, nb * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(P.viol.data(), B.batch_viol, nb * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(P.ok.data(), B.batch_ok, nb * 4, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(P.it.data(), B.batch_it, nb * 4, hipMemcpyDeviceToHost, st));
  HIP_OK(hipEventRecord(X.ev1, st));
  HIP_OK(hipStreamSynchronize(st));
  HIP_OK(hipGetLastError());
  HIP_OK(hipEventElapsedTime(&ms_all, X.ev0, X.ev1));
  return true;
}

// what the device knows of every instance at the end of the call
struct Results {
  std::vector<double> inc, lb, Z; std::vector<int> flags, ninc, oc, dn; std::vector<long long> nodes, iters;
  std::vector<signed char> fix; unsigned long long rowiters = 0, as[32] = {0};
};
bool read_back(const DevCtx& X, int n, Results& R) {
  const DevBuf& B = X.B; const Layout& Y = X.Y;
  R.inc.resize(n); R.lb.resize(n); R.flags.resize(n); R.ninc.resize(n); R.oc.resize(n); R.dn.resize(n); R.nodes.resize(n); R.iters.resize(n);
  HIP_OK(hipMemcpy(R.inc.data(), B.inc_obj, n * 8, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(R.lb.data(), B.lower_bound, n * 8, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(R.flags.data(), B.inst_flags, n * 4, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(R.ninc.data(), B.inst_ninc, n * 4, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(R.oc.data(), B.open_count, n * 4, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(R.dn.data(), B.inst_done, n * 4, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(R.nodes.data(), B.inst_nodes, n * 8, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(R.iters.data(), B.inst_iters, n * 8, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(&R.rowiters, B.stat_rowiters, 8, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(R.as, B.as_stats, 256, hipMemcpyDeviceToHost));
  if (B.stats && R.as[0] + R.as[2] > 0) print_as_stats(R.as);
  R.fix.resize((size_t)n * Y.fixlen); R.Z.resize((size_t)n * Y.N * Y.nz);
  HIP_OK(hipMemcpy(R.fix.data(), B.inc_fix, R.fix.size(), hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(R.Z.data(), B.inc_Z, R.Z.size() * 8, hipMemcpyDeviceToHost));
  return true;
}
// ... of which the polished solution replaces the incumbent's where the polish converged
bool take_polished(const DevCtx& X, miqp_solver_t* const* S, int n, const HostTables& H, const Polished& P, Results& R) {
  const DevBuf& B = X.B; const Layout& Y = X.Y;
  std::vector<double> h_pZ((size_t)n * Y.N * Y.nz);
  HIP_OK(hipMemcpy(h_pZ.data(), B.batch_Z, h_pZ.size() * 8, hipMemcpyDeviceToHost));
  for (int k = 0; k < n; ++k) {
    if (!(R.inc[k] < 1e299)) continue;
    if (P.viol[k] <= FEAS_TOL && (P.ok[k] || P.it[k] >= 10)) {
      int nign = 0; for (int q = 0; q < Y.C * Y.O * Y.N * 5; ++q) nign += R.fix[(size_t)k * Y.fixlen + Y.f_obs + q] >= Y.L;
      R.inc[k] = P.obj[k] + H.h_const[k] + nign * S[k]->inst.w_slack_obs;
      std::copy(h_pZ.begin() + (size_t)k * Y.N * Y.nz, h_pZ.begin() + (size_t)(k + 1) * Y.N * Y.nz, R.Z.begin() + (size_t)k * Y.N * Y.nz);
    }
  }
  return true;
}

// tree split: the owner of the best incumbent hands its polished solution to every rank: {objective, states, completed record};
// the verdict of the whole job is the same on every rank
bool split_broadcast(const SplitCtx* split, const SplitState& sp, Results& R) {
  std::vector<unsigned char> buf(8 + R.Z.size() * 8 + R.fix.size());
  unsigned long long w[2] = {R.inc[0] < 1e299 ? ((host_d2key(R.inc[0]) & ~0xFFFFFull) | (unsigned long long)split->rank) : ~0ull, ~0ull};
  if (split->fn(split->user, 0, w, 2, 0) != 0) { std::fprintf(stderr, "[miqp_gpu] incumbent exchange failed\n"); return false; }
  if (w[0] < 0xFFF0000000000000ull) {
    const int owner = (int)(w[0] & 0xFFFFFull);
    if (owner == split->rank) { std::memcpy(buf.data(), &R.inc[0], 8); std::memcpy(buf.data() + 8, R.Z.data(), R.Z.size() * 8); std::memcpy(buf.data() + 8 + R.Z.size() * 8, R.fix.data(), R.fix.size()); }
    if (split->fn(split->user, 1, buf.data(), (int)buf.size(), owner) != 0) { std::fprintf(stderr, "[miqp_gpu] solution broadcast failed\n"); return false; }
    std::memcpy(&R.inc[0], buf.data(), 8); std::memcpy(R.Z.data(), buf.data() + 8, R.Z.size() * 8); std::memcpy(R.fix.data(), buf.data() + 8 + R.Z.size() * 8, R.fix.size());
    R.lb[0] = std::min(sp.lb, R.inc[0]);
  }
  R.flags[0] = sp.finished ? 0 : 1; R.oc[0] = 0; R.dn[0] = 1;
  return true;
}

// host and device times of a call, as the handles report them (miqp_solver_last_timing / _last_active_set / _last_setup)
struct CallTimes { double t_setup = 0, t_ctx = 0, t_tables = 0, t_solve = 0, ms_ipm = 0, ms_std = 0; float ms_all = 0; bool ctx_built = false, std_timed = false; };

// status, properties and solution of every handle
void report(miqp_solver_t* const* S, int* statuses, const Layout& Y, const HostTables& H, const Rounds& L, const Results& R, const CallTimes& T, bool split) {
  const int n = L.n;
  long long tot_iters = 0; for (int k = 0; k < n; ++k) tot_iters += R.iters[k];
  for (int k = 0; k < n; ++k) {
    miqp_solver* s = S[k];
    bool have = R.inc[k] < 1e299;
    bool unfinished = (R.flags[k] & 3) || R.oc[k] > 0 || !R.dn[k];   // bit 0: a list or the record pool overflowed, bit 1: retired at its time limit
    if (!split && k >= L.next_q && !H.h_done[k]) {   // never admitted (the round loop was abandoned): the solver did not run on it - not a time-limit verdict
      s->status = MIQP_STATUS_FAILED_SEG_FAULT; s->has_sol = false; s->props.objective = NAN; s->props.gap = NAN; s->props.best_bound = NAN; s->props.status = 0; s->props.time = 0.0;
      s->err = "the queue was abandoned before this instance was admitted";
      statuses[k] = s->status; continue;
    }
    s->props.time = L.t_done[k] >= 0 ? L.t_done[k] : std::max(0.0, T.t_solve - L.t_admit[k]);   // from the instance's admission to its proof (or to the end of the call)
    s->admit_s = L.t_admit[k];
    s->props.NrIterations = (int)std::min<long long>(R.iters[k], 2147483647LL); s->props.nodes = R.nodes[k];
    s->props.NrSolutionPool = R.ninc[k];
    s->timing[0] = T.ms_all * 1e-3; s->timing[1] = T.ms_ipm * 1e-3; s->timing[2] = (double)(L.nev / 2); s->timing[3] = (double)L.launched_nodes;
    s->timing[4] = (double)tot_iters; s->timing[5] = (double)R.rowiters;
    s->as_timing[0] = (double)R.as[0]; s->as_timing[1] = (double)R.as[1]; s->as_timing[2] = (double)R.as[2]; s->as_timing[3] = (double)R.as[3];
    s->as_timing[4] = (double)R.as[6]; s->as_timing[5] = (double)R.as[7]; s->as_timing[6] = T.ms_std * 1e-3; s->as_timing[7] = T.std_timed ? (double)(L.nev / 2) : 0.0;
    s->setup[0] = T.t_setup; s->setup[1] = T.t_ctx; s->setup[2] = T.ctx_built ? 1.0 : 0.0;
    s->err.clear();
    if (L.stalled[k] && unfinished) s->err = "retired without a proof: no progress for 64 branch-and-bound rounds (not a time-limit verdict)";
    if (have) {
      s->status = MIQP_STATUS_SUCCESS; s->has_sol = true;
      s->props.objective = R.inc[k];
      double lb = std::min(R.lb[k], R.inc[k]);
      // nodes within the gap of the incumbent are dropped without being refined: what is proven is the smaller of the open
      // list's best bound and incumbent - gap*|incumbent| (CPLEX reports the bound of its remaining nodes the same way)
      const double lb_tol = R.inc[k] - H.h_gap[k] * std::fabs(R.inc[k]);
      lb = std::min(lb, lb_tol);
      s->props.best_bound = lb; s->props.gap = std::fabs(lb - R.inc[k]) / (1e-10 + std::fabs(R.inc[k]));
      // (a proof closed to the tolerance reports a gap of at most the tolerance: the rounding of the subtraction above put the quotient 1e-16 over it
      // for every second incumbent at tolerances of 1e-6 and below - whether `gap <= tolerance` held depended on the last bit of the objective)
      if (lb == lb_tol && s->props.gap > H.h_gap[k]) s->props.gap = H.h_gap[k];
      s->props.status = unfinished ? MIQP_CPX_STAT_TIME_LIM_FEAS : (s->props.gap <= 1e-9 ? MIQP_CPX_STAT_OPTIMAL : MIQP_CPX_STAT_OPTIMAL_TOL);
      s->Z.assign(R.Z.begin() + (size_t)k * Y.N * Y.nz, R.Z.begin() + (size_t)(k + 1) * Y.N * Y.nz);
      s->comp.assign(R.fix.begin() + (size_t)k * Y.fixlen, R.fix.begin() + (size_t)(k + 1) * Y.fixlen);
    } else {
      s->status = unfinished ? (L.stalled[k] ? MIQP_STATUS_FAILED_SEG_FAULT : MIQP_STATUS_FAILED_TIMEOUT) : MIQP_STATUS_FAILED_NO_SOLUT;   // (a stalled instance did not run out of time: the solver could not go on)
      s->props.objective = NAN; s->props.gap = NAN; s->props.best_bound = R.lb[k];
      s->props.status = unfinished ? MIQP_CPX_STAT_TIME_LIM_INFEAS : MIQP_CPX_STAT_INFEASIBLE;
    }
    statuses[k] = s->status;
  }
  if (L.abandoned) std::fprintf(stderr, "[miqp_gpu] the round loop was abandoned with %d of %d instances never admitted: they report FAILED_SEG_FAULT, the call fails\n", n - L.next_q, n);
}

// solution pool (solution_pool.hip): the buffers and the reset of a call with a pool (nothing without one); the kept entries to the handles
bool pool_prepare(DevCtx& X, miqp_solver_t* const* S, int n);
bool pool_read_back(const DevCtx& X, miqp_solver_t* const* S, int n, const Results& R);   // (R.fix: the incumbents' records)

// starts from the carried pool (miqp_solver_set_pool_starts): what a solve takes from the handle's pool before it drops it - the first
// min(pool_starts, pool_n) entries in pool order of a pool that a carry put there and that no solve stands behind.  A tree split takes none
void pool_starts_take(miqp_solver* s, bool split) {
  s->drop_starts();
  if (split || s->pool_starts <= 0 || !s->has_inst || !s->pool_carried || s->pool_n <= 0 || s->pool_fixlen <= 0) return;
  const int t = std::min(s->pool_starts, s->pool_n);
  if (s->pool_fix.size() < (size_t)t * s->pool_fixlen) return;
  s->st_offer = t; s->st_fixlen = s->pool_fixlen;
  s->st_fix.assign(s->pool_fix.begin(), s->pool_fix.begin() + (size_t)t * s->pool_fixlen);
}
// ... and behind the pool's read-back, on the host: where each start of the solve stands in the pool it left (pool_carry.hip)
void pool_starts_places(miqp_solver* s, const Layout& Y);

// ---------------------------------------------------------------- the batch solve
bool solve_batch_impl(miqp_solver_t* const* S, int n, int* statuses, const SplitCtx* split = nullptr, int inflight = 0, int lane = 0, int lanes = 1) {
  // every way out of this function that is not report() at its end (a failed HIP call, a failed exchange) leaves "the solver could not
  // run" behind: a caller's zero-filled status array would otherwise read as SUCCESS for instances that were never solved.  Every phase
  // returns false on such a failure (HIP_OK does, after naming the call) and nothing before report() touches `statuses`
  for (int k = 0; k < n; ++k) { statuses[k] = MIQP_STATUS_FAILED_SEG_FAULT; if (S[k]) { S[k]->status = MIQP_STATUS_FAILED_SEG_FAULT; S[k]->has_sol = false; S[k]->rescache.reset(); pool_starts_take(S[k], split != nullptr); S[k]->drop_pool(); } }
  if (split && n != 1) return false;
  BatchShape bs = batch_layout(S, n);
  if (!bs.ok) { for (int k = 0; k < n; ++k) { if (S[k]) S[k]->err = bs.err; statuses[k] = MIQP_STATUS_FAILED_SEG_FAULT; } std::fprintf(stderr, "[miqp_gpu] %s\n", bs.err.c_str()); return false; }
  const Layout& Y = bs.Y;
  const miqp_solver_opts& O0 = S[0]->opts;
  auto fail_all = [&](const char* why) { if (why) std::fprintf(stderr, "[miqp_gpu] %s\n", why); for (int k = 0; k < n; ++k) statuses[k] = MIQP_STATUS_FAILED_SEG_FAULT; return false; };
  for (int k = 1; k < n; ++k) if (S[k]->opts.device != O0.device) return fail_all("instances of one batch must name the same device (use miqp_solver_solve_batch_multi to span devices)");
  const double t_enter = wall_s();
  DevCtx* Xp = ctx_for_device(O0.device, lane);
  if (!Xp) return fail_all(nullptr);
  warn_ignored_switches();
  DevCtx& X = *Xp;
  std::lock_guard<std::mutex> ctx_lock(X.mu);
  if (hipSetDevice(X.device) != hipSuccess) return fail_all("hipSetDevice failed");
  const CallSwitches sw = read_call_switches();
  // the root records of the call: today's, plus - when a handle offers starts from its carried pool (records of another length are not offered) - the
  // largest max_starts SETTING among the handles that do.  The setting, not the number offered: the context is kept only while the root stride stays
  // (ctx_matches), and a receding horizon carries another number of records every cycle
  int starts = 0;
  for (int k = 0; k < n; ++k) { if (S[k]->st_fixlen != Y.fixlen) S[k]->st_offer = 0; if (S[k]->st_offer > 0) starts = std::max(starts, S[k]->pool_starts); }
  const CallShape sh = plan_call(Y, O0, n, inflight, lanes, split != nullptr, sw, starts);
  const size_t l_ipm = ipm_lds_bytes(Y), l_eval = eval_lds_bytes(Y, sw.seq_kinds);
  CallTimes T;
  {
    // the fallible part of the set-up (device buffers, kernel attributes).  In a tree split the ranks agree on its outcome with
    // one exchange before the first round: a rank that failed alone would otherwise leave its peers waiting in their all-reduce
    bool setup_ok = ctx_prepare(X, Y, n, sh.NS, sh.open_cap, sh.npr, sh.MAXR, sh.clamp_open, lanes, &T.ctx_built);
    if (setup_ok && (l_ipm > 160 * 1024 || l_eval > 160 * 1024)) { std::fprintf(stderr, "[miqp_gpu] instance too large for LDS (%zu bytes)\n", l_ipm); setup_ok = false; }
    if (setup_ok && !set_kernel_lds(Y, l_ipm, l_eval)) setup_ok = false;
    if (setup_ok && !pool_prepare(X, S, n)) setup_ok = false;
    if (split) {
      unsigned long long w = setup_ok ? 1ull : 0ull;
      if (split->fn(split->user, 0, &w, 1, 0) != 0) return fail_all("set-up exchange failed");
      if (setup_ok && w == 0ull) return fail_all("another rank of the tree split failed its set-up");
    }
    if (!setup_ok) return fail_all(nullptr);
  }
  T.t_ctx = wall_s() - t_enter;
  HostTables H;
  prepare_instances(S, Y, sh, split, H);
  T.t_tables = wall_s() - t_enter - T.t_ctx;
  apply_call_switches(X, sh, sw, H.h_gap);
  if (!upload_and_reset(X, H, sh)) return fail_all(nullptr);

  Rounds L(X, sh, H, split, O0.verbose, l_eval);
  if (!L.run()) return fail_all(nullptr);
  T.t_setup = L.t0 - t_enter;
  if (sw.dump_open && !dump_open_list(X, sw.dump_open, L.rounds, sh.NS, H.h_const[0])) return fail_all(nullptr);

  Polished P;
  if (!polish(X, n, P, T.ms_all)) return fail_all(nullptr);
#ifdef MIQP_PROFILE
  if (!print_profile(X)) return fail_all(nullptr);
#endif
  if (X.B.stats && !print_stats(X)) return fail_all(nullptr);
  if (process_switches().round_log) { std::fprintf(stderr, "[rounds]"); for (int v : L.round_bc) std::fprintf(stderr, " %d", v); std::fprintf(stderr, "\n"); }
  for (size_t e = 0; e + 1 < L.nev; e += 2) { float ms = 0; HIP_OK(hipEventElapsedTime(&ms, X.ipm_ev[e], X.ipm_ev[e + 1])); T.ms_ipm += ms; }
  T.std_timed = L.use_par;   // (the event is recorded in the concurrent launch path only)
  if (T.std_timed) for (size_t e = 0; e + 1 < L.nev; e += 2) { float ms = 0; if (hipEventElapsedTime(&ms, X.ipm_ev[e], X.std_ev[e / 2]) == hipSuccess) T.ms_std += ms; }
  T.t_solve = wall_s() - L.t0;

  Results R;
  if (!read_back(X, n, R) || !take_polished(X, S, n, H, P, R)) return fail_all(nullptr);
  if (X.pool.on && !pool_read_back(X, S, n, R)) return fail_all(nullptr);   // (before the broadcast of a tree split: a rank keeps the pool of its own search)
  if (split && !split_broadcast(split, L.sp, R)) return fail_all(nullptr);
  report(S, statuses, Y, H, L, R, T, split != nullptr);
  for (int k = 0; k < n; ++k) if (!S[k]->has_sol) S[k]->drop_pool();
  for (int k = 0; k < n; ++k) if (S[k]->st_n > 0) pool_starts_places(S[k], Y);
  if (sw.stats) std::fprintf(stderr, "[miqp_gpu stats] reachable-set diameter (L1) of instance 0: %.1f\n", H.D[Y.d_misc + 2]);
  if (sw.stats) std::fprintf(stderr, "[miqp_gpu stats] host: setup %.3f s (device context %.3f, instance tables and presolve %.3f, upload %.3f), rounds %.3f s (%d), results %.3f s\n", T.t_setup, T.t_ctx, T.t_tables, T.t_setup - T.t_ctx - T.t_tables, T.t_solve, L.rounds, wall_s() - L.t0 - T.t_solve);
  return !L.abandoned;
}

}  // namespace

#include "certify.hip"
#include "pool_blocks.hip"
#include "fixed_chain.hip"
#include "fixed_batch.hip"
#include "as_fixed.hip"
#include "solution_pool.hip"
#include "pool_improve.hip"
#include "pool_label.hip"
#include "pool_settle.hip"
#include "pool_explore.hip"
#include "pool_carry.hip"

// the caches of the calls above, by device ordinal; used under the device lock (DevCtx::mu of lane 0)
std::map<int, std::tuple<CertDev, FixedDev, PoolImproveDev, PoolEntryDev, PoolLabelDev, PoolSettleDev, PoolExploreDev, PoolCarryDev>> g_call_devs;
template <class D> D& call_dev(int device) { return std::get<D>(g_call_devs[device]); }

// ================================================================================================
//  C ABI
// ================================================================================================
extern "C" {

const char* miqp_gpu_version(void) { return "miqp_gpu 0.1 (gfx950)"; }

miqp_solver_t* miqp_solver_create(const miqp_solver_opts* opts) {
  miqp_solver* s = new miqp_solver();
  if (opts) s->opts = *opts; else { s->opts.precision = 12; s->opts.device = -1; s->opts.gap_override = -1; }
  if (s->opts.precision <= 0) s->opts.precision = 12;
  return s;
}

void miqp_solver_destroy(miqp_solver_t* s) { delete s; }

int miqp_solver_set_params(miqp_solver_t* s, const miqp_model_params_c* p) {
  if (!s || !p) return -1;
  s->has_inst = inst_from_params(p, s->opts.precision - 2, s->inst, s->err);
  s->rescache.reset(); s->drop_fixed_batch(); s->drop_pool(); s->drop_starts();
  s->has_sol = false;   // MIP starts stay registered (the reference keeps them in the wrapper across resetParameters)
  if (!s->has_inst) std::fprintf(stderr, "[miqp_gpu] %s\n", s->err.c_str());
  return s->has_inst ? 0 : -2;
}

int miqp_solver_load_dat(miqp_solver_t* s, const char* path) {
  if (!s || !path) return -1;
  s->has_inst = inst_from_dat(path, s->inst, s->err);
  s->has_sol = false; s->rescache.reset(); s->drop_fixed_batch(); s->drop_pool(); s->drop_starts();
  if (!s->has_inst) std::fprintf(stderr, "[miqp_gpu] %s\n", s->err.c_str());
  return s->has_inst ? 0 : -2;
}

int miqp_solver_override_settings(miqp_solver_t* s, double max_solution_time, double relative_mip_gap_tolerance) {
  if (!s || !s->has_inst) return -1;
  s->inst.tilim = max_solution_time; s->inst.gap = relative_mip_gap_tolerance;
  return 0;
}

int miqp_solver_get_dims(const miqp_solver_t* s, int* o) {
  if (!s || !s->has_inst) return -1;
  o[0] = s->inst.C; o[1] = s->inst.N; o[2] = s->inst.R; o[3] = s->inst.E; o[4] = s->inst.O; o[5] = s->inst.L;
  return 0;
}

int miqp_solver_set_warmstart(miqp_solver_t* s, const miqp_raw_results_c* start, int warmstart_type) {
  if (!s) return -1;
  if (warmstart_type == MIQP_WARMSTART_NONE || !start) { s->ws[0].reset(); s->ws[1].reset(); return 0; }
  // slot 1: the last-solution start (readMIPStarts of the .mst file); slot 0: the receding-horizon start.  With
  // MIQP_WARMSTART_BOTH the caller registers each of the two with its own call (type RECEDING_HORIZON / LAST_SOLUTION)
  const int slot = warmstart_type == MIQP_WARMSTART_LAST_SOLUTION ? 1 : 0;
  if (start->N < 2 || start->NrCars < 1 || start->NrRegions < 1 || start->NrEnvironments < 0 || start->NrObstacles < 0 || start->MaxLinesObstacles < 0 ||
      start->NrCarToCarCollisions != start->NrCars - 1) return -2;
  if (s->has_inst && !dims_match(*start, s->inst)) { s->ws[slot].reset(); return -3; }   // a start of another shape is ignored
  s->ws[slot].reset(new OwnedResults(start->NrCars, start->N, start->NrRegions, start->NrEnvironments, start->NrObstacles, start->MaxLinesObstacles));
  s->ws[slot]->copy_from(*start);
  return 0;
}

int miqp_solver_solve_batch(miqp_solver_t* const* solvers, int n, int* statuses) {
  if (!solvers || n < 1 || !statuses) return -1;
  return solve_batch_impl(solvers, n, statuses) ? 0 : -2;
}

// A long queue is drained by LANES: the instances are dealt round robin to `lanes` sub-queues, each with its share of the slots,
// its own device context (pools, streams) and its own host thread, all on the same device.  The rounds of the lanes are not
// synchronised with each other, so the phases of a round that leave most of the device idle - the memory-backed launch on
// the few large nodes (it lasts as long as its slowest node), selection, the host's look at the counters between two
// rounds - run beside the on-chip launch of another lane.  Measured on one MI355X (tools/lanes_sweep.sh, the bench queue):
// 633 solves/s with one lane, 660 with two, 649 with three, 571 with four - the on-chip kernel fills the register files, so
// what hides is little, and the per-launch times of concurrent lanes no longer say what a kernel costs.  OFF by default
// (MIQP_LANES=2 switches it on); lanes are used when every lane keeps at least 128 instances in flight and the queue is
// longer than the slots.
int miqp_solver_solve_stream(miqp_solver_t* const* solvers, int n, int inflight, int* statuses) {
  if (!solvers || n < 1 || !statuses) return -1;
  int lanes = knob_int(KNOB_P("MIQP_LANES"), 1);
  if (lanes > 8) lanes = 8;
  while (lanes > 1 && (inflight <= 0 || inflight >= n || inflight / lanes < 128)) lanes--;
  if (lanes <= 1) return solve_batch_impl(solvers, n, statuses, nullptr, inflight) ? 0 : -2;
  for (int b = 0; b < n; ++b) { if (!solvers[b]) return -1; if (solvers[b]->opts.device != solvers[0]->opts.device) lanes = 1; }
  if (lanes <= 1) return solve_batch_impl(solvers, n, statuses, nullptr, inflight) ? 0 : -2;
  std::vector<std::vector<miqp_solver_t*>> sub(lanes); std::vector<std::vector<int>> st(lanes);
  for (int b = 0; b < n; ++b) sub[b % lanes].push_back(solvers[b]);
  std::vector<char> ok(lanes, 0);
  std::vector<std::thread> th;
  for (int l = 0; l < lanes; ++l) {
    st[l].assign(sub[l].size(), MIQP_STATUS_FAILED_SEG_FAULT);
    const int infl = (inflight + lanes - 1 - l) / lanes;   // the slots are dealt like the instances
    th.emplace_back([&, l, infl] { ok[l] = solve_batch_impl(sub[l].data(), (int)sub[l].size(), st[l].data(), nullptr, infl, l, lanes) ? 1 : 0; });
  }
  for (auto& t : th) t.join();
  int rc = 0;
  for (int b = 0; b < n; ++b) statuses[b] = st[b % lanes][b / lanes];
  for (int l = 0; l < lanes; ++l) if (!ok[l]) rc = -2;
  return rc;
}

int miqp_solver_solve_batch_multi(miqp_solver_t* const* solvers, int n, int gpus, int* statuses) {
  if (!solvers || n < 1 || !statuses) return -1;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { std::fprintf(stderr, "[miqp_gpu] no HIP device: the solver has no CPU path\n"); for (int k = 0; k < n; ++k) statuses[k] = MIQP_STATUS_FAILED_SEG_FAULT; return -2; }
  if (gpus <= 0 || gpus > ndev) gpus = ndev;
  if (gpus > n) gpus = n;
  // instance b -> device b mod G; no data-path exchange between the shards
  std::vector<std::vector<miqp_solver_t*>> shard(gpus); std::vector<std::vector<int>> st(gpus);
  for (int b = 0; b < n; ++b) { if (!solvers[b]) return -1; solvers[b]->opts.device = b % gpus; shard[b % gpus].push_back(solvers[b]); }
  std::vector<char> ok(gpus, 0);
  std::vector<std::thread> th;
  for (int g = 0; g < gpus; ++g) {
    st[g].assign(shard[g].size(), MIQP_STATUS_FAILED_SEG_FAULT);
    th.emplace_back([&, g] { ok[g] = solve_batch_impl(shard[g].data(), (int)shard[g].size(), st[g].data()) ? 1 : 0; });
  }
  for (auto& t : th) t.join();
  int rc = 0;
  for (int b = 0; b < n; ++b) statuses[b] = st[b % gpus][b / gpus];
  for (int g = 0; g < gpus; ++g) if (!ok[g]) rc = -2;
  return rc;
}

int miqp_solver_solve_split(miqp_solver_t* s, double timestamp, int world, int rank, miqp_exchange_fn exchange, void* user) {
  (void)timestamp;
  if (!s || !s->has_inst || world < 1 || rank < 0 || rank >= world || !exchange) return MIQP_STATUS_FAILED_SEG_FAULT;
  SplitCtx sc{world, rank, exchange, user};
  miqp_solver_t* one[1] = {s}; int st = MIQP_STATUS_FAILED_SEG_FAULT;
  if (!solve_batch_impl(one, 1, &st, &sc)) return MIQP_STATUS_FAILED_SEG_FAULT;
  return st;
}

int miqp_solver_split_roots(const miqp_solver_t* s, int world, int rank, int* root_of_pair, int* index, int* value, int cap, int* nroots_out, int* ncombos_out) {
  if (!s || !s->has_inst || world < 1 || rank < 0 || rank >= world) return -1;
  miqp_solver_t* one[1] = {const_cast<miqp_solver_t*>(s)};
  BatchShape bs = batch_layout(one, 1);
  if (!bs.ok) return -2;
  std::vector<double> D(bs.Y.dstride); std::vector<int> T(bs.Y.istride);
  compile_instance(s->inst, bs.Y, D.data(), T.data());
  std::vector<std::vector<std::pair<int, int>>> combos; split_roots(bs.Y, T.data(), combos, world);
  int np = 0, nr = 0;
  for (size_t q = 0; q < combos.size(); ++q) {
    if ((int)(q % (size_t)world) != rank) continue;
    for (auto& d : combos[q]) { if (np < cap) { if (root_of_pair) root_of_pair[np] = nr; if (index) index[np] = d.first; if (value) value[np] = d.second; } np++; }
    nr++;
  }
  if (nroots_out) *nroots_out = nr;
  if (ncombos_out) *ncombos_out = (int)combos.size();
  return np;
}

// ---------------------------------------------------------------- RCCL transport of the exchange (librccl loaded at run time)
struct Id128 { char b[128]; };   // ncclUniqueId is passed by value
namespace {
struct Rccl {
  void* lib = nullptr; void* comm = nullptr; int world = 0, rank = 0, device = -1; void* dbuf = nullptr; size_t dcap = 0; hipStream_t stream = nullptr;
  int (*GetUniqueId)(void*) = nullptr;
  int (*CommInitRank)(void**, int, Id128, int) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*Broadcast)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
};
Rccl g_rccl; std::mutex g_rccl_mu;
bool rccl_load() {
  if (g_rccl.lib) return true;
  for (const char* nm : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) { g_rccl.lib = dlopen(nm, RTLD_NOW | RTLD_LOCAL); if (g_rccl.lib) break; }
  if (!g_rccl.lib) { std::fprintf(stderr, "[miqp_gpu] librccl not found: %s\n", dlerror()); return false; }
  g_rccl.GetUniqueId = (int (*)(void*))dlsym(g_rccl.lib, "ncclGetUniqueId");
  g_rccl.CommInitRank = (int (*)(void**, int, Id128, int))dlsym(g_rccl.lib, "ncclCommInitRank");
  g_rccl.CommDestroy = (int (*)(void*))dlsym(g_rccl.lib, "ncclCommDestroy");
  g_rccl.AllReduce = (int (*)(const void*, void*, size_t, int, int, void*, hipStream_t))dlsym(g_rccl.lib, "ncclAllReduce");
  g_rccl.Broadcast = (int (*)(const void*, void*, size_t, int, int, void*, hipStream_t))dlsym(g_rccl.lib, "ncclBroadcast");
  return g_rccl.GetUniqueId && g_rccl.CommInitRank && g_rccl.CommDestroy && g_rccl.AllReduce && g_rccl.Broadcast;
}
// miqp_exchange_fn over the communicator: tiny host buffers staged through one device buffer
int rccl_exchange(void*, int op, void* buf, int count, int root) {
  Rccl& R = g_rccl;
  if (!R.comm) return -1;
  const size_t bytes = op == 0 ? (size_t)count * 8 : (size_t)count;
  if (hipSetDevice(R.device) != hipSuccess) return -2;
  if (bytes > R.dcap) { if (R.dbuf) (void)hipFree(R.dbuf); R.dcap = std::max<size_t>(bytes, 1 << 16); if (hipMalloc(&R.dbuf, R.dcap) != hipSuccess) { R.dbuf = nullptr; R.dcap = 0; return -2; } }
  if (hipMemcpyAsync(R.dbuf, buf, bytes, hipMemcpyHostToDevice, R.stream) != hipSuccess) return -2;
  const int rc = op == 0 ? R.AllReduce(R.dbuf, R.dbuf, (size_t)count, /*ncclUint64*/ 5, /*ncclMin*/ 3, R.comm, R.stream)
                         : R.Broadcast(R.dbuf, R.dbuf, bytes, /*ncclUint8*/ 1, root, R.comm, R.stream);
  if (rc != 0) return -3;
  if (hipMemcpyAsync(buf, R.dbuf, bytes, hipMemcpyDeviceToHost, R.stream) != hipSuccess) return -2;
  return hipStreamSynchronize(R.stream) == hipSuccess ? 0 : -2;
}
}  // namespace

int miqp_comm_unique_id(char* out128) {
  std::lock_guard<std::mutex> lk(g_rccl_mu);
  if (!out128 || !rccl_load()) return -1;
  return g_rccl.GetUniqueId(out128) == 0 ? 0 : -2;
}
int miqp_comm_init(int world, int rank, const char* id128, int device) {
  std::lock_guard<std::mutex> lk(g_rccl_mu);
  if (!id128 || world < 1 || rank < 0 || rank >= world || !rccl_load()) return -1;
  if (g_rccl.comm) return -4;   // one communicator per process
  int ndev = 0; if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { std::fprintf(stderr, "[miqp_gpu] no HIP device\n"); return -2; }
  if (device < 0) { if (hipGetDevice(&device) != hipSuccess) device = 0; }
  if (hipSetDevice(device) != hipSuccess) return -2;
  Id128 id; std::memcpy(id.b, id128, 128);
  if (g_rccl.CommInitRank(&g_rccl.comm, world, id, rank) != 0) { g_rccl.comm = nullptr; return -3; }
  if (hipStreamCreate(&g_rccl.stream) != hipSuccess) return -2;
  g_rccl.world = world; g_rccl.rank = rank; g_rccl.device = device;
  return 0;
}
int miqp_comm_finalize(void) {
  std::lock_guard<std::mutex> lk(g_rccl_mu);
  if (g_rccl.comm) { g_rccl.CommDestroy(g_rccl.comm); g_rccl.comm = nullptr; }
  if (g_rccl.dbuf) { (void)hipFree(g_rccl.dbuf); g_rccl.dbuf = nullptr; g_rccl.dcap = 0; }
  if (g_rccl.stream) { (void)hipStreamDestroy(g_rccl.stream); g_rccl.stream = nullptr; }
  return 0;
}
int miqp_comm_selftest(miqp_exchange_fn exchange, void* user, int world, int rank) {
  if (!exchange) { if (!g_rccl.comm) return -1; exchange = rccl_exchange; world = g_rccl.world; rank = g_rccl.rank; }
  // all-reduce(min) of unsigned words: one word that is smallest on the last rank, one on rank 0, one with the top bit set
  unsigned long long w[3] = {1000ull - (unsigned long long)rank, 5ull + (unsigned long long)rank, 0x8000000000000000ull + (unsigned long long)(world - rank)};
  if (exchange(user, 0, w, 3, 0) != 0) return -2;
  if (w[0] != 1000ull - (unsigned long long)(world - 1) || w[1] != 5ull || w[2] != 0x8000000000000001ull) return -3;
  for (int root = 0; root < world; ++root) {
    unsigned char b[37]; for (int k = 0; k < 37; ++k) b[k] = (unsigned char)(rank == root ? (7 * k + root) & 255 : 0xEE);
    if (exchange(user, 1, b, 37, root) != 0) return -4;
    for (int k = 0; k < 37; ++k) if (b[k] != (unsigned char)((7 * k + root) & 255)) return -5;
  }
  return 0;
}
int miqp_solver_solve_split_rccl(miqp_solver_t* s, double timestamp) {
  if (!g_rccl.comm || !s) return MIQP_STATUS_FAILED_SEG_FAULT;
  s->opts.device = g_rccl.device;
  return miqp_solver_solve_split(s, timestamp, g_rccl.world, g_rccl.rank, rccl_exchange, nullptr);
}

int miqp_solver_raw_sizes(const miqp_solver_t* s, int* out4) {
  if (!s || !s->has_inst || !out4) return -1;
  raw_sizes(s->inst, out4[0], out4[1], out4[2], out4[3]);
  return 0;
}

int miqp_solver_lift_tables(const miqp_solver_t* s, double* out, int cap) {
  if (!s || !s->has_inst || !out) return -1;
  miqp_solver_t* one[1] = {const_cast<miqp_solver_t*>(s)};
  BatchShape bs = batch_layout(one, 1);
  if (!bs.ok) return -2;
  const int n = bs.Y.C * 2 * bs.Y.N * 16;
  if (cap < n) return -3;
  std::vector<double> D(bs.Y.dstride, 0.0);
  lift_tables(s->inst, bs.Y, D.data());
  std::copy(D.begin() + bs.Y.d_lift, D.begin() + bs.Y.d_lift + n, out);
  return n;
}

int miqp_solver_solve(miqp_solver_t* s, double timestamp) {
  (void)timestamp;
  if (!s || !s->has_inst) return MIQP_STATUS_FAILED_SEG_FAULT;
  miqp_solver_t* one[1] = {s}; int st = MIQP_STATUS_FAILED_SEG_FAULT;
  if (!solve_batch_impl(one, 1, &st)) return MIQP_STATUS_FAILED_SEG_FAULT;
  return st;
}

int miqp_solver_last_admission(const miqp_solver_t* s, double* out1) { if (!s || !out1) return -1; out1[0] = s->admit_s; return 0; }

const char* miqp_solver_last_error(const miqp_solver_t* s) { return s ? s->err.c_str() : "null handle"; }

int miqp_solver_get_results(const miqp_solver_t* s, miqp_raw_results_c* out) {
  if (!s || !out || !s->has_sol) return -1;
  if (!dims_match(*out, s->inst)) return -2;   // the caller's record must be sized for this instance
  if (s->rescache) { out->N = s->rescache->r.N; out->NrEnvironments = s->rescache->r.NrEnvironments; out->NrRegions = s->rescache->r.NrRegions; out->NrObstacles = s->rescache->r.NrObstacles;
                     out->MaxLinesObstacles = s->rescache->r.MaxLinesObstacles; out->NrCarToCarCollisions = s->rescache->r.NrCarToCarCollisions; out->NrCars = s->rescache->r.NrCars;
                     s->rescache->copy_to(*out); return 0; }
  std::vector<double> D(s->lay.dstride); std::vector<int> T(s->lay.istride);
  compile_instance(s->inst, s->lay, D.data(), T.data());
  fill_results(s->inst, s->lay, D.data(), T.data(), s->comp.data(), s->Z.data(), out);
  return 0;
}

int miqp_solver_materialize_results(miqp_solver_t* const* solvers, int n, int threads) {
  if (!solvers || n < 0) return -1;
  int nth = threads > 0 ? threads : std::min((int)std::thread::hardware_concurrency(), 32);   // (20 480 records on a 2 x 64-core host: 0.29 / 0.16 / 0.13 / 0.15 / 0.25 s at 8 / 16 / 32 / 64 / 256 threads)
  nth = std::max(1, std::min(nth, std::max(1, n / 4)));
  std::atomic<int> next{0}, made{0};
  auto work = [&] {
    std::vector<double> D; std::vector<int> T;   // (one pair of table buffers per thread, not per record)
    for (int k = next.fetch_add(1); k < n; k = next.fetch_add(1)) {
      miqp_solver* s = solvers[k];
      if (!s || !s->has_sol || s->rescache) continue;
      std::unique_ptr<OwnedResults> R(new OwnedResults(s->inst));
      D.resize(s->lay.dstride); T.resize(s->lay.istride);
      compile_instance(s->inst, s->lay, D.data(), T.data());
      fill_results(s->inst, s->lay, D.data(), T.data(), s->comp.data(), s->Z.data(), &R->r);
      s->rescache = std::move(R); made.fetch_add(1);
    }
  };
  if (nth <= 1) work();
  else { std::vector<std::thread> th; for (int t = 0; t < nth; ++t) th.emplace_back(work); for (auto& t : th) t.join(); }
  return made.load();
}

int miqp_solver_get_properties(const miqp_solver_t* s, miqp_solution_properties_c* out) {
  if (!s || !out) return -1;
  *out = s->props;
  return 0;
}

int miqp_solver_last_timing(const miqp_solver_t* s, double* out6) {
  if (!s || !out6) return -1;
  for (int k = 0; k < 6; ++k) out6[k] = s->timing[k];
  return 0;
}

int miqp_solver_last_active_set(const miqp_solver_t* s, double* out8) {
  if (!s || !out8) return -1;
  for (int k = 0; k < 8; ++k) out8[k] = s->as_timing[k];
  return 0;
}

int miqp_solver_last_fixed_route(const miqp_solver_t* s) { return s ? s->fixed_route : -1; }

int miqp_gpu_has_active_set(int num_cars, int num_steps) { return miqp::as_shape_ok(num_cars, num_steps) ? 1 : 0; }

int miqp_solver_launch_plan(const miqp_solver_t* s, int bc, int overlap, int par, const int* cls_n3, int cus, double free_gb, int flags, int* out, int cap) {
  if (!s || !s->has_inst || !cls_n3 || !out || bc < 1 || cus < 1 || free_gb <= 0) return -1;
  miqp_solver_t* one[1] = {const_cast<miqp_solver_t*>(s)};
  const BatchShape bs = batch_layout(one, 1);
  if (!bs.ok) return -2;
  const CallSwitches sw = read_call_switches(); const CtxSwitches cs = read_ctx_switches(); const ProcessSwitches& ps = process_switches();
  const CallShape sh = plan_call(bs.Y, s->opts, 1, 0, 1, false, sw);
  const CtxSizes Z = ctx_sizes(bs.Y, 1, sh.NS, sh.open_cap, sh.npr, sh.MAXR, sh.clamp_open, 1, true, (size_t)(free_gb * 1073741824.0), cus, cs);
  const PlanCaps caps = {Z.oc_grid, Z.ocb_grid, Z.probe_grid, Z.ipm_grid_max, Z.concurrent_big && !(flags & 2), Z.as_cap && (flags & 1), true, true, true, true};
  const PlanSwitches psw = {ps.big_grid_cap, ps.big_w1, ps.big_w2, sw.big_pad, cs.as_chunk, cs.as_quota};
  const RoundPlan P = plan_node_launches(bs.Y, caps, psw, cls_n3, bc, overlap != 0, par);
  if ((size_t)cap * sizeof(int) < (size_t)P.n * sizeof(NodeLaunch)) return -3;
  std::memcpy(out, P.l, (size_t)P.n * sizeof(NodeLaunch));
  return P.n;
}

int miqp_solver_last_setup(const miqp_solver_t* s, double* out3) {
  if (!s || !out3) return -1;
  for (int k = 0; k < 3; ++k) out3[k] = s->setup[k];
  return 0;
}

int miqp_solver_export_lp(const miqp_solver_t* s, const char* path) {
  if (!s || !s->has_inst || !path) return -1;
  return miqp::export_lp(s->inst, path);
}

// ---------------------------------------------------------------- planner core (rows f1 / f2 of SURVEY.md section 8)
int miqp_fraction_parameters(int nr_regions, float max_velocity_fitting, double* out) {
  if (nr_regions < 1 || !out) return -1;
  miqp::fraction_parameters(nr_regions, max_velocity_fitting, out); return 0;
}
int miqp_fitting_polynomial_parameters(int nr_regions, float max_velocity_fitting, float min_velocity_fitting, double* out) {
  if (nr_regions < 1 || !out) return -1;
  return miqp::fitting_polynomial_parameters(nr_regions, max_velocity_fitting, min_velocity_fitting, out) ? 0 : -2;
}
int miqp_mean_angles(const double* fraction_parameters, int nr_regions, double* out) {
  if (!fraction_parameters || nr_regions < 1 || !out) return -1;
  miqp::mean_angles(fraction_parameters, nr_regions, out); return 0;
}
int miqp_limits_per_region(const double* fraction_parameters, int nr_regions, float long_min, float long_max, float lat_min, float lat_max,
                           double* min_x, double* max_x, double* min_y, double* max_y) {
  if (!fraction_parameters || nr_regions < 1 || !min_x || !max_x || !min_y || !max_y) return -1;
  miqp::limits_per_region(fraction_parameters, nr_regions, long_min, long_max, lat_min, lat_max, min_x, max_x, min_y, max_y); return 0;
}
int miqp_calculate_region_idx(const double* fraction_parameters, int nr_regions, float vx, float vy, int* out) {
  if (!fraction_parameters || nr_regions < 1 || !out) return -1;
  return miqp::calculate_region_idx(fraction_parameters, nr_regions, vx, vy, out);
}
int miqp_reserve_neighbor_regions(int* row, int nr_regions, int expansions) {
  if (!row || nr_regions < 1) return -1;
  return miqp::reserve_neighbor_regions(row, nr_regions, expansions) ? 1 : 0;
}
int miqp_calculate_possible_regions(const double* fraction_parameters, int nr_regions, const double* theta_ref, int n, int* flags) {
  if (!fraction_parameters || nr_regions < 1 || !theta_ref || !flags) return -1;
  miqp::calculate_possible_regions(fraction_parameters, nr_regions, theta_ref, n, flags); return 0;
}
int miqp_reference_trajectory(const double* ref_xy, int n_ref, const double* state5, double dt, int num_points, double line_interp_inc, double vel_desired,
                              double delta_s_desired, double acc_lat_max, int vel_curve_dep, double* out) {
  if (!ref_xy || n_ref < 2 || !state5 || num_points < 1 || !out || !(dt > 0) || delta_s_desired < 0) return -1;
  miqp::PolyLine line; line.build(ref_xy, n_ref);
  if (line.x.size() < 2) return -2;
  miqp::reference_trajectory(line, state5, dt, num_points, line_interp_inc, vel_desired, delta_s_desired, acc_lat_max, vel_curve_dep != 0, out);
  return 0;
}
int miqp_update_car(const double* settings12, const double* fraction_parameters, const double* initial_state6, const double* ref_xy, int n_ref, double desired_velocity,
                    double delta_s_desired, double timestep, int track_reference_positions, int is_ego, int num_cars, double* ref4N, int* possible_region, double* weights8) {
  if (!settings12 || !fraction_parameters || !initial_state6 || !ref_xy || n_ref < 2 || !ref4N || !possible_region || !weights8 || num_cars < 1) return -1;
  miqp::CarUpdateSettings S{(int)settings12[0], (int)settings12[1], (int)settings12[2], (int)settings12[3], settings12[4], settings12[5], settings12[6], settings12[7],
                            settings12[8], settings12[9], settings12[10], settings12[11]};
  if (S.nr_regions < 1 || S.nr_steps < 2 || !(S.ts > 0)) return -1;
  return miqp::update_car(S, fraction_parameters, initial_state6, ref_xy, n_ref, desired_velocity, delta_s_desired, timestep, track_reference_positions != 0, is_ego != 0,
                          num_cars, ref4N, possible_region, weights8) ? 0 : 1;
}
int miqp_calculate_warmstart(const miqp_raw_results_c* last, miqp_raw_results_c* out, double ts, double minimum_region_change_speed) {
  if (!last || !out || last->N != out->N || last->NrCars != out->NrCars || last->NrRegions != out->NrRegions || last->N < 2) return -1;
  miqp::calculate_warmstart(*last, *out, ts, minimum_region_change_speed); return 0;
}

int miqp_initial_pose_check(const miqp_model_params_c* p) {
  if (!p || p->NumCars < 1 || !p->IntitialState || !p->WheelBase || (p->nr_environments > 0 && (!p->env_offsets || !p->env_vertices))) return -2;
  return miqp::initial_pose_check(*p);
}
int miqp_select_environment(const double* pieces_xy, const int* piece_off, int n_pieces, const double* traj_xy, const int* traj_off, int n_traj, int* selected) {
  if (n_pieces < 0 || n_traj < 0 || (n_pieces > 0 && (!pieces_xy || !piece_off || !selected)) || (n_traj > 0 && (!traj_xy || !traj_off))) return -1;
  int cnt = 0;
  for (int e = 0; e < n_pieces; ++e) {
    bool hit = false;
    for (int t = 0; t < n_traj && !hit; ++t) hit = miqp::polyline_hits_convex(traj_xy + 2 * traj_off[t], traj_off[t + 1] - traj_off[t], pieces_xy + 2 * piece_off[e], piece_off[e + 1] - piece_off[e]);
    selected[e] = hit ? 1 : 0; cnt += hit ? 1 : 0;
  }
  return cnt;
}
int miqp_obstacle_intersects_environment(const double* pieces_xy, const int* piece_off, int n_pieces, const double* obstacle_xy, int n_steps, int is_static) {
  if (n_pieces < 0 || n_steps < 1 || !obstacle_xy || (n_pieces > 0 && (!pieces_xy || !piece_off))) return -1;
  return miqp::obstacle_intersects_environment(pieces_xy, piece_off, n_pieces, obstacle_xy, n_steps, is_static != 0) ? 1 : 0;
}
int miqp_bark_trajectory(const miqp_raw_results_c* results, int car, double start_time, double ts, double min_speed, double* out_rows5) {
  if (!results || !out_rows5 || car < 0 || car >= results->NrCars || results->N < 0 || !results->vel_x || !results->vel_y || !results->pos_x || !results->pos_y) return -1;
  return miqp::bark_trajectory(*results, car, start_time, ts, min_speed, out_rows5);
}
int miqp_obstacles_roi(double x, double y, double theta, double behind_distance, double front_distance, double side_distance, double* roi_xy) {
  if (!roi_xy) return -1;
  miqp::obstacles_roi(x, y, theta, behind_distance, front_distance, side_distance, roi_xy);
  return 0;
}
int miqp_obstacle_intersects_environment_roi(const double* pieces_xy, const int* piece_off, int n_pieces, const double* obstacle_xy, int n_steps, int is_static, const double* roi_xy) {
  if (n_pieces < 0 || n_steps < 1 || !obstacle_xy || (n_pieces > 0 && (!pieces_xy || !piece_off))) return -1;
  return miqp::obstacle_intersects_environment(pieces_xy, piece_off, n_pieces, obstacle_xy, n_steps, is_static != 0, roi_xy) ? 1 : 0;
}
int miqp_environment_warmstart(const miqp_raw_results_c* last, miqp_raw_results_c* out, const int* ids_old, int n_old, const int* ids_new, int n_new) {
  if (!last || !out || n_old < 0 || n_new < 0 || last->NrEnvironments != n_old || out->NrEnvironments != n_new || last->N != out->N || last->NrCars != out->NrCars) return -1;
  const int* const in[5] = {last->notWithinEnvironmentRear, last->notWithinEnvironmentFrontUbUb, last->notWithinEnvironmentFrontLbUb, last->notWithinEnvironmentFrontUbLb, last->notWithinEnvironmentFrontLbLb};
  int* const o[5] = {out->notWithinEnvironmentRear, out->notWithinEnvironmentFrontUbUb, out->notWithinEnvironmentFrontLbUb, out->notWithinEnvironmentFrontUbLb, out->notWithinEnvironmentFrontLbLb};
  miqp::environment_warmstart(in, o, last->NrCars, last->N, ids_old, n_old, ids_new, n_new);
  return 0;
}

// MiqpPlanner::Plan, the part between the environment update and the trajectory read-out (src/miqp_planner.cpp:634-645,
// 692-766): initial regions of every car from its initial velocity, all combinations, one solve per combination until
// one succeeds; the start region is made possible for the attempt and rolled back when the attempt fails.
int miqp_plan(miqp_solver_t* s, miqp_model_params_c* p, int* initial_region, int* possible_region, const miqp_raw_results_c* warmstart, int warmstart_type,
              double timestamp, int* status_out) {
  if (!s || !p || !initial_region || !possible_region || p->NumCars < 1 || p->nr_regions < 1) return 0;
  p->initial_region = initial_region; p->possible_region = possible_region;
  const int C = p->NumCars, R = p->nr_regions;
  // with an environment: every car's rear and front axle point must lie within one of its pieces, else Plan fails before any
  // solve (src/miqp_planner.cpp:654-685)
  if (p->nr_environments > 0 && p->env_offsets && p->env_vertices && p->WheelBase) {
    const int bad = miqp::initial_pose_check(*p);
    if (bad >= 0) { std::fprintf(stderr, "[miqp_gpu] Initial pose %s collides for car idx = %d\n", (bad & 1) ? "front" : "rear", bad >> 1); if (status_out) *status_out = MIQP_STATUS_FAILED_NO_SOLUT; return 0; }
  }
  std::vector<std::vector<int>> per_car(C), combos;
  std::vector<int> idx(R);
  for (int c = 0; c < C; ++c) {
    int m = miqp::calculate_region_idx(p->fraction_parameters, R, (float)p->IntitialState[c * 6 + 1], (float)p->IntitialState[c * 6 + 4], idx.data());
    per_car[c].assign(idx.begin(), idx.begin() + m);
    if (m < 1) return 0;
  }
  miqp::region_combinations(per_car, combos);
  int status = MIQP_STATUS_FAILED_NO_SOLUT;
  std::vector<char> rollback(C, 0);
  for (auto& comb : combos) {
    for (int c = 0; c < C; ++c) {
      initial_region[c] = comb[c] + 1;   // OPL is 1-based
      if (possible_region[c * R + comb[c]] == 0) { possible_region[c * R + comb[c]] = 1; rollback[c] = 1; } else rollback[c] = 0;
    }
    if (miqp_solver_set_params(s, p) != 0) { status = MIQP_STATUS_FAILED_SEG_FAULT; break; }
    if ((warmstart_type == MIQP_WARMSTART_RECEDING_HORIZON || warmstart_type == MIQP_WARMSTART_BOTH) && warmstart)
      miqp_solver_set_warmstart(s, warmstart, warmstart_type);
    status = miqp_solver_solve(s, timestamp);
    if (status == MIQP_STATUS_SUCCESS) break;
    if (status == MIQP_STATUS_FAILED_SEG_FAULT || status == MIQP_STATUS_FAILED_TIMEOUT) break;
    for (int c = 0; c < C; ++c) if (rollback[c]) possible_region[c * R + comb[c]] = 0;
  }
  if (status_out) *status_out = status;
  return status == MIQP_STATUS_SUCCESS ? 1 : 0;
}


int miqp_solver_write_dat(const miqp_solver_t* s, const char* path) {
  if (!s || !s->has_inst || !path) return -1;
  FILE* f = std::fopen(path, "w"); if (!f) return -2;
  bool ok = miqp::write_dat(s->inst, f);
  return (std::fclose(f) == 0 && ok) ? 0 : -3;
}

int miqp_solver_write_solution(const miqp_solver_t* s, const char* path) {
  if (!s || !s->has_sol || !path) return -1;
  OwnedResults R(s->inst);
  if (miqp_solver_get_results(s, &R.r) != 0) return -2;
  FILE* f = std::fopen(path, "w"); if (!f) return -2;
  bool ok = miqp::write_solution(R.r, s->props.objective, f);
  return (std::fclose(f) == 0 && ok) ? 0 : -3;
}

int miqp_solver_write_mst(const miqp_solver_t* s, const char* path) {
  if (!s || !s->has_sol || !path) return -1;
  OwnedResults R(s->inst);
  if (miqp_solver_get_results(s, &R.r) != 0) return -2;
  FILE* f = std::fopen(path, "w"); if (!f) return -2;
  bool ok = miqp::write_mst(R.r, s->props.objective, f);
  return (std::fclose(f) == 0 && ok) ? 0 : -3;
}

int miqp_solver_read_mst(miqp_solver_t* s, const char* path) {
  if (!s || !s->has_inst || !path) return -1;
  OwnedResults R(s->inst);
  if (miqp::read_mst(path, R.r) <= 0) return -2;
  return miqp_solver_set_warmstart(s, &R.r, MIQP_WARMSTART_LAST_SOLUTION);
}

int miqp_solver_solve_fixed(miqp_solver_t* s, const miqp_raw_results_c* fixed, miqp_raw_results_c* out, double* objective, int* iterations) {
  if (s) s->fixed_route = -1;   // (a call that returns before its launches leaves no route of an earlier one behind)
  if (!s || !s->has_inst || !fixed) return -1;
  miqp_solver_t* one[1] = {s};
  BatchShape bs = batch_layout(one, 1);
  if (!bs.ok) return -2;
  const Layout& Y = bs.Y;
  if (!dims_match(*fixed, s->inst) || (out && !dims_match(*out, s->inst))) return -2;
  DevCtx* Xp = ctx_for_device(s->opts.device);
  if (!Xp) return -3;
  DevCtx& X = *Xp;
  std::lock_guard<std::mutex> ctx_lock(X.mu);
  if (!ctx_prepare(X, Y, 1, 1, 64, 16, 3)) return -3;
  if (!set_kernel_lds(Y, ipm_lds_bytes(Y), eval_lds_bytes(Y, read_call_switches().seq_kinds))) return -3;
  std::vector<double> D(Y.dstride); std::vector<int> T(Y.istride);
  compile_instance(s->inst, Y, D.data(), T.data());
  std::vector<signed char> fix;
  if (!fix_from_results(s->inst, Y, T.data(), fixed, fix)) return -4;
  DevBuf& B = X.B; hipStream_t st = X.stream;
  int one_i = 1, zero = 0;
  if (hipMemcpyAsync((void*)B.inst_d, D.data(), D.size() * 8, hipMemcpyHostToDevice, st) != hipSuccess) return -3;
  (void)hipMemcpyAsync((void*)B.inst_i, T.data(), T.size() * 4, hipMemcpyHostToDevice, st);
  (void)hipMemcpyAsync(B.pool_fix, fix.data(), Y.fixlen, hipMemcpyHostToDevice, st);
  (void)hipMemcpyAsync(B.batch_count, &one_i, 4, hipMemcpyHostToDevice, st);
  (void)hipMemcpyAsync(B.batch_node, &zero, 4, hipMemcpyHostToDevice, st);
  (void)hipMemcpyAsync(B.batch_inst, &zero, 4, hipMemcpyHostToDevice, st);
  (void)hipMemsetAsync(B.inst_nodes, 0, 8, st); (void)hipMemsetAsync(B.inst_iters, 0, 8, st); (void)hipMemsetAsync(B.stat_rowiters, 0, 8, st);
  { DevBuf Bp = B; Bp.qp_tol = QP_TOL_FINAL; Bp.use_cutoff = 0; Bp.ws_on = 0;
    launch_ipm_batch(X, Bp, 1, st); }
  std::vector<double> Z((size_t)Y.N * Y.nz); double obj = 0, viol = 0; int ok = 0, it = 0;
  (void)hipMemcpyAsync(Z.data(), B.batch_Z, Z.size() * 8, hipMemcpyDeviceToHost, st);
  (void)hipMemcpyAsync(&obj, B.batch_obj, 8, hipMemcpyDeviceToHost, st);
  (void)hipMemcpyAsync(&viol, B.batch_viol, 8, hipMemcpyDeviceToHost, st);
  (void)hipMemcpyAsync(&ok, B.batch_ok, 4, hipMemcpyDeviceToHost, st);
  (void)hipMemcpyAsync(&it, B.batch_it, 4, hipMemcpyDeviceToHost, st);
  // the hand-over counters of the serial chain say which of its launches solved the node (with one node in the batch each is 0 or 1)
  int ovf = 0, ovf2 = 0;
  if (X.oc_grid > 0) {
    (void)hipMemcpyAsync(&ovf, B.ovf_count, 4, hipMemcpyDeviceToHost, st);
    if (X.ocb_grid > 0) (void)hipMemcpyAsync(&ovf2, B.ovf2_count, 4, hipMemcpyDeviceToHost, st);
  }
  if (hipStreamSynchronize(st) != hipSuccess || hipGetLastError() != hipSuccess) return -3;
  s->fixed_route = X.oc_grid <= 0 ? 3 : ovf == 0 ? 0 : (X.ocb_grid > 0 && ovf2 == 0) ? 1 : 2;
  HostGeo G{s->inst, Y, D.data(), T.data()}; double cobj = 0; (void)step0_check(G, cobj);
  // the points the record ignores cost WEIGHTS_SLACK_OBSTACLE each: a constant no node kernel charges (eval_kernel adds it for the search, soft_cost of
  // fixed_chain.hip for the batch calls, in this order of operations)
  int nign = 0; for (int q = 0; q < Y.C * Y.O * Y.N * 5; ++q) nign += fix[Y.f_obs + q] >= Y.L;
  // (the product is ROUNDED before the sum, as __dmul_rn rounds it in soft_cost: the volatile keeps a host compiler that may fuse - an FMA target
  // with fp-contract on - from doing so, or the batch calls would differ from this one in the last bit)
  volatile double soft = nign > 0 ? (double)nign * D[Y.d_misc + 1] : 0.0;
  const double konst = cobj + soft;
  if (objective) *objective = obj + konst;
  if (iterations) *iterations = it;
  if (!ok || viol > FEAS_TOL) return 1;
  if (out) {
    // undecided leaf disjunctions: canonical completion is done by fill_results (it evaluates every side)
    for (auto& b : fix) if (b < 0) b = 0;
    fill_results(s->inst, Y, D.data(), T.data(), fix.data(), Z.data(), out);
  }
  return 0;
}

}  // extern "C"

// fixed_batch.hip - many fixed-binary QPs of ONE instance in one device call (miqp_solver_solve_fixed_batch, _fixed_batch_record).
//
// The question miqp_solver_solve_fixed answers for one record - the best continuous trajectory under its integer decisions, and its cost - asked
// for n records of the instance the handle holds.  No reference counterpart as an entry point: the reference walks its alternative start
// configurations one after the other, one cplex.solve() each (src/miqp_planner.cpp:694-749); a caller that enumerates manoeuvres - left or right
// of each obstacle, before or after the other car - asks it hundreds of times for one instance.
//
// Host side: one compile_instance, one upload of the tables and one device lock for the call.  The accepted entries (records of the instance's
// shape; the others are status 2 and never reach the device) are numbered 0 .. m - 1 in the caller's order - their index in the call - and go through
// the serial interior point chain of solve_fixed (launch_ipm_batch: standard on-chip block, larger block, memory-backed kernel) in chunks of
// FB_CHUNK nodes: node k of a chunk is batch slot k, instance 0, fix record at slot k of pool_fix, with the settings of the single call (QP_TOL_FINAL,
// no cutoff, cold start).  The fix records of chunk j + 1 travel through pinned staging to a device staging buffer on a second stream while the
// launches of chunk j run; the solver stream copies them into pool_fix when that chain has ended.  What the chain keeps per slot or per launch is
// reset per chunk: the hand-over counts (by the launches themselves), the size marks of the slots' records (pool_big), the launch split and the
// depth words of the slots (batch_large, batch_depth: an earlier solve's may lie there) and the per-instance counters.
//
// Kernel: one launch per chunk, behind the chain on the solver stream, makes the chunk's outcome one compact download.  Workgroup 0 derives the
// route of every node from the chain's hand-over lists (the rule of solve_fixed), writes one miqp_fixed_result_c per node at its index in the
// call and reduces (objective, index) over the feasible nodes - xor tree per wavefront, four-entry LDS step across them, ties to the lower index.
// The wavefronts of the other workgroups copy the trajectory rows, one row per wavefront at a time, as 16-byte loads and stores.  No atomics, no scratch.
#pragma once

namespace {

constexpr int FB_CHUNK = 1024;    // nodes per launch group (miqp_gpu_fixed_batch_chunk): four per CU of the standard on-chip launch, one download of 32 KB + the rows
constexpr int FB_CAP = 65536;     // entries per call (include/miqp_gpu.h)
constexpr int FB_NT = 256;
constexpr int FB_ROW_BLOCKS = 256;

// The price of the obstacle points a fix record ignores (byte L at a point of a soft obstacle: WEIGHTS_SLACK_OBSTACLE each, a constant of the node's
// QP).  No node kernel charges it - eval_kernel adds it for the search - so the collect kernels do, from the chunk's fix records in pool_fix.
struct SoftCost {
  const signed char* fix;     // slot 0 of pool_fix: node k of a chunk is slot k
  const double* inst_d;       // the instances' tables (the weight is D[d_w] of the node's instance)
  int fixlen, f_obs, n_obs, L, dstride, d_w;   // n_obs = C * O * N * 5 bytes from f_obs on
};

__device__ inline double soft_cost(const SoftCost& S, int k, int inst) {
  const signed char* f = S.fix + (size_t)k * S.fixlen + S.f_obs;
  int n = 0;
  for (int q = 0; q < S.n_obs; ++q) n += f[q] >= S.L ? 1 : 0;
  return n > 0 ? __dmul_rn((double)n, S.inst_d[(size_t)inst * S.dstride + S.d_w]) : 0.0;   // (a rounded product, never fused into the sum: the bits of the host's in miqp_solver_solve_fixed)
}

struct FixedBatchArgs {
  const int* ovf_list; const int* ovf_count; const int* ovf2_list; const int* ovf2_count;
  const int* batch_ok; const int* batch_it; const double* batch_obj; const double* batch_viol; const double* batch_Z;
  miqp_fixed_result_c* res;   // of the chunk's first node
  double* Z;                  // idem: [bc][row_doubles]
  double* best_obj; int* best_idx;   // the chunk's minimum
  int bc, base, row_doubles;  // nodes of the chunk, index in the call of its first node, N * nz (even: nz = 8 per car)
  int onchip, big;            // the shape has the on-chip kernel / its larger variant
  double cobj;                // constant cost of step 0 (step0_check)
  SoftCost soft;
};

__global__ __launch_bounds__(FB_NT) void fixed_batch_collect_kernel(const FixedBatchArgs A) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  if (blockIdx.x > 0) {   // trajectory rows: batch slot -> index in the call
    const int nw = ((int)gridDim.x - 1) * (FB_NT / 64), row2 = A.row_doubles >> 1;
    for (int node = ((int)blockIdx.x - 1) * (FB_NT / 64) + wave; node < A.bc; node += nw) {
      const double2* src = (const double2*)(A.batch_Z + (size_t)node * A.row_doubles);
      double2* dst = (double2*)(A.Z + (size_t)node * A.row_doubles);
      for (int q = lane; q < row2; q += 64) dst[q] = src[q];
    }
    return;
  }
  miqp_fixed_result_c* const R = A.res;
  // pass 1: the launch of the chain that solved each node, from its hand-over lists (miqp_solver_solve_fixed: 3 without an on-chip kernel, else 0,
  // 1 when the standard block handed the node on, 2 when the larger one did too - or when there is no larger one)
  for (int k = tid; k < A.bc; k += FB_NT) R[k].route = A.onchip ? 0 : 3;
  __syncthreads();
  if (A.onchip) {
    const int n1 = min(*A.ovf_count, A.bc);
    for (int q = tid; q < n1; q += FB_NT) { const int node = A.ovf_list[q]; if ((unsigned)node < (unsigned)A.bc) R[node].route = A.big ? 1 : 2; }
    __syncthreads();
    if (A.big) {
      const int n2 = min(*A.ovf2_count, A.bc);
      for (int q = tid; q < n2; q += FB_NT) { const int node = A.ovf2_list[q]; if ((unsigned)node < (unsigned)A.bc) R[node].route = 2; }
    }
  }
  // pass 2: verdict, objective, iterations and violation of each node; the lane's best feasible one (its nodes ascend: a tie keeps the lower index)
  double bo = 1e308; int bi = 0x7FFFFFFF;
  for (int k = tid; k < A.bc; k += FB_NT) {
    const int ok = A.batch_ok[k]; const double viol = A.batch_viol[k], obj = A.batch_obj[k] + (A.cobj + soft_cost(A.soft, k, 0));
    const int st = (!ok || viol > FEAS_TOL) ? 1 : 0;
    R[k].status = st; R[k].iterations = A.batch_it[k]; R[k].reserved = 0; R[k].objective = obj; R[k].violation = viol;
    if (st == 0 && obj < bo) { bo = obj; bi = k; }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const double oo = __shfl_xor(bo, d, 64); const int oi = __shfl_xor(bi, d, 64);
    if (oo < bo || (oo == bo && oi < bi)) { bo = oo; bi = oi; }
  }
  __shared__ double s_o[FB_NT / 64]; __shared__ int s_i[FB_NT / 64];
  if (lane == 0) { s_o[wave] = bo; s_i[wave] = bi; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < FB_NT / 64; ++w) if (s_o[w] < bo || (s_o[w] == bo && s_i[w] < bi)) { bo = s_o[w]; bi = s_i[w]; }
    *A.best_obj = bo; *A.best_idx = bi == 0x7FFFFFFF ? -1 : A.base + bi;
  }
}

// ---------------------------------------------------------------------------------------------------------------- device cache
// staging and result buffers of the batch call, cached per device and never taken from the solver's pools (grown, not shrunk)
struct FixedBatchDev {
  hipStream_t s_up = nullptr; hipEvent_t ev_up[2] = {}, ev_taken[2] = {};
  signed char* h_stage[2] = {nullptr, nullptr}; signed char* d_stage[2] = {nullptr, nullptr}; size_t stage_cap = 0;
  miqp_fixed_result_c* d_res = nullptr; double* d_best_obj = nullptr; int* d_best_idx = nullptr; size_t res_cap = 0;
  double* d_Z = nullptr; size_t z_cap = 0;
  bool ensure(size_t stage_bytes, size_t n, size_t z_doubles) {
    if (!s_up) {
      HIP_OK(hipStreamCreateWithFlags(&s_up, hipStreamNonBlocking));
      for (int b = 0; b < 2; ++b) { HIP_OK(hipEventCreateWithFlags(&ev_up[b], hipEventDisableTiming)); HIP_OK(hipEventCreateWithFlags(&ev_taken[b], hipEventDisableTiming)); }
    }
    if (stage_bytes > stage_cap) {
      for (int b = 0; b < 2; ++b) { if (h_stage[b]) (void)hipHostFree(h_stage[b]); if (d_stage[b]) (void)hipFree(d_stage[b]); h_stage[b] = nullptr; d_stage[b] = nullptr; }
      stage_cap = 0;
      for (int b = 0; b < 2; ++b) { HIP_OK(hipHostMalloc((void**)&h_stage[b], stage_bytes, hipHostMallocDefault)); HIP_OK(hipMalloc((void**)&d_stage[b], stage_bytes)); }
      stage_cap = stage_bytes;
    }
    if (n > res_cap) {
      if (d_res) (void)hipFree(d_res); if (d_best_obj) (void)hipFree(d_best_obj); if (d_best_idx) (void)hipFree(d_best_idx);
      d_res = nullptr; d_best_obj = nullptr; d_best_idx = nullptr; res_cap = 0;
      size_t want = 1024; while (want < n) want <<= 1;
      HIP_OK(hipMalloc((void**)&d_res, want * sizeof(miqp_fixed_result_c)));
      HIP_OK(hipMalloc((void**)&d_best_obj, (want / FB_CHUNK + 1) * sizeof(double))); HIP_OK(hipMalloc((void**)&d_best_idx, (want / FB_CHUNK + 1) * sizeof(int)));
      res_cap = want;
    }
    if (z_doubles > z_cap) {
      if (d_Z) (void)hipFree(d_Z);
      d_Z = nullptr; z_cap = 0;
      HIP_OK(hipMalloc((void**)&d_Z, z_doubles * sizeof(double)));
      z_cap = z_doubles;
    }
    return true;
  }
};
std::map<int, FixedBatchDev> g_fixed_batch_dev;   // by device ordinal; used under the device lock (DevCtx::mu of lane 0)

SoftCost soft_cost_args(const DevBuf& B, const Layout& Y) {
  SoftCost S;
  S.fix = B.pool_fix; S.inst_d = B.inst_d; S.fixlen = Y.fixlen; S.f_obs = Y.f_obs; S.n_obs = Y.C * Y.O * Y.N * 5; S.L = Y.L; S.dstride = Y.dstride; S.d_w = Y.d_misc + 1;
  return S;
}

// the int arrays fix_from_results reads
bool fixed_record_ok(const miqp_raw_results_c& r) {
  const void* need[] = {r.notWithinEnvironmentRear, r.notWithinEnvironmentFrontUbUb, r.notWithinEnvironmentFrontLbUb, r.notWithinEnvironmentFrontUbLb, r.notWithinEnvironmentFrontLbLb,
                        r.active_region, r.region_change_not_allowed_x_positive, r.region_change_not_allowed_y_positive, r.region_change_not_allowed_x_negative,
                        r.region_change_not_allowed_y_negative, r.region_change_not_allowed_combined, r.deltacc, r.deltacc_front, r.car2car_collision,
                        r.slackvarsObstacle, r.slackvarsObstacle_front};
  for (const void* q : need) if (!q) return false;
  return true;
}

// the chunks of `fix` (m records) through the chain; tmp[m] and Zout receive the results.  false: HIP error
bool fixed_batch_run(DevCtx& X, FixedBatchDev& G, const Layout& Y, const std::vector<double>& D, const std::vector<int>& T, const std::vector<signed char>& fix, int m, double cobj,
                     std::vector<miqp_fixed_result_c>& tmp, std::vector<double>& Zout, std::vector<double>& best_obj, std::vector<int>& best_idx, float& dev_ms) {
  DevBuf& B = X.B; hipStream_t st = X.stream;
  const size_t fl = (size_t)Y.fixlen, row = (size_t)Y.N * Y.nz;
  const int nch = (m + FB_CHUNK - 1) / FB_CHUNK;
  std::vector<int> ident(FB_CHUNK); for (int k = 0; k < FB_CHUNK; ++k) ident[k] = k;
  HIP_OK(hipMemcpyAsync((void*)B.inst_d, D.data(), D.size() * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync((void*)B.inst_i, T.data(), T.size() * 4, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(B.batch_node, ident.data(), (size_t)FB_CHUNK * 4, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemsetAsync(B.batch_inst, 0, (size_t)FB_CHUNK * 4, st));
  bool used[2] = {false, false};
  auto stage = [&](int j) -> bool {   // fix records of chunk j: pinned staging -> device staging, on the upload stream
    const int p = j & 1, c0 = j * FB_CHUNK, bc = std::min(FB_CHUNK, m - c0);
    if (used[p]) { HIP_OK(hipEventSynchronize(G.ev_up[p])); HIP_OK(hipStreamWaitEvent(G.s_up, G.ev_taken[p], 0)); }   // (chunk j - 2: its upload has left the pinned buffer, its copy into pool_fix the device one)
    std::memcpy(G.h_stage[p], fix.data() + (size_t)c0 * fl, (size_t)bc * fl);
    HIP_OK(hipMemcpyAsync(G.d_stage[p], G.h_stage[p], (size_t)bc * fl, hipMemcpyHostToDevice, G.s_up));
    HIP_OK(hipEventRecord(G.ev_up[p], G.s_up));
    used[p] = true;
    return true;
  };
  if (!stage(0)) return false;
  HIP_OK(hipEventRecord(X.ev0, st));
  DevBuf Bp = B; Bp.qp_tol = QP_TOL_FINAL; Bp.use_cutoff = 0; Bp.ws_on = 0;
  for (int j = 0; j < nch; ++j) {
    if (j + 1 < nch && !stage(j + 1)) return false;
    const int p = j & 1, c0 = j * FB_CHUNK, bc = std::min(FB_CHUNK, m - c0);
    HIP_OK(hipStreamWaitEvent(st, G.ev_up[p], 0));
    HIP_OK(hipMemcpyAsync(B.pool_fix, G.d_stage[p], (size_t)bc * fl, hipMemcpyDeviceToDevice, st));
    HIP_OK(hipEventRecord(G.ev_taken[p], st));
    HIP_OK(hipMemsetD32Async((hipDeviceptr_t)B.batch_count, bc, 1, st));
    // nothing of the chunk before, or of an earlier solve, stays in the slots
    HIP_OK(hipMemsetAsync(B.pool_big, 0, (size_t)bc, st)); HIP_OK(hipMemsetAsync(B.batch_large, 0, (size_t)bc, st)); HIP_OK(hipMemsetAsync(B.batch_depth, 0, (size_t)bc * 4, st));
    HIP_OK(hipMemsetAsync(B.inst_nodes, 0, 8, st)); HIP_OK(hipMemsetAsync(B.inst_iters, 0, 8, st)); HIP_OK(hipMemsetAsync(B.stat_rowiters, 0, 8, st));
    launch_ipm_batch(X, Bp, bc, st);   // (zeroes the hand-over counts of its launches)
    FixedBatchArgs A;
    A.ovf_list = B.ovf_list; A.ovf_count = B.ovf_count; A.ovf2_list = B.ovf2_list; A.ovf2_count = B.ovf2_count;
    A.batch_ok = B.batch_ok; A.batch_it = B.batch_it; A.batch_obj = B.batch_obj; A.batch_viol = B.batch_viol; A.batch_Z = B.batch_Z;
    A.res = G.d_res + c0; A.Z = G.d_Z + (size_t)c0 * row; A.best_obj = G.d_best_obj + j; A.best_idx = G.d_best_idx + j;
    A.bc = bc; A.base = c0; A.row_doubles = (int)row; A.onchip = X.oc_grid > 0 ? 1 : 0; A.big = X.ocb_grid > 0 ? 1 : 0; A.cobj = cobj; A.soft = soft_cost_args(B, Y);
    hipLaunchKernelGGL(fixed_batch_collect_kernel, dim3(1 + std::min(FB_ROW_BLOCKS, (bc + FB_NT / 64 - 1) / (FB_NT / 64))), dim3(FB_NT), 0, st, A);
    HIP_OK(hipGetLastError());
  }
  HIP_OK(hipEventRecord(X.ev1, st));
  tmp.resize(m); Zout.resize((size_t)m * row); best_obj.resize(nch); best_idx.resize(nch);
  HIP_OK(hipMemcpyAsync(tmp.data(), G.d_res, (size_t)m * sizeof(miqp_fixed_result_c), hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(Zout.data(), G.d_Z, (size_t)m * row * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(best_obj.data(), G.d_best_obj, (size_t)nch * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(best_idx.data(), G.d_best_idx, (size_t)nch * 4, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st)); HIP_OK(hipStreamSynchronize(G.s_up)); HIP_OK(hipGetLastError());
  (void)hipEventElapsedTime(&dev_ms, X.ev0, X.ev1);
  return true;
}

// The part of a fixed-batch call that runs PREPARED fix bytes (miqp_solver_solve_fixed_batch; miqp_solver_pool_solve of solution_pool.hip): open() takes the
// device and its lock, brings the context to the sizes of the batch call, compiles the instance and checks its first step; run() sends m fix records of
// Y.fixlen bytes through the chain.  The lock is held until the object goes.  Both return 0 or -3 (no device / kernel image / HIP error)
struct FixedBatchCall {
  miqp_solver_t* s = nullptr; Layout Y{}; DevCtx* X = nullptr; std::unique_lock<std::mutex> lock;
  std::vector<double> D; std::vector<int> T; double cobj = 0;
  int open(miqp_solver_t* s_, const Layout& Y_) {
    s = s_; Y = Y_;
    X = ctx_for_device(s->opts.device);
    if (!X) return -3;
    lock = std::unique_lock<std::mutex>(X->mu);
    bool rebuilt = false; const double t_ctx = wall_s();
    if (!ctx_prepare(*X, Y, 1, 1, 64, FB_CHUNK, 3, false, 1, &rebuilt)) return -3;
    s->setup[1] = wall_s() - t_ctx; s->setup[2] = rebuilt ? 1.0 : 0.0;
    if (X->batch_cap < FB_CHUNK || X->batch_alloc < FB_CHUNK || X->pool_cap < FB_CHUNK) { std::fprintf(stderr, "[miqp_gpu] the device context does not hold a chunk of %d nodes\n", FB_CHUNK); return -3; }
    if (!set_kernel_lds(Y, ipm_lds_bytes(Y), eval_lds_bytes(Y, read_call_switches().seq_kinds))) return -3;
    D.resize(Y.dstride); T.resize(Y.istride);
    compile_instance(s->inst, Y, D.data(), T.data());
    HostGeo G{s->inst, Y, D.data(), T.data()}; (void)step0_check(G, cobj);
    return 0;
  }
  int run(const std::vector<signed char>& fix, int m, std::vector<miqp_fixed_result_c>& tmp, std::vector<double>& Z, std::vector<double>& bo, std::vector<int>& bi, float& dev_ms) {
    FixedBatchDev& F = g_fixed_batch_dev[X->device];
    if (!F.ensure((size_t)FB_CHUNK * Y.fixlen, (size_t)m, (size_t)m * Y.N * Y.nz)) return -3;
    if (!fixed_batch_run(*X, F, Y, D, T, fix, m, cobj, tmp, Z, bo, bi, dev_ms)) { (void)hipStreamSynchronize(X->stream); (void)hipStreamSynchronize(F.s_up); return -3; }
    return 0;
  }
};

}  // namespace

extern "C" {

int miqp_gpu_fixed_result_size(void) { return (int)sizeof(miqp_fixed_result_c); }
int miqp_gpu_fixed_batch_chunk(void) { return FB_CHUNK; }

int miqp_solver_solve_fixed_batch(miqp_solver_t* s, const miqp_raw_results_c* const* fixed, int n, miqp_fixed_result_c* out, int* best) {
  if (s) s->drop_fixed_batch();
  if (!s || !s->has_inst || !fixed || !out || n <= 0) return -1;
  if (n > FB_CAP) return -5;
  const double t_call = wall_s();
  if (best) *best = -1;
  for (int k = 0; k < n; ++k) { out[k].status = 2; out[k].route = -1; out[k].iterations = 0; out[k].reserved = 0; out[k].objective = std::nan(""); out[k].violation = std::nan(""); }
  miqp_solver_t* one[1] = {s};
  BatchShape bs = batch_layout(one, 1);
  if (!bs.ok) return -2;
  const Layout& Y = bs.Y;
  // the accepted entries, in the caller's order: entry where[c] is node c of the call
  std::vector<int> where; where.reserve(n);
  for (int k = 0; k < n; ++k) if (fixed[k] && fixed_record_ok(*fixed[k]) && dims_match(*fixed[k], s->inst)) where.push_back(k);
  const int m = (int)where.size();
  if (m == 0) return 0;   // (nothing to run: no device is touched)
  FixedBatchCall call;
  if (call.open(s, Y) != 0) return -3;
  const std::vector<int>& T = call.T;
  const size_t fl = (size_t)Y.fixlen;
  std::vector<signed char> fix((size_t)m * fl);
  {   // fix records on a few host threads when there are many (at most 16, as everywhere)
    const int nth = std::max(1, std::min({16, process_switches().prep_threads, (int)std::thread::hardware_concurrency(), m / 256}));
    std::atomic<int> next{0};
    auto work = [&] {
      std::vector<signed char> one_fix;
      for (int c = next.fetch_add(1); c < m; c = next.fetch_add(1)) { (void)fix_from_results(s->inst, Y, T.data(), fixed[where[c]], one_fix); std::memcpy(fix.data() + (size_t)c * fl, one_fix.data(), fl); }
    };
    if (nth <= 1) work();
    else { std::vector<std::thread> th; for (int t = 0; t < nth; ++t) th.emplace_back(work); for (auto& t : th) t.join(); }
  }
  s->setup[0] = wall_s() - t_call;
  std::vector<miqp_fixed_result_c> tmp; std::vector<double> Z, bo; std::vector<int> bi; float dev_ms = 0.0f;
  if (call.run(fix, m, tmp, Z, bo, bi, dev_ms) != 0) return -3;
  for (int c = 0; c < m; ++c) out[where[c]] = tmp[c];
  {   // the minimum of the call from the chunks' minima (ascending chunks: a tie keeps the lower index)
    double b = 0; int at = -1;
    for (size_t j = 0; j < bo.size(); ++j) if (bi[j] >= 0 && bi[j] < m && (at < 0 || bo[j] < b)) { b = bo[j]; at = bi[j]; }
    if (best) *best = at < 0 ? -1 : where[at];
  }
  s->fb_n = n; s->fb_slot.assign(n, -1);
  for (int c = 0; c < m; ++c) if (tmp[c].status == 0) s->fb_slot[where[c]] = c;
  s->fb_Z.swap(Z); s->fb_fix.swap(fix);
  const int nch = (m + FB_CHUNK - 1) / FB_CHUNK;
  s->timing[0] = wall_s() - t_call; s->timing[1] = dev_ms * 1e-3; s->timing[2] = nch; s->timing[3] = m; s->timing[4] = 0; s->timing[5] = 0;
  for (int c = 0; c < m; ++c) s->timing[4] += tmp[c].iterations;
  return 0;
}

int miqp_solver_fixed_batch_record(miqp_solver_t* s, int k, miqp_raw_results_c* out) {
  if (!s || !out || !s->has_inst || s->fb_n <= 0 || k < 0 || k >= s->fb_n) return -1;
  const int c = s->fb_slot[k];
  if (c < 0) return 1;
  if (!dims_match(*out, s->inst)) return -2;
  miqp_solver_t* one[1] = {s};
  BatchShape bs = batch_layout(one, 1);
  if (!bs.ok) return -1;
  const Layout& Y = bs.Y;
  std::vector<double> D(Y.dstride); std::vector<int> T(Y.istride);
  compile_instance(s->inst, Y, D.data(), T.data());
  // undecided leaf disjunctions: canonical completion is done by fill_results (it evaluates every side), as in the single call
  std::vector<signed char> fix(s->fb_fix.begin() + (size_t)c * Y.fixlen, s->fb_fix.begin() + (size_t)(c + 1) * Y.fixlen);
  for (auto& b : fix) if (b < 0) b = 0;
  fill_results(s->inst, Y, D.data(), T.data(), fix.data(), s->fb_Z.data() + (size_t)c * Y.N * Y.nz, out);
  return 0;
}

}  // extern "C"

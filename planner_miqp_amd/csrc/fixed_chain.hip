// fixed_chain.hip - fix records through the serial interior point chain, ONCE for every entry point that sends them there: the record calls of
// fixed_batch.hip, the refinement of solution_pool.hip, the climb of pool_improve.hip and the explore of pool_explore.hip.  DESIGN.md 6b.
//
// The node kernels take nodes of many instances in one launch - they read batch_inst[node] and index the instance tables by it, which is how every
// round of the branch and bound runs.  A call here is over n handles (one handle is the case n = 1): one device lock, one context (the common Layout
// of the handles: batch_layout), the n instances compiled on host threads, their tables uploaded once (FixedCall::open).  Its nodes go through the
// chain of solve_fixed (launch_ipm_batch: standard on-chip block, larger block, memory-backed kernel) in chunks of FB_CHUNK: node k of a chunk is
// batch slot k, its fix record slot k of pool_fix, batch_inst[k] the index of its handle in the call, with the settings of the single call
// (QP_TOL_FINAL, no cutoff, cold start).  With use_cutoff = 0 and ws_on = 0 the node kernels read, per instance, their tables (inst_d, inst_i) and the
// incumbent words inc_key / inc_ext, whose value node_cutoff then drops; they add to inst_nodes / inst_iters.  So nothing per instance needs a
// value but the tables.
//
// fixed_chunk is one chunk: what the chain keeps per slot or per launch is reset - the hand-over counts (by the launches themselves), the size marks
// of the slots' records (pool_big), the launch split and the depth words of the slots (batch_large, batch_depth: an earlier solve's may lie there)
// and the counters of the call's instances - then the chain, then fixed_collect_kernel.  Who fills pool_fix and batch_inst is the caller's business:
// fixed_run copies them from staging, the climb and the explore have pool_neighbour_kernel write them.
//
// fixed_run is the chunks of prepared fix bytes, numbered handle-major in the caller's order.  The records of chunk j + 1, their batch_inst slice
// and their segment table travel through pinned staging to a device staging buffer on a second stream while the launches of chunk j run; the solver
// stream copies them into place when that chain has ended.
//
// Kernel: one launch per chunk, behind the chain on the solver stream, makes the chunk's outcome one compact download.  Workgroup 0 derives the
// route of every node from the chain's hand-over lists (the rule of solve_fixed), writes one miqp_fixed_result_c per node - the constant cost of
// step 0 and the price of the ignored obstacle points per node from its instance - and, where the host passes the chunk's segment table (first node
// of every handle present in the chunk), ONE MINIMUM PER SEGMENT: a wavefront takes a segment at a time, reduces (objective, index within the
// handle) over its feasible nodes with the xor tree - ties to the lower index - and writes the pair to the segment's slot.  A handle whose nodes
// straddle chunks gets one partial result per chunk; the host folds them in ascending chunk order.  The wavefronts of the other workgroups copy the
// trajectory rows, one row per wavefront at a time, as 16-byte loads and stores.  No atomics, no LDS, no scratch, nothing that depends on arrival order.
#pragma once

namespace {

constexpr int FB_CHUNK = 1024;    // nodes per launch group (miqp_gpu_fixed_batch_chunk): four per CU of the standard on-chip launch, one download of 32 KB + the rows
constexpr int FB_CAP = 65536;     // entries per call (include/miqp_gpu.h)
constexpr int FB_NT = 256;
constexpr int FB_ROW_BLOCKS = 256;

// The price of the obstacle points a fix record ignores (byte L at a point of a soft obstacle: WEIGHTS_SLACK_OBSTACLE each, a constant of the node's
// QP).  No node kernel charges it - eval_kernel adds it for the search - so the collect kernel does, from the chunk's fix records in pool_fix.
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

struct FixedCollectArgs {
  const int* ovf_list; const int* ovf_count; const int* ovf2_list; const int* ovf2_count;
  const int* batch_ok; const int* batch_it; const double* batch_obj; const double* batch_viol; const double* batch_Z; const int* batch_inst;
  const double* cobj;         // [n_inst] constant cost of step 0 of every handle (step0_check)
  const int* hfirst;          // [n_inst] node of the call that is entry 0 of the handle
  const int* seg;             // [nseg + 1] first node (in the chunk) of every handle present in the chunk; seg[nseg] = bc
  miqp_fixed_result_c* res;   // of the chunk's first node
  double* Z;                  // idem: [bc][row_doubles]
  double* seg_obj; int* seg_idx;   // of the chunk's first segment: the minimum of each and its index within the handle (-1: none feasible)
  int bc, base, nseg, n_inst, row_doubles;   // nodes of the chunk, node of the call of its first, segments (0: no minima; hfirst, seg, seg_obj and seg_idx are not read), handles of the call, N * nz (even: nz = 8 per car)
  int onchip, big;            // the shape has the on-chip kernel / its larger variant
  SoftCost soft;              // the price of the ignored points, per node from its fix record and its instance's weight
};

__global__ __launch_bounds__(FB_NT) void fixed_collect_kernel(const FixedCollectArgs A) {
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
  // pass 2: verdict, objective, iterations and violation of each node
  for (int k = tid; k < A.bc; k += FB_NT) {
    const int inst = A.batch_inst[k];
    const int ok = A.batch_ok[k]; const double viol = A.batch_viol[k], obj = A.batch_obj[k] + ((unsigned)inst < (unsigned)A.n_inst ? A.cobj[inst] + soft_cost(A.soft, k, inst) : 0.0);
    R[k].status = (!ok || viol > FEAS_TOL) ? 1 : 0; R[k].iterations = A.batch_it[k]; R[k].reserved = 0; R[k].objective = obj; R[k].violation = viol;
  }
  __syncthreads();   // (pass 3 reads the objectives pass 2 wrote: each carries the price of its own record's ignored points)
  // pass 3: the minimum of every segment, a wavefront per segment at a time (a lane's nodes ascend: a tie keeps the lower index)
  for (int s = wave; s < A.nseg; s += FB_NT / 64) {
    const int a = max(0, min(A.seg[s], A.bc)), b = max(a, min(A.seg[s + 1], A.bc));
    const int inst = a < b ? A.batch_inst[a] : -1;
    const bool known = (unsigned)inst < (unsigned)A.n_inst;
    double bo = 1e308; int bi = 0x7FFFFFFF;
    for (int k = a + lane; k < b; k += 64) {
      const int ok = A.batch_ok[k]; const double viol = A.batch_viol[k], obj = R[k].objective;
      if (ok && !(viol > FEAS_TOL) && obj < bo) { bo = obj; bi = k; }
    }
    pool_wave_argmin(bo, bi);
    if (lane == 0) { A.seg_obj[s] = bo; A.seg_idx[s] = (bi == 0x7FFFFFFF || !known) ? -1 : A.base + bi - A.hfirst[inst]; }
  }
}

// ---------------------------------------------------------------------------------------------------------------- device cache
// staging, result and per-handle buffers of the fixed calls, cached per device and never taken from the solver's pools (DevArr: grown, not shrunk;
// the staging and the trajectories exactly as large as the largest call so far).  Used under the device lock (DevCtx::mu of lane 0)
struct FixedDev {
  hipStream_t s_up = nullptr; hipEvent_t ev_up[2] = {}, ev_taken[2] = {};
  DevArr<signed char, true> h_stage[2]; DevArr<signed char> d_stage[2];
  DevArr<miqp_fixed_result_c> d_res;
  DevArr<double> d_Z;
  DevArr<int> d_seg;   // [FB_CHUNK + 1] the segment table of the chunk in flight (its batch_inst slice is copied into DevBuf::batch_inst)
  DevArr<double> d_cobj; DevArr<int> d_hfirst;
  DevArr<double> d_sobj; DevArr<int> d_sidx;
  // what open() needs: the per-handle words
  bool ensure_handles(size_t n_inst) { return d_cobj.need(n_inst, 64) && d_hfirst.need(n_inst, 64); }
  // what fixed_run needs: staging of a chunk, results and trajectories of n nodes, the minima of nsegs segments
  bool ensure_run(size_t stage_bytes, size_t n, size_t z_doubles, size_t nsegs) {
    if (!s_up) {
      HIP_OK(hipStreamCreateWithFlags(&s_up, hipStreamNonBlocking));
      for (int b = 0; b < 2; ++b) { HIP_OK(hipEventCreateWithFlags(&ev_up[b], hipEventDisableTiming)); HIP_OK(hipEventCreateWithFlags(&ev_taken[b], hipEventDisableTiming)); }
    }
    for (int b = 0; b < 2; ++b) if (!h_stage[b].need(stage_bytes) || !d_stage[b].need(stage_bytes)) return false;
    return d_seg.need(FB_CHUNK + 1) && d_res.need(n, 1024) && d_Z.need(z_doubles) && d_sobj.need(nsegs, 128) && d_sidx.need(nsegs, 128);
  }
};

// work(k) for k < n on at most 16 host threads (one per `per` items)
template <class F> void fixed_threads(int n, int per, F work) {
  const int nth = std::max(1, std::min({16, process_switches().prep_threads, (int)std::thread::hardware_concurrency(), n / std::max(1, per)}));
  if (nth <= 1) { for (int k = 0; k < n; ++k) work(k); return; }
  std::atomic<int> next{0}; std::vector<std::thread> th;
  for (int t = 0; t < nth; ++t) th.emplace_back([&] { for (int k = next.fetch_add(1); k < n; k = next.fetch_add(1)) work(k); });
  for (auto& t : th) t.join();
}

// the DevBuf the chain is launched with: the settings of miqp_solver_solve_fixed
DevBuf fixed_chain_settings(const DevBuf& B) { DevBuf Bp = B; Bp.qp_tol = QP_TOL_FINAL; Bp.use_cutoff = 0; Bp.ws_on = 0; return Bp; }

// where a chunk's outcome goes: results and trajectory rows of its first node; with nseg > 0 the minima of its segments (table in FixedDev::d_seg)
struct FixedChunk {
  int bc, base;   // nodes of the chunk, node of the call (of the slice, for the climb) of its first
  miqp_fixed_result_c* res; double* Z;
  int nseg = 0; double* seg_obj = nullptr; int* seg_idx = nullptr;
};

// One chunk on the solver stream: the per-chunk resets, the chain, the collect.  pool_fix and batch_inst of slots 0 .. bc - 1 are the caller's, enqueued
// in front.  Bp: fixed_chain_settings of the context's DevBuf.  false: HIP error
bool fixed_chunk(DevCtx& X, const DevBuf& Bp, const Layout& Y, const FixedDev& F, int n_inst, const FixedChunk& C) {
  const DevBuf& B = X.B; hipStream_t st = X.stream; const int bc = C.bc;
  HIP_OK(hipMemsetD32Async((hipDeviceptr_t)B.batch_count, bc, 1, st));
  // nothing of the chunk before, or of an earlier solve, stays in the slots or in the counters of the call's instances
  HIP_OK(hipMemsetAsync(B.pool_big, 0, (size_t)bc, st)); HIP_OK(hipMemsetAsync(B.batch_large, 0, (size_t)bc, st)); HIP_OK(hipMemsetAsync(B.batch_depth, 0, (size_t)bc * 4, st));
  HIP_OK(hipMemsetAsync(B.inst_nodes, 0, (size_t)n_inst * 8, st)); HIP_OK(hipMemsetAsync(B.inst_iters, 0, (size_t)n_inst * 8, st)); HIP_OK(hipMemsetAsync(B.stat_rowiters, 0, 8, st));
  launch_ipm_batch(X, Bp, bc, st);   // (zeroes the hand-over counts of its launches)
  FixedCollectArgs A;
  A.ovf_list = B.ovf_list; A.ovf_count = B.ovf_count; A.ovf2_list = B.ovf2_list; A.ovf2_count = B.ovf2_count;
  A.batch_ok = B.batch_ok; A.batch_it = B.batch_it; A.batch_obj = B.batch_obj; A.batch_viol = B.batch_viol; A.batch_Z = B.batch_Z; A.batch_inst = B.batch_inst;
  A.cobj = F.d_cobj; A.hfirst = C.nseg > 0 ? F.d_hfirst : nullptr; A.seg = C.nseg > 0 ? F.d_seg : nullptr;
  A.res = C.res; A.Z = C.Z; A.seg_obj = C.seg_obj; A.seg_idx = C.seg_idx;
  A.bc = bc; A.base = C.base; A.nseg = C.nseg; A.n_inst = n_inst; A.row_doubles = Y.N * Y.nz; A.onchip = X.oc_grid > 0 ? 1 : 0; A.big = X.ocb_grid > 0 ? 1 : 0;
  A.soft.fix = B.pool_fix; A.soft.inst_d = B.inst_d; A.soft.fixlen = Y.fixlen; A.soft.f_obs = Y.f_obs; A.soft.n_obs = Y.C * Y.O * Y.N * 5; A.soft.L = Y.L; A.soft.dstride = Y.dstride; A.soft.d_w = Y.d_misc + 1;
  hipLaunchKernelGGL(fixed_collect_kernel, dim3(1 + std::min(FB_ROW_BLOCKS, (bc + FB_NT / 64 - 1) / (FB_NT / 64))), dim3(FB_NT), 0, st, A);
  HIP_OK(hipGetLastError());
  return true;
}

// what a caller enqueues behind a chunk's fixed_chunk while the chunk's records still lie in pool_fix: (first node of the chunk, its nodes) -> false on a HIP error
using FixedAfterChunk = std::function<bool(int, int)>;

// The chunks of `fix` (m records; inst[k]: the handle of record k, ascending) through the chain.  tmp[m] and Zout receive the results, best[h] the
// index WITHIN handle h's records of this run of its feasible minimum (-1: none), groups the number of chunks.  after (may be NULL) runs behind
// every chunk.  false: HIP error
bool fixed_run(DevCtx& X, FixedDev& G, const Layout& Y, int n_inst, const std::vector<signed char>& fix, const std::vector<int>& inst, int m,
               std::vector<miqp_fixed_result_c>& tmp, std::vector<double>& Zout, std::vector<int>& best, float& dev_ms, int& groups, const FixedAfterChunk* after = nullptr) {
  DevBuf& B = X.B; hipStream_t st = X.stream;
  const size_t fl = (size_t)Y.fixlen, row = (size_t)Y.N * Y.nz;
  const int nch = (m + FB_CHUNK - 1) / FB_CHUNK;
  groups = nch;
  // the segments of every chunk: [sfirst[j], sfirst[j + 1]) of seg_node (chunk-relative first nodes) and seg_h (their handles)
  std::vector<int> hfirst(n_inst, 0), sfirst(nch + 1, 0), seg_node, seg_h;
  for (int k = m - 1; k >= 0; --k) hfirst[inst[k]] = k;
  for (int j = 0; j < nch; ++j) {
    const int c0 = j * FB_CHUNK, bc = std::min(FB_CHUNK, m - c0);
    for (int k = 0; k < bc; ++k) if (k == 0 || inst[c0 + k] != inst[c0 + k - 1]) { seg_node.push_back(k); seg_h.push_back(inst[c0 + k]); }
    sfirst[j + 1] = (int)seg_node.size();
  }
  const int nsegs = (int)seg_node.size();
  // (a chunk in staging: FB_CHUNK records, FB_CHUNK handle indices, at most FB_CHUNK + 1 segment entries)
  if (!G.ensure_run((size_t)FB_CHUNK * fl + (size_t)(2 * FB_CHUNK + 16) * 4, (size_t)m, (size_t)m * row, (size_t)nsegs)) return false;
  HIP_OK(hipMemcpyAsync(G.d_hfirst, hfirst.data(), (size_t)n_inst * 4, hipMemcpyHostToDevice, st));
  bool used[2] = {false, false};
  // a chunk in staging: its fix records, its batch_inst slice, its segment table (bc * fl bytes, bc ints, segments + 1 ints; fl is a multiple of 16)
  auto stage = [&](int j) -> bool {   // pinned staging -> device staging, on the upload stream
    const int p = j & 1, c0 = j * FB_CHUNK, bc = std::min(FB_CHUNK, m - c0), ns = sfirst[j + 1] - sfirst[j];
    if (used[p]) { HIP_OK(hipEventSynchronize(G.ev_up[p])); HIP_OK(hipStreamWaitEvent(G.s_up, G.ev_taken[p], 0)); }   // (chunk j - 2: its upload has left the pinned buffer, its copies the device one)
    std::memcpy(G.h_stage[p], fix.data() + (size_t)c0 * fl, (size_t)bc * fl);
    int* const hi = (int*)(G.h_stage[p] + (size_t)bc * fl);
    std::memcpy(hi, inst.data() + c0, (size_t)bc * 4);
    std::memcpy(hi + bc, seg_node.data() + sfirst[j], (size_t)ns * 4); hi[bc + ns] = bc;
    HIP_OK(hipMemcpyAsync(G.d_stage[p], G.h_stage[p], (size_t)bc * fl + (size_t)(bc + ns + 1) * 4, hipMemcpyHostToDevice, G.s_up));
    HIP_OK(hipEventRecord(G.ev_up[p], G.s_up));
    used[p] = true;
    return true;
  };
  if (!stage(0)) return false;
  HIP_OK(hipEventRecord(X.ev0, st));
  const DevBuf Bp = fixed_chain_settings(B);
  for (int j = 0; j < nch; ++j) {
    if (j + 1 < nch && !stage(j + 1)) return false;
    const int p = j & 1, c0 = j * FB_CHUNK, bc = std::min(FB_CHUNK, m - c0), ns = sfirst[j + 1] - sfirst[j];
    HIP_OK(hipStreamWaitEvent(st, G.ev_up[p], 0));
    HIP_OK(hipMemcpyAsync(B.pool_fix, G.d_stage[p], (size_t)bc * fl, hipMemcpyDeviceToDevice, st));
    HIP_OK(hipMemcpyAsync(B.batch_inst, G.d_stage[p] + (size_t)bc * fl, (size_t)bc * 4, hipMemcpyDeviceToDevice, st));
    HIP_OK(hipMemcpyAsync(G.d_seg, G.d_stage[p] + (size_t)bc * fl + (size_t)bc * 4, (size_t)(ns + 1) * 4, hipMemcpyDeviceToDevice, st));
    HIP_OK(hipEventRecord(G.ev_taken[p], st));
    FixedChunk C{bc, c0, G.d_res + c0, G.d_Z + (size_t)c0 * row, ns, G.d_sobj + sfirst[j], G.d_sidx + sfirst[j]};
    if (!fixed_chunk(X, Bp, Y, G, n_inst, C)) return false;
    if (after && !(*after)(c0, bc)) return false;
  }
  HIP_OK(hipEventRecord(X.ev1, st));
  std::vector<double> sobj(nsegs); std::vector<int> sidx(nsegs);
  tmp.resize(m); Zout.resize((size_t)m * row);
  HIP_OK(hipMemcpyAsync(tmp.data(), G.d_res, (size_t)m * sizeof(miqp_fixed_result_c), hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(Zout.data(), G.d_Z, (size_t)m * row * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(sobj.data(), G.d_sobj, (size_t)nsegs * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(sidx.data(), G.d_sidx, (size_t)nsegs * 4, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st)); HIP_OK(hipStreamSynchronize(G.s_up)); HIP_OK(hipGetLastError());
  (void)hipEventElapsedTime(&dev_ms, X.ev0, X.ev1);
  // the minimum of every handle from its segments' minima (ascending chunks: a tie keeps the lower index)
  best.assign(n_inst, -1);
  std::vector<double> bobj(n_inst, 0.0);
  for (int q = 0; q < nsegs; ++q) {
    const int h = seg_h[q];
    if (sidx[q] >= 0 && (best[h] < 0 || sobj[q] < bobj[h])) { bobj[h] = sobj[q]; best[h] = sidx[q]; }
  }
  return true;
}

// The part of a fixed call that runs PREPARED fix bytes: open() takes the device and its lock, brings the context to the sizes of the batch call for n
// instances (up to 64 handles: the context a one-handle call asks for), compiles the instances on host threads, checks their first steps and uploads
// the tables and the slot numbers once; run() sends m fix records through the chain.  The lock is held until the object goes.  Both return 0 or -3
// (no device / kernel image / HIP error)
struct FixedCall {
  miqp_solver_t* const* S = nullptr; int n = 0; Layout Y{}; DevCtx* X = nullptr; std::unique_lock<std::mutex> lock;
  std::vector<double> D; std::vector<int> T; std::vector<double> cobj;
  int open(miqp_solver_t* const* S_, int n_, const Layout& Y_) {
    S = S_; n = n_; Y = Y_;
    X = ctx_for_device(S[0]->opts.device);
    if (!X) return -3;
    lock = std::unique_lock<std::mutex>(X->mu);
    bool rebuilt = false; const double t_ctx = wall_s();
    if (!ctx_prepare(*X, Y, n, 1, 64, FB_CHUNK, 3, false, 1, &rebuilt)) return -3;
    const double ctx_s = wall_s() - t_ctx;
    for (int h = 0; h < n; ++h) { S[h]->setup[1] = ctx_s; S[h]->setup[2] = rebuilt ? 1.0 : 0.0; }
    if (X->batch_cap < FB_CHUNK || X->batch_alloc < FB_CHUNK || X->pool_cap < FB_CHUNK) { std::fprintf(stderr, "[miqp_gpu] the device context does not hold a chunk of %d nodes\n", FB_CHUNK); return -3; }
    if (X->n_inst_cap < n) { std::fprintf(stderr, "[miqp_gpu] the device context holds the tables of %d instances, the call has %d\n", X->n_inst_cap, n); return -3; }
    if (!set_kernel_lds(Y, ipm_lds_bytes(Y), eval_lds_bytes(Y, read_call_switches().seq_kinds))) return -3;
    D.resize((size_t)n * Y.dstride); T.resize((size_t)n * Y.istride); cobj.assign(n, 0.0);
    fixed_threads(n, 8, [&](int h) {
      double* d = D.data() + (size_t)h * Y.dstride; int* t = T.data() + (size_t)h * Y.istride;
      compile_instance(S[h]->inst, Y, d, t);
      HostGeo G{S[h]->inst, Y, d, t}; (void)step0_check(G, cobj[h]);
    });
    return upload() ? 0 : -3;
  }
  FixedDev& dev() const { return call_dev<FixedDev>(X->device); }
  const double* tabD(int h) const { return D.data() + (size_t)h * Y.dstride; }
  const int* tabT(int h) const { return T.data() + (size_t)h * Y.istride; }
  bool upload() {
    FixedDev& F = dev();
    if (!F.ensure_handles((size_t)n)) return false;
    DevBuf& B = X->B; hipStream_t st = X->stream;
    std::vector<int> ident(FB_CHUNK); for (int k = 0; k < FB_CHUNK; ++k) ident[k] = k;
    HIP_OK(hipMemcpyAsync((void*)B.inst_d, D.data(), D.size() * 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync((void*)B.inst_i, T.data(), T.size() * 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(B.batch_node, ident.data(), (size_t)FB_CHUNK * 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(F.d_cobj, cobj.data(), (size_t)n * 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipStreamSynchronize(st));   // (ident is a local)
    return true;
  }
  int run(const std::vector<signed char>& fix, const std::vector<int>& inst, int m, std::vector<miqp_fixed_result_c>& tmp, std::vector<double>& Z, std::vector<int>& best, float& dev_ms, int& groups,
          const FixedAfterChunk* after = nullptr) {
    FixedDev& F = dev();
    if (!fixed_run(*X, F, Y, n, fix, inst, m, tmp, Z, best, dev_ms, groups, after)) { (void)hipStreamSynchronize(X->stream); if (F.s_up) (void)hipStreamSynchronize(F.s_up); return -3; }
    return 0;
  }
};

// what the multi entries refuse before a device is touched: 0, or -1 (a NULL handle, one without an instance, one named twice), -2 (handles that
// batch_layout refuses, with its text as the handles' last error, or that differ in opts.device)
int fixed_multi_check(miqp_solver_t* const* S, int n, BatchShape& bs) {
  for (int h = 0; h < n; ++h) if (!S[h] || !S[h]->has_inst) return -1;
  { std::vector<const miqp_solver_t*> seen(S, S + n); std::sort(seen.begin(), seen.end()); if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) return -1; }
  bs = batch_layout(S, n);
  if (!bs.ok) { for (int h = 0; h < n; ++h) S[h]->err = bs.err; return -2; }
  for (int h = 1; h < n; ++h) if (S[h]->opts.device != S[0]->opts.device) { for (int q = 0; q < n; ++q) S[q]->err = "the handles of one call must name the same device"; return -2; }
  return 0;
}

// every entry refused until the device has answered it
void fixed_refuse(miqp_fixed_result_c* out, int n) {
  for (int k = 0; k < n; ++k) { out[k].status = 2; out[k].route = -1; out[k].iterations = 0; out[k].reserved = 0; out[k].objective = std::nan(""); out[k].violation = std::nan(""); }
}

// record c of what a fixed call left on the handle (fix bytes and trajectory rows, Layout order) as the record solve_fixed would have returned.
// 0, or -1 when batch_layout refuses the handle
int fixed_hand_out(const miqp_solver_t* s, const std::vector<signed char>& fixes, const std::vector<double>& Zs, int c, miqp_raw_results_c* out) {
  miqp_solver_t* one[1] = {const_cast<miqp_solver_t*>(s)};
  BatchShape bs = batch_layout(one, 1);
  if (!bs.ok) return -1;
  const Layout& Y = bs.Y;
  std::vector<double> D(Y.dstride); std::vector<int> T(Y.istride);
  compile_instance(s->inst, Y, D.data(), T.data());
  // undecided leaf disjunctions: canonical completion is done by fill_results (it evaluates every side), as in the single call
  std::vector<signed char> fix(fixes.begin() + (size_t)c * Y.fixlen, fixes.begin() + (size_t)(c + 1) * Y.fixlen);
  for (auto& b : fix) if (b < 0) b = 0;
  fill_results(s->inst, Y, D.data(), T.data(), fix.data(), Zs.data() + (size_t)c * Y.N * Y.nz, out);
  return 0;
}

}  // namespace

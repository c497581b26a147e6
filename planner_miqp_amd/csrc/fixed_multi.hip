// fixed_multi.hip - fix records and solution pools of MANY instances in one device call (miqp_solver_solve_fixed_multi, miqp_solver_pool_solve_multi).
//
// fixed_batch.hip answers many records of the instance ONE handle holds; the product's path is a queue of thousands of handles, and a loop of
// single-handle calls over them pays per handle what that call pays once: a device lock, a compile_instance, an upload of the tables, a chain of
// launches that is as long for one node as for a thousand - and a context rebuild whenever two handles differ in their own Layout.  No reference
// counterpart: the reference has one IloCplex per wrapper and walks its alternative start configurations one cplex.solve() at a time.
//
// The node kernels take nodes of many instances in one launch already - they read batch_inst[node] and index the instance tables by it, which is
// how every round of the branch and bound runs.  Here the nodes of a call are numbered handle-major in the caller's order, node k of a chunk is
// batch slot k with batch_inst[k] = the index of its handle in the call, and the chain, its settings and its per-chunk resets are those of
// fixed_batch_run.  One device lock, one context (the common Layout of the handles: batch_layout), the n instances compiled on host threads, their
// tables uploaded once.  With use_cutoff = 0 and ws_on = 0 the three node kernels read, per instance, their tables (inst_d, inst_i) and the incumbent
// words inc_key / inc_ext, whose value node_cutoff then drops; they add to inst_nodes / inst_iters.  So nothing per instance needs a value but the
// tables, and the counters are cleared for all n instances per chunk.
//
// Kernel: fixed_multi_collect_kernel does per chunk what fixed_batch_collect_kernel does, with the constant cost of step 0 taken per node from its
// instance, and ONE MINIMUM PER HANDLE instead of one per chunk: the host passes the chunk's segment table (first node of every handle present in
// the chunk), a wavefront of workgroup 0 takes a segment at a time, reduces (objective, index within the handle) over its feasible nodes with the
// xor tree - ties to the lower index - and writes the pair to the segment's slot.  A handle whose nodes straddle chunks gets one partial result per
// chunk; the host folds them in ascending chunk order.  No atomics, no LDS, no scratch, nothing that depends on arrival order.
#pragma once

namespace {

struct FixedMultiArgs {
  const int* ovf_list; const int* ovf_count; const int* ovf2_list; const int* ovf2_count;
  const int* batch_ok; const int* batch_it; const double* batch_obj; const double* batch_viol; const double* batch_Z; const int* batch_inst;
  const double* cobj;         // [n_inst] constant cost of step 0 of every handle (step0_check)
  const int* hfirst;          // [n_inst] node of the call that is entry 0 of the handle
  const int* seg;             // [nseg + 1] first node (in the chunk) of every handle present in the chunk; seg[nseg] = bc
  miqp_fixed_result_c* res;   // of the chunk's first node
  double* Z;                  // idem: [bc][row_doubles]
  double* seg_obj; int* seg_idx;   // of the chunk's first segment: the minimum of each and its index within the handle (-1: none feasible)
  int bc, base, nseg, n_inst, row_doubles;   // nodes of the chunk, node of the call of its first, segments, handles of the call, N * nz
  int onchip, big;
  SoftCost soft;              // the price of the ignored points, per node from its fix record and its instance's weight
};

__global__ __launch_bounds__(FB_NT) void fixed_multi_collect_kernel(const FixedMultiArgs A) {
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
  // pass 1: the launch of the chain that solved each node, from its hand-over lists (the rule of fixed_batch_collect_kernel)
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
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const double oo = __shfl_xor(bo, d, 64); const int oi = __shfl_xor(bi, d, 64);
      if (oo < bo || (oo == bo && oi < bi)) { bo = oo; bi = oi; }
    }
    if (lane == 0) { A.seg_obj[s] = bo; A.seg_idx[s] = (bi == 0x7FFFFFFF || !known) ? -1 : A.base + bi - A.hfirst[inst]; }
  }
}

// ---------------------------------------------------------------------------------------------------------------- device cache
// what the multi call needs beside the staging and result buffers of the batch call (FixedBatchDev, shared with it): per device, grown, not shrunk
struct FixedMultiDev {
  int* d_inst = nullptr; int* d_seg = nullptr;   // [FB_CHUNK + 1] a chunk's batch_inst slice is copied into DevBuf::batch_inst; its segment table stays here
  double* d_cobj = nullptr; int* d_hfirst = nullptr; size_t inst_cap = 0;
  double* d_sobj = nullptr; int* d_sidx = nullptr; size_t seg_cap = 0;
  bool ensure(size_t n_inst, size_t nsegs) {
    if (!d_seg) HIP_OK(hipMalloc((void**)&d_seg, (size_t)(FB_CHUNK + 1) * sizeof(int)));
    if (n_inst > inst_cap) {
      if (d_cobj) (void)hipFree(d_cobj); if (d_hfirst) (void)hipFree(d_hfirst);
      d_cobj = nullptr; d_hfirst = nullptr; inst_cap = 0;
      size_t want = 64; while (want < n_inst) want <<= 1;
      HIP_OK(hipMalloc((void**)&d_cobj, want * sizeof(double))); HIP_OK(hipMalloc((void**)&d_hfirst, want * sizeof(int)));
      inst_cap = want;
    }
    if (nsegs > seg_cap) {
      if (d_sobj) (void)hipFree(d_sobj); if (d_sidx) (void)hipFree(d_sidx);
      d_sobj = nullptr; d_sidx = nullptr; seg_cap = 0;
      size_t want = 128; while (want < nsegs) want <<= 1;
      HIP_OK(hipMalloc((void**)&d_sobj, want * sizeof(double))); HIP_OK(hipMalloc((void**)&d_sidx, want * sizeof(int)));
      seg_cap = want;
    }
    return true;
  }
};
std::map<int, FixedMultiDev> g_fixed_multi_dev;   // by device ordinal; used under the device lock (DevCtx::mu of lane 0)

// work(k) for k < n on at most 16 host threads (one per `per` items)
template <class F> void fixed_multi_threads(int n, int per, F work) {
  const int nth = std::max(1, std::min({16, process_switches().prep_threads, (int)std::thread::hardware_concurrency(), n / std::max(1, per)}));
  if (nth <= 1) { for (int k = 0; k < n; ++k) work(k); return; }
  std::atomic<int> next{0}; std::vector<std::thread> th;
  for (int t = 0; t < nth; ++t) th.emplace_back([&] { for (int k = next.fetch_add(1); k < n; k = next.fetch_add(1)) work(k); });
  for (auto& t : th) t.join();
}

// The chunks of `fix` (m records; inst[k]: the handle of record k, ascending) through the chain.  tmp[m] and Zout receive the results, best[h] the
// index WITHIN handle h's records of this run of its feasible minimum (-1: none).  false: HIP error
bool fixed_multi_run(DevCtx& X, FixedBatchDev& G, FixedMultiDev& M, const Layout& Y, int n_inst, const std::vector<signed char>& fix, const std::vector<int>& inst, int m,
                     std::vector<miqp_fixed_result_c>& tmp, std::vector<double>& Zout, std::vector<int>& best, float& dev_ms, int& groups) {
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
  if (!M.ensure((size_t)n_inst, (size_t)nsegs)) return false;
  HIP_OK(hipMemcpyAsync(M.d_hfirst, hfirst.data(), (size_t)n_inst * 4, hipMemcpyHostToDevice, st));
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
  DevBuf Bp = B; Bp.qp_tol = QP_TOL_FINAL; Bp.use_cutoff = 0; Bp.ws_on = 0;
  for (int j = 0; j < nch; ++j) {
    if (j + 1 < nch && !stage(j + 1)) return false;
    const int p = j & 1, c0 = j * FB_CHUNK, bc = std::min(FB_CHUNK, m - c0), ns = sfirst[j + 1] - sfirst[j];
    HIP_OK(hipStreamWaitEvent(st, G.ev_up[p], 0));
    HIP_OK(hipMemcpyAsync(B.pool_fix, G.d_stage[p], (size_t)bc * fl, hipMemcpyDeviceToDevice, st));
    HIP_OK(hipMemcpyAsync(B.batch_inst, G.d_stage[p] + (size_t)bc * fl, (size_t)bc * 4, hipMemcpyDeviceToDevice, st));
    HIP_OK(hipMemcpyAsync(M.d_seg, G.d_stage[p] + (size_t)bc * fl + (size_t)bc * 4, (size_t)(ns + 1) * 4, hipMemcpyDeviceToDevice, st));
    HIP_OK(hipEventRecord(G.ev_taken[p], st));
    HIP_OK(hipMemsetD32Async((hipDeviceptr_t)B.batch_count, bc, 1, st));
    // nothing of the chunk before, or of an earlier solve, stays in the slots or in the counters of the call's instances
    HIP_OK(hipMemsetAsync(B.pool_big, 0, (size_t)bc, st)); HIP_OK(hipMemsetAsync(B.batch_large, 0, (size_t)bc, st)); HIP_OK(hipMemsetAsync(B.batch_depth, 0, (size_t)bc * 4, st));
    HIP_OK(hipMemsetAsync(B.inst_nodes, 0, (size_t)n_inst * 8, st)); HIP_OK(hipMemsetAsync(B.inst_iters, 0, (size_t)n_inst * 8, st)); HIP_OK(hipMemsetAsync(B.stat_rowiters, 0, 8, st));
    launch_ipm_batch(X, Bp, bc, st);   // (zeroes the hand-over counts of its launches)
    FixedMultiArgs A;
    A.ovf_list = B.ovf_list; A.ovf_count = B.ovf_count; A.ovf2_list = B.ovf2_list; A.ovf2_count = B.ovf2_count;
    A.batch_ok = B.batch_ok; A.batch_it = B.batch_it; A.batch_obj = B.batch_obj; A.batch_viol = B.batch_viol; A.batch_Z = B.batch_Z; A.batch_inst = B.batch_inst;
    A.cobj = M.d_cobj; A.hfirst = M.d_hfirst; A.seg = M.d_seg;
    A.res = G.d_res + c0; A.Z = G.d_Z + (size_t)c0 * row; A.seg_obj = M.d_sobj + sfirst[j]; A.seg_idx = M.d_sidx + sfirst[j];
    A.bc = bc; A.base = c0; A.nseg = ns; A.n_inst = n_inst; A.row_doubles = (int)row; A.onchip = X.oc_grid > 0 ? 1 : 0; A.big = X.ocb_grid > 0 ? 1 : 0; A.soft = soft_cost_args(B, Y);
    hipLaunchKernelGGL(fixed_multi_collect_kernel, dim3(1 + std::min(FB_ROW_BLOCKS, (bc + FB_NT / 64 - 1) / (FB_NT / 64))), dim3(FB_NT), 0, st, A);
    HIP_OK(hipGetLastError());
  }
  HIP_OK(hipEventRecord(X.ev1, st));
  std::vector<double> sobj(nsegs); std::vector<int> sidx(nsegs);
  tmp.resize(m); Zout.resize((size_t)m * row);
  HIP_OK(hipMemcpyAsync(tmp.data(), G.d_res, (size_t)m * sizeof(miqp_fixed_result_c), hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(Zout.data(), G.d_Z, (size_t)m * row * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(sobj.data(), M.d_sobj, (size_t)nsegs * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(sidx.data(), M.d_sidx, (size_t)nsegs * 4, hipMemcpyDeviceToHost, st));
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

// The part of a multi call that runs PREPARED fix bytes: open() takes the device and its lock, brings the context to the sizes of the batch call for n
// instances (up to 64 handles: the context the single-handle call asks for), compiles the instances on host threads, checks their first steps and
// uploads the tables; run() sends m fix records through the chain.  The lock is held until the object goes.  Both return 0 or -3
struct FixedMultiCall {
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
    fixed_multi_threads(n, 8, [&](int h) {
      double* d = D.data() + (size_t)h * Y.dstride; int* t = T.data() + (size_t)h * Y.istride;
      compile_instance(S[h]->inst, Y, d, t);
      HostGeo G{S[h]->inst, Y, d, t}; (void)step0_check(G, cobj[h]);
    });
    return upload() ? 0 : -3;
  }
  const double* tabD(int h) const { return D.data() + (size_t)h * Y.dstride; }
  const int* tabT(int h) const { return T.data() + (size_t)h * Y.istride; }
  bool upload() {
    FixedMultiDev& M = g_fixed_multi_dev[X->device];
    if (!M.ensure((size_t)n, 1)) return false;
    DevBuf& B = X->B; hipStream_t st = X->stream;
    std::vector<int> ident(FB_CHUNK); for (int k = 0; k < FB_CHUNK; ++k) ident[k] = k;
    HIP_OK(hipMemcpyAsync((void*)B.inst_d, D.data(), D.size() * 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync((void*)B.inst_i, T.data(), T.size() * 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(B.batch_node, ident.data(), (size_t)FB_CHUNK * 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(M.d_cobj, cobj.data(), (size_t)n * 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipStreamSynchronize(st));   // (ident is a local)
    return true;
  }
  int run(const std::vector<signed char>& fix, const std::vector<int>& inst, int m, std::vector<miqp_fixed_result_c>& tmp, std::vector<double>& Z, std::vector<int>& best, float& dev_ms, int& groups) {
    FixedBatchDev& F = g_fixed_batch_dev[X->device]; FixedMultiDev& M = g_fixed_multi_dev[X->device];
    // (a chunk in staging: FB_CHUNK records, FB_CHUNK handle indices, at most FB_CHUNK + 1 segment entries)
    if (!F.ensure((size_t)FB_CHUNK * Y.fixlen + (size_t)(2 * FB_CHUNK + 16) * 4, (size_t)m, (size_t)m * Y.N * Y.nz)) return -3;
    if (!fixed_multi_run(*X, F, M, Y, n, fix, inst, m, tmp, Z, best, dev_ms, groups)) { (void)hipStreamSynchronize(X->stream); (void)hipStreamSynchronize(F.s_up); return -3; }
    return 0;
  }
};

// what both entries refuse before a device is touched: 0, or -1 (a NULL handle, one without an instance, one named twice), -2 (handles that batch_layout
// refuses, with its text as the handles' last error, or that differ in opts.device)
int fixed_multi_check(miqp_solver_t* const* S, int n, BatchShape& bs) {
  for (int h = 0; h < n; ++h) if (!S[h] || !S[h]->has_inst) return -1;
  { std::vector<const miqp_solver_t*> seen(S, S + n); std::sort(seen.begin(), seen.end()); if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) return -1; }
  bs = batch_layout(S, n);
  if (!bs.ok) { for (int h = 0; h < n; ++h) S[h]->err = bs.err; return -2; }
  for (int h = 1; h < n; ++h) if (S[h]->opts.device != S[0]->opts.device) { for (int q = 0; q < n; ++q) S[q]->err = "the handles of one call must name the same device"; return -2; }
  return 0;
}

}  // namespace

extern "C" {

int miqp_solver_solve_fixed_multi(miqp_solver_t* const* solvers, int n, const miqp_raw_results_c* const* fixed, const int* first, miqp_fixed_result_c* out, int* best) {
  if (!solvers || !fixed || !first || !out || n <= 0 || first[0] != 0) return -1;
  for (int h = 0; h < n; ++h) if (first[h + 1] < first[h]) return -1;
  BatchShape bs;
  if (const int rc = fixed_multi_check(solvers, n, bs)) return rc;
  const int total = first[n];
  if (total > FB_CAP) return -5;
  const Layout& Y = bs.Y;
  const double t_call = wall_s();
  for (int h = 0; h < n; ++h) { solvers[h]->drop_fixed_batch(); if (best) best[h] = -1; }
  for (int k = 0; k < total; ++k) { out[k].status = 2; out[k].route = -1; out[k].iterations = 0; out[k].reserved = 0; out[k].objective = std::nan(""); out[k].violation = std::nan(""); }
  // the accepted entries, handle-major in the caller's order: entry where[c] is node c of the call, nfirst[h] the first node of handle h
  std::vector<int> where, inst, nfirst(n + 1, 0); where.reserve(total); inst.reserve(total);
  for (int h = 0; h < n; ++h) {
    for (int k = first[h]; k < first[h + 1]; ++k) if (fixed[k] && fixed_record_ok(*fixed[k]) && dims_match(*fixed[k], solvers[h]->inst)) { where.push_back(k); inst.push_back(h); }
    nfirst[h + 1] = (int)where.size();
  }
  const int m = (int)where.size();
  if (m == 0) return 0;   // (nothing to run: no device is touched)
  FixedMultiCall call;
  if (call.open(solvers, n, Y) != 0) return -3;
  const size_t fl = (size_t)Y.fixlen, row = (size_t)Y.N * Y.nz;
  std::vector<signed char> fix((size_t)m * fl);
  {   // fix records on a few host threads when there are many
    const int blocks = (m + 255) / 256;
    fixed_multi_threads(blocks, 1, [&](int b) {
      std::vector<signed char> one_fix;
      for (int c = b * 256; c < std::min(m, (b + 1) * 256); ++c) {
        const int h = inst[c];
        (void)fix_from_results(solvers[h]->inst, Y, call.tabT(h), fixed[where[c]], one_fix); std::memcpy(fix.data() + (size_t)c * fl, one_fix.data(), fl);
      }
    });
  }
  const double setup_s = wall_s() - t_call;
  std::vector<miqp_fixed_result_c> tmp; std::vector<double> Z; std::vector<int> hbest; float dev_ms = 0.0f; int groups = 0;
  if (call.run(fix, inst, m, tmp, Z, hbest, dev_ms, groups) != 0) return -3;
  for (int c = 0; c < m; ++c) out[where[c]] = tmp[c];
  const double call_s = wall_s() - t_call;
  for (int h = 0; h < n; ++h) {
    miqp_solver_t* s = solvers[h];
    const int c0 = nfirst[h], mh = nfirst[h + 1] - c0, nh = first[h + 1] - first[h];
    s->setup[0] = setup_s;
    s->timing[0] = call_s; s->timing[1] = dev_ms * 1e-3; s->timing[2] = groups; s->timing[3] = mh; s->timing[4] = 0; s->timing[5] = 0;
    for (int c = c0; c < c0 + mh; ++c) s->timing[4] += tmp[c].iterations;
    if (mh == 0) continue;   // (an empty range, or every entry refused: the handle keeps nothing, as behind the single call)
    if (best) best[h] = hbest[h] < 0 || hbest[h] >= mh ? -1 : where[c0 + hbest[h]] - first[h];
    s->fb_n = nh; s->fb_slot.assign(nh, -1);
    for (int c = 0; c < mh; ++c) if (tmp[c0 + c].status == 0) s->fb_slot[where[c0 + c] - first[h]] = c;
    s->fb_Z.assign(Z.begin() + (size_t)c0 * row, Z.begin() + (size_t)(c0 + mh) * row);
    s->fb_fix.assign(fix.begin() + (size_t)c0 * fl, fix.begin() + (size_t)(c0 + mh) * fl);
  }
  return 0;
}

int miqp_solver_pool_solve_multi(miqp_solver_t* const* solvers, int n, miqp_fixed_result_c* out, int cap, int* counts) {
  if (!solvers || !out || !counts || n <= 0 || cap < 1) return -1;
  BatchShape bs;
  if (const int rc = fixed_multi_check(solvers, n, bs)) return rc;
  const Layout& Y = bs.Y; const size_t fl = (size_t)Y.fixlen, row = (size_t)Y.N * Y.nz;
  // entries of every handle: ent[h] of them, the first at node efirst[h] of the first pass
  std::vector<int> ent(n), efirst(n + 1, 0);
  for (int h = 0; h < n; ++h) {
    ent[h] = std::min(miqp_solver_pool_count(solvers[h]), cap);
    if (ent[h] > 0 && solvers[h]->pool_fixlen != Y.fixlen) return -1;
    efirst[h + 1] = efirst[h] + ent[h];
  }
  const int total = efirst[n];
  if (total > FB_CAP) return -5;
  for (int h = 0; h < n; ++h) { solvers[h]->pr_n = 0; counts[h] = 0; }
  if (total == 0) return 0;   // (nothing to run: no device is touched)
  const double t_call = wall_s();
  FixedMultiCall call;
  if (call.open(solvers, n, Y) != 0) return -3;
  // per handle, as miqp_solver_pool_solve keeps them: the labels its entries are solved with, those of their own solutions, the last answers
  struct PerHandle { std::vector<signed char> fix, canon; std::vector<miqp_fixed_result_c> tmp; std::vector<double> Z; int passes = 0; bool moving = true; };
  std::vector<PerHandle> H(n);
  for (int h = 0; h < n; ++h) { H[h].moving = ent[h] > 0; H[h].fix.assign(solvers[h]->pool_fix.begin(), solvers[h]->pool_fix.begin() + (size_t)ent[h] * fl); H[h].canon.resize((size_t)ent[h] * fl); }
  float dev_ms = 0.0f; int groups = 0;
  for (int pass = 0; pass < POOL_PASSES; ++pass) {
    // the entries of the handles whose labels moved in the pass before (the first pass: all)
    std::vector<int> live, inst, lfirst;
    std::vector<signed char> fix;
    for (int h = 0; h < n; ++h) if (H[h].moving) { live.push_back(h); lfirst.push_back((int)inst.size()); inst.insert(inst.end(), ent[h], h); fix.insert(fix.end(), H[h].fix.begin(), H[h].fix.end()); }
    if (live.empty()) break;
    const int m = (int)inst.size();
    std::vector<miqp_fixed_result_c> tmp; std::vector<double> Z; std::vector<int> hbest; float ms = 0.0f; int g = 0;
    if (call.run(fix, inst, m, tmp, Z, hbest, ms, g) != 0) return -3;
    dev_ms += ms; groups += g;
    fixed_multi_threads((int)live.size(), 4, [&](int q) {
      const int h = live[q], c0 = lfirst[q]; miqp_solver_t* s = solvers[h]; PerHandle& P = H[h];
      P.tmp.assign(tmp.begin() + c0, tmp.begin() + c0 + ent[h]); P.Z.assign(Z.begin() + (size_t)c0 * row, Z.begin() + (size_t)(c0 + ent[h]) * row);
      P.passes++;
      OwnedResults R(s->inst); std::vector<signed char> one, full;
      for (int k = 0; k < ent[h]; ++k) {
        std::memcpy(P.canon.data() + (size_t)k * fl, P.fix.data() + (size_t)k * fl, fl);
        if (P.tmp[k].status != 0) continue;
        full.assign(P.fix.begin() + (size_t)k * fl, P.fix.begin() + (size_t)(k + 1) * fl);
        for (auto& b : full) if (b < 0) b = 0;
        fill_results(s->inst, Y, call.tabD(h), call.tabT(h), full.data(), P.Z.data() + (size_t)k * row, &R.r);
        (void)fix_from_results(s->inst, Y, call.tabT(h), &R.r, one);
        std::memcpy(P.canon.data() + (size_t)k * fl, one.data(), fl);
      }
      // when the labels are the ones just solved with, that call answers with these bits; at the last pass the answers stay those of the labels they were solved with
      P.moving = P.canon != P.fix;
      if (P.moving && P.passes < POOL_PASSES) P.fix = P.canon;
    });
  }
  const double call_s = wall_s() - t_call;
  int left = 0;
  for (int h = 0; h < n; ++h) {
    miqp_solver_t* s = solvers[h]; PerHandle& P = H[h]; const int m = ent[h];
    s->timing[0] = call_s; s->timing[1] = dev_ms * 1e-3; s->timing[2] = P.passes; s->timing[3] = 0; s->timing[4] = 0; s->timing[5] = 0;
    if (m == 0) continue;
    if (P.moving) {
      char msg[220]; std::snprintf(msg, sizeof msg, "miqp_solver_pool_solve_multi: the labels of the pool entries still moved after %d passes; an entry may differ from what miqp_solver_solve_fixed answers for its record", P.passes);
      s->err = msg; std::fprintf(stderr, "[miqp_gpu] %s\n", msg);
    }
    // entries whose records carry the same binaries - under the handle's filter: the same signature - are ONE solution (pool_same_entry, shared with
    // miqp_solver_pool_solve): the first in pool order stays, the handle's pool shrinks with it
    std::vector<miqp_fixed_result_c>& tmp = P.tmp; std::vector<signed char>& fix = P.fix; std::vector<signed char>& canon = P.canon; std::vector<double>& Z = P.Z;
    int kept = 0;
    for (int k = 0; k < m; ++k) {
      bool dup = false;
      for (int j = 0; j < kept && !dup; ++j) dup = tmp[k].status == 0 && tmp[j].status == 0 && pool_same_entry(Y, s->pool_fam, canon.data() + (size_t)k * fl, canon.data() + (size_t)j * fl);
      if (dup) continue;
      if (kept != k) {
        tmp[kept] = tmp[k]; s->pool_obj[kept] = s->pool_obj[k];
        std::memmove(fix.data() + (size_t)kept * fl, fix.data() + (size_t)k * fl, fl); std::memmove(canon.data() + (size_t)kept * fl, canon.data() + (size_t)k * fl, fl);
        std::memmove(s->pool_fix.data() + (size_t)kept * fl, s->pool_fix.data() + (size_t)k * fl, fl);
        std::memmove(Z.data() + (size_t)kept * row, Z.data() + (size_t)k * row, row * sizeof(double));
      }
      kept++;
    }
    if (kept < m) {   // (entries behind `cap`, not refined by this call, move up unchanged)
      s->pool_obj.erase(s->pool_obj.begin() + kept, s->pool_obj.begin() + m);
      s->pool_fix.erase(s->pool_fix.begin() + (size_t)kept * fl, s->pool_fix.begin() + (size_t)m * fl);
      s->pool_n -= m - kept;
    }
    fix.resize((size_t)kept * fl); Z.resize((size_t)kept * row);
    for (int k = 0; k < kept; ++k) out[(size_t)h * cap + k] = tmp[k];
    counts[h] = kept; left += kept;
    s->pr_n = kept; s->pr_ok.assign(kept, 0);
    for (int k = 0; k < kept; ++k) s->pr_ok[k] = tmp[k].status == 0 ? 1 : 0;
    s->pr_Z.swap(Z); s->pr_fix.swap(fix);
    s->timing[3] = kept; s->timing[5] = P.moving ? 1 : 0;
    for (int k = 0; k < kept; ++k) s->timing[4] += tmp[k].iterations;
  }
  return left;
}

}  // extern "C"

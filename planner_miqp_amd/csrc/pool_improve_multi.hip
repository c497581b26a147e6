// pool_improve_multi.hip - the climb of pool_improve.hip over the kept entries of MANY handles in one device call (miqp_solver_pool_improve_multi),
// and the slices of a pass as a pure host function (miqp_gpu_pool_improve_plan).  DESIGN.md 6g.
//
// The product's path is a drained queue of hundreds to thousands of handles.  A loop of miqp_solver_pool_improve over them pays per handle a device
// lock, a compile_instance, an upload of the tables, per pass a chain of launches that is as long for 19 neighbours as for 1024, and per pass a
// host synchronisation.  Here the entries of all handles are numbered handle-major in the caller's order, ONE pass of the call is one pass of every
// handle that still moves, and the neighbours of all of them fill common launch groups of FB_CHUNK nodes.
//
// The kernels are those of the single call - it is their one-handle case: every entry carries its handle's index in the call (ent_inst, which
// pool_neighbour_kernel writes to batch_inst beside the node's record, so that the node kernels read that handle's tables) and its handle's filter
// (ent_fam, which pool_moves_kernel reads); the dims are common (batch_layout).  Per entry nothing else differs, so a handle's entries get the bits
// the single call gives them: a node's answer is a function of its record and its instance's tables alone.
//
// SLICES.  The results of a pass are not all kept at once: a slice is a run of whole entries whose neighbours fit the PoolImproveDev::NB_MAX results
// of the single call's buffer, formed greedily in entry order (miqp_gpu_pool_improve_plan; the host loop calls that very function).  Per slice: its
// nodes in chunks of FB_CHUNK through launch_ipm_batch with the resets of fixed_multi_run, fixed_multi_collect_kernel without segments (the constant
// cost of step 0 per node from its instance) into the slice's results, pool_pick_kernel over the slice's entries.  Behind the last slice
// pool_moves_kernel and pool_offsets_kernel for the next pass.  The host knows the counts of a pass from the read-back of the pass before, enqueues
// all slices without waiting and synchronises once per pass: one PoolWord and one count per entry.  Pass 0 - every entry's own record - is the same
// loop with one node per entry.
//
// Device memory of the call: entries x (record + POOL_MOVES_MAX moves of 16 bytes + a few words), grown, not shrunk, cached per device, beside the
// fixed slice buffers of the single call; it does not depend on the number of neighbours.
#pragma once

namespace {

// per-entry buffers of the multi call (the slice buffers - results, one chunk of trajectories - are PoolImproveDev's)
struct PoolImproveMultiDev {
  signed char* cur = nullptr; size_t cur_cap = 0;
  double* cur_obj = nullptr; int* act = nullptr; int* cnt = nullptr; int* off = nullptr; int* ent_inst = nullptr; int* ent_fam = nullptr;
  int4* moves = nullptr; PoolWord* words = nullptr; size_t ent_cap = 0;
  void drop_entries() {
    if (cur_obj) (void)hipFree(cur_obj); if (act) (void)hipFree(act); if (cnt) (void)hipFree(cnt); if (off) (void)hipFree(off);
    if (ent_inst) (void)hipFree(ent_inst); if (ent_fam) (void)hipFree(ent_fam); if (moves) (void)hipFree(moves); if (words) (void)hipFree(words);
    cur_obj = nullptr; act = nullptr; cnt = nullptr; off = nullptr; ent_inst = nullptr; ent_fam = nullptr; moves = nullptr; words = nullptr; ent_cap = 0;
  }
  bool ensure(size_t m, size_t fl) {
    if (m > ent_cap) {
      drop_entries();
      size_t want = 64; while (want < m) want <<= 1;
      HIP_OK(hipMalloc((void**)&cur_obj, want * sizeof(double))); HIP_OK(hipMalloc((void**)&act, want * sizeof(int))); HIP_OK(hipMalloc((void**)&cnt, want * sizeof(int)));
      HIP_OK(hipMalloc((void**)&off, (want + 1) * sizeof(int))); HIP_OK(hipMalloc((void**)&ent_inst, want * sizeof(int))); HIP_OK(hipMalloc((void**)&ent_fam, want * sizeof(int)));
      HIP_OK(hipMalloc((void**)&words, want * sizeof(PoolWord))); HIP_OK(hipMalloc((void**)&moves, want * POOL_MOVES_MAX * sizeof(int4)));
      ent_cap = want;   // (set when all eight are there: a failure half-way is taken up from the start)
    }
    if (m * fl > cur_cap) {
      if (cur) (void)hipFree(cur);
      cur = nullptr; cur_cap = 0;
      size_t want = 64 * fl; while (want < m * fl) want <<= 1;
      HIP_OK(hipMalloc((void**)&cur, want));
      cur_cap = want;
    }
    return true;
  }
};
std::map<int, PoolImproveMultiDev> g_pool_improve_multi_dev;   // by device ordinal; used under the device lock

// the slices of a pass, greedily in entry order: an entry opens a new slice when its (clamped) moves do not fit the results left of the current one
int pool_improve_slices(const int* move_counts, int entries, int* slice_first, int cap) {
  int ns = 1, sum = 0;
  for (int e = 0; e < entries; ++e) {
    const int c = std::min(std::max(move_counts[e], 0), POOL_MOVES_MAX);
    if (sum + c > PoolImproveDev::NB_MAX) { ns++; sum = 0; }
    sum += c;
  }
  if (ns + 1 > cap) return -3;
  ns = 0; sum = 0; slice_first[0] = 0;
  for (int e = 0; e < entries; ++e) {
    const int c = std::min(std::max(move_counts[e], 0), POOL_MOVES_MAX);
    if (sum + c > PoolImproveDev::NB_MAX) { slice_first[++ns] = e; sum = 0; }
    sum += c;
  }
  slice_first[++ns] = entries;
  return ns;
}

struct PoolImproveMultiOut {
  std::vector<PoolWord> first;   // pass 0, per entry
  std::vector<double> after; std::vector<int> moves;   // per entry
  std::vector<signed char> fix;  // the m records at the end
  std::vector<int> passes; std::vector<long> neighbours, iterations; std::vector<char> still_moving;   // per handle
  float dev_ms = 0.0f;
  std::string err;
};

// m entries (einst[e] ascending: the handle of entry e; efam[e] its filter; hfirst[h] .. hfirst[h + 1] the entries of handle h).  false: HIP error or
// the LDS refusal (O.err); nothing of any handle has been touched
bool pool_improve_multi_run(DevCtx& X, PoolImproveDev& G, PoolImproveMultiDev& M, FixedMultiDev& FM, const Layout& Y, int n_inst, const signed char* fix,
                            const std::vector<int>& einst, const std::vector<int>& efam, const std::vector<int>& hfirst, int m, int max_passes, PoolImproveMultiOut& O) {
  DevBuf& B = X.B; hipStream_t st = X.stream;
  const size_t fl = (size_t)Y.fixlen, row = (size_t)Y.N * Y.nz;
  const PoolDims dims = pool_dims(Y);
  const size_t gen_lds = 3 * fl + (size_t)pool_sites(dims) * sizeof(int);
  if (gen_lds > POOL_MOVES_LDS_MAX) { O.err = "miqp_solver_pool_improve_multi: the fix record of this shape does not fit the LDS of pool_moves_kernel three times"; std::fprintf(stderr, "[miqp_gpu] %s (%zu bytes)\n", O.err.c_str(), gen_lds); return false; }
  HIP_OK(hipFuncSetAttribute((const void*)pool_moves_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gen_lds));
  HIP_OK(hipMemcpyAsync(M.cur, fix, (size_t)m * fl, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(M.ent_inst, einst.data(), (size_t)m * 4, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(M.ent_fam, efam.data(), (size_t)m * 4, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemsetAsync(M.cnt, 0, (size_t)m * sizeof(int), st)); HIP_OK(hipMemsetAsync(M.act, 0, (size_t)m * sizeof(int), st)); HIP_OK(hipMemsetAsync(M.off, 0, (size_t)(m + 1) * sizeof(int), st));
  DevBuf Bp = B; Bp.qp_tol = QP_TOL_FINAL; Bp.use_cutoff = 0; Bp.ws_on = 0;
  PoolImproveArgs A;
  A.cur = M.cur; A.cur_obj = M.cur_obj; A.act = M.act; A.cnt = M.cnt; A.moves = M.moves; A.words = M.words; A.res = G.res; A.pool_fix = B.pool_fix;
  A.ent_inst = M.ent_inst; A.ent_fam = M.ent_fam; A.off = M.off; A.batch_inst = B.batch_inst;
  A.dims = dims; A.fixlen = (int)fl; A.m = m;
  std::vector<PoolWord> words(m); std::vector<int> cnt(m), first(m + 2), offh(m + 1);
  // one pass: counts[e] nodes of entry e (own: one each, the entry's own record), slice by slice; behind it the moves of the next pass and the read-back
  auto run_pass = [&](const std::vector<int>& counts, int own) -> bool {
    const int ns = miqp_gpu_pool_improve_plan(counts.data(), m, first.data(), m + 2);
    if (ns < 1) return false;
    offh[0] = 0;
    for (int e = 0; e < m; ++e) offh[e + 1] = offh[e] + counts[e];
    HIP_OK(hipEventRecord(X.ev0, st));
    for (int s = 0; s < ns; ++s) {
      const int e0 = first[s], e1 = first[s + 1], nodes = offh[e1] - offh[e0];
      if (nodes > PoolImproveDev::NB_MAX) { std::fprintf(stderr, "[miqp_gpu] miqp_solver_pool_improve_multi: a slice of %d nodes\n", nodes); return false; }
      for (int k0 = 0; k0 < nodes; k0 += FB_CHUNK) {
        const int bc = std::min(FB_CHUNK, nodes - k0);
        hipLaunchKernelGGL(pool_neighbour_kernel, dim3((bc + 3) / 4), dim3(256), 0, st, A, offh[e0] + k0, bc, own);
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemsetD32Async((hipDeviceptr_t)B.batch_count, bc, 1, st));
        HIP_OK(hipMemsetAsync(B.pool_big, 0, (size_t)bc, st)); HIP_OK(hipMemsetAsync(B.batch_large, 0, (size_t)bc, st)); HIP_OK(hipMemsetAsync(B.batch_depth, 0, (size_t)bc * 4, st));
        HIP_OK(hipMemsetAsync(B.inst_nodes, 0, (size_t)n_inst * 8, st)); HIP_OK(hipMemsetAsync(B.inst_iters, 0, (size_t)n_inst * 8, st)); HIP_OK(hipMemsetAsync(B.stat_rowiters, 0, 8, st));
        launch_ipm_batch(X, Bp, bc, st);
        FixedMultiArgs F;
        F.ovf_list = B.ovf_list; F.ovf_count = B.ovf_count; F.ovf2_list = B.ovf2_list; F.ovf2_count = B.ovf2_count;
        F.batch_ok = B.batch_ok; F.batch_it = B.batch_it; F.batch_obj = B.batch_obj; F.batch_viol = B.batch_viol; F.batch_Z = B.batch_Z; F.batch_inst = B.batch_inst;
        F.cobj = FM.d_cobj; F.hfirst = nullptr; F.seg = nullptr; F.seg_obj = nullptr; F.seg_idx = nullptr;   // (nseg = 0: the climb picks per entry, the kernel reads none of the four)
        F.res = G.res + k0; F.Z = G.Z;   // (the climb has no use for the trajectories: one chunk's worth is written over)
        F.bc = bc; F.base = k0; F.nseg = 0; F.n_inst = n_inst; F.row_doubles = (int)row; F.onchip = X.oc_grid > 0 ? 1 : 0; F.big = X.ocb_grid > 0 ? 1 : 0; F.soft = soft_cost_args(B, Y);
        hipLaunchKernelGGL(fixed_multi_collect_kernel, dim3(1 + std::min(FB_ROW_BLOCKS, (bc + FB_NT / 64 - 1) / (FB_NT / 64))), dim3(FB_NT), 0, st, F);
        HIP_OK(hipGetLastError());
      }
      if (e1 > e0) hipLaunchKernelGGL(pool_pick_kernel, dim3(e1 - e0), dim3(64), 0, st, A, e0, (int)PoolImproveDev::NB_MAX, own);
      HIP_OK(hipGetLastError());
    }
    hipLaunchKernelGGL(pool_moves_kernel, dim3(m), dim3(64), gen_lds, st, A);
    hipLaunchKernelGGL(pool_offsets_kernel, dim3(1), dim3(256), 0, st, A);
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(X.ev1, st));
    HIP_OK(hipMemcpyAsync(words.data(), M.words, (size_t)m * sizeof(PoolWord), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(cnt.data(), M.cnt, (size_t)m * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st)); HIP_OK(hipGetLastError());
    float ms = 0.0f; (void)hipEventElapsedTime(&ms, X.ev0, X.ev1); O.dev_ms += ms;
    return true;
  };
  if (!run_pass(std::vector<int>(m, 1), 1)) return false;
  O.first = words; O.after.resize(m); O.moves.assign(m, 0);
  for (int k = 0; k < m; ++k) O.after[k] = words[k].objective;
  O.passes.assign(n_inst, 0); O.neighbours.assign(n_inst, 0); O.iterations.assign(n_inst, 0); O.still_moving.assign(n_inst, 0);
  std::vector<long> th(n_inst);
  for (int pass = 0;;) {
    long total = 0;
    std::fill(th.begin(), th.end(), 0L);
    for (int k = 0; k < m; ++k) { if (cnt[k] < 0 || cnt[k] > POOL_MOVES_MAX) { std::fprintf(stderr, "[miqp_gpu] miqp_solver_pool_improve_multi: move count %d of entry %d\n", cnt[k], k); return false; } total += cnt[k]; th[einst[k]] += cnt[k]; }
    if (total == 0 || pass == max_passes) break;
    const std::vector<int> counts = cnt;   // (run_pass reads the next pass's counts into cnt)
    if (!run_pass(counts, 0)) return false;
    pass++;
    bool any = false;
    // a handle without neighbours in this pass has stopped, as the single call's loop stops when its move total is 0: its figures stay
    for (int h = 0; h < n_inst; ++h) {
      if (th[h] == 0) continue;
      O.passes[h]++; O.neighbours[h] += th[h];
      bool any_h = false;
      for (int k = hfirst[h]; k < hfirst[h + 1]; ++k) {
        O.iterations[h] += words[k].iterations;
        if (words[k].accepted) { any_h = true; O.moves[k]++; O.after[k] = words[k].objective; }
      }
      O.still_moving[h] = any_h && pass == max_passes ? 1 : 0;
      any = any || any_h;
    }
    if (!any) break;
  }
  O.fix.resize((size_t)m * fl);
  HIP_OK(hipMemcpy(O.fix.data(), M.cur, (size_t)m * fl, hipMemcpyDeviceToHost));
  return true;
}

}  // namespace

extern "C" {

int miqp_gpu_pool_improve_plan(const int* move_counts, int entries, int* slice_first, int cap) {
  if (!move_counts || !slice_first || entries <= 0 || cap < 0) return -1;
  return pool_improve_slices(move_counts, entries, slice_first, cap);
}

int miqp_solver_pool_improve_multi(miqp_solver_t* const* solvers, int n, int max_passes, miqp_pool_improve_c* out, int cap, int* counts) {
  if (!solvers || !out || !counts || n <= 0 || cap < 1) return -1;
  if (max_passes < 1 || max_passes > POOL_IMPROVE_PASSES_MAX) return -2;
  BatchShape bs;
  if (const int rc = fixed_multi_check(solvers, n, bs)) return rc;
  const Layout& Y = bs.Y; const size_t fl = (size_t)Y.fixlen;
  // entries of every handle, handle-major in the caller's order: ent[h] of them, the first is entry hfirst[h] of the call
  std::vector<int> ent(n), hfirst(n + 1, 0);
  for (int h = 0; h < n; ++h) {
    const miqp_solver_t* s = solvers[h];
    ent[h] = std::min(miqp_solver_pool_count(s), cap);
    if (ent[h] > 0 && (s->pool_fixlen != Y.fixlen || s->pool_fix.size() < (size_t)ent[h] * fl || s->pool_obj.size() < (size_t)ent[h])) return -1;
    hfirst[h + 1] = hfirst[h] + ent[h];
  }
  for (int h = 0; h < n; ++h)   // (a handle that kept nothing is left alone whatever its filter)
    if (ent[h] > 0 && (solvers[h]->pool_fam < 1 || solvers[h]->pool_fam >= POOL_FAM_TIMING)) {
      char msg[200]; std::snprintf(msg, sizeof msg, "miqp_solver_pool_improve_multi: handle %d of the call kept entries under filter %d; the climb needs a filter in 1 .. 15", h, solvers[h]->pool_fam);
      solvers[h]->err = msg;
      return -2;
    }
  const int m = hfirst[n];
  if (m > FB_CAP) return -5;
  if (m == 0) { for (int h = 0; h < n; ++h) counts[h] = 0; return 0; }   // (nothing to run: no device is touched)
  for (int h = 0; h < n; ++h) if (ent[h] > 0) solvers[h]->err.clear();   // (miqp_solver_last_error of a handle with entries speaks of this call from here on)
  { int ndev = 0; if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return -3; }
  const double t_call = wall_s();
  FixedMultiCall call;
  if (call.open(solvers, n, Y) != 0) return -3;
  std::vector<signed char> fix((size_t)m * fl); std::vector<int> einst(m), efam(m);
  for (int h = 0; h < n; ++h) {
    if (ent[h] > 0) std::memcpy(fix.data() + (size_t)hfirst[h] * fl, solvers[h]->pool_fix.data(), (size_t)ent[h] * fl);
    for (int k = hfirst[h]; k < hfirst[h + 1]; ++k) { einst[k] = h; efam[k] = solvers[h]->pool_fam; }
  }
  PoolImproveDev& G = g_pool_improve_dev[call.X->device]; PoolImproveMultiDev& M = g_pool_improve_multi_dev[call.X->device]; FixedMultiDev& FM = g_fixed_multi_dev[call.X->device];
  PoolImproveMultiOut O;
  if (!G.ensure(fl, (size_t)Y.N * Y.nz) || !M.ensure((size_t)m, fl) || !pool_improve_multi_run(*call.X, G, M, FM, Y, n, fix.data(), einst, efam, hfirst, m, max_passes, O)) {
    (void)hipStreamSynchronize(call.X->stream);
    if (!O.err.empty()) for (int h = 0; h < n; ++h) if (ent[h] > 0) solvers[h]->err = O.err;
    return -3;
  }
  const double call_s = wall_s() - t_call;
  int moved = 0;
  for (int h = 0; h < n; ++h) {
    miqp_solver_t* s = solvers[h];
    counts[h] = ent[h];
    if (ent[h] == 0) continue;   // (left alone: its last error and last timing stay those of what it did last)
    s->timing[0] = call_s; s->timing[1] = O.dev_ms * 1e-3; s->timing[2] = O.passes[h]; s->timing[3] = (double)O.neighbours[h]; s->timing[4] = (double)O.iterations[h]; s->timing[5] = O.still_moving[h] ? 1 : 0;
    miqp_pool_improve_c* const o = out + (size_t)h * cap;
    for (int k = 0; k < ent[h]; ++k) {
      const int e = hfirst[h] + k;
      const bool live = O.first[e].accepted != 0;
      o[k].before = O.first[e].objective; o[k].after = live ? O.after[e] : o[k].before; o[k].moves = live ? O.moves[e] : 0; o[k].status = live ? 0 : 1;
      if (!live) continue;   // (an entry whose own QP is not feasible at the tight tolerance stays as it was found)
      std::memcpy(s->pool_fix.data() + (size_t)k * fl, O.fix.data() + (size_t)e * fl, fl);
      s->pool_obj[k] = o[k].after;
      if (o[k].moves > 0) moved++;
    }
    s->pr_n = 0; std::vector<char>().swap(s->pr_ok); std::vector<signed char>().swap(s->pr_fix); std::vector<double>().swap(s->pr_Z);
    if (O.still_moving[h]) {
      char msg[200]; std::snprintf(msg, sizeof msg, "miqp_solver_pool_improve_multi: an entry still moved in the last of %d passes; more passes may improve the pool further", max_passes);
      s->err = msg;
    }
  }
  return moved;
}

}  // extern "C"

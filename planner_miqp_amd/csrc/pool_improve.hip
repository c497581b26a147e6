// pool_improve.hip - every kept entry of the solution pool hill-climbed inside its own manoeuvre class, for one handle (miqp_solver_pool_improve) and for
// the pools of many in one device call (miqp_solver_pool_improve_multi; the slices of a pass as a pure host function, miqp_gpu_pool_improve_plan), and
// decision records through the fixed chain (miqp_solver_solve_decisions).  DESIGN.md 6f, 6g.
//
// The manoeuvre filter (solution_pool.hip) keeps one entry per class, and what it keeps is the smallest LEAF of the class the search happened to
// evaluate, not the class's best trajectory.  What separates such a leaf from a good one is WHEN a car changes its alternative, not WHAT it changes
// to (the premise of lns_kernel), and a change of timing leaves the timing-free signature of a site unchanged by construction.  So
// the local search of a class is lns_kernel's neighbourhood restricted to the moves that keep the signature:
//
//   a MOVE is (first, stride, count, value): the bytes d[first + k * stride], k < count, take `value`.  Of a site (pool_site: the bytes b[i] of one
//   disjunction along the horizon) every CHANGE POINT i = 2 .. N - 1 with b[i] != b[i - 1], both decided, offers
//     L1  b[i] := b[i - 1]                 L2  b[i], b[i + 1] := b[i - 1]   (i + 1 < N)       the change one or two steps later
//     E1  b[i - 1] := b[i]                 E2  b[i - 2], b[i - 1] := b[i]   (i - 2 >= 1)      ... or earlier
//   Step 0 is never written and every value is one the site already holds, so it is a valid alternative of that site.  A move is KEPT when the
//   site's family is not in the filter or the site's signature is the same behind it (a move that swallows a whole run leaves the class).  Order:
//   site, change point, L1 L2 E1 E2; at most POOL_MOVES_MAX per record, the first ones in that order.
//
// pool_site_moves below is that definition, once, for the host (miqp_gpu_pool_moves) and the device (pool_moves_kernel).
//
// The climb, per pass, all on the solver stream (the steps the kernels share with the explore's and the settle's are in pool_blocks.hip):
//   pool_moves_kernel      one wavefront per entry: the record staged and signed in LDS, the kept moves of its sites under the ENTRY's filter
//                          counted, numbered and written to the move table in HBM (pool_count_scan_emit, one lane per site)
//   pool_offsets_kernel    one workgroup: the exclusive scan of the per-entry counts, off[0 .. m] - neighbour off[e] + j is move j of entry e
//   pool_neighbour_kernel  one wavefront per node of the chunk being launched: neighbour number -> (entry, move), the entry's current record with
//                          the move patched in into slot k of pool_fix; the entry's instance into slot k of batch_inst
//   fixed_chunk            the chain of the fixed calls with its resets and settings and fixed_collect_kernel behind it, without segments (fixed_chain.hip)
//   pool_pick_kernel       one wavefront per entry over its contiguous range of results: the feasible neighbour of the lowest objective, ties to the
//                          lower move number; accepted when it is below the entry's objective by more than 1e-9 (1 + |objective|) - then the move is
//                          patched into the entry's current record and the objective replaced
// MANY HANDLES.  The product's path is a drained queue of hundreds to thousands of handles, and a loop of one-handle calls over them pays per handle a
// device lock, a compile_instance, an upload of the tables, per pass a chain of launches that is as long for 19 neighbours as for 1024, and per pass a
// host synchronisation.  So the climb is written over the entries of n handles, numbered handle-major in the caller's order: every entry carries its
// handle's index in the call (ent_inst, which pool_neighbour_kernel writes to batch_inst beside the node's record, so that the node kernels read that
// handle's tables) and its handle's filter (ent_fam, which pool_moves_kernel reads); the dims are common (batch_layout).  ONE pass of the call is one
// pass of every handle that still moves, and the neighbours of all of them fill common launch groups of FB_CHUNK nodes.  Per entry nothing else
// differs, so a handle's entries get the same bits whatever else is in the call: a node's answer is a function of its record and its instance's
// tables alone.  miqp_solver_pool_improve is the call with one handle.
//
// SLICES.  The results of a pass are not all kept at once: a slice is a run of whole entries whose neighbours fit PoolImproveDev::NB_MAX results,
// formed greedily in entry order (miqp_gpu_pool_improve_plan; the host loop calls that very function).  Per slice: its nodes in chunks of FB_CHUNK
// through pool_neighbour_kernel and fixed_chunk into the slice's results, pool_pick_kernel over the slice's entries.  Behind the last slice
// pool_moves_kernel and pool_offsets_kernel for the next pass.  The host knows the counts of a pass from the read-back of the pass before, enqueues
// all slices without waiting and synchronises once per pass.  Pass 0 - every entry's own record - is the same loop with one node per entry.
// Device memory: entries x (record + POOL_MOVES_MAX moves of 16 bytes + a few words), grown, not shrunk, cached per device, beside the fixed slice
// buffers; it does not depend on the number of neighbours.
// Owner computes: no atomics, no lock, no wavefront waits on another, no scratch.  The host reads back, per pass, one (accepted, iterations,
// objective) triple and one move count per entry.  An entry that did not move in a pass is not expanded again: its record, hence its neighbours and
// their answers, would be the ones just rejected.  (The literal loop - every live entry expanded in every pass - ends on the same records and
// objectives; it solves those neighbours again, so its neighbour and iteration counts are larger.)
#pragma once

namespace {

constexpr int POOL_IMPROVE_PASSES_MAX = 64;
constexpr size_t POOL_MOVES_LDS_MAX = 160 * 1024;   // dynamic LDS of pool_moves_kernel (3 fixlen + 4 sites bytes): the LDS of a gfx950 workgroup; a larger shape is refused with a message

// the kept moves of site s in their order; emit(j, move) receives move j of the site, the number of moves is returned.  rec: the record (the site's
// bytes are patched and restored on the way), sg0: its signature under fam at the site's bytes, sg1: -1 at the site's bytes, before and after
template <class Emit>
__host__ __device__ inline int pool_site_moves(const PoolDims& d, int fam, int s, signed char* rec, const signed char* sg0, signed char* sg1, Emit emit) {
  const PoolSite t = pool_site(d, s);
  const bool selected = (fam & t.family) != 0;
  int n = 0;
  for (int i = 2; i < d.N; ++i) {
    const signed char a = rec[t.first + (i - 1) * t.step], b = rec[t.first + i * t.step];
    if (a < 0 || b < 0 || a == b) continue;
    for (int kind = 0; kind < 4; ++kind) {
      int i0, cnt; signed char v;
      if (kind == 0) { i0 = i; cnt = 1; v = a; }
      else if (kind == 1) { if (i + 1 >= d.N) continue; i0 = i; cnt = 2; v = a; }
      else if (kind == 2) { i0 = i - 1; cnt = 1; v = b; }
      else { if (i - 2 < 1) continue; i0 = i - 2; cnt = 2; v = b; }
      bool keep = true;
      if (selected) {
        signed char* const p0 = rec + t.first + i0 * t.step; signed char* const p1 = rec + t.first + (i0 + cnt - 1) * t.step;
        const signed char o0 = *p0, o1 = *p1;
        *p0 = v; *p1 = v;
        pool_site_signature(d, fam, s, rec, sg1);
        for (int q = 0; q < d.N; ++q) { const int at = t.first + q * t.step; if (sg1[at] != sg0[at]) keep = false; sg1[at] = (signed char)-1; }
        *p0 = o0; *p1 = o1;
      }
      if (keep) { emit(n, PoolMove{t.first + i0 * t.step, t.step, cnt, (int)v}); n++; }
    }
  }
  return n;
}

// "below the current objective by more than the allowance" (the allowance of the active-set kernel's bound), every operation
// rounded on its own on both sides so that host code can restate it
__host__ __device__ inline bool pool_improves(double cur, double obj) {
#ifdef __HIP_DEVICE_COMPILE__
  return __dsub_rn(cur, obj) > __dmul_rn(1e-9, __dadd_rn(1.0, fabs(cur)));
#else
  volatile double gain = cur - obj, room = 1.0 + std::fabs(cur); volatile double allow = 1e-9 * room;
  return gain > allow;
#endif
}

struct PoolWord { int accepted, iterations; double objective; };   // what the host reads per entry and pass

struct PoolImproveArgs {
  signed char* cur; double* cur_obj; int* act; int* cnt; int4* moves; PoolWord* words;   // per entry: current record and objective, expand it in the next pass, moves of this pass
  const int* ent_inst; const int* ent_fam;   // per entry: its handle's index in the call and that handle's filter
  int* off;                         // [m + 1] exclusive scan of the clamped move counts (pool_offsets_kernel): neighbour off[e] + j is move j of entry e, off[m] the pass total
  const miqp_fixed_result_c* res;   // of the first node of the SLICE being picked (a slice: a run of whole entries whose nodes fit NB_MAX results)
  signed char* pool_fix;            // the chain's fix records: slot k of the chunk
  int* batch_inst;                  // the chain's instance of slot k
  PoolDims dims; int fixlen, m;     // (one shape for every handle of a call: batch_layout)
};

__global__ __launch_bounds__(64) void pool_moves_kernel(const PoolImproveArgs A) {
  extern __shared__ uint4 pm_lds[];   // the record, its signature, a second signature; behind them one int per site
  const int e = blockIdx.x, lane = threadIdx.x, chunks = A.fixlen >> 4;
  if (!A.act[e]) { if (lane == 0) A.cnt[e] = 0; return; }
  uint4* const rec4 = pm_lds; uint4* const sg04 = rec4 + chunks; uint4* const sg14 = sg04 + chunks;
  signed char* const rec = (signed char*)rec4; const signed char* const sg0 = (const signed char*)sg04; signed char* const sg1 = (signed char*)sg14;
  const int fam = A.ent_fam[e];
  pool_stage(rec4, (const uint4*)(A.cur + (size_t)e * A.fixlen), chunks, lane, sg04);
  for (int c = lane; c < chunks; c += 64) sg14[c] = make_uint4(~0u, ~0u, ~0u, ~0u);
  pool_sign(A.dims, fam, rec4, sg04, lane);
  // (a site reads and writes its own bytes of the record and of the second signature and no others: the lanes do not meet until the scan)
  const int total = pool_count_scan_emit(pool_sites(A.dims), (int*)(sg14 + chunks), A.moves + (size_t)e * POOL_MOVES_MAX, lane,
                                         [&](int s, auto emit) { return pool_site_moves(A.dims, fam, s, rec, sg0, sg1, emit); });
  if (lane == 0) A.cnt[e] = total;
}

// off[0 .. m] behind pool_moves_kernel: ONE workgroup, the exclusive scan of the clamped counts in tiles of 256 entries (pool_tile_scan).
// m <= 65536 entries of at most 512 moves: a pass total is at most 2^25
__global__ __launch_bounds__(256) void pool_offsets_kernel(const PoolImproveArgs A) {
  __shared__ int carry[4];
  int base = 0;
  for (int t0 = 0; t0 < A.m; t0 += 256) {   // (A.m is uniform: every thread meets every barrier)
    const int e = t0 + threadIdx.x;
    const int at = pool_tile_scan(e < A.m ? min(max(A.cnt[e], 0), POOL_MOVES_MAX) : 0, carry, base);
    if (e < A.m) A.off[e] = at;
  }
  if (threadIdx.x == 0) A.off[A.m] = base;
}

// nodes c0 .. c0 + bc - 1 of the pass into slots 0 .. bc - 1 of pool_fix and batch_inst; own: pass 0, node e is entry e's own record.  Else node g is
// move g - off[e] of the entry e with off[e] <= g < off[e + 1] (pool_entry_of), patched into the entry's record on its way (pool_stage)
__global__ __launch_bounds__(256) void pool_neighbour_kernel(const PoolImproveArgs A, int c0, int bc, int own) {
  const int lane = threadIdx.x & 63, slot = blockIdx.x * 4 + (threadIdx.x >> 6), chunks = A.fixlen >> 4;
  if (slot >= bc) return;
  int e = c0 + slot, j = -1;
  if (!own) {
    const int g = c0 + slot;
    if (g < 0 || g >= A.off[A.m]) return;
    e = pool_entry_of(A.off, A.m, g); j = g - A.off[e];
    if (j >= POOL_MOVES_MAX) return;
  }
  if (e < 0 || e >= A.m) return;
  const int4 mv = j >= 0 ? A.moves[(size_t)e * POOL_MOVES_MAX + j] : make_int4(0, 1, 0, 0);
  pool_stage((uint4*)(A.pool_fix + (size_t)slot * A.fixlen), (const uint4*)(A.cur + (size_t)e * A.fixlen), chunks, lane, nullptr, mv);
  if (lane == 0) A.batch_inst[slot] = A.ent_inst[e];
}

// entries e0 .. e0 + gridDim.x - 1: one slice, whose first node's result is A.res[0]; nb_max: results the buffer behind A.res holds
__global__ __launch_bounds__(64) void pool_pick_kernel(const PoolImproveArgs A, int e0, int nb_max, int own) {
  const int e = e0 + blockIdx.x, lane = threadIdx.x;
  if (e >= A.m) return;
  if (own) {
    if (lane == 0 && (int)blockIdx.x < nb_max) {
      const miqp_fixed_result_c r = A.res[blockIdx.x]; const int live = r.status == 0 ? 1 : 0;
      A.cur_obj[e] = r.objective; A.act[e] = live;
      A.words[e] = PoolWord{live, r.iterations, r.objective};
    }
    return;
  }
  const int off = A.off[e] - A.off[e0];
  int n = A.act[e] ? min(max(A.cnt[e], 0), POOL_MOVES_MAX) : 0;
  if (off < 0 || off + n > nb_max) n = 0;   // (the host forms the slices so that this does not happen: miqp_gpu_pool_improve_plan)
  const double cur = A.cur_obj[e];
  double bo = 1e308; int bj = 0x7FFFFFFF, it = 0;
  for (int j = lane; j < n; j += 64) {   // (a lane's moves ascend: a tie keeps the lower number)
    const miqp_fixed_result_c r = A.res[off + j];
    it += r.iterations;
    if (r.status == 0 && r.objective < bo) { bo = r.objective; bj = j; }
  }
  pool_wave_argmin(bo, bj);
  for (int d = 32; d >= 1; d >>= 1) it += __shfl_xor(it, d, 64);
  const bool acc = bj != 0x7FFFFFFF && pool_improves(cur, bo);
  if (acc) {
    const int4 mv = A.moves[(size_t)e * POOL_MOVES_MAX + bj];
    if (lane < mv.z) { const int at = mv.x + lane * mv.y; if ((unsigned)at < (unsigned)A.fixlen) A.cur[(size_t)e * A.fixlen + at] = (signed char)mv.w; }
  }
  if (lane == 0) {
    if (acc) A.cur_obj[e] = bo;
    A.act[e] = acc ? 1 : 0;
    A.words[e] = PoolWord{acc ? 1 : 0, it, acc ? bo : cur};
  }
}

// ---------------------------------------------------------------------------------------------------------------- device cache
// buffers of the climb and the explore, cached per device like FixedDev and never taken from the solver's pools (DevArr: grown, not shrunk).  The slice
// buffers - the collect kernel copies the chunk's trajectories: the climb has no use for them, one chunk's worth is written over:
struct PoolImproveDev {
  static constexpr int NB_MAX = MIQP_POOL_MAX * POOL_MOVES_MAX;   // results of a slice
  DevArr<miqp_fixed_result_c> res; DevArr<double> Z;
  bool ensure(size_t row) { return res.need(NB_MAX) && Z.need((size_t)FB_CHUNK * row); }
};

// ... and the per-entry buffers: never fewer than the MIQP_POOL_MAX places the explore fills
struct PoolEntryDev {
  DevArr<signed char> cur; DevArr<double> cur_obj; DevArr<int> act, cnt, off, ent_inst, ent_fam; DevArr<int4> moves; DevArr<PoolWord> words;
  bool ensure(size_t m, size_t fl) {
    static_assert(MIQP_POOL_MAX <= 64, "the smallest allocation holds a pool");
    return cur_obj.need(m, 64) && act.need(m, 64) && cnt.need(m, 64) && off.need(m, 64, 1) && ent_inst.need(m, 64) && ent_fam.need(m, 64) && words.need(m, 64) &&
           moves.need(m * POOL_MOVES_MAX, 64 * POOL_MOVES_MAX) && cur.need(m * fl, 64 * fl);
  }
};

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

struct PoolImproveOut {
  std::vector<PoolWord> first;   // pass 0, per entry
  std::vector<double> after; std::vector<int> moves;   // per entry
  std::vector<signed char> fix;  // the m records at the end
  std::vector<int> passes; std::vector<long> neighbours, iterations; std::vector<char> still_moving;   // per handle
  float dev_ms = 0.0f;
  std::string err;
};

// m entries of the call's handles (einst[e] ascending: the handle of entry e; efam[e] its filter; hfirst[h] .. hfirst[h + 1] the entries of handle h;
// `name`: the entry point, for the messages).  false: HIP error or the LDS refusal (O.err); nothing of any handle has been touched
bool pool_improve_run(const FixedCall& call, const char* name, const signed char* fix, const std::vector<int>& einst, const std::vector<int>& efam, const std::vector<int>& hfirst,
                      int m, int max_passes, PoolImproveOut& O) {
  DevCtx& X = *call.X; const Layout& Y = call.Y; const int n_inst = call.n;
  DevBuf& B = X.B; hipStream_t st = X.stream;
  const size_t fl = (size_t)Y.fixlen, row = (size_t)Y.N * Y.nz;
  PoolImproveDev& G = call_dev<PoolImproveDev>(X.device); PoolEntryDev& M = call_dev<PoolEntryDev>(X.device);
  if (!G.ensure(row) || !M.ensure((size_t)m, fl)) return false;
  const PoolDims dims = pool_dims(Y);
  const size_t gen_lds = 3 * fl + (size_t)pool_sites(dims) * sizeof(int);
  if (gen_lds > POOL_MOVES_LDS_MAX) { O.err = std::string(name) + ": the fix record of this shape does not fit the LDS of pool_moves_kernel three times"; std::fprintf(stderr, "[miqp_gpu] %s (%zu bytes)\n", O.err.c_str(), gen_lds); return false; }
  HIP_OK(hipFuncSetAttribute((const void*)pool_moves_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gen_lds));
  HIP_OK(hipMemcpyAsync(M.cur, fix, (size_t)m * fl, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(M.ent_inst, einst.data(), (size_t)m * 4, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(M.ent_fam, efam.data(), (size_t)m * 4, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemsetAsync(M.cnt, 0, (size_t)m * sizeof(int), st)); HIP_OK(hipMemsetAsync(M.act, 0, (size_t)m * sizeof(int), st)); HIP_OK(hipMemsetAsync(M.off, 0, (size_t)(m + 1) * sizeof(int), st));
  const DevBuf Bp = fixed_chain_settings(B);
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
      if (nodes > PoolImproveDev::NB_MAX) { std::fprintf(stderr, "[miqp_gpu] %s: a slice of %d nodes\n", name, nodes); return false; }
      for (int k0 = 0; k0 < nodes; k0 += FB_CHUNK) {
        const int bc = std::min(FB_CHUNK, nodes - k0);
        hipLaunchKernelGGL(pool_neighbour_kernel, dim3((bc + 3) / 4), dim3(256), 0, st, A, offh[e0] + k0, bc, own);
        HIP_OK(hipGetLastError());
        // (no segments: the climb picks per entry; it has no use for the trajectories, one chunk's worth is written over)
        if (!fixed_chunk(X, Bp, Y, call.dev(), n_inst, FixedChunk{bc, k0, G.res + k0, G.Z})) return false;
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
    for (int k = 0; k < m; ++k) { if (cnt[k] < 0 || cnt[k] > POOL_MOVES_MAX) { std::fprintf(stderr, "[miqp_gpu] %s: move count %d of entry %d\n", name, cnt[k], k); return false; } total += cnt[k]; th[einst[k]] += cnt[k]; }
    if (total == 0 || pass == max_passes) break;
    const std::vector<int> counts = cnt;   // (run_pass reads the next pass's counts into cnt)
    if (!run_pass(counts, 0)) return false;
    pass++;
    bool any = false;
    // a handle without neighbours in this pass has stopped: its figures stay
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

// What the handles receive of a climb: per handle with entries its out records (out + h * stride), the moved records and objectives of its pool, its
// last_timing and, when it still moved in the last pass, its last error; counts[h] (may be NULL) the entries.  Returns the entries that moved
int pool_improve_store(const FixedCall& call, const char* name, const std::vector<int>& hfirst, const PoolImproveOut& O, int max_passes, double t_call, miqp_pool_improve_c* out, int stride, int* counts) {
  const size_t fl = (size_t)call.Y.fixlen;
  const double call_s = wall_s() - t_call;
  int moved = 0;
  for (int h = 0; h < call.n; ++h) {
    miqp_solver_t* s = call.S[h]; const int ent = hfirst[h + 1] - hfirst[h];
    if (counts) counts[h] = ent;
    if (ent == 0) continue;   // (left alone: its last error and last timing stay those of what it did last)
    s->timing[0] = call_s; s->timing[1] = O.dev_ms * 1e-3; s->timing[2] = O.passes[h]; s->timing[3] = (double)O.neighbours[h]; s->timing[4] = (double)O.iterations[h]; s->timing[5] = O.still_moving[h] ? 1 : 0;
    miqp_pool_improve_c* const o = out + (size_t)h * stride;
    for (int k = 0; k < ent; ++k) {
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
      char msg[200]; std::snprintf(msg, sizeof msg, "%s: an entry still moved in the last of %d passes; more passes may improve the pool further", name, max_passes);
      s->err = msg;
    }
  }
  return moved;
}

// the climb of the first ent[h] entries of every handle of an open call.  Entries that moved, or -3 (the handles with entries then carry the run's refusal, if it gave one)
int pool_improve_call(const FixedCall& call, const char* name, const std::vector<int>& ent, int max_passes, double t_call, miqp_pool_improve_c* out, int stride, int* counts) {
  const int n = call.n; const size_t fl = (size_t)call.Y.fixlen;
  std::vector<int> hfirst(n + 1, 0);
  for (int h = 0; h < n; ++h) hfirst[h + 1] = hfirst[h] + ent[h];
  const int m = hfirst[n];
  std::vector<signed char> fix((size_t)m * fl); std::vector<int> einst(m), efam(m);
  for (int h = 0; h < n; ++h) {
    if (ent[h] > 0) std::memcpy(fix.data() + (size_t)hfirst[h] * fl, call.S[h]->pool_fix.data(), (size_t)ent[h] * fl);
    for (int k = hfirst[h]; k < hfirst[h + 1]; ++k) { einst[k] = h; efam[k] = call.S[h]->pool_fam; }
  }
  PoolImproveOut O;
  if (!pool_improve_run(call, name, fix.data(), einst, efam, hfirst, m, max_passes, O)) {
    (void)hipStreamSynchronize(call.X->stream);
    if (!O.err.empty()) for (int h = 0; h < n; ++h) if (ent[h] > 0) call.S[h]->err = O.err;
    return -3;
  }
  return pool_improve_store(call, name, hfirst, O, max_passes, t_call, out, stride, counts);
}

// a decision record against the instance's tables: every byte is -1 (undecided) or an alternative of its site
bool decisions_in_range(const HostInst& I, const Layout& Y, const int* T, const signed char* d) {
  const int C = I.C, N = I.N, O = I.O, L = I.L, E = I.E;
  for (int c = 0; c < C; ++c)
    for (int i = 0; i < N; ++i) {
      const int v = d[Y.f_reg + c * N + i];
      if (v < -1) return false;
      if (v >= 0) {
        const int q = v >> 2, h = v & 3;
        if (q >= T[Y.i_nposs + c]) return false;
        if (h != 3 && h >= std::max(1, T[Y.i_nhs + c * Y.P + q])) return false;
      }
      for (int pt = 0; pt < 5; ++pt) {
        const int e = d[Y.f_env + (c * N + i) * 5 + pt];
        if (e < -1 || e >= E) return false;
        for (int o = 0; o < O; ++o) {
          const int k = d[Y.f_obs + ((c * O + o) * N + i) * 5 + pt];
          if (k < -1 || k > L || (k == L && !I.obs_soft[o])) return false;
        }
      }
    }
  for (int p = 0; p < Y.NP; ++p)
    for (int i = 0; i < N; ++i)
      for (int g = 0; g < 4; ++g) { const int a = d[Y.f_c2c + (p * N + i) * 4 + g]; if (a < -1 || a > 3) return false; }
  return true;
}

}  // namespace

extern "C" {

int miqp_gpu_pool_moves_max(void) { return POOL_MOVES_MAX; }
int miqp_gpu_pool_improve_size(void) { return (int)sizeof(miqp_pool_improve_c); }

int miqp_gpu_pool_moves(int cars, int steps, int obstacles, int families, const signed char* decisions, int* moves4, int cap) {
  if (!decisions || !moves4 || cars <= 0 || steps <= 0 || obstacles < 0) return -1;
  if (families < 1 || families >= POOL_FAM_TIMING) return -2;
  const PoolDims d{cars, steps, obstacles, cars * (cars - 1) / 2};
  const size_t D = (size_t)pool_declen(d);
  std::vector<signed char> rec(decisions, decisions + D), sg0(D), sg1(D, (signed char)-1);
  pool_signature(d, families, rec.data(), sg0.data(), D);
  std::vector<PoolMove> mv;
  for (int s = 0, n = pool_sites(d); s < n && (int)mv.size() < POOL_MOVES_MAX; ++s)
    (void)pool_site_moves(d, families, s, rec.data(), sg0.data(), sg1.data(), [&](int, const PoolMove& m) { if ((int)mv.size() < POOL_MOVES_MAX) mv.push_back(m); });
  if (cap < (int)mv.size()) return -3;
  for (size_t k = 0; k < mv.size(); ++k) { moves4[4 * k] = mv[k].first; moves4[4 * k + 1] = mv[k].stride; moves4[4 * k + 2] = mv[k].count; moves4[4 * k + 3] = mv[k].value; }
  return (int)mv.size();
}

int miqp_solver_solve_decisions(miqp_solver_t* s, const signed char* decisions, int n, miqp_fixed_result_c* out, int* best) {
  if (s) s->drop_fixed_batch();
  if (!s || !s->has_inst || !decisions || !out || n <= 0) return -1;
  if (n > FB_CAP) return -5;
  const double t_call = wall_s();
  if (best) *best = -1;
  fixed_refuse(out, n);
  miqp_solver_t* one[1] = {s};
  BatchShape bs = batch_layout(one, 1);
  if (!bs.ok) return -2;
  const Layout& Y = bs.Y;
  const size_t fl = (size_t)Y.fixlen, D = (size_t)Y.f_c2n;
  // the tables for the range check, before any device is asked for: a call whose records are all refused touches none.  FixedCall::open
  // compiles the instance again for the run - deliberately: its tables belong to the call object, and one compile is small beside the chain
  std::vector<double> Dt(Y.dstride); std::vector<int> T(Y.istride);
  compile_instance(s->inst, Y, Dt.data(), T.data());
  std::vector<int> where; where.reserve(n);
  for (int k = 0; k < n; ++k) if (decisions_in_range(s->inst, Y, T.data(), decisions + (size_t)k * D)) where.push_back(k);
  const int m = (int)where.size();
  if (m == 0) return 0;   // (nothing to run: no device is touched)
  FixedCall call;
  if (call.open(one, 1, Y) != 0) return -3;
  std::vector<signed char> fix((size_t)m * fl, (signed char)-1);
  for (int c = 0; c < m; ++c) std::memcpy(fix.data() + (size_t)c * fl, decisions + (size_t)where[c] * D, D);
  const int first[2] = {0, n};   // (miqp_solver_fixed_batch_record hands out the trajectories of this call too)
  return fixed_answer(call, fix, std::vector<int>(m, 0), where, {0, m}, first, out, best, t_call);
}

int miqp_solver_pool_improve(miqp_solver_t* s, int max_passes, miqp_pool_improve_c* out, int cap) {
  if (s) s->err.clear();   // (miqp_solver_last_error speaks of this call from here on)
  if (!s || !s->has_inst || !out || cap < 1) return -1;
  if (s->pool_fam < 1 || s->pool_fam >= POOL_FAM_TIMING) return -2;   // without a filter, or with the timing bit, every move leaves the class
  if (max_passes < 1 || max_passes > POOL_IMPROVE_PASSES_MAX) return -2;
  const int m = std::min(miqp_solver_pool_count(s), cap);
  if (m == 0) return 0;
  { int ndev = 0; if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return -3; }
  miqp_solver_t* one[1] = {s};
  BatchShape bs = batch_layout(one, 1);
  if (!bs.ok || bs.Y.fixlen != s->pool_fixlen || s->pool_fix.size() < (size_t)m * bs.Y.fixlen) return -1;
  const double t_call = wall_s();
  FixedCall call;
  if (call.open(one, 1, bs.Y) != 0) return -3;
  return pool_improve_call(call, "miqp_solver_pool_improve", {m}, max_passes, t_call, out, 0, nullptr);
}

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
  std::vector<int> ent(n); int m = 0;   // the entries of every handle
  for (int h = 0; h < n; ++h) {
    const miqp_solver_t* s = solvers[h];
    ent[h] = std::min(miqp_solver_pool_count(s), cap);
    if (ent[h] > 0 && (s->pool_fixlen != Y.fixlen || s->pool_fix.size() < (size_t)ent[h] * fl || s->pool_obj.size() < (size_t)ent[h])) return -1;
    m += ent[h];
  }
  for (int h = 0; h < n; ++h)   // (a handle that kept nothing is left alone whatever its filter)
    if (ent[h] > 0 && (solvers[h]->pool_fam < 1 || solvers[h]->pool_fam >= POOL_FAM_TIMING)) {
      char msg[200]; std::snprintf(msg, sizeof msg, "miqp_solver_pool_improve_multi: handle %d of the call kept entries under filter %d; the climb needs a filter in 1 .. 15", h, solvers[h]->pool_fam);
      solvers[h]->err = msg;
      return -2;
    }
  if (m > FB_CAP) return -5;
  if (m == 0) { for (int h = 0; h < n; ++h) counts[h] = 0; return 0; }   // (nothing to run: no device is touched)
  for (int h = 0; h < n; ++h) if (ent[h] > 0) solvers[h]->err.clear();   // (miqp_solver_last_error of a handle with entries speaks of this call from here on)
  { int ndev = 0; if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return -3; }
  const double t_call = wall_s();
  FixedCall call;
  if (call.open(solvers, n, Y) != 0) return -3;
  return pool_improve_call(call, "miqp_solver_pool_improve_multi", ent, max_passes, t_call, out, cap, counts);
}

}  // extern "C"

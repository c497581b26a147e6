// pool_improve.hip - every kept entry of the solution pool hill-climbed inside its own manoeuvre class (miqp_solver_pool_improve), and decision
// records through the fixed-batch chain (miqp_solver_solve_decisions).  DESIGN.md 6f.
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
// The climb, per pass, all on the solver stream:
//   pool_moves_kernel      one wavefront per entry: the record staged in LDS, one lane per site (in a loop when there are more sites than lanes)
//                          counts its kept moves under the ENTRY's filter, a wave scan over the per-site counts numbers them, the lanes write them
//                          to the move table in HBM
//   pool_offsets_kernel    one workgroup: the exclusive scan of the per-entry counts, off[0 .. m] - neighbour off[e] + j is move j of entry e
//   pool_neighbour_kernel  one wavefront per node of the chunk being launched: neighbour number -> (entry, move) by binary search in the scan, the
//                          entry's current record in 16-byte loads, the move patched in registers, 16-byte stores into slot k of pool_fix; the
//                          entry's instance into slot k of batch_inst
//   launch_ipm_batch       the chain of the fixed batch with its settings (QP_TOL_FINAL, no cutoff, cold start), fixed_batch_collect_kernel behind it
//   pool_pick_kernel       one wavefront per entry over its contiguous range of results: the feasible neighbour of the lowest objective, ties to the
//                          lower move number; accepted when it is below the entry's objective by more than 1e-9 (1 + |objective|) - then the move is
//                          patched into the entry's current record and the objective replaced
// The kernels serve the entries of MANY handles as well (pool_improve_multi.hip: per entry its handle's index and filter; the results of a pass kept a
// SLICE of entries at a time); this file's call is their one-handle case - every entry instance 0 and the handle's filter, one slice.
// Owner computes: no atomics, no lock, no wavefront waits on another, no scratch.  The host reads back, per pass, one (accepted, iterations,
// objective) triple and one move count per entry.  An entry that did not move in a pass is not expanded again: its record, hence its neighbours and
// their answers, would be the ones just rejected.  (The literal loop - every live entry expanded in every pass - ends on the same records and
// objectives; it solves those neighbours again, so its neighbour and iteration counts are larger.)
#pragma once

namespace {

constexpr int POOL_MOVES_MAX = 512;   // moves per record (miqp_gpu_pool_moves_max): LNS_MAX
constexpr int POOL_IMPROVE_PASSES_MAX = 64;
constexpr size_t POOL_MOVES_LDS_MAX = 160 * 1024;   // dynamic LDS of pool_moves_kernel (3 fixlen + 4 sites bytes): the LDS of a gfx950 workgroup; a larger shape is refused with a message

struct PoolMove { int first, stride, count, value; };

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
  const int* ent_inst; const int* ent_fam;   // per entry: its handle's index in the call (0 in the single call) and that handle's filter
  int* off;                         // [m + 1] exclusive scan of the clamped move counts (pool_offsets_kernel): neighbour off[e] + j is move j of entry e, off[m] the pass total
  const miqp_fixed_result_c* res;   // of the first node of the SLICE being picked (a slice: a run of whole entries whose nodes fit NB_MAX results)
  signed char* pool_fix;            // the chain's fix records: slot k of the chunk
  int* batch_inst;                  // the chain's instance of slot k
  PoolDims dims; int fixlen, m;     // (one shape for every handle of a call: batch_layout)
};

__global__ __launch_bounds__(64) void pool_moves_kernel(const PoolImproveArgs A) {
  extern __shared__ uint4 pm_lds[];   // the record, its signature, a second signature; behind them one int per site
  const int e = blockIdx.x, lane = threadIdx.x, chunks = A.fixlen >> 4, nsites = pool_sites(A.dims);
  if (!A.act[e]) { if (lane == 0) A.cnt[e] = 0; return; }
  uint4* const rec4 = pm_lds; uint4* const sg04 = rec4 + chunks; uint4* const sg14 = sg04 + chunks;
  signed char* const rec = (signed char*)rec4; signed char* const sg0 = (signed char*)sg04; signed char* const sg1 = (signed char*)sg14;
  int* const scnt = (int*)(sg14 + chunks);
  const uint4* src = (const uint4*)(A.cur + (size_t)e * A.fixlen);
  for (int c = lane; c < chunks; c += 64) { rec4[c] = src[c]; sg04[c] = make_uint4(~0u, ~0u, ~0u, ~0u); sg14[c] = make_uint4(~0u, ~0u, ~0u, ~0u); }
  __syncthreads();
  // (a site reads and writes its own bytes of the three blocks and no others: the lanes do not meet until the scan)
  const int fam = A.ent_fam[e];
  for (int s = lane; s < nsites; s += 64) {
    pool_site_signature(A.dims, fam, s, rec, sg0);
    scnt[s] = pool_site_moves(A.dims, fam, s, rec, sg0, sg1, [](int, const PoolMove&) {});
  }
  __syncthreads();
  int total = 0;   // exclusive scan of the per-site counts, 64 sites at a time
  for (int s0 = 0; s0 < nsites; s0 += 64) {
    const int c = s0 + lane < nsites ? scnt[s0 + lane] : 0;
    int x = c;
    for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_up(x, o, 64); if (lane >= o) x += y; }
    if (s0 + lane < nsites) scnt[s0 + lane] = total + x - c;
    total += __shfl(x, 63, 64);
  }
  __syncthreads();
  int4* const out = A.moves + (size_t)e * POOL_MOVES_MAX;
  for (int s = lane; s < nsites; s += 64) {
    const int off = scnt[s];
    if (off >= POOL_MOVES_MAX) continue;
    (void)pool_site_moves(A.dims, fam, s, rec, sg0, sg1, [&](int j, const PoolMove& mv) { if (off + j < POOL_MOVES_MAX) out[off + j] = make_int4(mv.first, mv.stride, mv.count, mv.value); });
  }
  if (lane == 0) A.cnt[e] = min(total, POOL_MOVES_MAX);
}

__device__ inline void pool_patch_byte(uint4& v, int p, int val) {   // byte p (0 .. 15) of v, without indexing the registers
  const unsigned sh = (unsigned)(p & 3) * 8u, keep = ~(0xFFu << sh), bits = ((unsigned)val & 0xFFu) << sh;
  const int w = p >> 2;
  v.x = w == 0 ? (v.x & keep) | bits : v.x; v.y = w == 1 ? (v.y & keep) | bits : v.y;
  v.z = w == 2 ? (v.z & keep) | bits : v.z; v.w = w == 3 ? (v.w & keep) | bits : v.w;
}

// off[0 .. m] behind pool_moves_kernel: ONE workgroup, tiles of 256 entries - a wave scan per wavefront, the four wavefront totals through LDS, the
// running total of the tiles before in a register of every lane.  m <= 65536 entries of at most 512 moves: a pass total is at most 2^25
__global__ __launch_bounds__(256) void pool_offsets_kernel(const PoolImproveArgs A) {
  __shared__ int carry[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int base = 0;
  for (int t0 = 0; t0 < A.m; t0 += 256) {   // (A.m is uniform: every lane meets every barrier)
    const int e = t0 + tid;
    const int c = e < A.m ? min(max(A.cnt[e], 0), POOL_MOVES_MAX) : 0;
    int x = c;
    for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_up(x, o, 64); if (lane >= o) x += y; }
    if (lane == 63) carry[wave] = x;
    __syncthreads();
    int before = 0;
    for (int w = 0; w < 4; ++w) before += w < wave ? carry[w] : 0;
    if (e < A.m) A.off[e] = base + before + x - c;
    base += carry[0] + carry[1] + carry[2] + carry[3];
    __syncthreads();
  }
  if (tid == 0) A.off[A.m] = base;
}

// nodes c0 .. c0 + bc - 1 of the pass into slots 0 .. bc - 1 of pool_fix and batch_inst; own: pass 0, node e is entry e's own record.  Else node g is
// move g - off[e] of the entry e with off[e] <= g < off[e + 1]: a binary search of at most 17 probes, the same in every lane of the wavefront
__global__ __launch_bounds__(256) void pool_neighbour_kernel(const PoolImproveArgs A, int c0, int bc, int own) {
  const int lane = threadIdx.x & 63, slot = blockIdx.x * 4 + (threadIdx.x >> 6), chunks = A.fixlen >> 4;
  if (slot >= bc) return;
  int e = c0 + slot, j = -1;
  if (!own) {
    const int g = c0 + slot;
    if (g < 0 || g >= A.off[A.m]) return;
    int lo = 0, hi = A.m;   // off[lo] <= g < off[hi]
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (A.off[mid] <= g) lo = mid; else hi = mid; }
    e = lo; j = g - A.off[lo];
    if (j >= POOL_MOVES_MAX) return;
  }
  if (e < 0 || e >= A.m) return;
  const int4 mv = j >= 0 ? A.moves[(size_t)e * POOL_MOVES_MAX + j] : make_int4(0, 1, 0, 0);
  const uint4* src = (const uint4*)(A.cur + (size_t)e * A.fixlen);
  uint4* dst = (uint4*)(A.pool_fix + (size_t)slot * A.fixlen);
  for (int c = lane; c < chunks; c += 64) {
    uint4 v = src[c];
    for (int k = 0; k < mv.z; ++k) { const int p = mv.x + k * mv.y - c * 16; if ((unsigned)p < 16u) pool_patch_byte(v, p, mv.w); }
    dst[c] = v;
  }
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
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const double oo = __shfl_xor(bo, d, 64); const int oj = __shfl_xor(bj, d, 64);
    it += __shfl_xor(it, d, 64);
    if (oo < bo || (oo == bo && oj < bj)) { bo = oo; bj = oj; }
  }
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
// buffers of the climb, cached per device like FixedBatchDev and never taken from the solver's pools (grown, not shrunk)
struct PoolImproveDev {
  signed char* cur = nullptr; size_t cur_cap = 0; double* Z = nullptr; size_t z_cap = 0;
  double* cur_obj = nullptr; int* act = nullptr; int* cnt = nullptr; int4* moves = nullptr; PoolWord* words = nullptr;
  miqp_fixed_result_c* res = nullptr; double* best_obj = nullptr; int* best_idx = nullptr;
  int* ent_inst = nullptr; int* ent_fam = nullptr; int* off = nullptr;   // what the kernels read per entry since they serve many handles: 0, the handle's filter; the scan
  static constexpr int NB_MAX = MIQP_POOL_MAX * POOL_MOVES_MAX;   // neighbours of a pass
  bool ensure(size_t fl, size_t row) {
    // (each of the fixed-size buffers on its own: an allocation that failed half-way is taken up where it stopped, nothing is allocated twice)
    if (!cur_obj) HIP_OK(hipMalloc((void**)&cur_obj, MIQP_POOL_MAX * sizeof(double)));
    if (!act) HIP_OK(hipMalloc((void**)&act, MIQP_POOL_MAX * sizeof(int)));
    if (!cnt) HIP_OK(hipMalloc((void**)&cnt, MIQP_POOL_MAX * sizeof(int)));
    if (!words) HIP_OK(hipMalloc((void**)&words, MIQP_POOL_MAX * sizeof(PoolWord)));
    if (!res) HIP_OK(hipMalloc((void**)&res, (size_t)NB_MAX * sizeof(miqp_fixed_result_c)));
    if (!best_obj) HIP_OK(hipMalloc((void**)&best_obj, (NB_MAX / FB_CHUNK + 1) * sizeof(double)));
    if (!best_idx) HIP_OK(hipMalloc((void**)&best_idx, (NB_MAX / FB_CHUNK + 1) * sizeof(int)));
    if (!moves) HIP_OK(hipMalloc((void**)&moves, (size_t)NB_MAX * sizeof(int4)));
    if (!ent_inst) HIP_OK(hipMalloc((void**)&ent_inst, MIQP_POOL_MAX * sizeof(int)));
    if (!ent_fam) HIP_OK(hipMalloc((void**)&ent_fam, MIQP_POOL_MAX * sizeof(int)));
    if (!off) HIP_OK(hipMalloc((void**)&off, (MIQP_POOL_MAX + 1) * sizeof(int)));
    if (MIQP_POOL_MAX * fl > cur_cap) {
      if (cur) (void)hipFree(cur);
      cur = nullptr; cur_cap = 0;
      HIP_OK(hipMalloc((void**)&cur, MIQP_POOL_MAX * fl));
      cur_cap = MIQP_POOL_MAX * fl;
    }
    if ((size_t)FB_CHUNK * row > z_cap) {   // (the collect kernel copies the chunk's trajectories: the climb has no use for them, one chunk's worth is written over)
      if (Z) (void)hipFree(Z);
      Z = nullptr; z_cap = 0;
      HIP_OK(hipMalloc((void**)&Z, (size_t)FB_CHUNK * row * sizeof(double)));
      z_cap = (size_t)FB_CHUNK * row;
    }
    return true;
  }
};
std::map<int, PoolImproveDev> g_pool_improve_dev;   // by device ordinal; used under the device lock

struct PoolImproveOut {
  std::vector<PoolWord> first;          // pass 0
  std::vector<double> after; std::vector<int> moves;
  std::vector<signed char> fix;         // the m records at the end
  int passes = 0; long neighbours = 0, iterations = 0; bool still_moving = false; float dev_ms = 0.0f;
  std::string err;
};

// false: HIP error (nothing of the handle has been touched)
bool pool_improve_run(DevCtx& X, PoolImproveDev& G, const FixedBatchCall& call, int fam, const signed char* fix, int m, int max_passes, PoolImproveOut& O) {
  DevBuf& B = X.B; hipStream_t st = X.stream; const Layout& Y = call.Y;
  const size_t fl = (size_t)Y.fixlen, row = (size_t)Y.N * Y.nz;
  const PoolDims dims = pool_dims(Y);
  std::vector<int> ident(FB_CHUNK); for (int k = 0; k < FB_CHUNK; ++k) ident[k] = k;
  HIP_OK(hipMemcpyAsync((void*)B.inst_d, call.D.data(), call.D.size() * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync((void*)B.inst_i, call.T.data(), call.T.size() * 4, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(B.batch_node, ident.data(), (size_t)FB_CHUNK * 4, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemsetAsync(B.batch_inst, 0, (size_t)FB_CHUNK * 4, st));
  HIP_OK(hipMemcpyAsync(G.cur, fix, (size_t)m * fl, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemsetAsync(G.cnt, 0, MIQP_POOL_MAX * sizeof(int), st)); HIP_OK(hipMemsetAsync(G.act, 0, MIQP_POOL_MAX * sizeof(int), st));
  HIP_OK(hipMemsetAsync(G.ent_inst, 0, MIQP_POOL_MAX * sizeof(int), st)); HIP_OK(hipMemsetAsync(G.off, 0, (MIQP_POOL_MAX + 1) * sizeof(int), st));
  HIP_OK(hipMemsetD32Async((hipDeviceptr_t)G.ent_fam, fam, MIQP_POOL_MAX, st));
  DevBuf Bp = B; Bp.qp_tol = QP_TOL_FINAL; Bp.use_cutoff = 0; Bp.ws_on = 0;
  PoolImproveArgs A;
  A.cur = G.cur; A.cur_obj = G.cur_obj; A.act = G.act; A.cnt = G.cnt; A.moves = G.moves; A.words = G.words; A.res = G.res; A.pool_fix = B.pool_fix;
  A.ent_inst = G.ent_inst; A.ent_fam = G.ent_fam; A.off = G.off; A.batch_inst = B.batch_inst;
  A.dims = dims; A.fixlen = (int)fl; A.m = m;
  const size_t gen_lds = 3 * fl + (size_t)pool_sites(dims) * sizeof(int);
  if (gen_lds > POOL_MOVES_LDS_MAX) { O.err = "miqp_solver_pool_improve: the fix record of this shape does not fit the LDS of pool_moves_kernel three times"; std::fprintf(stderr, "[miqp_gpu] %s (%zu bytes)\n", O.err.c_str(), gen_lds); return false; }
  HIP_OK(hipFuncSetAttribute((const void*)pool_moves_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gen_lds));
  // `total` nodes of a pass through the chain, a chunk at a time (the per-chunk resets of fixed_batch_run)
  auto solve_nodes = [&](int total, int own) -> bool {
    for (int c0 = 0, j = 0; c0 < total; c0 += FB_CHUNK, ++j) {
      const int bc = std::min(FB_CHUNK, total - c0);
      hipLaunchKernelGGL(pool_neighbour_kernel, dim3((bc + 3) / 4), dim3(256), 0, st, A, c0, bc, own);
      HIP_OK(hipGetLastError());
      HIP_OK(hipMemsetD32Async((hipDeviceptr_t)B.batch_count, bc, 1, st));
      HIP_OK(hipMemsetAsync(B.pool_big, 0, (size_t)bc, st)); HIP_OK(hipMemsetAsync(B.batch_large, 0, (size_t)bc, st)); HIP_OK(hipMemsetAsync(B.batch_depth, 0, (size_t)bc * 4, st));
      HIP_OK(hipMemsetAsync(B.inst_nodes, 0, 8, st)); HIP_OK(hipMemsetAsync(B.inst_iters, 0, 8, st)); HIP_OK(hipMemsetAsync(B.stat_rowiters, 0, 8, st));
      launch_ipm_batch(X, Bp, bc, st);
      FixedBatchArgs F;
      F.ovf_list = B.ovf_list; F.ovf_count = B.ovf_count; F.ovf2_list = B.ovf2_list; F.ovf2_count = B.ovf2_count;
      F.batch_ok = B.batch_ok; F.batch_it = B.batch_it; F.batch_obj = B.batch_obj; F.batch_viol = B.batch_viol; F.batch_Z = B.batch_Z;
      F.res = G.res + c0; F.Z = G.Z; F.best_obj = G.best_obj + j; F.best_idx = G.best_idx + j;
      F.bc = bc; F.base = c0; F.row_doubles = (int)row; F.onchip = X.oc_grid > 0 ? 1 : 0; F.big = X.ocb_grid > 0 ? 1 : 0; F.cobj = call.cobj; F.soft = soft_cost_args(B, call.Y);
      hipLaunchKernelGGL(fixed_batch_collect_kernel, dim3(1 + std::min(FB_ROW_BLOCKS, (bc + FB_NT / 64 - 1) / (FB_NT / 64))), dim3(FB_NT), 0, st, F);
      HIP_OK(hipGetLastError());
    }
    return true;
  };
  // behind a pass: its pick, the moves of the next one, and the words of both to the host
  std::vector<PoolWord> words(m); std::vector<int> cnt(m);
  auto finish_pass = [&](int own) -> bool {
    hipLaunchKernelGGL(pool_pick_kernel, dim3(m), dim3(64), 0, st, A, 0, (int)PoolImproveDev::NB_MAX, own);   // (at most MIQP_POOL_MAX entries: one slice)
    hipLaunchKernelGGL(pool_moves_kernel, dim3(m), dim3(64), gen_lds, st, A);
    hipLaunchKernelGGL(pool_offsets_kernel, dim3(1), dim3(256), 0, st, A);
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(X.ev1, st));
    HIP_OK(hipMemcpyAsync(words.data(), G.words, (size_t)m * sizeof(PoolWord), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(cnt.data(), G.cnt, (size_t)m * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st)); HIP_OK(hipGetLastError());
    float ms = 0.0f; (void)hipEventElapsedTime(&ms, X.ev0, X.ev1); O.dev_ms += ms;
    return true;
  };
  HIP_OK(hipEventRecord(X.ev0, st));
  if (!solve_nodes(m, 1) || !finish_pass(1)) return false;
  O.first = words; O.after.resize(m); O.moves.assign(m, 0);
  for (int k = 0; k < m; ++k) O.after[k] = words[k].objective;
  for (;;) {
    long total = 0;
    for (int k = 0; k < m; ++k) { if (cnt[k] < 0 || cnt[k] > POOL_MOVES_MAX) { std::fprintf(stderr, "[miqp_gpu] miqp_solver_pool_improve: move count %d of entry %d\n", cnt[k], k); return false; } total += cnt[k]; }
    if (total == 0 || O.passes == max_passes) break;
    HIP_OK(hipEventRecord(X.ev0, st));
    if (!solve_nodes((int)total, 0) || !finish_pass(0)) return false;
    O.passes++; O.neighbours += total;
    bool any = false;
    for (int k = 0; k < m; ++k) {
      O.iterations += words[k].iterations;
      if (words[k].accepted) { any = true; O.moves[k]++; O.after[k] = words[k].objective; }
    }
    O.still_moving = any && O.passes == max_passes;
    if (!any) break;
  }
  O.fix.resize((size_t)m * fl);
  HIP_OK(hipMemcpy(O.fix.data(), G.cur, (size_t)m * fl, hipMemcpyDeviceToHost));
  return true;
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
  for (int k = 0; k < n; ++k) { out[k].status = 2; out[k].route = -1; out[k].iterations = 0; out[k].reserved = 0; out[k].objective = std::nan(""); out[k].violation = std::nan(""); }
  miqp_solver_t* one[1] = {s};
  BatchShape bs = batch_layout(one, 1);
  if (!bs.ok) return -2;
  const Layout& Y = bs.Y;
  const size_t fl = (size_t)Y.fixlen, D = (size_t)Y.f_c2n;
  // the tables for the range check, before any device is asked for: a call whose records are all refused touches none.  FixedBatchCall::open
  // compiles the instance again for the run - deliberately: its tables belong to the call object, and one compile is small beside the chain
  std::vector<double> Dt(Y.dstride); std::vector<int> T(Y.istride);
  compile_instance(s->inst, Y, Dt.data(), T.data());
  std::vector<int> where; where.reserve(n);
  for (int k = 0; k < n; ++k) if (decisions_in_range(s->inst, Y, T.data(), decisions + (size_t)k * D)) where.push_back(k);
  const int m = (int)where.size();
  if (m == 0) return 0;   // (nothing to run: no device is touched)
  FixedBatchCall call;
  if (call.open(s, Y) != 0) return -3;
  std::vector<signed char> fix((size_t)m * fl, (signed char)-1);
  for (int c = 0; c < m; ++c) std::memcpy(fix.data() + (size_t)c * fl, decisions + (size_t)where[c] * D, D);
  s->setup[0] = wall_s() - t_call;
  std::vector<miqp_fixed_result_c> tmp; std::vector<double> Z, bo; std::vector<int> bi; float dev_ms = 0.0f;
  if (call.run(fix, m, tmp, Z, bo, bi, dev_ms) != 0) return -3;
  for (int c = 0; c < m; ++c) out[where[c]] = tmp[c];
  {
    double b = 0; int at = -1;
    for (size_t j = 0; j < bo.size(); ++j) if (bi[j] >= 0 && bi[j] < m && (at < 0 || bo[j] < b)) { b = bo[j]; at = bi[j]; }
    if (best) *best = at < 0 ? -1 : where[at];
  }
  s->fb_n = n; s->fb_slot.assign(n, -1);   // (miqp_solver_fixed_batch_record hands out the trajectories of this call too)
  for (int c = 0; c < m; ++c) if (tmp[c].status == 0) s->fb_slot[where[c]] = c;
  s->fb_Z.swap(Z); s->fb_fix.swap(fix);
  const int nch = (m + FB_CHUNK - 1) / FB_CHUNK;
  s->timing[0] = wall_s() - t_call; s->timing[1] = dev_ms * 1e-3; s->timing[2] = nch; s->timing[3] = m; s->timing[4] = 0; s->timing[5] = 0;
  for (int c = 0; c < m; ++c) s->timing[4] += tmp[c].iterations;
  return 0;
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
  const Layout& Y = bs.Y; const size_t fl = (size_t)Y.fixlen;
  const double t_call = wall_s();
  FixedBatchCall call;
  if (call.open(s, Y) != 0) return -3;
  PoolImproveDev& G = g_pool_improve_dev[call.X->device];
  PoolImproveOut O;
  if (!G.ensure(fl, (size_t)Y.N * Y.nz) || !pool_improve_run(*call.X, G, call, s->pool_fam, s->pool_fix.data(), m, max_passes, O)) { (void)hipStreamSynchronize(call.X->stream); if (!O.err.empty()) s->err = O.err; return -3; }
  int moved = 0;
  for (int k = 0; k < m; ++k) {
    const bool live = O.first[k].accepted != 0;
    out[k].before = O.first[k].objective; out[k].after = live ? O.after[k] : out[k].before; out[k].moves = live ? O.moves[k] : 0; out[k].status = live ? 0 : 1;
    if (!live) continue;   // (an entry whose own QP is not feasible at the tight tolerance stays as it was found)
    std::memcpy(s->pool_fix.data() + (size_t)k * fl, O.fix.data() + (size_t)k * fl, fl);
    s->pool_obj[k] = out[k].after;
    if (out[k].moves > 0) moved++;
  }
  s->pr_n = 0; std::vector<char>().swap(s->pr_ok); std::vector<signed char>().swap(s->pr_fix); std::vector<double>().swap(s->pr_Z);
  s->timing[0] = wall_s() - t_call; s->timing[1] = O.dev_ms * 1e-3; s->timing[2] = O.passes; s->timing[3] = (double)O.neighbours; s->timing[4] = (double)O.iterations; s->timing[5] = O.still_moving ? 1 : 0;
  if (O.still_moving) {
    char msg[200]; std::snprintf(msg, sizeof msg, "miqp_solver_pool_improve: an entry still moved in the last of %d passes; more passes may improve the pool further", max_passes);
    s->err = msg;
  }
  return moved;
}

}  // extern "C"

// pool_carry.hip - the kept manoeuvres of one planning cycle carried into the pool of the next (miqp_solver_pool_carry).  DESIGN.md 6l.
//
// Counterpart of re-adding the members of a CPLEX solution pool as MIP starts of the next model.  A receding-horizon caller solves a new instance every
// cycle, and miqp_solver_set_params empties the pool: the fallback the explore paid for in cycle t is gone in cycle t + 1.  The CARRY takes the kept
// decision records of a SOURCE handle (cycle t), shifts them by `shift` steps along every site, re-expresses them in the alternatives of the
// DESTINATION handle's instance (cycle t + 1), settles them there (pool_settle.hip, its kernels as they are) and admits them to the destination's free
// places under its filter - one device-resident sequence on the solver stream of the destination's device.
//
// The SHIFT of a record (pool_shift_site below, once, for the host - miqp_gpu_pool_shift - and the device - pool_shift_kernel): for every site of
// pool_site and every step i = 1 .. N - 1 the destination byte is the source byte of step min(i + shift, N - 1) - the last decided state is held -,
// re-expressed: a region byte q * 4 + h becomes region_map[c * p_src + q] * 4 + h (the destination's possible-region index of the same region number;
// h belongs to the region's table, which both instances share), an environment byte e becomes env_map[e] (the destination piece of the same edges, or
// -1: undecided, the settle labels it), obstacle and car/car bytes stay (obstacle o of the destination is obstacle o of the source `shift` steps
// later: the caller's contract).  Negative bytes stay -1, step 0 of every site is -1, the bytes behind the decision bytes are -1.  A region byte
// without a target makes the whole record UNMAPPABLE: a record with an undecided region byte has no labels, so it cannot be settled.
//
// The call:
//   pool_shift_kernel        one wavefront per source entry: the record staged in LDS (16-byte loads), one lane per site - in a loop when there are
//                            more sites than lanes - through pool_shift_site, the maps read from device memory; the shifted record leaves in 16-byte
//                            stores, to its carry place (what an admitted entry stores) and to its record of the settle rounds; one word per record
//                            says "unmappable", one whether it is live in round 1
//   the settle rounds        pool_settle.hip unchanged: the destination's own kept entries (records 0 .. n0 - 1, so that their settled signatures
//                            exist - pass 0 of the settled explore) and the mappable carried records (n0 + k) in the same rounds; the compaction
//                            forms the live list of round 1 from the words of the shift kernel.  The answers of round 1 are kept: objective and
//                            iterations of an admitted entry are its FIRST solve's, the settled explore's convention
//   pool_carry_admit_kernel  ONE wavefront, a sibling of the explore's admission built from the same steps of pool_blocks.hip: the signatures of the
//                            destination's entries, then the feasible carried records in ascending (objective of the first solve, source number):
//                            beyond the cost cap (5), plain signature in the pool (3), no settled labels or settled signature in the pool (4), no
//                            place free (6), else appended behind the pool (0) - the entries admitted earlier count in both signature tests.  An
//                            EMPTY destination pool admits its first record whatever the cap; that record's objective is obj0 from then on
// Owner computes: no atomics, no scratch, no wavefront waits on another.  The shift kernel is latency-bound (at most 16 wavefronts); it exists so that
// shift, settle and admission stay one device-resident sequence, not for throughput.
// Out of scope: many (source, destination) pairs in one call; obstacle re-numbering; replacing a kept entry by a better carried one of its class
// (the climb's job); feeding carried records to the SEARCH as MIP starts (that would change solves).
#pragma once

namespace {

// the two maps of a carry; a NULL map is the identity.  region[c * p_src + q]: the destination's possible-region index of the source's q-th possible
// region of car c, or -1; env[e]: the destination's piece of the source's piece e, or -1
struct PoolCarryMaps { const int* region; int p_src; const int* env; int e_src; };

// site s of a record shifted into out (another record: out is not rec).  False: a region byte of the site has no target (it is -1 in out)
__host__ __device__ inline bool pool_shift_site(const PoolDims& d, int s, int shift, const PoolCarryMaps& M, const signed char* rec, signed char* out) {
  const PoolSite t = pool_site(d, s);
  bool ok = true;
  out[t.first] = -1;
  for (int i = 1; i < d.N; ++i) {
    const int j = i + shift < d.N - 1 ? i + shift : d.N - 1;
    int v = rec[t.first + j * t.step];
    if (v < 0) v = -1;
    else if (t.family == POOL_FAM_REGION && M.region) {   // (site s < C is the region site of car s)
      const int q = v >> 2, to = q < M.p_src ? M.region[s * M.p_src + q] : -1;
      if (to < 0 || to > 31) { v = -1; ok = false; } else v = to * 4 + (v & 3);
    } else if (t.family == POOL_FAM_ENVIRONMENT && M.env) {
      const int to = v < M.e_src ? M.env[v] : -1;
      v = to < 0 || to > 127 ? -1 : to;
    }
    out[t.first + i * t.step] = (signed char)v;
  }
  return ok;
}

struct PoolCarryArgs {
  PoolDims dims; int fixlen, fam, ns, n0, K, shift;   // ns source entries, n0 kept entries of the destination, K its capacity
  PoolCarryMaps maps;                 // (device memory)
  const signed char* src;             // [ns] the source's records
  signed char* shifted;               // [ns] the carry places: the shifted records
  int* unmappable;                    // [ns]
  // the settle rounds' words (PoolSettleArgs): record j < n0 is the destination's entry j, record n0 + k the carried record k
  signed char* lab; int* moved; const int* solves; const miqp_fixed_result_c* last;
  const miqp_fixed_result_c* first;   // [n0 + ns] the answers of round 1
  // the destination's places
  signed char* pool; double* pool_obj; signed char* sig; signed char* csig; int* has_sig;   // [MIQP_POOL_MAX]
  double max_rel;
  miqp_pool_carry_c* out;             // [ns]
  int* state;                         // [0] entries in the pool, [1] admitted
};

__global__ __launch_bounds__(64) void pool_shift_kernel(const PoolCarryArgs A) {
  extern __shared__ uint4 ps_lds[];   // the source record, the shifted record
  const int k = blockIdx.x, lane = threadIdx.x, chunks = A.fixlen >> 4;
  if (k >= A.ns) return;
  uint4* const rec = ps_lds; uint4* const out = rec + chunks;
  pool_stage(rec, (const uint4*)A.src + (size_t)k * chunks, chunks, lane, out);   // (out: all -1)
  __syncthreads();
  bool ok = true;
  for (int s = lane, n = pool_sites(A.dims); s < n; s += 64) ok = pool_shift_site(A.dims, s, A.shift, A.maps, (const signed char*)rec, (signed char*)out) && ok;
  const bool bad = __ballot(!ok) != 0ull;
  __syncthreads();
  pool_stage((uint4*)A.shifted + (size_t)k * chunks, out, chunks, lane);
  pool_stage((uint4*)A.lab + (size_t)(A.n0 + k) * chunks, out, chunks, lane);
  if (lane == 0) { A.unmappable[k] = bad ? 1 : 0; A.moved[A.n0 + k] = bad ? 0 : 1; }
}

constexpr int POOL_CARRY_ADMITTED = 0, POOL_CARRY_INFEASIBLE = 1, POOL_CARRY_UNMAPPABLE = 2, POOL_CARRY_KNOWN = 3, POOL_CARRY_SETTLED_KNOWN = 4, POOL_CARRY_BEYOND_CAP = 5,
              POOL_CARRY_NO_PLACE = 6;

__global__ __launch_bounds__(64) void pool_carry_admit_kernel(const PoolCarryArgs A) {
  extern __shared__ uint4 ca_lds[];   // the candidate's record, its signature, its settled labels, their signature
  const int lane = threadIdx.x, chunks = A.fixlen >> 4;
  const int ns = min(max(A.ns, 0), MIQP_POOL_MAX), K = min(max(A.K, 0), MIQP_POOL_MAX), n0 = min(max(A.n0, 0), K);
  uint4* const cand = ca_lds; uint4* const csg = cand + chunks; uint4* const clab = csg + chunks; uint4* const clsg = clab + chunks;
  uint4* const pool = (uint4*)A.pool; uint4* const sig = (uint4*)A.sig; uint4* const ssig = (uint4*)A.csig;
  // both signatures of the destination's own entries (a kept entry without settled labels has no settled signature: it matches nothing)
  for (int j = 0; j < n0; ++j) {
    pool_stage(cand, pool + (size_t)j * chunks, chunks, lane, csg);
    pool_sign(A.dims, A.fam, cand, csg, lane);
    pool_stage(sig + (size_t)j * chunks, csg, chunks, lane);
    pool_stage(clab, (const uint4*)A.lab + (size_t)j * chunks, chunks, lane, clsg);
    pool_sign(A.dims, A.fam, clab, clsg, lane);
    pool_stage(ssig + (size_t)j * chunks, clsg, chunks, lane);
  }
  for (int j = lane; j < MIQP_POOL_MAX; j += 64) A.has_sig[j] = j < n0 && A.last[j].status == 0 ? 1 : 0;
  // lane k holds source entry k: its record of `out` as far as it is known without a visit, and the objective the visiting order goes by
  double key = POOL_ADMIT_NONE;
  if (lane < ns) {
    const bool bad = A.unmappable[lane] != 0;
    const miqp_fixed_result_c r = A.first[n0 + lane];
    const bool feasible = !bad && r.status == 0 && r.objective < POOL_ADMIT_NONE;
    miqp_pool_carry_c o;
    o.status = bad ? POOL_CARRY_UNMAPPABLE : POOL_CARRY_INFEASIBLE; o.place = -1; o.solves = bad ? 0 : abs(A.solves[n0 + lane]); o.iterations = bad ? 0 : r.iterations;
    o.objective = bad ? __longlong_as_double(0x7FF8000000000000ll) : r.objective; o.reserved = 0; o.reserved1 = 0;
    A.out[lane] = o;
    if (feasible) key = r.objective;
  }
  __syncthreads();
  int n = n0, added = 0;
  double obj0 = n0 > 0 ? A.pool_obj[0] : 0.0;
  for (int visit = 0; visit < ns; ++visit) {
    double bo = key; int bg = key < POOL_ADMIT_NONE ? lane : 0x7FFFFFFF;
    pool_wave_argmin(bo, bg);
    if (bg == 0x7FFFFFFF) break;
    if (lane == bg) key = POOL_ADMIT_NONE;
    int st;
    if (n > 0 && !pool_within_cap(obj0, bo, A.max_rel)) st = POOL_CARRY_BEYOND_CAP;
    else {
      pool_stage(cand, (const uint4*)A.shifted + (size_t)bg * chunks, chunks, lane, csg);
      pool_sign(A.dims, A.fam, cand, csg, lane);
      if (pool_known(csg, sig, n, chunks, lane)) st = POOL_CARRY_KNOWN;
      else if (A.solves[n0 + bg] == 0 || A.last[n0 + bg].status != 0) st = POOL_CARRY_SETTLED_KNOWN;   // (no settled labels)
      else {
        pool_stage(clab, (const uint4*)A.lab + (size_t)(n0 + bg) * chunks, chunks, lane, clsg);
        pool_sign(A.dims, A.fam, clab, clsg, lane);
        if (pool_known(clsg, ssig, n, chunks, lane, A.has_sig)) st = POOL_CARRY_SETTLED_KNOWN;
        else if (n >= K) st = POOL_CARRY_NO_PLACE;
        else {
          for (int c = lane; c < chunks; c += 64) { pool[(size_t)n * chunks + c] = cand[c]; sig[(size_t)n * chunks + c] = csg[c]; ssig[(size_t)n * chunks + c] = clsg[c]; }
          if (lane == 0) { A.pool_obj[n] = bo; A.has_sig[n] = 1; A.out[bg].place = n; }
          if (n == 0) obj0 = bo;
          st = POOL_CARRY_ADMITTED; n++; added++;
        }
      }
    }
    if (lane == 0) A.out[bg].status = st;
    __syncthreads();   // (the appended signatures are compared with the next record's)
  }
  if (lane == 0) { A.state[0] = n; A.state[1] = added; }
}

// buffers of the call beside the settle rounds', cached per device (DevArr: grown, not shrunk), and the events around its two kernels
struct PoolCarryDev {
  DevArr<signed char> src, shifted, pool, sig, csig; DevArr<int> rmap, emap, unmappable, has_sig, state; DevArr<double> pool_obj; DevArr<miqp_fixed_result_c> first; DevArr<miqp_pool_carry_c> out;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  bool ensure(size_t fl, size_t nr, size_t ne) {
    const size_t m = MIQP_POOL_MAX;
    for (auto& e : ev) if (!e) HIP_OK(hipEventCreate(&e));
    return src.need(m * fl) && shifted.need(m * fl) && pool.need(m * fl) && sig.need(m * fl) && csig.need(m * fl) && rmap.need(nr, 256) && emap.need(ne, 64) && unmappable.need(m) &&
           has_sig.need(m) && state.need(2) && pool_obj.need(m) && first.need(2 * m) && out.need(m);
  }
};

thread_local double g_pool_carry_last[2] = {0.0, 0.0};   // seconds of the calling thread's last carry in pool_shift_kernel and in pool_carry_admit_kernel

// Both maps of a carry from the two loaded instances, and what the carry refuses of a pair of instances (err: why).  rmap: C x p_src, emap: E of src
bool pool_carry_build_maps(const HostInst& A, const HostInst& B, std::vector<int>& rmap, int& p_src, std::vector<int>& emap, std::string& err) {
  if (A.C != B.C || A.N != B.N || A.O != B.O || A.L != B.L) { err = "the carry needs two instances of the same cars, steps, obstacles and obstacle edges"; return false; }
  if (A.obs_soft != B.obs_soft) { err = "the carry needs the same soft flags of the obstacles on both instances"; return false; }
  bool tables = A.R == B.R && A.frac == B.frac && A.acc_lim == B.acc_lim && A.jerk_lim == B.jerk_lim && A.vm == B.vm;
  for (int k = 0; k < 6 && tables; ++k) tables = A.poly[k] == B.poly[k];
  if (!tables) { err = "the carry needs the same region tables on both instances: the half-plane of a region byte belongs to its region's table"; return false; }
  const int C = A.C, R = A.R;
  p_src = max_possible(A);
  rmap.assign((size_t)C * p_src, -1);
  for (int c = 0; c < C; ++c) {
    std::vector<int> at(R, -1);
    for (int j = 0, q = 0; j < R; ++j) if (B.possible[c * R + j] == 1) at[j] = q++;
    for (int j = 0, q = 0; j < R; ++j) if (A.possible[c * R + j] == 1) rmap[(size_t)c * p_src + q++] = at[j];
  }
  emap.assign(A.E, -1);
  for (int e = 0; e < A.E; ++e) {
    const int n = A.env_off[e + 1] - A.env_off[e];
    for (int f = 0; f < B.E && emap[e] < 0; ++f)
      if (B.env_off[f + 1] - B.env_off[f] == n && std::equal(A.env_edges.begin() + (size_t)A.env_off[e] * 4, A.env_edges.begin() + (size_t)A.env_off[e + 1] * 4, B.env_edges.begin() + (size_t)B.env_off[f] * 4)) emap[e] = f;
  }
  return true;
}

// what the call found out before it touches a device
struct PoolCarryPlan { Layout Y; int ns, n0, K, p_src; std::vector<int> rmap, emap; };

// The device part of the carry.  own: the destination's n0 entries and src: the source's ns, both completed as miqp_solver_solve_decisions completes
// decision bytes.  false: HIP error or a refusal (err)
struct PoolCarryOut { std::vector<miqp_pool_carry_c> out; std::vector<signed char> fix; std::vector<double> obj; std::vector<int> solves; int n = 0, added = 0; PoolSettleTally tally; float dev_ms = 0, shift_ms = 0, admit_ms = 0; std::string err; };
bool pool_carry_run(const FixedCall& call, const PoolCarryPlan& P, int fam, int shift, double max_rel, const std::vector<signed char>& own, const std::vector<double>& own_obj, const std::vector<signed char>& src, PoolCarryOut& O) {
  DevCtx& X = *call.X; DevBuf& B = X.B; hipStream_t st = X.stream; const Layout& Y = P.Y;
  const size_t fl = (size_t)Y.fixlen; const int n = P.n0 + P.ns;
  static const char* const name = "miqp_solver_pool_carry";
  if (4 * fl > POOL_EXPLORE_LDS_MAX) {
    O.err = std::string(name) + ": the fix record of this shape does not fit the LDS of pool_carry_admit_kernel four times";
    std::fprintf(stderr, "[miqp_gpu] %s (%zu bytes)\n", O.err.c_str(), 4 * fl); return false;
  }
  if (!pool_label_fits(Y, name, O.err)) return false;
  PoolImproveDev& R = call_dev<PoolImproveDev>(X.device); PoolSettleDev& W = call_dev<PoolSettleDev>(X.device); PoolCarryDev& Q = call_dev<PoolCarryDev>(X.device);
  if (!R.ensure((size_t)Y.N * Y.nz) || !W.ensure((size_t)n, fl) || !Q.ensure(fl, P.rmap.size(), std::max<size_t>(P.emap.size(), 1)) || !pool_label_set_lds(Y)) return false;
  HIP_OK(hipFuncSetAttribute((const void*)pool_shift_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(2 * fl)));
  HIP_OK(hipFuncSetAttribute((const void*)pool_carry_admit_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(4 * fl)));
  const DevBuf Bp = fixed_chain_settings(B);
  const PoolSettleArgs S = pool_settle_args(W, B, Y, n);
  PoolCarryArgs A;
  A.dims = pool_dims(Y); A.fixlen = (int)fl; A.fam = fam; A.ns = P.ns; A.n0 = P.n0; A.K = P.K; A.shift = shift;
  A.maps = PoolCarryMaps{Q.rmap, P.p_src, Q.emap, (int)P.emap.size()};
  A.src = Q.src; A.shifted = Q.shifted; A.unmappable = Q.unmappable; A.lab = W.cur; A.moved = W.moved; A.solves = W.solves; A.last = W.last; A.first = Q.first;
  A.pool = Q.pool; A.pool_obj = Q.pool_obj; A.sig = Q.sig; A.csig = Q.csig; A.has_sig = Q.has_sig; A.max_rel = max_rel; A.out = Q.out; A.state = Q.state;
  std::vector<int> live0(n, 0); for (int j = 0; j < P.n0; ++j) live0[j] = 1;   // (the destination's own entries are live in round 1; the shift kernel says which carried ones are)
  HIP_OK(hipMemsetAsync(B.batch_inst, 0, (size_t)FB_CHUNK * 4, st));
  HIP_OK(hipMemcpyAsync(Q.src, src.data(), (size_t)P.ns * fl, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(Q.rmap, P.rmap.data(), P.rmap.size() * sizeof(int), hipMemcpyHostToDevice, st));
  if (!P.emap.empty()) HIP_OK(hipMemcpyAsync(Q.emap, P.emap.data(), P.emap.size() * sizeof(int), hipMemcpyHostToDevice, st));
  if (P.n0 > 0) {
    HIP_OK(hipMemcpyAsync(W.cur, own.data(), (size_t)P.n0 * fl, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(Q.pool, own.data(), (size_t)P.n0 * fl, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(Q.pool_obj, own_obj.data(), (size_t)P.n0 * sizeof(double), hipMemcpyHostToDevice, st));
  }
  HIP_OK(hipMemcpyAsync(W.moved, live0.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, st));
  HIP_OK(hipMemsetAsync(W.inst, 0, (size_t)n * sizeof(int), st)); HIP_OK(hipMemsetAsync(W.round_it, 0, (size_t)n * sizeof(int), st));
  HIP_OK(hipMemsetAsync(W.solves, 0, (size_t)n * sizeof(int), st)); HIP_OK(hipMemsetAsync(W.acc_it, 0, (size_t)n * sizeof(int), st));
  HIP_OK(hipMemsetAsync(W.last, 0xFF, (size_t)n * sizeof(miqp_fixed_result_c), st)); HIP_OK(hipMemsetAsync(Q.first, 0xFF, (size_t)n * sizeof(miqp_fixed_result_c), st));   // (status -1: never solved)
  HIP_OK(hipEventRecord(X.ev0, st));
  HIP_OK(hipEventRecord(Q.ev[0], st));
  hipLaunchKernelGGL(pool_shift_kernel, dim3(P.ns), dim3(64), 2 * fl, st, A);
  HIP_OK(hipGetLastError());
  HIP_OK(hipEventRecord(Q.ev[1], st));
  int live = 0;
  if (!pool_settle_compact(X, S, live, O.tally)) return false;   // (waits: live0 is a local)
  if (!pool_settle_rounds(call, Bp, S, R.Z, 1, live, O.tally, 1)) return false;
  HIP_OK(hipMemcpyAsync(Q.first, W.last, (size_t)n * sizeof(miqp_fixed_result_c), hipMemcpyDeviceToDevice, st));
  if (!pool_settle_rounds(call, Bp, S, R.Z, 2, live, O.tally)) return false;
  HIP_OK(hipEventRecord(Q.ev[2], st));
  hipLaunchKernelGGL(pool_carry_admit_kernel, dim3(1), dim3(64), 4 * fl, st, A);
  HIP_OK(hipGetLastError());
  HIP_OK(hipEventRecord(Q.ev[3], st));
  HIP_OK(hipEventRecord(X.ev1, st));
  int state[2] = {0, 0};
  O.out.resize(P.ns); O.fix.resize((size_t)MIQP_POOL_MAX * fl); O.obj.resize(MIQP_POOL_MAX); O.solves.resize(n);
  HIP_OK(hipMemcpyAsync(state, Q.state, sizeof state, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(O.out.data(), Q.out, (size_t)P.ns * sizeof(miqp_pool_carry_c), hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(O.fix.data(), Q.pool, (size_t)MIQP_POOL_MAX * fl, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(O.obj.data(), Q.pool_obj, (size_t)MIQP_POOL_MAX * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(O.solves.data(), W.solves, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st)); HIP_OK(hipGetLastError());
  (void)hipEventElapsedTime(&O.dev_ms, X.ev0, X.ev1); (void)hipEventElapsedTime(&O.shift_ms, Q.ev[0], Q.ev[1]); (void)hipEventElapsedTime(&O.admit_ms, Q.ev[2], Q.ev[3]);
  O.n = state[0]; O.added = state[1];
  if (O.n != P.n0 + O.added || O.added < 0 || O.added > P.ns || O.n > P.K) { std::fprintf(stderr, "[miqp_gpu] %s: %d entries behind %d, %d admitted\n", name, O.n, P.n0, O.added); return false; }
  return true;
}

// what both entries refuse of a pair of handles, -1 or -2, else 0 with the maps
int pool_carry_pair(const miqp_solver_t* src, const miqp_solver_t* dst, std::vector<int>& rmap, int& p_src, std::vector<int>& emap, std::string& err) {
  if (!src || !dst || src == dst || !src->has_inst || !dst->has_inst) return -1;
  return pool_carry_build_maps(src->inst, dst->inst, rmap, p_src, emap, err) ? 0 : -2;
}

}  // namespace

extern "C" {

int miqp_gpu_pool_carry_size(void) { return (int)sizeof(miqp_pool_carry_c); }

int miqp_gpu_pool_shift(int cars, int steps, int obstacles, int shift, const int* region_map, int p_src, const int* env_map, int e_src, const signed char* decisions, signed char* out, int len) {
  if (!decisions || !out || cars <= 0 || steps <= 0 || obstacles < 0 || (region_map && p_src <= 0) || (env_map && e_src < 0)) return -1;
  if (shift < 1 || shift > steps - 2) return -2;
  const PoolDims d{cars, steps, obstacles, cars * (cars - 1) / 2};
  const int D = pool_declen(d);
  if (len < D) return -3;
  const PoolCarryMaps M{region_map, p_src, env_map, e_src};
  std::memset(out, 0xFF, (size_t)len);
  bool ok = true;
  for (int s = 0, n = pool_sites(d); s < n; ++s) ok = pool_shift_site(d, s, shift, M, decisions, out) && ok;
  return ok ? D : -4;
}

int miqp_solver_pool_carry_maps(const miqp_solver_t* src, const miqp_solver_t* dst, int* region_map, int cap_r, int* env_map, int cap_e) {
  if (dst) const_cast<miqp_solver_t*>(dst)->err.clear();
  if (!region_map || !env_map || cap_r < 0 || cap_e < 0) return -1;
  std::vector<int> rmap, emap; int p_src = 0; std::string err;
  if (const int rc = pool_carry_pair(src, dst, rmap, p_src, emap, err)) { if (dst && !err.empty()) const_cast<miqp_solver_t*>(dst)->err = err; return rc; }
  if (cap_r < (int)rmap.size() || cap_e < (int)emap.size()) return -3;
  std::copy(rmap.begin(), rmap.end(), region_map); std::copy(emap.begin(), emap.end(), env_map);
  return p_src;
}

int miqp_solver_pool_carry(miqp_solver_t* dst, const miqp_solver_t* src, int shift, double max_rel, miqp_pool_carry_c* out, int cap) {
  static const char* const name = "miqp_solver_pool_carry";
  if (dst) dst->err.clear();   // (miqp_solver_last_error speaks of this call from here on)
  if (!out || cap < 0 || max_rel != max_rel) return -1;
  PoolCarryPlan P; std::string err;
  if (const int rc = pool_carry_pair(src, dst, P.rmap, P.p_src, P.emap, err)) { if (dst && !err.empty()) dst->err = err; return rc; }
  if (shift < 1 || shift > dst->inst.N - 2) return -2;
  P.K = std::min(dst->pool_cap, MIQP_POOL_MAX);
  if (P.K <= 0 || dst->pool_fam < 1 || dst->pool_fam >= POOL_FAM_TIMING) return -2;
  P.ns = std::min(miqp_solver_pool_count(src), MIQP_POOL_MAX); P.n0 = miqp_solver_pool_count(dst);
  if (cap < P.ns) return -2;
  miqp_solver_t* one[1] = {dst};
  BatchShape bs = batch_layout(one, 1);
  if (!bs.ok) { dst->err = bs.err; return -2; }
  P.Y = bs.Y;
  const size_t fl = (size_t)P.Y.fixlen, D = (size_t)P.Y.f_c2n;
  if (P.ns > 0 && (src->pool_fixlen != P.Y.fixlen || src->pool_fix.size() < (size_t)P.ns * fl)) return -1;
  if (P.n0 > 0 && (dst->pool_fixlen != P.Y.fixlen || dst->pool_fix.size() < (size_t)P.n0 * fl || dst->pool_obj.size() < (size_t)P.n0)) return -1;
  if (P.ns == 0 || P.n0 >= P.K) return 0;   // (nothing to carry, or no free place: no device is touched)
  { int ndev = 0; if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return -3; }
  const double t_call = wall_s();
  // decision bytes, completed as miqp_solver_solve_decisions completes them: the bytes behind them are "none"
  std::vector<signed char> own((size_t)P.n0 * fl, (signed char)-1), from((size_t)P.ns * fl, (signed char)-1);
  for (int j = 0; j < P.n0; ++j) std::memcpy(own.data() + (size_t)j * fl, dst->pool_fix.data() + (size_t)j * fl, D);
  for (int k = 0; k < P.ns; ++k) std::memcpy(from.data() + (size_t)k * fl, src->pool_fix.data() + (size_t)k * fl, D);
  const std::vector<double> own_obj(dst->pool_obj.begin(), dst->pool_obj.begin() + P.n0);
  const double setup_s = wall_s() - t_call;
  FixedCall call;
  if (call.open(one, 1, P.Y) != 0) return -3;
  PoolCarryOut O;
  if (!pool_carry_run(call, P, dst->pool_fam, shift, max_rel, own, own_obj, from, O)) {
    (void)hipStreamSynchronize(call.X->stream);
    if (!O.err.empty()) dst->err = O.err;
    return -3;
  }
  // the old entries stay as the handle holds them; the admitted ones go behind them
  dst->pool_fix.resize((size_t)P.n0 * fl); dst->pool_obj.resize(P.n0);
  dst->pool_fix.insert(dst->pool_fix.end(), O.fix.begin() + (size_t)P.n0 * fl, O.fix.begin() + (size_t)O.n * fl);
  dst->pool_obj.insert(dst->pool_obj.end(), O.obj.begin() + P.n0, O.obj.begin() + O.n);
  dst->pool_n = O.n; dst->pool_fixlen = (int)fl;
  if (!dst->has_sol && O.n > 0) dst->pool_carried = true;   // (a pool without a solve behind it: the carried entries are all it holds)
  dst->pr_n = 0; std::vector<char>().swap(dst->pr_ok); std::vector<signed char>().swap(dst->pr_fix); std::vector<double>().swap(dst->pr_Z);
  for (int k = 0; k < P.ns; ++k) out[k] = O.out[k];
  int still = 0;
  for (int k = 0; k < P.ns; ++k) if (O.solves[P.n0 + k] < 0) still++;
  if (still) {
    char msg[200]; std::snprintf(msg, sizeof msg, "%s: the labels of %d carried records still moved after %d solves; their settled signature is that of the last labels", name, still, POOL_PASSES);
    dst->err = msg;
  }
  dst->setup[0] = setup_s;
  dst->timing[0] = wall_s() - t_call; dst->timing[1] = O.dev_ms * 1e-3; dst->timing[2] = O.tally.groups; dst->timing[3] = (double)O.tally.solves; dst->timing[4] = (double)O.tally.iterations; dst->timing[5] = still ? 1 : 0;
  g_pool_carry_last[0] = O.shift_ms * 1e-3; g_pool_carry_last[1] = O.admit_ms * 1e-3;
  return O.added;
}

void miqp_gpu_pool_carry_last(double* shift_s, double* admit_s) {
  if (shift_s) *shift_s = g_pool_carry_last[0];
  if (admit_s) *admit_s = g_pool_carry_last[1];
}

}  // extern "C"

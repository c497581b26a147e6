// pool_carry.hip - the kept manoeuvres of one planning cycle carried into the pool of the next (miqp_solver_pool_carry, for many pairs of
// handles in one call miqp_solver_pool_carry_multi).  DESIGN.md 6l, 6m.
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
//   pool_shift_kernel        one wavefront per (pair, source entry): the record staged in LDS (16-byte loads), one lane per site - in a loop when there are
//                            more sites than lanes - through pool_shift_site, the maps read from device memory; the shifted record leaves in 16-byte
//                            stores, to its carry place (what an admitted entry stores) and to its record of the settle rounds; one word per record
//                            says "unmappable", one whether it is live in round 1
//   the settle rounds        pool_settle.hip unchanged: the destination's own kept entries (records 0 .. n0 - 1, so that their settled signatures
//                            exist - pass 0 of the settled explore) and the mappable carried records (n0 + k) in the same rounds; the compaction
//                            forms the live list of round 1 from the words of the shift kernel.  The answers of round 1 are kept: objective and
//                            iterations of an admitted entry are its FIRST solve's, the settled explore's convention
//   pool_carry_admit_kernel  ONE wavefront per pair, a sibling of the explore's admission built from the same steps of pool_blocks.hip: the signatures of the
//                            destination's entries, then the feasible carried records in ascending (objective of the first solve, source number):
//                            beyond the cost cap (5), plain signature in the pool (3), no settled labels or settled signature in the pool (4), no
//                            place free (6), else appended behind the pool (0) - the entries admitted earlier count in both signature tests.  An
//                            EMPTY destination pool admits its first record whatever the cap; that record's objective is obj0 from then on
// Owner computes: no atomics, no scratch, no wavefront waits on another.  The shift kernel is latency-bound (at most 16 wavefronts a pair); it exists
// so that shift, settle and admission stay one device-resident sequence, not for throughput.
//
// MANY PAIRS (miqp_solver_pool_carry_multi).  pool_carry_run carries the pools of np (source, destination) pairs whose destinations
// share a shape; miqp_solver_pool_carry is that run with one pair, on the same kernels.  The carry is almost only settle rounds, and a round costs
// the same for 30 records as for a thousand: the records of all pairs are numbered densely and pair-major - a pair's own kept entries, then its
// carried records - so that the rounds of all pairs fill common launch groups.  inst[k] of a record is its destination's index in the call.
// Everything per PLACE (the source records, the carry places, the destination's pool, both signatures, has_sig, `out`) is strided by MIQP_POOL_MAX
// per pair; per pair one row of words (PoolCarryPair: its first record, n0, ns, K, filter, p_src, e_src and where its two maps begin in the call's
// two map arrays) and six state words.  pool_shift_kernel runs one wavefront per (pair, source entry), pool_carry_admit_kernel one workgroup of one
// wavefront per pair: it sees its own records only, in the single call's order, so a pair's answer is the single call's, bit for bit.  What the
// single call's host summed over its rounds - launch groups, solves, iterations - the admission sums per pair from the per-record words `solves`
// and `acc_it`: a pair has at most 32 records, so its launch groups are the rounds in which it had a live record, the largest |solves| among them.
// Out of scope: obstacle re-numbering; replacing a kept entry by a better carried one of its class (the climb's job).
//
// STARTS FROM THE CARRIED POOL (miqp_solver_set_pool_starts, miqp_solver_pool_starts_last).  With the switch on, the solve behind a carry
// into an empty pool takes the first min(max_starts, entries) carried records as MIP-start roots of round 1 (prepare_instances, miqp_gpu.hip) -
// that makes the carry the whole counterpart of re-adding the old pool's members as MIP starts.  It is host code only: a pool entry already is a fix
// record, the start roots are nodes of round 1 like the warm-start roots, and eval_kernel, select_kernel and the capture kernels run as they are.
// The end of this file holds the setting and the places of the starts in the pool behind the solve.
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

// the words of one pair of a call (device memory, one row per pair).  first: the call's number of the pair's first record - records first .. first +
// n0 - 1 are the destination's own kept entries, first + n0 + k is the carried record k; ns source entries, n0 kept entries of the destination, K its
// capacity, fam its filter; rmap, emap: where the pair's maps begin in the call's two map arrays
struct PoolCarryPair { int first, n0, ns, K, fam, p_src, e_src, rmap, emap; };
constexpr int POOL_CARRY_STATE = 6;   // state words of a pair: entries in the pool, admitted, rounds with a live record, solves, their iterations, carried records still moving

// Places - the source's records, the carry places, the destination's pool and what goes with it - are strided by MIQP_POOL_MAX per pair: place
// p * MIQP_POOL_MAX + k is place k of pair p.  With one pair every numbering is the single call's
struct PoolCarryArgs {
  PoolDims dims; int fixlen, np, shift;   // np pairs
  const PoolCarryPair* pair;          // [np]
  const int* rmap; const int* emap;   // the region maps of all pairs, their environment maps (device memory)
  const signed char* src;             // [places] the sources' records
  signed char* shifted;               // [places] the carry places: the shifted records
  int* unmappable;                    // [places]
  // the settle rounds' words (PoolSettleArgs), by the call's record number
  signed char* lab; int* moved; const int* solves; const int* acc_it; const miqp_fixed_result_c* last;
  const miqp_fixed_result_c* first;   // [records] the answers of round 1
  // the destinations' places
  signed char* pool; double* pool_obj; signed char* sig; signed char* csig; int* has_sig;   // [places]
  double max_rel;
  miqp_pool_carry_c* out;             // [places]
  int* state;                         // [np][POOL_CARRY_STATE]
};

// One wavefront per (pair, source entry): blockIdx.x is the place
__global__ __launch_bounds__(64) void pool_shift_kernel(const PoolCarryArgs A) {
  extern __shared__ uint4 ps_lds[];   // the source record, the shifted record
  const int p = blockIdx.x / MIQP_POOL_MAX, k = blockIdx.x % MIQP_POOL_MAX, lane = threadIdx.x, chunks = A.fixlen >> 4;
  if (p >= A.np) return;
  const PoolCarryPair W = A.pair[p];
  if (k >= W.ns || W.n0 < 0) return;   // (uniform)
  const PoolCarryMaps maps{A.rmap + W.rmap, W.p_src, A.emap + W.emap, W.e_src};
  const size_t place = blockIdx.x, r = (size_t)W.first + W.n0 + k;
  uint4* const rec = ps_lds; uint4* const out = rec + chunks;
  pool_stage(rec, (const uint4*)A.src + place * chunks, chunks, lane, out);   // (out: all -1)
  __syncthreads();
  bool ok = true;
  for (int s = lane, n = pool_sites(A.dims); s < n; s += 64) ok = pool_shift_site(A.dims, s, A.shift, maps, (const signed char*)rec, (signed char*)out) && ok;
  const bool bad = __ballot(!ok) != 0ull;
  __syncthreads();
  pool_stage((uint4*)A.shifted + place * chunks, out, chunks, lane);
  pool_stage((uint4*)A.lab + r * chunks, out, chunks, lane);
  if (lane == 0) { A.unmappable[place] = bad ? 1 : 0; A.moved[r] = bad ? 0 : 1; }
}

constexpr int POOL_CARRY_ADMITTED = 0, POOL_CARRY_INFEASIBLE = 1, POOL_CARRY_UNMAPPABLE = 2, POOL_CARRY_KNOWN = 3, POOL_CARRY_SETTLED_KNOWN = 4, POOL_CARRY_BEYOND_CAP = 5,
              POOL_CARRY_NO_PLACE = 6;

// One workgroup of one wavefront per pair: blockIdx.x is the pair.  Everything below is the pair's own: its places, its records from its first on
__global__ __launch_bounds__(64) void pool_carry_admit_kernel(const PoolCarryArgs A) {
  extern __shared__ uint4 ca_lds[];   // the candidate's record, its signature, its settled labels, their signature
  const int lane = threadIdx.x, chunks = A.fixlen >> 4, p = blockIdx.x;
  if (p >= A.np) return;   // (uniform)
  const PoolCarryPair W = A.pair[p];
  const int ns = min(max(W.ns, 0), MIQP_POOL_MAX), K = min(max(W.K, 0), MIQP_POOL_MAX), n0 = min(max(W.n0, 0), K), fam = W.fam;
  const size_t pb = (size_t)p * MIQP_POOL_MAX;   // the pair's first place
  uint4* const cand = ca_lds; uint4* const csg = cand + chunks; uint4* const clab = csg + chunks; uint4* const clsg = clab + chunks;
  uint4* const pool = (uint4*)A.pool + pb * chunks; uint4* const sig = (uint4*)A.sig + pb * chunks; uint4* const ssig = (uint4*)A.csig + pb * chunks;
  const uint4* const shifted = (const uint4*)A.shifted + pb * chunks; const uint4* const lab = (const uint4*)A.lab + (size_t)W.first * chunks;
  const int* const solves = A.solves + W.first; const miqp_fixed_result_c* const last = A.last + W.first;
  int* const has_sig = A.has_sig + pb; double* const pool_obj = A.pool_obj + pb; miqp_pool_carry_c* const out = A.out + pb;
  // both signatures of the destination's own entries (a kept entry without settled labels has no settled signature: it matches nothing)
  for (int j = 0; j < n0; ++j) {
    pool_stage(cand, pool + (size_t)j * chunks, chunks, lane, csg);
    pool_sign(A.dims, fam, cand, csg, lane);
    pool_stage(sig + (size_t)j * chunks, csg, chunks, lane);
    pool_stage(clab, lab + (size_t)j * chunks, chunks, lane, clsg);
    pool_sign(A.dims, fam, clab, clsg, lane);
    pool_stage(ssig + (size_t)j * chunks, clsg, chunks, lane);
  }
  for (int j = lane; j < MIQP_POOL_MAX; j += 64) has_sig[j] = j < n0 && last[j].status == 0 ? 1 : 0;
  // the pair's sums over its records, one per lane (at most 32): what the host of a single call sums over its rounds.  A record was live in
  // rounds 1 .. |solves|, so the largest |solves| is the number of rounds - of launch groups - the pair took part in
  {
    const bool mine = lane < n0 + ns;
    const int sv = mine ? solves[lane] : 0;
    int rounds = abs(sv), all = abs(sv), it = mine ? A.acc_it[W.first + lane] : 0, still = mine && lane >= n0 && sv < 0 ? 1 : 0;
    for (int d = 32; d >= 1; d >>= 1) { rounds = max(rounds, __shfl_xor(rounds, d, 64)); all += __shfl_xor(all, d, 64); it += __shfl_xor(it, d, 64); still += __shfl_xor(still, d, 64); }
    if (lane == 0) { int* const st = A.state + (size_t)p * POOL_CARRY_STATE; st[2] = rounds; st[3] = all; st[4] = it; st[5] = still; }
  }
  // lane k holds source entry k: its record of `out` as far as it is known without a visit, and the objective the visiting order goes by
  double key = POOL_ADMIT_NONE;
  if (lane < ns) {
    const bool bad = A.unmappable[pb + lane] != 0;
    const miqp_fixed_result_c r = A.first[W.first + n0 + lane];
    const bool feasible = !bad && r.status == 0 && r.objective < POOL_ADMIT_NONE;
    miqp_pool_carry_c o;
    o.status = bad ? POOL_CARRY_UNMAPPABLE : POOL_CARRY_INFEASIBLE; o.place = -1; o.solves = bad ? 0 : abs(solves[n0 + lane]); o.iterations = bad ? 0 : r.iterations;
    o.objective = bad ? __longlong_as_double(0x7FF8000000000000ll) : r.objective; o.reserved = 0; o.reserved1 = 0;
    out[lane] = o;
    if (feasible) key = r.objective;
  }
  __syncthreads();
  int n = n0, added = 0;
  double obj0 = n0 > 0 ? pool_obj[0] : 0.0;
  for (int visit = 0; visit < ns; ++visit) {
    double bo = key; int bg = key < POOL_ADMIT_NONE ? lane : 0x7FFFFFFF;
    pool_wave_argmin(bo, bg);
    if (bg == 0x7FFFFFFF) break;
    if (lane == bg) key = POOL_ADMIT_NONE;
    int st;
    if (n > 0 && !pool_within_cap(obj0, bo, A.max_rel)) st = POOL_CARRY_BEYOND_CAP;
    else {
      pool_stage(cand, shifted + (size_t)bg * chunks, chunks, lane, csg);
      pool_sign(A.dims, fam, cand, csg, lane);
      if (pool_known(csg, sig, n, chunks, lane)) st = POOL_CARRY_KNOWN;
      else if (solves[n0 + bg] == 0 || last[n0 + bg].status != 0) st = POOL_CARRY_SETTLED_KNOWN;   // (no settled labels)
      else {
        pool_stage(clab, lab + (size_t)(n0 + bg) * chunks, chunks, lane, clsg);
        pool_sign(A.dims, fam, clab, clsg, lane);
        if (pool_known(clsg, ssig, n, chunks, lane, has_sig)) st = POOL_CARRY_SETTLED_KNOWN;
        else if (n >= K) st = POOL_CARRY_NO_PLACE;
        else {
          for (int c = lane; c < chunks; c += 64) { pool[(size_t)n * chunks + c] = cand[c]; sig[(size_t)n * chunks + c] = csg[c]; ssig[(size_t)n * chunks + c] = clsg[c]; }
          if (lane == 0) { pool_obj[n] = bo; has_sig[n] = 1; out[bg].place = n; }
          if (n == 0) obj0 = bo;
          st = POOL_CARRY_ADMITTED; n++; added++;
        }
      }
    }
    if (lane == 0) out[bg].status = st;
    __syncthreads();   // (the appended signatures are compared with the next record's)
  }
  if (lane == 0) { A.state[(size_t)p * POOL_CARRY_STATE] = n; A.state[(size_t)p * POOL_CARRY_STATE + 1] = added; }
}

// buffers of the call beside the settle rounds', cached per device (DevArr: grown, not shrunk), and the events around its two kernels
// Per place and per pair, so they grow with the pairs of a call; `first` with its records (np pairs, nrec records, nr and ne map words in all)
struct PoolCarryDev {
  DevArr<signed char> src, shifted, pool, sig, csig; DevArr<int> rmap, emap, unmappable, has_sig, state; DevArr<double> pool_obj; DevArr<miqp_fixed_result_c> first; DevArr<miqp_pool_carry_c> out;
  DevArr<PoolCarryPair> pair;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  bool ensure(size_t np, size_t nrec, size_t fl, size_t nr, size_t ne) {
    const size_t m = np * MIQP_POOL_MAX, f = MIQP_POOL_MAX;
    for (auto& e : ev) if (!e) HIP_OK(hipEventCreate(&e));
    return src.need(m * fl, f * fl) && shifted.need(m * fl, f * fl) && pool.need(m * fl, f * fl) && sig.need(m * fl, f * fl) && csig.need(m * fl, f * fl) && rmap.need(nr, 256) && emap.need(ne, 64) &&
           unmappable.need(m, f) && has_sig.need(m, f) && state.need(np * POOL_CARRY_STATE, 64) && pool_obj.need(m, f) && first.need(nrec, 2 * f) && out.need(m, f) && pair.need(np, 16);
  }
};

thread_local double g_pool_carry_last[2] = {0.0, 0.0};   // seconds of the calling thread's last carry in pool_shift_kernel and in pool_carry_admit_kernel
thread_local int g_pool_carry_multi_last[2] = {0, 0};    // rounds and launch groups of the calling thread's last miqp_solver_pool_carry_multi (miqp_gpu_pool_carry_multi_last)

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

// what the call found out of one pair before it touches a device
struct PoolCarryPlan { miqp_solver_t* dst = nullptr; const miqp_solver_t* src = nullptr; int ns = 0, n0 = 0, K = 0, p_src = 0; std::vector<int> rmap, emap; };

// The host side of a call's uploads: the pairs' words, their maps in a row, and the records - own (the destinations' entries) and src (the sources'),
// both completed as miqp_solver_solve_decisions completes decision bytes: the bytes behind them are "none"
struct PoolCarryStage {
  int n = 0;   // records of the call
  std::vector<PoolCarryPair> pair; std::vector<int> rmap, emap, live0, inst; std::vector<signed char> src, pool, cur; std::vector<double> obj;
  PoolCarryStage(const std::vector<PoolCarryPlan>& P, const Layout& Y) {
    const size_t fl = (size_t)Y.fixlen, D = (size_t)Y.f_c2n, np = P.size(), m = np * MIQP_POOL_MAX;
    pair.resize(np);
    for (size_t q = 0; q < np; ++q) {
      pair[q] = PoolCarryPair{n, P[q].n0, P[q].ns, P[q].K, P[q].dst->pool_fam, P[q].p_src, (int)P[q].emap.size(), (int)rmap.size(), (int)emap.size()};
      rmap.insert(rmap.end(), P[q].rmap.begin(), P[q].rmap.end()); emap.insert(emap.end(), P[q].emap.begin(), P[q].emap.end());
      n += P[q].n0 + P[q].ns;
    }
    src.assign(m * fl, (signed char)-1); pool.assign(m * fl, (signed char)-1); cur.assign((size_t)n * fl, (signed char)-1); obj.assign(m, 0.0);
    live0.assign(n, 0); inst.resize(n);   // (the destinations' own entries are live in round 1; the shift kernel says which carried ones are)
    for (size_t q = 0; q < np; ++q) {
      const PoolCarryPlan& p = P[q]; const size_t pb = q * MIQP_POOL_MAX, first = (size_t)pair[q].first;
      for (int j = 0; j < p.n0; ++j) {
        std::memcpy(cur.data() + (first + j) * fl, p.dst->pool_fix.data() + (size_t)j * fl, D);
        std::memcpy(pool.data() + (pb + j) * fl, p.dst->pool_fix.data() + (size_t)j * fl, D);
        obj[pb + j] = p.dst->pool_obj[j]; live0[first + j] = 1;
      }
      for (int k = 0; k < p.ns; ++k) std::memcpy(src.data() + (pb + k) * fl, p.src->pool_fix.data() + (size_t)k * fl, D);
      for (int r = 0; r < p.n0 + p.ns; ++r) inst[first + r] = (int)q;
    }
  }
};

// The device part of the carry of the call's pairs: pair q carries into handle q of the open call.  false: HIP error or a refusal (err); nothing of
// any handle has been touched
struct PoolCarryOut {
  std::vector<miqp_pool_carry_c> out; std::vector<signed char> fix; std::vector<double> obj;   // the places at the end, MIQP_POOL_MAX per pair
  std::vector<int> state;   // POOL_CARRY_STATE words per pair
  PoolSettleTally tally; float dev_ms = 0, shift_ms = 0, admit_ms = 0; std::string err;
};
bool pool_carry_run(const FixedCall& call, const std::vector<PoolCarryPlan>& P, const PoolCarryStage& G, int shift, double max_rel, PoolCarryOut& O) {
  DevCtx& X = *call.X; DevBuf& B = X.B; hipStream_t st = X.stream; const Layout& Y = call.Y;
  const size_t fl = (size_t)Y.fixlen; const int np = (int)P.size(), m = np * MIQP_POOL_MAX, n = G.n;
  static const char* const name = "miqp_solver_pool_carry";
  if (np != call.n || np < 1 || n < 1 || n > FB_CAP) return false;
  if (4 * fl > POOL_EXPLORE_LDS_MAX) {
    O.err = std::string(name) + ": the fix record of this shape does not fit the LDS of pool_carry_admit_kernel four times";
    std::fprintf(stderr, "[miqp_gpu] %s (%zu bytes)\n", O.err.c_str(), 4 * fl); return false;
  }
  if (!pool_label_fits(Y, name, O.err)) return false;
  PoolImproveDev& R = call_dev<PoolImproveDev>(X.device); PoolSettleDev& W = call_dev<PoolSettleDev>(X.device); PoolCarryDev& Q = call_dev<PoolCarryDev>(X.device);
  if (!R.ensure((size_t)Y.N * Y.nz) || !W.ensure((size_t)n, fl) || !Q.ensure((size_t)np, (size_t)n, fl, std::max<size_t>(G.rmap.size(), 1), std::max<size_t>(G.emap.size(), 1)) || !pool_label_set_lds(Y)) return false;
  HIP_OK(hipFuncSetAttribute((const void*)pool_shift_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(2 * fl)));
  HIP_OK(hipFuncSetAttribute((const void*)pool_carry_admit_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(4 * fl)));
  const DevBuf Bp = fixed_chain_settings(B);
  const PoolSettleArgs S = pool_settle_args(W, B, Y, n);
  PoolCarryArgs A;
  A.dims = pool_dims(Y); A.fixlen = (int)fl; A.np = np; A.shift = shift; A.pair = Q.pair; A.rmap = Q.rmap; A.emap = Q.emap;
  A.src = Q.src; A.shifted = Q.shifted; A.unmappable = Q.unmappable; A.lab = W.cur; A.moved = W.moved; A.solves = W.solves; A.acc_it = W.acc_it; A.last = W.last; A.first = Q.first;
  A.pool = Q.pool; A.pool_obj = Q.pool_obj; A.sig = Q.sig; A.csig = Q.csig; A.has_sig = Q.has_sig; A.max_rel = max_rel; A.out = Q.out; A.state = Q.state;
  HIP_OK(hipMemsetAsync(B.batch_inst, 0, (size_t)FB_CHUNK * 4, st));
  HIP_OK(hipMemcpyAsync(Q.pair, G.pair.data(), (size_t)np * sizeof(PoolCarryPair), hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(Q.src, G.src.data(), (size_t)m * fl, hipMemcpyHostToDevice, st));
  if (!G.rmap.empty()) HIP_OK(hipMemcpyAsync(Q.rmap, G.rmap.data(), G.rmap.size() * sizeof(int), hipMemcpyHostToDevice, st));
  if (!G.emap.empty()) HIP_OK(hipMemcpyAsync(Q.emap, G.emap.data(), G.emap.size() * sizeof(int), hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(W.cur, G.cur.data(), (size_t)n * fl, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(Q.pool, G.pool.data(), (size_t)m * fl, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(Q.pool_obj, G.obj.data(), (size_t)m * sizeof(double), hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(W.moved, G.live0.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(W.inst, G.inst.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, st));
  HIP_OK(hipMemsetAsync(W.round_it, 0, (size_t)n * sizeof(int), st));
  HIP_OK(hipMemsetAsync(W.solves, 0, (size_t)n * sizeof(int), st)); HIP_OK(hipMemsetAsync(W.acc_it, 0, (size_t)n * sizeof(int), st));
  HIP_OK(hipMemsetAsync(W.last, 0xFF, (size_t)n * sizeof(miqp_fixed_result_c), st)); HIP_OK(hipMemsetAsync(Q.first, 0xFF, (size_t)n * sizeof(miqp_fixed_result_c), st));   // (status -1: never solved)
  HIP_OK(hipEventRecord(X.ev0, st));
  HIP_OK(hipEventRecord(Q.ev[0], st));
  hipLaunchKernelGGL(pool_shift_kernel, dim3(m), dim3(64), 2 * fl, st, A);
  HIP_OK(hipGetLastError());
  HIP_OK(hipEventRecord(Q.ev[1], st));
  int live = 0;
  if (!pool_settle_compact(X, S, live, O.tally)) return false;   // (waits: the stage is the caller's and outlives the call)
  if (!pool_settle_rounds(call, Bp, S, R.Z, 1, live, O.tally, 1)) return false;
  HIP_OK(hipMemcpyAsync(Q.first, W.last, (size_t)n * sizeof(miqp_fixed_result_c), hipMemcpyDeviceToDevice, st));
  if (!pool_settle_rounds(call, Bp, S, R.Z, 2, live, O.tally)) return false;
  HIP_OK(hipEventRecord(Q.ev[2], st));
  hipLaunchKernelGGL(pool_carry_admit_kernel, dim3(np), dim3(64), 4 * fl, st, A);
  HIP_OK(hipGetLastError());
  HIP_OK(hipEventRecord(Q.ev[3], st));
  HIP_OK(hipEventRecord(X.ev1, st));
  O.state.assign((size_t)np * POOL_CARRY_STATE, 0); O.out.resize(m); O.fix.resize((size_t)m * fl); O.obj.resize(m);
  HIP_OK(hipMemcpyAsync(O.state.data(), Q.state, O.state.size() * sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(O.out.data(), Q.out, (size_t)m * sizeof(miqp_pool_carry_c), hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(O.fix.data(), Q.pool, (size_t)m * fl, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(O.obj.data(), Q.pool_obj, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st)); HIP_OK(hipGetLastError());
  (void)hipEventElapsedTime(&O.dev_ms, X.ev0, X.ev1); (void)hipEventElapsedTime(&O.shift_ms, Q.ev[0], Q.ev[1]); (void)hipEventElapsedTime(&O.admit_ms, Q.ev[2], Q.ev[3]);
  for (int q = 0; q < np; ++q) {
    const int* const s = O.state.data() + (size_t)q * POOL_CARRY_STATE;
    if (s[0] != P[q].n0 + s[1] || s[1] < 0 || s[1] > P[q].ns || s[0] > P[q].K || s[2] < 0 || s[2] > POOL_PASSES || s[3] < 0 || s[4] < 0 || s[5] < 0 || s[5] > P[q].ns) {
      std::fprintf(stderr, "[miqp_gpu] %s: pair %d: %d entries behind %d, %d admitted, %d rounds\n", name, q, s[0], P[q].n0, s[1], s[2]); return false;
    }
  }
  return true;
}

// The carry of pairs that all take part (entries to carry, a free place), behind every refusal but -3: one lock, one context over the destinations,
// one upload, the run, and - behind its last read-back - what the handles keep: the admitted entries behind the old ones, which stay as the handle
// holds them, the dropped refined pool, last_timing and the "still moved" text.  outs[q]: the `out` rows of pair q, counts[q]: its admitted
// entries.  Entries admitted in all, or -3 (the destinations then carry the run's refusal, if it gave one)
int pool_carry_call(const std::vector<PoolCarryPlan>& P, const Layout& Y, int shift, double max_rel, double t_call, miqp_pool_carry_c* const* outs, int* counts, int* rounds = nullptr, int* groups = nullptr) {
  static const char* const name = "miqp_solver_pool_carry";
  const int np = (int)P.size(); const size_t fl = (size_t)Y.fixlen;
  const PoolCarryStage G(P, Y);
  const double setup_s = wall_s() - t_call;
  std::vector<miqp_solver_t*> dsts(np);
  for (int q = 0; q < np; ++q) dsts[q] = P[q].dst;
  FixedCall call;
  if (call.open(dsts.data(), np, Y) != 0) return -3;
  PoolCarryOut O;
  if (!pool_carry_run(call, P, G, shift, max_rel, O)) {
    (void)hipStreamSynchronize(call.X->stream);
    if (!O.err.empty()) for (int q = 0; q < np; ++q) dsts[q]->err = O.err;
    return -3;
  }
  const double call_s = wall_s() - t_call;
  int all = 0, most = 0;
  for (int q = 0; q < np; ++q) {
    miqp_solver_t* dst = dsts[q]; const int n0 = P[q].n0; const int* const s = O.state.data() + (size_t)q * POOL_CARRY_STATE;
    const signed char* const pf = O.fix.data() + (size_t)q * MIQP_POOL_MAX * fl; const double* const po = O.obj.data() + (size_t)q * MIQP_POOL_MAX;
    dst->pool_fix.resize((size_t)n0 * fl); dst->pool_obj.resize(n0);
    dst->pool_fix.insert(dst->pool_fix.end(), pf + (size_t)n0 * fl, pf + (size_t)s[0] * fl);
    dst->pool_obj.insert(dst->pool_obj.end(), po + n0, po + s[0]);
    dst->pool_n = s[0]; dst->pool_fixlen = (int)fl;
    if (!dst->has_sol && s[0] > 0) dst->pool_carried = true;   // (a pool without a solve behind it: the carried entries are all it holds)
    dst->pr_n = 0; std::vector<char>().swap(dst->pr_ok); std::vector<signed char>().swap(dst->pr_fix); std::vector<double>().swap(dst->pr_Z);
    for (int k = 0; k < P[q].ns; ++k) outs[q][k] = O.out[(size_t)q * MIQP_POOL_MAX + k];
    counts[q] = s[1];
    if (s[5]) {
      char msg[200]; std::snprintf(msg, sizeof msg, "%s: the labels of %d carried records still moved after %d solves; their settled signature is that of the last labels", name, s[5], POOL_PASSES);
      dst->err = msg;
    }
    dst->setup[0] = setup_s;
    dst->timing[0] = call_s; dst->timing[1] = O.dev_ms * 1e-3; dst->timing[2] = s[2]; dst->timing[3] = (double)s[3]; dst->timing[4] = (double)s[4]; dst->timing[5] = s[5] ? 1 : 0;
    all += s[1]; most = std::max(most, s[2]);
  }
  g_pool_carry_last[0] = O.shift_ms * 1e-3; g_pool_carry_last[1] = O.admit_ms * 1e-3;
  if (rounds) *rounds = most;
  if (groups) *groups = O.tally.groups;
  return all;
}

// what both entries refuse of a pair of handles, -1 or -2, else 0 with the maps
int pool_carry_pair(const miqp_solver_t* src, const miqp_solver_t* dst, std::vector<int>& rmap, int& p_src, std::vector<int>& emap, std::string& err) {
  if (!src || !dst || src == dst || !src->has_inst || !dst->has_inst) return -1;
  return pool_carry_build_maps(src->inst, dst->inst, rmap, p_src, emap, err) ? 0 : -2;
}

// the kept pools of a pair hold records of the Layout's length
bool pool_carry_fits(const PoolCarryPlan& P, const Layout& Y) {
  const size_t fl = (size_t)Y.fixlen;
  if (P.ns > 0 && (P.src->pool_fixlen != Y.fixlen || P.src->pool_fix.size() < (size_t)P.ns * fl)) return false;
  return P.n0 == 0 || (P.dst->pool_fixlen == Y.fixlen && P.dst->pool_fix.size() >= (size_t)P.n0 * fl && P.dst->pool_obj.size() >= (size_t)P.n0);
}

// Starts from the carried pool, behind the solve's read-back: st_place[k] is the entry of the pool the solve left that stands for start k - under the
// handle's filter the entry of the start's plain signature, without one the entry of the same decision bytes -, -1 when the pool holds none
void pool_starts_places(miqp_solver* s, const Layout& Y) {
  const size_t fl = (size_t)Y.fixlen, D = (size_t)Y.f_c2n;
  s->st_place.assign(s->st_n, -1);
  if (s->pool_n <= 0 || s->pool_fixlen != Y.fixlen || s->st_fixlen != Y.fixlen || s->pool_fix.size() < (size_t)s->pool_n * fl || s->st_fix.size() < (size_t)s->st_n * fl) return;
  const int fam = s->pool_fam & POOL_FAM_ALL;
  std::vector<signed char> esig, ssig(fl);
  if (fam) { esig.resize((size_t)s->pool_n * fl); for (int j = 0; j < s->pool_n; ++j) pool_signature(pool_dims(Y), fam, s->pool_fix.data() + (size_t)j * fl, esig.data() + (size_t)j * fl, fl); }
  for (int k = 0; k < s->st_n; ++k) {
    const signed char* const st = s->st_fix.data() + (size_t)k * fl;
    if (fam) pool_signature(pool_dims(Y), fam, st, ssig.data(), fl);
    for (int j = 0; j < s->pool_n && s->st_place[k] < 0; ++j)
      if (fam ? std::memcmp(ssig.data(), esig.data() + (size_t)j * fl, fl) == 0 : std::memcmp(st, s->pool_fix.data() + (size_t)j * fl, D) == 0) s->st_place[k] = j;
  }
}

}  // namespace

extern "C" {

int miqp_solver_set_pool_starts(miqp_solver_t* s, int max_starts) {
  if (!s || max_starts < 0 || max_starts > MIQP_POOL_MAX) return -1;
  s->pool_starts = max_starts;
  return 0;
}

int miqp_solver_get_pool_starts(const miqp_solver_t* s) { return s ? s->pool_starts : -1; }

int miqp_solver_pool_starts_last(const miqp_solver_t* s, int* place, int cap) {
  if (!s) return -1;
  for (int k = 0; place && k < s->st_n && k < cap; ++k) place[k] = k < (int)s->st_place.size() ? s->st_place[k] : -1;
  return s->st_n;
}

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
  if (dst) dst->err.clear();   // (miqp_solver_last_error speaks of this call from here on)
  if (!out || cap < 0 || max_rel != max_rel) return -1;
  std::vector<PoolCarryPlan> one(1);
  PoolCarryPlan& P = one[0]; std::string err;
  if (const int rc = pool_carry_pair(src, dst, P.rmap, P.p_src, P.emap, err)) { if (dst && !err.empty()) dst->err = err; return rc; }
  if (shift < 1 || shift > dst->inst.N - 2) return -2;
  P.dst = dst; P.src = src;
  P.K = std::min(dst->pool_cap, MIQP_POOL_MAX);
  if (P.K <= 0 || dst->pool_fam < 1 || dst->pool_fam >= POOL_FAM_TIMING) return -2;
  P.ns = std::min(miqp_solver_pool_count(src), MIQP_POOL_MAX); P.n0 = miqp_solver_pool_count(dst);
  if (cap < P.ns) return -2;
  miqp_solver_t* h[1] = {dst};
  BatchShape bs = batch_layout(h, 1);
  if (!bs.ok) { dst->err = bs.err; return -2; }
  if (!pool_carry_fits(P, bs.Y)) return -1;
  if (P.ns == 0 || P.n0 >= P.K) return 0;   // (nothing to carry, or no free place: no device is touched)
  { int ndev = 0; if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return -3; }
  const double t_call = wall_s();
  int added = 0;
  return pool_carry_call(one, bs.Y, shift, max_rel, t_call, &out, &added);
}

int miqp_solver_pool_carry_multi(miqp_solver_t* const* dsts, const miqp_solver_t* const* srcs, int n, int shift, double max_rel, miqp_pool_carry_c* out, int cap, int* counts) {
  static const char* const name = "miqp_solver_pool_carry_multi";
  if (!dsts || !srcs || !out || !counts || n <= 0 || cap < 0 || max_rel != max_rel) return -1;
  if (n > FB_CAP / (2 * MIQP_POOL_MAX)) return -5;   // (on the count alone: the arrays are not read)
  for (int p = 0; p < n; ++p) if (!dsts[p] || !srcs[p] || srcs[p] == dsts[p] || !dsts[p]->has_inst || !srcs[p]->has_inst) return -1;
  {  // a destination named twice, or one that is the source of another pair: the answer would depend on the order of the pairs
    std::vector<const miqp_solver_t*> d(dsts, dsts + n), s(srcs, srcs + n);
    std::sort(d.begin(), d.end()); std::sort(s.begin(), s.end());
    if (std::adjacent_find(d.begin(), d.end()) != d.end()) return -1;
    for (const miqp_solver_t* h : d) if (std::binary_search(s.begin(), s.end(), h)) return -1;
  }
  // what the single call refuses of a pair with -2, pair by pair: the first refusal decides, and its reason is that destination's last error
  std::vector<PoolCarryPlan> all(n);
  for (int p = 0; p < n; ++p) {
    PoolCarryPlan& P = all[p]; miqp_solver_t* dst = dsts[p]; std::string err;
    P.dst = dst; P.src = srcs[p];
    if (shift < 1 || shift > dst->inst.N - 2) return -2;
    if (!pool_carry_build_maps(srcs[p]->inst, dst->inst, P.rmap, P.p_src, P.emap, err)) { dst->err = err; return -2; }
    P.K = std::min(dst->pool_cap, MIQP_POOL_MAX);
    if (P.K <= 0 || dst->pool_fam < 1 || dst->pool_fam >= POOL_FAM_TIMING) {
      char msg[200]; std::snprintf(msg, sizeof msg, "%s: the destination of pair %d has capacity %d and filter %d; the carry needs a capacity and a filter in 1 .. 15", name, p, dst->pool_cap, dst->pool_fam);
      dst->err = msg; return -2;
    }
    P.ns = std::min(miqp_solver_pool_count(srcs[p]), MIQP_POOL_MAX); P.n0 = miqp_solver_pool_count(dst);
  }
  BatchShape bs;
  if (const int rc = fixed_multi_check(dsts, n, bs)) return rc;
  int most = 0;
  for (int p = 0; p < n; ++p) { if (!pool_carry_fits(all[p], bs.Y)) return -1; most = std::max(most, all[p].ns); }
  if (cap < most) return -2;
  for (int p = 0; p < n; ++p) dsts[p]->err.clear();   // (miqp_solver_last_error of every destination speaks of this call from here on)
  // a pair takes part when it has entries to carry and its destination a free place
  std::vector<int> part;
  for (int p = 0; p < n; ++p) if (all[p].ns > 0 && all[p].n0 < all[p].K) part.push_back(p);
  if (part.empty()) { for (int p = 0; p < n; ++p) counts[p] = 0; return 0; }   // (nothing to run: no device is touched)
  { int ndev = 0; if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return -3; }
  const double t_call = wall_s();
  const int np = (int)part.size();
  std::vector<PoolCarryPlan> P(np); std::vector<miqp_pool_carry_c*> outs(np); std::vector<int> added(np, 0);
  for (int q = 0; q < np; ++q) { P[q] = std::move(all[part[q]]); outs[q] = out + (size_t)part[q] * cap; }
  int rounds = 0, groups = 0;
  const int rc = pool_carry_call(P, bs.Y, shift, max_rel, t_call, outs.data(), added.data(), &rounds, &groups);
  if (rc < 0) return rc;
  for (int p = 0; p < n; ++p) counts[p] = 0;
  for (int q = 0; q < np; ++q) counts[part[q]] = added[q];
  g_pool_carry_multi_last[0] = rounds; g_pool_carry_multi_last[1] = groups;
  return rc;
}

void miqp_gpu_pool_carry_multi_last(int* rounds, int* groups) {
  if (rounds) *rounds = g_pool_carry_multi_last[0];
  if (groups) *groups = g_pool_carry_multi_last[1];
}

void miqp_gpu_pool_carry_last(double* shift_s, double* admit_s) {
  if (shift_s) *shift_s = g_pool_carry_last[0];
  if (admit_s) *admit_s = g_pool_carry_last[1];
}

}  // extern "C"

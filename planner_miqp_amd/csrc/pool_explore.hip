// pool_explore.hip - the free places of a filtered solution pool filled with NEIGHBOURING manoeuvre classes (miqp_solver_pool_explore).  DESIGN.md 6h.
//
// Counterpart of IloCplex::populate for a CPLEX user.  The pool holds leaves the branch and bound evaluated, and the search prunes everything beyond
// its gap: a manoeuvre that is clearly worse than the optimum but valid - the car passes the obstacle on the other side - usually never becomes a
// leaf, and a caller who asked for 16 fallbacks gets one.  The climb (pool_improve.hip) moves inside a class; this file steps ACROSS classes:
//
//   a JUMP is a move (first, stride, count, value) of the families MIQP_POOL_BY_OBSTACLE and MIQP_POOL_BY_CAR_CAR that are in the filter.
//   A UNIT is a group - the five point-sites of one (car, obstacle), or the four group-sites of one car pair: their bytes of one step are contiguous
//   in the record - or one site.  A RUN of a unit is a maximal range [i0, i1] inside 1 .. N - 1 over which every byte of the unit is decided (>= 0)
//   and the unit's bytes stay what they are.  For every run and every alternative v (an obstacle edge 0 .. L - 1 - never the soft alternative L, which
//   a run may hold and be jumped from - or a car/car alternative 0 .. 3) all bytes of the unit over the run take v: of a group one contiguous range
//   of stride 1 (all points of a car have to change edge together to pass on the other side), of a site its bytes at the site's stride.  A
//   candidate whose bytes all hold v already is skipped, and so is one behind which the signature is the same - which happens exactly when, for
//   every site it writes, the decided bytes around the run are (p, q) = (a, v) or (v, a), a the site's byte in the run: the run then only moves a
//   change point, which is a move of the climb, not a jump.  Step 0 and undecided bytes are never written.  Order: obstacle groups by c * O + o,
//   pairs, then the sites in pool_site order; inside a unit the runs by i0, then v ascending; at most POOL_MOVES_MAX per record, the first ones.
//
// pool_unit_jumps below is that definition, once, for the host (miqp_gpu_pool_jumps) and the device (pool_jumps_kernel).
//
// The call, per pass, all on the solver stream (pass 1 expands every kept entry, pass p > 1 the entries pass p - 1 added):
//   pool_jumps_kernel      one wavefront per place of the pool: the record staged in LDS, its jumps counted, numbered and written to the move
//                          table (pool_count_scan_emit of pool_blocks.hip, one lane per unit)
//   pool_offsets_kernel, pool_neighbour_kernel, fixed_chunk
//                          the climb's, unchanged, chunk by chunk: the 16 places of a handle have at most 16 x 512 jumps, the 8192 results the
//                          climb holds, so one handle never needs slices (many do: below)
//   pool_admit_kernel      ONE wavefront per handle: the objectives of the pass's feasible neighbours within the cost cap staged in LDS; then, as long as a
//                          place is free, the smallest (objective, neighbour number) by wave reduction, its patched record and that record's signature
//                          under the handle's filter built in LDS, compared with the signatures of everything in the pool - the entries admitted
//                          earlier in this pass included; a new signature is appended behind the pool: decision bytes, objective, signature and
//                          the `out` record.  The visiting order makes the first neighbour of a new class that class's best of the pass.  No
//                          existing entry is changed or moved.
// Owner computes: no atomics, no lock, no wavefront waits on another, no scratch; records move as 16-byte loads and stores.  The host waits once per
// pass and reads the number admitted, their `out` records and the jump counts of the next pass.
//
// DISTINCT admission (miqp_solver_pool_explore_distinct; opt-in, the call above is unchanged): most neighbours of a new signature are
// an entry's own solution under other labels.  The distinct call solves the kept entries' own records first (pass 0), has pool_label_kernel
// (pool_label.hip) write the canonical record of every solved node behind its chunk, keeps per place the signature of that record beside the plain
// one (pool_pass0_kernel) and admits a neighbour only when BOTH signatures are new (pool_admit_distinct_kernel: the same body, one more test).
//
// SETTLED admission (miqp_solver_pool_explore_settled; opt-in, both calls above are unchanged): first labels are an intermediate of
// the iteration the refinement runs, and it merges by the final ones.  The settled call carries every candidate of a pass to ITS fixed point
// (pool_settle.hip) and admits by the signature of the settled labels, so that miqp_solver_pool_solve behind it merges away nothing it added:
//   pass 0                     the kept entries' own records through the settle rounds; pool_pass0_kernel writes, per kept entry, the plain
//                              signature and the signature of its settled labels (none when its own QP is not feasible: it never matches)
//   pool_settle_pick_kernel    behind a pass's chain and labels, one wavefront per neighbour: a CANDIDATE is feasible, within the cost cap, and its
//                              plain signature - of the parent's bytes behind the jump, rebuilt in LDS as the admission does - is new against
//                              the pool at the START of the pass.  The pool only grows within a pass, so every neighbour the serial admission can
//                              admit is a candidate.  A candidate whose first labels are its record is settled with one solve; the others enter
//                              the settle rounds (round 2 on) under their first labels
//   pool_admit_settled_kernel  the admission body with the settled test in place of the canonical one: a candidate is admitted when its plain
//                              signature is new and the signature of its settled labels is new among the settled signatures of the pool, the
//                              entries admitted earlier in the pass included; `reserved` of its record carries the solves its settling took
//
// MANY HANDLES (miqp_solver_pool_explore_multi).  pool_explore_run explores the pools of n handles of one shape; the three calls above
// are that run with one handle, on the same kernels.  All handles start pass 1 together, one pass of the call is one pass of every handle that
// still adds, and their neighbours fill common launch groups.  Places are numbered handle-major with a stride of MIQP_POOL_MAX; per place the
// handle's index (ent_inst, which pool_neighbour_kernel hands to the node kernels) and its filter (ent_fam), per handle its capacity, its edge
// count, the objective of its entry 0 and its four state words.  A handle's admission is its own workgroup of one wavefront and sees its own
// neighbours only, numbered from its first, in the single call's order - so a handle's answer is the single call's, bit for bit.  A handle that is
// full or admitted nothing gets no jumps from then on: the admission marks no place of it for expansion.  The settle rounds sum solves and iterations
// per record (PoolSettleArgs::acc_it), and the handle's admission sums over its own neighbours.
// SLICES: the result, label and settle buffers hold 8192 neighbours; a slice is a run of WHOLE handles whose neighbours of the pass fit them,
// formed greedily in handle order (miqp_gpu_pool_explore_plan; the host loop calls that very function).  Per slice the chain and labels in chunks of
// FB_CHUNK with results relative to the slice, the settled mode's pick, compaction and rounds, then the admission of the slice's handles; behind the
// last slice the jumps and offsets of the next pass.  The host waits once per pass (the settled mode: also once per round of a slice).  Pass 0
// numbers the kept entries of all handles handle-major; off[] carries that numbering and the move table an empty move per place
#pragma once

namespace {

constexpr int POOL_EXPLORE_PASSES_MAX = 64;
constexpr size_t POOL_EXPLORE_LDS_MAX = 160 * 1024;   // dynamic LDS of either kernel: the LDS of a gfx950 workgroup; a larger shape is refused with a message

struct PoolJumpDims { PoolDims d; int L; };   // PoolDims and the edge count of an obstacle (max_lines_obstacles)

__host__ __device__ inline int pool_jump_groups(const PoolDims& d) { return d.C * d.O + d.NP; }
__host__ __device__ inline int pool_jump_units(const PoolDims& d) { return pool_jump_groups(d) + pool_sites(d); }

// unit u of a record: byte k (k < width) of step i lies at base + i * row + k; alts alternatives 0 .. alts - 1; alts == 0: the unit has no jumps
struct PoolUnit { int base, row, width, alts; };
__host__ __device__ inline PoolUnit pool_jump_unit(const PoolJumpDims& J, int fam, int u) {
  const PoolDims& d = J.d;
  const int f_obs = d.C * d.N * 6, f_c2c = f_obs + d.C * d.O * d.N * 5;
  const int obs = (fam & POOL_FAM_OBSTACLE) ? J.L : 0, c2c = (fam & POOL_FAM_CAR_CAR) ? 4 : 0;
  if (u < d.C * d.O) return PoolUnit{f_obs + u * d.N * 5, 5, 5, obs};
  u -= d.C * d.O;
  if (u < d.NP) return PoolUnit{f_c2c + u * d.N * 4, 4, 4, c2c};
  u -= d.NP;
  const PoolSite t = pool_site(d, u);
  return PoolUnit{t.first, t.step, 1, t.family == POOL_FAM_OBSTACLE ? obs : t.family == POOL_FAM_CAR_CAR ? c2c : 0};
}

// the jumps of unit u in their order; emit(j, move) receives jump j of the unit, the number of jumps is returned
template <class Emit>
__host__ __device__ inline int pool_unit_jumps(const PoolJumpDims& J, int fam, int u, const signed char* rec, Emit emit) {
  const PoolUnit t = pool_jump_unit(J, fam, u);
  const int N = J.d.N;
  if (t.alts <= 0) return 0;
  int n = 0;
  for (int i0 = 1; i0 < N;) {
    const signed char* const r0 = rec + t.base + i0 * t.row;
    bool decided = true;
    for (int k = 0; k < t.width; ++k) decided = decided && r0[k] >= 0;
    if (!decided) { i0++; continue; }
    int i1 = i0;
    for (; i1 + 1 < N; ++i1) {
      bool same = true;
      for (int k = 0; k < t.width; ++k) same = same && r0[k] == r0[(i1 + 1 - i0) * t.row + k];
      if (!same) break;
    }
    for (int v = 0; v < t.alts; ++v) {
      bool changes = false;   // the signature of some site the jump writes
      for (int k = 0; k < t.width && !changes; ++k) {
        const int a = r0[k];
        if (a == v) continue;
        int p = -1, q = -1;   // the decided bytes of the site around the run
        for (int i = i0 - 1; i >= 1 && p < 0; --i) p = rec[t.base + i * t.row + k];
        for (int i = i1 + 1; i < N && q < 0; ++i) q = rec[t.base + i * t.row + k];
        changes = !((p == a && q == v) || (p == v && q == a));
      }
      if (!changes) continue;
      emit(n, PoolMove{t.base + i0 * t.row, t.width == 1 ? t.row : 1, t.width * (i1 - i0 + 1), v});
      n++;
    }
    i0 = i1 + 1;
  }
  return n;
}

// MANY HANDLES (miqp_solver_pool_explore_multi).  The places of a call are numbered handle-major with a fixed stride: place
// h * MIQP_POOL_MAX + j is place j of handle h, whatever the handle's capacity (the places from its capacity on are never expanded and never
// filled).  A neighbour number is the call's (off[] is one scan over all places); everything a handle's admission indexes - its staged objectives,
// the place a neighbour belongs to - is relative to the handle, and what a SLICE holds (results, labels, the words of the settle rounds) is relative
// to the slice's first neighbour, off[h0 * MIQP_POOL_MAX].  With one handle all three numberings are the same.
struct PoolExploreArgs {
  PoolImproveArgs A;              // the climb's: cur = the places of the pools, act = expand it in this pass, cnt, moves, off, res, ent_inst, ent_fam; A.m = places
  int nh;                         // handles of the call: A.m = nh * MIQP_POOL_MAX
  const int* hK; const int* hL;   // [nh] a handle's capacity and the edge count of its obstacles
  const double* hobj0;            // [nh] the objective of a handle's entry 0: what the cost cap is relative to
  signed char* sig;               // [places] the signatures of the pools' entries under their handle's filter
  int* state;                     // [nh][4]: [0] entries in the pool, [1] admitted by the last pass, [2] iterations of the last pass's solves, [3] the solves of its settle rounds
  miqp_pool_explore_c* out;       // [places] the records of the last pass's admitted entries, from the handle's first place on
  double max_rel; int pass;
  // the distinct call only (miqp_solver_pool_explore_distinct, below): the signatures of the entries' CANONICAL records under the handle's filter, and
  // the labelled record of every neighbour of the pass (pool_label_kernel, chunk by chunk)
  signed char* csig;              // [places]
  const signed char* lab;         // [NB_MAX]
  // the settled call only (miqp_solver_pool_explore_settled): csig holds the signatures of the SETTLED labels, lab the settled labels of every
  // neighbour of the pass (PoolSettleArgs::cur); a place has a settled signature when has_sig says so; fin and solves: the last answer of every
  // neighbour's settling and the number of its solves (0: no candidate)
  int* has_sig;                   // [places]
  const miqp_fixed_result_c* fin; const int* solves;   // [NB_MAX]
  const int* settle_it;           // [NB_MAX] the iterations of a neighbour's settle rounds (PoolSettleArgs::acc_it)
};

// what a wavefront knows of the handle it works for: its first place, its first neighbour relative to the slice, and its tables' words
struct PoolHandleView { int pb, K, n0, first, rel; };   // first: the call's number of its first neighbour (off[pb]); rel: first - the slice's first
__device__ inline PoolHandleView pool_handle_view(const PoolExploreArgs& E, int h, int h0) {
  const int pb = h * MIQP_POOL_MAX, K = min(max(E.hK[h], 0), MIQP_POOL_MAX), first = E.A.off[pb];
  return PoolHandleView{pb, K, min(max(E.state[4 * h], 0), K), first, first - E.A.off[h0 * MIQP_POOL_MAX]};
}

__global__ __launch_bounds__(64) void pool_jumps_kernel(const PoolExploreArgs E) {
  extern __shared__ uint4 pj_lds[];   // the record; behind it one int per unit
  const PoolImproveArgs& A = E.A;
  const int e = blockIdx.x, lane = threadIdx.x, chunks = A.fixlen >> 4;
  if (e >= A.m) return;
  if (!A.act[e]) { if (lane == 0) A.cnt[e] = 0; return; }
  const PoolJumpDims J{A.dims, E.hL[e / MIQP_POOL_MAX]};
  const signed char* const rec = (const signed char*)pj_lds;
  pool_stage(pj_lds, (const uint4*)(A.cur + (size_t)e * A.fixlen), chunks, lane);
  __syncthreads();
  const int fam = A.ent_fam[e];
  const int total = pool_count_scan_emit(pool_jump_units(A.dims), (int*)(pj_lds + chunks), A.moves + (size_t)e * POOL_MOVES_MAX, lane,
                                         [&](int u, auto emit) { return pool_unit_jumps(J, fam, u, rec, emit); });
  if (lane == 0) A.cnt[e] = total;
}

// The neighbour of place e behind the move mv, the whole wavefront: the parent's record with the move patched in into rec, its signature under the
// handle's filter into sg (both in LDS).  e: the call's number of the place, pb: of its handle's first.  True: the signature is one of the first n
// of the handle's pool
__device__ inline bool pool_candidate_known(const PoolExploreArgs& E, int pb, int e, const int4 mv, uint4* rec, uint4* sg, int n, int lane) {
  const PoolImproveArgs& A = E.A; const int chunks = A.fixlen >> 4;
  pool_stage(rec, (const uint4*)A.cur + (size_t)e * chunks, chunks, lane, sg, mv);
  pool_sign(A.dims, A.ent_fam[pb], rec, sg, lane);
  return pool_known(sg, (const uint4*)E.sig + (size_t)pb * chunks, n, chunks, lane);
}

// Pass 0, the whole wavefront: record j < n of the array src(j) names (the handle's places, or its labels of the pass: both from the handle's first
// on) signed under the handle's filter into place j of dst, the handle's first place.  rec, sg: a record and a signature in LDS
template <class Src>
__device__ inline void pool_sign_places(const PoolExploreArgs& E, int pb, uint4* rec, uint4* sg, int n, Src src, uint4* dst, int lane) {
  const PoolImproveArgs& A = E.A; const int chunks = A.fixlen >> 4, fam = A.ent_fam[pb];
  for (int j = 0; j < n; ++j) {
    pool_stage(rec, src(j) + (size_t)j * chunks, chunks, lane, sg);
    pool_sign(A.dims, fam, rec, sg, lane);
    pool_stage(dst + (size_t)j * chunks, sg, chunks, lane);
  }
}

// The admission of a pass.  DISTINCT (miqp_solver_pool_explore_distinct): a candidate of a new signature is admitted only when the signature of its
// CANONICAL record - the labels of its own solution, E.lab - is new as well, among the canonical signatures of everything in the pool (E.csig: the
// kept entries' from pass 0, the admitted ones' appended here); a candidate dropped for that takes no place.  Without DISTINCT none of that is compiled.
// SETTLED (miqp_solver_pool_explore_settled; MODE 2, which includes the code of DISTINCT): E.lab are the settled labels, E.csig the signatures of
// those, and a neighbour without settled labels - no candidate of the pick kernel, or not feasible at its last solve - is passed over
constexpr int POOL_ADMIT_PLAIN = MIQP_POOL_EXPLORE_PLAIN, POOL_ADMIT_DISTINCT = MIQP_POOL_EXPLORE_DISTINCT, POOL_ADMIT_SETTLED = MIQP_POOL_EXPLORE_SETTLED;
static_assert(POOL_ADMIT_PLAIN == 0 && POOL_ADMIT_DISTINCT == 1 && POOL_ADMIT_SETTLED == 2, "the modes index the table of admission kernels");
template <int MODE>
__device__ inline void pool_admit_body(const PoolExploreArgs& E, int h0, int nb_max, uint4* pa_lds) {
  const PoolImproveArgs& A = E.A;
  constexpr bool DISTINCT = MODE != POOL_ADMIT_PLAIN, SETTLED = MODE == POOL_ADMIT_SETTLED;
  const int lane = threadIdx.x, chunks = A.fixlen >> 4, h = h0 + blockIdx.x;
  if (h >= E.nh) return;   // (uniform)
  const PoolHandleView V = pool_handle_view(E, h, h0);
  const int K = V.K, n0 = V.n0;
  uint4* const cand = pa_lds; uint4* const csig = cand + chunks;
  uint4* const ccan = csig + chunks; uint4* const ccsg = ccan + chunks;   // DISTINCT: the candidate's labelled record and its signature
  double* const key = (double*)(csig + (DISTINCT ? 3 : 1) * chunks);
  // everything from here on is the handle's: its places, its run of off, its neighbours numbered from its first; the pass's results, labels and
  // settle words of neighbour g lie at rel + g of the slice's.  (The host forms the slices of whole handles that fit: a handle that does not lie
  // inside the slice's results has no neighbours here)
  const int* const off = A.off + V.pb;
  int total = min(max(off[MIQP_POOL_MAX] - V.first, 0), MIQP_POOL_MAX * POOL_MOVES_MAX);
  if (V.rel < 0 || V.rel + total > nb_max) total = 0;
  const miqp_fixed_result_c* const res = A.res + V.rel;
  const double obj0 = E.hobj0[h];
  int* const state = E.state + 4 * h;
  uint4* const pool = (uint4*)A.cur + (size_t)V.pb * chunks; uint4* const sig = (uint4*)E.sig + (size_t)V.pb * chunks;
  // the signatures of the entries that have none yet: all of them in pass 1, later the ones the pass before appended (their signature is written
  // with them) - so only pass 1 builds any
  if (E.pass == 1) pool_sign_places(E, V.pb, cand, csig, n0, [&](int) { return (const uint4*)pool; }, sig, lane);
  // the objectives of the pass's candidates, place by place (off ascends from the handle's first: every neighbour below `total` is visited once)
  int it = 0, settle_solves = 0;
  for (int e = 0; e < K; ++e)
    for (int g0 = off[e] - V.first, g1 = min(off[e + 1] - V.first, total), g = g0 + lane; g < g1; g += 64) {
      const miqp_fixed_result_c r = res[g];
      it += r.iterations;
      if (SETTLED) { const int sv = E.solves[V.rel + g]; if (sv != 0) { settle_solves += abs(sv) - 1; it += E.settle_it[V.rel + g]; } }   // (a candidate's first solve is the chain's)
      key[g] = pool_is_candidate(r, obj0, E.max_rel, g - g0, e, n0) ? r.objective : POOL_ADMIT_NONE;
    }
  for (int d = 32; d >= 1; d >>= 1) { it += __shfl_xor(it, d, 64); if (SETTLED) settle_solves += __shfl_xor(settle_solves, d, 64); }
  __syncthreads();
  int n = n0, added = 0;
  while (n < K) {
    double bo = POOL_ADMIT_NONE; int bg = 0x7FFFFFFF;
    for (int g = lane; g < total; g += 64) {   // (a lane's neighbours ascend: a tie keeps the lower number)
      const double o = key[g];
      if (o < bo) { bo = o; bg = g; }
    }
    pool_wave_argmin(bo, bg);
    if (bg == 0x7FFFFFFF) break;
    __syncthreads();
    if (lane == 0) key[bg] = POOL_ADMIT_NONE;
    const int e = pool_entry_of(off, MIQP_POOL_MAX, V.first + bg);   // (the handle's places only.  A staged objective: a candidate, so its move is one of the table and e < n0)
    const int4 mv = A.moves[(size_t)(V.pb + e) * POOL_MOVES_MAX + bg - (off[e] - V.first)];
    if (pool_candidate_known(E, V.pb, V.pb + e, mv, cand, csig, n, lane)) continue;
    int solves = 0;
    if (SETTLED) {
      solves = E.solves[V.rel + bg];
      if (solves == 0 || E.fin[V.rel + bg].status != 0) continue;   // (uniform: no settled labels)
    }
    if (DISTINCT) {
      uint4* const can = (uint4*)E.csig + (size_t)V.pb * chunks;
      pool_stage(ccan, (const uint4*)E.lab + (size_t)(V.rel + bg) * chunks, chunks, lane, ccsg);
      pool_sign(A.dims, A.ent_fam[V.pb], ccan, ccsg, lane);
      if (pool_known(ccsg, can, n, chunks, lane, SETTLED ? E.has_sig + V.pb : nullptr)) continue;   // (an alias of an entry: the same solution under labels of another signature)
      pool_stage(can + (size_t)n * chunks, ccsg, chunks, lane);
      if (SETTLED && lane == 0) E.has_sig[V.pb + n] = 1;
    }
    for (int c = lane; c < chunks; c += 64) { pool[(size_t)n * chunks + c] = cand[c]; sig[(size_t)n * chunks + c] = csig[c]; }   // (one loop for both: two cost the plain kernel four registers)
    if (lane == 0) {
      A.cur_obj[V.pb + n] = bo;
      miqp_pool_explore_c o;
      o.parent = e; o.pass = E.pass; o.first = mv.x; o.stride = mv.y; o.count = mv.z; o.value = mv.w; o.iterations = res[bg].iterations; o.reserved = SETTLED ? abs(solves) : 0; o.objective = bo;
      E.out[V.pb + added] = o;
    }
    n++; added++;
    __syncthreads();   // (the appended signature is compared with the next candidate's)
  }
  // the next pass expands what this one added - nothing when the pool is full now: a one-handle loop stops there on the host, a handle among many
  // is told here, and a handle that admitted nothing has no place marked either.  From then on it has no jumps (pool_jumps_kernel)
  for (int j = lane; j < MIQP_POOL_MAX; j += 64) A.act[V.pb + j] = j >= n0 && j < n && n < K ? 1 : 0;
  if (lane == 0) { state[0] = n; state[1] = added; state[2] = it; state[3] = settle_solves; }
}

// One workgroup of one wavefront per handle of the slice that begins with handle h0: blockIdx.x + h0 is the handle
__global__ __launch_bounds__(64) void pool_admit_kernel(const PoolExploreArgs E, int h0, int nb_max) {
  extern __shared__ uint4 pa_lds[];   // the candidate's record, its signature; behind them one objective per neighbour of the handle
  pool_admit_body<POOL_ADMIT_PLAIN>(E, h0, nb_max, pa_lds);
}

__global__ __launch_bounds__(64) void pool_admit_distinct_kernel(const PoolExploreArgs E, int h0, int nb_max) {
  extern __shared__ uint4 pa_lds[];   // the candidate's record, its signature, its labelled record, that one's signature; behind them the objectives
  pool_admit_body<POOL_ADMIT_DISTINCT>(E, h0, nb_max, pa_lds);
}

__global__ __launch_bounds__(64) void pool_admit_settled_kernel(const PoolExploreArgs E, int h0, int nb_max) {
  extern __shared__ uint4 pa_lds[];   // the candidate's record, its signature, its settled labels, their signature; behind them the objectives
  pool_admit_body<POOL_ADMIT_SETTLED>(E, h0, nb_max, pa_lds);
}

// Behind the chain and the labels of a pass of the settled call, one wavefront per neighbour: is it a candidate (see the head of the file), and did
// its labels move.  Writes the neighbour's words of the settle rounds (PoolSettleArgs, by neighbour number): its first labels as the record of
// round 2, its first answer, 1 solve (0: no candidate), the moved flag.  first_lab: the labelled records of the pass's neighbours
// The neighbours are those of the slice of handles h0 .. h1 - 1, numbered from the slice's first; a neighbour's handle comes from its place
__global__ __launch_bounds__(64) void pool_settle_pick_kernel(const PoolExploreArgs E, const PoolSettleArgs S, const signed char* first_lab, int h0, int h1, int nb_max) {
  extern __shared__ uint4 pk_lds[];   // the neighbour's record, its signature
  const PoolImproveArgs& A = E.A;
  const int g = blockIdx.x, lane = threadIdx.x, chunks = A.fixlen >> 4;
  if (h0 < 0 || h1 > E.nh || h0 >= h1) return;
  const int* const off = A.off + h0 * MIQP_POOL_MAX; const int places = (h1 - h0) * MIQP_POOL_MAX;
  const int total = min(max(off[places] - off[0], 0), nb_max);
  if (g >= total || g >= S.n) return;
  uint4* const rec = pk_lds; uint4* const sg = rec + chunks;
  const int e = h0 * MIQP_POOL_MAX + pool_entry_of(off, places, off[0] + g), jm = off[0] + g - A.off[e];   // (e: the call's number of the place)
  const int h = e / MIQP_POOL_MAX, pb = h * MIQP_POOL_MAX, n0 = min(max(E.state[4 * h], 0), min(max(E.hK[h], 0), MIQP_POOL_MAX));
  // (cand and moved are uniform over the wavefront.)  The pool only grows within a pass: new against its first n0 signatures is what the admission can ask at most
  bool cand = pool_is_candidate(A.res[g], E.hobj0[h], E.max_rel, jm, e - pb, n0);
  if (cand) cand = !pool_candidate_known(E, pb, e, A.moves[(size_t)e * POOL_MOVES_MAX + jm], rec, sg, n0, lane);
  bool moved = false;
  if (cand) {
    const uint4* const lab = (const uint4*)first_lab + (size_t)g * chunks;
    moved = pool_records_differ(lab, rec, chunks, lane);
    pool_stage((uint4*)S.cur + (size_t)g * chunks, lab, chunks, lane);
  }
  if (lane == 0) { pool_settle_copy_result(S.last + g, A.res + g); S.solves[g] = cand ? 1 : 0; S.moved[g] = moved ? 1 : 0; S.round_it[g] = 0; S.acc_it[g] = 0; S.inst[g] = A.ent_inst[e]; }
}

// Pass 0 of the distinct and the settled call, ONE wavefront, behind the kept entries' own solves.  Distinct (behind the chain and pool_label_kernel):
// per kept entry the signature of its canonical record - of its as-found bytes when its own QP is not feasible at the tight tolerance - and the
// iterations of the pass.  Settled (behind the settle rounds): per kept entry its plain signature (the pick kernel of pass 1 compares with it) and
// the signature of its settled labels, with the word that says whether it has one
// One wavefront per handle of the slice that begins with handle h0 (blockIdx.x + h0 is the handle): pass 0 numbers the kept entries of the call
// handle-major, off[] holds that numbering, and the results and labels are the slice's
__global__ __launch_bounds__(64) void pool_pass0_kernel(const PoolExploreArgs E, int h0, int nb_max, int settled) {
  extern __shared__ uint4 p0_lds[];   // a record, its signature
  const PoolImproveArgs& A = E.A;
  const int lane = threadIdx.x, chunks = A.fixlen >> 4, h = h0 + blockIdx.x;
  if (h >= E.nh) return;   // (uniform)
  uint4* const rec = p0_lds; uint4* const sg = rec + chunks;
  const PoolHandleView V = pool_handle_view(E, h, h0);
  const int n0 = V.rel < 0 || V.rel + V.n0 > nb_max ? 0 : V.n0;   // (the host forms the slices so that this does not happen)
  const uint4* const cur = (const uint4*)A.cur + (size_t)V.pb * chunks; const uint4* const lab = (const uint4*)E.lab + (size_t)V.rel * chunks;
  uint4* const csig = (uint4*)E.csig + (size_t)V.pb * chunks;
  int* const state = E.state + 4 * h;
  if (settled) {
    int it = 0, solves = 0;   // (the solves of the handle's own records and their iterations: the compaction sums a round over the whole call)
    for (int j = 0; j < n0; ++j) { it += E.settle_it[V.rel + j]; solves += abs(E.solves[V.rel + j]); }
    pool_sign_places(E, V.pb, rec, sg, n0, [&](int) { return cur; }, (uint4*)E.sig + (size_t)V.pb * chunks, lane);
    pool_sign_places(E, V.pb, rec, sg, n0, [&](int) { return lab; }, csig, lane);
    for (int j = lane; j < MIQP_POOL_MAX; j += 64) E.has_sig[V.pb + j] = j < n0 && E.fin[V.rel + j].status == 0 ? 1 : 0;
    if (lane == 0) { state[2] = it; state[3] = solves; }
  } else {
    const miqp_fixed_result_c* const res = A.res + V.rel;
    int it = 0;
    for (int j = 0; j < n0; ++j) it += res[j].iterations;
    pool_sign_places(E, V.pb, rec, sg, n0, [&](int j) { return res[j].status == 0 ? lab : cur; }, csig, lane);
    if (lane == 0) state[2] = it;
  }
}

// buffers of the call beside the climb's (PoolImproveDev, PoolEntryDev), cached per device (DevArr: grown, not shrunk).  Per place and per handle,
// so they grow with the handles of a call and not with the neighbours of a pass.  has_sig is the settled call's (a place has a settled signature);
// csig and lab the distinct and the settled call's: the second signatures of the places and the labelled records of a slice's neighbours
struct PoolExploreDev {
  DevArr<signed char> sig, csig, lab; DevArr<int> state, has_sig, hK, hL; DevArr<double> hobj0; DevArr<miqp_pool_explore_c> out;
  bool ensure(size_t nh, size_t fl) {
    const size_t m = nh * MIQP_POOL_MAX;
    return state.need(4 * nh, 256) && hK.need(nh, 64) && hL.need(nh, 64) && hobj0.need(nh, 64) && has_sig.need(m, 64) && out.need(m, 64) && sig.need(m * fl, 64 * fl);
  }
  bool ensure_distinct(size_t nh, size_t fl) { return csig.need(nh * MIQP_POOL_MAX * fl, 64 * fl) && lab.need((size_t)PoolImproveDev::NB_MAX * fl); }
};

// the slices of a pass, greedily in handle order: a handle opens a new slice when its neighbours do not fit the results left of the current one; a
// handle without neighbours rides along.  -2: a total outside 0 .. NB_MAX, -3: slice_first holds fewer than slices + 1 words
int pool_explore_slices(const int* totals, int n, int* slice_first, int cap) {
  int ns = 1, sum = 0;
  for (int h = 0; h < n; ++h) {
    if (totals[h] < 0 || totals[h] > PoolImproveDev::NB_MAX) return -2;
    if (sum + totals[h] > PoolImproveDev::NB_MAX) { ns++; sum = 0; }
    sum += totals[h];
  }
  if (ns + 1 > cap) return -3;
  ns = 0; sum = 0; slice_first[0] = 0;
  for (int h = 0; h < n; ++h) {
    if (sum + totals[h] > PoolImproveDev::NB_MAX) { slice_first[++ns] = h; sum = 0; }
    sum += totals[h];
  }
  slice_first[++ns] = n;
  return ns;
}

// what the run knows of a handle of the call: its filter, the edge count of its obstacles, its n entries (fix: their records) of K places, entry 0's objective
struct PoolExploreHandle { int fam, L, n, K; double obj0; const signed char* fix; };

struct PoolExploreOut {
  std::vector<std::vector<miqp_pool_explore_c>> added;   // per handle, in the order of admission
  std::vector<signed char> fix; std::vector<double> obj;   // the places at the end, MIQP_POOL_MAX per handle
  std::vector<int> have, passes; std::vector<long> neighbours, iterations; std::vector<char> still_adding;   // per handle
  int call_passes = 0, call_slices = 0; float dev_ms = 0.0f;
  std::string err;
};

// The pools of the call's handles explored, H[h] for handle h of the call.  false: HIP error, or a refusal (O.err); nothing of any handle has been
// touched.  name: the entry point, for its messages; mode POOL_ADMIT_DISTINCT: pass 0 in front, the labels of every chunk, the admission by both
// signatures (miqp_solver_pool_explore_distinct); POOL_ADMIT_SETTLED: pass 0 and every slice's candidates through the settle rounds, the admission by
// the settled signature (.._explore_settled).  One pass is one pass of every handle that still has jumps; a handle that is full or admitted nothing has
// none from then on (pool_admit_body), so its figures stay those of its own last pass
bool pool_explore_run(const FixedCall& call, const char* name, int mode, const std::vector<PoolExploreHandle>& H, double max_rel, int max_passes, PoolExploreOut& O) {
  DevCtx& X = *call.X; DevBuf& B = X.B; hipStream_t st = X.stream; const Layout& Y = call.Y;
  const size_t fl = (size_t)Y.fixlen;
  const int nh = call.n, m = nh * MIQP_POOL_MAX;
  if ((int)H.size() != nh || nh < 1 || nh > FB_CAP / MIQP_POOL_MAX) return false;
  const bool distinct = mode != POOL_ADMIT_PLAIN, settled = mode == POOL_ADMIT_SETTLED;   // (distinct: what both opt-in calls need - labels, pass 0, the second signature)
  int kept = 0; for (int h = 0; h < nh; ++h) kept += H[h].n;
  const int settle_cap = std::max((int)PoolImproveDev::NB_MAX, kept);   // (pass 0 of the settled call settles the kept entries of all handles at once)
  PoolImproveDev& R = call_dev<PoolImproveDev>(X.device); PoolEntryDev& G = call_dev<PoolEntryDev>(X.device); PoolExploreDev& Q = call_dev<PoolExploreDev>(X.device);
  PoolSettleDev& W = call_dev<PoolSettleDev>(X.device);
  if (!R.ensure((size_t)Y.N * Y.nz) || !G.ensure((size_t)m, fl) || !Q.ensure((size_t)nh, fl) || (distinct && !Q.ensure_distinct((size_t)nh, fl))) return false;
  if (settled && !W.ensure((size_t)settle_cap, fl)) return false;
  // per mode: the admission kernel, the records its LDS holds beside the objectives of a pass, and how the refusal names both
  struct Mode { void (*admit)(PoolExploreArgs, int, int); int records; const char* kernel; const char* times; };
  static const Mode modes[3] = {{pool_admit_kernel, 2, "pool_admit_kernel", "twice"}, {pool_admit_distinct_kernel, 4, "pool_admit_distinct_kernel", "four times"},
                                {pool_admit_settled_kernel, 4, "pool_admit_settled_kernel", "four times"}};
  const Mode& M = modes[mode];
  const PoolDims dims = pool_dims(Y);
  const size_t jump_lds = fl + (size_t)pool_jump_units(dims) * sizeof(int), admit_lds = M.records * fl + (size_t)PoolImproveDev::NB_MAX * sizeof(double);
  if (std::max(jump_lds, admit_lds) > POOL_EXPLORE_LDS_MAX) {
    O.err = std::string(name) + ": the fix record of this shape does not fit the LDS of " + M.kernel + " " + M.times + " beside the objectives of a pass";
    std::fprintf(stderr, "[miqp_gpu] %s (%zu bytes)\n", O.err.c_str(), std::max(jump_lds, admit_lds)); return false;
  }
  if (distinct && !pool_label_fits(Y, name, O.err)) return false;
  HIP_OK(hipFuncSetAttribute((const void*)pool_jumps_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)jump_lds));
  HIP_OK(hipFuncSetAttribute((const void*)M.admit, hipFuncAttributeMaxDynamicSharedMemorySize, (int)admit_lds));
  if (distinct) {
    HIP_OK(hipFuncSetAttribute((const void*)pool_pass0_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(2 * fl)));
    if (!pool_label_set_lds(Y)) return false;
  }
  if (settled) HIP_OK(hipFuncSetAttribute((const void*)pool_settle_pick_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(2 * fl)));
  // the places, handle-major: the kept entries of a handle in front of its stride, the rest undecided and never expanded.  off0: the numbering of
  // pass 0 - the kept entries of the call, handle-major - as a scan over the places; kfix and kinst: those entries' records and handles, in a row
  std::vector<signed char> cur0((size_t)m * fl, (signed char)-1), kfix(settled ? (size_t)kept * fl : 0);
  std::vector<int> act(m, 0), einst(m), efam(m), state0(4 * (size_t)nh, 0), hK(nh), hL(nh), off0(m + 1, 0), kinst(kept), kn(nh);
  std::vector<double> hobj0(nh);
  for (int h = 0, at = 0; h < nh; ++h) {
    const PoolExploreHandle& P = H[h];
    if (P.n < 1 || P.n > P.K || P.K > MIQP_POOL_MAX || !P.fix) return false;
    std::memcpy(cur0.data() + (size_t)h * MIQP_POOL_MAX * fl, P.fix, (size_t)P.n * fl);
    if (settled) std::memcpy(kfix.data() + (size_t)at * fl, P.fix, (size_t)P.n * fl);
    for (int j = 0; j < MIQP_POOL_MAX; ++j) {
      const int e = h * MIQP_POOL_MAX + j;
      act[e] = j < P.n ? 1 : 0; einst[e] = h; efam[e] = P.fam; off0[e] = at + std::min(j, P.n);
    }
    for (int j = 0; j < P.n; ++j) kinst[at + j] = h;
    state0[4 * (size_t)h] = P.n; hK[h] = P.K; hL[h] = P.L; hobj0[h] = P.obj0; kn[h] = P.n;
    at += P.n; off0[(size_t)(h + 1) * MIQP_POOL_MAX] = at;
  }
  HIP_OK(hipMemsetAsync(B.batch_inst, 0, (size_t)FB_CHUNK * 4, st));
  HIP_OK(hipMemcpyAsync(G.cur, cur0.data(), (size_t)m * fl, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(G.act, act.data(), (size_t)m * sizeof(int), hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(G.ent_inst, einst.data(), (size_t)m * sizeof(int), hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(G.ent_fam, efam.data(), (size_t)m * sizeof(int), hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(G.off, off0.data(), (size_t)(m + 1) * sizeof(int), hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(Q.state, state0.data(), 4 * (size_t)nh * sizeof(int), hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(Q.hK, hK.data(), (size_t)nh * sizeof(int), hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(Q.hL, hL.data(), (size_t)nh * sizeof(int), hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(Q.hobj0, hobj0.data(), (size_t)nh * sizeof(double), hipMemcpyHostToDevice, st));
  HIP_OK(hipMemsetAsync(G.cnt, 0, (size_t)m * sizeof(int), st)); HIP_OK(hipMemsetAsync(G.cur_obj, 0, (size_t)m * sizeof(double), st));
  const DevBuf Bp = fixed_chain_settings(B);
  PoolExploreArgs E;
  PoolImproveArgs& A = E.A;
  A.cur = G.cur; A.cur_obj = G.cur_obj; A.act = G.act; A.cnt = G.cnt; A.moves = G.moves; A.words = G.words; A.res = R.res; A.pool_fix = B.pool_fix;
  A.ent_inst = G.ent_inst; A.ent_fam = G.ent_fam; A.off = G.off; A.batch_inst = B.batch_inst;
  A.dims = dims; A.fixlen = (int)fl; A.m = m;   // (every place of every pool is an entry of the kernels: a free one is not expanded and has no jumps)
  E.nh = nh; E.hK = Q.hK; E.hL = Q.hL; E.hobj0 = Q.hobj0; E.sig = Q.sig; E.state = Q.state; E.out = Q.out; E.max_rel = max_rel; E.pass = 0;
  E.csig = distinct ? Q.csig.p : nullptr; E.lab = settled ? W.cur.p : distinct ? Q.lab.p : nullptr;
  E.has_sig = Q.has_sig; E.fin = settled ? W.last.p : nullptr; E.solves = settled ? W.solves.p : nullptr; E.settle_it = settled ? W.acc_it.p : nullptr;
  PoolSettleTally tally;   // (the settle rounds' own sums over the call: the handles' figures come from the device, per handle)
  std::vector<int> first(nh + 2), offh(nh + 1);
  // the slices of a pass whose handle h has totals[h] nodes (miqp_gpu_pool_explore_plan, the very function), and the call's number of every handle's first
  auto plan = [&](const std::vector<int>& totals) -> int {
    const int ns = miqp_gpu_pool_explore_plan(totals.data(), nh, first.data(), nh + 2);
    offh[0] = 0;
    for (int h = 0; h < nh; ++h) offh[h + 1] = offh[h] + totals[h];
    return ns;
  };
  // `nodes` nodes from the call's number g0 on through the chain, a chunk at a time, as the climb sends them (no segments, the trajectories written
  // over); results and labels relative to g0
  auto solve_nodes = [&](int g0, int nodes) -> bool {
    for (int k0 = 0; k0 < nodes; k0 += FB_CHUNK) {
      const int bc = std::min(FB_CHUNK, nodes - k0);
      hipLaunchKernelGGL(pool_neighbour_kernel, dim3((bc + 3) / 4), dim3(256), 0, st, A, g0 + k0, bc, 0);
      HIP_OK(hipGetLastError());
      if (!fixed_chunk(X, Bp, Y, call.dev(), nh, FixedChunk{bc, k0, R.res + k0, R.Z})) return false;
      if (distinct && !pool_label_chunk(X, Y, nh, bc, R.res + k0, R.Z, Q.lab + (size_t)k0 * fl)) return false;   // (per chunk: the next one writes over R.Z)
    }
    return true;
  };
  // behind a pass: the jumps of the next one, and what the host needs of both
  std::vector<int> cnt(m), state(4 * (size_t)nh); std::vector<miqp_pool_explore_c> rec(m);
  auto finish_pass = [&]() -> bool {
    hipLaunchKernelGGL(pool_jumps_kernel, dim3(m), dim3(64), jump_lds, st, E);
    hipLaunchKernelGGL(pool_offsets_kernel, dim3(1), dim3(256), 0, st, A);
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(X.ev1, st));
    HIP_OK(hipMemcpyAsync(cnt.data(), G.cnt, (size_t)m * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(state.data(), Q.state, state.size() * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(rec.data(), Q.out, (size_t)m * sizeof(miqp_pool_explore_c), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st)); HIP_OK(hipGetLastError());
    float ms = 0.0f; (void)hipEventElapsedTime(&ms, X.ev0, X.ev1); O.dev_ms += ms;
    return true;
  };
  // the settled call, behind the chain and labels of the slice of handles h0 .. h1 - 1: the candidates, the live list of those whose labels moved,
  // their rounds from the second on
  auto settle_slice = [&](int h0, int h1, int nodes) -> bool {
    const PoolSettleArgs S = pool_settle_args(W, B, Y, nodes);
    hipLaunchKernelGGL(pool_settle_pick_kernel, dim3(nodes), dim3(64), 2 * fl, st, E, S, (const signed char*)Q.lab, h0, h1, (int)PoolImproveDev::NB_MAX);
    HIP_OK(hipGetLastError());
    int live = 0;
    return pool_settle_compact(X, S, live, tally) && pool_settle_rounds(call, Bp, S, R.Z, 2, live, tally);
  };
  O.added.assign(nh, {}); O.have = kn; O.passes.assign(nh, 0); O.neighbours.assign(nh, 0); O.iterations.assign(nh, 0); O.still_adding.assign(nh, 0);
  HIP_OK(hipEventRecord(X.ev0, st));
  if (settled) {   // pass 0: the kept entries' own records to their fixed points, all handles at once; the signatures of both kinds
    if (!pool_settle_records(call, Bp, pool_settle_args(W, B, Y, kept), R.Z, kfix.data(), kinst.data(), tally)) return false;
    hipLaunchKernelGGL(pool_pass0_kernel, dim3(nh), dim3(64), 2 * fl, st, E, 0, settle_cap, 1);
    HIP_OK(hipGetLastError());
  } else if (distinct) {   // pass 0: the kept entries' own records through the chain - node g of off0 is a place with the empty move -, their labels, the signatures of those
    HIP_OK(hipMemset2DAsync(G.moves, (size_t)POOL_MOVES_MAX * sizeof(int4), 0, sizeof(int4), (size_t)m, st));
    const int ns = plan(kn);
    if (ns < 1) return false;
    for (int s = 0; s < ns; ++s) {
      const int h0 = first[s], h1 = first[s + 1];
      if (!solve_nodes(offh[h0], offh[h1] - offh[h0])) return false;
      hipLaunchKernelGGL(pool_pass0_kernel, dim3(h1 - h0), dim3(64), 2 * fl, st, E, h0, (int)PoolImproveDev::NB_MAX, 0);
      HIP_OK(hipGetLastError());
    }
  }
  if (!finish_pass()) return false;
  if (distinct)
    for (int h = 0; h < nh; ++h) { O.neighbours[h] += settled ? state[4 * (size_t)h + 3] : kn[h]; O.iterations[h] += state[4 * (size_t)h + 2]; }
  std::vector<int> th(nh);
  for (int pass = 0;;) {
    long total = 0;
    for (int h = 0; h < nh; ++h) {
      th[h] = 0;
      for (int k = h * MIQP_POOL_MAX; k < (h + 1) * MIQP_POOL_MAX; ++k) {
        if (cnt[k] < 0 || cnt[k] > POOL_MOVES_MAX) { std::fprintf(stderr, "[miqp_gpu] %s: jump count %d of place %d\n", name, cnt[k], k); return false; }
        th[h] += cnt[k];
      }
      total += th[h];
    }
    if (total == 0 || pass == max_passes) break;
    E.pass = pass + 1;
    const int ns = plan(th);
    if (ns < 1) return false;
    HIP_OK(hipEventRecord(X.ev0, st));
    for (int s = 0; s < ns; ++s) {
      const int h0 = first[s], h1 = first[s + 1], nodes = offh[h1] - offh[h0];
      if (nodes > PoolImproveDev::NB_MAX) { std::fprintf(stderr, "[miqp_gpu] %s: a slice of %d nodes\n", name, nodes); return false; }
      if (nodes == 0 || h1 <= h0) continue;   // (handles without jumps: nothing to admit, and the host does not read their words)
      if (!solve_nodes(offh[h0], nodes) || (settled && !settle_slice(h0, h1, nodes))) return false;
      hipLaunchKernelGGL(M.admit, dim3(h1 - h0), dim3(64), admit_lds, st, E, h0, (int)PoolImproveDev::NB_MAX);
      HIP_OK(hipGetLastError());
      O.call_slices++;
    }
    if (!finish_pass()) return false;
    pass++; O.call_passes++;
    for (int h = 0; h < nh; ++h) {   // a handle without jumps in this pass has stopped: its figures stay
      if (th[h] == 0) continue;
      const int* const sh = state.data() + 4 * (size_t)h;
      if (sh[0] != O.have[h] + sh[1] || sh[1] < 0 || sh[0] > H[h].K || sh[3] < 0) { std::fprintf(stderr, "[miqp_gpu] %s: handle %d: %d entries behind %d, %d admitted\n", name, h, sh[0], O.have[h], sh[1]); return false; }
      O.passes[h]++; O.neighbours[h] += th[h] + (settled ? sh[3] : 0); O.iterations[h] += sh[2];
      for (int k = 0; k < sh[1]; ++k) O.added[h].push_back(rec[(size_t)h * MIQP_POOL_MAX + k]);
      O.have[h] = sh[0];
      O.still_adding[h] = sh[1] > 0 && pass == max_passes ? 1 : 0;
    }
  }
  O.fix.resize((size_t)m * fl); O.obj.resize(m);
  HIP_OK(hipMemcpy(O.fix.data(), G.cur, (size_t)m * fl, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(O.obj.data(), G.cur_obj, (size_t)m * sizeof(double), hipMemcpyDeviceToHost));
  return true;
}

// What the handles receive of a run, behind its last read-back: the added entries behind the ones they hold, the `out` records (outs[h], counts[h]),
// last_timing, the dropped refined pool and, when the last pass still added and places are free, the last error.  Entries added in all, or -3 when the
// run's figures do not fit a handle (nothing has been written then)
int pool_explore_store(const FixedCall& call, const char* name, const std::vector<PoolExploreHandle>& H, const PoolExploreOut& O, int max_passes, double t_call,
                       miqp_pool_explore_c* const* outs, int* const* counts) {
  const size_t fl = (size_t)call.Y.fixlen;
  for (int h = 0; h < call.n; ++h) if (O.have[h] != H[h].n + (int)O.added[h].size() || O.have[h] > H[h].K) return -3;
  const double call_s = wall_s() - t_call;
  int all = 0;
  for (int h = 0; h < call.n; ++h) {
    miqp_solver_t* s = call.S[h]; const int n = H[h].n, added = (int)O.added[h].size();
    // the old entries stay as the handle holds them; the added ones go behind them
    const signed char* const pf = O.fix.data() + (size_t)h * MIQP_POOL_MAX * fl; const double* const po = O.obj.data() + (size_t)h * MIQP_POOL_MAX;
    s->pool_fix.resize((size_t)n * fl); s->pool_obj.resize(n);
    s->pool_fix.insert(s->pool_fix.end(), pf + (size_t)n * fl, pf + (size_t)(n + added) * fl);
    s->pool_obj.insert(s->pool_obj.end(), po + n, po + n + added);
    s->pool_n = n + added;
    for (int k = 0; k < added; ++k) outs[h][k] = O.added[h][k];
    if (counts[h]) *counts[h] = added;
    s->pr_n = 0; std::vector<char>().swap(s->pr_ok); std::vector<signed char>().swap(s->pr_fix); std::vector<double>().swap(s->pr_Z);
    s->timing[0] = call_s; s->timing[1] = O.dev_ms * 1e-3; s->timing[2] = O.passes[h]; s->timing[3] = (double)O.neighbours[h]; s->timing[4] = (double)O.iterations[h]; s->timing[5] = O.still_adding[h] ? 1 : 0;
    if (O.still_adding[h] && n + added < H[h].K) {
      char msg[200]; std::snprintf(msg, sizeof msg, "%s: the last of %d passes still added an entry and places are free; more passes may fill them", name, max_passes);
      s->err = msg;
    }
    all += added;
  }
  return all;
}

// the explore of the pools of every handle of an open call (all of them have entries and free places).  Entries added, or -3 (the handles then carry
// the run's refusal, if it gave one)
int pool_explore_call(const FixedCall& call, const char* name, int mode, int max_passes, double max_rel, double t_call, miqp_pool_explore_c* const* outs, int* const* counts,
                      int* passes_run = nullptr, int* slices_run = nullptr) {
  std::vector<PoolExploreHandle> H(call.n);
  for (int h = 0; h < call.n; ++h) {
    const miqp_solver_t* s = call.S[h];
    H[h] = PoolExploreHandle{s->pool_fam, s->inst.L, miqp_solver_pool_count(s), std::min(s->pool_cap, MIQP_POOL_MAX), s->pool_obj[0], s->pool_fix.data()};
  }
  PoolExploreOut O;
  if (!pool_explore_run(call, name, mode, H, max_rel, max_passes, O)) {
    (void)hipStreamSynchronize(call.X->stream);
    if (!O.err.empty()) for (int h = 0; h < call.n; ++h) call.S[h]->err = O.err;
    return -3;
  }
  if (passes_run) *passes_run = O.call_passes;
  if (slices_run) *slices_run = O.call_slices;
  return pool_explore_store(call, name, H, O, max_passes, t_call, outs, counts);
}

}  // namespace

extern "C" {

int miqp_gpu_pool_explore_size(void) { return (int)sizeof(miqp_pool_explore_c); }

int miqp_gpu_pool_jumps(int cars, int steps, int obstacles, int max_lines, int families, const signed char* decisions, int* moves4, int cap) {
  if (!decisions || !moves4 || cars <= 0 || steps <= 0 || obstacles < 0 || max_lines < 0) return -1;
  if (families < 1 || families >= POOL_FAM_TIMING || !(families & (POOL_FAM_OBSTACLE | POOL_FAM_CAR_CAR))) return -2;
  const PoolJumpDims J{PoolDims{cars, steps, obstacles, cars * (cars - 1) / 2}, max_lines};
  std::vector<PoolMove> mv;
  for (int u = 0, n = pool_jump_units(J.d); u < n && (int)mv.size() < POOL_MOVES_MAX; ++u)
    (void)pool_unit_jumps(J, families, u, decisions, [&](int, const PoolMove& m) { if ((int)mv.size() < POOL_MOVES_MAX) mv.push_back(m); });
  if (cap < (int)mv.size()) return -3;
  for (size_t k = 0; k < mv.size(); ++k) { moves4[4 * k] = mv[k].first; moves4[4 * k + 1] = mv[k].stride; moves4[4 * k + 2] = mv[k].count; moves4[4 * k + 3] = mv[k].value; }
  return (int)mv.size();
}

int miqp_gpu_pool_explore_plan(const int* handle_totals, int n, int* slice_first, int cap) {
  if (!handle_totals || !slice_first || n <= 0 || cap < 0) return -1;
  return pool_explore_slices(handle_totals, n, slice_first, cap);
}

}  // extern "C"

namespace {

thread_local int g_pool_explore_multi_last[2] = {0, 0};   // passes and slices of the calling thread's last miqp_solver_pool_explore_multi (miqp_gpu_pool_explore_multi_last)

// a filter the explore can jump under: in 1 .. 15 with the obstacle or the car/car family
inline bool pool_explore_filter_ok(int fam) { return fam >= 1 && fam < POOL_FAM_TIMING && (fam & (POOL_FAM_OBSTACLE | POOL_FAM_CAR_CAR)); }

// the three explore entries of one handle: what they refuse, then the run with one handle and what the handle keeps
int pool_explore_entry(miqp_solver_t* s, const char* name, int mode, int max_passes, double max_rel, miqp_pool_explore_c* out, int cap) {
  if (s) s->err.clear();   // (miqp_solver_last_error speaks of this call from here on)
  if (!s || !s->has_inst || !out || cap < 0 || max_rel != max_rel) return -1;
  if (!pool_explore_filter_ok(s->pool_fam)) return -2;
  if (max_passes < 1 || max_passes > POOL_EXPLORE_PASSES_MAX) return -2;
  const int n = miqp_solver_pool_count(s), K = std::min(s->pool_cap, MIQP_POOL_MAX);
  if (n == 0 || n >= K) return 0;   // (nothing to jump from, or no free place: no device is touched)
  if (cap < K - n) return -2;
  { int ndev = 0; if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return -3; }
  miqp_solver_t* one[1] = {s};
  BatchShape bs = batch_layout(one, 1);
  if (!bs.ok || bs.Y.fixlen != s->pool_fixlen || s->pool_fix.size() < (size_t)n * bs.Y.fixlen || s->pool_obj.size() < (size_t)n) return -1;
  const double t_call = wall_s();
  FixedCall call;
  if (call.open(one, 1, bs.Y) != 0) return -3;
  int* const none[1] = {nullptr};
  return pool_explore_call(call, name, mode, max_passes, max_rel, t_call, &out, none);
}

}  // namespace

extern "C" {

int miqp_solver_pool_explore(miqp_solver_t* s, int max_passes, double max_rel, miqp_pool_explore_c* out, int cap) {
  return pool_explore_entry(s, "miqp_solver_pool_explore", POOL_ADMIT_PLAIN, max_passes, max_rel, out, cap);
}

int miqp_solver_pool_explore_distinct(miqp_solver_t* s, int max_passes, double max_rel, miqp_pool_explore_c* out, int cap) {
  return pool_explore_entry(s, "miqp_solver_pool_explore_distinct", POOL_ADMIT_DISTINCT, max_passes, max_rel, out, cap);
}

int miqp_solver_pool_explore_settled(miqp_solver_t* s, int max_passes, double max_rel, miqp_pool_explore_c* out, int cap) {
  return pool_explore_entry(s, "miqp_solver_pool_explore_settled", POOL_ADMIT_SETTLED, max_passes, max_rel, out, cap);
}

int miqp_solver_pool_explore_multi(miqp_solver_t* const* solvers, int n, int mode, int max_passes, double max_rel, miqp_pool_explore_c* out, int cap, int* counts) {
  static const char* const name = "miqp_solver_pool_explore_multi";
  if (!solvers || !out || !counts || n <= 0 || cap < 0 || max_rel != max_rel || mode < POOL_ADMIT_PLAIN || mode > POOL_ADMIT_SETTLED) return -1;
  if (max_passes < 1 || max_passes > POOL_EXPLORE_PASSES_MAX) return -2;
  if (n > FB_CAP / MIQP_POOL_MAX) return -5;
  BatchShape bs;
  if (const int rc = fixed_multi_check(solvers, n, bs)) return rc;
  const Layout& Y = bs.Y; const size_t fl = (size_t)Y.fixlen;
  // a handle takes part when it has entries and free places
  std::vector<int> part; int need = 0;
  for (int h = 0; h < n; ++h) {
    const miqp_solver_t* s = solvers[h];
    const int k = miqp_solver_pool_count(s), K = std::min(s->pool_cap, MIQP_POOL_MAX);
    if (k > 0 && (s->pool_fixlen != Y.fixlen || s->pool_fix.size() < (size_t)k * fl || s->pool_obj.size() < (size_t)k)) return -1;
    if (k == 0 || k >= K) continue;
    part.push_back(h); need = std::max(need, K - k);
  }
  for (const int h : part)
    if (!pool_explore_filter_ok(solvers[h]->pool_fam)) {
      char msg[240]; std::snprintf(msg, sizeof msg, "%s: handle %d of the call has entries and free places under filter %d; the explore needs a filter in 1 .. 15 with the obstacle or the car/car family", name, h, solvers[h]->pool_fam);
      solvers[h]->err = msg;
      return -2;
    }
  if (cap < need) return -2;
  for (int h = 0; h < n; ++h) solvers[h]->err.clear();   // (miqp_solver_last_error of every handle speaks of this call from here on)
  if (part.empty()) { for (int h = 0; h < n; ++h) counts[h] = 0; return 0; }   // (nothing to run: no device is touched)
  { int ndev = 0; if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return -3; }
  const int np = (int)part.size();
  std::vector<miqp_solver_t*> S(np); std::vector<miqp_pool_explore_c*> outs(np); std::vector<int> added(np, 0); std::vector<int*> cnts(np);
  for (int q = 0; q < np; ++q) { S[q] = solvers[part[q]]; outs[q] = out + (size_t)part[q] * cap; cnts[q] = &added[q]; }
  const double t_call = wall_s();
  FixedCall call;
  if (call.open(S.data(), np, Y) != 0) return -3;
  int passes_run = 0, slices_run = 0;
  // (what a handle hears of the run - the LDS refusal, "the last of N passes still added" - is word for word what its single call of the mode says)
  static const char* const single[3] = {"miqp_solver_pool_explore", "miqp_solver_pool_explore_distinct", "miqp_solver_pool_explore_settled"};
  const int rc = pool_explore_call(call, single[mode], mode, max_passes, max_rel, t_call, outs.data(), cnts.data(), &passes_run, &slices_run);
  if (rc < 0) return rc;
  for (int h = 0; h < n; ++h) counts[h] = 0;
  for (int q = 0; q < np; ++q) counts[part[q]] = added[q];
  g_pool_explore_multi_last[0] = passes_run; g_pool_explore_multi_last[1] = slices_run;
  return rc;
}

void miqp_gpu_pool_explore_multi_last(int* passes, int* slices) {
  if (passes) *passes = g_pool_explore_multi_last[0];
  if (slices) *slices = g_pool_explore_multi_last[1];
}

}  // extern "C"

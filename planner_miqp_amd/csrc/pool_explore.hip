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
//                          the climb's, unchanged, chunk by chunk: at most 16 entries of 512 jumps are the 8192 results the climb holds - no slices
//   pool_admit_kernel      ONE wavefront: the objectives of the pass's feasible neighbours within the cost cap staged in LDS; then, as long as a
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

struct PoolExploreArgs {
  PoolImproveArgs A;              // the climb's: cur = the places of the pool, act = expand it in this pass, cnt, moves, off, res, ent_fam; A.m = places
  int L;                          // edge count of an obstacle
  signed char* sig;               // [places] the signatures of the pool's entries under the handle's filter
  int* state;                     // [0] entries in the pool, [1] admitted by the last pass, [2] iterations of the last pass's neighbours
  miqp_pool_explore_c* out;       // [places] the records of the last pass's admitted entries
  double obj0, max_rel; int pass;
  // the distinct call only (miqp_solver_pool_explore_distinct, below): the signatures of the entries' CANONICAL records under the handle's filter, and
  // the labelled record of every neighbour of the pass (pool_label_kernel, chunk by chunk)
  signed char* csig;              // [places]
  const signed char* lab;         // [NB_MAX]
  // the settled call only (miqp_solver_pool_explore_settled): csig holds the signatures of the SETTLED labels, lab the settled labels of every
  // neighbour of the pass (PoolSettleArgs::cur); a place has a settled signature when has_sig says so; fin and solves: the last answer of every
  // neighbour's settling and the number of its solves (0: no candidate)
  int* has_sig;                   // [places]
  const miqp_fixed_result_c* fin; const int* solves;   // [NB_MAX]
};

__global__ __launch_bounds__(64) void pool_jumps_kernel(const PoolExploreArgs E) {
  extern __shared__ uint4 pj_lds[];   // the record; behind it one int per unit
  const PoolImproveArgs& A = E.A;
  const int e = blockIdx.x, lane = threadIdx.x, chunks = A.fixlen >> 4;
  const PoolJumpDims J{A.dims, E.L};
  if (e >= A.m) return;
  if (!A.act[e]) { if (lane == 0) A.cnt[e] = 0; return; }
  const signed char* const rec = (const signed char*)pj_lds;
  pool_stage(pj_lds, (const uint4*)(A.cur + (size_t)e * A.fixlen), chunks, lane);
  __syncthreads();
  const int fam = A.ent_fam[e];
  const int total = pool_count_scan_emit(pool_jump_units(A.dims), (int*)(pj_lds + chunks), A.moves + (size_t)e * POOL_MOVES_MAX, lane,
                                         [&](int u, auto emit) { return pool_unit_jumps(J, fam, u, rec, emit); });
  if (lane == 0) A.cnt[e] = total;
}

// The neighbour of place e behind the move mv, the whole wavefront: the parent's record with the move patched in into rec, its signature under the
// handle's filter into sg (both in LDS).  True: the signature is one of the first n of the pool
__device__ inline bool pool_candidate_known(const PoolExploreArgs& E, int e, const int4 mv, uint4* rec, uint4* sg, int n, int lane) {
  const PoolImproveArgs& A = E.A; const int chunks = A.fixlen >> 4;
  pool_stage(rec, (const uint4*)A.cur + (size_t)e * chunks, chunks, lane, sg, mv);
  pool_sign(A.dims, A.ent_fam[0], rec, sg, lane);
  return pool_known(sg, (const uint4*)E.sig, n, chunks, lane);
}

// Pass 0, the whole wavefront: record j < n of the array src(j) names (the pool's places, or the labels of the pass) signed under the handle's
// filter into place j of dst.  rec, sg: a record and a signature in LDS
template <class Src>
__device__ inline void pool_sign_places(const PoolExploreArgs& E, uint4* rec, uint4* sg, int n, Src src, uint4* dst, int lane) {
  const PoolImproveArgs& A = E.A; const int chunks = A.fixlen >> 4, fam = A.ent_fam[0];
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
constexpr int POOL_ADMIT_PLAIN = 0, POOL_ADMIT_DISTINCT = 1, POOL_ADMIT_SETTLED = 2;
template <int MODE>
__device__ inline void pool_admit_body(const PoolExploreArgs& E, int nb_max, uint4* pa_lds) {
  const PoolImproveArgs& A = E.A;
  constexpr bool DISTINCT = MODE != POOL_ADMIT_PLAIN, SETTLED = MODE == POOL_ADMIT_SETTLED;
  const int lane = threadIdx.x, chunks = A.fixlen >> 4, K = A.m;
  uint4* const cand = pa_lds; uint4* const csig = cand + chunks;
  uint4* const ccan = csig + chunks; uint4* const ccsg = ccan + chunks;   // DISTINCT: the candidate's labelled record and its signature
  double* const key = (double*)(csig + (DISTINCT ? 3 : 1) * chunks);
  const int n0 = min(max(E.state[0], 0), K), total = min(max(A.off[K], 0), nb_max);
  uint4* const pool = (uint4*)A.cur; uint4* const sig = (uint4*)E.sig;
  // the signatures of the entries that have none yet: all of them in pass 1, later the ones the pass before appended (their signature is written
  // with them) - so only pass 1 builds any
  if (E.pass == 1) pool_sign_places(E, cand, csig, n0, [&](int) { return (const uint4*)pool; }, sig, lane);
  // the objectives of the pass's candidates, place by place (off[0] = 0 and off ascends: every neighbour below `total` is visited once)
  int it = 0;
  for (int e = 0; e < K; ++e)
    for (int g0 = A.off[e], g1 = min(A.off[e + 1], total), g = g0 + lane; g < g1; g += 64) {
      const miqp_fixed_result_c r = A.res[g];
      it += r.iterations;
      key[g] = pool_is_candidate(r, E.obj0, E.max_rel, g - g0, e, n0) ? r.objective : POOL_ADMIT_NONE;
    }
  for (int d = 32; d >= 1; d >>= 1) it += __shfl_xor(it, d, 64);
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
    const int e = pool_entry_of(A.off, K, bg);   // (a staged objective: a candidate, so its move is one of the table and e < n0)
    const int4 mv = A.moves[(size_t)e * POOL_MOVES_MAX + bg - A.off[e]];
    if (pool_candidate_known(E, e, mv, cand, csig, n, lane)) continue;
    int solves = 0;
    if (SETTLED) {
      solves = E.solves[bg];
      if (solves == 0 || E.fin[bg].status != 0) continue;   // (uniform: no settled labels)
    }
    if (DISTINCT) {
      uint4* const can = (uint4*)E.csig;
      pool_stage(ccan, (const uint4*)E.lab + (size_t)bg * chunks, chunks, lane, ccsg);
      pool_sign(A.dims, A.ent_fam[0], ccan, ccsg, lane);
      if (pool_known(ccsg, can, n, chunks, lane, SETTLED ? E.has_sig : nullptr)) continue;   // (an alias of an entry: the same solution under labels of another signature)
      pool_stage(can + (size_t)n * chunks, ccsg, chunks, lane);
      if (SETTLED && lane == 0) E.has_sig[n] = 1;
    }
    for (int c = lane; c < chunks; c += 64) { pool[(size_t)n * chunks + c] = cand[c]; sig[(size_t)n * chunks + c] = csig[c]; }   // (one loop for both: two cost the plain kernel four registers)
    if (lane == 0) {
      A.cur_obj[n] = bo;
      miqp_pool_explore_c o;
      o.parent = e; o.pass = E.pass; o.first = mv.x; o.stride = mv.y; o.count = mv.z; o.value = mv.w; o.iterations = A.res[bg].iterations; o.reserved = SETTLED ? abs(solves) : 0; o.objective = bo;
      E.out[added] = o;
    }
    n++; added++;
    __syncthreads();   // (the appended signature is compared with the next candidate's)
  }
  for (int j = lane; j < K; j += 64) A.act[j] = j >= n0 && j < n ? 1 : 0;   // the next pass expands what this one added
  if (lane == 0) { E.state[0] = n; E.state[1] = added; E.state[2] = it; }
}

__global__ __launch_bounds__(64) void pool_admit_kernel(const PoolExploreArgs E, int nb_max) {
  extern __shared__ uint4 pa_lds[];   // the candidate's record, its signature; behind them one objective per neighbour of the pass
  pool_admit_body<POOL_ADMIT_PLAIN>(E, nb_max, pa_lds);
}

__global__ __launch_bounds__(64) void pool_admit_distinct_kernel(const PoolExploreArgs E, int nb_max) {
  extern __shared__ uint4 pa_lds[];   // the candidate's record, its signature, its labelled record, that one's signature; behind them the objectives
  pool_admit_body<POOL_ADMIT_DISTINCT>(E, nb_max, pa_lds);
}

__global__ __launch_bounds__(64) void pool_admit_settled_kernel(const PoolExploreArgs E, int nb_max) {
  extern __shared__ uint4 pa_lds[];   // the candidate's record, its signature, its settled labels, their signature; behind them the objectives
  pool_admit_body<POOL_ADMIT_SETTLED>(E, nb_max, pa_lds);
}

// Behind the chain and the labels of a pass of the settled call, one wavefront per neighbour: is it a candidate (see the head of the file), and did
// its labels move.  Writes the neighbour's words of the settle rounds (PoolSettleArgs, by neighbour number): its first labels as the record of
// round 2, its first answer, 1 solve (0: no candidate), the moved flag.  first_lab: the labelled records of the pass's neighbours
__global__ __launch_bounds__(64) void pool_settle_pick_kernel(const PoolExploreArgs E, const PoolSettleArgs S, const signed char* first_lab, int nb_max) {
  extern __shared__ uint4 pk_lds[];   // the neighbour's record, its signature
  const PoolImproveArgs& A = E.A;
  const int g = blockIdx.x, lane = threadIdx.x, chunks = A.fixlen >> 4, K = A.m;
  const int n0 = min(max(E.state[0], 0), K), total = min(max(A.off[K], 0), nb_max);
  if (g >= total || g >= S.n) return;
  uint4* const rec = pk_lds; uint4* const sg = rec + chunks;
  const int e = pool_entry_of(A.off, K, g), jm = g - A.off[e];
  // (cand and moved are uniform over the wavefront.)  The pool only grows within a pass: new against its first n0 signatures is what the admission can ask at most
  bool cand = pool_is_candidate(A.res[g], E.obj0, E.max_rel, jm, e, n0);
  if (cand) cand = !pool_candidate_known(E, e, A.moves[(size_t)e * POOL_MOVES_MAX + jm], rec, sg, n0, lane);
  bool moved = false;
  if (cand) {
    const uint4* const lab = (const uint4*)first_lab + (size_t)g * chunks;
    moved = pool_records_differ(lab, rec, chunks, lane);
    pool_stage((uint4*)S.cur + (size_t)g * chunks, lab, chunks, lane);
  }
  if (lane == 0) { pool_settle_copy_result(S.last + g, A.res + g); S.solves[g] = cand ? 1 : 0; S.moved[g] = moved ? 1 : 0; S.round_it[g] = 0; }
}

// Pass 0 of the distinct and the settled call, ONE wavefront, behind the kept entries' own solves.  Distinct (behind the chain and pool_label_kernel):
// per kept entry the signature of its canonical record - of its as-found bytes when its own QP is not feasible at the tight tolerance - and the
// iterations of the pass.  Settled (behind the settle rounds): per kept entry its plain signature (the pick kernel of pass 1 compares with it) and
// the signature of its settled labels, with the word that says whether it has one
__global__ __launch_bounds__(64) void pool_pass0_kernel(const PoolExploreArgs E, int settled) {
  extern __shared__ uint4 p0_lds[];   // a record, its signature
  const PoolImproveArgs& A = E.A;
  const int lane = threadIdx.x, chunks = A.fixlen >> 4, K = A.m;
  uint4* const rec = p0_lds; uint4* const sg = rec + chunks;
  const int n0 = min(max(E.state[0], 0), K);
  const uint4* const cur = (const uint4*)A.cur; const uint4* const lab = (const uint4*)E.lab;
  if (settled) {
    pool_sign_places(E, rec, sg, n0, [&](int) { return cur; }, (uint4*)E.sig, lane);
    pool_sign_places(E, rec, sg, n0, [&](int) { return lab; }, (uint4*)E.csig, lane);
    for (int j = lane; j < K; j += 64) E.has_sig[j] = j < n0 && E.fin[j].status == 0 ? 1 : 0;
  } else {
    int it = 0;
    for (int j = 0; j < n0; ++j) it += A.res[j].iterations;
    pool_sign_places(E, rec, sg, n0, [&](int j) { return A.res[j].status == 0 ? lab : cur; }, (uint4*)E.csig, lane);
    if (lane == 0) E.state[2] = it;
  }
}

// buffers of the call beside the climb's (PoolImproveDev, PoolEntryDev), cached per device (DevArr: grown, not shrunk).  has_sig is the settled
// call's (a place has a settled signature); csig and lab the distinct and the settled call's: the second signatures of the places and the labelled
// records of a pass's neighbours
struct PoolExploreDev {
  DevArr<signed char> sig, csig, lab; DevArr<int> state, has_sig; DevArr<miqp_pool_explore_c> out;
  bool ensure(size_t fl) { return state.need(4) && has_sig.need(MIQP_POOL_MAX) && out.need(MIQP_POOL_MAX) && sig.need(MIQP_POOL_MAX * fl); }
  bool ensure_distinct(size_t fl) { return csig.need(MIQP_POOL_MAX * fl) && lab.need((size_t)PoolImproveDev::NB_MAX * fl); }
};

struct PoolExploreOut {
  std::vector<miqp_pool_explore_c> added;
  std::vector<signed char> fix; std::vector<double> obj;   // the places of the pool at the end
  int passes = 0; long neighbours = 0, iterations = 0; bool still_adding = false; float dev_ms = 0.0f;
  std::string err;
};

// false: HIP error (nothing of the handle has been touched).  n: entries in the pool, K: its places; name: the entry point, for its messages;
// mode POOL_ADMIT_DISTINCT: pass 0 in front, the labels of every chunk, the admission by both signatures (miqp_solver_pool_explore_distinct);
// POOL_ADMIT_SETTLED: pass 0 and every pass's candidates through the settle rounds, the admission by the settled signature (.._explore_settled)
bool pool_explore_run(const FixedCall& call, const char* name, int mode, int fam, int L, const signed char* fix, int n, int K, double obj0, double max_rel, int max_passes, PoolExploreOut& O) {
  DevCtx& X = *call.X; DevBuf& B = X.B; hipStream_t st = X.stream; const Layout& Y = call.Y;
  const size_t fl = (size_t)Y.fixlen;
  const bool distinct = mode != POOL_ADMIT_PLAIN, settled = mode == POOL_ADMIT_SETTLED;   // (distinct: what both opt-in calls need - labels, pass 0, the second signature)
  PoolImproveDev& R = call_dev<PoolImproveDev>(X.device); PoolEntryDev& G = call_dev<PoolEntryDev>(X.device); PoolExploreDev& Q = call_dev<PoolExploreDev>(X.device);
  PoolSettleDev& W = call_dev<PoolSettleDev>(X.device);
  if (!R.ensure((size_t)Y.N * Y.nz) || !G.ensure(MIQP_POOL_MAX, fl) || !Q.ensure(fl) || (distinct && !Q.ensure_distinct(fl))) return false;
  if (settled && !W.ensure((size_t)PoolImproveDev::NB_MAX, fl)) return false;
  // per mode: the admission kernel, the records its LDS holds beside the objectives of a pass, and how the refusal names both
  struct Mode { void (*admit)(PoolExploreArgs, int); int records; const char* kernel; const char* times; };
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
  std::vector<int> act(MIQP_POOL_MAX, 0); for (int k = 0; k < n; ++k) act[k] = 1;
  const int state0[4] = {n, 0, 0, 0};
  HIP_OK(hipMemsetAsync(B.batch_inst, 0, (size_t)FB_CHUNK * 4, st));
  HIP_OK(hipMemsetAsync(G.cur, 0xFF, (size_t)MIQP_POOL_MAX * fl, st));
  HIP_OK(hipMemcpyAsync(G.cur, fix, (size_t)n * fl, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(G.act, act.data(), MIQP_POOL_MAX * sizeof(int), hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(Q.state, state0, sizeof state0, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemsetAsync(G.cnt, 0, MIQP_POOL_MAX * sizeof(int), st)); HIP_OK(hipMemsetAsync(G.cur_obj, 0, MIQP_POOL_MAX * sizeof(double), st));
  HIP_OK(hipMemsetAsync(G.ent_inst, 0, MIQP_POOL_MAX * sizeof(int), st)); HIP_OK(hipMemsetAsync(G.off, 0, (MIQP_POOL_MAX + 1) * sizeof(int), st));
  HIP_OK(hipMemsetD32Async((hipDeviceptr_t)G.ent_fam, fam, MIQP_POOL_MAX, st));
  const DevBuf Bp = fixed_chain_settings(B);
  PoolExploreArgs E;
  PoolImproveArgs& A = E.A;
  A.cur = G.cur; A.cur_obj = G.cur_obj; A.act = G.act; A.cnt = G.cnt; A.moves = G.moves; A.words = G.words; A.res = R.res; A.pool_fix = B.pool_fix;
  A.ent_inst = G.ent_inst; A.ent_fam = G.ent_fam; A.off = G.off; A.batch_inst = B.batch_inst;
  A.dims = dims; A.fixlen = (int)fl; A.m = K;   // (every place of the pool is an entry of the kernels: a free one is not expanded and has no jumps)
  E.L = L; E.sig = Q.sig; E.state = Q.state; E.out = Q.out; E.obj0 = obj0; E.max_rel = max_rel; E.pass = 0;
  E.csig = distinct ? Q.csig.p : nullptr; E.lab = settled ? W.cur.p : distinct ? Q.lab.p : nullptr;
  E.has_sig = Q.has_sig; E.fin = settled ? W.last.p : nullptr; E.solves = settled ? W.solves.p : nullptr;
  PoolSettleTally tally;   // (the settled call's: the solves of its settle rounds and their iterations)
  // `total` neighbours of a pass through the chain, a chunk at a time, as the climb sends them (no segments, the trajectories written over)
  auto solve_nodes = [&](int total) -> bool {
    for (int c0 = 0; c0 < total; c0 += FB_CHUNK) {
      const int bc = std::min(FB_CHUNK, total - c0);
      hipLaunchKernelGGL(pool_neighbour_kernel, dim3((bc + 3) / 4), dim3(256), 0, st, A, c0, bc, 0);
      HIP_OK(hipGetLastError());
      if (!fixed_chunk(X, Bp, Y, call.dev(), 1, FixedChunk{bc, c0, R.res + c0, R.Z})) return false;
      if (distinct && !pool_label_chunk(X, Y, 1, bc, R.res + c0, R.Z, Q.lab + (size_t)c0 * fl)) return false;   // (per chunk: the next one writes over R.Z)
    }
    return true;
  };
  // behind a pass (admit: not in front of the first one): the jumps of the next one, and what the host needs of both
  std::vector<int> cnt(MIQP_POOL_MAX); int state[4] = {n, 0, 0, 0}; std::vector<miqp_pool_explore_c> rec(MIQP_POOL_MAX);
  auto finish_pass = [&](bool admit) -> bool {
    if (admit) hipLaunchKernelGGL(M.admit, dim3(1), dim3(64), admit_lds, st, E, (int)PoolImproveDev::NB_MAX);
    hipLaunchKernelGGL(pool_jumps_kernel, dim3(K), dim3(64), jump_lds, st, E);
    hipLaunchKernelGGL(pool_offsets_kernel, dim3(1), dim3(256), 0, st, A);
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(X.ev1, st));
    HIP_OK(hipMemcpyAsync(cnt.data(), G.cnt, MIQP_POOL_MAX * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(state, Q.state, sizeof state, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(rec.data(), Q.out, MIQP_POOL_MAX * sizeof(miqp_pool_explore_c), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st)); HIP_OK(hipGetLastError());
    float ms = 0.0f; (void)hipEventElapsedTime(&ms, X.ev0, X.ev1); O.dev_ms += ms;
    return true;
  };
  // the settled call, behind a pass's chain and labels: the candidates, the live list of those whose labels moved, their rounds from the second on
  auto settle_pass = [&](int total) -> bool {
    const PoolSettleArgs S = pool_settle_args(W, B, Y, total);
    hipLaunchKernelGGL(pool_settle_pick_kernel, dim3(total), dim3(64), 2 * fl, st, E, S, (const signed char*)Q.lab, (int)PoolImproveDev::NB_MAX);
    HIP_OK(hipGetLastError());
    int live = 0;
    return pool_settle_compact(X, S, live, tally) && pool_settle_rounds(call, Bp, S, R.Z, 2, live, tally);
  };
  HIP_OK(hipEventRecord(X.ev0, st));
  if (settled) {   // pass 0: the kept entries' own records to their fixed points, the signatures of both kinds
    if (!pool_settle_records(call, Bp, pool_settle_args(W, B, Y, n), R.Z, G.cur, true, tally)) return false;
  } else if (distinct) {   // pass 0, as in the climb: the kept entries' own records through the chain, their labels, the signatures of those
    hipLaunchKernelGGL(pool_neighbour_kernel, dim3((n + 3) / 4), dim3(256), 0, st, A, 0, n, 1);
    HIP_OK(hipGetLastError());
    if (!fixed_chunk(X, Bp, Y, call.dev(), 1, FixedChunk{n, 0, R.res, R.Z}) || !pool_label_chunk(X, Y, 1, n, R.res, R.Z, Q.lab)) return false;
  }
  if (distinct) { hipLaunchKernelGGL(pool_pass0_kernel, dim3(1), dim3(64), 2 * fl, st, E, settled ? 1 : 0); HIP_OK(hipGetLastError()); }
  if (!finish_pass(false)) return false;
  if (distinct && !settled) { O.neighbours += n; O.iterations += state[2]; }
  int have = n;
  for (;;) {
    long total = 0;
    for (int k = 0; k < K; ++k) { if (cnt[k] < 0 || cnt[k] > POOL_MOVES_MAX) { std::fprintf(stderr, "[miqp_gpu] %s: jump count %d of entry %d\n", name, cnt[k], k); return false; } total += cnt[k]; }
    if (total == 0 || total > PoolImproveDev::NB_MAX || O.passes == max_passes || have >= K) break;
    E.pass = O.passes + 1;
    HIP_OK(hipEventRecord(X.ev0, st));
    if (!solve_nodes((int)total) || (settled && !settle_pass((int)total)) || !finish_pass(true)) return false;
    if (state[0] != have + state[1] || state[1] < 0 || state[0] > K) { std::fprintf(stderr, "[miqp_gpu] %s: %d entries behind %d, %d admitted\n", name, state[0], have, state[1]); return false; }
    O.passes++; O.neighbours += total; O.iterations += state[2];
    for (int k = 0; k < state[1]; ++k) O.added.push_back(rec[k]);
    have = state[0];
    O.still_adding = state[1] > 0 && O.passes == max_passes;
    if (state[1] == 0) break;
  }
  O.neighbours += tally.solves; O.iterations += tally.iterations;
  O.fix.resize((size_t)have * fl); O.obj.resize(have);
  HIP_OK(hipMemcpy(O.fix.data(), G.cur, (size_t)have * fl, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(O.obj.data(), G.cur_obj, (size_t)have * sizeof(double), hipMemcpyDeviceToHost));
  return true;
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

}  // extern "C"

namespace {

// the three explore entries: what they refuse, the run, what the handle keeps
int pool_explore_entry(miqp_solver_t* s, const char* name, int mode, int max_passes, double max_rel, miqp_pool_explore_c* out, int cap) {
  if (s) s->err.clear();   // (miqp_solver_last_error speaks of this call from here on)
  if (!s || !s->has_inst || !out || cap < 0 || max_rel != max_rel) return -1;
  if (s->pool_fam < 1 || s->pool_fam >= POOL_FAM_TIMING || !(s->pool_fam & (POOL_FAM_OBSTACLE | POOL_FAM_CAR_CAR))) return -2;
  if (max_passes < 1 || max_passes > POOL_EXPLORE_PASSES_MAX) return -2;
  const int n = miqp_solver_pool_count(s), K = std::min(s->pool_cap, MIQP_POOL_MAX);
  if (n == 0 || n >= K) return 0;   // (nothing to jump from, or no free place: no device is touched)
  if (cap < K - n) return -2;
  { int ndev = 0; if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return -3; }
  miqp_solver_t* one[1] = {s};
  BatchShape bs = batch_layout(one, 1);
  if (!bs.ok || bs.Y.fixlen != s->pool_fixlen || s->pool_fix.size() < (size_t)n * bs.Y.fixlen || s->pool_obj.size() < (size_t)n) return -1;
  const Layout& Y = bs.Y; const size_t fl = (size_t)Y.fixlen;
  const double t_call = wall_s();
  FixedCall call;
  if (call.open(one, 1, Y) != 0) return -3;
  PoolExploreOut O;
  if (!pool_explore_run(call, name, mode, s->pool_fam, s->inst.L, s->pool_fix.data(), n, K, s->pool_obj[0], max_rel, max_passes, O)) {
    (void)hipStreamSynchronize(call.X->stream); if (!O.err.empty()) s->err = O.err; return -3;
  }
  const int added = (int)O.added.size();
  if ((int)O.obj.size() != n + added || n + added > K) return -3;
  // the old entries stay as the handle holds them; the added ones go behind them
  s->pool_fix.resize((size_t)n * fl); s->pool_obj.resize(n);
  s->pool_fix.insert(s->pool_fix.end(), O.fix.begin() + (size_t)n * fl, O.fix.end());
  s->pool_obj.insert(s->pool_obj.end(), O.obj.begin() + n, O.obj.end());
  s->pool_n = n + added;
  for (int k = 0; k < added; ++k) out[k] = O.added[k];
  s->pr_n = 0; std::vector<char>().swap(s->pr_ok); std::vector<signed char>().swap(s->pr_fix); std::vector<double>().swap(s->pr_Z);
  s->timing[0] = wall_s() - t_call; s->timing[1] = O.dev_ms * 1e-3; s->timing[2] = O.passes; s->timing[3] = (double)O.neighbours; s->timing[4] = (double)O.iterations; s->timing[5] = O.still_adding ? 1 : 0;
  if (O.still_adding && n + added < K) {
    char msg[200]; std::snprintf(msg, sizeof msg, "%s: the last of %d passes still added an entry and places are free; more passes may fill them", name, max_passes);
    s->err = msg;
  }
  return added;
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

}  // extern "C"

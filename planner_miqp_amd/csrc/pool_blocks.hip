// pool_blocks.hip - the wavefront-level steps the solution-pool kernels are built from, each ONCE: solution_pool.hip, pool_improve.hip, pool_label.hip,
// pool_settle.hip and pool_explore.hip call them, and fixed_collect_kernel (fixed_chain.hip) takes its minimum from here.  DESIGN.md 6e.
//
// A RECORD is a fix record of `chunks` 16-byte pieces (fixlen >> 4), in HBM or in LDS; its SIGNATURE under a filter is a block of the same size.
// Every function below that takes `lane` is called by a whole wavefront of 64 with uniform arguments, one record per wavefront; the two that hold a
// barrier (pool_sign, pool_tile_scan) by every thread of the workgroup.  No atomics, no scratch; records move as 16-byte loads and stores.
//   pool_stage            record -> record, optionally with a MOVE patched in on the way and a signature block reset to ~0 beside it
//   pool_sign             the signature of a record in LDS, one lane per site, in a loop when there are more sites than lanes
//   pool_cmp, pool_known, pool_records_differ      bytes of two records in order; a signature among the first n kept; any difference at all
//   pool_entry_of         the entry a neighbour number belongs to, by binary search in the scan of the move counts
//   pool_wave_argmin      (objective, index) of the wavefront, a tie to the lower index
//   pool_wave_scan, pool_tile_scan, pool_count_scan_emit   the 64-wide inclusive scan; a workgroup's scan in tiles of 256; per-unit counts ->
//                         numbered moves in the move table
//   pool_is_candidate     which neighbours of a pass the explore may admit
// The definitions the host restates (pool_site_signature, pool_within_cap) are __host__ __device__ and serve both sides.
#pragma once

namespace {

constexpr int POOL_MOVES_MAX = 512;   // moves per record (miqp_gpu_pool_moves_max): LNS_MAX
constexpr double POOL_ADMIT_NONE = 1e308;   // in the staged objectives of the explore: not feasible, beyond the cap, or visited

// (first, stride, count, value): the bytes d[first + k * stride], k < count, take `value` (pool_improve.hip); in the move table as an int4
struct PoolMove { int first, stride, count, value; };

// ---------------------------------------------------------------------------------------------------------------- sites and signatures
constexpr int POOL_FAM_REGION = 1, POOL_FAM_ENVIRONMENT = 2, POOL_FAM_OBSTACLE = 4, POOL_FAM_CAR_CAR = 8, POOL_FAM_TIMING = 16, POOL_FAM_ALL = 31;

// the sites of a decision record - one disjunction followed along the horizon: the byte of step i of a site lies at first + i * step
struct PoolDims { int C, N, O, NP; };
struct PoolSite { int first, step, family; };
__host__ __device__ inline int pool_declen(const PoolDims& d) { return d.C * d.N * 6 + d.C * d.O * d.N * 5 + d.NP * d.N * 4; }
__host__ __device__ inline int pool_sites(const PoolDims& d) { return d.C * 6 + d.C * d.O * 5 + d.NP * 4; }
__host__ __device__ inline PoolSite pool_site(const PoolDims& d, int s) {
  const int f_env = d.C * d.N, f_obs = f_env + d.C * d.N * 5, f_c2c = f_obs + d.C * d.O * d.N * 5;
  if (s < d.C) return PoolSite{s * d.N, 1, POOL_FAM_REGION};
  s -= d.C;
  if (s < d.C * 5) return PoolSite{f_env + (s / 5) * d.N * 5 + s % 5, 5, POOL_FAM_ENVIRONMENT};
  s -= d.C * 5;
  if (s < d.C * d.O * 5) return PoolSite{f_obs + (s / 5) * d.N * 5 + s % 5, 5, POOL_FAM_OBSTACLE};
  s -= d.C * d.O * 5;
  return PoolSite{f_c2c + (s >> 2) * d.N * 4 + (s & 3), 4, POOL_FAM_CAR_CAR};
}
// the signature bytes of ONE site (sg is -1 there before): with the timing bit its bytes as they are, step 0 included; without it the alternatives of
// steps 1 .. N - 1 in their order, undecided bytes skipped, repeats collapsed, left-packed from step 1 - of a region byte the possible-region index
// (byte >> 2: the low two bits are the half-plane or slow alternative)
__host__ __device__ inline void pool_site_signature(const PoolDims& d, int fam, int s, const signed char* rec, signed char* sg) {
  const PoolSite t = pool_site(d, s);
  if (!(fam & t.family)) return;
  if (fam & POOL_FAM_TIMING) { for (int i = 0; i < d.N; ++i) sg[t.first + i * t.step] = rec[t.first + i * t.step]; return; }
  int last = -1, w = 0;
  for (int i = 1; i < d.N; ++i) {
    int v = rec[t.first + i * t.step];
    if (v < 0) continue;
    if (t.family == POOL_FAM_REGION) v >>= 2;
    if (v != last) { w++; sg[t.first + w * t.step] = (signed char)v; last = v; }
  }
}

// the signature of the record at rec4 into sg4 (both in LDS, sg4 reset to ~0 by the staging in front); both barriers are the block's
__device__ inline void pool_sign(const PoolDims& d, int fam, const uint4* rec4, uint4* sg4, int lane) {
  const int nsites = pool_sites(d);
  __syncthreads();
  for (int s = lane; s < nsites; s += 64) pool_site_signature(d, fam, s, (const signed char*)rec4, (signed char*)sg4);
  __syncthreads();
}

// ---------------------------------------------------------------------------------------------------------------- records
__device__ inline void pool_patch_byte(uint4& v, int p, int val) {   // byte p (0 .. 15) of v, without indexing the registers
  const unsigned sh = (unsigned)(p & 3) * 8u, keep = ~(0xFFu << sh), bits = ((unsigned)val & 0xFFu) << sh;
  const int w = p >> 2;
  v.x = w == 0 ? (v.x & keep) | bits : v.x; v.y = w == 1 ? (v.y & keep) | bits : v.y;
  v.z = w == 2 ? (v.z & keep) | bits : v.z; v.w = w == 3 ? (v.w & keep) | bits : v.w;
}

// src -> dst; sig (may be NULL): a block reset to ~0 beside it; mv: a move (x, y, z, w) = (first, stride, count, value) patched into the pieces on
// their way (count 0: none) - a byte of the move outside the piece in hand is not this piece's.  A lane has one or two pieces of a record: the
// loop stays as written (unrolled sixteen times it holds 64 registers for pieces that are not there)
__device__ inline void pool_stage(uint4* dst, const uint4* src, int chunks, int lane, uint4* sig = nullptr, const int4 mv = make_int4(0, 1, 0, 0)) {
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
  for (int c = lane; c < chunks; c += 64) {
    uint4 v = src[c];
    for (int k = 0; k < mv.z; ++k) { const int p = mv.x + k * mv.y - c * 16; if ((unsigned)p < 16u) pool_patch_byte(v, p, mv.w); }
    dst[c] = v;
    if (sig) sig[c] = make_uint4(~0u, ~0u, ~0u, ~0u);
  }
}

// bytes of two records, as unsigned: < 0, 0, > 0
__device__ inline int pool_cmp(const uint4* a, const uint4* b, int chunks, int lane) {
  for (int c0 = 0; c0 < chunks; c0 += 64) {
    const int c = c0 + lane; int sign = 0;
    if (c < chunks) {
      const uint4 x = a[c], y = b[c];
      if (x.x != y.x || x.y != y.y || x.z != y.z || x.w != y.w) {
        const unsigned char* p = (const unsigned char*)&x; const unsigned char* q = (const unsigned char*)&y;
        for (int t = 15; t >= 0; --t) if (p[t] != q[t]) sign = p[t] < q[t] ? -1 : 1;
      }
    }
    const unsigned long long m = __ballot(sign != 0);
    if (m) return __shfl(sign, __ffsll((long long)m) - 1, 64);
  }
  return 0;
}

// sg is one of the first n signatures of sigs (has, may be NULL: only the places it marks count)
__device__ inline bool pool_known(const uint4* sg, const uint4* sigs, int n, int chunks, int lane, const int* has = nullptr) {
  bool known = false;
  for (int j = 0; j < n && !known; ++j) known = (!has || has[j]) && pool_cmp(sg, sigs + (size_t)j * chunks, chunks, lane) == 0;
  return known;
}

// do two records differ anywhere: 16-byte compares and one ballot
__device__ inline bool pool_records_differ(const uint4* a, const uint4* b, int chunks, int lane) {
  bool diff = false;
  for (int c = lane; c < chunks; c += 64) { const uint4 x = a[c], y = b[c]; diff = diff || x.x != y.x || x.y != y.y || x.z != y.z || x.w != y.w; }
  return __ballot(diff) != 0ull;
}

// ---------------------------------------------------------------------------------------------------------------- numbers of a wavefront
// the entry of neighbour g, 0 <= g < off[m]: the largest e with off[e] <= g (off[0 .. m] ascends, with runs of equal values where entries have no
// moves) - at most 17 probes, the same in every lane
__device__ inline int pool_entry_of(const int* off, int m, int g) {
  int lo = 0, hi = m;   // off[lo] <= g < off[hi]
  while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (off[mid] <= g) lo = mid; else hi = mid; }
  return lo;
}

// the smallest (bo, bi) of the wavefront into every lane; equal objectives: the lower index.  A lane that visits its own indices in ascending
// order and takes only a strictly smaller objective brings the first minimum of its own, so the result is the first minimum of all
__device__ inline void pool_wave_argmin(double& bo, int& bi) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const double oo = __shfl_xor(bo, d, 64); const int oi = __shfl_xor(bi, d, 64);
    if (oo < bo || (oo == bo && oi < bi)) { bo = oo; bi = oi; }
  }
}

// inclusive scan over the 64 lanes
__device__ inline int pool_wave_scan(int x, int lane) {
  for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_up(x, o, 64); if (lane >= o) x += y; }
  return x;
}

// One tile of a scan by ONE workgroup of 256 (every thread calls, with its value c of this tile): a wave scan per wavefront, the four wavefront
// totals through carry[4] in LDS.  Returns base + the values in front of this thread's; base, the total of the tiles before in a register of every
// thread, moves on by the tile's total
__device__ inline int pool_tile_scan(int c, int* carry, int& base) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x = pool_wave_scan(c, lane);
  if (lane == 63) carry[wave] = x;
  __syncthreads();
  int before = 0;
  for (int w = 0; w < 4; ++w) before += w < wave ? carry[w] : 0;
  const int at = base + before + x - c;
  base += carry[0] + carry[1] + carry[2] + carry[3];
  __syncthreads();
  return at;
}

// The moves of one record into its row of the move table: unit(u, emit) calls emit(j, move) for move j of unit u in order and returns their number.
// One lane per unit (in a loop when there are more units than lanes) counts into ucnt[nunits] (LDS), a wave scan numbers the units' moves, the
// lanes write the first POOL_MOVES_MAX of them.  Returns the record's (clamped) count.  The block's record is staged in front of the call
template <class Unit>
__device__ inline int pool_count_scan_emit(int nunits, int* ucnt, int4* out, int lane, Unit unit) {
  for (int u = lane; u < nunits; u += 64) ucnt[u] = unit(u, [](int, const PoolMove&) {});
  __syncthreads();
  int total = 0;   // exclusive scan of the per-unit counts, 64 units at a time
  for (int u0 = 0; u0 < nunits; u0 += 64) {
    const int c = u0 + lane < nunits ? ucnt[u0 + lane] : 0;
    const int x = pool_wave_scan(c, lane);
    if (u0 + lane < nunits) ucnt[u0 + lane] = total + x - c;
    total += __shfl(x, 63, 64);
  }
  __syncthreads();
  for (int u = lane; u < nunits; u += 64) {
    const int off = ucnt[u];
    if (off >= POOL_MOVES_MAX) continue;
    (void)unit(u, [&](int j, const PoolMove& mv) { if (off + j < POOL_MOVES_MAX) out[off + j] = make_int4(mv.first, mv.stride, mv.count, mv.value); });
  }
  return min(total, POOL_MOVES_MAX);
}

// ---------------------------------------------------------------------------------------------------------------- the explore's candidates
// "within the cost cap": objective - obj0 <= max_rel |obj0|, every operation rounded on its own on both sides so that host code can restate it
__host__ __device__ inline bool pool_within_cap(double obj0, double obj, double max_rel) {
  if (max_rel < 0.0) return true;
#ifdef __HIP_DEVICE_COMPILE__
  return __dsub_rn(obj, obj0) <= __dmul_rn(max_rel, fabs(obj0));
#else
  volatile double over = obj - obj0; volatile double room = max_rel * std::fabs(obj0);
  return over <= room;
#endif
}

// neighbour jm of place e is a candidate of the pass: feasible, an objective the staging can hold, within the cap, a move of the table, and its
// parent one of the n0 entries the pass began with
__device__ inline bool pool_is_candidate(const miqp_fixed_result_c& r, double obj0, double max_rel, int jm, int e, int n0) {
  return r.status == 0 && r.objective < POOL_ADMIT_NONE && pool_within_cap(obj0, r.objective, max_rel) && jm >= 0 && jm < POOL_MOVES_MAX && e < n0;
}

}  // namespace

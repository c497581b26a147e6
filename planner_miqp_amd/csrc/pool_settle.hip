// pool_settle.hip - decision records solved and re-labelled on the device until their labels stay (miqp_solver_settle_decisions), and the rounds
// the settled explore runs for the candidates of a pass (pool_explore.hip: miqp_solver_pool_explore_settled).  DESIGN.md 6j.
//
// One labelling of a solution is not where the refinement ends (miqp_solver_pool_solve: pool_refine): a record solved under the labels of its own
// solution can slide to a neighbouring solution, whose labels differ again.  SETTLING a record is that iteration for one record: r0 its bytes,
// completed to a fix record as miqp_solver_solve_decisions completes them; for p = 1 .. POOL_PASSES: solve r(p - 1) through the fixed chain, stop
// when the answer is not feasible; label the solution (pool_label_kernel) to c(p); stop - SETTLED - when c(p) is r(p - 1) byte for byte over the
// whole record; else r(p) = c(p).  A record still moving after POOL_PASSES solves keeps the labels of its last solve, as the refinement does.  The
// chain answers a record bit for bit whatever its place and its neighbours, so the iteration per record is the refinement's per entry.
//
// A ROUND is one p for every record that still moves (the LIVE list), in chunks of FB_CHUNK, all on the solver stream:
//   pool_settle_gather_kernel   one wavefront per slot of the chunk: live record -> slot of pool_fix, in 16-byte loads and stores; batch_inst
//   fixed_chunk, pool_label_kernel   as they are
//   pool_settle_step_kernel     one wavefront per slot: the labelled record against the record it was solved with (16-byte compares, one ballot);
//                               the labels into the record's own place, the result, the solve count and the moved flag to the record's OWN index -
//                               the live list is compacted, so this is a scatter by original index
//   pool_settle_compact_kernel  behind the round's last chunk, ONE workgroup: the exclusive scan of the moved flags in record order, tiles of 256
//                               (pool_tile_scan of pool_blocks.hip, as pool_offsets_kernel) - writes the live list of the next round, ascending
//                               by original index whatever the order of arrival, and sums the round's iterations
// The host waits once per round and reads two words: the live count that sizes the next round, and the iterations.  A round without a live record is
// not launched.  Owner computes: no atomics, no wavefront waits on another, no scratch.
// Device memory, cached per device, grown and not shrunk: n x (fixlen + 56) bytes for the n records of a call (labels, last result, solve count,
// moved flag, iterations of the round and of all rounds, instance, live list) and FB_CHUNK x (fixlen + 32) for a chunk's labels and results; the chunk's trajectory rows are the climb's.
#pragma once

namespace {

struct PoolSettleArgs {
  signed char* cur;                 // [n] the labels record k is solved with next - at the end: the labels its last solve ran with
  miqp_fixed_result_c* last;        // [n] the answer of record k's last solve
  int* solves;                      // [n] solves of record k so far; -POOL_PASSES: still moving behind the last one
  int* moved;                       // [n] record k is live in the next round
  int* round_it;                    // [n] iterations of record k's solve in this round (0 when it was not live)
  int* acc_it;                      // [n] iterations of record k's solves of the rounds so far: the compaction sums a round over the whole call, the explore of many handles sums these per handle
  int* inst;                        // [n] the instance of record k in the call: its handle's index
  int* live;                        // [n] the live list: original indices, ascending
  int* state;                       // [0] live records of the next round, [1] iterations of the round
  signed char* pool_fix; int* batch_inst;   // the chain's fix records and instances: slot k of the chunk
  signed char* lab;                 // [FB_CHUNK] the labelled records of the chunk
  miqp_fixed_result_c* res;         // [FB_CHUNK] the results of the chunk
  int fixlen, n, round;
};

// a result record as two 16-byte moves (one lane calls)
static_assert(sizeof(miqp_fixed_result_c) == 32, "a result record is two 16-byte pieces");
__device__ inline void pool_settle_copy_result(miqp_fixed_result_c* dst, const miqp_fixed_result_c* src) {
  const uint4 a = ((const uint4*)src)[0], b = ((const uint4*)src)[1];
  ((uint4*)dst)[0] = a; ((uint4*)dst)[1] = b;
}

__global__ __launch_bounds__(256) void pool_settle_gather_kernel(const PoolSettleArgs S, int c0, int bc) {
  const int lane = threadIdx.x & 63, slot = blockIdx.x * 4 + (threadIdx.x >> 6), chunks = S.fixlen >> 4;
  if (slot >= bc || c0 + slot >= S.n) return;
  const int k = S.live[c0 + slot];
  if ((unsigned)k >= (unsigned)S.n) return;
  pool_stage((uint4*)S.pool_fix + (size_t)slot * chunks, (const uint4*)S.cur + (size_t)k * chunks, chunks, lane);
  if (lane == 0) S.batch_inst[slot] = S.inst[k];
}

__global__ __launch_bounds__(256) void pool_settle_step_kernel(const PoolSettleArgs S, int c0, int bc) {
  const int lane = threadIdx.x & 63, slot = blockIdx.x * 4 + (threadIdx.x >> 6), chunks = S.fixlen >> 4;
  if (slot >= bc || c0 + slot >= S.n) return;
  const int k = S.live[c0 + slot];
  if ((unsigned)k >= (unsigned)S.n) return;
  const int status = S.res[slot].status;
  const uint4* lab = (const uint4*)S.lab + (size_t)slot * chunks;
  const bool moving = status == 0 && pool_records_differ(lab, (const uint4*)S.pool_fix + (size_t)slot * chunks, chunks, lane);   // (the slot is the wavefront's: every lane is here)
  const bool go = moving && S.round < POOL_PASSES;
  if (go) pool_stage((uint4*)S.cur + (size_t)k * chunks, lab, chunks, lane);
  if (lane == 0) { pool_settle_copy_result(S.last + k, S.res + slot); S.solves[k] = moving && !go ? -S.round : S.round; S.moved[k] = go ? 1 : 0; S.round_it[k] = S.res[slot].iterations; S.acc_it[k] += S.res[slot].iterations; }
}

__global__ __launch_bounds__(256) void pool_settle_compact_kernel(const PoolSettleArgs S) {
  __shared__ int carry[4], itw[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int base = 0, it = 0;
  for (int t0 = 0; t0 < S.n; t0 += 256) {   // (S.n is uniform: every thread meets every barrier)
    const int k = t0 + tid;
    const int f = k < S.n && S.moved[k] ? 1 : 0;
    if (k < S.n) { it += S.round_it[k]; S.round_it[k] = 0; }
    const int at = pool_tile_scan(f, carry, base);
    if (f) S.live[at] = k;   // (at most k flags in front of record k: the place is below S.n)
  }
  for (int d = 32; d >= 1; d >>= 1) it += __shfl_xor(it, d, 64);
  if (lane == 0) itw[wave] = it;
  __syncthreads();
  if (tid == 0) { S.state[0] = base; S.state[1] = itw[0] + itw[1] + itw[2] + itw[3]; }
}

// (DevArr: grown, not shrunk; the chunk's labels exactly FB_CHUNK records)
struct PoolSettleDev {
  DevArr<signed char> cur, lab; DevArr<miqp_fixed_result_c> last, res; DevArr<int> solves, moved, round_it, acc_it, inst, live, state;
  bool ensure(size_t n, size_t fl) {
    return state.need(2) && res.need(FB_CHUNK) && last.need(n, 1024) && solves.need(n, 1024) && moved.need(n, 1024) && round_it.need(n, 1024) && acc_it.need(n, 1024) && inst.need(n, 1024) && live.need(n, 1024) &&
           cur.need(n * fl, 1024 * fl) && lab.need((size_t)FB_CHUNK * fl);
  }
};

// the kernel arguments of a call over n records (n <= the capacity `ensure` was asked for)
PoolSettleArgs pool_settle_args(const PoolSettleDev& Q, const DevBuf& B, const Layout& Y, int n) {
  PoolSettleArgs S;
  S.cur = Q.cur; S.last = Q.last; S.solves = Q.solves; S.moved = Q.moved; S.round_it = Q.round_it; S.acc_it = Q.acc_it; S.inst = Q.inst; S.live = Q.live; S.state = Q.state;
  S.pool_fix = B.pool_fix; S.batch_inst = B.batch_inst; S.lab = Q.lab; S.res = Q.res; S.fixlen = Y.fixlen; S.n = n; S.round = 0;
  return S;
}

struct PoolSettleTally { long solves = 0, iterations = 0; int groups = 0; };

// the live list behind a round (or behind the explore's pick kernel, which is round 1 of its candidates): the host reads its length.  false: HIP error
bool pool_settle_compact(DevCtx& X, const PoolSettleArgs& S, int& live, PoolSettleTally& T) {
  int state[2] = {0, 0};
  hipLaunchKernelGGL(pool_settle_compact_kernel, dim3(1), dim3(256), 0, X.stream, S);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(state, S.state, sizeof state, hipMemcpyDeviceToHost, X.stream));
  HIP_OK(hipStreamSynchronize(X.stream)); HIP_OK(hipGetLastError());
  if (state[0] < 0 || state[0] > S.n || state[1] < 0) { std::fprintf(stderr, "[miqp_gpu] settle: %d live records of %d\n", state[0], S.n); return false; }
  live = state[0]; T.iterations += state[1];
  return true;
}

// Rounds `first` .. POOL_PASSES over the `live` records of the list in S.live, whose instances are among the call's.  Bp: fixed_chain_settings; Z: the
// rows of one chunk.  A caller that wants the words of a round before the next one writes over them (the carry: the answers of round 1) stops behind
// round `last` and goes on from there with the live count it received.  false: HIP error
bool pool_settle_rounds(const FixedCall& call, const DevBuf& Bp, PoolSettleArgs S, double* Z, int first, int& live, PoolSettleTally& T, int last = POOL_PASSES) {
  DevCtx& X = *call.X; const Layout& Y = call.Y; hipStream_t st = X.stream;
  for (int p = first; p <= last && live > 0; ++p) {
    S.round = p;
    for (int c0 = 0; c0 < live; c0 += FB_CHUNK) {
      const int bc = std::min(FB_CHUNK, live - c0);
      hipLaunchKernelGGL(pool_settle_gather_kernel, dim3((bc + 3) / 4), dim3(256), 0, st, S, c0, bc);
      HIP_OK(hipGetLastError());
      if (!fixed_chunk(X, Bp, Y, call.dev(), call.n, FixedChunk{bc, c0, S.res, Z})) return false;
      if (!pool_label_chunk(X, Y, call.n, bc, S.res, Z, S.lab)) return false;
      hipLaunchKernelGGL(pool_settle_step_kernel, dim3((bc + 3) / 4), dim3(256), 0, st, S, c0, bc);
      HIP_OK(hipGetLastError());
      T.groups++;
    }
    T.solves += live;
    if (!pool_settle_compact(X, S, live, T)) return false;
  }
  return true;
}

// n records (fix bytes on the host) settled from round 1: uploads them, resets the per-record words, runs the rounds.  inst (host; NULL: all of
// instance 0): the instance of every record.  false: HIP error
bool pool_settle_records(const FixedCall& call, const DevBuf& Bp, const PoolSettleArgs& S, double* Z, const signed char* fix, const int* inst, PoolSettleTally& T) {
  hipStream_t st = call.X->stream; const size_t fl = (size_t)call.Y.fixlen;
  std::vector<int> ident(S.n); for (int k = 0; k < S.n; ++k) ident[k] = k;
  HIP_OK(hipMemcpyAsync(S.cur, fix, (size_t)S.n * fl, hipMemcpyHostToDevice, st));
  if (inst) HIP_OK(hipMemcpyAsync(S.inst, inst, (size_t)S.n * sizeof(int), hipMemcpyHostToDevice, st));
  else HIP_OK(hipMemsetAsync(S.inst, 0, (size_t)S.n * sizeof(int), st));
  HIP_OK(hipMemcpyAsync(S.live, ident.data(), (size_t)S.n * sizeof(int), hipMemcpyHostToDevice, st));
  HIP_OK(hipMemsetAsync(S.round_it, 0, (size_t)S.n * sizeof(int), st)); HIP_OK(hipMemsetAsync(S.moved, 0, (size_t)S.n * sizeof(int), st));
  HIP_OK(hipMemsetAsync(S.solves, 0, (size_t)S.n * sizeof(int), st)); HIP_OK(hipMemsetAsync(S.acc_it, 0, (size_t)S.n * sizeof(int), st));
  HIP_OK(hipStreamSynchronize(st));   // (ident is a local)
  int live = S.n;
  return pool_settle_rounds(call, Bp, S, Z, 1, live, T);
}

}  // namespace

extern "C" {

int miqp_gpu_pool_settle_passes(void) { return POOL_PASSES; }

int miqp_solver_settle_decisions(miqp_solver_t* s, const signed char* decisions, int n, miqp_fixed_result_c* out, signed char* settled, int* solves, int* best) {
  if (s) { s->drop_fixed_batch(); s->err.clear(); }
  if (!s || !s->has_inst || !decisions || !out || !settled || !solves || n <= 0) return -1;
  if (n > FB_CAP) return -5;
  const double t_call = wall_s();
  if (best) *best = -1;
  fixed_refuse(out, n);
  miqp_solver_t* one[1] = {s};
  BatchShape bs = batch_layout(one, 1);
  if (!bs.ok) return -2;
  const Layout& Y = bs.Y;
  const size_t fl = (size_t)Y.fixlen, D = (size_t)Y.f_c2n;
  std::memset(settled, 0xFF, (size_t)n * D);
  std::fill(solves, solves + n, 0);
  std::vector<double> Dt(Y.dstride); std::vector<int> T(Y.istride);
  compile_instance(s->inst, Y, Dt.data(), T.data());
  std::vector<int> where; where.reserve(n);
  for (int k = 0; k < n; ++k) if (decisions_in_range(s->inst, Y, T.data(), decisions + (size_t)k * D)) where.push_back(k);
  const int m = (int)where.size();
  if (m == 0) return 0;   // (nothing to run: no device is touched)
  if (!pool_label_fits(Y, "miqp_solver_settle_decisions", s->err)) return -3;
  const double setup_s = wall_s() - t_call;
  FixedCall call;
  if (call.open(one, 1, Y) != 0) return -3;
  DevCtx& X = *call.X;
  PoolSettleDev& Q = call_dev<PoolSettleDev>(X.device); PoolImproveDev& R = call_dev<PoolImproveDev>(X.device);
  std::vector<signed char> fix((size_t)m * fl, (signed char)-1);
  for (int c = 0; c < m; ++c) std::memcpy(fix.data() + (size_t)c * fl, decisions + (size_t)where[c] * D, D);
  std::vector<miqp_fixed_result_c> last(m); std::vector<int> cnt(m);
  PoolSettleTally tally; float dev_ms = 0.0f;
  const auto run = [&]() -> bool {
    if (!Q.ensure((size_t)m, fl) || !R.ensure((size_t)Y.N * Y.nz) || !pool_label_set_lds(Y)) return false;
    const DevBuf Bp = fixed_chain_settings(X.B);
    const PoolSettleArgs S = pool_settle_args(Q, X.B, Y, m);
    HIP_OK(hipEventRecord(X.ev0, X.stream));
    if (!pool_settle_records(call, Bp, S, R.Z, fix.data(), nullptr, tally)) return false;
    HIP_OK(hipEventRecord(X.ev1, X.stream));
    HIP_OK(hipMemcpyAsync(last.data(), Q.last, (size_t)m * sizeof(miqp_fixed_result_c), hipMemcpyDeviceToHost, X.stream));
    HIP_OK(hipMemcpyAsync(cnt.data(), Q.solves, (size_t)m * sizeof(int), hipMemcpyDeviceToHost, X.stream));
    HIP_OK(hipMemcpyAsync(fix.data(), Q.cur, (size_t)m * fl, hipMemcpyDeviceToHost, X.stream));
    HIP_OK(hipStreamSynchronize(X.stream)); HIP_OK(hipGetLastError());
    (void)hipEventElapsedTime(&dev_ms, X.ev0, X.ev1);
    return true;
  };
  if (!run()) { (void)hipStreamSynchronize(X.stream); return -3; }
  int b = -1, still = 0;
  for (int c = 0; c < m; ++c) {
    const int k = where[c];
    out[k] = last[c]; solves[k] = cnt[c];
    if (cnt[c] < 0) still++;
    if (last[c].status != 0) continue;
    std::memcpy(settled + (size_t)k * D, fix.data() + (size_t)c * fl, D);
    if (b < 0 || last[c].objective < last[b].objective) b = c;   // (ascending: a tie keeps the lower index)
  }
  if (best) *best = b < 0 ? -1 : where[b];
  if (still) {
    char msg[200]; std::snprintf(msg, sizeof msg, "miqp_solver_settle_decisions: the labels of %d records still moved after %d solves; their rows are the labels of the last one", still, POOL_PASSES);
    s->err = msg; std::fprintf(stderr, "[miqp_gpu] %s\n", msg);
  }
  s->setup[0] = setup_s;
  s->timing[0] = wall_s() - t_call; s->timing[1] = dev_ms * 1e-3; s->timing[2] = tally.groups; s->timing[3] = (double)tally.solves; s->timing[4] = (double)tally.iterations; s->timing[5] = still ? 1 : 0;
  return 0;
}

}  // extern "C"

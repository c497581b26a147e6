// solution_pool.hip - the K best distinct integer solutions of a solve (miqp_solver_set_pool, _pool_count, _pool_found, _pool_solve, _pool_solve_multi,
// _pool_record).
//
// Counterpart of the CPLEX solution pool (IloCplex::getSolnPoolNsolns, getObjValue(i), getValues(x, i)), which a user of the reference reaches through the
// IloCplex its wrapper owns; the reference source itself has no call site for it.  A solve returns its incumbent; every other integer-feasible leaf the
// branch and bound reaches is dropped at the end of its round.  A planner wants those leaves - the second- and third-best manoeuvre is the fallback when the
// best one fails a downstream check - and the search enumerates them for free: eval_kernel writes every integer-feasible node of a round as a finished
// candidate (completed fix record in batch_comp, key, instance and objective in batch_candkey, batch_candinst, batch_obj), select_kernel then keeps the round's
// winner.  Every incumbent is such a candidate: inc_fix has one writer, select_kernel's copy of the winning candidate, and the warm-start roots, the
// local-search leaves and the rounding probes are nodes of a round's batch like any other.
//
// Capture (only when a handle of the call asked for a pool - else no buffer, no launch): behind each round's eval_kernel, on the solver stream,
//   pool_compact_kernel  the batch slots with a candidate -> a short list (wave ballot, one atomic append per wavefront)
//   pool_merge_kernel    owner computes: one wavefront per instance in flight walks the list, takes the entries of its own instance and merges them into
//                        the instance's pool in HBM - `capacity` records, sorted, with the objective as found and the record hash beside them.
// No lock, no wavefront waits on another, no scratch; records move as 16-byte loads and stores.
//
// The pool of an instance is a function of the SET of candidates seen, not of their arrival order: it keeps the `capacity` smallest in the order
// (objective as found, record hash, bytes of the record), all distinct.  A record here is the DECISION part of the completed fix record - regions,
// environment pieces, obstacle edges, car/car alternatives; the mask bytes behind it (car/car exclusions, region sets) say how the search got to the leaf,
// not what the leaf decides, and are reset to "none" as in a record built from a RawResults.  The same record found again keeps its smaller objective.
// With the bit-reproducibility of a single solve this makes the pool of a single solve reproducible bit for bit.  Ties of the search itself (the same
// objective to 44 bits: select_kernel then takes the smaller hash of the whole record) could put another record of the same objective in front of the
// incumbent's, or at capacity push it out: pool_read_back puts the incumbent's record first, so entry 0 is the incumbent at every capacity.
//
// Memory: n_inst x stride x (fixlen + 12) + 8 n_inst + 4 batch_alloc + 8 bytes, stride = the largest capacity of the call's handles (n_inst = 51 200 handles
// of two cars x 8 steps, capacity 8: 0.2 GB); with a filter in the call n_inst x stride x fixlen + 4 n_inst more (the signatures, the family sets).
// A rank of a tree split keeps the pool of its own search; pools are not exchanged.
//
// Refinement: pool entries were found at node tolerance; miqp_solver_pool_solve sends them through the fixed chain (fixed_chain.hip) at the tight
// tolerance.  What the caller gets per entry is what miqp_solver_solve_fixed answers for the entry's RawResults record: the call re-labels each record
// with the canonical binaries of its own solution (fill_results / fix_from_results: the first alternative that holds) and solves again until the labels stay.
// Entries that end with the same labels are one solution under several names - the optimum of one record also holds the alternatives of the other, so
// both QPs have the same minimiser - and are merged there, the best found staying (of the one-car helper shape c1n6r16hex the search keeps 4 records,
// all of them the incumbent's trajectory).  The capture cannot see this: it has the decisions of a leaf, not a tight solution.  So a pool can hand out
// fewer than `capacity` solutions although the search saw more distinct ones.
//
// Manoeuvre filter (miqp_solver_set_pool_filter; off by default - then nothing below runs): the near-optimal leaves of ONE manoeuvre differ in
// WHEN a car changes its alternative, and a pool that tells entries apart by every decision byte fills with those timing variants.  With a filter two
// candidates are the same entry when their SIGNATURES agree (pool_signature below: per site - one disjunction followed along the horizon - the
// sequence of alternatives with repeats collapsed, for the selected families), and the pool keeps the smallest member of each class: the `capacity`
// smallest class minima of the set seen.  pool_filter_kernel replaces pool_merge_kernel in a call that has a handle with a filter; the signatures of the
// entries kept lie in a buffer of their own (n_inst x stride x fixlen bytes, only then).  A handle of such a call WITHOUT a filter is merged exactly as
// pool_merge_kernel merges it: its signature is its record.
#pragma once

namespace {

constexpr int MIQP_POOL_MAX = 16;
constexpr int POOL_PASSES = 6;   // re-labelling passes of miqp_solver_pool_solve (the alternatives of a disjunction only move to earlier ones: it ends)

struct PoolArgs {
  const unsigned long long* candkey; const int* candinst; const double* batch_obj; const signed char* batch_comp; const int* slot_inst;
  int* list; int* count;          // count[par]: this capture's; count[par ^ 1] is zeroed for the next capture
  signed char* fix; double* obj; unsigned int* hash; int* cnt; const int* cap;
  int bc, fixlen, declen, stride, list_cap, par, n_inst;
};

__global__ __launch_bounds__(256) void pool_compact_kernel(const PoolArgs A) {
  const int k = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
  if (k == 0) A.count[A.par ^ 1] = 0;
  const bool is = k < A.bc && A.candkey[k] != ~0ull;
  const unsigned long long m = __ballot(is);
  int base = 0;
  if (lane == 0 && m) base = atomicAdd(&A.count[A.par], __popcll(m));
  base = __shfl(base, 0, 64);
  if (is) { const int p = base + __popcll(m & ((1ull << lane) - 1ull)); if (p < A.list_cap) A.list[p] = k; }
}

__global__ __launch_bounds__(64) void pool_merge_kernel(const PoolArgs A) {
  extern __shared__ uint4 cand[];   // the candidate's record, mask bytes reset
  const int lane = threadIdx.x;
  const int inst = A.slot_inst[blockIdx.x];
  if (inst < 0 || inst >= A.n_inst) return;
  const int K = min(A.cap[inst], A.stride);
  if (K <= 0) return;
  const int m = min(A.count[A.par], min(A.bc, A.list_cap)), chunks = A.fixlen >> 4;
  uint4* const rec = (uint4*)(A.fix + (size_t)inst * A.stride * A.fixlen);
  double* const pobj = A.obj + (size_t)inst * A.stride; unsigned int* const phash = A.hash + (size_t)inst * A.stride;
  int cnt = min(A.cnt[inst], K);
  // the list 64 entries at a time: every lane looks at one entry, a ballot says which are this instance's (a wide stream has thousands of entries
  // and a handful per instance: the loads of a step are independent, not a chain of two per entry)
  for (int q0 = 0; q0 < m; q0 += 64) {
    int mynode = q0 + lane < m ? A.list[q0 + lane] : -1;
    if ((unsigned)mynode >= (unsigned)A.bc || A.candinst[mynode] != inst) mynode = -1;
    unsigned long long own = __ballot(mynode >= 0);
    for (; own; own &= own - 1ull) {
      const int node = __shfl(mynode, __ffsll((long long)own) - 1, 64);
      __syncthreads();
      int h = 0;
      {
        const uint4* src = (const uint4*)(A.batch_comp + (size_t)node * A.fixlen);
        for (int c = lane; c < chunks; c += 64) {
          uint4 v = src[c]; signed char* b = (signed char*)&v;
          for (int t = 0; t < 16; ++t) { const int k = c * 16 + t; if (k >= A.declen) b[t] = (signed char)-1; else h += ((int)b[t] + 3) * (2 * k + 1); }
          cand[c] = v;
        }
        for (int o = 32; o > 0; o >>= 1) h += __shfl_xor(h, o, 64);
      }
      __syncthreads();
      const unsigned int hs = (unsigned int)h; const double o = A.batch_obj[node]; const unsigned long long ok = d2key(o);
      // the same record already kept: the smaller objective stays (and the entry moves to its new place)
      int dup = -1;
      for (int j = 0; j < cnt && dup < 0; ++j) if (phash[j] == hs && pool_cmp(cand, rec + (size_t)j * chunks, chunks, lane) == 0) dup = j;
      if (dup >= 0) {
        if (!(ok < d2key(pobj[dup]))) continue;
        for (int j = dup; j + 1 < cnt; ++j) {
          for (int c = lane; c < chunks; c += 64) rec[(size_t)j * chunks + c] = rec[(size_t)(j + 1) * chunks + c];
          if (lane == 0) { pobj[j] = pobj[j + 1]; phash[j] = phash[j + 1]; }
          __syncthreads();
        }
        cnt--;
      }
      int p = 0;
      for (int j = 0; j < cnt; ++j) {
        const unsigned long long kj = d2key(pobj[j]); const unsigned int hj = phash[j];
        bool less = kj < ok || (kj == ok && hj < hs);
        if (!less && kj == ok && hj == hs) less = pool_cmp(rec + (size_t)j * chunks, cand, chunks, lane) < 0;
        if (less) p = j + 1;
      }
      if (p >= K) continue;
      const int last = min(cnt, K - 1);   // entries p .. last - 1 move down by one (the one at K - 1 leaves)
      for (int j = last; j > p; --j) {
        for (int c = lane; c < chunks; c += 64) rec[(size_t)j * chunks + c] = rec[(size_t)(j - 1) * chunks + c];
        if (lane == 0) { pobj[j] = pobj[j - 1]; phash[j] = phash[j - 1]; }
        __syncthreads();
      }
      for (int c = lane; c < chunks; c += 64) rec[(size_t)p * chunks + c] = cand[c];
      if (lane == 0) { pobj[p] = o; phash[p] = hs; }
      cnt = min(cnt + 1, K);
      __syncthreads();
    }
  }
  if (lane == 0) A.cnt[inst] = cnt;
}

// ---------------------------------------------------------------------------------------------------------------- manoeuvre filter
// (the families, the sites of a record and the signature of a site: pool_blocks.hip)
struct PoolFilterArgs { PoolArgs A; signed char* sig; const int* fam; PoolDims dims; };

// pool_merge_kernel with the filter: the same launch (one wavefront per instance in flight, owner computes, ballot over 64 list entries), the same
// order of the pool; what changes is which entry a candidate IS.  The candidate's signature is built in a second LDS block (one lane per site, in a
// loop when there are more sites than lanes) and compared with the signatures kept beside the records; a candidate of a kept signature replaces that
// entry when it is smaller in the pool's order, else it is dropped.  fam[inst] == 0: the signature is the record, and every step below is
// pool_merge_kernel's (the signature buffer is not touched)
__global__ __launch_bounds__(64) void pool_filter_kernel(const PoolFilterArgs F) {
  extern __shared__ uint4 cand[];   // the candidate's record, mask bytes reset; behind it its signature
  const PoolArgs& A = F.A;
  const int lane = threadIdx.x;
  const int inst = A.slot_inst[blockIdx.x];
  if (inst < 0 || inst >= A.n_inst) return;
  const int K = min(A.cap[inst], A.stride);
  if (K <= 0) return;
  const int fam = F.fam[inst] & POOL_FAM_ALL;
  const int m = min(A.count[A.par], min(A.bc, A.list_cap)), chunks = A.fixlen >> 4;
  uint4* const csig = fam ? cand + chunks : cand;
  uint4* const rec = (uint4*)(A.fix + (size_t)inst * A.stride * A.fixlen);
  uint4* const sig = fam ? (uint4*)(F.sig + (size_t)inst * A.stride * A.fixlen) : rec;
  double* const pobj = A.obj + (size_t)inst * A.stride; unsigned int* const phash = A.hash + (size_t)inst * A.stride;
  int cnt = min(A.cnt[inst], K);
  for (int q0 = 0; q0 < m; q0 += 64) {
    int mynode = q0 + lane < m ? A.list[q0 + lane] : -1;
    if ((unsigned)mynode >= (unsigned)A.bc || A.candinst[mynode] != inst) mynode = -1;
    unsigned long long own = __ballot(mynode >= 0);
    for (; own; own &= own - 1ull) {
      const int node = __shfl(mynode, __ffsll((long long)own) - 1, 64);
      __syncthreads();
      int h = 0;
      {
        const uint4* src = (const uint4*)(A.batch_comp + (size_t)node * A.fixlen);
        for (int c = lane; c < chunks; c += 64) {
          uint4 v = src[c]; signed char* b = (signed char*)&v;
          for (int t = 0; t < 16; ++t) { const int k = c * 16 + t; if (k >= A.declen) b[t] = (signed char)-1; else h += ((int)b[t] + 3) * (2 * k + 1); }
          cand[c] = v;
          if (fam) csig[c] = make_uint4(~0u, ~0u, ~0u, ~0u);
        }
        for (int o = 32; o > 0; o >>= 1) h += __shfl_xor(h, o, 64);
      }
      if (fam) pool_sign(F.dims, fam, cand, csig, lane); else __syncthreads();
      const unsigned int hs = (unsigned int)h; const double o = A.batch_obj[node]; const unsigned long long ok = d2key(o);
      // an entry of this signature already kept: the smaller of the two in the pool's order stays (and moves to its new place)
      int dup = -1;
      for (int j = 0; j < cnt && dup < 0; ++j) if ((fam || phash[j] == hs) && pool_cmp(csig, sig + (size_t)j * chunks, chunks, lane) == 0) dup = j;
      if (dup >= 0) {
        const unsigned long long kd = d2key(pobj[dup]); const unsigned int hd = phash[dup];
        bool less = ok < kd || (ok == kd && hs < hd);
        if (fam && !less && ok == kd && hs == hd) less = pool_cmp(cand, rec + (size_t)dup * chunks, chunks, lane) < 0;
        if (!less) continue;
        for (int j = dup; j + 1 < cnt; ++j) {
          for (int c = lane; c < chunks; c += 64) {
            rec[(size_t)j * chunks + c] = rec[(size_t)(j + 1) * chunks + c];
            if (fam) sig[(size_t)j * chunks + c] = sig[(size_t)(j + 1) * chunks + c];
          }
          if (lane == 0) { pobj[j] = pobj[j + 1]; phash[j] = phash[j + 1]; }
          __syncthreads();
        }
        cnt--;
      }
      int p = 0;
      for (int j = 0; j < cnt; ++j) {
        const unsigned long long kj = d2key(pobj[j]); const unsigned int hj = phash[j];
        bool less = kj < ok || (kj == ok && hj < hs);
        if (!less && kj == ok && hj == hs) less = pool_cmp(rec + (size_t)j * chunks, cand, chunks, lane) < 0;
        if (less) p = j + 1;
      }
      if (p >= K) continue;
      const int last = min(cnt, K - 1);   // entries p .. last - 1 move down by one (the one at K - 1 leaves)
      for (int j = last; j > p; --j) {
        for (int c = lane; c < chunks; c += 64) {
          rec[(size_t)j * chunks + c] = rec[(size_t)(j - 1) * chunks + c];
          if (fam) sig[(size_t)j * chunks + c] = sig[(size_t)(j - 1) * chunks + c];
        }
        if (lane == 0) { pobj[j] = pobj[j - 1]; phash[j] = phash[j - 1]; }
        __syncthreads();
      }
      for (int c = lane; c < chunks; c += 64) { rec[(size_t)p * chunks + c] = cand[c]; if (fam) sig[(size_t)p * chunks + c] = csig[c]; }
      if (lane == 0) { pobj[p] = o; phash[p] = hs; }
      cnt = min(cnt + 1, K);
      __syncthreads();
    }
  }
  if (lane == 0) A.cnt[inst] = cnt;
}

// the whole signature on the host: sg[0 .. fixlen) (-1 behind the decisions, like the mask bytes of a pool record)
inline void pool_signature(const PoolDims& d, int fam, const signed char* rec, signed char* sg, size_t len) {
  std::memset(sg, 0xFF, len);
  for (int s = 0, n = pool_sites(d); s < n; ++s) pool_site_signature(d, fam, s, rec, sg);
}
inline PoolDims pool_dims(const Layout& Y) { return PoolDims{Y.C, Y.N, Y.O, Y.NP}; }

// "the same entry" of the refinement (miqp_solver_pool_solve and miqp_solver_pool_solve_multi, so that the two cannot drift apart): two feasible
// entries whose final labels a, b are the same binaries, or - under the handle's filter - have the same signature
inline bool pool_same_entry(const Layout& Y, int fam, const signed char* a, const signed char* b) {
  const size_t fl = (size_t)Y.fixlen;
  if (std::memcmp(a, b, fl) == 0) return true;
  if (!(fam & POOL_FAM_ALL)) return false;
  std::vector<signed char> sa(fl), sb(fl);
  pool_signature(pool_dims(Y), fam, a, sa.data(), fl); pool_signature(pool_dims(Y), fam, b, sb.data(), fl);
  return sa == sb;
}

// ---------------------------------------------------------------------------------------------------------------- host: capture
template <class Tp> bool pool_alloc(DevCtx& X, Tp** p, size_t n) { X.drop(p); return X.alloc(p, n); }

bool pool_prepare(DevCtx& X, miqp_solver_t* const* S, int n) {
  int stride = 0; bool filt = false;   // (a filter counts only on a handle that has a pool)
  for (int k = 0; k < n; ++k) { stride = std::max(stride, std::min(S[k]->pool_cap, MIQP_POOL_MAX)); filt = filt || (S[k]->pool_cap > 0 && (S[k]->pool_fam & POOL_FAM_ALL) != 0); }
  X.pool.on = stride > 0; X.pool.filt = false;
  if (!X.pool.on) return true;
  SolPoolDev& Q = X.pool; const size_t fl = (size_t)X.Y.fixlen;
  if (!Q.fix || Q.n_inst < n || Q.stride < stride || Q.list_cap < X.batch_alloc || (filt && !Q.sig)) {
    filt = filt || Q.sig != nullptr;   // (a context that held signatures keeps holding them: a later call with a filter finds them)
    const size_t bytes = (size_t)n * stride * (fl + 12) + (size_t)n * 8 + (size_t)X.batch_alloc * 4 + 8 + (filt ? (size_t)n * stride * fl + (size_t)n * 4 : 0);
    Q.n_inst = 0;
    bool ok = pool_alloc(X, &Q.fix, (size_t)n * stride * fl) && pool_alloc(X, &Q.obj, (size_t)n * stride) && pool_alloc(X, &Q.hash, (size_t)n * stride) &&
              pool_alloc(X, &Q.cnt, (size_t)n) && pool_alloc(X, &Q.cap, (size_t)n) && pool_alloc(X, &Q.list, (size_t)X.batch_alloc) && pool_alloc(X, &Q.count, 2);
    if (ok && filt) ok = pool_alloc(X, &Q.sig, (size_t)n * stride * fl) && pool_alloc(X, &Q.fam, (size_t)n);
    if (!ok) {
      char msg[200]; std::snprintf(msg, sizeof msg, "the solution pool of this call (%d instances x %d entries%s, %zu bytes) does not fit the device", n, stride, filt ? ", with signatures" : "", bytes);
      for (int k = 0; k < n; ++k) S[k]->err = msg;
      std::fprintf(stderr, "[miqp_gpu] %s\n", msg);
      X.pool.on = false; return false;
    }
    Q.n_inst = n; Q.stride = stride; Q.list_cap = X.batch_alloc;
  }
  std::vector<int> cap(n); for (int k = 0; k < n; ++k) cap[k] = std::max(0, std::min(S[k]->pool_cap, MIQP_POOL_MAX));
  HIP_OK(hipMemcpyAsync(Q.cap, cap.data(), (size_t)n * 4, hipMemcpyHostToDevice, X.stream));
  std::vector<int> fam(n, 0);
  for (int k = 0; k < n; ++k) if (cap[k] > 0 && (S[k]->pool_fam & POOL_FAM_ALL)) { fam[k] = S[k]->pool_fam & POOL_FAM_ALL; Q.filt = true; }
  if (Q.filt) HIP_OK(hipMemcpyAsync(Q.fam, fam.data(), (size_t)n * 4, hipMemcpyHostToDevice, X.stream));
  HIP_OK(hipMemsetAsync(Q.cnt, 0, (size_t)n * 4, X.stream)); HIP_OK(hipMemsetAsync(Q.count, 0, 8, X.stream)); Q.captures = 0;
  HIP_OK(hipStreamSynchronize(X.stream));   // (cap and fam are locals)
  return true;
}

// The parity of the list counter follows the captures that were launched, not the rounds: a round without a batch (every instance in flight ended
// at once - with one in flight, every instance's end; a rank of a tree split with nothing left) launches none, and the word it would have zeroed
// would come back a round later with the count of two rounds before
bool pool_capture(DevCtx& X, int bc) {
  const DevBuf& B = X.B; SolPoolDev& Q = X.pool;
  PoolArgs A;
  A.candkey = B.batch_candkey; A.candinst = B.batch_candinst; A.batch_obj = B.batch_obj; A.batch_comp = B.batch_comp; A.slot_inst = B.slot_inst;
  A.list = Q.list; A.count = Q.count; A.fix = Q.fix; A.obj = Q.obj; A.hash = Q.hash; A.cnt = Q.cnt; A.cap = Q.cap;
  A.bc = std::min(bc, Q.list_cap); A.fixlen = X.Y.fixlen; A.declen = X.Y.f_c2n; A.stride = Q.stride; A.list_cap = Q.list_cap; A.par = Q.captures & 1; A.n_inst = std::min(X.n_inst, Q.n_inst);
  if (A.bc <= 0) return true;
  Q.captures++;
  hipLaunchKernelGGL(pool_compact_kernel, dim3((A.bc + 255) / 256), dim3(256), 0, X.stream, A);
  if (Q.filt) {
    PoolFilterArgs F; F.A = A; F.sig = Q.sig; F.fam = Q.fam; F.dims = pool_dims(X.Y);
    hipLaunchKernelGGL(pool_filter_kernel, dim3(X.n_slots), dim3(64), 2 * (size_t)X.Y.fixlen, X.stream, F);
  } else
    hipLaunchKernelGGL(pool_merge_kernel, dim3(X.n_slots), dim3(64), (size_t)X.Y.fixlen, X.stream, A);
  HIP_OK(hipGetLastError());
  return true;
}

// next to read_back: every handle receives its kept records, the objectives as found and the count.  Entry 0 is the incumbent the call reports, on
// every path: it is a candidate of some round and the smallest in the search's order - the objective to 44 bits, then the hash of the WHOLE record -
// which the pool's order (the full objective, then the hash of the decisions) follows except among records whose objectives agree to those 44 bits.
// There another record can sort in front of the incumbent's, or (capacity 1, or that many ties) push it out: the incumbent's record (R.fix, mask
// bytes reset like a pool record) is moved to the front, or put there with the objective it was found with, the last entry leaving - under a filter the
// entry of the incumbent's signature, when there is one: the pool keeps one entry per signature
bool pool_read_back(const DevCtx& X, miqp_solver_t* const* S, int n, const Results& R) {
  const SolPoolDev& Q = X.pool; const size_t fl = (size_t)X.Y.fixlen; const int declen = X.Y.f_c2n;
  std::vector<int> cnt(n); std::vector<double> obj((size_t)n * Q.stride), inc(n); std::vector<signed char> fix((size_t)n * Q.stride * fl);
  HIP_OK(hipMemcpy(cnt.data(), Q.cnt, (size_t)n * 4, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(obj.data(), Q.obj, obj.size() * 8, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(fix.data(), Q.fix, fix.size(), hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(inc.data(), X.B.inc_obj, (size_t)n * 8, hipMemcpyDeviceToHost));   // (as found: R.inc is the polished one by now)
  std::vector<signed char> mine(fl), msig(fl), esig(fl);
  for (int k = 0; k < n; ++k) {
    miqp_solver* s = S[k];
    const int K = std::max(0, std::min(s->pool_cap, Q.stride));
    int c = std::max(0, std::min(cnt[k], K));
    double* po = obj.data() + (size_t)k * Q.stride; signed char* pf = fix.data() + (size_t)k * Q.stride * fl;
    if (K > 0 && inc[k] < 1e299 && R.fix.size() >= (size_t)(k + 1) * fl) {
      std::memcpy(mine.data(), R.fix.data() + (size_t)k * fl, fl);
      for (size_t q = (size_t)declen; q < fl; ++q) mine[q] = (signed char)-1;
      int at = -1;
      for (int j = 0; j < c && at < 0; ++j) if (std::memcmp(pf + (size_t)j * fl, mine.data(), fl) == 0) at = j;
      int twin = -1;   // the entry of the incumbent's signature, its record not being kept
      const int fam = s->pool_fam & POOL_FAM_ALL;
      if (at < 0 && fam) {
        pool_signature(pool_dims(X.Y), fam, mine.data(), msig.data(), fl);
        for (int j = 0; j < c && twin < 0; ++j) { pool_signature(pool_dims(X.Y), fam, pf + (size_t)j * fl, esig.data(), fl); if (esig == msig) twin = j; }
      }
      if (at != 0) {
        const double o = at > 0 ? po[at] : inc[k];
        const int last = at > 0 ? at : (twin >= 0 ? twin : std::min(c, K - 1));   // entries 0 .. last - 1 move down by one
        std::memmove(pf + fl, pf, (size_t)last * fl); std::memmove(po + 1, po, (size_t)last * 8);
        std::memcpy(pf, mine.data(), fl); po[0] = o;
        if (at < 0 && twin < 0) c = std::min(c + 1, K);
      }
    }
    s->pool_n = c; s->pool_fixlen = (int)fl;
    s->pool_obj.assign(po, po + c);
    s->pool_fix.assign(pf, pf + (size_t)c * fl);
  }
  return true;
}

// The refinement of the first ent[h] pool entries of every handle of an open call (`name`: the entry point, for its messages).  Passes: the entries
// of the handles whose labels moved in the pass before (the first pass: all) run through the chain and are re-labelled with the canonical binaries
// of their own solutions, at most POOL_PASSES times.  Then, per handle, entries whose records carry the same binaries are ONE solution (the optimum
// of one holds the alternatives of the other too, so both QPs have the same strictly convex minimiser), and under the handle's filter so are
// entries whose final labels have one signature (pool_same_entry): the first in pool order stays, the handle's pool shrinks with it.  The handle
// keeps what miqp_solver_pool_record hands out and its last_timing; kept[h] receives its answers.  false: HIP error
bool pool_refine(FixedCall& call, const int* ent, const char* name, double t_call, std::vector<std::vector<miqp_fixed_result_c>>& kept_out) {
  const int n = call.n; miqp_solver_t* const* solvers = call.S;
  const Layout& Y = call.Y; const size_t fl = (size_t)Y.fixlen, row = (size_t)Y.N * Y.nz;
  // per handle: the labels its entries are solved with, those of their own solutions (the ones a caller of miqp_solver_solve_fixed would send for
  // its record), the last answers
  struct PerHandle { std::vector<signed char> fix, canon; std::vector<miqp_fixed_result_c> tmp; std::vector<double> Z; int passes = 0; bool moving = true; };
  std::vector<PerHandle> H(n);
  for (int h = 0; h < n; ++h) { H[h].moving = ent[h] > 0; H[h].fix.assign(solvers[h]->pool_fix.begin(), solvers[h]->pool_fix.begin() + (size_t)ent[h] * fl); H[h].canon.resize((size_t)ent[h] * fl); }
  float dev_ms = 0.0f;
  for (int pass = 0; pass < POOL_PASSES; ++pass) {
    std::vector<int> live, inst, lfirst;
    std::vector<signed char> fix;
    for (int h = 0; h < n; ++h) if (H[h].moving) { live.push_back(h); lfirst.push_back((int)inst.size()); inst.insert(inst.end(), ent[h], h); fix.insert(fix.end(), H[h].fix.begin(), H[h].fix.end()); }
    if (live.empty()) break;
    const int m = (int)inst.size();
    std::vector<miqp_fixed_result_c> tmp; std::vector<double> Z; std::vector<int> hbest; float ms = 0.0f; int g = 0;
    if (call.run(fix, inst, m, tmp, Z, hbest, ms, g) != 0) return false;
    dev_ms += ms;
    fixed_threads((int)live.size(), 4, [&](int q) {
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
  kept_out.assign(n, {});
  for (int h = 0; h < n; ++h) {
    miqp_solver_t* s = solvers[h]; PerHandle& P = H[h]; const int m = ent[h];
    s->timing[0] = call_s; s->timing[1] = dev_ms * 1e-3; s->timing[2] = P.passes; s->timing[3] = 0; s->timing[4] = 0; s->timing[5] = 0;
    if (m == 0) continue;
    if (P.moving) {   // not seen on any instance so far; the entries are then answers to the labels of the last pass, not yet to those of their own records
      char msg[220]; std::snprintf(msg, sizeof msg, "%s: the labels of the pool entries still moved after %d passes; an entry may differ from what miqp_solver_solve_fixed answers for its record", name, P.passes);
      s->err = msg; std::fprintf(stderr, "[miqp_gpu] %s\n", msg);
    }
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
    fix.resize((size_t)kept * fl); Z.resize((size_t)kept * row); tmp.resize(kept);
    s->pr_n = kept; s->pr_ok.assign(kept, 0);
    for (int k = 0; k < kept; ++k) s->pr_ok[k] = tmp[k].status == 0 ? 1 : 0;
    s->pr_Z.swap(Z); s->pr_fix.swap(fix);
    s->timing[3] = kept; s->timing[5] = P.moving ? 1 : 0;
    for (int k = 0; k < kept; ++k) s->timing[4] += tmp[k].iterations;
    kept_out[h].swap(tmp);
  }
  return true;
}

}  // namespace

extern "C" {

int miqp_gpu_pool_max(void) { return MIQP_POOL_MAX; }

int miqp_solver_set_pool(miqp_solver_t* s, int capacity) {
  if (!s) return -1;
  if (capacity < 0 || capacity > MIQP_POOL_MAX) return -2;
  s->pool_cap = capacity;
  return 0;
}

int miqp_solver_set_pool_filter(miqp_solver_t* s, int families) {
  if (!s) return -1;
  if (families < 0 || families > POOL_FAM_ALL) return -2;
  s->pool_fam = families;
  return 0;
}

int miqp_gpu_pool_signature(int cars, int steps, int obstacles, int families, const signed char* decisions, signed char* out, int len) {
  if (!decisions || !out || cars <= 0 || steps <= 0 || obstacles < 0) return -1;
  if (families < 1 || families > POOL_FAM_ALL) return -2;
  const PoolDims d{cars, steps, obstacles, cars * (cars - 1) / 2};
  const int D = pool_declen(d);
  if (len < D) return -3;
  pool_signature(d, families, decisions, out, (size_t)D);
  return D;
}

int miqp_solver_pool_signature(const miqp_solver_t* s, const miqp_raw_results_c* rec, int families, signed char* out, int cap) {
  if (!s || !rec || !out || !s->has_inst) return -1;
  if (families < 1 || families > POOL_FAM_ALL || !cert_candidate_ok(*rec)) return -2;
  if (!dims_match(*rec, s->inst)) return -3;   // a record of another shape is never indexed
  miqp_solver_t* one[1] = {const_cast<miqp_solver_t*>(s)};
  BatchShape bs = batch_layout(one, 1);
  if (!bs.ok) return -1;
  const Layout& Y = bs.Y;
  if (cap < Y.f_c2n) return -4;
  std::vector<double> D(Y.dstride); std::vector<int> T(Y.istride);
  compile_instance(s->inst, Y, D.data(), T.data());
  std::vector<signed char> fix, sg((size_t)Y.fixlen);
  if (!fix_from_results(s->inst, Y, T.data(), rec, fix)) return -2;
  pool_signature(pool_dims(Y), families, fix.data(), sg.data(), sg.size());
  std::memcpy(out, sg.data(), (size_t)Y.f_c2n);
  return Y.f_c2n;
}

int miqp_solver_pool_found_decisions(const miqp_solver_t* s, int k, signed char* out, int cap) {
  if (!s || !out || k < 0 || k >= miqp_solver_pool_count(s)) return -1;
  const PoolDims d{s->inst.C, s->inst.N, s->inst.O, s->inst.C * (s->inst.C - 1) / 2};
  const int D = pool_declen(d);
  if (D > s->pool_fixlen || s->pool_fix.size() < (size_t)(k + 1) * s->pool_fixlen) return -1;
  if (cap < D) return -3;
  std::memcpy(out, s->pool_fix.data() + (size_t)k * s->pool_fixlen, (size_t)D);
  return D;
}

int miqp_solver_pool_count(const miqp_solver_t* s) { return (s && s->has_inst && (s->has_sol || s->pool_carried) && s->pool_cap > 0) ? s->pool_n : 0; }

int miqp_solver_pool_found(const miqp_solver_t* s, double* obj, int cap) {
  if (!s || !obj || cap < 0) return -1;
  const int n = std::min(miqp_solver_pool_count(s), cap);
  for (int k = 0; k < n; ++k) obj[k] = s->pool_obj[k];
  return n;
}

int miqp_solver_pool_solve(miqp_solver_t* s, miqp_fixed_result_c* out, int cap) {
  if (s) { s->pr_n = 0; }
  if (!s || !s->has_inst || !out || cap < 1) return -1;
  { int ndev = 0; if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return -3; }
  const int m = std::min(miqp_solver_pool_count(s), cap);
  if (m == 0) return 0;
  miqp_solver_t* one[1] = {s};
  BatchShape bs = batch_layout(one, 1);
  if (!bs.ok || bs.Y.fixlen != s->pool_fixlen) return -1;
  const double t_call = wall_s();
  FixedCall call;
  if (call.open(one, 1, bs.Y) != 0) return -3;
  std::vector<std::vector<miqp_fixed_result_c>> kept;
  if (!pool_refine(call, &m, "miqp_solver_pool_solve", t_call, kept)) return -3;
  std::copy(kept[0].begin(), kept[0].end(), out);
  return (int)kept[0].size();
}

int miqp_solver_pool_solve_multi(miqp_solver_t* const* solvers, int n, miqp_fixed_result_c* out, int cap, int* counts) {
  if (!solvers || !out || !counts || n <= 0 || cap < 1) return -1;
  BatchShape bs;
  if (const int rc = fixed_multi_check(solvers, n, bs)) return rc;
  std::vector<int> ent(n); int total = 0;
  for (int h = 0; h < n; ++h) {
    ent[h] = std::min(miqp_solver_pool_count(solvers[h]), cap);
    if (ent[h] > 0 && solvers[h]->pool_fixlen != bs.Y.fixlen) return -1;
    total += ent[h];
  }
  if (total > FB_CAP) return -5;
  for (int h = 0; h < n; ++h) { solvers[h]->pr_n = 0; counts[h] = 0; }
  if (total == 0) return 0;   // (nothing to run: no device is touched)
  const double t_call = wall_s();
  FixedCall call;
  if (call.open(solvers, n, bs.Y) != 0) return -3;
  std::vector<std::vector<miqp_fixed_result_c>> kept;
  if (!pool_refine(call, ent.data(), "miqp_solver_pool_solve_multi", t_call, kept)) return -3;
  int left = 0;
  for (int h = 0; h < n; ++h) { std::copy(kept[h].begin(), kept[h].end(), out + (size_t)h * cap); counts[h] = (int)kept[h].size(); left += counts[h]; }
  return left;
}

int miqp_solver_pool_record(miqp_solver_t* s, int k, miqp_raw_results_c* out) {
  if (!s || !out || !s->has_inst || s->pr_n <= 0 || k < 0 || k >= s->pr_n) return -1;
  if (!s->pr_ok[k]) return 1;
  if (!dims_match(*out, s->inst)) return -2;
  return fixed_hand_out(s, s->pr_fix, s->pr_Z, k, out);
}

}  // extern "C"

// pool_label.hip - the canonical labels of solved nodes where they lie (pool_label_kernel), the decision records of a caller solved and labelled in
// one call (miqp_solver_canonical_decisions), and the host restatement both are pinned with (miqp_solver_canonical_labels).  DESIGN.md 6i.
//
// A fix record says which alternative of every disjunction a node ASSERTS.  Its solution usually holds more than the asserted ones - an obstacle far
// away is cleared on several edges at once - so two records of different bytes can be one trajectory.  What tells solutions apart is the CANONICAL
// record of the solution: per disjunction the FIRST alternative that holds at the returned point, which is what the host builds from one RawResults
// record at a time (fill_results, then fix_from_results; miqp_gpu.hip).  The explore (pool_explore.hip) needs it for thousands of nodes per pass
// whose trajectories never leave the device and are written over chunk by chunk: this kernel labels a chunk behind its fixed_chunk.
//
// pool_label_byte below is fix_from_results(fill_results(Z, record)) for ONE decision byte (site, step >= 1), as the library's hand-outs call the
// pair (fixed_hand_out, pool_refine): an undecided byte of the record counts as alternative 0 there, so the argmin branch fill_results has for an
// undecided car/car byte is never taken behind a hand-out and is not restated.
//   region        q * 4 + h: q the record's own possible-region index (looked up again through its region number, as fix_from_results does); h = 3
//                 stays 3, else the first half-plane k < nhs(c, q) whose "change not allowed" flag is 0 - the direction of the record's own h, or a
//                 direction whose velocity bound |v| <= vm fails - and 0 when none is
//   environment   the first piece e with env_viol(e, X, Y) <= tol at the point's coordinates, else -1
//   obstacle      L when the record's byte is >= L and the obstacle is soft; else the first edge k < L with obs_viol <= tol - none holds when the
//                 record ignores the point - else -1
//   car/car       the first a in 0 .. 3 with a == chosen || need <= tol, need reduced by the slack of the chosen alternative in groups 0 and 3
// tol = 10 FEAS_TOL; points are HostGeo::point with the region index of the record.  The labels are threshold tests on a X + b Y - c and on the point
// polynomials, so the device evaluates in the host's order with every operation rounded on its own (PL_MUL, PL_ADD, PL_SUB: the host side of the
// library is x86-64 without fused multiply-add): a label then agrees with the host's bit for bit, ties at tol included.
// A node that is not feasible gets an all -1 record, and so does a record with an undecided region byte at a step >= 1 (or a region index beyond the
// tables): the points of that step have no region to be taken in.
//
// Kernel: one wavefront per node.  The record and the trajectory row are staged in LDS with 16-byte loads, the lanes take the decision bytes
// (site x step, in a loop when there are more than 64) and write them into a second record in LDS, which leaves as 16-byte stores.  The instance's
// tables are read through L2: every node of a handle shares them.  No atomics, no wavefront waits on another, no scratch.
#pragma once

#ifdef __HIP_DEVICE_COMPILE__
#define PL_MUL(a, b) __dmul_rn((a), (b))
#define PL_ADD(a, b) __dadd_rn((a), (b))
#define PL_SUB(a, b) __dsub_rn((a), (b))
#define PL_ENV_PT ENV_PT_D
#define PL_OBS_PT OBS_PT_D
#else
#define PL_MUL(a, b) ((a) * (b))
#define PL_ADD(a, b) ((a) + (b))
#define PL_SUB(a, b) ((a) - (b))
#define PL_ENV_PT ENV_PT_H
#define PL_OBS_PT OBS_PT_H
#endif

namespace {

constexpr size_t POOL_LABEL_LDS_MAX = 160 * 1024;   // dynamic LDS of pool_label_kernel (two records and a trajectory row): the LDS of a gfx950 workgroup

// HostGeo::point at a step >= 1 (z: the step's row of the trajectory)
__host__ __device__ inline void pl_point(const Layout& Y, const double* D, const double* z, int c, int q, int tx, int ty, double& X, double& Yc) {
  const double* rt = D + Y.d_reg + (c * Y.P + q) * REGSZ;
  const double vx = z[6 * c + 1], vy = z[6 * c + 4];
  X = z[6 * c + 0]; Yc = z[6 * c + 3];
  if (tx != PT_R) { const double* p = rt + 19 + (tx == PT_U ? 0 : 3); X = PL_ADD(X, PL_ADD(PL_ADD(p[0], PL_MUL(p[1], vx)), PL_MUL(p[2], vy))); }
  if (ty != PT_R) { const double* p = rt + 25 + (ty == PT_U ? 0 : 3); Yc = PL_ADD(Yc, PL_ADD(PL_ADD(p[0], PL_MUL(p[1], vx)), PL_MUL(p[2], vy))); }
}

// a X + b Y - c of an edge (HostGeo::env_viol's term, HostGeo::obs_viol)
__host__ __device__ inline double pl_edge(const double* ed, double X, double Yc) { return PL_SUB(PL_ADD(PL_MUL(ed[0], X), PL_MUL(ed[1], Yc)), ed[2]); }

__host__ __device__ inline double pl_env_viol(const Layout& Y, const double* D, const int* T, int e, double X, double Yc) {
  double v = -1e300;
  for (int k = 0, n = T[Y.i_envn + e]; k < n; ++k) { const double x = pl_edge(D + Y.d_env + (e * Y.EL + k) * 3, X, Yc); if (v < x) v = x; }   // (std::max(v, x))
  return v;
}

// HostGeo::c2c_viol at a step >= 1
__host__ __device__ inline double pl_c2c_viol(const Layout& Y, const double* D, const double* z, int p, int c1, int c2, int i, int grp, int alt, int q1, int q2) {
  const double Dsep = D[Y.d_dsep + p * Y.N + i], S = D[Y.d_ssl + i];
  const bool isx = alt < 2, lo = (alt == 0 || alt == 2), soft = (grp == 0 || grp == 3);
  int ca, cb, ta, tb;
  if (grp == 0) { ta = tb = PT_R; ca = lo ? c1 : c2; cb = lo ? c2 : c1; }
  else if (grp == 1) { if (lo) { ca = c1; ta = PT_R; cb = c2; tb = PT_L; } else { ca = c2; ta = PT_U; cb = c1; tb = PT_R; } }
  else if (grp == 2) { if (lo) { ca = c2; ta = PT_R; cb = c1; tb = PT_L; } else { ca = c1; ta = PT_U; cb = c2; tb = PT_R; } }
  else { if (lo) { ca = c2; ta = PT_U; cb = c1; tb = PT_L; } else { ca = c1; ta = PT_U; cb = c2; tb = PT_L; } }
  double XA, YA, XB, YB;
  pl_point(Y, D, z, ca, ca == c1 ? q1 : q2, ta, ta, XA, YA); pl_point(Y, D, z, cb, cb == c1 ? q1 : q2, tb, tb, XB, YB);
  return PL_ADD(isx ? PL_SUB(XA, XB) : PL_SUB(YA, YB), soft ? PL_ADD(Dsep, S) : Dsep);
}

// every region byte of the steps >= 1 is decided and indexes the tables (the whole record is -1 otherwise)
__host__ __device__ inline bool pool_label_region_ok(const Layout& Y, const signed char* rec, int k) {   // k < C * N
  if (k % Y.N == 0) return true;
  const int code = rec[Y.f_reg + k];
  return code >= 0 && (code >> 2) < Y.P;
}

// decision byte t of a labelled record: t = s * (N - 1) + i - 1, s a site in pool_site order, i its step >= 1.  `at` receives the byte's place.
// rec: a record whose regions pool_label_region_ok accepts; Z: its trajectory row; D, T: the tables of its instance
__host__ __device__ inline int pool_label_byte(const Layout& Y, const double* D, const int* T, const signed char* rec, const double* Z, int t, int& at) {
  const int N = Y.N, C = Y.C, O = Y.O, L = Y.L;
  const double tol = 10 * FEAS_TOL;
  int s = t / (N - 1); const int i = 1 + t % (N - 1);
  const double* z = Z + (size_t)i * Y.nz;
  if (s < C) {   // ---- region
    const int c = s;
    at = Y.f_reg + c * N + i;
    const int code = rec[at], q = code >> 2, h0 = code & 3;
    const int j = T[Y.i_regj + c * Y.P + q];
    int q2 = -1;
    for (int k = 0, n = T[Y.i_nposs + c]; k < n && k < Y.P; ++k) if (T[Y.i_regj + c * Y.P + k] == j) q2 = k;
    if (q2 < 0) return -1;
    if (h0 == 3) return q2 * 4 + 3;
    const double vx = z[6 * c + 1], vy = z[6 * c + 4], vm = D[Y.d_glob + 6];
    int xp = vx <= vm, xn = vx >= -vm, yp = vy <= vm, yn = vy >= -vm;
    {
      const int* hs = T + Y.i_hs + ((c * Y.P + q) * 2 + h0) * 2;
      if (hs[0] == 0 && hs[1] > 0) xp = 0;
      if (hs[0] == 0 && hs[1] < 0) xn = 0;
      if (hs[0] == 1 && hs[1] > 0) yp = 0;
      if (hs[0] == 1 && hs[1] < 0) yn = 0;
    }
    int h = 0;
    for (int k = 0, n = T[Y.i_nhs + c * Y.P + q2]; k < n && k < 2; ++k) {
      const int* hs = T + Y.i_hs + ((c * Y.P + q2) * 2 + k) * 2;
      const int b = hs[0] == 0 ? (hs[1] > 0 ? xp : xn) : (hs[1] > 0 ? yp : yn);
      if (b == 0) { h = k; break; }
    }
    return q2 * 4 + h;
  }
  s -= C;
  if (s < C * 5) {   // ---- environment
    const int c = s / 5, pt = s % 5, q = rec[Y.f_reg + c * N + i] >> 2;
    at = Y.f_env + (c * N + i) * 5 + pt;
    double X, Yc; pl_point(Y, D, z, c, q, PL_ENV_PT[pt][0], PL_ENV_PT[pt][1], X, Yc);
    for (int e = 0; e < Y.E; ++e) if (pl_env_viol(Y, D, T, e, X, Yc) <= tol) return e;
    return -1;
  }
  s -= C * 5;
  if (s < C * O * 5) {   // ---- obstacle
    const int co = s / 5, pt = s % 5, c = co / O, o = co % O, q = rec[Y.f_reg + c * N + i] >> 2;
    at = Y.f_obs + (co * N + i) * 5 + pt;
    const bool ignored = rec[at] >= L;
    if (ignored) return T[Y.i_obssoft + o] ? L : -1;
    double X, Yc; pl_point(Y, D, z, c, q, PL_OBS_PT[pt][0], PL_OBS_PT[pt][1], X, Yc);
    for (int k = 0; k < L; ++k) if (pl_edge(D + Y.d_obs + ((o * N + i) * L + k) * 3, X, Yc) <= tol) return k;
    return -1;
  }
  s -= C * O * 5;
  {   // ---- car/car
    const int p = s >> 2, g = s & 3;
    int c1 = 0, c2 = 1;   // pair p in the order c1 < c2
    for (int a = 0, k = 0; a < C; ++a) for (int b = a + 1; b < C; ++b, ++k) if (k == p) { c1 = a; c2 = b; }
    at = Y.f_c2c + (p * N + i) * 4 + g;
    const int q1 = rec[Y.f_reg + c1 * N + i] >> 2, q2 = rec[Y.f_reg + c2 * N + i] >> 2;
    const int chosen = rec[at] < 0 ? 0 : rec[at];   // (an undecided byte is alternative 0 behind the library's hand-outs)
    const double v0 = pl_c2c_viol(Y, D, z, p, c1, c2, i, g, 0, q1, q2), v1 = pl_c2c_viol(Y, D, z, p, c1, c2, i, g, 1, q1, q2);
    const double v2 = pl_c2c_viol(Y, D, z, p, c1, c2, i, g, 2, q1, q2), v3 = pl_c2c_viol(Y, D, z, p, c1, c2, i, g, 3, q1, q2);
    const double vc = chosen == 0 ? v0 : chosen == 1 ? v1 : chosen == 2 ? v2 : v3;
    double sl0 = 0.0, sl1 = 0.0;   // the slack of the chosen alternative: of the x pair (0, 1) or of the y pair (2, 3)
    if ((g == 0 || g == 3) && vc > 0) { if (chosen < 2) sl0 = vc; else sl1 = vc; }
    if (chosen == 0 || PL_SUB(v0, sl0) <= tol) return 0;
    if (chosen == 1 || PL_SUB(v1, sl0) <= tol) return 1;
    if (chosen == 2 || PL_SUB(v2, sl1) <= tol) return 2;
    if (chosen == 3 || PL_SUB(v3, sl1) <= tol) return 3;
    return -1;
  }
}

struct PoolLabelArgs {
  Layout Y;
  const signed char* fix;           // slot 0 of pool_fix: node k of the chunk is slot k
  const double* Z;                  // [bc][N * nz] the chunk's trajectory rows as fixed_collect_kernel left them
  const miqp_fixed_result_c* res;   // of the chunk's first node
  const int* batch_inst;            // the instance of slot k
  const double* inst_d; const int* inst_i;
  signed char* out;                 // [bc][fixlen] the labelled record of the chunk's first node
  int bc, n_inst;
};

__global__ __launch_bounds__(64) void pool_label_kernel(const PoolLabelArgs A) {
  extern __shared__ uint4 pl_lds[];   // the record, the labelled record, the trajectory row
  const Layout& Y = A.Y;
  const int k = blockIdx.x, lane = threadIdx.x, chunks = Y.fixlen >> 4, zchunks = (Y.N * Y.nz) >> 1;
  if (k >= A.bc) return;
  uint4* const rec4 = pl_lds; uint4* const out4 = rec4 + chunks; uint4* const z4 = out4 + chunks;
  const int inst = A.batch_inst[k];
  bool ok = A.res[k].status == 0 && (unsigned)inst < (unsigned)A.n_inst;   // (uniform over the wavefront)
  {
    const uint4* src = (const uint4*)(A.fix + (size_t)k * Y.fixlen);
    pool_stage(rec4, src, chunks, lane, out4);
    if (ok) { const uint4* zs = (const uint4*)(A.Z + (size_t)k * Y.N * Y.nz); for (int c = lane; c < zchunks; c += 64) z4[c] = zs[c]; }
  }
  __syncthreads();
  const signed char* const rec = (const signed char*)rec4; signed char* const out = (signed char*)out4; const double* const Z = (const double*)z4;
  if (ok) {
    bool bad = false;
    for (int q = lane; q < Y.C * Y.N; q += 64) bad = bad || !pool_label_region_ok(Y, rec, q);
    ok = __ballot(bad) == 0ull;
  }
  if (ok) {
    const double* D = A.inst_d + (size_t)inst * Y.dstride; const int* T = A.inst_i + (size_t)inst * Y.istride;
    const int nbytes = pool_sites(PoolDims{Y.C, Y.N, Y.O, Y.NP}) * (Y.N - 1);
    for (int t = lane; t < nbytes; t += 64) { int at = 0; const int v = pool_label_byte(Y, D, T, rec, Z, t, at); out[at] = (signed char)v; }
  }
  __syncthreads();
  pool_stage((uint4*)(A.out + (size_t)k * Y.fixlen), out4, chunks, lane);
}

// the labelled records of a call, cached per device (DevArr: grown, not shrunk)
struct PoolLabelDev {
  DevArr<signed char> canon;
  bool ensure(size_t bytes) { return canon.need(bytes, (size_t)1 << 20); }
};

inline size_t pool_label_lds(const Layout& Y) { return 2 * (size_t)Y.fixlen + (size_t)Y.N * Y.nz * sizeof(double); }

// false, with the text: the shape does not fit the kernel's LDS (decided before a device is asked for)
bool pool_label_fits(const Layout& Y, const char* name, std::string& err) {
  if (pool_label_lds(Y) <= POOL_LABEL_LDS_MAX) return true;
  err = std::string(name) + ": the fix record of this shape does not fit the LDS of pool_label_kernel twice beside a trajectory row";
  std::fprintf(stderr, "[miqp_gpu] %s (%zu bytes)\n", err.c_str(), pool_label_lds(Y));
  return false;
}
bool pool_label_set_lds(const Layout& Y) {
  HIP_OK(hipFuncSetAttribute((const void*)pool_label_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pool_label_lds(Y)));
  return true;
}

// the chunk fixed_chunk just ran (bc nodes in slots 0 .. bc - 1 of pool_fix, results and rows at res and Z) labelled into out, on the solver stream
bool pool_label_chunk(DevCtx& X, const Layout& Y, int n_inst, int bc, const miqp_fixed_result_c* res, const double* Z, signed char* out) {
  const DevBuf& B = X.B;
  PoolLabelArgs A;
  A.Y = Y; A.fix = B.pool_fix; A.Z = Z; A.res = res; A.batch_inst = B.batch_inst; A.inst_d = B.inst_d; A.inst_i = B.inst_i; A.out = out; A.bc = bc; A.n_inst = n_inst;
  hipLaunchKernelGGL(pool_label_kernel, dim3(bc), dim3(64), pool_label_lds(Y), X.stream, A);
  HIP_OK(hipGetLastError());
  return true;
}

// pool_label_byte over a whole record on the host: canon[0 .. fixlen)
void pool_label_host(const Layout& Y, const double* D, const int* T, const signed char* rec, const double* Z, signed char* canon) {
  std::memset(canon, 0xFF, (size_t)Y.fixlen);
  for (int k = 0; k < Y.C * Y.N; ++k) if (!pool_label_region_ok(Y, rec, k)) return;
  const int nbytes = pool_sites(pool_dims(Y)) * (Y.N - 1);
  for (int t = 0; t < nbytes; ++t) { int at = 0; const int v = pool_label_byte(Y, D, T, rec, Z, t, at); canon[at] = (signed char)v; }
}

}  // namespace

extern "C" {

int miqp_solver_canonical_labels(const miqp_solver_t* s, const signed char* decisions, const double* trajectories, int n, int via, signed char* canon) {
  if (!s || !s->has_inst || !decisions || !trajectories || !canon || n <= 0) return -1;
  if (via != 0 && via != 1) return -2;
  miqp_solver_t* one[1] = {const_cast<miqp_solver_t*>(s)};
  BatchShape bs = batch_layout(one, 1);
  if (!bs.ok) return -2;
  const Layout& Y = bs.Y; const size_t fl = (size_t)Y.fixlen, D = (size_t)Y.f_c2n, row = (size_t)Y.N * Y.nz;
  std::vector<double> Dt(Y.dstride); std::vector<int> T(Y.istride);
  compile_instance(s->inst, Y, Dt.data(), T.data());
  std::vector<signed char> fix(fl), lab(fl), one_fix;
  OwnedResults R(s->inst);
  int labelled = 0;
  for (int k = 0; k < n; ++k) {
    signed char* const dst = canon + (size_t)k * D;
    std::memset(dst, 0xFF, D);
    if (!decisions_in_range(s->inst, Y, T.data(), decisions + (size_t)k * D)) continue;
    std::fill(fix.begin(), fix.end(), (signed char)-1);
    std::memcpy(fix.data(), decisions + (size_t)k * D, D);
    bool ok = true;
    for (int q = 0; q < Y.C * Y.N; ++q) ok = ok && pool_label_region_ok(Y, fix.data(), q);
    if (!ok) continue;
    if (via == 0) pool_label_host(Y, Dt.data(), T.data(), fix.data(), trajectories + (size_t)k * row, lab.data());
    else {   // the record as fixed_hand_out completes it, then the two host functions
      for (auto& b : fix) if (b < 0) b = 0;
      fill_results(s->inst, Y, Dt.data(), T.data(), fix.data(), trajectories + (size_t)k * row, &R.r);
      (void)fix_from_results(s->inst, Y, T.data(), &R.r, one_fix);
      std::memcpy(lab.data(), one_fix.data(), fl);
    }
    std::memcpy(dst, lab.data(), D);
    labelled++;
  }
  return labelled;
}

int miqp_solver_canonical_decisions(miqp_solver_t* s, const signed char* decisions, int n, miqp_fixed_result_c* out, signed char* canon, int* best) {
  if (s) { s->drop_fixed_batch(); s->err.clear(); }
  if (!s || !s->has_inst || !decisions || !out || !canon || n <= 0) return -1;
  if (n > FB_CAP) return -5;
  const double t_call = wall_s();
  if (best) *best = -1;
  fixed_refuse(out, n);
  miqp_solver_t* one[1] = {s};
  BatchShape bs = batch_layout(one, 1);
  if (!bs.ok) return -2;
  const Layout& Y = bs.Y;
  const size_t fl = (size_t)Y.fixlen, D = (size_t)Y.f_c2n, row = (size_t)Y.N * Y.nz;
  std::memset(canon, 0xFF, (size_t)n * D);
  std::vector<double> Dt(Y.dstride); std::vector<int> T(Y.istride);
  compile_instance(s->inst, Y, Dt.data(), T.data());
  std::vector<int> where; where.reserve(n);
  for (int k = 0; k < n; ++k) if (decisions_in_range(s->inst, Y, T.data(), decisions + (size_t)k * D)) where.push_back(k);
  const int m = (int)where.size();
  if (m == 0) return 0;   // (nothing to run: no device is touched)
  if (!pool_label_fits(Y, "miqp_solver_canonical_decisions", s->err)) return -3;
  FixedCall call;
  if (call.open(one, 1, Y) != 0) return -3;
  PoolLabelDev& Q = call_dev<PoolLabelDev>(call.X->device);
  if (!Q.ensure((size_t)m * fl) || !pool_label_set_lds(Y)) return -3;
  std::vector<signed char> fix((size_t)m * fl, (signed char)-1);
  for (int c = 0; c < m; ++c) std::memcpy(fix.data() + (size_t)c * fl, decisions + (size_t)where[c] * D, D);
  const int first[2] = {0, n};
  // behind every chunk's fixed_chunk, while its records lie in pool_fix: the chunk's labels
  const FixedAfterChunk label = [&](int c0, int bc) {
    const FixedDev& F = call.dev();
    return pool_label_chunk(*call.X, Y, 1, bc, F.d_res + c0, F.d_Z + (size_t)c0 * row, Q.canon + (size_t)c0 * fl);
  };
  const int rc = fixed_answer(call, fix, std::vector<int>(m, 0), where, {0, m}, first, out, best, t_call, &label);
  if (rc != 0) return rc;
  std::vector<signed char> lab((size_t)m * fl);
  if (hipMemcpy(lab.data(), Q.canon, (size_t)m * fl, hipMemcpyDeviceToHost) != hipSuccess) return -3;
  for (int c = 0; c < m; ++c) std::memcpy(canon + (size_t)where[c] * D, lab.data() + (size_t)c * fl, D);
  return 0;
}

}  // extern "C"

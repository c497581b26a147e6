// certify.hip - a-posteriori certificate of delivered records against the raw big-M model (miqp_solver_certify, _certify_batch).
//
// What is evaluated is the materialised RawResults record the caller holds, not the incumbent of the branch and bound: the
// rows of cplexmodel/*.mod are generated on the fly (the row walker of raw_model.hpp, which also writes the .lp) from a
// compact parameter block of the host instance, one workgroup of 256 threads per record.  Included by miqp_gpu.hip.
//
// Kernel layout: the twelve continuous arrays of the record are staged in LDS once (12 x C x N doubles; a chunk with a
// record beyond CERT_LDS_DOUBLES runs the variant that reads them from global memory), then family by family the threads
// stride over the family's index space and keep a running (violation, row) maximum; a fixed xor-tree over the wavefront
// and a four-entry LDS step over the wavefronts end each family (ties: lower row).  The objective is summed the same way,
// in a fixed order.  One lane writes the struct.  No atomics, no scratch.
//
// Host side: records are packed on at most 16 host threads into pinned staging, uploaded in chunks on one stream while the
// kernel of the previous chunk runs on another; two staging and two device buffers of at most CERT_CHUNK_BYTES each, cached
// per device and never taken from the solver's pools.  The call holds the device lock of a solve and touches no solver context.
#pragma once
#include "raw_model.hpp"

namespace {

constexpr int CERT_NT = 256;
constexpr int CERT_LDS_DOUBLES = 3072;                 // 24 KB: 12 x C x N up to C x N = 256 (cfg5: 120)
constexpr size_t CERT_CHUNK_BYTES = (size_t)48 << 20;  // per buffer; two device buffers + the output stay below 256 MB
constexpr size_t CERT_BLOB_MAX = (size_t)112 << 20;    // a single record larger than this is refused

__device__ __forceinline__ void cert_wave_max(double& v, unsigned& row) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const double ov = __shfl_xor(v, d, 64); const unsigned orow = (unsigned)__shfl_xor((int)row, d, 64);
    if (ov > v || (ov == v && orow < row)) { v = ov; row = orow; }
  }
}
__device__ __forceinline__ double cert_wave_sum(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

template <bool STAGE>
__global__ __launch_bounds__(CERT_NT) void certify_kernel(const char* __restrict__ buf, miqp_certificate_c* __restrict__ out) {
  __shared__ double s_cont[STAGE ? CERT_LDS_DOUBLES : 1];
  __shared__ double s_v[4]; __shared__ unsigned s_r[4];
  __shared__ double s_fam[8]; __shared__ unsigned s_famrow[8];
  __shared__ double s_obj, s_int;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const size_t* off = (const size_t*)buf;
  CertView V; V.bind(buf + off[blockIdx.x]);
  if (STAGE) {
    const int n = 12 * V.Y.C * V.Y.N;
    for (int q = tid; q < n; q += CERT_NT) s_cont[q] = V.cont[q];
    V.cont = s_cont;
    __syncthreads();
  }
#pragma unroll
  for (int f = 0; f < 8; ++f) {
    CertMax m{0.0, -1};
    RawEval ev{V, m, 0.0, 0};
    raw_family(f, V, tid, CERT_NT, ev);
    double v = m.v; unsigned row = (unsigned)m.row;
    cert_wave_max(v, row);
    if (lane == 0) { s_v[wave] = v; s_r[wave] = row; }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < 4; ++w) if (s_v[w] > v || (s_v[w] == v && s_r[w] < row)) { v = s_v[w]; row = s_r[w]; }
      s_fam[f] = v; s_famrow[f] = row;
    }
    __syncthreads();
  }
  {
    double o = cert_wave_sum(cert_objective(V, tid, CERT_NT));
    double b = cert_int_infeas(V, tid, CERT_NT); unsigned dummy = 0;
    cert_wave_max(b, dummy);
    if (lane == 0) s_v[wave] = o;
    __syncthreads();
    if (tid == 0) s_obj = (s_v[0] + s_v[1]) + (s_v[2] + s_v[3]);
    __syncthreads();
    if (lane == 0) s_v[wave] = b;
    __syncthreads();
    if (tid == 0) s_int = fmax(fmax(s_v[0], s_v[1]), fmax(s_v[2], s_v[3]));
    __syncthreads();
  }
  if (tid == 0) {
    miqp_certificate_c c;
    double worst = 0.0; int wf = 0, wr = -1;
    for (int f = 0; f < 8; ++f) { c.family_violation[f] = s_fam[f]; if (s_fam[f] > worst) { worst = s_fam[f]; wf = f + 1; wr = (int)s_famrow[f]; } }
    c.max_violation = worst; c.objective = s_obj; c.max_int_infeas = s_int;
    c.worst_family = wf; c.worst_row = wf ? wr : -1; c.rows = V.base[8]; c.status = 0;
    out[blockIdx.x] = c;
  }
}

// ---------------------------------------------------------------------------------------------------------------- device cache
struct CertDev {
  hipStream_t s_up = nullptr, s_k = nullptr;
  hipEvent_t ev_up[2] = {}, ev_done[2] = {}, t_up0[2] = {}, t_up1[2] = {}, t_k0[2] = {}, t_k1[2] = {};
  DevArr<char, true> h_stage[2]; DevArr<char> d_blob[2];
  DevArr<miqp_certificate_c> d_out;
  bool streams = false;
  bool ensure(size_t bytes, size_t n_out) {
    if (!streams) {
      HIP_OK(hipStreamCreateWithFlags(&s_up, hipStreamNonBlocking)); HIP_OK(hipStreamCreateWithFlags(&s_k, hipStreamNonBlocking));
      for (int b = 0; b < 2; ++b) {
        HIP_OK(hipEventCreateWithFlags(&ev_up[b], hipEventDisableTiming)); HIP_OK(hipEventCreateWithFlags(&ev_done[b], hipEventDisableTiming));
        HIP_OK(hipEventCreate(&t_up0[b])); HIP_OK(hipEventCreate(&t_up1[b])); HIP_OK(hipEventCreate(&t_k0[b])); HIP_OK(hipEventCreate(&t_k1[b]));
      }
      streams = true;
    }
    for (int b = 0; b < 2; ++b) if (!h_stage[b].need(bytes, (size_t)1 << 20) || !d_blob[b].need(bytes, (size_t)1 << 20)) return false;
    return d_out.need(n_out, 256);
  }
};
double g_cert_timing[4] = {0, 0, 0, 0};   // of the last certify call of the process: host packing, upload, kernel, whole call (seconds)

struct CertJob { const HostInst* I; const miqp_raw_results_c* r; size_t bytes; };

void cert_no_solution(miqp_certificate_c& c) {
  const double nan = std::nan("");
  c.max_violation = nan; c.objective = nan; c.max_int_infeas = nan;
  for (int f = 0; f < 8; ++f) c.family_violation[f] = nan;
  c.worst_family = -1; c.worst_row = -1; c.rows = -1; c.status = 1;
}

// jobs -> out (one entry per job), on `device`.  err: why not.
bool certify_jobs(int device, const std::vector<CertJob>& jobs, miqp_certificate_c* out, std::string& err) {
  const double t_call = wall_s();
  const int n = (int)jobs.size();
  if (n == 0) return true;
  DevCtx* X = ctx_for_device(device);
  if (!X) { err = "no HIP device: a certificate is evaluated on the device only, the library has no host evaluation"; return false; }
  std::lock_guard<std::mutex> lk(X->mu);
  if (hipSetDevice(X->device) != hipSuccess) { err = "hipSetDevice failed"; return false; }
  // chunks of consecutive jobs
  size_t big = 0; for (const CertJob& j : jobs) big = std::max(big, j.bytes);
  if (big + 16 > CERT_BLOB_MAX) { err = "record too large for the certificate's staging buffers"; return false; }
  const size_t chunk_cap = std::max(CERT_CHUNK_BYTES, big + 4096);
  std::vector<int> start{0}; std::vector<size_t> need;
  {
    size_t used = 0; int cnt = 0;
    for (int k = 0; k < n; ++k) {
      const size_t add = jobs[k].bytes + 8;
      if (cnt > 0 && used + add + 16 > chunk_cap) { need.push_back(used + 16); start.push_back(k); used = 0; cnt = 0; }
      used += add; ++cnt;
    }
    need.push_back(used + 16);
    start.push_back(n);
  }
  const int nchunks = (int)need.size();
  CertDev& G = call_dev<CertDev>(X->device);
  if (!G.ensure(*std::max_element(need.begin(), need.end()), (size_t)n)) { err = "device or pinned memory for the certificate could not be allocated"; return false; }
  double pack_s = 0.0; float up_ms = 0.0f, k_ms = 0.0f; bool used_buf[2] = {false, false};
  auto harvest = [&](int b) {
    float a = 0, c = 0;
    if (hipEventElapsedTime(&a, G.t_up0[b], G.t_up1[b]) == hipSuccess) up_ms += a;
    if (hipEventElapsedTime(&c, G.t_k0[b], G.t_k1[b]) == hipSuccess) k_ms += c;
  };
  for (int ch = 0; ch < nchunks; ++ch) {
    const int b = ch & 1, k0 = start[ch], cnt = start[ch + 1] - k0;
    if (used_buf[b]) { if (hipEventSynchronize(G.ev_done[b]) != hipSuccess) { err = "certificate kernel failed"; return false; } harvest(b); }
    const double t0 = wall_s();
    char* H = G.h_stage[b]; size_t* off = (size_t*)H;
    size_t o = ((size_t)cnt * 8 + 15) & ~(size_t)15; bool stage = true;
    for (int k = 0; k < cnt; ++k) {
      off[k] = o; o += jobs[k0 + k].bytes;
      if (12 * jobs[k0 + k].I->C * jobs[k0 + k].I->N > CERT_LDS_DOUBLES) stage = false;
    }
    const int nth = std::max(1, std::min({16, (int)std::thread::hardware_concurrency(), cnt / 32}));
    std::atomic<int> next{0};
    auto work = [&] { for (int k = next.fetch_add(1); k < cnt; k = next.fetch_add(1)) { cert_pack_params(*jobs[k0 + k].I, H + off[k]); cert_pack_record(*jobs[k0 + k].I, *jobs[k0 + k].r, H + off[k]); } };
    if (nth <= 1) work();
    else { std::vector<std::thread> th; for (int t = 0; t < nth; ++t) th.emplace_back(work); for (auto& t : th) t.join(); }
    pack_s += wall_s() - t0;
    bool ok = hipEventRecord(G.t_up0[b], G.s_up) == hipSuccess;
    ok = ok && hipMemcpyAsync(G.d_blob[b], H, o, hipMemcpyHostToDevice, G.s_up) == hipSuccess;
    ok = ok && hipEventRecord(G.t_up1[b], G.s_up) == hipSuccess && hipEventRecord(G.ev_up[b], G.s_up) == hipSuccess;
    ok = ok && hipStreamWaitEvent(G.s_k, G.ev_up[b], 0) == hipSuccess && hipEventRecord(G.t_k0[b], G.s_k) == hipSuccess;
    if (ok) {
      if (stage) hipLaunchKernelGGL(certify_kernel<true>, dim3(cnt), dim3(CERT_NT), 0, G.s_k, (const char*)G.d_blob[b], G.d_out + k0);
      else hipLaunchKernelGGL(certify_kernel<false>, dim3(cnt), dim3(CERT_NT), 0, G.s_k, (const char*)G.d_blob[b], G.d_out + k0);
      ok = hipGetLastError() == hipSuccess;
    }
    ok = ok && hipEventRecord(G.t_k1[b], G.s_k) == hipSuccess && hipEventRecord(G.ev_done[b], G.s_k) == hipSuccess;
    if (!ok) { (void)hipStreamSynchronize(G.s_up); (void)hipStreamSynchronize(G.s_k); err = "launch of the certificate kernel failed (no kernel image for this device?)"; return false; }
    used_buf[b] = true;
  }
  if (hipStreamSynchronize(G.s_k) != hipSuccess || hipStreamSynchronize(G.s_up) != hipSuccess) { err = "certificate kernel failed"; return false; }
  for (int b = 0; b < 2; ++b) if (used_buf[b]) harvest(b);
  if (hipMemcpy(out, G.d_out, (size_t)n * sizeof(miqp_certificate_c), hipMemcpyDeviceToHost) != hipSuccess) { err = "copy of the certificates failed"; return false; }
  g_cert_timing[0] = pack_s; g_cert_timing[1] = up_ms * 1e-3; g_cert_timing[2] = k_ms * 1e-3; g_cert_timing[3] = wall_s() - t_call;
  return true;
}

bool cert_candidate_ok(const miqp_raw_results_c& r) {
  const void* need[] = {r.u_x, r.u_y, r.pos_x, r.vel_x, r.acc_x, r.pos_y, r.vel_y, r.acc_y, r.pos_x_front_UB, r.pos_x_front_LB, r.pos_y_front_UB, r.pos_y_front_LB,
                        r.notWithinEnvironmentRear, r.notWithinEnvironmentFrontUbUb, r.notWithinEnvironmentFrontLbUb, r.notWithinEnvironmentFrontUbLb, r.notWithinEnvironmentFrontLbLb,
                        r.active_region, r.region_change_not_allowed_x_positive, r.region_change_not_allowed_y_positive, r.region_change_not_allowed_x_negative,
                        r.region_change_not_allowed_y_negative, r.region_change_not_allowed_combined, r.deltacc, r.deltacc_front, r.car2car_collision, r.slackvars,
                        r.slackvarsObstacle, r.slackvarsObstacle_front};
  for (const void* q : need) if (!q) return false;
  return true;
}

}  // namespace

extern "C" {

int miqp_gpu_certificate_size(void) { return (int)sizeof(miqp_certificate_c); }

int miqp_solver_certify_batch(miqp_solver_t* const* solvers, int n, miqp_certificate_c* out) {
  if (!solvers || n < 0 || !out) return -1;
  if (n == 0) return 0;
  for (int k = 0; k < n; ++k) if (!solvers[k]) return -1;
  (void)miqp_solver_materialize_results(solvers, n, 16);   // the records the callers will be handed: built once, kept in the handles
  std::vector<CertJob> jobs; std::vector<int> where; jobs.reserve(n); where.reserve(n);
  for (int k = 0; k < n; ++k) {
    miqp_solver* s = solvers[k];
    if (!s->has_inst || !s->has_sol || !s->rescache) { cert_no_solution(out[k]); continue; }
    jobs.push_back({&s->inst, &s->rescache->r, cert_blob_bytes(s->inst)}); where.push_back(k);
  }
  if (jobs.empty()) return 0;
  std::vector<miqp_certificate_c> tmp(jobs.size());
  std::string err;
  if (!certify_jobs(solvers[where[0]]->opts.device, jobs, tmp.data(), err)) {
    for (int k : where) solvers[k]->err = err;
    std::fprintf(stderr, "[miqp_gpu] %s\n", err.c_str());
    return -4;
  }
  for (size_t q = 0; q < jobs.size(); ++q) out[where[q]] = tmp[q];
  return 0;
}

int miqp_solver_certify(miqp_solver_t* s, const miqp_raw_results_c* candidate, miqp_certificate_c* out) {
  if (!s || !out) return -1;
  if (!candidate) { miqp_solver_t* one[1] = {s}; return miqp_solver_certify_batch(one, 1, out); }
  if (!s->has_inst) return -1;
  if (!cert_candidate_ok(*candidate)) return -2;
  if (!dims_match(*candidate, s->inst)) return -3;   // a record of another shape is never indexed
  std::vector<CertJob> jobs{{&s->inst, candidate, cert_blob_bytes(s->inst)}};
  std::string err;
  if (!certify_jobs(s->opts.device, jobs, out, err)) { s->err = err; std::fprintf(stderr, "[miqp_gpu] %s\n", err.c_str()); return -4; }
  return 0;
}

int miqp_gpu_certify_last_timing(double* out4) {
  if (!out4) return -1;
  for (int k = 0; k < 4; ++k) out4[k] = g_cert_timing[k];
  return 0;
}

}  // extern "C"

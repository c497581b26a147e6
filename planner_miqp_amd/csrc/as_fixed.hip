// as_fixed.hip - fix records through the ACTIVE-SET launches, one node at a time: a diagnostic entry (miqp_solver_solve_fixed_as, _fixed_as_record)
// for the tests that hold as_onchip_kernel against the oracle node by node (tests/test_as_node_gpu.py).  DESIGN.md 4.  Host code only: no kernel
// of its own, nothing a solve runs.
//
// A search forgives the active-set kernel almost anything - a node it cannot finish goes to the interior point a round later, a parent's M that
// no longer fits starts the node cold, and the incumbent that is returned has been polished by the interior point.  Here a fix record is ONE node
// of ONE launch of NODE_KERNEL[NK_AS] or NODE_KERNEL[NK_AS_BIG], with the LDS size and grid the round planner gives that launch, started cold or
// from the final active set of an earlier node of the same call, with a cutoff of the caller's choosing, and what the kernel decided is read back
// as it wrote it: verdict, objective, bound allowance, violation, steps, final active set, and the 32 counters of as_stats.
//
// Built on FixedCall (fixed_chain.hip): one lock, one context, the tables uploaded once; node k of the call is batch slot k and slot k of pool_fix
// (one chunk: at most FB_CHUNK records, so that a parent's slot is never overwritten before its children have read it).  What the search does
// for a child in eval_kernel - copy batch_A of the parent into pool_A of the child's record, batch_Mtag into pool_Mtag, a depth of at least 1 -
// is done here by copies on the solver stream between the launches.  The records run in generations, all cold ones first; within a generation
// the nodes of one cutoff value share a launch.  Which nodes a launch takes is said by the split byte batch_large, as in a round: the byte of
// the launch's own class on its nodes, the other one on the rest.
#pragma once

namespace {

constexpr int FA_CAP = FB_CHUNK;   // records per call

// the launch of the standard (block 0) or larger (block 1) active-set kernel over bc batch slots, as plan_node_launches sizes it in a concurrent
// round of this context.  false: the plan has no such launch (the context has no larger block)
struct AsLaunch { NodeKernelFn fn; int grid; size_t lds; };
bool as_fixed_launch(const DevCtx& X, int block, int bc, AsLaunch& out) {
  static const int unknown[3] = {-1, -1, -1};
  const ProcessSwitches& ps = process_switches();
  const PlanCaps caps = {X.oc_grid, X.ocb_grid, X.probe_grid, X.ipm_grid_max, true, true, true, true, true, true};
  const PlanSwitches sw = {ps.big_grid_cap, ps.big_w1, ps.big_w2, read_call_switches().big_pad, X.B.as_chunk, X.B.as_quota};
  const RoundPlan P = plan_node_launches(X.Y, caps, sw, unknown, bc, true, 0);
  const int kind = block ? NK_AS_BIG : NK_AS;
  for (int i = 0; i < P.n; ++i)
    if (P.l[i].kind == kind && NODE_KERNEL[kind][X.Y.C - 1]) { out = AsLaunch{NODE_KERNEL[kind][X.Y.C - 1], P.l[i].grid, (size_t)P.l[i].lds}; return true; }
  return false;
}

struct AsFixedHost {   // what comes back from the device, per slot
  std::vector<int> ok, it; std::vector<double> obj, viol, bound, Z; std::vector<unsigned short> A; std::vector<unsigned char> big;
  unsigned long long stats[32];
};

// The device part.  fix: n records; depth[k]: the depth word of node k; kcut[k]: the cutoff in the kernel's units (has[k] != 0), launch[q]: the
// nodes of launch q in the order of the launches.  false: HIP error
bool as_fixed_device(FixedCall& call, const AsLaunch& L, int block, int n, const std::vector<signed char>& fix, const int* start, const std::vector<int>& depth,
                     const std::vector<char>& has, const std::vector<double>& kcut, const std::vector<std::vector<int>>& launch, AsFixedHost& H) {
  DevCtx& X = *call.X; DevBuf& B = X.B; hipStream_t st = X.stream; const Layout& Y = call.Y;
  const size_t fl = (size_t)Y.fixlen, row = (size_t)Y.N * Y.nz;
  const double zero_d = 0.0, none = 1e300;
  HIP_OK(hipMemcpyAsync(B.pool_fix, fix.data(), (size_t)n * fl, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemsetAsync(B.batch_inst, 0, (size_t)n * 4, st));
  HIP_OK(hipMemsetD32Async((hipDeviceptr_t)B.batch_count, n, 1, st));
  HIP_OK(hipMemcpyAsync(B.batch_depth, depth.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
  // nothing of an earlier call stays in the slots: the size marks, the verdicts (-1: no launch took the node), the active sets and their tags
  HIP_OK(hipMemsetAsync(B.pool_big, 0, (size_t)n, st));
  HIP_OK(hipMemsetAsync(B.batch_ok, 0xFF, (size_t)n * 4, st));
  if (X.as_batch_A) HIP_OK(hipMemsetAsync(X.as_batch_A, 0xFF, (size_t)n * 128, st));
  if (B.ring_M) HIP_OK(hipMemsetAsync(B.batch_Mtag, 0, (size_t)n * 8, st));
  HIP_OK(hipMemsetAsync(B.as_stats, 0, 256, st));
  HIP_OK(hipMemsetAsync(B.inst_nodes, 0, 8, st)); HIP_OK(hipMemsetAsync(B.inst_iters, 0, 8, st));
  // the incumbent words of the one instance: the kernel's test reads min(inc_key, inc_ext) - gap * (...) - inst_const, so with no key, no gap and
  // no constant it sees inc_ext as it is
  HIP_OK(hipMemsetAsync(B.inc_key, 0xFF, 8, st));
  HIP_OK(hipMemcpyAsync(B.inst_gap, &zero_d, 8, hipMemcpyHostToDevice, st)); HIP_OK(hipMemcpyAsync(B.inst_const, &zero_d, 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipStreamSynchronize(st));
  DevBuf Bp = B;
  Bp.ws_on = 0; Bp.batch_A = X.as_batch_A; Bp.pool_A = X.as_pool_A; Bp.cls_list = nullptr; Bp.cls_take = 0; Bp.as_probe_first = 0;
  Bp.ovf_mode = 0; Bp.as_split = 0; Bp.skip_probes = 0; Bp.bounce = 1;
  std::vector<unsigned char> large(n);
  for (const std::vector<int>& g : launch) {
    if (g.empty()) continue;
    const int k0 = g[0];
    // the split byte: this launch's class on its nodes, the other class on the rest
    std::fill(large.begin(), large.end(), (unsigned char)(block ? 0 : 1));
    for (int k : g) large[k] = (unsigned char)(block ? 1 : 0);
    HIP_OK(hipMemcpyAsync(B.batch_large, large.data(), (size_t)n, hipMemcpyHostToDevice, st));
    for (int k : g) {   // a child: the parent's final active set and the tag of its M into the child's record, as eval_kernel writes them
      if (start[k] == -1) continue;
      const bool keepM = start[k] >= 0; const int p = keepM ? start[k] : -(start[k] + 2);
      HIP_OK(hipMemcpyAsync(X.as_pool_A + (size_t)k * 64, X.as_batch_A + (size_t)p * 64, 128, hipMemcpyDeviceToDevice, st));
      if (B.ring_M) {
        if (keepM) HIP_OK(hipMemcpyAsync(B.pool_Mtag + k, B.batch_Mtag + p, 8, hipMemcpyDeviceToDevice, st));
        else HIP_OK(hipMemsetAsync(B.pool_Mtag + k, 0, 8, st));
      }
    }
    Bp.use_cutoff = has[k0] ? 1 : 0;
    HIP_OK(hipMemcpyAsync(B.inc_ext, has[k0] ? &kcut[k0] : &none, 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemsetAsync(Bp.work_counter, 0, 4, st));
    hipLaunchKernelGGL(L.fn, dim3(L.grid), dim3(64), L.lds, st, Bp);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(st));   // (large and the cutoff word are read from host memory by the copies above)
  }
  H.ok.resize(n); H.it.resize(n); H.obj.resize(n); H.viol.resize(n); H.bound.resize(n); H.Z.resize((size_t)n * row); H.A.assign((size_t)n * 64, 0xFFFFu); H.big.resize(n);
  HIP_OK(hipMemcpyAsync(H.ok.data(), B.batch_ok, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(H.it.data(), B.batch_it, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(H.obj.data(), B.batch_obj, (size_t)n * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(H.viol.data(), B.batch_viol, (size_t)n * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(H.bound.data(), B.batch_bound, (size_t)n * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(H.Z.data(), B.batch_Z, (size_t)n * row * 8, hipMemcpyDeviceToHost, st));
  if (X.as_batch_A) HIP_OK(hipMemcpyAsync(H.A.data(), X.as_batch_A, (size_t)n * 128, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(H.big.data(), B.pool_big, (size_t)n, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(H.stats, B.as_stats, 256, hipMemcpyDeviceToHost, st));
  // what the next call of any kind expects to find: no incumbent, no marks, no depth words, every slot of the one class
  HIP_OK(hipMemcpyAsync(B.inc_ext, &none, 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemsetAsync(B.pool_big, 0, (size_t)n, st)); HIP_OK(hipMemsetAsync(B.batch_large, 0, (size_t)n, st)); HIP_OK(hipMemsetAsync(B.batch_depth, 0, (size_t)n * 4, st));
  HIP_OK(hipMemsetAsync(B.as_stats, 0, 256, st));
  HIP_OK(hipStreamSynchronize(st)); HIP_OK(hipGetLastError());
  return true;
}

void as_fixed_refuse(miqp_as_node_c* out, int n) {
  for (int k = 0; k < n; ++k) { out[k].status = -1; out[k].steps = 0; out[k].active = 0; out[k].reserved = 0; out[k].objective = out[k].bound = out[k].violation = std::nan(""); }
}

}  // namespace

extern "C" {

int miqp_gpu_as_node_size(void) { return (int)sizeof(miqp_as_node_c); }

int miqp_solver_solve_fixed_as(miqp_solver_t* s, const miqp_raw_results_c* const* fixed, int n, const int* start, int block, const double* cutoff,
                               miqp_as_node_c* out, unsigned long long* info32) {
  if (!s || !s->has_inst || !fixed || !out || n <= 0 || (block != 0 && block != 1)) { if (s) s->err = "solve_fixed_as: invalid arguments or no instance"; return -1; }
  if (n > FA_CAP) { s->err = "solve_fixed_as: more records than one launch group holds"; return -5; }
  s->err.clear();
  as_fixed_refuse(out, n);
  if (info32) std::memset(info32, 0, 256);
  miqp_solver_t* one[1] = {s};
  BatchShape bs = batch_layout(one, 1);
  if (!bs.ok) { s->err = bs.err; return -2; }
  const Layout& Y = bs.Y;
  if (!miqp::as_shape_ok(Y.C, Y.N)) { s->err = "solve_fixed_as: the shape has no active-set launches (one or two cars, up to 20 steps)"; return -6; }
  if (knob_off(KNOB_P("MIQP_AS"))) { s->err = "solve_fixed_as: the active-set launches are switched off (MIQP_AS=0)"; return -7; }
  std::vector<int> gen(n, 0), depth(n, 0);
  for (int k = 0; k < n && start; ++k) {
    if (start[k] == -1) continue;
    const int p = start[k] >= 0 ? start[k] : -(start[k] + 2);
    if (p >= k) { s->err = "solve_fixed_as: node " + std::to_string(k) + " names node " + std::to_string(p) + " as its start; a start lies before its node"; return -8; }
    gen[k] = gen[p] + 1; depth[k] = 1 << 6;
  }
  const size_t fl = (size_t)Y.fixlen;
  std::vector<double> D(Y.dstride); std::vector<int> T(Y.istride);
  compile_instance(s->inst, Y, D.data(), T.data());
  std::vector<signed char> fix((size_t)n * fl), one_fix;
  std::vector<double> soft(n, 0.0);
  for (int k = 0; k < n; ++k) {
    if (!fixed[k] || !fixed_record_ok(*fixed[k]) || !dims_match(*fixed[k], s->inst) || !fix_from_results(s->inst, Y, T.data(), fixed[k], one_fix)) {
      s->err = "solve_fixed_as: record " + std::to_string(k) + " is refused (NULL, a NULL array in it, or other sizes than the instance)"; return -4;
    }
    std::memcpy(fix.data() + (size_t)k * fl, one_fix.data(), fl);
    // the price of the points the record ignores, as miqp_solver_solve_fixed charges it (a rounded product)
    int nign = 0; for (int q = 0; q < Y.C * Y.O * Y.N * 5; ++q) nign += one_fix[Y.f_obs + q] >= Y.L;
    volatile double pr = nign > 0 ? (double)nign * D[Y.d_misc + 1] : 0.0;
    soft[k] = pr;
  }
  s->drop_fixed_batch();   // (every refusal above leaves what an earlier call kept on the handle)
  FixedCall call;
  if (call.open(one, 1, Y) != 0) { s->err = "solve_fixed_as: no device, no kernel image or a HIP error"; return -3; }
  DevCtx& X = *call.X;
  AsLaunch L{};
  if (!X.as_cap || !as_fixed_launch(X, block, n, L) || L.grid < 1) { s->err = "solve_fixed_as: the device context has no launch of that block for this shape"; return -9; }
  bool any_start = false; for (int k = 0; k < n; ++k) any_start = any_start || depth[k] != 0;
  if (any_start && (!X.as_batch_A || !X.as_pool_A || X.B.z_cap < n)) { s->err = "solve_fixed_as: the device context keeps no active sets for starts"; return -9; }
  // the launches: generation by generation, within one the nodes of one cutoff value together (in the kernel's units: without the constants
  // that the returned objective carries)
  const double cobj = call.cobj[0];
  std::vector<char> has(n, 0); std::vector<double> kcut(n, 0.0);
  std::map<std::tuple<int, int, unsigned long long>, std::vector<int>> groups;
  for (int k = 0; k < n; ++k) {
    unsigned long long bits = 0ull;
    if (cutoff && cutoff[k] == cutoff[k] && cutoff[k] < 1e299) { has[k] = 1; kcut[k] = cutoff[k] - (cobj + soft[k]); std::memcpy(&bits, &kcut[k], 8); }
    groups[std::make_tuple(gen[k], (int)has[k], bits)].push_back(k);
  }
  std::vector<std::vector<int>> launch;
  for (auto& g : groups) launch.push_back(g.second);
  std::vector<int> st_(n, -1); if (start) st_.assign(start, start + n);
  AsFixedHost H;
  if (!as_fixed_device(call, L, block, n, fix, st_.data(), depth, has, kcut, launch, H)) { (void)hipStreamSynchronize(X.stream); s->err = "solve_fixed_as: HIP error"; return -3; }
  const size_t row = (size_t)Y.N * Y.nz;
  int lost = 0;
  s->fb_n = n; s->fb_slot.assign(n, -1);
  for (int k = 0; k < n; ++k) {
    miqp_as_node_c& o = out[k];
    const int ok = H.ok[k];
    if (ok == 5) { o.status = (H.big[k] & 4) ? 4 : 3; continue; }
    if (ok != 1 && ok != 2) { ++lost; continue; }
    const double konst = cobj + soft[k];
    o.status = ok == 2 ? 2 : (H.viol[k] > FEAS_TOL ? 1 : 0);
    o.steps = H.it[k];
    for (int q = 0; q < 64; ++q) o.active += H.A[(size_t)k * 64 + q] != 0xFFFFu ? 1 : 0;
    o.objective = H.obj[k] + konst; o.bound = o.objective - H.bound[k]; o.violation = H.viol[k];
    if (o.status == 0) s->fb_slot[k] = k;
  }
  s->fb_Z.assign(H.Z.begin(), H.Z.begin() + (size_t)n * row); s->fb_fix = fix;
  if (info32) std::memcpy(info32, H.stats, 256);
  if (lost) { s->err = "solve_fixed_as: " + std::to_string(lost) + " nodes were taken by no launch"; return -3; }
  return 0;
}

int miqp_solver_fixed_as_record(miqp_solver_t* s, int k, miqp_raw_results_c* out) { return miqp_solver_fixed_batch_record(s, k, out); }

}  // extern "C"

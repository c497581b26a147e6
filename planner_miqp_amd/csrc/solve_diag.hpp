// solve_diag.hpp - the diagnostics of a solve: traces, the replay timer, the open-list dump and the printers of the profile and statistics counters.
//
// Not a header of its own right: miqp_gpu.hip includes it once, inside its anonymous namespace and behind launch_ipm_batch (one translation unit;
// DevCtx, DevBuf, HIP_OK and the launch helpers are those of the including file).  Each function is one guarded call in the round loop or behind it:
// switched off it costs nothing, switched on it adds the synchronisations and copies written here and nothing else.  The output formats are
// compared between runs and builds (MIQP_TRACE was made for diffing): they do not change.
#pragma once

// MIQP_DEBUG_SYNC: synchronise and report after a kernel group of the round (fault localisation)
inline void debug_sync(hipStream_t st, int round, const char* stage, int nodes = -1) {
  hipError_t e_ = hipStreamSynchronize(st);
  if (nodes >= 0) std::fprintf(stderr, "[dbg] round %d %s (%d nodes): %s\n", round, stage, nodes, hipGetErrorString(e_));
  else std::fprintf(stderr, "[dbg] round %d %s: %s\n", round, stage, hipGetErrorString(e_));
}

// MIQP_TRACE: what the selection picked (list bound, depth word), the incumbent it pruned with, its mode
inline bool trace_selection(const DevCtx& X, int rounds, int bc) {
  const DevBuf& B = X.B;
  std::vector<double> sb(bc); std::vector<int> sd(bc); double io_ = 0; int md_ = 0;
  HIP_OK(hipMemcpy(sb.data(), B.batch_bound, (size_t)bc * 8, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(sd.data(), B.batch_depth, (size_t)bc * 4, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(&io_, B.inc_obj, 8, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(&md_, B.inst_mode, 4, hipMemcpyDeviceToHost));
  std::vector<int> ord(bc); for (int k = 0; k < bc; ++k) ord[k] = k;
  std::sort(ord.begin(), ord.end(), [&](int a, int b) { return sd[a] != sd[b] ? sd[a] > sd[b] : sb[a] < sb[b]; });
  std::fprintf(stderr, "[sel] r%d mode %d incumbent %a:", rounds, md_, io_);
  for (int k : ord) std::fprintf(stderr, " %d.%d/%a", sd[k] >> 6, sd[k] & 63, sb[k]);
  std::fprintf(stderr, "\n");
  return true;
}

// MIQP_TRACE: the solved batch of the round in an order that does not depend on the batch slots, for diffing two runs
inline bool trace_batch(const DevCtx& X, int rounds, int bc) {
  const DevBuf& B = X.B; hipStream_t st = X.stream;
  HIP_OK(hipStreamSynchronize(st));
  if (X.stream2) HIP_OK(hipStreamSynchronize(X.stream2));
  std::vector<int> hd(bc), hi(bc), hk(bc); std::vector<double> ho(bc), hb(bc), hv(bc);
  HIP_OK(hipMemcpy(hd.data(), B.batch_depth, bc * 4, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(hi.data(), B.batch_it, bc * 4, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(hk.data(), B.batch_ok, bc * 4, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(ho.data(), B.batch_obj, bc * 8, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(hb.data(), B.batch_bound, bc * 8, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(hv.data(), B.batch_viol, bc * 8, hipMemcpyDeviceToHost));
  std::vector<int> ord(bc); for (int k = 0; k < bc; ++k) ord[k] = k;
  std::sort(ord.begin(), ord.end(), [&](int a, int b) { return hd[a] != hd[b] ? hd[a] < hd[b] : (ho[a] != ho[b] ? ho[a] < ho[b] : hi[a] < hi[b]); });
  { int oc_ = 0, fc_ = 0, tk_ = 0, dm_ = 0; double nt_ = 0;
    HIP_OK(hipMemcpy(&oc_, B.open_count, 4, hipMemcpyDeviceToHost)); if (B.far_cap > 0) HIP_OK(hipMemcpy(&fc_, B.far_count, 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(&nt_, B.near_thr, 8, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(&tk_, B.slot_take, 4, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(&dm_, B.slot_demand, 4, hipMemcpyDeviceToHost));
    std::fprintf(stderr, "[lists] r%d batch %d: near list after selection %d, far tier %d, near_thr %g, share of the next round %d, demand %d\n", rounds, bc, oc_, fc_, nt_, tk_, dm_); }
  for (int k : ord) std::fprintf(stderr, "[trace] r%d depth %d.%d ok %d it %d obj %a bound %a viol %.3e\n", rounds, hd[k] >> 6, hd[k] & 63, hk[k], hi[k], ho[k], hb[k], hv[k]);
  return true;
}

// MIQP_LAUNCH_TRACE: the two interior point launches of the round apart, and what the memory-backed one had to solve
inline bool trace_launches(const DevCtx& X, int rounds, int bc, size_t nev) {
  const DevBuf& B = X.B; hipStream_t st = X.stream;
  HIP_OK(hipStreamSynchronize(st));
  float m1 = 0, m2 = 0; HIP_OK(hipEventElapsedTime(&m1, X.ipm_ev[nev], X.ev_mid)); HIP_OK(hipEventElapsedTime(&m2, X.ev_mid, X.ipm_ev[nev + 1]));
  int oc = 0; HIP_OK(hipMemcpy(&oc, B.ovf_count, 4, hipMemcpyDeviceToHost));
  std::vector<int> ol(std::max(oc, 1)), hit(bc), hdw(bc), hok(bc);
  if (oc > 0) HIP_OK(hipMemcpy(ol.data(), B.ovf_list, (size_t)oc * 4, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(hit.data(), B.batch_it, (size_t)bc * 4, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(hdw.data(), B.batch_depth, (size_t)bc * 4, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(hok.data(), B.batch_ok, (size_t)bc * 4, hipMemcpyDeviceToHost));
  int np = 0, mxp = 0, mxo = 0, mxc = 0; long long sp = 0, so = 0, sc = 0;
  for (int q = 0; q < oc; ++q) { const int k = ol[q]; if ((hdw[k] & 63) == 63 && (hdw[k] >> 6) >= 1) { np++; sp += hit[k]; mxp = std::max(mxp, hit[k]); } else { so += hit[k]; mxo = std::max(mxo, hit[k]); } }
  std::vector<char> isov(bc, 0); for (int q = 0; q < oc; ++q) isov[ol[q]] = 1;
  for (int k = 0; k < bc; ++k) if (!isov[k]) { sc += hit[k]; mxc = std::max(mxc, hit[k]); }
  // (with the concurrent launches of the large nodes - the default - the first time is the standard launch incl. its wait for room, the
  // second the wait for the second stream after it, and the node split below is empty: nothing is handed on behind the standard launch;
  // MIQP_CONCURRENT_BIG=0 MIQP_OC_BIG=0 gives the two launches of the first half of round 3 apart)
  std::fprintf(stderr, "[launch] round %d nodes %d: on-chip %.2f ms (%d nodes, mean it %.1f, max %d); behind it %.2f ms: %d probes (mean it %.1f, max %d), %d others (mean it %.1f, max %d)\n",
               rounds, bc, m1, bc - oc, (double)sc / std::max(1, bc - oc), mxc, m2, np, (double)sp / std::max(1, np), mxp, oc - np, (double)so / std::max(1, oc - np), mxo);
  return true;
}

// MIQP_REPLAY=k: the first batch that is at least half full (from round MIQP_REPLAY_ROUND on) is solved k more times under a timer - the kernels
// only read and write batch slots; with -DMIQP_ABLATE followed by the cost map of the on-chip kernel
inline bool replay_batch(DevCtx& X, int bc) {
  static int replay = process_switches().replay;
  if (replay <= 0) return true;
  const DevBuf& B = X.B; hipStream_t st = X.stream; const Layout& Y = X.Y; (void)Y;
  hipEvent_t e0, e1; HIP_OK(hipEventCreate(&e0)); HIP_OK(hipEventCreate(&e1));
  HIP_OK(hipEventRecord(e0, st));
  for (int r = 0; r < replay; ++r) launch_ipm_batch(X, B, bc, st);
  HIP_OK(hipEventRecord(e1, st)); HIP_OK(hipStreamSynchronize(st));
  float ms = 0; HIP_OK(hipEventElapsedTime(&ms, e0, e1));
  std::vector<int> its(bc); HIP_OK(hipMemcpy(its.data(), B.batch_it, (size_t)bc * 4, hipMemcpyDeviceToHost));
  long long tot = 0; for (int v : its) tot += v;
  std::fprintf(stderr, "[miqp_gpu replay] %d nodes, %lld node-iterations: %.3f ms per pass, %.1f ns per node-iteration\n", bc, tot, ms / replay, 1e6 * ms / replay / (double)tot);
#ifdef MIQP_ABLATE
  if (X.oc_grid > 0 && Y.C == 2) {   // cost map of the on-chip kernel: the same batch, 15 iterations per node, parts switched off
    const size_t l_oc = (size_t)oc_lds_layout(Y.N, Y.fixlen).total;
    auto run = [&](auto kern, int mask) {
      HIP_OK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)l_oc));
      auto once = [&] { (void)hipMemsetAsync(B.work_counter, 0, 4, st); (void)hipMemsetAsync(B.ovf_count, 0, 4, st); hipLaunchKernelGGL(kern, dim3(std::min(bc, X.oc_grid)), dim3(64), l_oc, st, B); };
      once(); HIP_OK(hipEventRecord(e0, st)); for (int r = 0; r < 3; ++r) once(); HIP_OK(hipEventRecord(e1, st)); HIP_OK(hipStreamSynchronize(st));
      float m2 = 0; HIP_OK(hipEventElapsedTime(&m2, e0, e1));
      std::fprintf(stderr, "[miqp_gpu ablate] mask %4d: %.3f ms per pass of %d nodes x 15 iterations = %.1f ns per node-iteration\n", mask, m2 / 3, bc, 1e6 * m2 / 3 / (bc * 15.0));
      return true;
    };
    run(ipm_onchip_kernel<2, OC_NSL, 1>, 1); run(ipm_onchip_kernel<2, OC_NSL, 3>, 3); run(ipm_onchip_kernel<2, OC_NSL, 5>, 5); run(ipm_onchip_kernel<2, OC_NSL, 9>, 9);
    run(ipm_onchip_kernel<2, OC_NSL, 17>, 17); run(ipm_onchip_kernel<2, OC_NSL, 33>, 33); run(ipm_onchip_kernel<2, OC_NSL, 65>, 65); run(ipm_onchip_kernel<2, OC_NSL, 129>, 129);
    run(ipm_onchip_kernel<2, OC_NSL, 257>, 257); run(ipm_onchip_kernel<2, OC_NSL, 513>, 513); run(ipm_onchip_kernel<2, OC_NSL, 1023>, 1023);
    run(ipm_onchip_kernel<2, OC_NSL, 1025>, 1025);   // the MFMA form of P [A B], [A B]' T on the model's column order
    launch_ipm_batch(X, B, bc, st);   // the replays clobbered the batch results: solve the real batch again
  }
#endif
  replay = 0;
  return true;
}

// progress of the first instance (opts.verbose == 1, every 25 rounds)
inline bool print_progress(const DevCtx& X, double t, int rounds, long long launched_nodes, double const0) {
  const DevBuf& B = X.B; hipStream_t st = X.stream;
  double lb0 = 0, io0 = 0; int oc0 = 0; unsigned long long k0 = 0;
  HIP_OK(hipMemcpyAsync(&lb0, B.lower_bound, 8, hipMemcpyDeviceToHost, st)); HIP_OK(hipMemcpyAsync(&io0, B.inc_obj, 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(&oc0, B.open_count, 4, hipMemcpyDeviceToHost, st)); HIP_OK(hipMemcpyAsync(&k0, B.inc_key, 8, hipMemcpyDeviceToHost, st));
  int fc0 = 0; HIP_OK(hipMemcpyAsync(&fc0, B.far_count, 4, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  std::fprintf(stderr, "[miqp_gpu] t %.2f s round %d nodes %lld: instance 0 bound %.4f incumbent %.4f open %d + %d\n", t, rounds, launched_nodes, lb0, k0 >= 0xFFF0000000000000ull ? INFINITY : io0 + const0, oc0, fc0);
  return true;
}

// MIQP_DUMP_OPEN=path: open list of instance 0 after the last round (bound, depth, fix record of the 400 lowest)
inline bool dump_open_list(const DevCtx& X, const char* dp, int rounds, int NS, double const0) {
  const DevBuf& B = X.B; const Layout& Y = X.Y; const int open_cap = X.open_cap;
  int oc0 = 0; HIP_OK(hipMemcpy(&oc0, B.open_count, 4, hipMemcpyDeviceToHost)); oc0 = std::min(oc0, open_cap);
  const size_t src = ((size_t)(rounds & 1) * NS + 0) * open_cap;
  std::vector<double> hb(oc0); std::vector<int> hn(oc0), hd(oc0);
  if (oc0 > 0) { HIP_OK(hipMemcpy(hb.data(), B.open_bound + src, (size_t)oc0 * 8, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(hn.data(), B.open_node + src, (size_t)oc0 * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(hd.data(), B.open_depth + src, (size_t)oc0 * 4, hipMemcpyDeviceToHost)); }
  std::vector<int> ord(oc0); for (int k = 0; k < oc0; ++k) ord[k] = k;
  std::sort(ord.begin(), ord.end(), [&](int x, int y) { return hb[x] < hb[y]; });
  if (FILE* f = std::fopen(dp, "w")) {
    std::fprintf(f, "%d %d %d %d %d %d %d\n", oc0, Y.fixlen, Y.f_reg, Y.f_env, Y.f_obs, Y.f_c2c, Y.N);
    std::vector<signed char> rec(Y.fixlen);
    for (int q = 0; q < std::min(oc0, 400); ++q) {
      int k = ord[q]; HIP_OK(hipMemcpy(rec.data(), B.pool_fix + (size_t)hn[k] * Y.fixlen, Y.fixlen, hipMemcpyDeviceToHost));
      std::fprintf(f, "%.9g %d", hb[k] + const0, hd[k] >> 6); for (int x = 0; x < Y.fixlen; ++x) std::fprintf(f, " %d", (int)rec[x]); std::fprintf(f, "\n");
    }
    std::fclose(f);
  }
  return true;
}

#ifdef MIQP_PROFILE
// -DMIQP_PROFILE: the per-phase clock counters of the kernels, printed and zeroed after every call
inline bool print_profile(const DevCtx& X) {
  const DevBuf& B = X.B;
  { unsigned long long pf[64]; HIP_OK(hipMemcpy(pf, B.prof + 64, 64 * 8, hipMemcpyDeviceToHost));
    const char* nm[10] = {"decode", "rowpass", "bw.phi", "bw.TS+p", "bw.readlane+LDL", "bw.Ksolve", "bw.update", "forward", "step", "update"};
    double tot = 0; for (int q = 0; q < 10; ++q) tot += (double)pf[q];
    { unsigned long long po[16]; HIP_OK(hipMemcpy(po, B.prof, 16 * 8, hipMemcpyDeviceToHost));
      const char* no[9] = {"build", "bw.rows/assemble", "bw.mfma", "bw.TS", "bw.cholK", "bw.P", "forward", "step", "update"};
      double to = 0; for (int q = 0; q < 9; ++q) to += (double)po[q];
      if (po[10]) { std::fprintf(stderr, "[miqp_gpu profile] memory-backed kernel nodes %llu iters %llu cycles/node-iter %.0f :", po[10], po[9], to / std::max(1ull, po[9]));
        for (int q = 0; q < 9; ++q) std::fprintf(stderr, " %s %.1f%% (%.0f)", no[q], 100.0 * po[q] / to, (double)po[q] / std::max(1ull, po[9]));
        std::fprintf(stderr, "; inside bw.TS, the stage-Hessian chain: weights + staging %.0f, single-entry rows %.0f, MFMA loop %.0f, reductions + diagonal %.0f", (double)po[12] / std::max(1ull, po[9]), (double)po[13] / std::max(1ull, po[9]), (double)po[14] / std::max(1ull, po[9]), (double)po[15] / std::max(1ull, po[9]));
        std::fprintf(stderr, "\n"); } }
    std::fprintf(stderr, "[miqp_gpu profile] on-chip nodes %llu iters %llu cycles/node-iter %.0f :", pf[11], pf[10], tot / std::max(1ull, pf[10]));
    for (int q = 0; q < 10; ++q) std::fprintf(stderr, " %s %.1f%% (%.0f)", nm[q], 100.0 * pf[q] / tot, (double)pf[q] / std::max(1ull, pf[10]));
    std::fprintf(stderr, "\n");
    { unsigned long long pa[14]; HIP_OK(hipMemcpy(pa, B.prof + 80, 14 * 8, hipMemcpyDeviceToHost));
      const char* na[9] = {"decode", "gains + first iterate", "scan", "response of the row", "q", "directions + ratio test + M update", "iterate refresh", "results", "warm start"};
      double ta = 0; for (int q = 0; q < 9; ++q) ta += (double)pa[q];
      if (pa[10]) { std::fprintf(stderr, "[miqp_gpu profile] active-set kernel nodes %llu steps %llu cycles/node %.0f :", pa[10], pa[11], ta / (double)pa[10]);
        for (int q = 0; q < 9; ++q) std::fprintf(stderr, " %s %.1f%% (%.0f)", na[q], 100.0 * pa[q] / ta, (double)pa[q] / (double)pa[10]);
        std::fprintf(stderr, "; inside the decode: bound classes %.0f, general-row pass %.0f", (double)pa[12] / (double)pa[10], (double)pa[13] / (double)pa[10]);
        std::fprintf(stderr, "\n");
        unsigned long long pw[3], pl[6]; HIP_OK(hipMemcpy(pw, B.prof + 94, 3 * 8, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(pl, B.prof + 120, 6 * 8, hipMemcpyDeviceToHost));
        if (pw[2] && pw[1] && pl[5]) std::fprintf(stderr, "[miqp_gpu profile] standard active-set launches: %llu wavefronts resident %.0f shader cycles = %.1f us each (shader clock %.0f MHz); per launch (%llu folded): span %.3f ms, from the first wavefront out of work to the last end %.3f ms, wavefronts %.0f, resident wavefront time / (span x wavefronts) %.3f\n",
          pw[2], (double)pw[0] / pw[2], (double)pw[1] / pw[2] / 100.0, 100.0 * (double)pw[0] / (double)pw[1], pl[5], (double)pl[3] / pl[5] / 1e5, (double)pl[4] / pl[5] / 1e5, (double)pw[2] / pl[5], ((double)pw[1]) / ((double)pl[3] * ((double)pw[2] / pl[5])));
        unsigned long long ph[16]; HIP_OK(hipMemcpy(ph, B.prof + 128, 16 * 8, hipMemcpyDeviceToHost));
        if (pw[2]) { std::fprintf(stderr, "[miqp_gpu profile] standard active-set wavefronts by their start after the launch's first (< 0.05 / 0.2 / 0.5 / 1 / 2 / 4 / 8 ms / later), %% :");
          for (int q = 0; q < 8; ++q) std::fprintf(stderr, " %.1f", 100.0 * ph[q] / pw[2]);
          std::fprintf(stderr, "; by the nodes they solved (0 / <= 4 / <= 16 / <= 32 / <= 64 / more), %% :");
          for (int q = 8; q < 14; ++q) std::fprintf(stderr, " %.1f", 100.0 * ph[q] / pw[2]);
          std::fprintf(stderr, "\n"); }
        if (const char* wd = X.sw.wave_dump) {
          std::vector<unsigned long long> w(4 * 4 * 4096); HIP_OK(hipMemcpy(w.data(), B.prof + 160, w.size() * 8, hipMemcpyDeviceToHost));
          if (FILE* f = std::fopen(wd, "w")) { for (int q = 0; q < 4 * 4096; ++q) if (w[4 * q]) std::fprintf(f, "%d %llu %llu %u %u %llu %d\n", q & 4095, w[4 * q], w[4 * q + 1], (unsigned)(w[4 * q + 2] >> 32), (unsigned)w[4 * q + 2], w[4 * q + 3], q >> 12); std::fclose(f); } } } }
    { unsigned long long pe[8]; HIP_OK(hipMemcpy(pe, B.prof + 100, 8 * 8, hipMemcpyDeviceToHost));
      const char* ne[6] = {"load", "regions", "leaf disjunctions", "branching", "lifting + reservation", "records"};
      double te = 0; for (int q = 0; q < 6; ++q) te += (double)pe[q];
      if (pe[6]) { std::fprintf(stderr, "[miqp_gpu profile] eval_kernel, %llu branched nodes, cycles/node %.0f :", pe[6], te / (double)pe[6]);
        for (int q = 0; q < 6; ++q) std::fprintf(stderr, " %s %.1f%% (%.0f)", ne[q], 100.0 * pe[q] / te, (double)pe[q] / (double)pe[6]);
        std::fprintf(stderr, "\n"); } }
    { unsigned long long ps[10]; HIP_OK(hipMemcpy(ps, B.prof + 110, 10 * 8, hipMemcpyDeviceToHost));
      const char* ns[8] = {"incumbent copy / kill", "setup", "pass 1 (prune, keys)", "far refill", "bound reduce + spill select", "focus + window + share", "radix select + ties", "pass 3 (emit, compact)"};
      double ts = 0; for (int q = 0; q < 8; ++q) ts += (double)ps[q];
      if (ps[8]) { std::fprintf(stderr, "[miqp_gpu profile] select_kernel, %llu workgroups that reached the end (thread 0's clock), mean list %.0f entries, cycles each %.0f :", ps[8], (double)ps[9] / (double)ps[8], ts / (double)ps[8]);
        for (int q = 0; q < 8; ++q) std::fprintf(stderr, " %s %.1f%% (%.0f)", ns[q], 100.0 * ps[q] / ts, (double)ps[q] / (double)ps[8]);
        std::fprintf(stderr, "\n"); } }
    HIP_OK(hipMemset(B.prof, 0, 160 * 8)); }
  return true;
}
#endif

// MIQP_STATS: node outcome / branching / set-tightening counters, printed and zeroed after every call
inline bool print_stats(const DevCtx& X) {
  const DevBuf& B = X.B; const Layout& Y = X.Y;
  unsigned long long hs[256]; HIP_OK(hipMemcpy(hs, B.stats, sizeof(hs), hipMemcpyDeviceToHost)); HIP_OK(hipMemset(B.stats, 0, sizeof(hs)));
  const double nn_ = (double)std::max(1ull, hs[0]);
  std::fprintf(stderr, "[miqp_gpu stats] on-chip nodes %llu (general rows %.1f, coefficients %.1f, box keys %.1f, iterations %.1f per node), handed over %llu; general rows / 32 histogram:", hs[0], hs[1] / nn_, hs[4] / nn_, hs[2] / nn_, hs[5] / nn_, hs[3]);
  for (int q = 0; q < 16; ++q) std::fprintf(stderr, " %llu", hs[8 + q]);
  std::fprintf(stderr, "\n");
  std::fprintf(stderr, "[miqp_gpu stats] node outcomes: infeasible %llu (%.1f it), cut off %llu (%.1f it), not converged %llu (%.1f it), solved %llu (%.1f it) of which: bound >= incumbent %llu, within gap %llu, integer feasible %llu, branched %llu (%.2f children; by kind region/env/obstacle/car-car: %llu x %.1f, %llu x %.1f, %llu x %.1f, %llu x %.1f)\n",
               hs[32], hs[36] / (double)std::max(1ull, hs[32]), hs[33], hs[37] / (double)std::max(1ull, hs[33]), hs[34], hs[38] / (double)std::max(1ull, hs[34]), hs[35], hs[39] / (double)std::max(1ull, hs[35]),
               hs[40], hs[41], hs[42], hs[43], hs[44] / (double)std::max(1ull, hs[43]), hs[48], hs[52] / (double)std::max(1ull, hs[48]), hs[49], hs[53] / (double)std::max(1ull, hs[49]),
               hs[50], hs[54] / (double)std::max(1ull, hs[50]), hs[51], hs[55] / (double)std::max(1ull, hs[51]));
  std::fprintf(stderr, "[miqp_gpu stats] region sets: tightened at %llu (car, step) sites, %llu nodes closed because a step had no region left; children not created because of their lifted bound %llu (multi-row lift larger than the single-row one: %llu), car/car sets tightened at %llu groups\n", hs[58], hs[59], hs[56], hs[57], hs[61]);
  std::fprintf(stderr, "[miqp_gpu stats] region branchings flagged by: own rows %llu (worst class acc box %llu, jerk box %llu, sector %llu, half-plane %llu, curvature %llu, slow square %llu), environment front rows %llu, obstacle front rows %llu, car/car front rows %llu; by step:",
               hs[64], hs[70], hs[71], hs[72], hs[73], hs[74], hs[75], hs[65], hs[66], hs[67]);
  for (int q = 0; q < 32 && q < Y.N; ++q) std::fprintf(stderr, " %llu", hs[160 + q]);
  std::fprintf(stderr, "\n[miqp_gpu stats] node outcomes by origin (processed: infeasible / cut off / not converged / solved):");
  const char* on_[16] = {"root|reg-ref", "reg-adjacent", "reg-other", "reg-slow", "env-ref", "env-other", "-", "-", "obs-ref", "obs-other", "-", "-", "c2c-ref", "c2c-other", "-", "probe"};
  for (int q = 0; q < 16; ++q) if (hs[80 + q]) std::fprintf(stderr, " %s %llu: %llu / %llu / %llu / %llu;", on_[q], hs[80 + q], hs[96 + q], hs[112 + q], hs[128 + q], hs[144 + q]);
  std::fprintf(stderr, "\n[miqp_gpu stats] infeasible rounding probes re-rounded: %llu", hs[62]);
  std::fprintf(stderr, "\n[miqp_gpu stats] handed-over nodes with >= 480 general rows: %llu, mean %.0f, most %llu general rows", hs[7], (double)hs[6] / std::max(1ull, hs[7]), hs[5]);
  std::fprintf(stderr, "\n[miqp_gpu stats] rounding probes by iterations / 3 (0-2, 3-5, ..., 45+):");
  { const char* oc_n[4] = {"infeasible", "cut off", "not converged", "solved"};
    for (int o = 0; o < 4; ++o) { std::fprintf(stderr, " %s", oc_n[o]); for (int q = 0; q < 16; ++q) std::fprintf(stderr, " %llu", hs[192 + 16 * o + q]); std::fprintf(stderr, ";"); } }
  std::fprintf(stderr, "\n");
  return true;
}

// MIQP_STATS: what the active-set launches did (h_as: the 32 counters of DevBuf::as_stats)
inline void print_as_stats(const unsigned long long* h_as) {
  std::fprintf(stderr, "[miqp_gpu stats] active-set launch: %llu nodes (%.1f steps, %.1f drops, %.1f rows from the parent's active set, %.1f active rows at the end per node; %llu infeasible, %llu cut off; %llu started from the parent's M, %llu fell back to a cold start), %llu handed to the interior point (no free slot %llu, step cap %llu, curvature %llu, down-date pivot %llu, rows off their equalities %llu, other %llu); M rebuilt because: the parent left none %llu, the ring had come round %llu, another row count %llu; in the larger block %llu nodes (%.1f steps), of them leaves of the local search %llu (%.1f steps), rounding probes %llu; by their general rows (<= 64 / 96 / 128 / 192 / more) %llu / %llu / %llu / %llu / %llu\n",
               h_as[0], h_as[1] / (double)std::max(1ull, h_as[0]), h_as[3] / (double)std::max(1ull, h_as[0]), h_as[7] / (double)std::max(1ull, h_as[0]), h_as[6] / (double)std::max(1ull, h_as[0]), h_as[4], h_as[5], h_as[8], h_as[9], h_as[2], h_as[11], h_as[12], h_as[13], h_as[14], h_as[15], h_as[10], h_as[17], h_as[18], h_as[19], h_as[20], h_as[21] / (double)std::max(1ull, h_as[20]), h_as[22], h_as[23] / (double)std::max(1ull, h_as[22]), h_as[29], h_as[24], h_as[25], h_as[26], h_as[27], h_as[28]);
}

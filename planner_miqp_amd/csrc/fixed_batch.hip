// fixed_batch.hip - many fixed-binary QPs in one device call: the records of ONE instance (miqp_solver_solve_fixed_batch, _fixed_batch_record) and
// the records of MANY (miqp_solver_solve_fixed_multi).  DESIGN.md 6b, 6d.
//
// The question miqp_solver_solve_fixed answers for one record - the best continuous trajectory under its integer decisions, and its cost - asked
// for n records of the instance the handle holds.  No reference counterpart as an entry point: the reference walks its alternative start
// configurations one after the other, one cplex.solve() each (src/miqp_planner.cpp:694-749); a caller that enumerates manoeuvres - left or right
// of each obstacle, before or after the other car - asks it hundreds of times for one instance.  The product's path is a queue of thousands of
// handles, and a loop of one-handle calls over them pays per handle what the call pays once: a device lock, a compile_instance, an upload of the
// tables, a chain of launches that is as long for one node as for a thousand - and a context rebuild whenever two handles differ in their own Layout.
//
// The accepted entries (records of their instance's shape; the others are status 2 and never reach the device) are numbered 0 .. m - 1 handle-major
// in the caller's order and go through FixedCall of fixed_chain.hip; the one-handle entry is the call with one handle.  What differs between the
// entries is what they refuse, and with which code, before a device is touched.
#pragma once

namespace {

// the int arrays fix_from_results reads
bool fixed_record_ok(const miqp_raw_results_c& r) {
  const void* need[] = {r.notWithinEnvironmentRear, r.notWithinEnvironmentFrontUbUb, r.notWithinEnvironmentFrontLbUb, r.notWithinEnvironmentFrontUbLb, r.notWithinEnvironmentFrontLbLb,
                        r.active_region, r.region_change_not_allowed_x_positive, r.region_change_not_allowed_y_positive, r.region_change_not_allowed_x_negative,
                        r.region_change_not_allowed_y_negative, r.region_change_not_allowed_combined, r.deltacc, r.deltacc_front, r.car2car_collision,
                        r.slackvarsObstacle, r.slackvarsObstacle_front};
  for (const void* q : need) if (!q) return false;
  return true;
}

// Behind the fix records of a call: they run, and every handle receives its answers.  Node c is entry where[c] of the caller's arrays and belongs to
// handle inst[c]; the nodes of handle h are nfirst[h] .. nfirst[h + 1] - 1, its entries first[h] .. first[h + 1] - 1.  out and best (may be NULL)
// are the caller's; after (may be NULL) is enqueued behind every chunk (fixed_run).  0 or -3
int fixed_answer(FixedCall& call, const std::vector<signed char>& fix, const std::vector<int>& inst, const std::vector<int>& where, const std::vector<int>& nfirst, const int* first,
                 miqp_fixed_result_c* out, int* best, double t_call, const FixedAfterChunk* after = nullptr) {
  const Layout& Y = call.Y; const size_t fl = (size_t)Y.fixlen, row = (size_t)Y.N * Y.nz;
  const int m = (int)where.size();
  const double setup_s = wall_s() - t_call;
  std::vector<miqp_fixed_result_c> tmp; std::vector<double> Z; std::vector<int> hbest; float dev_ms = 0.0f; int groups = 0;
  if (call.run(fix, inst, m, tmp, Z, hbest, dev_ms, groups, after) != 0) return -3;
  for (int c = 0; c < m; ++c) out[where[c]] = tmp[c];
  const double call_s = wall_s() - t_call;
  for (int h = 0; h < call.n; ++h) {
    miqp_solver_t* s = call.S[h];
    const int c0 = nfirst[h], mh = nfirst[h + 1] - c0, nh = first[h + 1] - first[h];
    s->setup[0] = setup_s;
    s->timing[0] = call_s; s->timing[1] = dev_ms * 1e-3; s->timing[2] = groups; s->timing[3] = mh; s->timing[4] = 0; s->timing[5] = 0;
    for (int c = c0; c < c0 + mh; ++c) s->timing[4] += tmp[c].iterations;
    if (mh == 0) continue;   // (an empty range, or every entry refused: the handle keeps nothing)
    if (best) best[h] = hbest[h] < 0 || hbest[h] >= mh ? -1 : where[c0 + hbest[h]] - first[h];
    s->fb_n = nh; s->fb_slot.assign(nh, -1);
    for (int c = 0; c < mh; ++c) if (tmp[c0 + c].status == 0) s->fb_slot[where[c0 + c] - first[h]] = c;
    s->fb_Z.assign(Z.begin() + (size_t)c0 * row, Z.begin() + (size_t)(c0 + mh) * row);
    s->fb_fix.assign(fix.begin() + (size_t)c0 * fl, fix.begin() + (size_t)(c0 + mh) * fl);
  }
  return 0;
}

// The entries of n handles from `out` initialised on: the accepted ones, their fix records on a few host threads when there are many, the run.
// 0 (also: nothing accepted, no device is touched) or -3
int fixed_records(miqp_solver_t* const* solvers, int n, const Layout& Y, const miqp_raw_results_c* const* fixed, const int* first, miqp_fixed_result_c* out, int* best, double t_call) {
  // the accepted entries, handle-major in the caller's order: entry where[c] is node c of the call, nfirst[h] the first node of handle h
  const int total = first[n];
  std::vector<int> where, inst, nfirst(n + 1, 0); where.reserve(total); inst.reserve(total);
  for (int h = 0; h < n; ++h) {
    for (int k = first[h]; k < first[h + 1]; ++k) if (fixed[k] && fixed_record_ok(*fixed[k]) && dims_match(*fixed[k], solvers[h]->inst)) { where.push_back(k); inst.push_back(h); }
    nfirst[h + 1] = (int)where.size();
  }
  const int m = (int)where.size();
  if (m == 0) return 0;
  FixedCall call;
  if (call.open(solvers, n, Y) != 0) return -3;
  const size_t fl = (size_t)Y.fixlen;
  std::vector<signed char> fix((size_t)m * fl);
  fixed_threads((m + 255) / 256, 1, [&](int b) {
    std::vector<signed char> one_fix;
    for (int c = b * 256; c < std::min(m, (b + 1) * 256); ++c) {
      const int h = inst[c];
      (void)fix_from_results(solvers[h]->inst, Y, call.tabT(h), fixed[where[c]], one_fix); std::memcpy(fix.data() + (size_t)c * fl, one_fix.data(), fl);
    }
  });
  return fixed_answer(call, fix, inst, where, nfirst, first, out, best, t_call);
}

}  // namespace

extern "C" {

int miqp_gpu_fixed_result_size(void) { return (int)sizeof(miqp_fixed_result_c); }
int miqp_gpu_fixed_batch_chunk(void) { return FB_CHUNK; }

int miqp_solver_solve_fixed_batch(miqp_solver_t* s, const miqp_raw_results_c* const* fixed, int n, miqp_fixed_result_c* out, int* best) {
  if (s) s->drop_fixed_batch();
  if (!s || !s->has_inst || !fixed || !out || n <= 0) return -1;
  if (n > FB_CAP) return -5;
  const double t_call = wall_s();
  if (best) *best = -1;
  fixed_refuse(out, n);
  miqp_solver_t* one[1] = {s};
  BatchShape bs = batch_layout(one, 1);
  if (!bs.ok) return -2;
  const int first[2] = {0, n};
  return fixed_records(one, 1, bs.Y, fixed, first, out, best, t_call);
}

int miqp_solver_fixed_batch_record(miqp_solver_t* s, int k, miqp_raw_results_c* out) {
  if (!s || !out || !s->has_inst || s->fb_n <= 0 || k < 0 || k >= s->fb_n) return -1;
  const int c = s->fb_slot[k];
  if (c < 0) return 1;
  if (!dims_match(*out, s->inst)) return -2;
  return fixed_hand_out(s, s->fb_fix, s->fb_Z, c, out);
}

int miqp_solver_solve_fixed_multi(miqp_solver_t* const* solvers, int n, const miqp_raw_results_c* const* fixed, const int* first, miqp_fixed_result_c* out, int* best) {
  if (!solvers || !fixed || !first || !out || n <= 0 || first[0] != 0) return -1;
  for (int h = 0; h < n; ++h) if (first[h + 1] < first[h]) return -1;
  BatchShape bs;
  if (const int rc = fixed_multi_check(solvers, n, bs)) return rc;
  if (first[n] > FB_CAP) return -5;
  const double t_call = wall_s();
  for (int h = 0; h < n; ++h) { solvers[h]->drop_fixed_batch(); if (best) best[h] = -1; }
  fixed_refuse(out, first[n]);
  return fixed_records(solvers, n, bs.Y, fixed, first, out, best, t_call);
}

}  // extern "C"

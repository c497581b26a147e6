// raw_model_check - both sinks of planner_miqp_amd/csrc/raw_model.hpp on the host, for tests/test_raw_model_cpu.py.
//
//   raw_model_check <instance.dat> <out.lp>
//
// Writes the .lp of the instance (the naming sink), fills a record from a fixed integer pattern, and prints
//   v <name> <value>                 every variable of the record, through raw_name and raw_value
//   r <row> <sense> <lhs> <rhs>      every row of the families A1..A8, walked as one thread with the evaluating sink
//   f <family> <first row> <violation> <row>     the running maximum the evaluating sink leaves per family
// Host headers only: no HIP, no library.  Test infrastructure, built with -fsanitize=address,undefined.
#include <cstdio>
#include <string>
#include <vector>

#include "../../planner_miqp_amd/csrc/lp_export.hpp"

using namespace miqp;

struct PrintEval : RawEval {
  void end(int sense, double rhs) {
    RawEval::end(sense, rhs);
    std::printf("r %d %s %.17g %.17g\n", r, sense == RAW_LE ? "<=" : (sense == RAW_GE ? ">=" : "="), lhs, rhs);
  }
};

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: raw_model_check <instance.dat> <out.lp>\n"); return 2; }
  HostInst I; std::string err;
  if (!inst_from_dat(argv[1], I, err)) { std::fprintf(stderr, "%s\n", err.c_str()); return 1; }
  const int rc = export_lp(I, argv[2]);
  if (rc != 0) { std::fprintf(stderr, "export_lp: %d\n", rc); return 1; }
  const int C = I.C, N = I.N, R = I.R, E = I.E, O = I.O, L = I.L, K = C - 1;
  // the record: one counter over all members; continuous values are quarters in [-5, 5], integer members 0 or 1
  unsigned n = 0;
  auto dbl = [&](size_t len) { std::vector<double> v(len); for (double& x : v) { x = (double)((int)(n * 37u % 41u) - 20) / 4.0; ++n; } return v; };
  auto bin = [&](size_t len) { std::vector<int> v(len); for (int& x : v) { x = (int)((n * 5u + n / 3u) & 1u); ++n; } return v; };
  std::vector<std::vector<double>> ct; for (int k = 0; k < 12; ++k) ct.push_back(dbl((size_t)C * N));
  std::vector<std::vector<int>> nw; for (int k = 0; k < 5; ++k) nw.push_back(bin((size_t)C * E * N));
  std::vector<int> ar = bin((size_t)C * N * R);
  std::vector<std::vector<int>> rch; for (int k = 0; k < 5; ++k) rch.push_back(bin((size_t)C * N));
  std::vector<int> d = bin((size_t)C * O * N * L), df = bin((size_t)C * O * N * L * 4), cc = bin((size_t)K * K * N * 16), sl = bin((size_t)K * K * N * 4);
  std::vector<int> so = bin((size_t)C * O * N), sof = bin((size_t)C * O * N * 4);
  std::vector<double> slr = dbl((size_t)K * K * N * 4);
  miqp_raw_results_c r = {};
  r.N = N; r.NrEnvironments = E; r.NrRegions = R; r.NrObstacles = O; r.MaxLinesObstacles = L; r.NrCarToCarCollisions = K; r.NrCars = C;
  double** const cp[12] = {&r.u_x, &r.u_y, &r.pos_x, &r.vel_x, &r.acc_x, &r.pos_y, &r.vel_y, &r.acc_y, &r.pos_x_front_UB, &r.pos_x_front_LB, &r.pos_y_front_UB, &r.pos_y_front_LB};
  for (int k = 0; k < 12; ++k) *cp[k] = ct[k].data();
  r.notWithinEnvironmentRear = nw[0].data(); r.notWithinEnvironmentFrontUbUb = nw[1].data(); r.notWithinEnvironmentFrontLbUb = nw[2].data();
  r.notWithinEnvironmentFrontUbLb = nw[3].data(); r.notWithinEnvironmentFrontLbLb = nw[4].data();
  r.active_region = ar.data();
  r.region_change_not_allowed_x_positive = rch[0].data(); r.region_change_not_allowed_y_positive = rch[1].data(); r.region_change_not_allowed_x_negative = rch[2].data();
  r.region_change_not_allowed_y_negative = rch[3].data(); r.region_change_not_allowed_combined = rch[4].data();
  r.deltacc = d.data(); r.deltacc_front = df.data(); r.car2car_collision = cc.data(); r.slackvars = sl.data();
  r.slackvarsObstacle = so.data(); r.slackvarsObstacle_front = sof.data(); r.slackvars_real = slr.data();

  std::vector<double> blob((cert_blob_bytes(I) + 7) / 8);
  cert_pack_params(I, blob.data());
  cert_pack_record(I, r, blob.data());
  CertView V; V.bind(blob.data());

  // every variable: the index ranges of each kind, in the order of its name
  for (int kind = 0; kind < RK_COUNT; ++kind) {
    int dim[5] = {1, 1, 1, 1, 1};
    if (kind < RK_AR || (kind >= RK_RC && kind < RK_NW)) { dim[0] = C; dim[1] = N; }
    else if (kind == RK_AR) { dim[0] = C; dim[1] = N; dim[2] = R; }
    else if (kind < RK_D) { dim[0] = C; dim[1] = E; dim[2] = N; }
    else if (kind == RK_D || kind == RK_DF) { dim[0] = C; dim[1] = O; dim[2] = N; dim[3] = L; dim[4] = kind == RK_DF ? 4 : 1; }
    else if (kind == RK_SO || kind == RK_SOF) { dim[0] = C; dim[1] = O; dim[2] = N; dim[3] = kind == RK_SOF ? 4 : 1; }
    else { dim[0] = K; dim[1] = K; dim[2] = N; dim[3] = kind == RK_CC ? 16 : 4; }
    for (int a = 0; a < dim[0]; ++a) for (int b = 0; b < dim[1]; ++b) for (int c = 0; c < dim[2]; ++c) for (int e = 0; e < dim[3]; ++e) for (int g = 0; g < dim[4]; ++g) {
      const RawVar v = raw_var(kind, a, b, c, e, g);
      std::printf("v %s %.17g\n", raw_name(v).c_str(), raw_value(V, v));
    }
  }
  for (int f = 0; f < 8; ++f) {
    CertMax m{0.0, -1};
    PrintEval ev{{V, m, 0.0, 0}};
    raw_family(f, V, 0, 1, ev);
    std::printf("f %d %d %.17g %d\n", f + 1, V.base[f], m.v, m.row);
  }
  return 0;
}

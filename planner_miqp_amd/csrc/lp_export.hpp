// lp_export.hpp - CPLEX LP-format dump of the raw big-M model of one instance (debug / interoperability format,
// replaces cplex.exportModel, src/cplex_wrapper.cpp:150-154), so that anyone with a CPLEX licence can re-solve the
// instance.  The `Subject To` rows are those of raw_model.hpp, the text the certificate kernel evaluates; objective,
// bounds and binaries are written here.
#pragma once
#include <cstdio>
#include <string>
#include <vector>

#include "raw_model.hpp"

namespace miqp {

// The writer is the naming sink of raw_model.hpp's row walker: it packs the parameter block of the instance with no record
// in it and walks the families A1..A8 as one thread.
struct LpWriter {
  const HostInst& I; FILE* f; long rows = 0; bool in_order = true;
  struct Term { std::string v; double c; };
  std::vector<Term> t;   // the open row: repeated names merged
  static std::string nm(int kind, int a, int b, int c = 0, int d = 0, int e = 0) { return raw_name(raw_var(kind, a, b, c, d, e)); }
  void begin(int r) { if (r != rows) in_order = false; t.clear(); }   // rows arrive as c1, c2, c3, ...
  void term(const RawVar& v, double c) {
    const std::string n = raw_name(v);
    for (auto& b : t) if (b.v == n) { b.c += c; return; }
    t.push_back({n, c});
  }
  void end(int sense, double rhs) {   // constants are folded into rhs already
    std::fprintf(f, " c%ld:", ++rows);
    bool any = false;
    for (auto& a : t) if (a.c != 0.0) { std::fprintf(f, " %+.17g %s", a.c, a.v.c_str()); any = true; }
    if (!any) std::fprintf(f, " 0 %s", t.empty() ? "dummy" : t[0].v.c_str());
    std::fprintf(f, " %s %.17g\n", sense == RAW_LE ? "<=" : (sense == RAW_GE ? ">=" : "="), rhs);
  }
  bool write() {
    const int C = I.C, N = I.N, R = I.R, E = I.E, O = I.O, L = I.L, K = C - 1;
    std::fprintf(f, "\\ planner-miqp MIQP (cplexmodel/*.mod), written by libmiqp_gpu\nMinimize\n obj:");
    // linear part of sum W (v - ref)^2, quadratic part below; the constant sum W ref^2 is omitted (objective_function.mod:7-19)
    const int sv[6] = {CV_PX, CV_VX, CV_AX, CV_PY, CV_VY, CV_AY};
    for (int c = 0; c < C; ++c) for (int i = 0; i < N; ++i) for (int k = 0; k < 6; ++k) {
      double w = I.W[c * 8 + k], r = I.ref[((size_t)c * N + i) * 6 + k];
      if (w != 0.0 && r != 0.0) std::fprintf(f, " %+.17g %s", -2.0 * w * r, nm(sv[k], c, i).c_str());
    }
    std::fprintf(f, " + [");
    for (int c = 0; c < C; ++c) for (int i = 0; i < N; ++i) {
      for (int k = 0; k < 6; ++k) if (I.W[c * 8 + k] != 0.0) std::fprintf(f, " %+.17g %s ^2", 2.0 * I.W[c * 8 + k], nm(sv[k], c, i).c_str());
      if (I.W[c * 8 + 6] != 0.0) std::fprintf(f, " %+.17g %s ^2", 2.0 * I.W[c * 8 + 6], nm(CV_UX, c, i).c_str());
      if (I.W[c * 8 + 7] != 0.0) std::fprintf(f, " %+.17g %s ^2", 2.0 * I.W[c * 8 + 7], nm(CV_UY, c, i).c_str());
      for (int o = 0; o < O; ++o) for (int p = 0; p < 5; ++p) std::fprintf(f, " %+.17g %s ^2", 2.0 * I.w_slack_obs, raw_name(raw_so(p, c, o, i)).c_str());
    }
    for (int a = 0; a < K; ++a) for (int b = 0; b < K; ++b) for (int i = 0; i < N; ++i) for (int q = 0; q < 4; ++q)
      std::fprintf(f, " %+.17g %s ^2", 2.0 * I.w_slack, nm(RK_SL, a, b, i, q).c_str());
    std::fprintf(f, " ] / 2\nSubject To\n");
    std::vector<double> blob((cert_blob_bytes(I) + 7) / 8);
    cert_pack_params(I, blob.data());
    CertView V; V.bind(blob.data());
    for (int fam = 0; fam < 8; ++fam) raw_family(fam, V, 0, 1, *this);
    // bounds: OPL dvar float is free; slack ranges of decision_variables.mod:43-53
    std::fprintf(f, "Bounds\n");
    for (int k = 0; k < RK_AR; ++k) for (int c = 0; c < C; ++c) for (int i = 0; i < N; ++i) std::fprintf(f, " %s free\n", nm(k, c, i).c_str());
    for (int c = 0; c < C; ++c) for (int o = 0; o < O; ++o) for (int i = 0; i < N; ++i) for (int p = 0; p < 5; ++p)
      std::fprintf(f, " 0 <= %s <= 1\n", raw_name(raw_so(p, c, o, i)).c_str());
    for (int a = 0; a < K; ++a) for (int b = 0; b < K; ++b) for (int i = 0; i < N; ++i) for (int q = 0; q < 4; ++q)
      std::fprintf(f, " 0 <= %s <= %.17g\n", nm(RK_SL, a, b, i, q).c_str(), I.max_slack);
    std::fprintf(f, "Binaries\n");
    auto B = [&](const std::string& s) { std::fprintf(f, " %s\n", s.c_str()); };
    for (int p = 0; p < 5; ++p) for (int c = 0; c < C; ++c) for (int e = 0; e < E; ++e) for (int i = 0; i < N; ++i) B(nm(RK_NW + p, c, e, i));
    for (int c = 0; c < C; ++c) for (int i = 0; i < N; ++i) for (int j = 0; j < R; ++j) B(nm(RK_AR, c, i, j));
    for (int k = 0; k < 5; ++k) for (int c = 0; c < C; ++c) for (int i = 0; i < N; ++i) B(nm(RK_RC + k, c, i));
    for (int c = 0; c < C; ++c) for (int o = 0; o < O; ++o) for (int i = 0; i < N; ++i) for (int k = 0; k < L; ++k) for (int p = 0; p < 5; ++p) B(raw_name(raw_dv(p, c, o, i, k)));
    for (int a = 0; a < K; ++a) for (int b = 0; b < K; ++b) for (int i = 0; i < N; ++i) for (int s = 0; s < 16; ++s) B(nm(RK_CC, a, b, i, s));
    std::fprintf(f, "End\n");
    return in_order && rows == V.base[8];
  }
};

// 0, -2: the file cannot be written, -3: the walker's rows did not arrive as c1, c2, ... up to the model's row count
inline int export_lp(const HostInst& I, const char* path) {
  FILE* f = std::fopen(path, "w");
  if (!f) return -2;
  LpWriter w{I, f};
  const bool ok = w.write();
  std::fclose(f);
  return ok ? 0 : -3;
}

}  // namespace miqp

// raw_model.hpp - the raw big-M rows of cplexmodel/*.mod, stated once: parameter layout, packer, variable ids, row walker.
//
// Nothing here stores a matrix: a row is decoded from (family, item, k) of a closed-form index space and handed to a sink as
// terms over variable ids - sink.begin(row), sink.term(var, coef) ..., sink.end(sense, rhs) - from the instance's parameter
// block alone.  Two sinks exist: RawEval below (the kernel of certify.hip: coef * value on a delivered record) and the
// LpWriter of lp_export.hpp (names).  So `worst_row` of a certificate is the 0-based index of the row `c<worst_row+1>` of
// miqp_solver_export_lp by construction: both walk this text, with the coefficients and big-M constants of parameters.mod:24-32.
// Compiles for the host without HIP (tests/standin/raw_model_check.cpp evaluates every row of both sinks there).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstring>
#include <string>

#include "host_inst.hpp"

#if defined(__HIPCC__)
#define CERT_HD __host__ __device__ __forceinline__
#else
#define CERT_HD inline
#endif

namespace miqp {

// ---------------------------------------------------------------------------------------------------------------- variables
// A variable of the model: its kind and up to five indices, in the order of its name.  The twelve continuous arrays come
// first (their kind is the index of the array in the record's continuous section), then the five region_change_not_allowed_*
// and the five notWithinEnvironment* in the order of the corner tables.  raw_value and raw_name are the only maps from ids.
enum { CV_UX = 0, CV_UY, CV_PX, CV_VX, CV_AX, CV_PY, CV_VY, CV_AY, CV_XFU, CV_XFL, CV_YFU, CV_YFL,
       RK_AR, RK_RC, RK_NW = RK_RC + 5, RK_D = RK_NW + 5, RK_DF, RK_SO, RK_SOF, RK_CC, RK_SL, RK_COUNT };
enum { RAW_LE = 0, RAW_GE, RAW_EQ };
enum { CS_TS = 0, CS_VMIN, CS_VMAX, CS_AMIN, CS_AMAX, CS_JMIN, CS_JMAX, CS_VM, CS_WSLACK, CS_WSLACK_OBS, CS_COUNT = 12 };

struct RawVar { int kind, x[5]; };
CERT_HD RawVar raw_var(int kind, int a, int b, int c = 0, int d = 0, int e = 0) { return RawVar{kind, {a, b, c, d, e}}; }
// a continuous array chosen at run time (by axis, corner or nibble): says so, or raw_value keeps every other kind's branch alive in the kernel
CERT_HD RawVar raw_cont(int k, int c, int i) { if (k < 0 || k >= RK_AR) __builtin_unreachable(); return raw_var(k, c, i); }
// point p of (car, obstacle, step): 0 the rear axle (deltacc, slackvarsObstacle), 1..4 the front points (*_front)
CERT_HD RawVar raw_dv(int p, int c, int o, int i, int k) { return p == 0 ? raw_var(RK_D, c, o, i, k) : raw_var(RK_DF, c, o, i, k, p - 1); }
CERT_HD RawVar raw_so(int p, int c, int o, int i) { return p == 0 ? raw_var(RK_SO, c, o, i) : raw_var(RK_SOF, c, o, i, p - 1); }

inline std::string raw_name(const RawVar& v) {
  static const char* const base[RK_COUNT] = {
      "u_x", "u_y", "pos_x", "vel_x", "acc_x", "pos_y", "vel_y", "acc_y", "pos_x_front_UB", "pos_x_front_LB", "pos_y_front_UB", "pos_y_front_LB",
      "active_region", "region_change_not_allowed_x_positive", "region_change_not_allowed_y_positive", "region_change_not_allowed_x_negative",
      "region_change_not_allowed_y_negative", "region_change_not_allowed_combined",
      "notWithinEnvironmentRear", "notWithinEnvironmentFrontUbUb", "notWithinEnvironmentFrontLbUb", "notWithinEnvironmentFrontUbLb", "notWithinEnvironmentFrontLbLb",
      "deltacc", "deltacc_front", "slackvarsObstacle", "slackvarsObstacle_front", "car2car_collision", "slackvars"};
  static const int nidx[RK_COUNT] = {2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 2, 2, 2, 2, 3, 3, 3, 3, 3, 4, 5, 3, 4, 4, 4};
  std::string s = base[v.kind];
  for (int k = 0; k < nidx[v.kind]; ++k) { s += "#"; s += std::to_string(v.x[k] + 1); }
  return s;
}

// ---------------------------------------------------------------------------------------------------------------- layout
// One instance = one blob: [header 8 int][doubles][ints][bytes], 16-byte padded.  Every offset follows from the header.
struct CertLay {
  int C, N, R, E, O, L, K, NE, NP;
  // doubles (index into the double section)
  int d_scal, d_safety, d_sslack, d_W, d_wb, d_rad, d_x0, d_front0, d_ref, d_acc, d_jerk, d_frac, d_poly, d_env, d_obs, d_cont, d_slack, nd;
  // ints
  int i_init, i_poss, i_a4off, i_cpre, i_edge_env, i_soft, ni;
  // bytes: the binary members first (one range for the integrality scan), then the obstacle slacks
  int b_nw, b_ar, b_rc, b_d, b_df, b_cc, nbin, b_sO, b_sOf, nb;
  size_t bytes;
  CERT_HD void init(int C_, int N_, int R_, int E_, int O_, int L_, int NE_) {
    C = C_; N = N_; R = R_; E = E_; O = O_; L = L_; NE = NE_; K = C - 1; NP = C * (C - 1) / 2;
    int o = 0;
    d_scal = o; o += CS_COUNT; d_safety = o; o += N; d_sslack = o; o += N; d_W = o; o += C * 8; d_wb = o; o += C; d_rad = o; o += C;
    d_x0 = o; o += C * 6; d_front0 = o; o += C * 2; d_ref = o; o += C * N * 6; d_acc = o; o += C * R * 4; d_jerk = o; o += C * R * 4;
    d_frac = o; o += R * 4; d_poly = o; o += 6 * R * 3; d_env = o; o += NE * 4; d_obs = o; o += O * N * L * 4;
    d_cont = o; o += 12 * C * N; d_slack = o; o += K * K * N * 4; nd = o;
    o = 0;
    i_init = o; o += C; i_poss = o; o += C * R; i_a4off = o; o += C * (R + 1); i_cpre = o; o += C + 1; i_edge_env = o; o += NE; i_soft = o; o += O;
    ni = (o + 1) & ~1;
    o = 0;
    b_nw = o; o += 5 * C * E * N; b_ar = o; o += C * N * R; b_rc = o; o += 5 * C * N; b_d = o; o += C * O * N * L; b_df = o; o += C * O * N * L * 4;
    b_cc = o; o += K * K * N * 16; nbin = o; b_sO = o; o += C * O * N; b_sOf = o; o += C * O * N * 4; nb = o;
    bytes = ((size_t)32 + (size_t)nd * 8 + (size_t)ni * 4 + (size_t)nb + 15) & ~(size_t)15;
  }
};

// first row of family f (0-based) into base[f], base[8] = rows of the model; a4tot: A4 rows of one step over all cars, NE:
// edges of all environment pieces.  The one count of the rows: CertView::bind and raw_sizes (miqp_gpu.hip) both call it.
CERT_HD void raw_row_bases(int C, int N, int R, int E, int O, int L, int NE, int a4tot, int base[9]) {
  const int K = C - 1;
  base[0] = 0;
  base[1] = C * 12 + R * C * 5 + C * 5;
  base[2] = base[1] + (N - 1) * C * 6;
  base[3] = base[2] + N * C * 12;
  base[4] = base[3] + (N - 1) * a4tot;
  base[5] = base[4] + (N - 1) * C * R * 15;
  base[6] = base[5] + (E > 0 ? N * C * (5 * NE + 5) : 0);
  base[7] = base[6] + (O > 0 ? N * C * O * (5 * L + 5) : 0);
  base[8] = base[7] + (C > 1 ? N * 20 * ((K - 1) * K / 2) + 24 * N * (C * K / 2) : 0);
}

struct CertView {
  CertLay Y;
  const double* D;       // double section
  const double* cont;    // the 12 continuous arrays [(k*C+c)*N+i]: the double section, or the kernel's copy of it in LDS
  const int* I;
  const signed char* B;
  int a4tot;             // A4 rows of one step (all cars)
  int base[9];           // first row of family f (0-based), base[8] = rows
  CERT_HD void bind(const void* blob) {
    const int* h = (const int*)blob;
    Y.init(h[0], h[1], h[2], h[3], h[4], h[5], h[6]);
    D = (const double*)((const char*)blob + 32); cont = D + Y.d_cont;
    I = (const int*)(D + Y.nd); B = (const signed char*)(I + Y.ni);
    a4tot = I[Y.i_cpre + Y.C];
    raw_row_bases(Y.C, Y.N, Y.R, Y.E, Y.O, Y.L, Y.NE, a4tot, base);
  }
  CERT_HD double X(int k, int c, int i) const { return cont[(k * Y.C + c) * Y.N + i]; }
  CERT_HD double S(int k) const { return D[Y.d_scal + k]; }
};

// value of a variable on the record of the blob
CERT_HD double raw_value(const CertView& V, const RawVar& v) {
  const CertLay& Y = V.Y; const int k = v.kind; const int* x = v.x;
  if (k < RK_AR) return V.X(k, x[0], x[1]);
  if (k == RK_AR) return (double)V.B[Y.b_ar + (x[0] * Y.N + x[1]) * Y.R + x[2]];
  if (k < RK_NW) return (double)V.B[Y.b_rc + ((k - RK_RC) * Y.C + x[0]) * Y.N + x[1]];
  if (k < RK_D) return (double)V.B[Y.b_nw + (((k - RK_NW) * Y.C + x[0]) * Y.E + x[1]) * Y.N + x[2]];
  if (k == RK_D) return (double)V.B[Y.b_d + ((x[0] * Y.O + x[1]) * Y.N + x[2]) * Y.L + x[3]];
  if (k == RK_DF) return (double)V.B[Y.b_df + (((x[0] * Y.O + x[1]) * Y.N + x[2]) * Y.L + x[3]) * 4 + x[4]];
  if (k == RK_SO) return (double)V.B[Y.b_sO + (x[0] * Y.O + x[1]) * Y.N + x[2]];
  if (k == RK_SOF) return (double)V.B[Y.b_sOf + ((x[0] * Y.O + x[1]) * Y.N + x[2]) * 4 + x[3]];
  if (k == RK_CC) return (double)V.B[Y.b_cc + ((x[0] * Y.K + x[1]) * Y.N + x[2]) * 16 + x[3]];
  return V.D[Y.d_slack + ((x[0] * Y.K + x[1]) * Y.N + x[2]) * 4 + x[3]];
}

// ---------------------------------------------------------------------------------------------------------------- sinks
// running maximum of one thread; rows arrive in increasing order, so `>` keeps the lowest index among equals
struct CertMax {
  double v; int row;
  CERT_HD void le(double lhs, double rhs, int r) { const double d = lhs - rhs; if (d > v) { v = d; row = r; } }
  CERT_HD void ge(double lhs, double rhs, int r) { const double d = rhs - lhs; if (d > v) { v = d; row = r; } }
  CERT_HD void eq(double lhs, double rhs, int r) { const double d = fabs(lhs - rhs); if (d > v) { v = d; row = r; } }
};

// the evaluating sink: coef * value in arrival order, the violation into the running maximum
struct RawEval {
  const CertView& V; CertMax& m; double lhs; int r;
  CERT_HD void begin(int row) { r = row; lhs = 0.0; }
  CERT_HD void term(const RawVar& v, double c) { lhs += c * raw_value(V, v); }
  CERT_HD void end(int sense, double rhs) { if (sense == RAW_LE) m.le(lhs, rhs, r); else if (sense == RAW_GE) m.ge(lhs, rhs, r); else m.eq(lhs, rhs, r); }
};

// a row of fixed length in one call: raw_row(sink, row, sense, rhs, var, coef, var, coef, ...)
template <class S> CERT_HD void raw_terms(S&) {}
template <class S, class... T> CERT_HD void raw_terms(S& s, const RawVar& v, double c, T... t) { s.term(v, c); raw_terms(s, t...); }
template <class S, class... T> CERT_HD void raw_row(S& s, int r, int sense, double rhs, T... t) { s.begin(r); raw_terms(s, t...); s.end(sense, rhs); }

// big-M constants of parameters.mod:24-32
#define CERT_M_JERK 10.0
#define CERT_M_VELFRAC 1000.0
#define CERT_M_POSPOLY 100.0
#define CERT_M_ACC 10.0
#define CERT_M_KAPPA 1000.0
#define CERT_M_VEL 100.0
#define CERT_M_ENV 10000.0
#define CERT_M_OBS 10000.0
#define CERT_M_AGENTS 1000.0

// ---------------------------------------------------------------------------------------------------------------- families
// Each hands the items tid, tid + nth, ... of its index space to the sink; with tid = 0, nth = 1 the rows arrive as 0, 1, 2, ...
// Duplicate rows and `==` fixings are kept as rows.

// A1 initial_conditions.mod:11-61
template <class S> CERT_HD void raw_A1(const CertView& V, int tid, int nth, S& s) {
  const CertLay& Y = V.Y; const int C = Y.C, N = Y.N, R = Y.R;
  for (int c = tid; c < C; c += nth) {
    int r = c * 12;
    const int sv[6] = {CV_PX, CV_VX, CV_AX, CV_PY, CV_VY, CV_AY};
    for (int k = 0; k < 6; ++k) raw_row(s, r++, RAW_EQ, V.D[Y.d_x0 + c * 6 + k], raw_cont(sv[k], c, 0), 1.0);
    const double fx = V.D[Y.d_front0 + 2 * c], fy = V.D[Y.d_front0 + 2 * c + 1];
    raw_row(s, r++, RAW_EQ, fx, raw_var(CV_XFU, c, 0), 1.0); raw_row(s, r++, RAW_EQ, fx, raw_var(CV_XFL, c, 0), 1.0);
    raw_row(s, r++, RAW_EQ, fy, raw_var(CV_YFU, c, 0), 1.0); raw_row(s, r++, RAW_EQ, fy, raw_var(CV_YFL, c, 0), 1.0);
    raw_row(s, r++, RAW_EQ, 0.0, raw_var(CV_UX, c, N - 1), 1.0); raw_row(s, r++, RAW_EQ, 0.0, raw_var(CV_UY, c, N - 1), 1.0);
  }
  for (int it = tid; it < R * C; it += nth) {
    const int j = it / C, c = it - j * C; int r = C * 12 + it * 5;
    const RawVar ar = raw_var(RK_AR, c, 0, j);
    raw_row(s, r++, RAW_EQ, (j + 1 == V.I[Y.i_init + c]) ? 1.0 : 0.0, ar, 1.0);
    const double* jl = V.D + Y.d_jerk + (c * R + j) * 4;
    for (int ax = 0; ax < 2; ++ax) {
      const RawVar u = raw_cont(ax ? CV_UY : CV_UX, c, 0);
      raw_row(s, r++, RAW_LE, jl[2 * ax + 1] + CERT_M_JERK, u, 1.0, ar, CERT_M_JERK);
      raw_row(s, r++, RAW_GE, jl[2 * ax] - CERT_M_JERK, u, 1.0, ar, -CERT_M_JERK);
    }
  }
  for (int it = tid; it < C * 5; it += nth) { const int c = it / 5, k = it - c * 5; raw_row(s, C * 12 + R * C * 5 + it, RAW_EQ, 0.0, raw_var(RK_RC + k, c, 0), 1.0); }
}

// A2 dynamics, model_region_constraints.mod:11-19
template <class S> CERT_HD void raw_A2(const CertView& V, int tid, int nth, S& s) {
  const CertLay& Y = V.Y; const int C = Y.C, N = Y.N; const double ts = V.S(CS_TS);
  for (int it = tid; it < (N - 1) * C * 2; it += nth) {
    const int ax = it & 1, ic = it >> 1, i = ic / C + 1, c = ic - (i - 1) * C; int r = V.base[1] + it * 3;
    const int P_ = ax ? CV_PY : CV_PX, V_ = ax ? CV_VY : CV_VX, A_ = ax ? CV_AY : CV_AX, U_ = ax ? CV_UY : CV_UX;
    const RawVar p0 = raw_cont(P_, c, i - 1), v0 = raw_cont(V_, c, i - 1), a0 = raw_cont(A_, c, i - 1), u0 = raw_cont(U_, c, i - 1);
    raw_row(s, r++, RAW_EQ, 0.0, raw_cont(P_, c, i), 1.0, p0, -1.0, v0, -ts, a0, -0.5 * ts * ts, u0, -ts * ts * ts / 6.0);
    raw_row(s, r++, RAW_EQ, 0.0, raw_cont(V_, c, i), 1.0, v0, -1.0, a0, -ts, u0, -0.5 * ts * ts);
    raw_row(s, r++, RAW_EQ, 0.0, raw_cont(A_, c, i), 1.0, a0, -1.0, u0, -ts);
  }
}

// A3 global limits :22-39 (the max_vel row bounds vel_x twice and vel_y never: the reference's model, kept)
template <class S> CERT_HD void raw_A3(const CertView& V, int tid, int nth, S& s) {
  const CertLay& Y = V.Y; const int C = Y.C, N = Y.N;
  const double vmin = V.S(CS_VMIN), vmax = V.S(CS_VMAX), amin = V.S(CS_AMIN), amax = V.S(CS_AMAX), jmin = V.S(CS_JMIN), jmax = V.S(CS_JMAX);
  for (int it = tid; it < N * C; it += nth) {
    const int i = it / C, c = it - i * C; int r = V.base[2] + it * 12;
    const RawVar vx = raw_var(CV_VX, c, i), vy = raw_var(CV_VY, c, i), ax = raw_var(CV_AX, c, i), ay = raw_var(CV_AY, c, i), ux = raw_var(CV_UX, c, i), uy = raw_var(CV_UY, c, i);
    raw_row(s, r++, RAW_GE, vmin, vx, 1.0); raw_row(s, r++, RAW_GE, vmin, vy, 1.0); raw_row(s, r++, RAW_LE, vmax, vx, 1.0); raw_row(s, r++, RAW_LE, vmax, vx, 1.0);
    raw_row(s, r++, RAW_LE, amax, ax, 1.0); raw_row(s, r++, RAW_GE, amin, ax, 1.0); raw_row(s, r++, RAW_LE, amax, ay, 1.0); raw_row(s, r++, RAW_GE, amin, ay, 1.0);
    raw_row(s, r++, RAW_LE, jmax, ux, 1.0); raw_row(s, r++, RAW_GE, jmin, ux, 1.0); raw_row(s, r++, RAW_LE, jmax, uy, 1.0); raw_row(s, r++, RAW_GE, jmin, uy, 1.0);
  }
}

// A4 region block :43-117; item (i, c, j), j == R: the sum row
template <class S> CERT_HD void raw_A4(const CertView& V, int tid, int nth, S& s) {
  const CertLay& Y = V.Y; const int C = Y.C, N = Y.N, R = Y.R;
  for (int it = tid; it < (N - 1) * C * (R + 1); it += nth) {
    const int j = it % (R + 1), ic = it / (R + 1), i = ic / C + 1, c = ic - (i - 1) * C;
    int r = V.base[3] + (i - 1) * V.a4tot + V.I[Y.i_cpre + c] + V.I[Y.i_a4off + c * (R + 1) + j];
    if (j == R) { s.begin(r); for (int jj = 0; jj < R; ++jj) s.term(raw_var(RK_AR, c, i, jj), 1.0); s.end(RAW_EQ, 1.0); continue; }
    const RawVar ar = raw_var(RK_AR, c, i, j);
    if (V.I[Y.i_poss + c * R + j] != 1) { raw_row(s, r, RAW_EQ, 0.0, ar, 1.0); continue; }
    const RawVar vx = raw_var(CV_VX, c, i), vy = raw_var(CV_VY, c, i), ax = raw_var(CV_AX, c, i), ay = raw_var(CV_AY, c, i), q = raw_var(RK_RC + 4, c, i);
    const double* F = V.D + Y.d_frac + j * 4;
    raw_row(s, r++, RAW_GE, -CERT_M_VELFRAC, vy, F[0], vx, -F[1], ar, -CERT_M_VELFRAC, q, CERT_M_VELFRAC);
    raw_row(s, r++, RAW_LE, CERT_M_VELFRAC, vy, F[2], vx, -F[3], ar, CERT_M_VELFRAC, q, -CERT_M_VELFRAC);
    const double wb = V.D[Y.d_wb + c];
    const int fv[4] = {CV_XFU, CV_XFL, CV_YFU, CV_YFL}, pv[4] = {CV_PX, CV_PX, CV_PY, CV_PY}, pt[4] = {2, 3, 0, 1};
    for (int k = 0; k < 4; ++k) {
      const double* p = V.D + Y.d_poly + (pt[k] * R + j) * 3;
      const RawVar f = raw_cont(fv[k], c, i), b = raw_cont(pv[k], c, i);
      raw_row(s, r++, RAW_GE, wb * p[0] - CERT_M_POSPOLY, f, 1.0, b, -1.0, vx, -wb * p[1], vy, -wb * p[2], ar, -CERT_M_POSPOLY);
      raw_row(s, r++, RAW_LE, wb * p[0] + CERT_M_POSPOLY, f, 1.0, b, -1.0, vx, -wb * p[1], vy, -wb * p[2], ar, CERT_M_POSPOLY);
    }
    const double* jl = V.D + Y.d_jerk + (c * R + j) * 4; const double* al = V.D + Y.d_acc + (c * R + j) * 4;
    for (int x = 0; x < 2; ++x) {
      const RawVar u = raw_cont(x ? CV_UY : CV_UX, c, i);
      raw_row(s, r++, RAW_LE, jl[2 * x + 1] + CERT_M_JERK, u, 1.0, ar, CERT_M_JERK); raw_row(s, r++, RAW_GE, jl[2 * x] - CERT_M_JERK, u, 1.0, ar, -CERT_M_JERK);
    }
    for (int x = 0; x < 2; ++x) {
      const RawVar av = x ? ay : ax;
      raw_row(s, r++, RAW_LE, al[2 * x + 1] + CERT_M_ACC, av, 1.0, ar, CERT_M_ACC); raw_row(s, r++, RAW_GE, al[2 * x] - CERT_M_ACC, av, 1.0, ar, -CERT_M_ACC);
    }
    const double rho = (F[1] + F[3]) / (F[0] + F[2]);
    const double* kx = V.D + Y.d_poly + (4 * R + j) * 3; const double* kn = V.D + Y.d_poly + (5 * R + j) * 3;
    raw_row(s, r++, RAW_LE, kx[0] + CERT_M_KAPPA, ay, 1.0, vx, -kx[1], vy, -kx[2], ax, -rho, ar, CERT_M_KAPPA, q, -CERT_M_KAPPA);
    raw_row(s, r++, RAW_GE, kn[0] - CERT_M_KAPPA, ay, 1.0, vx, -kn[1], vy, -kn[2], ax, -rho, ar, -CERT_M_KAPPA, q, CERT_M_KAPPA);
  }
}

// A5 minimum_speed_constraints.mod:9-49 (stated once per region, as OPL does)
template <class S> CERT_HD void raw_A5(const CertView& V, int tid, int nth, S& s) {
  const CertLay& Y = V.Y; const int C = Y.C, N = Y.N, R = Y.R; const double vm = V.S(CS_VM);
  for (int it = tid; it < (N - 1) * C * R; it += nth) {
    const int j = it % R, ic = it / R, i = ic / C + 1, c = ic - (i - 1) * C; int r = V.base[4] + it * 15;
    const RawVar xp = raw_var(RK_RC, c, i), yp = raw_var(RK_RC + 1, c, i), xn = raw_var(RK_RC + 2, c, i), yn = raw_var(RK_RC + 3, c, i), cb = raw_var(RK_RC + 4, c, i);
    for (int x = 0; x < 2; ++x) {
      const RawVar v = raw_cont(x ? CV_VY : CV_VX, c, i), p = x ? yp : xp, n_ = x ? yn : xn;
      raw_row(s, r++, RAW_GE, vm, v, 1.0, p, CERT_M_VEL); raw_row(s, r++, RAW_LE, vm + CERT_M_VEL, v, 1.0, p, CERT_M_VEL);
      raw_row(s, r++, RAW_LE, vm + CERT_M_VEL, v, -1.0, n_, CERT_M_VEL); raw_row(s, r++, RAW_GE, vm, v, -1.0, n_, CERT_M_VEL);
    }
    const RawVar a1 = raw_var(RK_AR, c, i, j), a0 = raw_var(RK_AR, c, i - 1, j);
    raw_row(s, r++, RAW_LE, 1.0, a1, 1.0, a0, -1.0, cb, 1.0); raw_row(s, r++, RAW_GE, -1.0, a1, 1.0, a0, -1.0, cb, -1.0);
    raw_row(s, r++, RAW_LE, 0.0, cb, 1.0, xp, -1.0); raw_row(s, r++, RAW_LE, 0.0, cb, 1.0, yp, -1.0);
    raw_row(s, r++, RAW_LE, 0.0, cb, 1.0, xn, -1.0); raw_row(s, r++, RAW_LE, 0.0, cb, 1.0, yn, -1.0);
    raw_row(s, r++, RAW_GE, -3.0, cb, 1.0, xp, -1.0, yp, -1.0, xn, -1.0, yn, -1.0);
  }
}

// cross product row of obstacle_environment_constraints.mod: cross((X, Y), e = <x1, y1, x2, y2>) + M * b, `sense` 0;
// the constant of the cross product goes to the right-hand side
template <class S> CERT_HD void raw_cross_row(S& s, int r, int sense, const double* e, const RawVar& X, const RawVar& Yv, const RawVar& b, double M) {
  const double dx = e[2] - e[0], dy = e[3] - e[1], k0 = -dx * e[1] + e[0] * dy;
  raw_row(s, r, sense, -k0, Yv, dx, X, -dy, b, M);
}

// A6 environment :6-47; item (i, c, k), k == NE: the five cardinality rows
template <class S> CERT_HD void raw_A6(const CertView& V, int tid, int nth, S& s) {
  const CertLay& Y = V.Y; const int C = Y.C, N = Y.N, E = Y.E, NE = Y.NE;
  if (E <= 0) return;
  const int ex[5] = {CV_PX, CV_XFU, CV_XFL, CV_XFU, CV_XFL}, ey[5] = {CV_PY, CV_YFU, CV_YFU, CV_YFL, CV_YFL};
  for (int it = tid; it < N * C * (NE + 1); it += nth) {
    const int k = it % (NE + 1), ic = it / (NE + 1), i = ic / C, c = ic - i * C; int r = V.base[5] + ic * (5 * NE + 5) + k * 5;
    if (k == NE) {
      for (int p = 0; p < 5; ++p) { s.begin(r++); for (int e = 0; e < E; ++e) s.term(raw_var(RK_NW + p, c, e, i), 1.0); s.end(RAW_LE, (double)(E - 1)); }
      continue;
    }
    const int e = V.I[Y.i_edge_env + k]; const double* ed = V.D + Y.d_env + k * 4;
    for (int p = 0; p < 5; ++p) raw_cross_row(s, r++, RAW_GE, ed, raw_cont(ex[p], c, i), raw_cont(ey[p], c, i), raw_var(RK_NW + p, c, e, i), CERT_M_ENV);
  }
}

// A7 obstacles :52-109; item (i, c, o, k), k == L: the five cardinality rows (with the soft obstacle's slack)
template <class S> CERT_HD void raw_A7(const CertView& V, int tid, int nth, S& s) {
  const CertLay& Y = V.Y; const int C = Y.C, N = Y.N, O = Y.O, L = Y.L;
  if (O <= 0) return;
  const int ox[5] = {CV_PX, CV_XFL, CV_XFU, CV_XFL, CV_XFU}, oy[5] = {CV_PY, CV_YFL, CV_YFL, CV_YFU, CV_YFU};
  for (int it = tid; it < N * C * O * (L + 1); it += nth) {
    const int k = it % (L + 1), ico = it / (L + 1), o = ico % O, ic = ico / O, i = ic / C, c = ic - i * C;
    int r = V.base[6] + ico * (5 * L + 5) + k * 5;
    if (k == L) {
      const bool soft = V.I[Y.i_soft + o] == 1;
      for (int p = 0; p < 5; ++p) {
        s.begin(r++); for (int kk = 0; kk < L; ++kk) s.term(raw_dv(p, c, o, i, kk), 1.0);
        if (soft) s.term(raw_so(p, c, o, i), -1.0);
        s.end(RAW_LE, (double)(L - 1));
      }
      continue;
    }
    const double* ed = V.D + Y.d_obs + ((size_t)(o * N + i) * L + k) * 4;
    for (int p = 0; p < 5; ++p) raw_cross_row(s, r++, RAW_LE, ed, raw_cont(ox[p], c, i), raw_cont(oy[p], c, i), raw_dv(p, c, o, i, k), -CERT_M_OBS);
  }
}

// A8 agent_collision_constraints.mod:10-73.  The sixteen separation rows as nibble tables (row w = 4 g + q, nibble w):
// left / right variable (kind of the continuous array), which car each belongs to (bit set: c2), the slack (15: none).
template <class S> CERT_HD void raw_A8(const CertView& V, int tid, int nth, S& s) {
  const CertLay& Y = V.Y; const int C = Y.C, N = Y.N, K = Y.K, NP = Y.NP;
  if (C <= 1) return;
  const int tri = (K - 1) * K / 2;
  for (int it = tid; it < N * tri; it += nth) {
    const int i = it / tri; int t = it - i * tri, c1 = 1; while (t >= c1) { t -= c1; ++c1; } const int c2 = t;
    int r = V.base[7] + it * 20;
    for (int q = 0; q < 4; ++q) raw_row(s, r++, RAW_EQ, 0.0, raw_var(RK_SL, c1, c2, i, q), 1.0);
    for (int q = 0; q < 16; ++q) raw_row(s, r++, RAW_EQ, 0.0, raw_var(RK_CC, c1, c2, i, q), 1.0);
  }
  const unsigned long long LV = 0xBA98552255225522ull;
  const unsigned long long RV = 0xAB89AB89AB895522ull;
  const unsigned LC2 = 0xFF00u, RC2 = 0x00FFu;           // left variable of c2 in rows 8..15, right variable of c2 in rows 0..7
  const unsigned long long SL = 0x3322FFFFFFFF1100ull;
  const int base_b = V.base[7] + N * 20 * tri;
  for (int it = tid; it < N * NP * 4; it += nth) {
    const int g = it & 3, ip = it >> 2, i = ip / NP; int t = ip - i * NP, c1 = 0; while (t >= C - 1 - c1) { t -= C - 1 - c1; ++c1; } const int c2 = c1 + 1 + t;
    const int goff = g == 0 ? 0 : 7 + 5 * (g - 1);
    int r = base_b + ip * 24 + goff;
    const double Dd = V.D[Y.d_rad + c1] + V.D[Y.d_rad + c2] + V.D[Y.d_safety + i], Ss = V.D[Y.d_sslack + i]; const int q2 = c2 - 1;
    for (int q = 0; q < 4; ++q) {
      const int w = 4 * g + q;
      const int lk = (int)((LV >> (4 * w)) & 15), rk = (int)((RV >> (4 * w)) & 15), sk = (int)((SL >> (4 * w)) & 15);
      const double sg = (q & 1) ? 1.0 : -1.0;
      s.begin(r++);
      s.term(raw_cont(lk, ((LC2 >> w) & 1) ? c2 : c1, i), 1.0); s.term(raw_cont(rk, ((RC2 >> w) & 1) ? c2 : c1, i), -1.0);
      s.term(raw_var(RK_CC, c1, q2, i, w), sg * CERT_M_AGENTS);
      if (sk != 15) s.term(raw_var(RK_SL, c1, q2, i, sk), sg);
      s.end((q & 1) ? RAW_GE : RAW_LE, sg * (Dd + (sk != 15 ? Ss : 0.0)));
    }
    s.begin(r++); for (int q = 0; q < 4; ++q) s.term(raw_var(RK_CC, c1, q2, i, 4 * g + q), 1.0); s.end(RAW_LE, 3.0);
    if (g == 0 || g == 3) for (int q = 0; q < 2; ++q) raw_row(s, r++, RAW_LE, Ss, raw_var(RK_SL, c1, q2, i, (g == 0 ? 0 : 2) + q), 1.0);
  }
}

template <class S> CERT_HD void raw_family(int f, const CertView& V, int tid, int nth, S& s) {
  switch (f) {
    case 0: raw_A1(V, tid, nth, s); break;
    case 1: raw_A2(V, tid, nth, s); break;
    case 2: raw_A3(V, tid, nth, s); break;
    case 3: raw_A4(V, tid, nth, s); break;
    case 4: raw_A5(V, tid, nth, s); break;
    case 5: raw_A6(V, tid, nth, s); break;
    case 6: raw_A7(V, tid, nth, s); break;
    default: raw_A8(V, tid, nth, s); break;
  }
}

// objective_function.mod:7-19 on the record: this thread's share of the sum (fixed order per thread)
CERT_HD double cert_objective(const CertView& V, int tid, int nth) {
  const CertLay& Y = V.Y; const int C = Y.C, N = Y.N;
  double s = 0.0;
  for (int it = tid; it < N * C; it += nth) {
    const int i = it / C, c = it - i * C; const double* W = V.D + Y.d_W + c * 8; const double* rf = V.D + Y.d_ref + (c * N + i) * 6;
    const double dx = V.X(CV_PX, c, i) - rf[0], dvx = V.X(CV_VX, c, i) - rf[1], dax = V.X(CV_AX, c, i) - rf[2];
    const double dy = V.X(CV_PY, c, i) - rf[3], dvy = V.X(CV_VY, c, i) - rf[4], day = V.X(CV_AY, c, i) - rf[5];
    const double ux = V.X(CV_UX, c, i), uy = V.X(CV_UY, c, i);
    s += W[0] * dx * dx + W[1] * dvx * dvx + W[2] * dax * dax + W[3] * dy * dy + W[4] * dvy * dvy + W[5] * day * day + W[6] * ux * ux + W[7] * uy * uy;
  }
  const double wo = V.S(CS_WSLACK_OBS), ws = V.S(CS_WSLACK);
  for (int q = tid; q < C * Y.O * N * 5; q += nth) { const double v = (double)V.B[Y.b_sO + q]; s += wo * v * v; }
  for (int q = tid; q < Y.K * Y.K * N * 4; q += nth) { const double v = V.D[Y.d_slack + q]; s += ws * v * v; }
  return s;
}

// distance of the delivered binaries from {0, 1} (they arrive as ints: 0 unless a member is outside {0, 1})
CERT_HD double cert_int_infeas(const CertView& V, int tid, int nth) {
  double w = 0.0;
  for (int q = tid; q < V.Y.nbin; q += nth) { const double b = (double)V.B[q]; const double d = b < 0.0 ? -b : b - 1.0; if (d > w) w = d; }
  return w;
}

// ---------------------------------------------------------------------------------------------------------------- packing (host)
inline int cert_edge_count(const HostInst& I) { return I.E > 0 ? I.env_off[I.E] : 0; }

inline size_t cert_blob_bytes(const HostInst& I) { CertLay Y; Y.init(I.C, I.N, I.R, I.E, I.O, I.L, cert_edge_count(I)); return Y.bytes; }

inline signed char cert_sat8(int v) { return (signed char)(v < -128 ? -128 : (v > 127 ? 127 : v)); }

// parameter block of `I` into `blob` (cert_blob_bytes(I) bytes), the record's members zero: all the row walker reads
inline void cert_pack_params(const HostInst& I, void* blob) {
  CertLay Y; Y.init(I.C, I.N, I.R, I.E, I.O, I.L, cert_edge_count(I));
  const int C = I.C, N = I.N, R = I.R, E = I.E, O = I.O, L = I.L;
  std::memset(blob, 0, Y.bytes);
  int* h = (int*)blob; h[0] = C; h[1] = N; h[2] = R; h[3] = E; h[4] = O; h[5] = L; h[6] = Y.NE; h[7] = 0;
  double* D = (double*)((char*)blob + 32); int* J = (int*)(D + Y.nd);
  double* s = D + Y.d_scal;
  s[CS_TS] = I.ts; s[CS_VMIN] = I.vmin; s[CS_VMAX] = I.vmax; s[CS_AMIN] = I.amin; s[CS_AMAX] = I.amax; s[CS_JMIN] = I.jmin; s[CS_JMAX] = I.jmax;
  s[CS_VM] = I.vm; s[CS_WSLACK] = I.w_slack; s[CS_WSLACK_OBS] = I.w_slack_obs;
  auto cp = [&](int off, const std::vector<double>& v, size_t n) { if (n) std::memcpy(D + off, v.data(), n * 8); };
  cp(Y.d_safety, I.safety, N); cp(Y.d_sslack, I.safety_slack, N); cp(Y.d_W, I.W, (size_t)C * 8); cp(Y.d_wb, I.wb, C); cp(Y.d_rad, I.rad, C);
  cp(Y.d_x0, I.x0, (size_t)C * 6); cp(Y.d_ref, I.ref, (size_t)C * N * 6); cp(Y.d_acc, I.acc_lim, (size_t)C * R * 4); cp(Y.d_jerk, I.jerk_lim, (size_t)C * R * 4);
  cp(Y.d_frac, I.frac, (size_t)R * 4);
  for (int k = 0; k < 6; ++k) cp(Y.d_poly + k * R * 3, I.poly[k], (size_t)R * 3);
  cp(Y.d_env, I.env_edges, (size_t)Y.NE * 4); cp(Y.d_obs, I.obs_edges, (size_t)O * N * L * 4);
  for (int c = 0; c < C; ++c) {   // the front axle at step 0, as initial_conditions.mod:30-45 fixes it
    const double th = std::atan2(I.x0[c * 6 + 4], I.x0[c * 6 + 1]);
    D[Y.d_front0 + 2 * c] = I.x0[c * 6] + std::cos(th) * I.wb[c]; D[Y.d_front0 + 2 * c + 1] = I.x0[c * 6 + 3] + std::sin(th) * I.wb[c];
  }
  for (int c = 0; c < C; ++c) J[Y.i_init + c] = I.init_region[c];
  int tot = 0;
  for (int c = 0; c < C; ++c) {
    int o = 0;
    for (int j = 0; j < R; ++j) { J[Y.i_poss + c * R + j] = I.possible[c * R + j]; J[Y.i_a4off + c * (R + 1) + j] = o; o += I.possible[c * R + j] == 1 ? 20 : 1; }
    J[Y.i_a4off + c * (R + 1) + R] = o;
    J[Y.i_cpre + c] = tot; tot += o + 1;
  }
  J[Y.i_cpre + C] = tot;
  for (int e = 0; e < E; ++e) for (int k = I.env_off[e]; k < I.env_off[e + 1]; ++k) J[Y.i_edge_env + k] = e;
  for (int o = 0; o < O; ++o) J[Y.i_soft + o] = I.obs_soft[o];
}

// the record `r` into a blob cert_pack_params has filled.  The car/car slacks are the record's real values when it carries
// them, else its truncated ints.  Integer members are stored as bytes, saturated to [-128, 127].
inline void cert_pack_record(const HostInst& I, const miqp_raw_results_c& r, void* blob) {
  CertLay Y; Y.init(I.C, I.N, I.R, I.E, I.O, I.L, cert_edge_count(I));
  const int C = I.C, N = I.N, R = I.R, E = I.E, O = I.O, L = I.L, K = C - 1;
  double* D = (double*)((char*)blob + 32); signed char* B = (signed char*)((int*)(D + Y.nd) + Y.ni);
  const double* const ct[12] = {r.u_x, r.u_y, r.pos_x, r.vel_x, r.acc_x, r.pos_y, r.vel_y, r.acc_y, r.pos_x_front_UB, r.pos_x_front_LB, r.pos_y_front_UB, r.pos_y_front_LB};
  for (int k = 0; k < 12; ++k) std::memcpy(D + Y.d_cont + (size_t)k * C * N, ct[k], (size_t)C * N * 8);
  for (int q = 0; q < K * K * N * 4; ++q) D[Y.d_slack + q] = r.slackvars_real ? r.slackvars_real[q] : (double)r.slackvars[q];
  auto pk = [&](int off, const int* v, size_t n) { for (size_t q = 0; q < n; ++q) B[off + q] = cert_sat8(v[q]); };
  const int* const nwp[5] = {r.notWithinEnvironmentRear, r.notWithinEnvironmentFrontUbUb, r.notWithinEnvironmentFrontLbUb, r.notWithinEnvironmentFrontUbLb, r.notWithinEnvironmentFrontLbLb};
  for (int p = 0; p < 5; ++p) pk(Y.b_nw + p * C * E * N, nwp[p], (size_t)C * E * N);
  pk(Y.b_ar, r.active_region, (size_t)C * N * R);
  const int* const rcp[5] = {r.region_change_not_allowed_x_positive, r.region_change_not_allowed_y_positive, r.region_change_not_allowed_x_negative,
                             r.region_change_not_allowed_y_negative, r.region_change_not_allowed_combined};
  for (int k = 0; k < 5; ++k) pk(Y.b_rc + k * C * N, rcp[k], (size_t)C * N);
  pk(Y.b_d, r.deltacc, (size_t)C * O * N * L); pk(Y.b_df, r.deltacc_front, (size_t)C * O * N * L * 4); pk(Y.b_cc, r.car2car_collision, (size_t)K * K * N * 16);
  pk(Y.b_sO, r.slackvarsObstacle, (size_t)C * O * N); pk(Y.b_sOf, r.slackvarsObstacle_front, (size_t)C * O * N * 4);
}

}  // namespace miqp

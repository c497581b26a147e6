// certify_rows.hpp - the raw big-M rows of cplexmodel/*.mod as closed-form index spaces, evaluated on one delivered record.
//
// Nothing here stores a matrix: a row is decoded from (family, item, k) and evaluated from the instance's parameter block
// and the record.  Row order, coefficients and big-M constants are those lp_export.hpp writes (parameters.mod:24-32), so
// `worst_row` is the 0-based index of the row `c<worst_row+1>` of miqp_solver_export_lp.  The code is shared by the kernel
// of certify.hip and by the host packer; only the kernel evaluates in the product build.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstring>

#include "host_inst.hpp"

#if defined(__HIPCC__)
#define CERT_HD __host__ __device__ __forceinline__
#else
#define CERT_HD inline
#endif

namespace miqp {

// ---------------------------------------------------------------------------------------------------------------- layout
// One instance = one blob: [header 8 int][doubles][ints][bytes], 16-byte padded.  Every offset follows from the header.
enum { CV_UX = 0, CV_UY, CV_PX, CV_VX, CV_AX, CV_PY, CV_VY, CV_AY, CV_XFU, CV_XFL, CV_YFU, CV_YFL };
enum { CS_TS = 0, CS_VMIN, CS_VMAX, CS_AMIN, CS_AMAX, CS_JMIN, CS_JMAX, CS_VM, CS_WSLACK, CS_WSLACK_OBS, CS_COUNT = 12 };

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
    const int C = Y.C, N = Y.N, R = Y.R;
    a4tot = I[Y.i_cpre + C];
    base[0] = 0;
    base[1] = C * 12 + R * C * 5 + C * 5;
    base[2] = base[1] + (N - 1) * C * 6;
    base[3] = base[2] + N * C * 12;
    base[4] = base[3] + (N - 1) * a4tot;
    base[5] = base[4] + (N - 1) * C * R * 15;
    base[6] = base[5] + (Y.E > 0 ? N * C * (5 * Y.NE + 5) : 0);
    base[7] = base[6] + (Y.O > 0 ? N * C * Y.O * (5 * Y.L + 5) : 0);
    base[8] = base[7] + (C > 1 ? N * 20 * ((Y.K - 1) * Y.K / 2) + 24 * N * Y.NP : 0);
  }
  CERT_HD double X(int k, int c, int i) const { return cont[(k * Y.C + c) * Y.N + i]; }
  CERT_HD double S(int k) const { return D[Y.d_scal + k]; }
  CERT_HD double ar(int c, int i, int j) const { return (double)B[Y.b_ar + (c * Y.N + i) * Y.R + j]; }
  CERT_HD double rc(int k, int c, int i) const { return (double)B[Y.b_rc + (k * Y.C + c) * Y.N + i]; }
  CERT_HD double nw(int p, int c, int e, int i) const { return (double)B[Y.b_nw + ((p * Y.C + c) * Y.E + e) * Y.N + i]; }
  CERT_HD double dv(int p, int c, int o, int i, int k) const {
    const int q = ((c * Y.O + o) * Y.N + i) * Y.L + k;
    return (double)(p == 0 ? B[Y.b_d + q] : B[Y.b_df + q * 4 + p - 1]);
  }
  CERT_HD double so(int p, int c, int o, int i) const {
    const int q = (c * Y.O + o) * Y.N + i;
    return (double)(p == 0 ? B[Y.b_sO + q] : B[Y.b_sOf + q * 4 + p - 1]);
  }
  CERT_HD double cc(int a, int b, int i, int s) const { return (double)B[Y.b_cc + ((a * Y.K + b) * Y.N + i) * 16 + s]; }
  CERT_HD double sl(int a, int b, int i, int s) const { return D[Y.d_slack + ((a * Y.K + b) * Y.N + i) * 4 + s]; }
};

// running maximum of one thread; rows arrive in increasing order, so `>` keeps the lowest index among equals
struct CertMax {
  double v; int row;
  CERT_HD void le(double lhs, double rhs, int r) { const double d = lhs - rhs; if (d > v) { v = d; row = r; } }
  CERT_HD void ge(double lhs, double rhs, int r) { const double d = rhs - lhs; if (d > v) { v = d; row = r; } }
  CERT_HD void eq(double lhs, double rhs, int r) { const double d = fabs(lhs - rhs); if (d > v) { v = d; row = r; } }
};

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
// Each evaluates the items tid, tid + nth, ... of its index space.

// A1 initial_conditions.mod:11-61
CERT_HD void cert_A1(const CertView& V, int tid, int nth, CertMax& m) {
  const CertLay& Y = V.Y; const int C = Y.C, N = Y.N, R = Y.R;
  for (int c = tid; c < C; c += nth) {
    int r = c * 12;
    const int sv[6] = {CV_PX, CV_VX, CV_AX, CV_PY, CV_VY, CV_AY};
    for (int k = 0; k < 6; ++k) m.eq(V.X(sv[k], c, 0), V.D[Y.d_x0 + c * 6 + k], r++);
    const double fx = V.D[Y.d_front0 + 2 * c], fy = V.D[Y.d_front0 + 2 * c + 1];
    m.eq(V.X(CV_XFU, c, 0), fx, r++); m.eq(V.X(CV_XFL, c, 0), fx, r++);
    m.eq(V.X(CV_YFU, c, 0), fy, r++); m.eq(V.X(CV_YFL, c, 0), fy, r++);
    m.eq(V.X(CV_UX, c, N - 1), 0.0, r++); m.eq(V.X(CV_UY, c, N - 1), 0.0, r++);
  }
  for (int it = tid; it < R * C; it += nth) {
    const int j = it / C, c = it - j * C; int r = C * 12 + it * 5;
    const double a = V.ar(c, 0, j);
    m.eq(a, (j + 1 == V.I[Y.i_init + c]) ? 1.0 : 0.0, r++);
    const double* jl = V.D + Y.d_jerk + (c * R + j) * 4;
    for (int ax = 0; ax < 2; ++ax) {
      const double u = V.X(ax ? CV_UY : CV_UX, c, 0);
      m.le(u + CERT_M_JERK * a, jl[2 * ax + 1] + CERT_M_JERK, r++);
      m.ge(u - CERT_M_JERK * a, jl[2 * ax] - CERT_M_JERK, r++);
    }
  }
  for (int it = tid; it < C * 5; it += nth) { const int c = it / 5, k = it - c * 5; m.eq(V.rc(k, c, 0), 0.0, C * 12 + R * C * 5 + it); }
}

// A2 dynamics, model_region_constraints.mod:11-19
CERT_HD void cert_A2(const CertView& V, int tid, int nth, CertMax& m) {
  const CertLay& Y = V.Y; const int C = Y.C, N = Y.N; const double ts = V.S(CS_TS);
  for (int it = tid; it < (N - 1) * C * 2; it += nth) {
    const int ax = it & 1, ic = it >> 1, i = ic / C + 1, c = ic - (i - 1) * C; int r = V.base[1] + it * 3;
    const int P_ = ax ? CV_PY : CV_PX, V_ = ax ? CV_VY : CV_VX, A_ = ax ? CV_AY : CV_AX, U_ = ax ? CV_UY : CV_UX;
    const double p0 = V.X(P_, c, i - 1), v0 = V.X(V_, c, i - 1), a0 = V.X(A_, c, i - 1), u0 = V.X(U_, c, i - 1);
    m.eq(V.X(P_, c, i) - p0 - ts * v0 - 0.5 * ts * ts * a0 - ts * ts * ts / 6.0 * u0, 0.0, r++);
    m.eq(V.X(V_, c, i) - v0 - ts * a0 - 0.5 * ts * ts * u0, 0.0, r++);
    m.eq(V.X(A_, c, i) - a0 - ts * u0, 0.0, r++);
  }
}

// A3 global limits :22-39 (the max_vel row bounds vel_x twice and vel_y never: the reference's model, kept)
CERT_HD void cert_A3(const CertView& V, int tid, int nth, CertMax& m) {
  const CertLay& Y = V.Y; const int C = Y.C, N = Y.N;
  const double vmin = V.S(CS_VMIN), vmax = V.S(CS_VMAX), amin = V.S(CS_AMIN), amax = V.S(CS_AMAX), jmin = V.S(CS_JMIN), jmax = V.S(CS_JMAX);
  for (int it = tid; it < N * C; it += nth) {
    const int i = it / C, c = it - i * C; int r = V.base[2] + it * 12;
    const double vx = V.X(CV_VX, c, i), vy = V.X(CV_VY, c, i), ax = V.X(CV_AX, c, i), ay = V.X(CV_AY, c, i), ux = V.X(CV_UX, c, i), uy = V.X(CV_UY, c, i);
    m.ge(vx, vmin, r++); m.ge(vy, vmin, r++); m.le(vx, vmax, r++); m.le(vx, vmax, r++);
    m.le(ax, amax, r++); m.ge(ax, amin, r++); m.le(ay, amax, r++); m.ge(ay, amin, r++);
    m.le(ux, jmax, r++); m.ge(ux, jmin, r++); m.le(uy, jmax, r++); m.ge(uy, jmin, r++);
  }
}

// A4 region block :43-117; item (i, c, j), j == R: the sum row
CERT_HD void cert_A4(const CertView& V, int tid, int nth, CertMax& m) {
  const CertLay& Y = V.Y; const int C = Y.C, N = Y.N, R = Y.R;
  for (int it = tid; it < (N - 1) * C * (R + 1); it += nth) {
    const int j = it % (R + 1), ic = it / (R + 1), i = ic / C + 1, c = ic - (i - 1) * C;
    int r = V.base[3] + (i - 1) * V.a4tot + V.I[Y.i_cpre + c] + V.I[Y.i_a4off + c * (R + 1) + j];
    if (j == R) { double s = 0.0; for (int jj = 0; jj < R; ++jj) s += V.ar(c, i, jj); m.eq(s, 1.0, r); continue; }
    const double a = V.ar(c, i, j);
    if (V.I[Y.i_poss + c * R + j] != 1) { m.eq(a, 0.0, r); continue; }
    const double vx = V.X(CV_VX, c, i), vy = V.X(CV_VY, c, i), ax = V.X(CV_AX, c, i), ay = V.X(CV_AY, c, i), q = V.rc(4, c, i);
    const double* F = V.D + Y.d_frac + j * 4;
    m.ge(F[0] * vy - F[1] * vx - CERT_M_VELFRAC * a + CERT_M_VELFRAC * q, -CERT_M_VELFRAC, r++);
    m.le(F[2] * vy - F[3] * vx + CERT_M_VELFRAC * a - CERT_M_VELFRAC * q, CERT_M_VELFRAC, r++);
    const double wb = V.D[Y.d_wb + c];
    const int fv[4] = {CV_XFU, CV_XFL, CV_YFU, CV_YFL}, pv[4] = {CV_PX, CV_PX, CV_PY, CV_PY}, pt[4] = {2, 3, 0, 1};
    for (int k = 0; k < 4; ++k) {
      const double* p = V.D + Y.d_poly + (pt[k] * R + j) * 3;
      const double l = V.X(fv[k], c, i) - V.X(pv[k], c, i) - wb * p[1] * vx - wb * p[2] * vy;
      m.ge(l - CERT_M_POSPOLY * a, wb * p[0] - CERT_M_POSPOLY, r++);
      m.le(l + CERT_M_POSPOLY * a, wb * p[0] + CERT_M_POSPOLY, r++);
    }
    const double* jl = V.D + Y.d_jerk + (c * R + j) * 4; const double* al = V.D + Y.d_acc + (c * R + j) * 4;
    for (int x = 0; x < 2; ++x) {
      const double u = V.X(x ? CV_UY : CV_UX, c, i);
      m.le(u + CERT_M_JERK * a, jl[2 * x + 1] + CERT_M_JERK, r++); m.ge(u - CERT_M_JERK * a, jl[2 * x] - CERT_M_JERK, r++);
    }
    for (int x = 0; x < 2; ++x) {
      const double av = x ? ay : ax;
      m.le(av + CERT_M_ACC * a, al[2 * x + 1] + CERT_M_ACC, r++); m.ge(av - CERT_M_ACC * a, al[2 * x] - CERT_M_ACC, r++);
    }
    const double rho = (F[1] + F[3]) / (F[0] + F[2]);
    const double* kx = V.D + Y.d_poly + (4 * R + j) * 3; const double* kn = V.D + Y.d_poly + (5 * R + j) * 3;
    m.le(ay - kx[1] * vx - kx[2] * vy - rho * ax + CERT_M_KAPPA * a - CERT_M_KAPPA * q, kx[0] + CERT_M_KAPPA, r++);
    m.ge(ay - kn[1] * vx - kn[2] * vy - rho * ax - CERT_M_KAPPA * a + CERT_M_KAPPA * q, kn[0] - CERT_M_KAPPA, r++);
  }
}

// A5 minimum_speed_constraints.mod:9-49 (stated once per region, as OPL does)
CERT_HD void cert_A5(const CertView& V, int tid, int nth, CertMax& m) {
  const CertLay& Y = V.Y; const int C = Y.C, N = Y.N, R = Y.R; const double vm = V.S(CS_VM);
  for (int it = tid; it < (N - 1) * C * R; it += nth) {
    const int j = it % R, ic = it / R, i = ic / C + 1, c = ic - (i - 1) * C; int r = V.base[4] + it * 15;
    const double xp = V.rc(0, c, i), yp = V.rc(1, c, i), xn = V.rc(2, c, i), yn = V.rc(3, c, i), cb = V.rc(4, c, i);
    for (int x = 0; x < 2; ++x) {
      const double v = V.X(x ? CV_VY : CV_VX, c, i), p = x ? yp : xp, n_ = x ? yn : xn;
      m.ge(v + CERT_M_VEL * p, vm, r++); m.le(v + CERT_M_VEL * p, vm + CERT_M_VEL, r++);
      m.le(-v + CERT_M_VEL * n_, vm + CERT_M_VEL, r++); m.ge(-v + CERT_M_VEL * n_, vm, r++);
    }
    const double da = V.ar(c, i, j) - V.ar(c, i - 1, j);
    m.le(da + cb, 1.0, r++); m.ge(da - cb, -1.0, r++);
    m.le(cb - xp, 0.0, r++); m.le(cb - yp, 0.0, r++); m.le(cb - xn, 0.0, r++); m.le(cb - yn, 0.0, r++);
    m.ge(cb - xp - yp - xn - yn, -3.0, r++);
  }
}

// cross product of obstacle_environment_constraints.mod as lhs + k0, with (X, Y) the point and e = <x1, y1, x2, y2>
CERT_HD double cert_cross(const double* e, double X, double Yc, double& k0) {
  const double dx = e[2] - e[0], dy = e[3] - e[1];
  k0 = -dx * e[1] + e[0] * dy;
  return dx * Yc - dy * X;
}

// A6 environment :6-47; item (i, c, k), k == NE: the five cardinality rows
CERT_HD void cert_A6(const CertView& V, int tid, int nth, CertMax& m) {
  const CertLay& Y = V.Y; const int C = Y.C, N = Y.N, E = Y.E, NE = Y.NE;
  if (E <= 0) return;
  const int ex[5] = {CV_PX, CV_XFU, CV_XFL, CV_XFU, CV_XFL}, ey[5] = {CV_PY, CV_YFU, CV_YFU, CV_YFL, CV_YFL};
  for (int it = tid; it < N * C * (NE + 1); it += nth) {
    const int k = it % (NE + 1), ic = it / (NE + 1), i = ic / C, c = ic - i * C; int r = V.base[5] + ic * (5 * NE + 5) + k * 5;
    if (k == NE) {
      for (int p = 0; p < 5; ++p) { double s = 0.0; for (int e = 0; e < E; ++e) s += V.nw(p, c, e, i); m.le(s, (double)(E - 1), r++); }
      continue;
    }
    const int e = V.I[Y.i_edge_env + k]; const double* ed = V.D + Y.d_env + k * 4;
    for (int p = 0; p < 5; ++p) {
      double k0; const double l = cert_cross(ed, V.X(ex[p], c, i), V.X(ey[p], c, i), k0);
      m.ge(l + CERT_M_ENV * V.nw(p, c, e, i), -k0, r++);
    }
  }
}

// A7 obstacles :52-109; item (i, c, o, k), k == L: the five cardinality rows (with the soft obstacle's slack)
CERT_HD void cert_A7(const CertView& V, int tid, int nth, CertMax& m) {
  const CertLay& Y = V.Y; const int C = Y.C, N = Y.N, O = Y.O, L = Y.L;
  if (O <= 0) return;
  const int ox[5] = {CV_PX, CV_XFL, CV_XFU, CV_XFL, CV_XFU}, oy[5] = {CV_PY, CV_YFL, CV_YFL, CV_YFU, CV_YFU};
  for (int it = tid; it < N * C * O * (L + 1); it += nth) {
    const int k = it % (L + 1), ico = it / (L + 1), o = ico % O, ic = ico / O, i = ic / C, c = ic - i * C;
    int r = V.base[6] + ico * (5 * L + 5) + k * 5;
    if (k == L) {
      const bool soft = V.I[Y.i_soft + o] == 1;
      for (int p = 0; p < 5; ++p) {
        double s = 0.0; for (int kk = 0; kk < L; ++kk) s += V.dv(p, c, o, i, kk);
        if (soft) s -= V.so(p, c, o, i);
        m.le(s, (double)(L - 1), r++);
      }
      continue;
    }
    const double* ed = V.D + Y.d_obs + ((size_t)(o * N + i) * L + k) * 4;
    for (int p = 0; p < 5; ++p) {
      double k0; const double l = cert_cross(ed, V.X(ox[p], c, i), V.X(oy[p], c, i), k0);
      m.le(l - CERT_M_OBS * V.dv(p, c, o, i, k), -k0, r++);
    }
  }
}

// A8 agent_collision_constraints.mod:10-73.  The sixteen separation rows as nibble tables (row r = 4 g + q):
// left / right variable (index of the continuous array), which car each belongs to (bit set: c2), the slack (15: none).
CERT_HD void cert_A8(const CertView& V, int tid, int nth, CertMax& m) {
  const CertLay& Y = V.Y; const int C = Y.C, N = Y.N, K = Y.K, NP = Y.NP;
  if (C <= 1) return;
  const int tri = (K - 1) * K / 2;
  for (int it = tid; it < N * tri; it += nth) {
    const int i = it / tri; int t = it - i * tri, c1 = 1; while (t >= c1) { t -= c1; ++c1; } const int c2 = t;
    int r = V.base[7] + it * 20;
    for (int s = 0; s < 4; ++s) m.eq(V.sl(c1, c2, i, s), 0.0, r++);
    for (int s = 0; s < 16; ++s) m.eq(V.cc(c1, c2, i, s), 0.0, r++);
  }
  const unsigned long long LV = 0xBA98552255225522ull;   // nibble w = row w; the same sixteen rows as the table in lp_export.hpp
  const unsigned long long RV = 0xAB89AB89AB895522ull;
  const unsigned LC2 = 0xFF00u, RC2 = 0x00FFu;           // left variable of c2 in rows 8..15, right variable of c2 in rows 0..7
  const unsigned long long SL = 0x3322FFFFFFFF1100ull;
  const int base_b = V.base[7] + N * 20 * tri;
  for (int it = tid; it < N * NP * 4; it += nth) {
    const int g = it & 3, ip = it >> 2, i = ip / NP; int t = ip - i * NP, c1 = 0; while (t >= C - 1 - c1) { t -= C - 1 - c1; ++c1; } const int c2 = c1 + 1 + t;
    const int goff = g == 0 ? 0 : 7 + 5 * (g - 1);
    int r = base_b + ip * 24 + goff;
    const double Dd = V.D[Y.d_rad + c1] + V.D[Y.d_rad + c2] + V.D[Y.d_safety + i], Ss = V.D[Y.d_sslack + i]; const int q2 = c2 - 1;
    double card = 0.0;
    for (int q = 0; q < 4; ++q) {
      const int w = 4 * g + q;
      const int lk = (int)((LV >> (4 * w)) & 15), rk = (int)((RV >> (4 * w)) & 15), sk = (int)((SL >> (4 * w)) & 15);
      const double lv = V.X(lk, ((LC2 >> w) & 1) ? c2 : c1, i), rv = V.X(rk, ((RC2 >> w) & 1) ? c2 : c1, i);
      const double b = V.cc(c1, q2, i, w), sg = (q & 1) ? 1.0 : -1.0;
      card += b;
      double l = lv - rv + sg * CERT_M_AGENTS * b, rhs = sg * Dd;
      if (sk != 15) { l += sg * V.sl(c1, q2, i, sk); rhs = sg * (Dd + Ss); }
      if (q & 1) m.ge(l, rhs, r++); else m.le(l, rhs, r++);
    }
    m.le(card, 3.0, r++);
    if (g == 0 || g == 3) for (int q = 0; q < 2; ++q) m.le(V.sl(c1, q2, i, (g == 0 ? 0 : 2) + q), Ss, r++);
  }
}

CERT_HD void cert_family(int f, const CertView& V, int tid, int nth, CertMax& m) {
  switch (f) {
    case 0: cert_A1(V, tid, nth, m); break;
    case 1: cert_A2(V, tid, nth, m); break;
    case 2: cert_A3(V, tid, nth, m); break;
    case 3: cert_A4(V, tid, nth, m); break;
    case 4: cert_A5(V, tid, nth, m); break;
    case 5: cert_A6(V, tid, nth, m); break;
    case 6: cert_A7(V, tid, nth, m); break;
    default: cert_A8(V, tid, nth, m); break;
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

// parameter block of `I` and the record `r` into `blob` (cert_blob_bytes(I) bytes).  The car/car slacks are the record's
// real values when it carries them, else its truncated ints.  Integer members are stored as bytes, saturated to [-128, 127].
inline void cert_pack(const HostInst& I, const miqp_raw_results_c& r, void* blob) {
  CertLay Y; Y.init(I.C, I.N, I.R, I.E, I.O, I.L, cert_edge_count(I));
  const int C = I.C, N = I.N, R = I.R, E = I.E, O = I.O, L = I.L, K = C - 1;
  std::memset(blob, 0, Y.bytes);
  int* h = (int*)blob; h[0] = C; h[1] = N; h[2] = R; h[3] = E; h[4] = O; h[5] = L; h[6] = Y.NE; h[7] = 0;
  double* D = (double*)((char*)blob + 32); int* J = (int*)(D + Y.nd); signed char* B = (signed char*)(J + Y.ni);
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
  const double* const ct[12] = {r.u_x, r.u_y, r.pos_x, r.vel_x, r.acc_x, r.pos_y, r.vel_y, r.acc_y, r.pos_x_front_UB, r.pos_x_front_LB, r.pos_y_front_UB, r.pos_y_front_LB};
  for (int k = 0; k < 12; ++k) std::memcpy(D + Y.d_cont + (size_t)k * C * N, ct[k], (size_t)C * N * 8);
  for (int q = 0; q < K * K * N * 4; ++q) D[Y.d_slack + q] = r.slackvars_real ? r.slackvars_real[q] : (double)r.slackvars[q];
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

// oc_decode.hip - from a node's fix record to the rows the on-chip node kernels work on (included by kernels.hip in front of ipm_onchip.hip and
// as_onchip.hip): the LDS block both kernels share, the tests of a (stage, slot) pair.  The decode itself - pass A and
// pass B - exists ONCE, as the text of oc_decode_body.inc, which ipm_onchip_kernel and as_onchip_kernel include into their node loop.
//
// What the decode leaves behind (one node, one wavefront):
//   * box rows (one coefficient +-1) as the orderable key of their tightest right-hand side at bkey[(stage * 2 + side) * 16 + column], ~0: no row;
//   * general rows (2..6 coefficients) packed in (stage, slot) order: gmeta[row] (x,y: column map, nibble c = 1 + index of the coefficient of
//     column c; z: coefficient offset | nn << 16 | stage << 20 | soft << 31; w: columns, 4 bits each), their coefficients in gcoef, their
//     right-hand sides in grhs, their number in sstart[N + 1].
// The kernels differ in four places, the static members of the policy type each names (IpmDecode in ipm_onchip.hip, AsDecode in as_onchip.hip):
//   col(l)         model column -> the kernel's column of a stage;
//   LANE_BOUNDS    the state / input bounds (classes 0 and 1) by one lane per (car, stage) instead of slot by slot through the full test;
//   ROW_IDENTITY   pass B leaves the (stage, slot) code of every packed row in cand[row] instead of the rows per stage in sstart[stage + 1];
//   MARKS          the profile build reads the clock where the sparse classes begin and where pass A ends (the active-set kernel's counters 9 and
//                  11; the interior point's marks, OCP_T, stand around the decode).
// What follows an overflow, and the prefix sum over sstart, are the kernels' own.
namespace miqp {

constexpr int OC_GCAP = 128;      // general rows kept on chip (2 register slots per lane)
constexpr int OC_SCR = 32;        // rows decoded per round through the dense scratch rows
constexpr int OC_SSTR = 17;       // stride of a scratch row (conflict free)
constexpr int OC_KL0 = 6;         // stages whose gains stay in LDS (interior point)

struct OcLds { int z, u, r, gmeta, gcoef, grhs, wd, sstart, cand, fix, total; };   // byte offsets
// capacity of the larger variant of the kernel (the nodes the standard one hands on: rounding probes and the other nodes with up
// to OC_GCAP_BIG general rows): 5 register slots per lane, one wavefront per SIMD, 4 blocks of ~34 KB per CU
constexpr int OC_GCAP_BIG = 320;
// packed coefficients of a block's general rows (432: with N = 20 and a 480-byte fix record the standard block stays within 160 KB / 8: 2 wavefronts per SIMD)
__host__ __device__ constexpr int oc_gcoef_of(int gcap) { return gcap == 128 ? 432 : gcap * 7 / 2; }
// (as_std: the block of the standard active-set launch - its second region holds one stage vector and the decode scratch, its third the box keys
// alone: 768 B less at N = 20, so that eight blocks leave 6 KB of a CU's 160 KB free instead of none - with none, the holes the larger launches'
// 34 KB blocks leave behind kept every CU at six or seven blocks, tools/wave_dump.py)
__host__ __device__ inline OcLds oc_lds_layout(int N, int fixlen, int OC_GCAP = miqp::OC_GCAP, bool as_std = false) {
  const int OC_GCOEF = oc_gcoef_of(OC_GCAP);
  OcLds L; int o = 0;
  L.z = o; o += N * 16 * 8;
  L.u = o; { int a = as_std ? N * 16 * 8 : N * 32 * 8, b = OC_SCR * OC_SSTR * 8; o += a > b ? a : b; }    // D | Gd  /  dZ | gains  /  decode scratch
  L.r = o; { int a = N * 32 * 8, b = as_std ? 0 : OC_GCAP * 16 + OC_KL0 * 64 * 8; o += a > b ? a : b; }   // box right-hand side keys (decode) / (sqrt(w), f) of the general rows + gains of the first stages
  L.gmeta = o; o += OC_GCAP * 16;
  L.gcoef = o; o += OC_GCOEF * 8;
  L.grhs = o; o += OC_GCAP * 8;
  L.wd = o; o += 16 * 8;
  L.sstart = o; o += ((N + 2) * 4 + 7) & ~7;
  L.cand = o; o += (OC_GCAP + 64) * 2;
  L.fix = o; o += (fixlen + 15) & ~15;
  L.total = (o + 15) & ~15;
  return L;
}

#define OC_WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)

// box row of (stage, slot), if that slot carries a row with a single coefficient +-1: column, sign, right-hand side
// (the cases of decode_row whose row touches one stage variable)
template <int C>
__device__ inline bool box_of_slot(const Layout& Y, const double* D, const int* T, const signed char* fix, int i, int slot, int& col, double& sgn, double& rhs) {
  if (slot >= C * Y.SC) return false;
  const int N = Y.N;
  const double* G = D + Y.d_glob;
  const int c = slot / Y.SC, rr = slot - c * Y.SC;
  const int code = i >= 1 ? (int)fix[Y.f_reg + c * N + i] : -1;
  const double* rt = code >= 0 ? D + Y.d_reg + (c * Y.P + (code >> 2)) * REGSZ : nullptr;
  if (rr < 7) {
    const double* Hc = (rt || rr < 3) ? D : region_hull(Y, D, T, fix, c, i);   // (only read when the region is undecided)
    switch (rr) {
      case 0: col = 6 * c + 1; sgn = -1; rhs = -G[0]; break;
      case 1: col = 6 * c + 4; sgn = -1; rhs = -G[0]; break;
      case 2: col = 6 * c + 1; sgn = 1; rhs = G[1]; break;
      case 3: col = 6 * c + 2; sgn = 1; rhs = rt ? rt[12] : Hc[1]; break;
      case 4: col = 6 * c + 2; sgn = -1; rhs = -(rt ? rt[11] : Hc[0]); break;
      case 5: col = 6 * c + 5; sgn = 1; rhs = rt ? rt[14] : Hc[3]; break;
      default: col = 6 * c + 5; sgn = -1; rhs = -(rt ? rt[13] : Hc[2]); break;
    }
    return true;
  }
  if (rr < 11) {
    const int s = (rr - 7) >> 1; const bool up = ((rr - 7) & 1) == 0;
    double lo, hi;
    if (i == 0) { lo = D[Y.d_u0box + c * 4 + 2 * s]; hi = D[Y.d_u0box + c * 4 + 2 * s + 1]; }
    else if (rt) { lo = rt[15 + 2 * s]; hi = rt[16 + 2 * s]; }
    else { const double* Hc = region_hull(Y, D, T, fix, c, i); lo = Hc[4 + 2 * s]; hi = Hc[5 + 2 * s]; }
    col = 6 * C + 2 * c + s; sgn = up ? 1.0 : -1.0; rhs = up ? hi : -lo;
    return true;
  }
  if (rr < 16) {
    if (code < 0) return false;   // the hull rows of an undecided region are general rows
    const int h = code & 3, k = rr - 11;
    if (h == 3) { col = 6 * c + (k < 2 ? 1 : 4); sgn = (k & 1) ? -1.0 : 1.0; rhs = G[6]; return true; }
    if (k == 2) {
      const int* hs = T + Y.i_hs + ((c * Y.P + (code >> 2)) * 2 + h) * 2;
      col = 6 * c + (hs[0] == 0 ? 1 : 4); sgn = -(double)hs[1]; rhs = -G[6];
      return true;
    }
    return false;
  }
  int q = rr - 16;
  const double* ed;
  if (q < 5 * Y.EL) {
    const int pt = q / Y.EL, k = q - pt * Y.EL;
    if (pt != 0) return false;
    const int e = Y.E == 1 ? 0 : (int)fix[Y.f_env + (c * N + i) * 5];
    ed = D + Y.d_env + (e * Y.EL + k) * 3;
  } else {
    q -= 5 * Y.EL;
    const int o = q / 5, pt = q - o * 5;
    if (pt != 0) return false;
    const int kk = (int)fix[Y.f_obs + ((c * Y.O + o) * N + i) * 5];
    ed = D + Y.d_obs + ((o * N + i) * Y.L + kk) * 3;
  }
  if (ed[1] == 0.0 && fabs(ed[0]) == 1.0) { col = 6 * c; sgn = ed[0]; rhs = ed[2]; return true; }
  if (ed[0] == 0.0 && fabs(ed[1]) == 1.0) { col = 6 * c + 3; sgn = ed[1]; rhs = ed[2]; return true; }
  return false;
}

// cheap necessary condition for slot (i, slot) to carry a row, from the fix record alone (the first tests of decode_row; no
// table loads): the decode walks all N x NSLOT slots with this and runs the full test only on the few hundred survivors
template <int C>
__device__ inline bool slot_maybe(const Layout& Y, const signed char* fix, int i, int slot) {
  const int N = Y.N;
  if (slot < C * Y.SC) {
    const int c = slot / Y.SC, rr = slot - c * Y.SC;
    if (rr < 11) return true;
    if (i < 1) return false;
    const int code = (int)fix[Y.f_reg + c * N + i];
    if (rr < 16) return code >= 0 ? ((code & 3) != 3 || rr - 11 <= 3) : rr - 11 <= 1;
    int q = rr - 16;
    if (q < 5 * Y.EL) {
      if (Y.E < 1) return false;
      const int pt = q / Y.EL;
      const int e = Y.E == 1 ? 0 : (int)fix[Y.f_env + (c * N + i) * 5 + pt];
      return e >= 0 && (pt == 0 || code >= 0);
    }
    q -= 5 * Y.EL;
    const int o = q / 5, pt = q - o * 5;
    const int kk = (int)fix[Y.f_obs + ((c * Y.O + o) * N + i) * 5 + pt];
    return kk >= 0 && kk < Y.L && (pt == 0 || code >= 0);
  }
  if (C < 2 || i < 1) return false;
  const int q = slot - C * Y.SC;
  if (q < Y.NP * 8) { const int p = q >> 3, grp = (q & 7) >> 1; return (int)fix[Y.f_c2c + (p * N + i) * 4 + grp] >= 0; }
  const int q2 = q - Y.NP * 8, p = q2 >> 4, grp = (q2 >> 2) & 3, alt = q2 & 3;
  const int m = (int)fix[Y.f_c2n + (p * N + i) * 4 + grp];
  return m > 0 && ((m >> alt) & 1);
}

}  // namespace miqp

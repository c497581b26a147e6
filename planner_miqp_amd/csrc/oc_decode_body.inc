// oc_decode_body.inc - pass A and pass B of the on-chip decode (oc_decode.hip), as the statements of a kernel's body: ipm_onchip_kernel and
// as_onchip_kernel include this text once each, inside their node loop.  (Text and not a function: a function is optimised on its own before it is
// inlined, and every production instantiation of the two kernels then came out with other registers and spills than before; as text the kernels'
// code is what it was when each carried a copy - profiles/decode_shared_isa.txt.)
//
// The including kernel defines OC_DECODE_POLICY (oc_decode.hip: IpmDecode / AsDecode - the four places where the kernels differ) and has in scope
//   C, NZ, OC_GCAP, OC_GCOEF   car count, columns of a stage, capacities of its block (general rows, their coefficients)
//   Y, D, T, fix               the node's tables and its fix record (in LDS)
//   N, NSLOT, tid, lt          Y.N, Y.NSLOT, the lane and the mask of the lanes below it
//   L0, LL                     the LDS block and its layout (oc_lds_layout)
//   scr, bkey, gmeta, gcoef, grhs, sstart, cand   the regions the decode writes; on entry bkey = ~0 and sstart = 0 (the kernels' per-node prologue)
// and finds afterwards
//   ngen, overflow, ncoef      general rows found by pass A; more rows or coefficients than the block holds (nothing packed is usable then, and
//                              sstart[N + 1] is stale); coefficients packed
//   sstart[N + 1]              general rows packed (read it behind the overflow branches, as the kernels do)
//   MIQP_PROFILE and OC_DECODE_POLICY::MARKS: ocd_t_sparse, ocd_t_rows - clock64() when the sparse classes began and when pass A ended.
#ifdef MIQP_PROFILE
    long long ocd_t_sparse = 0, ocd_t_rows = 0;
#endif
    // ---- pass A: which (stage, slot) pairs carry a row; box rows go straight to their key, general rows are marked in a
    // bitmap over (stage, slot).  The pairs are walked class by class (velocity / acceleration bounds, jerk bounds, region
    // rows, rear-point edges, front-point edges, obstacles, car/car, car/car exclusions), so that the lanes of one pass take
    // the same branch of the decoder and their table loads go out together; the bitmap restores the (stage, slot) order.
    int ngen = 0;
    {
      unsigned long long* const bmp = (unsigned long long*)scr;          // [nw] one bit per (stage, slot)
      const int nw = (N * NSLOT + 63) >> 6;
      unsigned short* const pre = (unsigned short*)(bmp + nw);           // [nw] general rows before every word
      for (int k = tid; k < nw; k += 64) bmp[k] = 0ull;
      OC_WAVE_SYNC();
      const int cls_off[8] = {0, 7, 11, 16, 16 + Y.EL, 16 + 5 * Y.EL, C * Y.SC, C * Y.SC + 8 * Y.NP};
      const int cls_cnt[8] = {7, 4, 5, Y.EL, 4 * Y.EL, 5 * Y.O, 8 * Y.NP, 16 * Y.NP};
      auto take = [&](int i, int slot) {   // full test of one (stage, slot); box rows to their key, general rows to the bitmap
        if (decode_row<C, false>(Y, D, T, fix, i, slot, nullptr).active) {
          int col; double sg, rh;
          if (box_of_slot<C>(Y, D, T, fix, i, slot, col, sg, rh)) atomicMin(&bkey[(i * 2 + (sg < 0.0 ? 1 : 0)) * 16 + OC_DECODE_POLICY::col(col)], d2key(rh));
          else { const int pcode = i * NSLOT + slot; atomicOr(&bmp[pcode >> 6], 1ull << (pcode & 63)); }
        }
      };
      // the candidates of the sparse classes (everything but the state / input bounds) are collected first with the cheap test
      unsigned short* const plist = pre + ((nw + 1 + 3) & ~3);
      const int LCAP = (int)(((char*)(L0 + LL.r) - (char*)plist) / 2) - 64;
      int nlist = 0;
      auto flush = [&]() {
        OC_WAVE_SYNC();
        for (int j0 = 0; j0 < nlist; j0 += 64) if (j0 + tid < nlist) { const int pc = plist[j0 + tid]; const int i = pc / NSLOT; take(i, pc - i * NSLOT); }
        OC_WAVE_SYNC();
        nlist = 0;
      };
      if constexpr (OC_DECODE_POLICY::LANE_BOUNDS) {
        // The state / input bounds (slots 0..10 of every car and stage: decode_row's cases rr < 11 with box_of_slot's right-hand sides) - three
        // quarters of a node's rows - one LANE PER (car, stage): its skip word, its region code and the eight box values (the region's table or the
        // hull of the region set) are loaded once for the eleven rows, instead of eleven walks through decode_row and box_of_slot in eight passes
        for (int e0 = 0; e0 < C * N; e0 += 64) {
          const int e = e0 + tid;
          if (e < C * N) {
            const int c = e / N, i = e - c * N;
            const double* G = D + Y.d_glob;
            const int code = i >= 1 ? (int)fix[Y.f_reg + c * N + i] : -1;
            const unsigned int skip = i >= 1 ? (unsigned int)T[Y.i_boxskip + c * N + i] : 0x7Fu;   // (stage 0: no state rows)
            const double* rt = code >= 0 ? D + Y.d_reg + (c * Y.P + (code >> 2)) * REGSZ : nullptr;
            const double* Hc = (!rt && i >= 1) ? region_hull(Y, D, T, fix, c, i) : nullptr;
            auto put = [&](int col, bool neg, double rh) { atomicMin(&bkey[(i * 2 + (neg ? 1 : 0)) * 16 + OC_DECODE_POLICY::col(col)], d2key(rh)); };
            if (i >= 1) {
              const double a_lo_x = rt ? rt[11] : Hc[0], a_hi_x = rt ? rt[12] : Hc[1], a_lo_y = rt ? rt[13] : Hc[2], a_hi_y = rt ? rt[14] : Hc[3];
              if (!(skip & 1u)) put(6 * c + 1, true, -G[0]);
              if (!(skip & 2u)) put(6 * c + 4, true, -G[0]);
              if (!(skip & 4u)) put(6 * c + 1, false, G[1]);
              if (!(skip & 8u)) put(6 * c + 2, false, a_hi_x);
              if (!(skip & 16u)) put(6 * c + 2, true, -a_lo_x);
              if (!(skip & 32u)) put(6 * c + 5, false, a_hi_y);
              if (!(skip & 64u)) put(6 * c + 5, true, -a_lo_y);
            }
            if (i <= N - 2) {
#pragma unroll
              for (int s_ = 0; s_ < 2; ++s_) {
                double lo, hi;
                if (i == 0) { lo = D[Y.d_u0box + c * 4 + 2 * s_]; hi = D[Y.d_u0box + c * 4 + 2 * s_ + 1]; }
                else if (rt) { lo = rt[15 + 2 * s_]; hi = rt[16 + 2 * s_]; }
                else { lo = Hc[4 + 2 * s_]; hi = Hc[5 + 2 * s_]; }
                put(6 * C + 2 * c + s_, false, hi); put(6 * C + 2 * c + s_, true, -lo);
              }
            }
          }
        }
      }
#pragma unroll 1
      for (int cl = 0; cl < 8; ++cl) {
#ifdef MIQP_PROFILE
        if (OC_DECODE_POLICY::MARKS && cl == 2) ocd_t_sparse = clock64();
#endif
        const int cnt = cls_cnt[cl], off = cls_off[cl];
        const bool percar = cl < 6;
        const int per = percar ? C * cnt : cnt, total = N * per;
        for (int e0 = 0; e0 < total; e0 += 64) {
          const int e = e0 + tid;
          int i = 0, slot = 0; bool in = e < total;
          if (in) { i = e / per; const int rem = e - i * per; slot = percar ? (rem / cnt) * Y.SC + off + rem % cnt : off + rem; }
          if (cl < 2) {   // the state / input bounds: every slot carries a row - or the lane pass above has decoded them
            if constexpr (!OC_DECODE_POLICY::LANE_BOUNDS) { if (in) take(i, slot); }
            continue;
          }
          const bool cnd = in && slot_maybe<C>(Y, fix, i, slot);
          const unsigned long long mk = __ballot(cnd);
          if (cnd) plist[nlist + __popcll(mk & lt)] = (unsigned short)(i * NSLOT + slot);
          nlist += __popcll(mk);
          if (nlist > LCAP) flush();
        }
      }
      flush();
      if (tid == 0) { int a = 0; for (int k = 0; k < nw; ++k) { pre[k] = (unsigned short)(a < 65535 ? a : 65535); a += __popcll(bmp[k]); } pre[nw] = (unsigned short)(a < 65535 ? a : 65535); }
      OC_WAVE_SYNC();
      ngen = pre[nw];
      if (ngen <= OC_GCAP)
        for (int k = tid; k < nw; k += 64) {
          unsigned long long bits = bmp[k]; int pos = pre[k];
          while (bits) { const int b = __ffsll((long long)bits) - 1; cand[pos++] = (unsigned short)(k * 64 + b); bits &= bits - 1ull; }
        }
      OC_WAVE_SYNC();
    }
#ifdef MIQP_PROFILE
    if (OC_DECODE_POLICY::MARKS) ocd_t_rows = clock64();
#endif
    // ---- pass B: the general rows, OC_SCR at a time through dense scratch rows; packed into LDS in (stage, slot) order
    bool overflow = ngen > OC_GCAP;
    int ncoef = 0;
    for (int c0 = 0; c0 < ngen && !overflow; c0 += OC_SCR) {
      double* g = scr + (tid & (OC_SCR - 1)) * OC_SSTR;
      RowOut r; r.active = false; r.rhs = 0; r.aq = 0;
      int i = 0, nn = 0;
      const bool mine = tid < OC_SCR && c0 + tid < ngen;
      int slot_ = 0;
      if (mine) { const int pcode = cand[c0 + tid]; i = pcode / NSLOT; slot_ = pcode - i * NSLOT; r = decode_row<C, true>(Y, D, T, fix, i, slot_, g); }
      unsigned long long map = 0ull; unsigned int cols = 0u;
      double v6[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) v6[k] = 0.0;
      if (mine) {
        for (int q = 0; q < NZ; ++q) {
          const double v = g[q];
          if (v != 0.0 && nn < 6) {
#pragma unroll
            for (int k = 0; k < 6; ++k) if (k == nn) v6[k] = v;
            const int pq = OC_DECODE_POLICY::col(q);
            map |= (unsigned long long)(nn + 1) << (4 * pq); cols |= (unsigned int)pq << (4 * nn); nn++;
          }
        }
      }
      const bool keep = mine && nn > 0;   // a row without coefficients constrains nothing
      // prefix sums over the lanes: row index and coefficient offset
      const unsigned long long mk = __ballot(keep);
      const unsigned long long b0 = __ballot(keep && (nn & 1)), b1 = __ballot(keep && (nn & 2)), b2 = __ballot(keep && (nn & 4));
      const int tot = __popcll(b0) + 2 * __popcll(b1) + 4 * __popcll(b2);
      if (ncoef + tot > OC_GCOEF) { overflow = true; break; }
      if (keep) {
        const int idx = sstart[N + 1] + __popcll(mk & lt);   // sstart[N + 1]: rows so far (lane-uniform value read before the update below)
        const int off = ncoef + __popcll(b0 & lt) + 2 * __popcll(b1 & lt) + 4 * __popcll(b2 & lt);
#pragma unroll
        for (int k = 0; k < 6; ++k) if (k < nn) gcoef[off + k] = v6[k];
        uint4 m4; m4.x = (unsigned int)map; m4.y = (unsigned int)(map >> 32);
        m4.z = (unsigned int)off | ((unsigned int)nn << 16) | ((unsigned int)i << 20) | (r.aq > 0.0 ? 0x80000000u : 0u); m4.w = cols;
        gmeta[idx] = m4; grhs[idx] = r.rhs;
        if constexpr (OC_DECODE_POLICY::ROW_IDENTITY) cand[idx] = (unsigned short)(i * NSLOT + slot_);   // identity of the packed row (idx <= its position in the candidate list: in-place compaction)
        else atomicAdd(&sstart[i + 1], 1);   // rows per stage, stored at stage + 1
      }
      OC_WAVE_SYNC();
      if (tid == 0) sstart[N + 1] += __popcll(mk);
      ncoef += tot;
      OC_WAVE_SYNC();
    }

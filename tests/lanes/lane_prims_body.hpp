// lane_prims_body.hpp -- TEST INFRASTRUCTURE.  One driver for every primitive of the "lanes" policy the step kernels are written against
// (lifelike_agility_and_play_amd/csrc/lanes.hpp GpuLanes and its wrappers; tests/emul/lanes_host.hpp HostLanes), shared source in the style of the
// kernel body: it is compiled once per lane policy and knows nothing of GPU or host.  What differs sits behind IO:
//   io.ld(w)      operand word w of this row as L::F.  The value goes through one multiply (by a 1.0 that comes from memory) on its way, so it is
//                 WRITTEN by an arithmetic instruction just before the call -- the primitive's own leading wait states protect its first DPP read, as in the kernel
//   io.st(w, x)   lane-varying result word w;  io.stu(w, x): an env-uniform (float) result, stored by every lane
//   io.pred(w)    operand word w > 0 as the predicate type row_ballot takes (per lane on the GPU; the host's per-env code is a row of one lane)
//   io.aux()      this row's AUX_WORDS floats of global memory (in and out);  io.auxd(): the double table of count_le16 (AUXD_WORDS, shared)
//   io.ia(k)      run-time integer argument k;  io.legc() / io.basec(): the constant tables as the kernel arguments carry them
// `targ` packs the template arguments of the primitive (S_, H_, K_, L_, I_, J_, LEG_; NEG_LO as bit 4 for turns4 / turns8).
#pragma once

#define LP_IN_WORDS 80
#define LP_OUT_WORDS 24
#define LP_AUX_WORDS 64
#define LP_AUXD_WORDS 24
// the `consts` buffer: legc [LC_COUNT][4] | candc [CAND_TABLE_WORDS][16] | basec [BC_COUNT] | 1.0f   (pmc_params.hpp, included by whoever includes this)
#define LP_CONSTS_LEGC 0
#define LP_CONSTS_CANDC (LC_COUNT * 4)
#define LP_CONSTS_BASEC (LP_CONSTS_CANDC + CAND_TABLE_WORDS * PMC_ROW)
#define LP_CONSTS_ONE (LP_CONSTS_BASEC + BC_COUNT)
#define LP_CONSTS_WORDS (LP_CONSTS_ONE + 1)

enum LanePrim {
  // moves
  LP_FROM_PREV_LEG = 0, LP_FROM_LEG2, LP_FROM_NEXT_LEG, LP_RBCAST, LP_SUBBCAST, LP_BCAST, LP_SUBBCAST6, LP_SUBBCAST6_AFTER, LP_GATHER_TRI3, LP_SPREAD3,
  LP_RMIN, LP_SUBMIN, LP_VEL_DX, LP_VEL_DQ, LP_PEER, LP_ROW_BALLOT, LP_LD16, LP_ST16, LP_ST16_ROT, LP_COPY16, LP_COUNT_LE16, LP_PARK_ROW, LP_CONE_LDS,
  LP_STAGE_ROW, LP_LEGC, LP_CANDC, LP_BASEC, LP_CANDC_OF, LP_SETTLE, LP_LANE_IDS, LP_PICK, LP_LDL_STL, LP_LDL2,
  // sums
  LP_QSUM = 40, LP_SUBSUM, LP_RSUM6, LP_QSUM6, LP_SUBSUM3, LP_SUFSUM4, LP_SUFSUM6,
  // multiply-adds
  LP_FMAC_RBCAST = 50, LP_FMAC_RBCAST_SETTLED, LP_GRAM4, LP_GRAM16, LP_GRAM_PIPE, LP_TURNS4, LP_TURNS8, LP_CONE_TURNS4, LP_VEL_DOT, LP_VEL_COMMIT, LP_VEL_COMMIT2,
  LP_TURNS16      // four turns4 blocks S_ = 0 .. 3 back to back: all sixteen turn masks in one call
};

// what the run-time integer arguments of a primitive may be: nothing a test passes may index past the buffers it handed over (both ABIs refuse the call otherwise)
static inline bool lp_args_in_bounds(int prim, const int* ia) {
  const auto in = [](int v, int lo, int hi) { return v >= lo && v <= hi; };
  switch (prim) {
    case LP_LD16: case LP_ST16: return in(ia[1], 1, LP_AUX_WORDS) && in(ia[0], 0, LP_AUX_WORDS);
    case LP_ST16_ROT: return in(ia[1], 1, LP_AUX_WORDS) && in(ia[0], 0, LP_AUX_WORDS) && in(ia[2], 0, ia[1]);
    case LP_COPY16: return in(ia[1], 1, LP_AUX_WORDS / 2) && in(ia[0], 0, LP_AUX_WORDS);
    case LP_COUNT_LE16: return in(ia[0], 0, LP_AUXD_WORDS - 1);
    case LP_PARK_ROW: return in(ia[0], 0, PMC_ROW_SCRATCH - 4);
    case LP_STAGE_ROW: return in(ia[0], 4, LP_AUX_WORDS) && ia[0] % 4 == 0;
    case LP_LEGC: return in(ia[0], 0, LC_COUNT - 1);
    case LP_CANDC: return in(ia[0], 0, CAND_TABLE_WORDS - 1);
    case LP_BASEC: return in(ia[0], 0, BC_COUNT - 1);
    case LP_CANDC_OF: return in(ia[0], 0, 3) && in(ia[1], 0, CAND_TABLE_WORDS - 1);
    case LP_LDL_STL: return in(ia[0], 0, 7) && in(ia[1], 0, 8);      // base + 3 * stride < LP_AUX_WORDS / 2
    case LP_LDL2: return in(ia[0], 0, 7) && in(ia[1], 1, 8) && in(ia[2], 0, 5) && in(ia[3], 0, 6);      // base + 3 * stride < LP_AUX_WORDS / 2 and < LP_AUXD_WORDS
    default: return true;
  }
}

#define LP_SW4(T, CALL)  switch (T) { case 0: { constexpr int T_ = 0; CALL; } break; case 1: { constexpr int T_ = 1; CALL; } break; \
                                      case 2: { constexpr int T_ = 2; CALL; } break; default: { constexpr int T_ = 3; CALL; } break; }
#define LP_SW2(T, CALL)  switch (T) { case 0: { constexpr int T_ = 0; CALL; } break; default: { constexpr int T_ = 1; CALL; } break; }
#define LP_SW6(T, CALL)  switch (T) { case 0: { constexpr int T_ = 0; CALL; } break; case 1: { constexpr int T_ = 1; CALL; } break; case 2: { constexpr int T_ = 2; CALL; } break; \
                                      case 3: { constexpr int T_ = 3; CALL; } break; case 4: { constexpr int T_ = 4; CALL; } break; default: { constexpr int T_ = 5; CALL; } break; }
#define LP_SW16(T, CALL) switch (T) { case 0: { constexpr int T_ = 0; CALL; } break; case 1: { constexpr int T_ = 1; CALL; } break; case 2: { constexpr int T_ = 2; CALL; } break; \
    case 3: { constexpr int T_ = 3; CALL; } break; case 4: { constexpr int T_ = 4; CALL; } break; case 5: { constexpr int T_ = 5; CALL; } break; case 6: { constexpr int T_ = 6; CALL; } break; \
    case 7: { constexpr int T_ = 7; CALL; } break; case 8: { constexpr int T_ = 8; CALL; } break; case 9: { constexpr int T_ = 9; CALL; } break; case 10: { constexpr int T_ = 10; CALL; } break; \
    case 11: { constexpr int T_ = 11; CALL; } break; case 12: { constexpr int T_ = 12; CALL; } break; case 13: { constexpr int T_ = 13; CALL; } break; \
    case 14: { constexpr int T_ = 14; CALL; } break; default: { constexpr int T_ = 15; CALL; } break; }

template <class L, class IO>
LL_D void run_prim(L& lanes, IO& io, int prim, int targ) {
  typedef typename L::F F;
  typedef typename L::F2 F2;
  typedef typename L::I I;
  switch (prim) {
    // ---- moves ---------------------------------------------------------------------------------------------------------------------------
    case LP_FROM_PREV_LEG: { F x = io.ld(0); io.st(0, L::from_prev_leg(x)); } break;
    case LP_FROM_LEG2: { F x = io.ld(0); io.st(0, L::from_leg2(x)); } break;
    case LP_FROM_NEXT_LEG: { F x = io.ld(0); io.st(0, L::from_next_leg(x)); } break;
    case LP_RBCAST: { F x = io.ld(0); LP_SW16(targ, io.stu(0, L::template rbcast<T_>(x))); } break;
    case LP_SUBBCAST: { F x = io.ld(0); LP_SW4(targ, io.st(0, L::template subbcast<T_>(x))); } break;
    case LP_BCAST: { F x = io.ld(0); LP_SW4(targ, io.stu(0, L::template bcast<T_>(x))); } break;
    case LP_SUBBCAST6: {
      F x[6], o[6];
      for (int i = 0; i < 6; i++) x[i] = io.ld(i);
      LP_SW4(targ, L::template subbcast6<T_>(x, o));
      for (int i = 0; i < 6; i++) io.st(i, o[i]);
    } break;
    case LP_SUBBCAST6_AFTER: {      // as the kernel uses it: directly behind a subbcast6 of the same x
      F x[6], o1[6], o2[6];
      for (int i = 0; i < 6; i++) x[i] = io.ld(i);
      L::template subbcast6<0>(x, o1);
      LP_SW4(targ, L::template subbcast6_after<T_>(x, o2, o1[0]));
      for (int i = 0; i < 6; i++) { io.st(i, o2[i]); io.st(6 + i, o1[i]); }
    } break;
    case LP_GATHER_TRI3: {
      F d[3], m[6];
      for (int i = 0; i < 3; i++) d[i] = io.ld(i);
      L::gather_tri3(d, m);
      for (int i = 0; i < 6; i++) io.st(i, m[i]);
    } break;
    case LP_SPREAD3: { F x = io.ld(0), o[3]; L::spread3(x, o); for (int i = 0; i < 3; i++) io.st(i, o[i]); } break;
    case LP_RMIN: { F x = io.ld(0); io.stu(0, L::rmin(x)); } break;
    case LP_SUBMIN: { F x = io.ld(0); io.st(0, L::submin(x)); } break;
    case LP_VEL_DX: { F a = io.ld(0), b = io.ld(1); LP_SW6(targ, io.stu(0, L::template vel_dx<T_>(a, b))); } break;
    case LP_VEL_DQ: { F j = io.ld(0); LP_SW4(targ, io.st(0, L::template vel_dq<T_>(j))); } break;
    case LP_PEER: { F x = io.ld(0); io.st(0, lanes.peer(x)); } break;
    case LP_ROW_BALLOT: io.stu(0, (float)lanes.row_ballot(io.pred(0))); break;
    case LP_LD16: io.st(0, lanes.ld16(io.aux(), io.ia(0), io.ia(1))); break;
    case LP_ST16: { F v = io.ld(0); lanes.st16(io.aux(), io.ia(0), io.ia(1), v); } break;
    case LP_ST16_ROT: { F v = io.ld(0); lanes.st16_rot(io.aux(), io.ia(0), io.ia(1), io.ia(2), v); } break;
    case LP_COPY16: lanes.copy16(io.aux() + LP_AUX_WORDS / 2, io.aux(), io.ia(0), io.ia(1)); break;
    case LP_COUNT_LE16: io.stu(0, (float)lanes.count_le16(io.auxd(), io.ia(0), io.auxd()[LP_AUXD_WORDS - 1])); break;
    case LP_PARK_ROW: {             // four row-uniform floats through the row scratch and back
      F x[4];
      float v[4], w[4];
      for (int i = 0; i < 4; i++) x[i] = io.ld(i);
      for (int i = 0; i < 4; i++) { v[i] = L::template rbcast<0>(x[i]); w[i] = 0.0f; }
      lanes.park_row(v, 4, io.ia(0));
      lanes.unpark_row(w, 4, io.ia(0));
      for (int i = 0; i < 4; i++) io.stu(i, w[i]);
    } break;
    case LP_CONE_LDS: {             // all eight (kind, S) records stored, the two of turn block `targ` read back: a slip in the record layout reads another block's words
      for (int k = 0; k < 2; k++)
        for (int s = 0; s < 4; s++) lanes.cone_store(k, s, io.ld((k * 4 + s) * 4), io.ld((k * 4 + s) * 4 + 1), io.ld((k * 4 + s) * 4 + 2), io.ld((k * 4 + s) * 4 + 3));
      lanes.row_sync();
      for (int k = 0; k < 2; k++) {
        F a, b, c, d;
        lanes.cone_load(k, targ, a, b, c, d);
        io.st(k * 4, a); io.st(k * 4 + 1, b); io.st(k * 4 + 2, c); io.st(k * 4 + 3, d);
      }
    } break;
    case LP_STAGE_ROW: {
      const float* p = lanes.stage_row(io.aux(), io.ia(0));
      for (int c = 0; c * 16 < io.ia(0); c++) io.st(c, lanes.ld16(p, c * 16, io.ia(0)));
    } break;
    // (the table index is a constant at every call of the kernel body, and the pinned policies hold the tables in registers: one call per index, the asked one kept)
    case LP_LEGC: {
      F r = lanes.lane_f(0.0f);
      LL_UNROLL
      for (int f = 0; f < LC_COUNT; f++) if (f == io.ia(0)) r = lanes.legc(io.legc(), f);
      io.st(0, r);
    } break;
    case LP_CANDC: {
      F r = lanes.lane_f(0.0f);
      LL_UNROLL
      for (int w = 0; w < CAND_TABLE_WORDS; w++) if (w == io.ia(0)) r = lanes.candc(w);
      io.st(0, r);
    } break;
    case LP_BASEC: {
      float r = 0.0f;
      LL_UNROLL
      for (int i = 0; i < BC_COUNT; i++) if (i == io.ia(0)) r = lanes.basec(io.basec(), i);
      io.stu(0, r);
    } break;
    case LP_CANDC_OF: io.st(0, lanes.candc_of(I(io.ia(0)), I(io.ia(1)))); break;
    case LP_SETTLE: { F x = io.ld(0); io.st(0, L::from_prev_leg(L::settle(x))); } break;
    case LP_LANE_IDS: {
      io.st(0, L::i2f(lanes.leg())); io.st(1, L::i2f(lanes.sub())); io.st(2, lanes.legf());
      io.st(3, lm::sel(lanes.is_leg(targ & 3), lanes.lane_f(1.0f), lanes.lane_f(0.0f)));
      io.st(4, lm::sel(lanes.is_sub(targ & 3), lanes.lane_f(1.0f), lanes.lane_f(0.0f)));
      io.st(5, lm::sel(lanes.is_lane(targ), lanes.lane_f(1.0f), lanes.lane_f(0.0f)));
    } break;
    case LP_PICK: {
      io.st(0, lanes.pick3(1.0f, 2.0f, 3.0f));
      io.st(1, L::i2f(lanes.pick4i(4, 5, 6, 7)));
      io.st(2, L::d2f(lanes.pick4d(8.0, 9.0, 10.0, 11.0)));
      io.st(3, L::i2f(L::f2i(io.ld(0))));
    } break;
    case LP_LDL_STL: {              // per-leg strided access: element base + stride * leg; stores from sub-lane 0 only
      F v = lanes.ldl(io.aux(), io.ia(0), io.ia(1));
      io.st(0, v);
      lanes.stl(io.aux() + LP_AUX_WORDS / 2, io.ia(0), io.ia(1), io.ld(0));
    } break;
    case LP_LDL2: {                 // stl under a lane predicate (a leg for targ 0 .. 3, a sub-lane for 4 .. 7: only sub-lane 0 ever stores), the double loads
      F v = io.ld(0), fi = io.ld(1);
      I idx = L::f2i(fi);           // (whole numbers 0 .. LP_AUXD_WORDS - 1 per lane: the caller's, checked where the case is made)
      if (targ < 4) lanes.stl_if(lanes.is_leg(targ & 3), io.aux(), io.ia(0), io.ia(1), v);
      else lanes.stl_if(lanes.is_sub(targ & 3), io.aux(), io.ia(0), io.ia(1), v);
      io.st(0, L::d2f(lanes.lddl(io.auxd(), io.ia(2), io.ia(3))));
      io.st(1, L::d2f(lanes.ldd_idx(io.auxd(), idx)));
    } break;
    // ---- sums ----------------------------------------------------------------------------------------------------------------------------
    case LP_QSUM: { F x = io.ld(0); io.stu(0, L::qsum(x)); } break;
    case LP_SUBSUM: { F x = io.ld(0); io.st(0, L::subsum(x)); } break;
    case LP_RSUM6: case LP_QSUM6: {
      F x[6];
      float o[6];
      for (int i = 0; i < 6; i++) x[i] = io.ld(i);
      if (prim == LP_RSUM6) L::rsum6(x, o); else L::qsum6(x, o);
      for (int i = 0; i < 6; i++) io.stu(i, o[i]);
    } break;
    case LP_SUBSUM3: {
      F x[3], o[3];
      for (int i = 0; i < 3; i++) x[i] = io.ld(i);
      L::subsum3(x, o);
      for (int i = 0; i < 3; i++) io.st(i, o[i]);
    } break;
    case LP_SUFSUM4: case LP_SUFSUM6: {
      F x[6];
      const int n = prim == LP_SUFSUM4 ? 4 : 6;
      for (int i = 0; i < 6; i++) x[i] = io.ld(i);
      if (prim == LP_SUFSUM4) L::sufsum4(x); else L::sufsum6(x);
      for (int i = 0; i < n; i++) io.st(i, x[i]);
    } break;
    // ---- multiply-adds -------------------------------------------------------------------------------------------------------------------
    case LP_FMAC_RBCAST: { F acc = io.ld(0), x = io.ld(1), k = io.ld(2); LP_SW16(targ, L::template fmac_rbcast<T_>(acc, x, k)); io.st(0, acc); } break;
    case LP_FMAC_RBCAST_SETTLED: {   // x has settled (lanes.hpp settle) when the DPP read comes
      F acc = io.ld(0), x = L::settle(io.ld(1)), k = io.ld(2);
      LP_SW16(targ, L::template fmac_rbcast_settled<T_>(acc, x, k));
      io.st(0, acc);
    } break;
    case LP_GRAM4: {                 // as the kernel chains it: blocks 0 .. targ back to back (blocks S_ > 0 have no wait states of their own)
      F x[6], y[6], g[16];
      for (int i = 0; i < 6; i++) { x[i] = io.ld(i); y[i] = io.ld(6 + i); }
      for (int i = 0; i < 16; i++) g[i] = io.ld(12 + i);
      L::template gram4<0>(x, y, g);
      if (targ >= 1) L::template gram4<1>(x, y, g);
      if (targ >= 2) L::template gram4<2>(x, y, g);
      if (targ >= 3) L::template gram4<3>(x, y, g);
      for (int i = 0; i < 16; i++) io.st(i, g[i]);
    } break;
    case LP_GRAM16: {
      F x[6], y[6], g[16];
      for (int i = 0; i < 6; i++) { x[i] = io.ld(i); y[i] = io.ld(6 + i); }
      L::gram16(x, y, g);
      for (int i = 0; i < 16; i++) io.st(i, g[i]);
    } break;
    case LP_GRAM_PIPE: {
      F x[6], y[6], g[16];
      for (int i = 0; i < 6; i++) { x[i] = io.ld(i); y[i] = io.ld(6 + i); }
      typename L::GramAcc a;
      L::template gram_mfma<0>(a, x[0], y[0]); L::template gram_mfma<1>(a, x[1], y[1]); L::template gram_mfma<2>(a, x[2], y[2]);
      L::template gram_mfma<3>(a, x[3], y[3]); L::template gram_mfma<4>(a, x[4], y[4]); L::template gram_mfma<5>(a, x[5], y[5]);
      L::gram_collect(a, g);
      for (int i = 0; i < 16; i++) io.st(i, g[i]);
    } break;
    case LP_TURNS4: {
      lanes.prepare_turn_masks();
      F u = io.ld(0), dl = io.ld(1), lo = io.ld(2), hi = io.ld(3), k0 = io.ld(4), k1 = io.ld(5), k2 = io.ld(6), k3 = io.ld(7);
      if (targ & 16) { LP_SW4(targ & 3, (lanes.template turns4<T_, true>(u, dl, lo, hi, k0, k1, k2, k3))); }
      else { LP_SW4(targ & 3, (lanes.template turns4<T_, false>(u, dl, lo, hi, k0, k1, k2, k3))); }
      io.st(0, u); io.st(1, dl);
    } break;
    case LP_TURNS16: {
      lanes.prepare_turn_masks();
      F u = io.ld(0), dl = io.ld(1), lo = io.ld(2), hi = io.ld(3), nk[16];
      for (int i = 0; i < 16; i++) nk[i] = io.ld(4 + i);
      lanes.template turns4<0>(u, dl, lo, hi, nk[0], nk[4], nk[8], nk[12]);
      lanes.template turns4<1>(u, dl, lo, hi, nk[1], nk[5], nk[9], nk[13]);
      lanes.template turns4<2>(u, dl, lo, hi, nk[2], nk[6], nk[10], nk[14]);
      lanes.template turns4<3>(u, dl, lo, hi, nk[3], nk[7], nk[11], nk[15]);
      io.st(0, u); io.st(1, dl);
    } break;
    case LP_TURNS8: {
      lanes.prepare_turn_masks();
      F u = io.ld(0), dl = io.ld(1), lo = io.ld(2), hi = io.ld(3), nk[16];
      for (int i = 0; i < 16; i++) nk[i] = io.ld(4 + i);
      if (targ & 16) { LP_SW2(targ & 1, (lanes.template turns8<T_, true>(u, dl, lo, hi, nk))); }
      else { LP_SW2(targ & 1, (lanes.template turns8<T_, false>(u, dl, lo, hi, nk))); }
      io.st(0, u); io.st(1, dl);
    } break;
    case LP_CONE_TURNS4: {
      lanes.prepare_turn_masks();
      F S1 = io.ld(0), S2 = io.ld(1), d1 = io.ld(2), d2 = io.ld(3), lam1 = io.ld(4), lam2 = io.ld(5), lim = io.ld(6), k11[16], k12[16], k21[16], k22[16];
      for (int i = 0; i < 16; i++) { k11[i] = io.ld(8 + i); k12[i] = io.ld(24 + i); k21[i] = io.ld(40 + i); k22[i] = io.ld(56 + i); }
      LP_SW4(targ, lanes.template cone_turns4<T_>(S1, S2, d1, d2, lam1, lam2, lim, k11, k12, k21, k22));
      io.st(0, S1); io.st(1, S2); io.st(2, d1); io.st(3, d2);
    } break;
    case LP_VEL_DOT: {
      F c = io.ld(0), VA = io.ld(11), VB = io.ld(12), VJ = io.ld(13);
      F2 a01 = L::pair(io.ld(1), io.ld(2)), a23 = L::pair(io.ld(3), io.ld(4)), b01 = L::pair(io.ld(5), io.ld(6)), j01 = L::pair(io.ld(7), io.ld(8)), j23 = L::pair(io.ld(9), io.ld(10));
      io.st(0, L::vel_dot(c, a01, a23, b01, j01, j23, VA, VB, VJ));
    } break;
    case LP_VEL_COMMIT: {
      F dl = io.ld(0), VA = io.ld(11), VB = io.ld(12), VJ = io.ld(13), lam = io.ld(14);
      F2 a01 = L::pair(io.ld(1), io.ld(2)), a23 = L::pair(io.ld(3), io.ld(4)), b01 = L::pair(io.ld(5), io.ld(6)), j01 = L::pair(io.ld(7), io.ld(8)), j23 = L::pair(io.ld(9), io.ld(10));
      L::vel_commit(dl, lam, a01, a23, b01, j01, j23, VA, VB, VJ);
      io.st(0, VA); io.st(1, VB); io.st(2, VJ); io.st(3, lam);
    } break;
    case LP_VEL_COMMIT2: {
      F dl1 = io.ld(0), VA = io.ld(11), VB = io.ld(12), VJ = io.ld(13), lam1 = io.ld(14), dl2 = io.ld(16), lam2 = io.ld(15);
      F2 a01 = L::pair(io.ld(1), io.ld(2)), a23 = L::pair(io.ld(3), io.ld(4)), b01 = L::pair(io.ld(5), io.ld(6)), j01 = L::pair(io.ld(7), io.ld(8)), j23 = L::pair(io.ld(9), io.ld(10));
      F2 c01 = L::pair(io.ld(17), io.ld(18)), c23 = L::pair(io.ld(19), io.ld(20)), e01 = L::pair(io.ld(21), io.ld(22)), k01 = L::pair(io.ld(23), io.ld(24)), k23 = L::pair(io.ld(25), io.ld(26));
      L::vel_commit2(dl1, lam1, a01, a23, b01, j01, j23, dl2, lam2, c01, c23, e01, k01, k23, VA, VB, VJ);
      io.st(0, VA); io.st(1, VB); io.st(2, VJ); io.st(3, lam1); io.st(4, lam2);
    } break;
    default: break;
  }
}

// solver_rows_body.hpp -- TEST INFRASTRUCTURE.  One driver for the members of Pmc<L> (lifelike_agility_and_play_amd/csrc/pmc_step.hpp) that turn whitened coefficients
// into constraint rows and sweep them: permute4, finish_row, cross_gram, gs_round, gs_cone_round, the contact builders (contact_row, and contact_rows_cone_piped with
// the pieces it is made of), their composition, and the small members around them (pd_target, pd_torque, clip_velocities, pick_rank).  In the style of lane_prims_body.hpp and math_helpers_body.hpp: shared source, compiled once per lane policy, ONE entry per launch.
// A sample is one environment ROW of 16 lanes (lane = 4 * leg + sub); what differs between GPU and host sits behind IO:
//   io.ld(w) / io.st(w, x)   operand / result word w of this row as L::F (the operand passes one multiply by a 1.0 from memory, so nothing folds)
//   io.ldu(w)                an env-uniform float (lane 0 of the row on the host, the lane's own copy on the GPU: the tests replicate it)
// A Row travels as SR_ROW_WORDS words, the F2 members written out as their two halves:
//   ca[0..3] | cb[0..1] | cj[0..3] | c | inv | lam | nk[0..15]
#pragma once

#define SR_IN_WORDS 96
#define SR_OUT_WORDS 120
#define SR_MAX_BLOCKS 64       // one-wave workgroups per launch: 64 x 4 = 256 rows
#define SR_ROW_WORDS 29
#define SR_ROW_C 10
#define SR_ROW_INV 11
#define SR_ROW_LAM 12
#define SR_ROW_NK 13
// the `consts` buffer is the one of lane_prims_body.hpp: legc [LC_COUNT][4] | candc [CAND_TABLE_WORDS][16] | basec [BC_COUNT] | 1.0f  (no entry reads the tables; the lane
// policies stage them as in the step kernels)
#define SR_CONSTS_LEGC 0
#define SR_CONSTS_CANDC (LC_COUNT * 4)
#define SR_CONSTS_BASEC (SR_CONSTS_CANDC + CAND_TABLE_WORDS * PMC_ROW)
#define SR_CONSTS_ONE (SR_CONSTS_BASEC + BC_COUNT)
#define SR_CONSTS_WORDS (SR_CONSTS_ONE + 1)

enum SolverRowsEntry {
  SR_PERMUTE4 = 0,
  SR_FINISH_ROW,        // targ = LIMIT
  SR_CROSS_GRAM,
  SR_GS_ROUND,          // targ 0: <LIMIT, UNILATERAL> = <true, true>, 1: <false, true>, 2: <false, false> -- the three the kernel uses
  SR_GS_CONE_ROUND,
  SR_CONTACT_ROWS,      // targ 0: contact_row x 3 + cross_gram x 2; 1: contact_rows_cone_piped (lane policies with kGramPipe only)
  SR_COMPOSE,           // the kernel's own order from the contact geometry to the velocity change: the rows (piped where the policy has the pipe), one normal round,
                        // then targ 0: one cone round, 1: the two pyramid rounds; then the way back (bwd6, lm_bwd)
  SR_PD,                // pd_target, then pd_torque with its max_tau argument (0: the default, StepParams::max_tau)
  SR_CLIP_VELOCITIES,
  SR_PICK_RANK,         // targ = K
  SR_SELF,              // targ 0: self_row_build, self_row_velocity, self_turn; 1: ... self_fric_turn; 2: the pieces alone: self_row_pack, self_row_velocity, self_row_apply, self_row_clear
  SR_PAIR,              // targ 0: pair_row_build (normal row) + pair_turn; 1: pair_row_build (tangential) + pair_fric_turn.  Both rows of an arena must be live (peer_u)
  SR_CAND_EVAL_POINT,
  SR_ENTRY_END
};

static inline int sr_max_targ(int entry) { return entry == SR_PICK_RANK ? 3 : (entry == SR_GS_ROUND || entry == SR_SELF) ? 2 : (entry == SR_PAIR || entry == SR_FINISH_ROW || entry == SR_CONTACT_ROWS || entry == SR_COMPOSE) ? 1 : 0; }

// what a launch may be asked: a known entry, a template argument it is instantiated for (the piped contact rows only where the lane policy has the pipe), a block count
// the caller's buffers (given in floats) hold.  Nothing a test passes may index past the buffers it handed over (both ABIs refuse the call otherwise).
static inline bool sr_args_in_bounds(int entry, int targ, bool policy_has_pipe, int n_blocks, long in_floats, long out_floats, long consts_floats) {
  if (entry < 0 || entry >= SR_ENTRY_END) return false;
  if (targ < 0 || targ > sr_max_targ(entry)) return false;
  if (entry == SR_CONTACT_ROWS && targ == 1 && !policy_has_pipe) return false;
  if (n_blocks < 1 || n_blocks > SR_MAX_BLOCKS) return false;
  return in_floats >= (long)n_blocks * 4 * SR_IN_WORDS * 16 && out_floats >= (long)n_blocks * 4 * SR_OUT_WORDS * 16 && consts_floats >= SR_CONSTS_WORDS;
}

template <class L, class IO>
LL_D void run_solver_rows(L& ln, IO& io, int entry, int targ) {
  typedef Pmc<L> K;
  typedef typename L::F F;
  typedef typename L::B B;
  typedef typename K::Row Row;
  const auto v3 = [&](int w) { return mk3<F>(io.ld(w), io.ld(w + 1), io.ld(w + 2)); };
  const auto ld_row = [&](int w, Row& r) {
    r.ca01 = L::pair(io.ld(w), io.ld(w + 1)); r.ca23 = L::pair(io.ld(w + 2), io.ld(w + 3)); r.cb01 = L::pair(io.ld(w + 4), io.ld(w + 5));
    r.cj01 = L::pair(io.ld(w + 6), io.ld(w + 7)); r.cj23 = L::pair(io.ld(w + 8), io.ld(w + 9));
    r.c = io.ld(w + SR_ROW_C); r.inv = io.ld(w + SR_ROW_INV); r.lam = io.ld(w + SR_ROW_LAM);
    for (int i = 0; i < 16; i++) r.nk[i] = io.ld(w + SR_ROW_NK + i);
  };
  // what finish_row leaves: the permuted coefficients, lam and the Gram scalars -- under LIMIT those of lanes 3, 7, 11, 15 are not formed and not stored
  const auto st_finished = [&](int w, const Row& r, bool limit) {
    io.st(w, r.ca01.x); io.st(w + 1, r.ca01.y); io.st(w + 2, r.ca23.x); io.st(w + 3, r.ca23.y); io.st(w + 4, r.cb01.x); io.st(w + 5, r.cb01.y);
    io.st(w + 6, r.cj01.x); io.st(w + 7, r.cj01.y); io.st(w + 8, r.cj23.x); io.st(w + 9, r.cj23.y);
    io.st(w + SR_ROW_LAM, r.lam);
    for (int i = 0; i < 16; i++)
      if (!(limit && (i & 3) == 3)) io.st(w + SR_ROW_NK + i, r.nk[i]);
  };
  const auto st_built = [&](int w, const Row& r) { st_finished(w, r, false); io.st(w + SR_ROW_C, r.c); io.st(w + SR_ROW_INV, r.inv); };
  switch (entry) {
    case SR_PERMUTE4: {
      F c[4];
      K::permute4(ln, io.ld(0), io.ld(1), io.ld(2), io.ld(3), c);
      for (int k = 0; k < 4; k++) io.st(k, c[k]);
    } break;
    case SR_FINISH_ROW: {
      F gt[6], jt[3];
      for (int i = 0; i < 6; i++) gt[i] = io.ld(i);
      for (int i = 0; i < 3; i++) jt[i] = io.ld(6 + i);
      Row r;
      r.inv = io.ld(9);
      if (targ) K::template finish_row<true>(ln, r, gt, jt);
      else K::template finish_row<false>(ln, r, gt, jt);
      st_finished(0, r, targ != 0);
    } break;
    case SR_CROSS_GRAM: {
      F gm[6], jm[3], go[6], jo[3], out[16];
      for (int i = 0; i < 6; i++) { gm[i] = io.ld(i); go[i] = io.ld(10 + i); }
      for (int i = 0; i < 3; i++) { jm[i] = io.ld(6 + i); jo[i] = io.ld(16 + i); }
      K::cross_gram(ln, io.ld(9), gm, jm, go, jo, out);
      for (int i = 0; i < 16; i++) io.st(i, out[i]);
    } break;
    case SR_GS_ROUND: {
      ln.prepare_turn_masks();             // as substep_impl does once in front of its rounds
      Row r;
      ld_row(0, r);
      F hi = io.ld(29), VA = io.ld(30), VB = io.ld(31), VJ = io.ld(32);
      if (targ == 0) K::template gs_round<true, true>(ln, r, hi, VA, VB, VJ);
      else if (targ == 1) K::template gs_round<false, true>(ln, r, hi, VA, VB, VJ);
      else K::template gs_round<false, false>(ln, r, hi, VA, VB, VJ);
      io.st(0, r.lam); io.st(1, VA); io.st(2, VB); io.st(3, VJ);
    } break;
    case SR_GS_CONE_ROUND: {
      ln.prepare_turn_masks();
      Row r1, r2;
      ld_row(0, r1);
      ld_row(SR_ROW_WORDS, r2);
      typename K::ConeX cx;
      for (int i = 0; i < 16; i++) { cx.n12[i] = io.ld(58 + i); cx.n21[i] = io.ld(74 + i); }
      F lim = io.ld(90), VA = io.ld(91), VB = io.ld(92), VJ = io.ld(93);
      if (L::kConeInLds)                   // as substep_impl: the cross scalars wait in the row's LDS scratch, the round reads them block by block
        for (int S = 0; S < 4; S++) {
          ln.cone_store(0, S, cx.n12[S], cx.n12[4 + S], cx.n12[8 + S], cx.n12[12 + S]);
          ln.cone_store(1, S, cx.n21[S], cx.n21[4 + S], cx.n21[8 + S], cx.n21[12 + S]);
        }
      K::gs_cone_round(ln, r1, r2, cx, lim, VA, VB, VJ);
      io.st(0, r1.lam); io.st(1, r2.lam); io.st(2, VA); io.st(3, VB); io.st(4, VJ);
    } break;
    case SR_CONTACT_ROWS: case SR_COMPOSE: {
      const V3<F> un = v3(0), ut1 = v3(3), ut2 = v3(6), Pb = v3(9), d1 = v3(12), d2 = v3(15), d3 = v3(18);
      typename K::LegFactor lf;
      lf.l11 = io.ld(21); lf.l21 = io.ld(22); lf.l31 = io.ld(23); lf.l22 = io.ld(24); lf.l32 = io.ld(25); lf.l33 = io.ld(26); lf.i11 = io.ld(27); lf.i22 = io.ld(28); lf.i33 = io.ld(29);
      lf.y1.a = v3(30); lf.y1.l = v3(33); lf.y2.a = v3(36); lf.y2.l = v3(39); lf.y3.a = v3(42); lf.y3.l = v3(45);
      F qs[3] = {io.ld(48), io.ld(49), io.ld(50)};
      const F bias = io.ld(51), zero = ln.lane_f(0.0f);
      const B cvalid = io.ld(52) > 0.5f;
      float Sb[21], Sd[6], xi[6];
      for (int i = 0; i < 21; i++) Sb[i] = io.ldu(53 + i);
      for (int i = 0; i < 6; i++) { Sd[i] = io.ldu(74 + i); xi[i] = io.ldu(80 + i); }
      Row rn, r1, r2;
      typename K::ConeX cx;
      const bool compose = entry == SR_COMPOSE, cone = !(compose && targ == 1);
      bool piped = false;
      if constexpr (L::kGramPipe) piped = compose ? (cone && !L::kConeInLds) : targ == 1;      // (substep_impl: CONE && kGramPipe && !kConeInLds)
      else if (!compose && targ == 1) break;
      if (compose) ln.prepare_turn_masks();      // as substep_impl does once in front of its rounds
      if (piped) {
        if constexpr (L::kGramPipe) K::contact_rows_cone_piped(ln, rn, r1, r2, cx, un, ut1, ut2, Pb, d1, d2, d3, lf, Sb, Sd, xi, qs, bias, cvalid);
      } else {                             // the kernel's own order where the policy has no pipe
        K::contact_row(ln, rn, un, Pb, d1, d2, d3, lf, Sb, Sd, xi, qs, bias, cvalid);
        if (cone) {
          F g1[6], j1[3], g2[6], j2[3];
          K::contact_row(ln, r1, ut1, Pb, d1, d2, d3, lf, Sb, Sd, xi, qs, zero, cvalid, g1, j1);
          K::contact_row(ln, r2, ut2, Pb, d1, d2, d3, lf, Sb, Sd, xi, qs, zero, cvalid, g2, j2);
          K::cross_gram(ln, r1.inv, g1, j1, g2, j2, cx.n12);
          K::cross_gram(ln, r2.inv, g2, j2, g1, j1, cx.n21);
          if (compose && L::kConeInLds)
            for (int S = 0; S < 4; S++) {
              ln.cone_store(0, S, cx.n12[S], cx.n12[4 + S], cx.n12[8 + S], cx.n12[12 + S]);
              ln.cone_store(1, S, cx.n21[S], cx.n21[4 + S], cx.n21[8 + S], cx.n21[12 + S]);
            }
        } else {
          K::contact_row(ln, r1, ut1, Pb, d1, d2, d3, lf, Sb, Sd, xi, qs, zero, cvalid);
          K::contact_row(ln, r2, ut2, Pb, d1, d2, d3, lf, Sb, Sd, xi, qs, zero, cvalid);
        }
      }
      if (!compose) {
        st_built(0, rn); st_built(SR_ROW_WORDS, r1); st_built(2 * SR_ROW_WORDS, r2);
        for (int i = 0; i < 16; i++) { io.st(87 + i, cx.n12[i]); io.st(103 + i, cx.n21[i]); }
        break;
      }
      // one iteration of substep_impl's loop from rest, then its way back to velocities: d(xi) = Lb^-T dx ; d(qd) = Lm^-T (dq - Y^T d(xi))
      F VA = zero, VB = zero, VJ = zero;
      const F big = ln.lane_f(3.0e38f), mu = io.ld(86);
      K::template gs_round<false, true>(ln, rn, big, VA, VB, VJ);
      F hi = mu * rn.lam;
      if (cone) {
        K::gs_cone_round(ln, r1, r2, cx, hi, VA, VB, VJ);
      } else {
        K::template gs_round<false, false>(ln, r1, hi, VA, VB, VJ);
        K::template gs_round<false, false>(ln, r2, hi, VA, VB, VJ);
      }
      float dx[6] = {L::template vel_dx<0>(VA, VB), L::template vel_dx<1>(VA, VB), L::template vel_dx<2>(VA, VB),
                     L::template vel_dx<3>(VA, VB), L::template vel_dx<4>(VA, VB), L::template vel_dx<5>(VA, VB)};
      F dq[3] = {L::template vel_dq<0>(VJ), L::template vel_dq<1>(VJ), L::template vel_dq<2>(VJ)};
      K::template bwd6<float>(Sb, Sd, dx);
      SV<float> dxi;
      dxi.a = mk3<float>(dx[0], dx[1], dx[2]); dxi.l = mk3<float>(dx[3], dx[4], dx[5]);
      F du[3];
      du[0] = dq[0] - dot(lf.y1, dxi); du[1] = dq[1] - dot(lf.y2, dxi); du[2] = dq[2] - dot(lf.y3, dxi);
      K::lm_bwd(lf, du);
      io.st(0, rn.lam); io.st(1, r1.lam); io.st(2, r2.lam);
      for (int i = 0; i < 6; i++) io.st(3 + i, ln.lane_f(dx[i]));
      for (int j = 0; j < 3; j++) io.st(9 + j, du[j]);
    } break;
    case SR_PD: {
      F q[3] = {io.ld(0), io.ld(1), io.ld(2)}, act[3] = {io.ld(3), io.ld(4), io.ld(5)}, qd[3] = {io.ld(6), io.ld(7), io.ld(8)}, tgt[3], tau[3];
      StepParams P{};
      P.kp = io.ldu(9); P.kd = io.ldu(10); P.max_tau = io.ldu(11);
      K::pd_target(ln, q, act, tgt);
      K::pd_torque(ln, P, q, qd, tgt, tau, io.ldu(12));
      for (int j = 0; j < 3; j++) { io.st(j, tgt[j]); io.st(3 + j, tau[j]); }
    } break;
    case SR_CLIP_VELOCITIES: {
      F qs[3] = {io.ld(0), io.ld(1), io.ld(2)};
      float xi[6];
      for (int i = 0; i < 6; i++) xi[i] = io.ldu(3 + i);
      K::clip_velocities(ln, xi, qs, io.ldu(9));
      for (int j = 0; j < 3; j++) io.st(j, qs[j]);
      for (int i = 0; i < 6; i++) io.st(3 + i, ln.lane_f(xi[i]));
    } break;
    case SR_PICK_RANK: {
      F nd = io.ld(5), ns = io.ld(6), nj = io.ld(7);
      const F rank = io.ld(0), me = io.ld(1), d = io.ld(2), sb = io.ld(3), jj = io.ld(4);
      switch (targ) {
        case 0: K::template pick_rank<0>(ln, rank, me, d, sb, jj, nd, ns, nj); break;
        case 1: K::template pick_rank<1>(ln, rank, me, d, sb, jj, nd, ns, nj); break;
        case 2: K::template pick_rank<2>(ln, rank, me, d, sb, jj, nd, ns, nj); break;
        default: K::template pick_rank<3>(ln, rank, me, d, sb, jj, nd, ns, nj); break;
      }
      io.st(0, nd); io.st(1, ns); io.st(2, nj);
    } break;
    case SR_SELF: {
      typedef typename K::SelfRow SelfRow;
      const F zero = ln.lane_f(0.0f);
      SelfRow rw;
      if (targ == 2) {                     // the pieces alone
        F jt[3] = {io.ld(0), io.ld(1), io.ld(2)}, VA = io.ld(10), VB = io.ld(11), VJ = io.ld(12);
        float gt[6];
        for (int i = 0; i < 6; i++) gt[i] = io.ldu(3 + i);
        K::self_row_pack(ln, jt, gt, rw);
        io.st(0, rw.sa); io.st(1, rw.sb); io.st(2, rw.sj);
        io.st(3, ln.lane_f(K::self_row_velocity(rw, VA, VB, VJ)));
        K::self_row_apply(ln, rw, io.ldu(9), VA, VB, VJ);
        io.st(4, VA); io.st(5, VB); io.st(6, VJ);
        rw.c = rw.inv = rw.lam = 1.0f;
        K::self_row_clear(ln, rw);
        io.st(7, rw.sa); io.st(8, rw.sb); io.st(9, rw.sj); io.st(10, ln.lane_f(rw.c)); io.st(11, ln.lane_f(rw.inv)); io.st(12, ln.lane_f(rw.lam));
        break;
      }
      const V3<F> ub = v3(0), e1 = v3(4), e2 = v3(7), e3 = v3(10);
      typename K::LegFactor lf;
      lf.l11 = io.ld(13); lf.l21 = io.ld(14); lf.l31 = io.ld(15); lf.l22 = io.ld(16); lf.l32 = io.ld(17); lf.l33 = io.ld(18); lf.i11 = io.ld(19); lf.i22 = io.ld(20); lf.i33 = io.ld(21);
      lf.y1.a = v3(22); lf.y1.l = v3(25); lf.y2.a = v3(28); lf.y2.l = v3(31); lf.y3.a = v3(34); lf.y3.l = v3(37);
      F qs[3] = {io.ld(40), io.ld(41), io.ld(42)}, VA = io.ld(73), VB = io.ld(74), VJ = io.ld(75);
      float Sb[21], Sd[6];
      for (int i = 0; i < 21; i++) Sb[i] = io.ldu(43 + i);
      for (int i = 0; i < 6; i++) Sd[i] = io.ldu(64 + i);
      const bool have = io.ldu(71) > 0.5f;
      K::self_row_build(ln, rw, ub, io.ld(3), e1, e2, e3, lf, Sb, Sd, qs, io.ldu(70), have);
      io.st(0, rw.sa); io.st(1, rw.sb); io.st(2, rw.sj); io.st(3, ln.lane_f(rw.c)); io.st(4, ln.lane_f(rw.inv)); io.st(5, ln.lane_f(rw.lam));
      if (have) rw.lam = io.ldu(76);       // a multiplier from an earlier iteration
      io.st(6, ln.lane_f(K::self_row_velocity(rw, VA, VB, VJ)));
      if (targ == 0) K::self_turn(ln, rw, VA, VB, VJ);
      else K::self_fric_turn(ln, rw, io.ldu(72), VA, VB, VJ);
      io.st(7, ln.lane_f(rw.lam)); io.st(8, VA); io.st(9, VB); io.st(10, VJ);
      (void)zero;
    } break;
    case SR_PAIR: {
      typedef typename K::SelfRow SelfRow;
      SelfRow rw;
      const V3<float> ub = mk3<float>(io.ldu(0), io.ldu(1), io.ldu(2)), pb = mk3<float>(io.ldu(3), io.ldu(4), io.ldu(5));
      const B mine = io.ld(6) > 0.5f;
      const V3<F> e1 = v3(7), e2 = v3(10), e3 = v3(13);
      typename K::LegFactor lf;
      lf.l11 = io.ld(16); lf.l21 = io.ld(17); lf.l31 = io.ld(18); lf.l22 = io.ld(19); lf.l32 = io.ld(20); lf.l33 = io.ld(21); lf.i11 = io.ld(22); lf.i22 = io.ld(23); lf.i33 = io.ld(24);
      lf.y1.a = v3(25); lf.y1.l = v3(28); lf.y2.a = v3(31); lf.y2.l = v3(34); lf.y3.a = v3(37); lf.y3.l = v3(40);
      F qs[3] = {io.ld(43), io.ld(44), io.ld(45)}, VA = io.ld(88), VB = io.ld(89), VJ = io.ld(90);
      float Sb[21], Sd[6], xi[6];
      for (int i = 0; i < 21; i++) Sb[i] = io.ldu(46 + i);
      for (int i = 0; i < 6; i++) { Sd[i] = io.ldu(67 + i); xi[i] = io.ldu(73 + i); }
      StepParams P{};
      P.erp = io.ldu(79); P.erp_deep = io.ldu(80); P.erp_deep_below = io.ldu(81); P.max_depen = io.ldu(82);
      const bool have = io.ldu(85) > 0.5f;
      const int me = io.ldu(87) > 0.5f ? 1 : 0;
      K::pair_row_build(ln, rw, ub, pb, mine, e1, e2, e3, lf, Sb, Sd, xi, qs, P, io.ldu(83), io.ldu(84), targ == 0, have, me);
      io.st(0, rw.sa); io.st(1, rw.sb); io.st(2, rw.sj); io.st(3, ln.lane_f(rw.c)); io.st(4, ln.lane_f(rw.inv)); io.st(5, ln.lane_f(rw.lam));
      if (have) rw.lam = io.ldu(91);
      io.st(6, ln.lane_f(K::self_row_velocity(rw, VA, VB, VJ)));
      if (targ == 0) K::pair_turn(ln, rw, VA, VB, VJ, me);
      else K::pair_fric_turn(ln, rw, io.ldu(86), VA, VB, VJ, me);
      io.st(7, ln.lane_f(rw.lam)); io.st(8, VA); io.st(9, VB); io.st(10, VJ);
    } break;
    case SR_CAND_EVAL_POINT: {
      typename K::Base bs{};
      bs.p = mk3<float>(io.ldu(0), io.ldu(1), io.ldu(2));
      M3<float> R;
      M3<F> lR;
      for (int i = 0; i < 9; i++) { R.m[i] = io.ldu(3 + i); lR.m[i] = io.ld(12 + i); }
      V3<F> Ew;
      F rs;
      K::cand_eval_point(ln, bs, R, lR, v3(21), v3(24), v3(27), v3(30), io.ld(33), io.ld(34), io.ld(35), Ew, rs);
      io.st(0, Ew.x); io.st(1, Ew.y); io.st(2, Ew.z); io.st(3, rs);
    } break;
    default: break;
  }
}

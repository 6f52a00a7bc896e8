// contact_scan_body.hpp -- TEST INFRASTRUCTURE.  One driver for the members of Pmc<L> (lifelike_agility_and_play_amd/csrc/pmc_step.hpp) that choose among contact
// candidates: the terrain-edge detectors reverse_edge and leg_edge, and self_pick, one slot of the leg-leg pick.  (The deepest-K selection of the ground contacts is still
// text of substep_impl: tests/contact_scan_common.py LATER.)
// In the style of solver_rows_body.hpp: shared source, compiled once per lane policy, ONE entry per launch.  A sample is one environment ROW of 16 lanes
// (lane = 4 * leg + sub); what differs between GPU and host sits behind IO:
//   io.ld(w) / io.st(w, x)   operand / result word w of this row as L::F (the operand passes one multiply by a 1.0 from memory, so nothing folds)
//   io.ldu(w)                an env-uniform float (lane 0 of the row on the host, the lane's own copy on the GPU: the tests replicate it)
//   io.legc() / io.basec()   the pinned leg and base tables of the `consts` buffer, as the kernel arguments carry them
// The edge entries read: base position (3) | R (9) | n_shapes | yawed ycx ycy ycs ysn | q1 q2 q3 (per lane) | endf / edgef (per lane) | - - | 6 box records of 8 words
#pragma once

#define CS_IN_WORDS 72
#define CS_OUT_WORDS 24
#define CS_MAX_BLOCKS 64       // one-wave workgroups per launch: 64 x 4 = 256 rows
#define CS_MAX_SHAPES 6
#define CS_EDGE_NSHAPES 12
#define CS_EDGE_YAW 13
#define CS_EDGE_Q 18
#define CS_EDGE_END 21
#define CS_EDGE_SHAPES 24
#define CS_PICK_WORDS 11       // what one slot of self_pick leaves: have | cmin | dsel | u6[0..5] | cd[0] | cd[1]
// the `consts` buffer is the one of lane_prims_body.hpp: legc [LC_COUNT][4] | candc [CAND_TABLE_WORDS][16] | basec [BC_COUNT] | 1.0f  (the edge entries read legc and basec,
// the tables of the default model; the lane policies stage them as in the step kernels)
#define CS_CONSTS_LEGC 0
#define CS_CONSTS_CANDC (LC_COUNT * 4)
#define CS_CONSTS_BASEC (CS_CONSTS_CANDC + CAND_TABLE_WORDS * PMC_ROW)
#define CS_CONSTS_ONE (CS_CONSTS_BASEC + BC_COUNT)
#define CS_CONSTS_WORDS (CS_CONSTS_ONE + 1)

enum ContactScanEntry {
  CS_SELF_PICK = 0,     // targ = slots - 1: the first slot, or the first and then the second on what the first left
  CS_REVERSE_EDGE,      // a terrain edge under the trunk: depth | Pb | nw
  CS_LEG_EDGE,          // a terrain edge across the leg's thigh and shank boxes (LegKin from leg_fk at the row's joint angles): depth | Pb | nw | link | shape
  CS_ENTRY_END
};

static inline int cs_max_targ(int entry) { return entry == CS_SELF_PICK ? 1 : 0; }

// what a launch may be asked: a known entry, a template argument it is instantiated for, a block count the caller's buffers (given in floats) hold.  Nothing a test passes
// may index past the buffers it handed over (both ABIs refuse the call otherwise).
static inline bool cs_args_in_bounds(int entry, int targ, int n_blocks, long in_floats, long out_floats, long consts_floats) {
  if (entry < 0 || entry >= CS_ENTRY_END) return false;
  if (targ < 0 || targ > cs_max_targ(entry)) return false;
  if (n_blocks < 1 || n_blocks > CS_MAX_BLOCKS) return false;
  return in_floats >= (long)n_blocks * 4 * CS_IN_WORDS * 16 && out_floats >= (long)n_blocks * 4 * CS_OUT_WORDS * 16 && consts_floats >= CS_CONSTS_WORDS;
}

template <class L, class IO>
LL_D void run_contact_scan(L& ln, IO& io, int entry, int targ) {
  typedef Pmc<L> K;
  typedef typename L::F F;
  const auto v3 = [&](int w) { return mk3<F>(io.ld(w), io.ld(w + 1), io.ld(w + 2)); };
  switch (entry) {
    case CS_SELF_PICK: {
      F cd[2] = {io.ld(0), io.ld(1)}, cpair[2] = {io.ld(2), io.ld(3)};
      V3<F> cP[2] = {v3(4), v3(7)}, cN[2] = {v3(10), v3(13)};
      for (int slot = 0; slot <= targ; slot++) {
        bool have;
        float cmin, dsel, u6[6];
        K::self_pick(ln, cd, cpair, cP, cN, have, cmin, dsel, u6);
        const int w = slot * CS_PICK_WORDS;
        io.st(w, ln.lane_f(have ? 1.0f : 0.0f)); io.st(w + 1, ln.lane_f(cmin)); io.st(w + 2, ln.lane_f(dsel));
        for (int i = 0; i < 6; i++) io.st(w + 3 + i, ln.lane_f(u6[i]));
        io.st(w + 9, cd[0]); io.st(w + 10, cd[1]);
      }
    } break;
    case CS_REVERSE_EDGE: case CS_LEG_EDGE: {
      alignas(16) float shp[(CS_MAX_SHAPES + 1) * 8];          // (one record past the list is readable, as in the row scratch of the step kernels)
      for (int i = 0; i < (CS_MAX_SHAPES + 1) * 8; i++) shp[i] = i < CS_MAX_SHAPES * 8 ? io.ldu(CS_EDGE_SHAPES + i) : 0.0f;
      typename K::SubstepExtra ex{};
      const int n = (int)(io.ldu(CS_EDGE_NSHAPES) + 0.5f);
      ex.shapes = shp; ex.n_shapes = n < 0 ? 0 : (n > CS_MAX_SHAPES ? CS_MAX_SHAPES : n);
      ex.yawed = io.ldu(CS_EDGE_YAW) > 0.5f; ex.ycx = io.ldu(CS_EDGE_YAW + 1); ex.ycy = io.ldu(CS_EDGE_YAW + 2); ex.ycs = io.ldu(CS_EDGE_YAW + 3); ex.ysn = io.ldu(CS_EDGE_YAW + 4);
      StepParams P{};
      P.legc = io.legc(); P.basec = io.basec(); P.margin_dist = (float)LLM_CONTACT_MARGIN;
      typename K::Base bs{};
      bs.p = mk3<float>(io.ldu(0), io.ldu(1), io.ldu(2));
      M3<float> R;
      for (int i = 0; i < 9; i++) R.m[i] = io.ldu(3 + i);
      F depth, link, shape;
      V3<F> Pb, nw;
      if (entry == CS_REVERSE_EDGE) {
        K::reverse_edge(ln, P, &ex, bs, R, io.ld(CS_EDGE_END), depth, Pb, nw);
      } else {
        const typename K::LegKin k = K::leg_fk(ln, io.legc(), io.ld(CS_EDGE_Q), io.ld(CS_EDGE_Q + 1), io.ld(CS_EDGE_Q + 2));
        K::leg_edge(ln, P, &ex, bs, R, k, io.legc(), io.ld(CS_EDGE_END), depth, Pb, nw, link, shape);
        io.st(7, link); io.st(8, shape);
      }
      io.st(0, depth); io.st(1, Pb.x); io.st(2, Pb.y); io.st(3, Pb.z); io.st(4, nw.x); io.st(5, nw.y); io.st(6, nw.z);
    } break;
    default: break;
  }
}

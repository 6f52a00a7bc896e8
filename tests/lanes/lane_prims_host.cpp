// lane_prims_host.cpp -- TEST INFRASTRUCTURE.  The primitive driver (lane_prims_body.hpp) instantiated for the 16-wide host stand-in of a DPP row
// (tests/emul/lanes_host.hpp), one row at a time, with the C ABI of lane_prims.hip: tests/test_lane_prims_emul.py holds the twin to the float64 statement
// here, tests/test_gpu_lane_prims.py holds the GPU lanes to the twin.  Built with the flags of libllenv_emul.so.
#include "../emul/lanes_host.hpp"

#include <thread>

#include "../../include/llenv_model.h"
#include "../../lifelike_agility_and_play_amd/csrc/lanes.hpp"
#include "../../lifelike_agility_and_play_amd/csrc/pmc_params.hpp"
#include "lane_prims_body.hpp"

static_assert(sizeof(((HostLanes*)0)->scratch_) == PMC_ROW_SCRATCH * sizeof(float), "lanes_host.hpp: scratch_ is PMC_ROW_SCRATCH floats");

struct HostIO {
  const float* in;       // this row's [LP_IN_WORDS][16]
  float* out;            // this row's [LP_OUT_WORDS][16]
  float* aux_;
  const double* auxd_;
  const float* consts;
  const int* ia_;
  fN ld(int w) const { const volatile float one = consts[LP_CONSTS_ONE]; fN r; for (int i = 0; i < EW; i++) r.v[i] = in[w * EW + i] * one; return r; }
  bool pred(int w) const { return in[w * EW] > 0.0f; }      // the host's per-env code is a row of one lane: lane 0 speaks
  void st(int w, const fN& x) const { for (int i = 0; i < EW; i++) out[w * EW + i] = x.v[i]; }
  void stu(int w, float x) const { for (int i = 0; i < EW; i++) out[w * EW + i] = x; }
  float* aux() const { return aux_; }
  const double* auxd() const { return auxd_; }
  int ia(int k) const { return ia_[k]; }
  const float* legc() const { return consts + LP_CONSTS_LEGC; }
  const float* basec() const { return consts + LP_CONSTS_BASEC; }
};

template <class L>
static void run_row(int row, PairLink* link, int prim, int targ, const float* in, float* out, float* aux, const double* auxd, const float* consts, const int* ia) {
  L ln(consts + LP_CONSTS_CANDC);
  ln.link_ = link;
  ln.side_ = row & 1;
  HostIO io{in + (long)row * LP_IN_WORDS * EW, out + (long)row * LP_OUT_WORDS * EW, aux + (long)row * LP_AUX_WORDS, auxd, consts, ia};
  run_prim(ln, io, prim, targ);
}

template <class L>
static void run_all(int prim, int targ, const float* in, float* out, int active, float* aux, const double* auxd, const float* consts, const int* ia) {
  if (prim == LP_PEER) {            // the two rows of a pair meet in PairLink, as the two robots of an arena do in emul.cpp
    for (int p = 0; p < 2; p++) {
      if (((active >> (2 * p)) & 3) != 3) continue;
      PairLink link;
      std::thread other([&] { run_row<L>(2 * p + 1, &link, prim, targ, in, out, aux, auxd, consts, ia); });
      run_row<L>(2 * p, &link, prim, targ, in, out, aux, auxd, consts, ia);
      other.join();
    }
    return;
  }
  for (int row = 0; row < 4; row++)
    if ((active >> row) & 1) run_row<L>(row, nullptr, prim, targ, in, out, aux, auxd, consts, ia);
}

extern "C" {
void ll_lane_prims_dims(int* d) {
  d[0] = LP_IN_WORDS; d[1] = LP_OUT_WORDS; d[2] = LP_AUX_WORDS; d[3] = LP_AUXD_WORDS; d[4] = LC_COUNT; d[5] = CAND_TABLE_WORDS; d[6] = BC_COUNT; d[7] = LP_CONSTS_WORDS;
  d[8] = LK_BASE; d[9] = PMC_ROW_SCRATCH; d[10] = -1; d[11] = -1; d[12] = -1; d[13] = 3; /* policies */ d[14] = HostLanes::kConeLdsAt;
}
int ll_lane_prims_run(int policy, int prim, int targ, const float* in, float* out, int active_rows, float* aux, const double* auxd, const float* consts, const int* ia) {
  if (!lp_args_in_bounds(prim, ia)) return -2;
  switch (policy) {
    case 0: run_all<HostLanes>(prim, targ, in, out, active_rows & 15, aux, auxd, consts, ia); break;
    case 1: run_all<WithConeInLdsHost<HostLanes>>(prim, targ, in, out, active_rows & 15, aux, auxd, consts, ia); break;
    case 2: run_all<WithGramPipeHost<HostLanes>>(prim, targ, in, out, active_rows & 15, aux, auxd, consts, ia); break;
    default: return -1;
  }
  return 0;
}
}

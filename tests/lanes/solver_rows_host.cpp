// solver_rows_host.cpp -- TEST INFRASTRUCTURE.  The row driver (solver_rows_body.hpp) instantiated for the 16-wide host stand-in of a DPP row (tests/emul/lanes_host.hpp),
// one row at a time, with the C ABI of solver_rows.hip: tests/test_solver_rows_emul.py holds this twin to the float64 statements, tests/test_gpu_solver_rows.py holds the
// GPU copies to the twin's error.  Built with the flags of libllenv_emul.so (correctly rounded IEEE operations, every multiply-add a product and a sum).
#include "../emul/lanes_host.hpp"

#include <thread>

#include "../../lifelike_agility_and_play_amd/csrc/pmc_step.hpp"
#include "solver_rows_body.hpp"

struct HostIO {
  const float* in;       // this row's [SR_IN_WORDS][16]
  float* out;            // this row's [SR_OUT_WORDS][16]
  const float* consts;
  fN ld(int w) const { const volatile float one = consts[SR_CONSTS_ONE]; fN r; for (int i = 0; i < EW; i++) r.v[i] = in[w * EW + i] * one; return r; }
  float ldu(int w) const { const volatile float one = consts[SR_CONSTS_ONE]; return in[w * EW] * one; }      // env-uniform: lane 0 speaks
  void st(int w, const fN& x) const { for (int i = 0; i < EW; i++) out[w * EW + i] = x.v[i]; }
};

template <class L>
static void run_row(long row, PairLink* link, int entry, int targ, const float* in, float* out, const float* consts) {
  L ln(consts + SR_CONSTS_CANDC);
  ln.link_ = link;
  ln.side_ = (int)(row & 1);
  HostIO io{in + row * SR_IN_WORDS * EW, out + row * SR_OUT_WORDS * EW, consts};
  run_solver_rows(ln, io, entry, targ);
}

template <class L>
static void run_all(int entry, int targ, int n_blocks, int active_rows, const float* in, float* out, const float* consts) {
  if (entry == SR_PAIR) {           // the two rows of an arena meet in PairLink, as the two robots do in emul.cpp; a pair runs only when both its rows are live
    for (long row = 0; row < (long)n_blocks * 4; row += 2) {
      if (((active_rows >> (row & 3)) & 3) != 3) continue;
      PairLink link;
      std::thread other([&] { run_row<L>(row + 1, &link, entry, targ, in, out, consts); });
      run_row<L>(row, &link, entry, targ, in, out, consts);
      other.join();
    }
    return;
  }
  for (long row = 0; row < (long)n_blocks * 4; row++)
    if ((active_rows >> (row & 3)) & 1) run_row<L>(row, nullptr, entry, targ, in, out, consts);
}

extern "C" {
void ll_solver_rows_dims(int* d) {
  d[0] = SR_IN_WORDS; d[1] = SR_OUT_WORDS; d[2] = SR_MAX_BLOCKS; d[3] = SR_CONSTS_WORDS; d[4] = 3; /* policies */ d[5] = -1; d[6] = -1; d[7] = SR_ENTRY_END; d[8] = -1;
}
int ll_solver_rows_run(int policy, int entry, int targ, int n_blocks, int active_rows, const float* in, long in_floats, float* out, long out_floats, const float* consts,
                       long consts_floats) {
  if (policy < 0 || policy > 2) return -1;
  if (!sr_args_in_bounds(entry, targ, policy == 2, n_blocks, in_floats, out_floats, consts_floats)) return -2;
  switch (policy) {
    case 0: run_all<HostLanes>(entry, targ, n_blocks, active_rows & 15, in, out, consts); break;
    case 1: run_all<WithConeInLdsHost<HostLanes>>(entry, targ, n_blocks, active_rows & 15, in, out, consts); break;
    default: run_all<WithGramPipeHost<HostLanes>>(entry, targ, n_blocks, active_rows & 15, in, out, consts); break;
  }
  return 0;
}
}

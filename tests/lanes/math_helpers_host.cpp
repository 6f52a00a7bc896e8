// math_helpers_host.cpp -- TEST INFRASTRUCTURE.  The helper driver (math_helpers_body.hpp) instantiated for the 16-wide host stand-in of a DPP row
// (tests/emul/lanes_host.hpp), one row at a time, with the C ABI of math_helpers.hip: tests/test_math_helpers_emul.py holds this twin to the float64 statements,
// tests/test_gpu_math_helpers.py holds the GPU copies to the twin.  Built with the flags of libllenv_emul.so (correctly rounded IEEE operations, glibc's float functions).
#include "../emul/lanes_host.hpp"

#include <string.h>

#include "../../lifelike_agility_and_play_amd/csrc/pmc_step.hpp"
#include "math_helpers_body.hpp"

struct HostIO {
  const float* in;       // this row's [MH_IN_WORDS][16]
  float* out;            // this row's [MH_OUT_WORDS][16]
  const double* auxd_;
  const float* consts;
  fN ld(int w) const { const volatile float one = consts[MH_CONSTS_ONE]; fN r; for (int i = 0; i < EW; i++) r.v[i] = in[w * EW + i] * one; return r; }
  float ldu(int w) const { const volatile float one = consts[MH_CONSTS_ONE]; return in[w * EW] * one; }      // env-uniform: lane 0 speaks
  void st(int w, const fN& x) const { for (int i = 0; i < EW; i++) out[w * EW + i] = x.v[i]; }
  void stu(int w, float x) const { for (int i = 0; i < EW; i++) out[w * EW + i] = x; }
  const double* auxd() const { return auxd_; }
  const float* legc() const { return consts + MH_CONSTS_LEGC; }
};
struct HostScalarIO {      // one lane of the row: the scalar helpers run once per lane
  const HostIO& io;
  int lane;
  float ld(int w) const { const volatile float one = io.consts[MH_CONSTS_ONE]; return io.in[w * EW + lane] * one; }
  uint32_t raw(int w) const { uint32_t u; memcpy(&u, io.in + w * EW + lane, 4); return u; }
  void st(int w, float x) const { io.out[w * EW + lane] = x; }
  void straw(int w, uint32_t u) const { memcpy(io.out + w * EW + lane, &u, 4); }
};

extern "C" {
void ll_math_helpers_dims(int* d) {
  d[0] = MH_IN_WORDS; d[1] = MH_OUT_WORDS; d[2] = MH_AUXD_WORDS; d[3] = MH_MAX_BLOCKS; d[4] = LC_COUNT; d[5] = CAND_TABLE_WORDS; d[6] = BC_COUNT; d[7] = MH_CONSTS_WORDS;
  d[8] = LK_BASE; d[9] = 1; /* policies */
}
int ll_math_helpers_run(int policy, int helper, int targ, int n_blocks, int active_rows, const float* in, long in_floats, float* out, long out_floats, const double* auxd,
                        long auxd_doubles, const float* consts, long consts_floats) {
  if (!mh_args_in_bounds(helper, targ, n_blocks, in_floats, out_floats, auxd_doubles, consts_floats)) return -2;
  if (policy != 0) return -1;
  for (long row = 0; row < (long)n_blocks * 4; row++) {
    if (!((active_rows >> (row & 3)) & 1)) continue;
    HostLanes ln(consts + MH_CONSTS_CANDC);
    HostIO io{in + row * MH_IN_WORDS * EW, out + row * MH_OUT_WORDS * EW, auxd, consts};
    if (helper < MH_SCALAR_END) {
      for (int lane = 0; lane < EW; lane++) { HostScalarIO sio{io, lane}; run_scalar_helper<HostLanes>(sio, helper); }
    } else {
      run_lane_helper(ln, io, helper, targ);
    }
  }
  return 0;
}
}

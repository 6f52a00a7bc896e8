// contact_scan_host.cpp -- TEST INFRASTRUCTURE.  The contact selection driver (contact_scan_body.hpp) instantiated for the 16-wide host stand-in of a DPP row
// (tests/emul/lanes_host.hpp), one row at a time, with the C ABI of contact_scan.hip: tests/test_contact_scan_emul.py holds this twin to the statements,
// tests/test_gpu_contact_scan.py holds the GPU copies to the twin, bit for bit.  Built with the flags of libllenv_emul.so (correctly rounded IEEE operations, every
// multiply-add a product and a sum).
#include "../emul/lanes_host.hpp"

#include "../../lifelike_agility_and_play_amd/csrc/pmc_step.hpp"
#include "../../lifelike_agility_and_play_amd/csrc/pmc_tables.hpp"
#include "contact_scan_body.hpp"

struct HostIO {
  const float* in;       // this row's [CS_IN_WORDS][16]
  float* out;            // this row's [CS_OUT_WORDS][16]
  const float* consts;
  fN ld(int w) const { const volatile float one = consts[CS_CONSTS_ONE]; fN r; for (int i = 0; i < EW; i++) r.v[i] = in[w * EW + i] * one; return r; }
  float ldu(int w) const { const volatile float one = consts[CS_CONSTS_ONE]; return in[w * EW] * one; }      // env-uniform: lane 0 speaks
  const float* legc() const { return consts + CS_CONSTS_LEGC; }
  const float* basec() const { return consts + CS_CONSTS_BASEC; }
  void st(int w, const fN& x) const { for (int i = 0; i < EW; i++) out[w * EW + i] = x.v[i]; }
};

template <class L>
static void run_all(int entry, int targ, int n_blocks, int active_rows, const float* in, float* out, const float* consts) {
  for (long row = 0; row < (long)n_blocks * 4; row++) {
    if (!((active_rows >> (row & 3)) & 1)) continue;
    L ln(consts + CS_CONSTS_CANDC);
    HostIO io{in + row * CS_IN_WORDS * EW, out + row * CS_OUT_WORDS * EW, consts};
    run_contact_scan(ln, io, entry, targ);
  }
}

extern "C" {
void ll_contact_scan_dims(int* d) {
  d[0] = CS_IN_WORDS; d[1] = CS_OUT_WORDS; d[2] = CS_MAX_BLOCKS; d[3] = CS_CONSTS_WORDS; d[4] = 1; /* policies */ d[5] = PMC_FRONT_TRIM; d[6] = CS_ENTRY_END; d[7] = CS_PICK_WORDS;
}
// the pinned tables of a model blob as the engines build them (csrc/pmc_tables.hpp), into the `consts` buffer's legc and basec; 0: done
int ll_contact_scan_tables(const double* blob, int blob_len, float* consts, long consts_floats) {
  std::vector<float> legc, basec;
  if (consts_floats < CS_CONSTS_WORDS || !pmc_build_tables(blob, blob_len, legc, basec).empty()) return -1;
  for (int i = 0; i < LC_COUNT * 4; i++) consts[CS_CONSTS_LEGC + i] = legc[i];
  for (int i = 0; i < BC_COUNT; i++) consts[CS_CONSTS_BASEC + i] = basec[i];
  return 0;
}
int ll_contact_scan_run(int policy, int entry, int targ, int n_blocks, int active_rows, const float* in, long in_floats, float* out, long out_floats, const float* consts,
                        long consts_floats) {
  if (policy != 0) return -1;
  if (!cs_args_in_bounds(entry, targ, n_blocks, in_floats, out_floats, consts_floats)) return -2;
  run_all<HostLanes>(entry, targ, n_blocks, active_rows & 15, in, out, consts);
  return 0;
}
}

// contact_scan.hip -- TEST INFRASTRUCTURE.  Up to 64 one-wave workgroups (four 16-lane rows each) run ONE of the contact selections of Pmc<L> (contact_scan_body.hpp)
// under the GPU lane policies of the step kernels whose row reductions differ -- the plain lanes and the pinned lanes of the one-wave-per-SIMD kernels (llenv.hip) -- so that
// tests/test_gpu_contact_scan.py can hold each to its host twin and to the statement (tests/contact_scan_ref.py), bit for bit.  Compiled with the product's flags; built
// again with -DPMC_FRONT_TRIM=0 (rmin of lanes.hpp in its earlier form: fminf over DPP moves).  Never linked into the product.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../lifelike_agility_and_play_amd/csrc/pmc_step.hpp"
#include "contact_scan_body.hpp"

struct CsArgs {
  const float* in;       // [n_blocks * 4 rows][CS_IN_WORDS][16]
  float* out;            // [n_blocks * 4 rows][CS_OUT_WORDS][16]
  const float* consts;   // legc [LC_COUNT][4] | candc [CAND_TABLE_WORDS][16] | basec [BC_COUNT] | 1.0f
  int entry, targ, active_rows;
};
struct GpuIO {
  const CsArgs& A;
  const long row;
  const int lane;
  const float one;
  __device__ GpuIO(const CsArgs& a) : A(a), row((long)blockIdx.x * 4 + ((threadIdx.x >> 4) & 3)), lane(threadIdx.x & 15), one(a.consts[CS_CONSTS_ONE]) {}
  __device__ float ld(int w) const { return A.in[(row * CS_IN_WORDS + w) * PMC_ROW + lane] * one; }
  __device__ float ldu(int w) const { return ld(w); }
  __device__ const float* legc() const { return A.consts + CS_CONSTS_LEGC; }
  __device__ const float* basec() const { return A.consts + CS_CONSTS_BASEC; }
  __device__ void st(int w, float x) const { A.out[(row * CS_OUT_WORDS + w) * PMC_ROW + lane] = x; }
};

template <class L>
__global__ __launch_bounds__(64) void contact_scan_kernel(CsArgs A) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  L ln(lds);
  // every one of the 64 lanes stages the tables, as in the step kernels; rows outside `active_rows` leave before the entry, which then runs under a partial EXEC
  if constexpr (L::kHoldLink) ln.stage_consts(A.consts + CS_CONSTS_LEGC, LC_COUNT, A.consts + CS_CONSTS_CANDC, CAND_TABLE_WORDS, A.consts + CS_CONSTS_BASEC);
  else ln.stage_consts(A.consts + CS_CONSTS_LEGC, LC_COUNT, A.consts + CS_CONSTS_CANDC, CAND_TABLE_WORDS);
  if (!((A.active_rows >> (threadIdx.x >> 4)) & 1)) return;
  GpuIO io(A);
  run_contact_scan(ln, io, A.entry, A.targ);
}

typedef GpuLanesPinned<LC_COUNT, 7, BC_COUNT, LK_BASE> GpuLanesPmc1Plain;     // as llenv.hip (LL_PIN_PMC)

static size_t cs_lds_bytes() { return ((size_t)LC_COUNT * 4 + (size_t)CAND_TABLE_WORDS * PMC_ROW + 4 * 12 + 4 * (size_t)PMC_ROW_SCRATCH) * sizeof(float); }

extern "C" {
// sizes of the buffers ll_contact_scan_run takes and the switch this copy was built with
void ll_contact_scan_dims(int* d) {
  d[0] = CS_IN_WORDS; d[1] = CS_OUT_WORDS; d[2] = CS_MAX_BLOCKS; d[3] = CS_CONSTS_WORDS; d[4] = 2; /* policies */ d[5] = PMC_FRONT_TRIM; d[6] = CS_ENTRY_END; d[7] = CS_PICK_WORDS;
}
// one launch of n_blocks one-wave workgroups on the null stream; the caller synchronises.  The buffer sizes are given in elements and checked against what the launch
// indexes.  Returns the HIP error of the launch (0: none), -1 for an unknown policy, -2 for arguments out of bounds.
int ll_contact_scan_run(int policy, int entry, int targ, int n_blocks, int active_rows, const float* in, long in_floats, float* out, long out_floats, const float* consts,
                        long consts_floats) {
  if (policy < 0 || policy > 1) return -1;
  if (!cs_args_in_bounds(entry, targ, n_blocks, in_floats, out_floats, consts_floats)) return -2;
  CsArgs A{in, out, consts, entry, targ, active_rows & 15};
  const size_t lds = cs_lds_bytes();
  switch (policy) {
    case 0: hipLaunchKernelGGL(contact_scan_kernel<GpuLanes>, dim3(n_blocks), dim3(64), lds, 0, A); break;
    default: hipLaunchKernelGGL(contact_scan_kernel<GpuLanesPmc1Plain>, dim3(n_blocks), dim3(64), lds, 0, A); break;
  }
  return (int)hipGetLastError();
}
}

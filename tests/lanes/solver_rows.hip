// solver_rows.hip -- TEST INFRASTRUCTURE.  Up to 64 one-wave workgroups (four 16-lane rows each) run ONE of the row builders or sweeps of Pmc<L>
// (solver_rows_body.hpp) under every GPU lane policy the step kernels are built with (llenv.hip), so that tests/test_gpu_solver_rows.py can hold each to its host twin
// and to the float64 statement (tests/solver_rows_ref.py).  Compiled with the product's flags; built again with -DLL_MFMA_GRAM=1 (finish_row, cross_gram and the contact
// rows form their Gram scalars on the matrix cores), -DLL_CONE_PIPE=0 (the cone round's turn) and -DLL_PEER_MODE=1 / 2 (peer_u of the robot-robot rows) for the forms
// the product does not ship.  Never linked into the product.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../lifelike_agility_and_play_amd/csrc/pmc_step.hpp"
#include "solver_rows_body.hpp"

struct SrArgs {
  const float* in;       // [n_blocks * 4 rows][SR_IN_WORDS][16]
  float* out;            // [n_blocks * 4 rows][SR_OUT_WORDS][16]
  const float* consts;   // legc [LC_COUNT][4] | candc [CAND_TABLE_WORDS][16] | basec [BC_COUNT] | 1.0f
  int entry, targ, active_rows;
};
struct GpuIO {
  const SrArgs& A;
  const long row;
  const int lane;
  const float one;
  __device__ GpuIO(const SrArgs& a) : A(a), row((long)blockIdx.x * 4 + ((threadIdx.x >> 4) & 3)), lane(threadIdx.x & 15), one(a.consts[SR_CONSTS_ONE]) {}
  __device__ float ld(int w) const { return A.in[(row * SR_IN_WORDS + w) * PMC_ROW + lane] * one; }
  __device__ float ldu(int w) const { return ld(w); }
  __device__ void st(int w, float x) const { A.out[(row * SR_OUT_WORDS + w) * PMC_ROW + lane] = x; }
};

template <class L>
__global__ __launch_bounds__(64) void solver_rows_kernel(SrArgs A) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  L ln(lds);
  // every one of the 64 lanes stages the tables, as in the step kernels; rows outside `active_rows` leave before the entry, which then runs under a partial EXEC
  if constexpr (L::kHoldLink) ln.stage_consts(A.consts + SR_CONSTS_LEGC, LC_COUNT, A.consts + SR_CONSTS_CANDC, CAND_TABLE_WORDS, A.consts + SR_CONSTS_BASEC);
  else ln.stage_consts(A.consts + SR_CONSTS_LEGC, LC_COUNT, A.consts + SR_CONSTS_CANDC, CAND_TABLE_WORDS);
  if (!((A.active_rows >> (threadIdx.x >> 4)) & 1)) return;
  GpuIO io(A);
  run_solver_rows(ln, io, A.entry, A.targ);
}

typedef GpuLanesPinned<LC_COUNT> GpuLanes1;                                   // as llenv.hip
typedef GpuLanesPinned<LC_COUNT, 7, BC_COUNT, LK_BASE> GpuLanesPmc1Plain;     // as llenv.hip (LL_PIN_PMC)

static size_t sr_lds_bytes() { return ((size_t)LC_COUNT * 4 + (size_t)CAND_TABLE_WORDS * PMC_ROW + 4 * 12 + 4 * (size_t)PMC_ROW_SCRATCH) * sizeof(float); }

extern "C" {
// sizes of the buffers ll_solver_rows_run takes and the switches this copy was built with
void ll_solver_rows_dims(int* d) {
  d[0] = SR_IN_WORDS; d[1] = SR_OUT_WORDS; d[2] = SR_MAX_BLOCKS; d[3] = SR_CONSTS_WORDS; d[4] = 7; /* policies */ d[5] = LL_CONE_PIPE; d[6] = LL_MFMA_GRAM; d[7] = SR_ENTRY_END; d[8] = LL_PEER_MODE;
}
// one launch of n_blocks one-wave workgroups on the null stream; the caller synchronises.  The buffer sizes are given in elements and checked against what the launch
// indexes.  Returns the HIP error of the launch (0: none), -1 for an unknown policy, -2 for arguments out of bounds.
int ll_solver_rows_run(int policy, int entry, int targ, int n_blocks, int active_rows, const float* in, long in_floats, float* out, long out_floats, const float* consts,
                       long consts_floats) {
  if (policy < 0 || policy > 6) return -1;
  if (!sr_args_in_bounds(entry, targ, policy == 6, n_blocks, in_floats, out_floats, consts_floats)) return -2;
  SrArgs A{in, out, consts, entry, targ, active_rows & 15};
  const size_t lds = sr_lds_bytes();
  switch (policy) {
    case 0: hipLaunchKernelGGL(solver_rows_kernel<GpuLanes>, dim3(n_blocks), dim3(64), lds, 0, A); break;
    case 1: hipLaunchKernelGGL(solver_rows_kernel<GpuLanes1>, dim3(n_blocks), dim3(64), lds, 0, A); break;
    case 2: hipLaunchKernelGGL(solver_rows_kernel<GpuLanesPmc1Plain>, dim3(n_blocks), dim3(64), lds, 0, A); break;
    case 3: hipLaunchKernelGGL(solver_rows_kernel<WithTurnMasksCmp<GpuLanes>>, dim3(n_blocks), dim3(64), lds, 0, A); break;
    case 4: hipLaunchKernelGGL(solver_rows_kernel<WithTurnMasksCmp<GpuLanesPmc1Plain>>, dim3(n_blocks), dim3(64), lds, 0, A); break;
    case 5: hipLaunchKernelGGL(solver_rows_kernel<WithConeInLds<GpuLanes1>>, dim3(n_blocks), dim3(64), lds, 0, A); break;
    default: hipLaunchKernelGGL(solver_rows_kernel<WithGramPipe<GpuLanesPmc1Plain>>, dim3(n_blocks), dim3(64), lds, 0, A); break;
  }
  return (int)hipGetLastError();
}
}

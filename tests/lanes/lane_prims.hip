// lane_prims.hip -- TEST INFRASTRUCTURE.  One 64-lane wave (four 16-lane rows) runs ONE primitive of the lane policy (lane_prims_body.hpp) under every
// GPU lane policy the step kernels are built with (llenv.hip), so that tests/test_gpu_lane_prims.py can hold each primitive to its host twin
// (tests/emul/lanes_host.hpp) and to the float64 statement (tests/lane_prims_ref.py).  Compiled with the product's flags; built again with
// -DLL_CONE_PIPE=0, -DLL_MFMA_GRAM=1, -DLL_PEER_MODE=1 / 2 for the forms the product does not ship.  Never linked into the product library.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../lifelike_agility_and_play_amd/csrc/lanes.hpp"
#include "../../include/llenv_model.h"
#include "../../lifelike_agility_and_play_amd/csrc/pmc_params.hpp"
#include "lane_prims_body.hpp"

struct LpArgs {
  const float* in;       // [4 rows][LP_IN_WORDS][16]
  float* out;            // [4 rows][LP_OUT_WORDS][16]
  float* aux;            // [4 rows][LP_AUX_WORDS]
  const double* auxd;    // [LP_AUXD_WORDS]
  const float* consts;   // legc [LC_COUNT][4] | candc [CAND_TABLE_WORDS][16] | basec [BC_COUNT] | 1.0f
  int prim, targ, active_rows;
  int ia[4];
};
struct GpuIO {
  const LpArgs& A;
  const int row, lane;
  const float one;
  __device__ GpuIO(const LpArgs& a) : A(a), row((threadIdx.x >> 4) & 3), lane(threadIdx.x & 15), one(a.consts[LP_CONSTS_ONE]) {}
  __device__ float ld(int w) const { return A.in[(row * LP_IN_WORDS + w) * PMC_ROW + lane] * one; }
  __device__ bool pred(int w) const { return A.in[(row * LP_IN_WORDS + w) * PMC_ROW + lane] > 0.0f; }
  __device__ void st(int w, float x) const { A.out[(row * LP_OUT_WORDS + w) * PMC_ROW + lane] = x; }
  __device__ void stu(int w, float x) const { st(w, x); }
  __device__ float* aux() const { return A.aux + row * LP_AUX_WORDS; }
  __device__ const double* auxd() const { return A.auxd; }
  __device__ int ia(int k) const { return A.ia[k]; }
  __device__ const float* legc() const { return A.consts + LP_CONSTS_LEGC; }
  __device__ const float* basec() const { return A.consts + LP_CONSTS_BASEC; }
};

template <class L>
__global__ __launch_bounds__(64) void lane_prims_kernel(LpArgs A) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  L ln(lds);
  // every one of the 64 lanes stages the tables, as in the step kernels; rows outside `active_rows` leave before the primitive, which then runs under a partial EXEC
  if constexpr (L::kHoldLink) ln.stage_consts(A.consts + LP_CONSTS_LEGC, LC_COUNT, A.consts + LP_CONSTS_CANDC, CAND_TABLE_WORDS, A.consts + LP_CONSTS_BASEC);
  else ln.stage_consts(A.consts + LP_CONSTS_LEGC, LC_COUNT, A.consts + LP_CONSTS_CANDC, CAND_TABLE_WORDS);
  if (!((A.active_rows >> (threadIdx.x >> 4)) & 1)) return;
  GpuIO io(A);
  run_prim(ln, io, A.prim, A.targ);
}

typedef GpuLanesPinned<LC_COUNT> GpuLanes1;                                   // as llenv.hip
typedef GpuLanesPinned<LC_COUNT, 7, BC_COUNT, LK_BASE> GpuLanesPmc1Plain;     // as llenv.hip (LL_PIN_PMC)

static size_t lp_lds_bytes() { return ((size_t)LC_COUNT * 4 + (size_t)CAND_TABLE_WORDS * PMC_ROW + 4 * 12 + 4 * (size_t)PMC_ROW_SCRATCH) * sizeof(float); }

extern "C" {
// sizes of the buffers ll_lane_prims_run takes and the switches this copy was built with
void ll_lane_prims_dims(int* d) {
  d[0] = LP_IN_WORDS; d[1] = LP_OUT_WORDS; d[2] = LP_AUX_WORDS; d[3] = LP_AUXD_WORDS; d[4] = LC_COUNT; d[5] = CAND_TABLE_WORDS; d[6] = BC_COUNT; d[7] = LP_CONSTS_WORDS;
  d[8] = LK_BASE; d[9] = PMC_ROW_SCRATCH; d[10] = LL_CONE_PIPE; d[11] = LL_MFMA_GRAM; d[12] = LL_PEER_MODE; d[13] = 7; /* policies */ d[14] = CONE_LDS_AT;
}
// one launch of one wave on the null stream; the caller synchronises.  Returns the HIP error of the launch (0: none), -1 for an unknown policy.
int ll_lane_prims_run(int policy, int prim, int targ, const float* in, float* out, int active_rows, float* aux, const double* auxd, const float* consts, const int* ia) {
  LpArgs A{in, out, aux, auxd, consts, prim, targ, active_rows & 15, {ia[0], ia[1], ia[2], ia[3]}};
  const size_t lds = lp_lds_bytes();
  if (!lp_args_in_bounds(prim, ia)) return -2;      // nothing a test passes may index past the buffers the launch was given
  switch (policy) {
    case 0: hipLaunchKernelGGL(lane_prims_kernel<GpuLanes>, dim3(1), dim3(64), lds, 0, A); break;
    case 1: hipLaunchKernelGGL(lane_prims_kernel<GpuLanes1>, dim3(1), dim3(64), lds, 0, A); break;
    case 2: hipLaunchKernelGGL(lane_prims_kernel<GpuLanesPmc1Plain>, dim3(1), dim3(64), lds, 0, A); break;
    case 3: hipLaunchKernelGGL(lane_prims_kernel<WithTurnMasksCmp<GpuLanes>>, dim3(1), dim3(64), lds, 0, A); break;
    case 4: hipLaunchKernelGGL(lane_prims_kernel<WithTurnMasksCmp<GpuLanesPmc1Plain>>, dim3(1), dim3(64), lds, 0, A); break;
    case 5: hipLaunchKernelGGL(lane_prims_kernel<WithConeInLds<GpuLanes1>>, dim3(1), dim3(64), lds, 0, A); break;
    case 6: hipLaunchKernelGGL(lane_prims_kernel<WithGramPipe<GpuLanesPmc1Plain>>, dim3(1), dim3(64), lds, 0, A); break;
    default: return -1;
  }
  return (int)hipGetLastError();
}
}

// math_helpers.hip -- TEST INFRASTRUCTURE.  Up to 64 one-wave workgroups (four 16-lane rows each) run ONE helper of pmc_math.hpp / Pmc<L> (math_helpers_body.hpp)
// under the GPU lane policies the step kernels are built with (llenv.hip), so that tests/test_gpu_math_helpers.py can hold each helper to its host twin and to
// the float64 statement (tests/math_helpers_ref.py).  Compiled with the product's flags.  Never linked into the product library.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../lifelike_agility_and_play_amd/csrc/pmc_step.hpp"
#include "math_helpers_body.hpp"

struct MhArgs {
  const float* in;       // [n_blocks * 4 rows][MH_IN_WORDS][16]
  float* out;            // [n_blocks * 4 rows][MH_OUT_WORDS][16]
  const double* auxd;    // [MH_AUXD_WORDS]
  const float* consts;   // legc [LC_COUNT][4] | candc [CAND_TABLE_WORDS][16] | basec [BC_COUNT] | 1.0f
  int helper, targ, active_rows;
};
struct GpuIO {
  const MhArgs& A;
  const long row;
  const int lane;
  const float one;
  __device__ GpuIO(const MhArgs& a) : A(a), row((long)blockIdx.x * 4 + ((threadIdx.x >> 4) & 3)), lane(threadIdx.x & 15), one(a.consts[MH_CONSTS_ONE]) {}
  __device__ float ld(int w) const { return A.in[(row * MH_IN_WORDS + w) * PMC_ROW + lane] * one; }
  __device__ float ldu(int w) const { return ld(w); }
  __device__ uint32_t raw(int w) const { return __builtin_bit_cast(uint32_t, A.in[(row * MH_IN_WORDS + w) * PMC_ROW + lane]); }
  __device__ void st(int w, float x) const { A.out[(row * MH_OUT_WORDS + w) * PMC_ROW + lane] = x; }
  __device__ void stu(int w, float x) const { st(w, x); }
  __device__ void straw(int w, uint32_t u) const { st(w, __builtin_bit_cast(float, u)); }
  __device__ const double* auxd() const { return A.auxd; }
  __device__ const float* legc() const { return A.consts + MH_CONSTS_LEGC; }
};

template <class L>
__global__ __launch_bounds__(64) void math_helpers_kernel(MhArgs A) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  L ln(lds);
  // every one of the 64 lanes stages the tables, as in the step kernels; rows outside `active_rows` leave before the helper, which then runs under a partial EXEC
  if constexpr (L::kHoldLink) ln.stage_consts(A.consts + MH_CONSTS_LEGC, LC_COUNT, A.consts + MH_CONSTS_CANDC, CAND_TABLE_WORDS, A.consts + MH_CONSTS_BASEC);
  else ln.stage_consts(A.consts + MH_CONSTS_LEGC, LC_COUNT, A.consts + MH_CONSTS_CANDC, CAND_TABLE_WORDS);
  if (!((A.active_rows >> (threadIdx.x >> 4)) & 1)) return;
  GpuIO io(A);
  if (A.helper < MH_SCALAR_END) run_scalar_helper<L>(io, A.helper);
  else run_lane_helper(ln, io, A.helper, A.targ);
}

typedef GpuLanesPinned<LC_COUNT> GpuLanes1;                                   // as llenv.hip
typedef GpuLanesPinned<LC_COUNT, 7, BC_COUNT, LK_BASE> GpuLanesPmc1Plain;     // as llenv.hip (LL_PIN_PMC)

static size_t mh_lds_bytes() { return ((size_t)LC_COUNT * 4 + (size_t)CAND_TABLE_WORDS * PMC_ROW + 4 * 12 + 4 * (size_t)PMC_ROW_SCRATCH) * sizeof(float); }

extern "C" {
// sizes of the buffers ll_math_helpers_run takes
void ll_math_helpers_dims(int* d) {
  d[0] = MH_IN_WORDS; d[1] = MH_OUT_WORDS; d[2] = MH_AUXD_WORDS; d[3] = MH_MAX_BLOCKS; d[4] = LC_COUNT; d[5] = CAND_TABLE_WORDS; d[6] = BC_COUNT; d[7] = MH_CONSTS_WORDS;
  d[8] = LK_BASE; d[9] = 3; /* policies */
}
// one launch of n_blocks one-wave workgroups on the null stream; the caller synchronises.  The buffer sizes are given in elements and checked against what the launch
// indexes.  Returns the HIP error of the launch (0: none), -1 for an unknown policy, -2 for arguments out of bounds.
int ll_math_helpers_run(int policy, int helper, int targ, int n_blocks, int active_rows, const float* in, long in_floats, float* out, long out_floats, const double* auxd,
                        long auxd_doubles, const float* consts, long consts_floats) {
  if (!mh_args_in_bounds(helper, targ, n_blocks, in_floats, out_floats, auxd_doubles, consts_floats)) return -2;
  MhArgs A{in, out, auxd, consts, helper, targ, active_rows & 15};
  const size_t lds = mh_lds_bytes();
  switch (policy) {
    case 0: hipLaunchKernelGGL(math_helpers_kernel<GpuLanes>, dim3(n_blocks), dim3(64), lds, 0, A); break;
    case 1: hipLaunchKernelGGL(math_helpers_kernel<GpuLanes1>, dim3(n_blocks), dim3(64), lds, 0, A); break;
    case 2: hipLaunchKernelGGL(math_helpers_kernel<GpuLanesPmc1Plain>, dim3(n_blocks), dim3(64), lds, 0, A); break;
    default: return -1;
  }
  return (int)hipGetLastError();
}
}

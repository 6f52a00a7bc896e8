// hl_score.inc -- the teacher-forced scorer of recorded unrolls (include/hl/llenv_hl_score.h).  Included after hl_league.inc: it reads the rows of
// hl_unroll.inc (HluRow) under the weights of an ll_hl_policy and runs the "fed" / on-chip-state modes of hl_policy.inc's device functions.
//
// One kernel of its own, hl_score_kernel: the geometry of hl_policy_pg_kernel (16 rows per workgroup, blockIdx.y 0 the policy chain, 1 the value
// chain, neither waiting on the other) with the unroll's time loop inside.  Time step t of row r lies t * row_floats behind the row's first frame and
// rows are unroll_length * row_floats apart, so the device functions see time step t as an observation buffer of that stride.  The LSTM state is
// loaded from S of the first frame into LDS (cs, hs), zeroed there where M says so, and never written to memory.
#include "../../include/hl/llenv_hl_score.h"

// The 16 columns of a scoring workgroup: rows row0 .. row0 + 15 of n_rows; the value of a row goes vs floats behind its neighbour's (srow: its
// only use with on-chip state).
struct HlScoreRows {
  int row0, n_rows;
  long vs;
  __device__ __forceinline__ int row(int m) const { return row0 + m; }
  __device__ __forceinline__ long srow(int m) const { return (long)(row0 + m) * vs; }
  __device__ __forceinline__ bool live(int m) const { return row0 + m < n_rows; }
};

// The thread's id as one time step sees it: the value is threadIdx.x, but the compiler is not told so (the step kernels' step loops do the same with
// their env).  Every address of the step's loads and stores derives from it, and none of those hundreds is carried across the time loop in a register:
// without this the kernel keeps them all and spills (256 registers and 3.3 KB of scratch per lane against the PG kernel's 111 and 68 B).  The mask
// restates the range of threadIdx.x: the shared device functions are compiled knowing the range of their wave / lane / tid arguments over ALL their
// callers, and without it the other policy kernels' machine code changes (v_min_i32 for v_min_u32 in pol_dense).
__device__ __forceinline__ int hl_score_step_tid(int tid) {
  asm volatile("" : "+v"(tid));
  return tid & (POL_THREADS - 1);
}

// Waves per SIMD the register budget is cut for, by A/B on the three cases of tools/hl_score_cost.py.  The compiler carries values across the time loop:
// left at two waves (256 registers) EPMC takes 244 and SEPMC 256 with 364 B of scratch, and one workgroup fits a CU where the PG kernel has two; at
// the PG kernel's four (128 registers) two fit and 292 B / 1088 B go to scratch.  EPMC 4096 rows: 20.1 ms at two, 18.9 ms at four; SEPMC 4096 rows
// 33.4 / 38.2 ms, the league's 2048 rows 23.2 / 31.0 ms.  So four for EPMC, two for SEPMC.
template <int KIND>
__global__ __launch_bounds__(POL_THREADS, KIND == LLH_EPMC ? 4 : 2) void hl_score_kernel(HlW W, const float* __restrict__ rows, int n_rows, int L, float* __restrict__ out) {
  typedef HluRow<KIND> Y;
  constexpr int NH = Y::NH, V_COL = 2 * NH;
  static_assert(V_COL < LLS_OUT_FLOATS, "neglogp | entropy | V fit an output row");
  __shared__ HlPgLds S;
  __shared__ float hcs[KIND == LLH_SEPMC ? 32 * POL_M : 1], hhs[KIND == LLH_SEPMC ? 32 * POL_M : 1];      // SEPMC's high-level LSTM
  const int tid = threadIdx.x;
  const int stride = L * Y::RF;
  const HlScoreRows R = {(int)blockIdx.x * POL_M, n_rows, (long)L * LLS_OUT_FLOATS};
  // this thread's (row, unit) of every LSTM, as hl_lstm has it; the trip count of the time loops is the workgroup's, so every barrier inside is met
  const int m = tid >> 5, j = tid & 31, sj = j * POL_M + m;
  const bool live = R.live(m);
  const float* row = rows + (long)(live ? R.row(m) : 0) * stride;
  if (blockIdx.y == 1) {
    HlVLds& V = S.u.V;
    V.cs[sj] = live ? row[Y::S_OFF + j] : 0.0f;
    V.hs[sj] = live ? row[Y::S_OFF + 32 + j] : 0.0f;
    for (int t = 0; t < L; t++) {
      const int id = hl_score_step_tid(tid), wave = id >> 6, lane = id & 63;
      if (t > 0 && live && row[(long)t * Y::RF + Y::M_OFF] != 0.0f) { V.cs[sj] = 0.0f; V.hs[sj] = 0.0f; }
      hl_value<KIND, true>(W, V, rows + (long)t * Y::RF, stride, nullptr, nullptr, out + (long)t * LLS_OUT_FLOATS + V_COL, R, wave, lane, id);
    }
    return;
  }
  HlLds& P = S.u.P;
  HlFed f;
  f.astride = stride; f.ostride = R.vs; f.hcs = hcs; f.hhs = hhs;
  P.cs[sj] = live ? row[Y::S_OFF + 128 + j] : 0.0f;
  P.hs[sj] = live ? row[Y::S_OFF + 160 + j] : 0.0f;
  if constexpr (KIND == LLH_SEPMC) {
    hcs[sj] = live ? row[Y::S_OFF + 192 + j] : 0.0f;
    hhs[sj] = live ? row[Y::S_OFF + 224 + j] : 0.0f;
  }
  for (int t = 0; t < L; t++) {
    const int id = hl_score_step_tid(tid), wave = id >> 6, lane = id & 63;
    if (t > 0 && live && row[(long)t * Y::RF + Y::M_OFF] != 0.0f) {
      P.cs[sj] = 0.0f; P.hs[sj] = 0.0f;
      if constexpr (KIND == LLH_SEPMC) { hcs[sj] = 0.0f; hhs[sj] = 0.0f; }
    }
    f.a = rows + (long)t * Y::RF + Y::A_OFF;
    f.out = out + (long)t * LLS_OUT_FLOATS;
    if (id < POL_M && R.live(id))
      for (int c = V_COL + 1; c < LLS_OUT_FLOATS; c++) f.out[(long)R.row(id) * f.ostride + c] = 0.0f;
    hl_pg_policy<KIND, true>(W, R, S, rows + (long)t * Y::RF, stride, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, wave, lane, id, f);
  }
}

static void hls_layout(int kind, ll_hl_score_layout_t* o) {
  const int nh = kind == LLH_EPMC ? LLH_EPMC_N_HEADS : LLH_SEPMC_N_HEADS;
  memset(o, 0, sizeof *o);
  o->kind = kind; o->n_heads = nh; o->out_floats = LLS_OUT_FLOATS;
  o->off[LLS_NEGLOGP] = 0; o->dim[LLS_NEGLOGP] = nh;
  o->off[LLS_ENTROPY] = nh; o->dim[LLS_ENTROPY] = nh;
  o->off[LLS_V] = 2 * nh; o->dim[LLS_V] = 1;
  o->off[LLS_PAD] = 2 * nh + 1; o->dim[LLS_PAD] = LLS_OUT_FLOATS - (2 * nh + 1);
}

// the argument checks of every scoring call (before the device is touched), then the launch
static void hls_launch(ll_hl_policy* w, const float* d_rows, int n_rows, int L, float* d_out, hipStream_t st) {
  LL_CHECK(w && d_rows && d_out, "null argument");
  LL_CHECK(n_rows > 0 && L > 0, "n_rows and unroll_length must be positive");
  const int rf = w->kind == LLH_EPMC ? LLU_EPMC_ROW_FLOATS : LLU_SEPMC_ROW_FLOATS;
  LL_CHECK((long long)L * rf <= 0x7FFFFFFFll, "unroll_length: a row's unroll must stay below 2^31 floats");
  LL_CHECK(w->d_vw, "the weight carrier has no value branch attached (ll_hl_policy_attach_value): scoring needs V");
  HIPCHK(hipSetDevice(w->device));
  const dim3 grid((n_rows + POL_M - 1) / POL_M, 2), block(POL_THREADS);
  if (w->kind == LLH_EPMC)
    hipLaunchKernelGGL(hl_score_kernel<LLH_EPMC>, grid, block, 0, st, w->W, d_rows, n_rows, L, d_out);
  else
    hipLaunchKernelGGL(hl_score_kernel<LLH_SEPMC>, grid, block, 0, st, w->W, d_rows, n_rows, L, d_out);
  HIPCHK(hipGetLastError());
}

// block `buffer` of ring r after `steps` recorded steps, on the engine's stream
static void hls_score_ring(ll_hl_policy* w, ENGINE* base, const HluRing* r, uint64_t steps, const char* who, int buffer, float* d_out) {
  LL_CHECK(w && d_out, "null argument");
  if (w->kind != r->kind)
    throw PmcError(LL_EINVAL, std::string(who) + (r->kind == LLH_EPMC ? ": the blocks are EPMC rows, the weight carrier is an LLH_SEPMC policy"
                                                                      : ": the blocks are SEPMC rows, the weight carrier is an LLH_EPMC policy"));
  LL_CHECK(w->device == base->bk.device, "the weight carrier and the engine live on different devices");
  LL_CHECK(buffer >= 0 && buffer < r->nbuf, "buffer index out of range");
  if (steps / (uint64_t)r->L <= (uint64_t)buffer)       // unroll k lives in block k % n_buffers: block b is first complete with unroll b
    throw PmcError(LL_ESTATE, std::string(who) + ": block " + std::to_string(buffer) + " holds no complete unroll yet");
  hls_launch(w, r->d_base + (size_t)buffer * r->n_rows * r->L * r->RF, r->n_rows, r->L, d_out, (hipStream_t)base->bk.stream_handle());
}

extern "C" {

int ll_hl_score_layout(int kind, ll_hl_score_layout_t* out) {
  LL_TRY
  LL_CHECK(out, "null argument");
  if (kind != LLH_EPMC && kind != LLH_SEPMC) throw PmcError(LL_EINVAL, "kind: LLH_EPMC (1) or LLH_SEPMC (2)");
  hls_layout(kind, out);
  LL_CATCH
}

int ll_hl_score_rows(ll_hl_policy* w, const float* d_rows, int n_rows, int unroll_length, float* d_out, void* hip_stream) {
  LL_TRY
  hls_launch(w, d_rows, n_rows, unroll_length, d_out, (hipStream_t)hip_stream);
  LL_CATCH
}

int ll_hl_score_unroll(ll_hl_policy* w, ll_hl_unroll* rec, int buffer, float* d_out) {
  LL_TRY
  LL_CHECK(rec, "null recorder");
  const HluRing ring = {rec->kind, rec->n_rows, rec->L, rec->nbuf, rec->RF, rec->d_base, rec->n_bytes};
  hls_score_ring(w, rec->base, &ring, rec->steps, "ll_hl_score_unroll", buffer, d_out);
  LL_CATCH
}

int ll_hl_score_league(ll_hl_policy* w, ll_hl_league* lg, int buffer, float* d_out) {
  LL_TRY
  LL_CHECK(lg, "null league");
  hls_score_ring(w, lg->base, &lg->ring, lg->steps, "ll_hl_score_league", buffer, d_out);
  LL_CATCH
}

}  // extern "C"

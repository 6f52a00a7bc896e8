// hl_league.inc -- the league actor of the SEPMC engine (include/hl/llenv_hl_league.h).  Included after hl_unroll.inc: it launches the row-mapped
// helpers of hl_policy.inc over a list of rows, and the record and TD(lambda) kernels of hl_unroll.inc over robot 0 of every arena.
//
// Two kernels of its own per step:
//   hl_league_plan_kernel   one workgroup: tally the episodes the last step ended under their opponent slot, draw the next opponent of those arenas,
//                           then a stable counting sort of the arenas by slot into a row list and a table of 16-row groups {slot, first, count}
//   hl_league_act_kernel    one launch for every row: learner groups (slot 0, rows 2 a), then the plan's opponent groups (rows 2 a + 1 through the row
//                           list, weights of the group's slot), then the learner groups' value branch.  The grid is the upper bound
//                           ceil(A / 16) + K of opponent groups; a workgroup beyond the plan's count returns at once.
#include "../../include/hl/llenv_hl_league.h"

#define HL_LEAGUE_SALT 0x1EA60Eu       // opponent draw: counter (arena, episode lo, episode hi, salt), word 0
#define HLG_PLAN_THREADS 1024
#define HLG_MAX_ARENAS 32768           // one plan workgroup: at most 32 arenas per thread
#define HLG_POL_FLOATS (LLH_SEPMC_N_FLOATS + 256)                  // a slot's policy arrays and the 256 zeros behind them (HlW::zero)
#define HLG_VF_OFF ((HLG_POL_FLOATS + 63) / 64 * 64)               // the learner's value branch starts 256-byte aligned, as its own allocation does
#define HLG_SLOT_FLOATS ((HLG_VF_OFF + LLH_SEPMC_VF_N_FLOATS + 63) / 64 * 64)

struct HlgPlan {
  int32_t* slot;                  // [A] the slot robot 1 of arena a acts with (0: not drawn yet)
  int64_t* episode;               // [A] episodes arena a has started
  unsigned long long* outcomes;   // [K][LLG_N_OUTCOMES]
  const float* cdf;               // [K]
  int32_t* rows;                  // [A] the rows 2 a + 1, sorted by slot, arenas ascending inside a slot
  int32_t* groups;                // [ceil(A / 16) + K][4]: slot, first (into rows), count, 0
  int32_t* n_groups;
  const uint8_t *done, *done_reason;
  int A, K;
};

// the slot u falls into: 1 + the first k with u < cdf[k].  u = ((w >> 8) + 0.5) 2^-24 in float32 rounds to 1 for the topmost word; cdf ends at
// exactly 1 from the last slot with a non-zero probability on, so that one u takes that slot.
__device__ __forceinline__ int hlg_slot_of(uint32_t w, const float* __restrict__ cdf, int K) {
  const float u = ((float)(w >> 8) + 0.5f) * 5.9604644775390625e-8f;
  int first_one = K - 1;
  for (int k = K - 1; k >= 0; k--)
    if (cdf[k] >= 1.0f) first_one = k;
  for (int k = 0; k < K; k++)
    if (u < cdf[k]) return 1 + k;
  return 1 + first_one;
}

__global__ __launch_bounds__(HLG_PLAN_THREADS) void hl_league_plan_kernel(HlgPlan p, uint64_t seed, int first_step) {
  __shared__ int cnt[LLG_MAX_OPPONENTS][HLG_PLAN_THREADS];       // per slot and thread: arenas of the thread's chunk; then their exclusive prefix
  __shared__ unsigned tally[LLG_MAX_OPPONENTS * LLG_N_OUTCOMES];
  __shared__ int total[LLG_MAX_OPPONENTS], base[LLG_MAX_OPPONENTS], gbase[LLG_MAX_OPPONENTS + 1];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int per = (p.A + HLG_PLAN_THREADS - 1) / HLG_PLAN_THREADS, a0 = tid * per, a1 = a0 + per < p.A ? a0 + per : p.A;
  if (tid < LLG_MAX_OPPONENTS * LLG_N_OUTCOMES) tally[tid] = 0u;
  __syncthreads();
  int c[LLG_MAX_OPPONENTS];
#pragma unroll
  for (int k = 0; k < LLG_MAX_OPPONENTS; k++) c[k] = 0;
  for (int a = a0; a < a1; a++) {
    int s = p.slot[a];
    if (first_step || p.done[2 * a]) {
      if (!first_step) {
        const unsigned why = p.done_reason[2 * a];
        unsigned* t = tally + (s - 1) * LLG_N_OUTCOMES;
        atomicAdd(t + 0, 1u);
        if (why & LLS_DONE_FALL) atomicAdd(t + 1, 1u);
        if (why & LLS_DONE_TIME) atomicAdd(t + 2, 1u);
        if (why & LLS_DONE_CATCH) atomicAdd(t + 3, 1u);
        if (why & LLS_DONE_NONFINITE) atomicAdd(t + 4, 1u);
      }
      const uint64_t ep = (uint64_t)p.episode[a];
      uint32_t w[4];
      philox4x32((uint32_t)a, (uint32_t)ep, (uint32_t)(ep >> 32), HL_LEAGUE_SALT, (uint32_t)seed, (uint32_t)(seed >> 32), w);
      s = hlg_slot_of(w[0], p.cdf, p.K);
      p.slot[a] = s;
      p.episode[a] = (int64_t)(ep + 1);
    }
#pragma unroll
    for (int k = 0; k < LLG_MAX_OPPONENTS; k++) c[k] += (s - 1 == k) ? 1 : 0;
  }
#pragma unroll
  for (int k = 0; k < LLG_MAX_OPPONENTS; k++) cnt[k][tid] = c[k];
  __syncthreads();
  if (wave < p.K) {                                              // wavefront k: exclusive prefix of slot k's counts over the threads
    int run = 0;
    for (int i = 0; i < HLG_PLAN_THREADS; i += 64) {
      const int v = cnt[wave][i + lane];
      int x = v;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(x, o);
        if (lane >= o) x += t;
      }
      cnt[wave][i + lane] = run + x - v;
      run += __shfl(x, 63);
    }
    if (lane == 0) total[wave] = run;
  }
  __syncthreads();
  if (tid == 0) {
    int b = 0, g = 0;
    for (int k = 0; k < p.K; k++) {
      base[k] = b; gbase[k] = g;
      b += total[k]; g += (total[k] + POL_M - 1) / POL_M;
    }
    gbase[p.K] = g;
    *p.n_groups = g;
  }
  __syncthreads();
  for (int k = 0; k < p.K; k++) {
    const int ng = gbase[k + 1] - gbase[k];
    for (int i = tid; i < ng; i += HLG_PLAN_THREADS) {
      int32_t* g = p.groups + 4 * (gbase[k] + i);
      const int left = total[k] - POL_M * i;
      g[0] = k + 1; g[1] = base[k] + POL_M * i; g[2] = left < POL_M ? left : POL_M; g[3] = 0;
    }
  }
  int pos[LLG_MAX_OPPONENTS];
#pragma unroll
  for (int k = 0; k < LLG_MAX_OPPONENTS; k++) pos[k] = k < p.K ? base[k] + cnt[k][tid] : 0;
  for (int a = a0; a < a1; a++) {
    const int s = p.slot[a];
#pragma unroll
    for (int k = 0; k < LLG_MAX_OPPONENTS; k++)
      if (s - 1 == k) p.rows[pos[k]++] = 2 * a + 1;
  }
  if (tid < p.K * LLG_N_OUTCOMES && tally[tid]) p.outcomes[tid] += tally[tid];
}

// HlW of slot 0 seen from another slot: every array `off` floats further on (one allocation [K + 1][HLG_SLOT_FLOATS])
struct HlWSlot {
  struct Arrays {
    const HlW* w;
    size_t off;
    __device__ __forceinline__ const float* operator[](int k) const { return w->a[k] + off; }
  } a;
  const float* zero;
};

// 16 rows through a list in LDS (-1: no row in that column); shift 1: the state and value of row 2 a live at a
struct HlList {
  const int* rows;
  int shift;
  __device__ __forceinline__ int row(int m) const { return rows[m]; }
  __device__ __forceinline__ int srow(int m) const { return rows[m] >> shift; }
  __device__ __forceinline__ bool live(int m) const { return rows[m] >= 0; }
};

__global__ __launch_bounds__(POL_THREADS) void hl_league_act_kernel(HlW W, const int32_t* __restrict__ rows, const int32_t* __restrict__ groups,
                                                                    const int32_t* __restrict__ n_groups, int A, int n_lg, int n_og, const float* __restrict__ obs,
                                                                    int stride, const uint8_t* __restrict__ reset, float* __restrict__ state, float* __restrict__ vstate,
                                                                    float* __restrict__ actions, int32_t* __restrict__ code_out, float* __restrict__ heading_out,
                                                                    float* __restrict__ neglogp, float* __restrict__ value, uint64_t seed, uint64_t step, int sample) {
  __shared__ HlPgLds S;
  __shared__ int lrow[POL_M];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  int b = blockIdx.x, slot = 0;
  const bool val = b >= n_lg + n_og;
  if (b < n_lg || val) {                                         // the learner: robot 0 of arenas 16 b .. 16 b + 15
    if (val) b -= n_lg + n_og;
    if (tid < POL_M) lrow[tid] = b * POL_M + tid < A ? 2 * (b * POL_M + tid) : -1;
  } else {
    const int g = b - n_lg;
    if (g >= *n_groups) return;
    slot = __builtin_amdgcn_readfirstlane(groups[4 * g]);
    const int first = groups[4 * g + 1], count = groups[4 * g + 2];
    if (tid < POL_M) lrow[tid] = tid < count ? rows[first + tid] : -1;
  }
  __syncthreads();
  HlWSlot Ws;
  Ws.a.w = &W; Ws.a.off = (size_t)slot * HLG_SLOT_FLOATS; Ws.zero = W.zero;
  const HlList R = {lrow, val ? 1 : 0};
  if (val) {
    hl_value<LLH_SEPMC>(Ws, S.u.V, obs, stride, reset, vstate, value, R, wave, lane, tid);
    return;
  }
  const bool me = slot == 0;                                     // the opponents' code, heading and neglogp go nowhere
  hl_pg_policy<LLH_SEPMC>(Ws, R, S, obs, stride, reset, state, actions, me ? code_out : nullptr, me ? heading_out : nullptr, me ? neglogp : nullptr, seed, step,
                          sample, wave, lane, tid);
}

struct ll_hl_league {
  int device, A, K, L, nbuf;
  ll_sepmc_engine* se;
  ENGINE* base;
  float* d_w;                      // [K + 1][HLG_SLOT_FLOATS]: policy arrays | 256 zeros | (slot 0) value branch
  HlW W;                           // slot 0's arrays
  float *d_state, *d_vstate;       // [2 A][128], [A][64]
  HluRing ring;                    // [nbuf][A][L][1244]
  float *d_neglogp, *d_value, *d_heading;     // what the act launch leaves for the recorder: [2 A][3], [A], [2 A] (the learner's rows are written)
  int32_t* d_code;                 // [2 A]
  HlgPlan plan;
  float* d_cdf;
  uint8_t* d_nodone;               // [2 A] zeros: the done buffer of ll_hl_league_plan_only
  std::vector<void*> dev;          // every device allocation
  float* h_stage[LLG_MAX_OPPONENTS + 1];      // pinned, one per slot, made at its first ll_hl_league_set_weights
  hipEvent_t ev[LLG_MAX_OPPONENTS + 1];       // the slot's last upload
  bool pending[LLG_MAX_OPPONENTS + 1], have_w[LLG_MAX_OPPONENTS + 1];
  float* h_cdf;                    // pinned [K]
  hipEvent_t cdf_ev;
  bool cdf_pending;
  double probs[LLG_MAX_OPPONENTS];
  uint64_t steps;
};

static void hlg_free(ll_hl_league* g) {
  (void)hipSetDevice(g->device);
  (void)hipDeviceSynchronize();            // a launch or an upload in flight still uses the buffers
  for (void* d : g->dev) (void)hipFree(d);
  for (int s = 0; s <= LLG_MAX_OPPONENTS; s++) {
    if (g->h_stage[s]) (void)hipHostFree(g->h_stage[s]);
    if (g->ev[s]) (void)hipEventDestroy(g->ev[s]);
  }
  if (g->h_cdf) (void)hipHostFree(g->h_cdf);
  if (g->cdf_ev) (void)hipEventDestroy(g->cdf_ev);
  delete g;
}

template <class T>
static T* hlg_alloc(ll_hl_league* g, size_t n, const char* what) {
  void* d = nullptr;
  if (hipMalloc(&d, n * sizeof(T)) != hipSuccess) {
    (void)hipGetLastError();
    throw PmcError(LL_ENOMEM, std::string("hipMalloc of ") + what + " failed: " + std::to_string(n * sizeof(T)) + " bytes");
  }
  g->dev.push_back(d);
  HIPCHK(hipMemset(d, 0, n * sizeof(T)));
  return static_cast<T*>(d);
}

// cdf[k]: the float32 running sum of the probabilities, exactly 1 from the last non-zero probability on
static void hlg_cdf(const double* probs, int K, float* cdf) {
  float run = 0.0f;
  int last = 0;
  for (int k = 0; k < K; k++)
    if (probs[k] > 0.0) last = k;
  for (int k = 0; k < K; k++) {
    run += (float)probs[k];
    cdf[k] = k >= last ? 1.0f : run;
  }
}

static void hlg_launch_record(ll_hl_league* g, hipStream_t st, int64_t post_step, int64_t pre_step) {
  HluArgs a;
  const StepParams& P = g->base->P;
  a.base = g->ring.d_base; a.obs = P.obs; a.reward = P.reward; a.actions = g->base->d_actions; a.done = P.done;
  a.state = g->d_state; a.vstate = g->d_vstate;
  a.neglogp = g->d_neglogp; a.value = g->d_value; a.heading = g->d_heading; a.code = g->d_code;
  a.n_rows = g->A; a.L = g->L;
  const int pob = post_step < 0 ? -1 : (int)((post_step / g->L) % g->nbuf), pos = post_step < 0 ? -1 : (int)(post_step % g->L);
  const int prb = pre_step < 0 ? -1 : (int)((pre_step / g->L) % g->nbuf), prs = pre_step < 0 ? -1 : (int)(pre_step % g->L);
  hipLaunchKernelGGL((hl_unroll_record_kernel<LLH_SEPMC, 2>), dim3((g->A + HLU_ROWS - 1) / HLU_ROWS), dim3(HLU_THREADS), 0, st, a, pob, pos, prb, prs);
  HIPCHK(hipGetLastError());
}

extern "C" {

int ll_hl_league_create(ll_sepmc_engine* e, int n_opponents, int unroll_length, int n_buffers, ll_hl_league** out) {
  LL_TRY
  LL_CHECK(out, "null argument");
  *out = nullptr;
  LL_CHECK(e, "null argument");
  LL_CHECK(n_opponents >= 1 && n_opponents <= LLG_MAX_OPPONENTS, "n_opponents must be 1 .. 8");
  LL_CHECK(unroll_length > 0 && n_buffers > 0, "unroll length and buffer count must be positive");
  ENGINE* base = &e->e->base;
  const int A = base->P.n_envs / 2, K = n_opponents;
  LL_CHECK(base->P.auto_reset, "the league actor needs an engine with auto_reset = 1: an arena's next episode starts inside the step that ends the last");
  LL_CHECK(A <= HLG_MAX_ARENAS, "the league actor plans at most 32768 arenas");
  LL_CHECK(base->P.obs_dim == LLH_SEPMC_OBS_DIM, "the engine's observation is not the policy's (965 columns)");
  int nd = 0;
  if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) throw PmcError(LL_ENODEV, "no HIP device available: the league actor has no CPU fallback");
  base->bk.use();
  ll_hl_league* g = new ll_hl_league();
  g->device = base->bk.device; g->A = A; g->K = K; g->L = unroll_length; g->nbuf = n_buffers; g->se = e; g->base = base; g->steps = 0;
  g->h_cdf = nullptr; g->cdf_ev = nullptr; g->cdf_pending = false;
  for (int s = 0; s <= LLG_MAX_OPPONENTS; s++) { g->h_stage[s] = nullptr; g->ev[s] = nullptr; g->pending[s] = false; g->have_w[s] = false; }
  try {
    g->ring.kind = LLH_SEPMC; g->ring.n_rows = A; g->ring.L = unroll_length; g->ring.nbuf = n_buffers; g->ring.RF = LLU_SEPMC_ROW_FLOATS;
    g->ring.n_bytes = (size_t)n_buffers * A * unroll_length * LLU_SEPMC_ROW_FLOATS * sizeof(float);
    g->ring.d_base = hlg_alloc<float>(g, g->ring.n_bytes / sizeof(float), "the unroll blocks");
    g->d_w = hlg_alloc<float>(g, (size_t)(K + 1) * HLG_SLOT_FLOATS, "the slots' weights");
    g->d_state = hlg_alloc<float>(g, (size_t)2 * A * 128, "the policy state");
    g->d_vstate = hlg_alloc<float>(g, (size_t)A * 64, "the value state");
    g->d_neglogp = hlg_alloc<float>(g, (size_t)2 * A * LLH_SEPMC_N_HEADS, "the act outputs");
    g->d_value = hlg_alloc<float>(g, (size_t)A, "the act outputs");
    g->d_heading = hlg_alloc<float>(g, (size_t)2 * A, "the act outputs");
    g->d_code = hlg_alloc<int32_t>(g, (size_t)2 * A, "the act outputs");
    g->d_cdf = hlg_alloc<float>(g, (size_t)K, "the plan");
    g->d_nodone = hlg_alloc<uint8_t>(g, (size_t)2 * A, "the plan");
    HlgPlan& p = g->plan;
    p.slot = hlg_alloc<int32_t>(g, (size_t)A, "the plan");
    p.episode = hlg_alloc<int64_t>(g, (size_t)A, "the plan");
    p.outcomes = hlg_alloc<unsigned long long>(g, (size_t)K * LLG_N_OUTCOMES, "the plan");
    p.rows = hlg_alloc<int32_t>(g, (size_t)A, "the plan");
    p.groups = hlg_alloc<int32_t>(g, (size_t)4 * ((A + POL_M - 1) / POL_M + K), "the plan");
    p.n_groups = hlg_alloc<int32_t>(g, 1, "the plan");
    p.cdf = g->d_cdf; p.done = base->P.done; p.done_reason = base->P.done_reason; p.A = A; p.K = K;
    if (hipHostMalloc((void**)&g->h_cdf, (size_t)K * sizeof(float), hipHostMallocDefault) != hipSuccess) {
      g->h_cdf = nullptr;
      throw PmcError(LL_ENOMEM, "hipHostMalloc failed");
    }
    HIPCHK(hipEventCreateWithFlags(&g->cdf_ev, hipEventDisableTiming));
    for (int k = 0; k < K; k++) g->probs[k] = 1.0 / K;                         // until ll_hl_league_set_probs: every opponent alike
    hlg_cdf(g->probs, K, g->h_cdf);
    HIPCHK(hipMemcpy(g->d_cdf, g->h_cdf, (size_t)K * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipDeviceSynchronize());
  } catch (...) {
    hlg_free(g);
    throw;
  }
  // slot 0's arrays in the packing of ll_hl_policy_create (0, 1, 51..151) and ll_hl_policy_attach_value (2..50)
  for (int i = 0; i < HL_MAX_ARRAY; i++) g->W.a[i] = nullptr;
  size_t off = 0;
  g->W.a[0] = g->d_w; g->W.a[1] = g->d_w + 135; off = 270;
  for (int i = 0; i < 46; i++) { g->W.a[51 + i] = g->d_w + off; off += (size_t)HL_HLC_SIZES[i]; }
  for (int i = 0; i < 55; i++) { g->W.a[97 + i] = g->d_w + off; off += (size_t)HL_MID_SIZES[i]; }
  g->W.zero = g->d_w + LLH_SEPMC_N_FLOATS;
  size_t voff = HLG_VF_OFF;
  for (int i = 0; i < 49; i++) { g->W.a[2 + i] = g->d_w + voff; voff += (size_t)HL_VF_SEPMC_SIZES[i]; }
  if (off != (size_t)LLH_SEPMC_N_FLOATS || voff != (size_t)HLG_VF_OFF + LLH_SEPMC_VF_N_FLOATS) {
    hlg_free(g);
    throw PmcError(LL_EINVAL, "internal: array size table");
  }
  *out = g;
  LL_CATCH
}

int ll_hl_league_destroy(ll_hl_league* g) {
  LL_TRY
  if (g) hlg_free(g);
  LL_CATCH
}

int ll_hl_league_set_weights(ll_hl_league* g, int slot, const float* h_weights, int n_floats, const float* h_vf_weights, int n_vf_floats) {
  LL_TRY
  LL_CHECK(g, "null league");
  LL_CHECK(h_weights, "null argument");
  LL_CHECK(slot >= 0 && slot <= g->K, "slot must be 0 (the learner) .. n_opponents");
  LL_CHECK(n_floats == LLH_SEPMC_N_FLOATS, "weights: expected arrays 0, 1, 51..151 of the SEPMC checkpoint (316806 floats)");
  if (slot == 0) {
    LL_CHECK(h_vf_weights, "h_vf_weights: slot 0 is the learner, its value branch comes with its policy");
    LL_CHECK(n_vf_floats == LLH_SEPMC_VF_N_FLOATS, "value weights: expected arrays 2..50 of the SEPMC checkpoint (182864 floats)");
  } else {
    LL_CHECK(!h_vf_weights, "h_vf_weights: an opponent slot has no value branch");
  }
  g->base->bk.use();
  hipStream_t st = (hipStream_t)g->base->bk.stream_handle();
  if (!g->h_stage[slot]) {
    const size_t n = slot == 0 ? (size_t)HLG_SLOT_FLOATS : (size_t)LLH_SEPMC_N_FLOATS;
    if (hipHostMalloc((void**)&g->h_stage[slot], n * sizeof(float), hipHostMallocDefault) != hipSuccess) {
      g->h_stage[slot] = nullptr;
      throw PmcError(LL_ENOMEM, "hipHostMalloc of the weight staging buffer failed");
    }
    HIPCHK(hipEventCreateWithFlags(&g->ev[slot], hipEventDisableTiming));
  }
  if (g->pending[slot]) HIPCHK(hipEventSynchronize(g->ev[slot]));            // the slot's staging buffer is free once its last upload has left it
  float* d = g->d_w + (size_t)slot * HLG_SLOT_FLOATS;
  memcpy(g->h_stage[slot], h_weights, (size_t)LLH_SEPMC_N_FLOATS * sizeof(float));
  HIPCHK(hipMemcpyAsync(d, g->h_stage[slot], (size_t)LLH_SEPMC_N_FLOATS * sizeof(float), hipMemcpyHostToDevice, st));
  if (slot == 0) {
    memcpy(g->h_stage[0] + HLG_VF_OFF, h_vf_weights, (size_t)LLH_SEPMC_VF_N_FLOATS * sizeof(float));
    HIPCHK(hipMemcpyAsync(d + HLG_VF_OFF, g->h_stage[0] + HLG_VF_OFF, (size_t)LLH_SEPMC_VF_N_FLOATS * sizeof(float), hipMemcpyHostToDevice, st));
  }
  HIPCHK(hipEventRecord(g->ev[slot], st));
  g->pending[slot] = true;
  g->have_w[slot] = true;
  LL_CATCH
}

int ll_hl_league_set_probs(ll_hl_league* g, const double* h_probs, int n) {
  LL_TRY
  LL_CHECK(g, "null league");
  LL_CHECK(h_probs, "null argument");
  LL_CHECK(n == g->K, "one probability per opponent slot");
  double sum = 0.0;
  for (int k = 0; k < n; k++) {
    LL_CHECK(h_probs[k] >= 0.0 && h_probs[k] <= 1.0 + 1e-6, "probabilities must lie in 0 .. 1");      // (a NaN fails the comparison)
    sum += h_probs[k];
  }
  LL_CHECK(sum >= 1.0 - 1e-6 && sum <= 1.0 + 1e-6, "probabilities must sum to 1 (within 1e-6)");
  g->base->bk.use();
  hipStream_t st = (hipStream_t)g->base->bk.stream_handle();
  if (g->cdf_pending) HIPCHK(hipEventSynchronize(g->cdf_ev));
  for (int k = 0; k < n; k++) g->probs[k] = h_probs[k];
  hlg_cdf(g->probs, n, g->h_cdf);
  HIPCHK(hipMemcpyAsync(g->d_cdf, g->h_cdf, (size_t)n * sizeof(float), hipMemcpyHostToDevice, st));
  HIPCHK(hipEventRecord(g->cdf_ev, st));
  g->cdf_pending = true;
  LL_CATCH
}

int ll_hl_league_steps(ll_hl_league* g, uint64_t seed, int sample, int n_steps) {
  LL_TRY
  LL_CHECK(g, "null league");
  LL_CHECK(n_steps > 0, "n_steps must be positive");
  if ((uint64_t)n_steps > (uint64_t)g->L * (uint64_t)g->nbuf)
    throw PmcError(LL_EINVAL, "ll_hl_league_steps: " + std::to_string(n_steps) + " steps do not fit the unroll ring of " + std::to_string(g->L) + " x " +
                                  std::to_string(g->nbuf) + " rows per arena");
  if (!g->se->e->have_reset) throw PmcError(LL_ESTATE, "the engine must be reset before ll_hl_league_steps");
  if (!g->have_w[0]) throw PmcError(LL_ESTATE, "slot 0 (the learner) has no weights: ll_hl_league_set_weights");
  for (int k = 0; k < g->K; k++)
    if (g->probs[k] > 0.0 && !g->have_w[k + 1])
      throw PmcError(LL_ESTATE, "opponent slot " + std::to_string(k + 1) + " can be drawn (probability " + std::to_string(g->probs[k]) + ") and has no weights");
  g->base->need_launchable(LL_ENGINE_SEPMC);
  g->base->bk.use();
  hipStream_t st = (hipStream_t)g->base->bk.stream_handle();
  const StepParams& P = g->base->P;
  const int n_lg = (g->A + POL_M - 1) / POL_M, n_og = n_lg + g->K;
  hlg_launch_record(g, st, -1, (int64_t)g->steps);
  for (int i = 0; i < n_steps; i++) {
    hipLaunchKernelGGL(hl_league_plan_kernel, dim3(1), dim3(HLG_PLAN_THREADS), 0, st, g->plan, seed, g->steps == 0 ? 1 : 0);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(hl_league_act_kernel, dim3(2 * n_lg + n_og), dim3(POL_THREADS), 0, st, g->W, g->plan.rows, g->plan.groups, g->plan.n_groups, g->A, n_lg, n_og,
                       P.obs, P.obs_dim, P.done, g->d_state, g->d_vstate, g->base->d_actions, g->d_code, g->d_heading, g->d_neglogp, g->d_value, seed, g->steps,
                       sample);
    HIPCHK(hipGetLastError());
    g->se->e->step(nullptr);
    hlg_launch_record(g, st, (int64_t)g->steps, i + 1 < n_steps ? (int64_t)g->steps + 1 : -1);
    g->steps += 1;
  }
  LL_CATCH
}

int ll_hl_league_plan_only(ll_hl_league* g, int n_launches) {
  LL_TRY
  LL_CHECK(g, "null league");
  LL_CHECK(n_launches > 0, "n_launches must be positive");
  if (g->steps == 0) throw PmcError(LL_ESTATE, "ll_hl_league_plan_only re-plans the arenas as they stand: run ll_hl_league_steps first");
  g->base->bk.use();
  hipStream_t st = (hipStream_t)g->base->bk.stream_handle();
  HlgPlan p = g->plan;
  p.done = g->d_nodone;                    // nobody finished: no tally, no draw, the same row list and group table written again
  for (int i = 0; i < n_launches; i++) hipLaunchKernelGGL(hl_league_plan_kernel, dim3(1), dim3(HLG_PLAN_THREADS), 0, st, p, (uint64_t)0, 0);
  HIPCHK(hipGetLastError());
  LL_CATCH
}

int ll_hl_league_position(ll_hl_league* g, int64_t* unroll_index, int* time_step) {
  LL_TRY
  LL_CHECK(g && unroll_index && time_step, "null argument");
  *unroll_index = (int64_t)(g->steps / (uint64_t)g->L);
  *time_step = (int)(g->steps % (uint64_t)g->L);
  LL_CATCH
}

int ll_hl_league_layout(ll_hl_league* g, ll_hl_unroll_layout_t* out) {
  LL_TRY
  LL_CHECK(g && out, "null argument");
  hlu_fill_layout(&g->ring, out);
  LL_CATCH
}

int ll_hl_league_finish(ll_hl_league* g, int buffer, float gamma, float lam, const float* d_bootstrap_value) {
  LL_TRY
  LL_CHECK(g, "null league");
  hlu_finish(g->base, &g->ring, g->steps, "ll_hl_league_finish", buffer, gamma, lam, d_bootstrap_value);
  LL_CATCH
}

int ll_hl_league_get_assignment(ll_hl_league* g, int32_t* h_slot, int64_t* h_episode) {
  LL_TRY
  LL_CHECK(g, "null league");
  g->base->bk.use();
  HIPCHK(hipDeviceSynchronize());
  if (h_slot) HIPCHK(hipMemcpy(h_slot, g->plan.slot, (size_t)g->A * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (h_episode) HIPCHK(hipMemcpy(h_episode, g->plan.episode, (size_t)g->A * sizeof(int64_t), hipMemcpyDeviceToHost));
  LL_CATCH
}

int ll_hl_league_get_outcomes(ll_hl_league* g, uint64_t* h_outcomes, int clear) {
  LL_TRY
  LL_CHECK(g, "null league");
  LL_CHECK(h_outcomes || clear, "null argument");
  g->base->bk.use();
  HIPCHK(hipDeviceSynchronize());
  const size_t bytes = (size_t)g->K * LLG_N_OUTCOMES * sizeof(uint64_t);
  if (h_outcomes) HIPCHK(hipMemcpy(h_outcomes, g->plan.outcomes, bytes, hipMemcpyDeviceToHost));
  if (clear) {
    HIPCHK(hipMemset(g->plan.outcomes, 0, bytes));
    HIPCHK(hipDeviceSynchronize());
  }
  LL_CATCH
}

int ll_hl_league_get_state(ll_hl_league* g, float* h_state, float* h_vstate) {
  LL_TRY
  LL_CHECK(g, "null league");
  g->base->bk.use();
  HIPCHK(hipDeviceSynchronize());
  if (h_state) HIPCHK(hipMemcpy(h_state, g->d_state, (size_t)2 * g->A * 128 * sizeof(float), hipMemcpyDeviceToHost));
  if (h_vstate) HIPCHK(hipMemcpy(h_vstate, g->d_vstate, (size_t)g->A * 64 * sizeof(float), hipMemcpyDeviceToHost));
  LL_CATCH
}

}  // extern "C"

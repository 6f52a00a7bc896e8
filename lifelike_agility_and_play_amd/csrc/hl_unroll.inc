// hl_unroll.inc -- the unroll recorder of the on-device EPMC / SEPMC actors (include/hl/llenv_hl_unroll.h).
// Included after epmc_capi.inc, sepmc_capi.inc and hl_policy.inc: it drives their engines and ll_hl_policy_act_pg and touches none of their kernels.
//
// Two kernels of its own, both pure streaming:
//   hl_unroll_record_kernel   one wave per row.  "pre" (before act_pg): X, S, M and the pad of the row the next step fills; "post" (after the
//                             step): A, neglogp, V, r, discount of the row that step filled.  The post of step t and the pre of step t + 1 read buffers
//                             nobody writes in between, so inside one ll_hl_unroll_steps call they share a launch.
//   hl_unroll_gae_kernel      ll_hl_unroll_finish: one thread per row walks its unroll backwards (pmc_gae_kernel's recursion).
#include "../../include/hl/llenv_hl_unroll.h"

#define HLU_THREADS 256
#define HLU_ROWS (HLU_THREADS / 64)      // rows per workgroup: one wave each

template <int KIND>
struct HluRow {
  static constexpr int OD = KIND == LLH_EPMC ? LLH_EPMC_OBS_DIM : LLH_SEPMC_OBS_DIM;
  static constexpr int NH = KIND == LLH_EPMC ? LLH_EPMC_N_HEADS : LLH_SEPMC_N_HEADS;
  static constexpr int A_DIM = KIND == LLH_EPMC ? 13 : 14;
  static constexpr int S_DIM = KIND == LLH_EPMC ? 192 : 256;
  static constexpr int A_OFF = OD, NL_OFF = A_OFF + A_DIM, R_OFF = NL_OFF + NH, V_OFF = R_OFF + 1, RW_OFF = V_OFF + 1, DC_OFF = RW_OFF + 1;
  static constexpr int S_OFF = DC_OFF + 1, M_OFF = S_OFF + S_DIM, PAD_OFF = M_OFF + 1;
  static constexpr int RF = (PAD_OFF + 3) / 4 * 4;
};
static_assert(HluRow<LLH_EPMC>::RF == LLU_EPMC_ROW_FLOATS && HluRow<LLH_SEPMC>::RF == LLU_SEPMC_ROW_FLOATS, "row size stated in llenv_hl_unroll.h");

struct HluArgs {
  float* base;                       // [n_buffers][n_rows][L][RF]
  const float *obs, *reward, *actions;
  const uint8_t* done;
  const float *state, *vstate;       // the policy's recurrent state [.][64 EPMC, 128 SEPMC] and value state [.][64]
  const float *neglogp, *value, *heading;
  const int32_t* code;
  int n_rows, L;
};

// column j of S for recorded row `row`, engine row `src`: vf c|h, pi (no LSTM: zeros), z c|h, and SEPMC's hlc c|h last
template <int KIND>
__device__ __forceinline__ float hlu_state_col(const HluArgs& a, int row, int src, int j) {
  if (j < 64) return a.vstate[(size_t)row * 64 + j];
  if (j < 128) return 0.0f;
  if (KIND == LLH_EPMC) return a.state[(size_t)src * 64 + (j - 128)];
  return j < 192 ? a.state[(size_t)src * 128 + 64 + (j - 128)] : a.state[(size_t)src * 128 + (j - 192)];
}

// post_slot / pre_slot: the time step inside post_buf / pre_buf, -1: that half of the launch is not wanted.  One wave per row; a lane issues every
// load of its share of the row before its first store, so a row costs one round of loads and one of stores.
// RSTEP: recorded row `row` is the engine's (and the policy's) row RSTEP * row; the value and its state are indexed by `row` itself.  1: every row
// (ll_hl_unroll); 2: robot 0 of every arena (hl_league.inc).
template <int KIND, int RSTEP = 1>
__global__ __launch_bounds__(HLU_THREADS) void hl_unroll_record_kernel(HluArgs a, int post_buf, int post_slot, int pre_buf, int pre_slot) {
  typedef HluRow<KIND> Y;
  const int lane = threadIdx.x & 63, row = blockIdx.x * HLU_ROWS + (threadIdx.x >> 6);
  if (row >= a.n_rows) return;
  const int src = row * RSTEP;
  const bool dn = a.done[src] != 0;
  if (post_slot >= 0) {
    float* dst = a.base + (((size_t)post_buf * a.n_rows + row) * a.L + post_slot) * Y::RF;
    const int k = lane;
    if (k < Y::A_DIM) {
      const int j = KIND == LLH_SEPMC ? k - 1 : k;                  // -1: the heading
      dst[Y::A_OFF + k] = j < 0 ? a.heading[src] : j == 0 ? (float)a.code[src] : a.actions[(size_t)src * 12 + (j - 1)];
    } else if (k < Y::A_DIM + Y::NH) {
      dst[Y::A_OFF + k] = a.neglogp[(size_t)src * Y::NH + (k - Y::A_DIM)];
    } else if (k == Y::A_DIM + Y::NH + 1) {                          // (R, one column before, is ll_hl_unroll_finish's)
      dst[Y::V_OFF] = a.value[row];
    } else if (k == Y::A_DIM + Y::NH + 2) {
      dst[Y::RW_OFF] = a.reward[src];
    } else if (k == Y::A_DIM + Y::NH + 3) {
      dst[Y::DC_OFF] = dn ? 0.0f : 1.0f;
    }
  }
  if (pre_slot >= 0) {
    float* dst = a.base + (((size_t)pre_buf * a.n_rows + row) * a.L + pre_slot) * Y::RF;        // 16-byte aligned: RF is a multiple of 4
    const float* x = a.obs + (size_t)src * Y::OD;
    // X in 16-byte stores; 16-byte loads where the source row is aligned too (every EPMC row, every fourth SEPMC row)
    constexpr int XQ = Y::OD / 4, NX = (XQ + 63) / 64;
    const bool aligned = (reinterpret_cast<uintptr_t>(x) & 15) == 0;
    float4 xv[NX];
#pragma unroll
    for (int i = 0; i < NX; i++) {
      const int q = lane + 64 * i;
      if (q < XQ) {
        if (aligned) xv[i] = *reinterpret_cast<const float4*>(x + 4 * q);
        else xv[i] = make_float4(x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3]);
      }
    }
    float xrest = 0.0f;
    if (lane < Y::OD % 4) xrest = x[XQ * 4 + lane];
    // S | M | pad: columns S_OFF .. RF - 1, scalars up to the next 16-byte boundary, 16-byte stores from there
    const float m = (dn && pre_slot > 0) ? 1.0f : 0.0f;
    auto col = [&](int c) -> float {
      const int j = c - Y::S_OFF;
      if (j < Y::S_DIM) return dn ? 0.0f : hlu_state_col<KIND>(a, row, src, j);
      return j == Y::S_DIM ? m : 0.0f;
    };
    constexpr int HEAD = (4 - Y::S_OFF % 4) % 4, Q0 = Y::S_OFF + HEAD, TQ = (Y::RF - Q0) / 4;
    static_assert((Y::RF - Q0) % 4 == 0 && Q0 % 4 == 0 && TQ <= 64, "tail of the row: whole quads, at most one per lane");
    float shead = 0.0f;
    if (lane < HEAD) shead = col(Y::S_OFF + lane);
    float4 tv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (lane < TQ) tv = make_float4(col(Q0 + 4 * lane), col(Q0 + 4 * lane + 1), col(Q0 + 4 * lane + 2), col(Q0 + 4 * lane + 3));
#pragma unroll
    for (int i = 0; i < NX; i++) {
      const int q = lane + 64 * i;
      if (q < XQ) *reinterpret_cast<float4*>(dst + 4 * q) = xv[i];
    }
    if (lane < Y::OD % 4) dst[XQ * 4 + lane] = xrest;
    if (lane < HEAD) dst[Y::S_OFF + lane] = shead;
    if (lane < TQ) *reinterpret_cast<float4*>(dst + Q0 + 4 * lane) = tv;
  }
}

// rows of one block: [n_rows][L][RF]; R | V | r | discount sit at r_off .. r_off + 3.  bootstrap[row * bstride]
__global__ void hl_unroll_gae_kernel(float* block, int n_rows, int L, int RF, int r_off, float gamma, float lam, const float* bootstrap, size_t bstride) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n_rows) return;
  float* rows = block + (size_t)row * L * RF;
  float adv = 0.0f, vnext = bootstrap[(size_t)row * bstride];
  for (int t = L - 1; t >= 0; t--) {
    float* r = rows + (size_t)t * RF + r_off;
    const float V = r[1], m = r[3];
    const float delta = r[2] + gamma * vnext * m - V;
    adv = delta + gamma * lam * m * adv;
    r[0] = adv + V;
    vnext = V;
  }
}

struct ll_hl_unroll {
  int kind, device, n_rows, L, nbuf, RF;
  ll_epmc_engine* ee;
  ll_sepmc_engine* se;
  ENGINE* base;                     // the engine's shared part: buffers, stream
  ll_hl_policy* pol;
  float* d_base;
  size_t n_bytes;
  float* d_out;                     // what act_pg writes for the recorder: neglogp [n_rows][n_heads] | value [n_rows] | heading [n_rows] | code [n_rows] (int32)
  float *d_neglogp, *d_value, *d_heading;
  int32_t* d_code;
  uint64_t steps;                   // control steps since create
};

// the ring [nbuf][n_rows][L][RF] of a recorder: what ll_hl_unroll and ll_hl_league (hl_league.inc) share
struct HluRing {
  int kind, n_rows, L, nbuf, RF;
  float* d_base;
  size_t n_bytes;
};

static void hlu_fill_layout(const HluRing* r, ll_hl_unroll_layout_t* o) {
  const bool ep = r->kind == LLH_EPMC;
  typedef HluRow<LLH_EPMC> E;
  typedef HluRow<LLH_SEPMC> S;
  memset(o, 0, sizeof *o);
  o->kind = r->kind; o->row_floats = r->RF; o->n_rows = r->n_rows; o->unroll_length = r->L; o->n_buffers = r->nbuf;
  const int off[LLU_N_FIELDS] = {0, ep ? E::A_OFF : S::A_OFF, ep ? E::NL_OFF : S::NL_OFF, ep ? E::R_OFF : S::R_OFF, ep ? E::V_OFF : S::V_OFF,
                                 ep ? E::RW_OFF : S::RW_OFF, ep ? E::DC_OFF : S::DC_OFF, ep ? E::S_OFF : S::S_OFF, ep ? E::M_OFF : S::M_OFF,
                                 ep ? E::PAD_OFF : S::PAD_OFF};
  const int dim[LLU_N_FIELDS] = {ep ? E::OD : S::OD, ep ? E::A_DIM : S::A_DIM, ep ? E::NH : S::NH, 1, 1, 1, 1, ep ? E::S_DIM : S::S_DIM, 1,
                                 ep ? E::RF - E::PAD_OFF : S::RF - S::PAD_OFF};
  for (int i = 0; i < LLU_N_FIELDS; i++) { o->off[i] = off[i]; o->dim[i] = dim[i]; }
  o->d_base = r->d_base; o->n_bytes = (uint64_t)r->n_bytes;
}

static int hlu_create(int kind, ll_epmc_engine* ee, ll_sepmc_engine* se, ll_hl_policy* p, int unroll_length, int n_buffers, ll_hl_unroll** out) {
  LL_TRY
  LL_CHECK(out, "null argument");
  *out = nullptr;
  LL_CHECK((ee || se) && p, "null argument");
  LL_CHECK(unroll_length > 0 && n_buffers > 0, "unroll length and buffer count must be positive");
  ENGINE* base = ee ? &ee->e->base : &se->e->base;
  const int n_rows = base->P.n_envs;
  if (p->kind != kind)
    throw PmcError(LL_EINVAL, kind == LLH_EPMC ? "the EPMC engine needs an LLH_EPMC policy" : "the SEPMC engine needs an LLH_SEPMC policy");
  LL_CHECK(p->d_vw, "the policy has no value branch attached (ll_hl_policy_attach_value): an unroll needs V");
  if (p->max_rows < n_rows)
    throw PmcError(LL_EINVAL, "the policy's max_rows (" + std::to_string(p->max_rows) + ") is smaller than the engine's row count (" + std::to_string(n_rows) + ")");
  LL_CHECK(p->device == base->bk.device, "the policy and the engine live on different devices");
  const int od = kind == LLH_EPMC ? LLH_EPMC_OBS_DIM : LLH_SEPMC_OBS_DIM, nh = kind == LLH_EPMC ? LLH_EPMC_N_HEADS : LLH_SEPMC_N_HEADS;
  LL_CHECK(base->P.obs_dim == od, "the engine's observation is not the policy's (916 EPMC, 965 SEPMC columns)");
  int nd = 0;
  if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) throw PmcError(LL_ENODEV, "no HIP device available: the unroll recorder has no CPU fallback");
  base->bk.use();
  ll_hl_unroll* r = new ll_hl_unroll();
  r->kind = kind; r->device = base->bk.device; r->n_rows = n_rows; r->L = unroll_length; r->nbuf = n_buffers;
  r->RF = kind == LLH_EPMC ? LLU_EPMC_ROW_FLOATS : LLU_SEPMC_ROW_FLOATS;
  r->ee = ee; r->se = se; r->base = base; r->pol = p; r->steps = 0; r->d_base = nullptr; r->d_out = nullptr;
  r->n_bytes = (size_t)n_buffers * n_rows * unroll_length * r->RF * sizeof(float);
  if (hipMalloc(&r->d_base, r->n_bytes) != hipSuccess) {
    (void)hipGetLastError();
    const size_t bytes = r->n_bytes;
    delete r;
    throw PmcError(LL_ENOMEM, "hipMalloc of the unroll blocks failed: " + std::to_string(bytes) + " bytes (" + std::to_string(n_buffers) + " x " + std::to_string(n_rows) +
                                  " rows x " + std::to_string(unroll_length) + " steps x " + std::to_string(r->RF) + " floats)");
  }
  if (hipMalloc(&r->d_out, (size_t)n_rows * (nh + 3) * sizeof(float)) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipFree(r->d_base);
    delete r;
    throw PmcError(LL_ENOMEM, "hipMalloc failed");
  }
  r->d_neglogp = r->d_out; r->d_value = r->d_out + (size_t)n_rows * nh; r->d_heading = r->d_value + n_rows;
  r->d_code = reinterpret_cast<int32_t*>(r->d_heading + n_rows);
  *out = r;
  LL_CATCH
}

static void hlu_launch_record(ll_hl_unroll* r, hipStream_t st, int64_t post_step, int64_t pre_step) {
  HluArgs a;
  const StepParams& P = r->base->P;
  a.base = r->d_base; a.obs = P.obs; a.reward = P.reward; a.actions = r->base->d_actions; a.done = P.done;
  a.state = r->pol->d_state; a.vstate = r->pol->d_vstate;
  a.neglogp = r->d_neglogp; a.value = r->d_value; a.heading = r->d_heading; a.code = r->d_code;
  a.n_rows = r->n_rows; a.L = r->L;
  const int pob = post_step < 0 ? -1 : (int)((post_step / r->L) % r->nbuf), pos = post_step < 0 ? -1 : (int)(post_step % r->L);
  const int prb = pre_step < 0 ? -1 : (int)((pre_step / r->L) % r->nbuf), prs = pre_step < 0 ? -1 : (int)(pre_step % r->L);
  const dim3 grid((r->n_rows + HLU_ROWS - 1) / HLU_ROWS), block(HLU_THREADS);
  if (r->kind == LLH_EPMC)
    hipLaunchKernelGGL(hl_unroll_record_kernel<LLH_EPMC>, grid, block, 0, st, a, pob, pos, prb, prs);
  else
    hipLaunchKernelGGL(hl_unroll_record_kernel<LLH_SEPMC>, grid, block, 0, st, a, pob, pos, prb, prs);
  HIPCHK(hipGetLastError());
}

// ll_hl_unroll_finish / ll_hl_league_finish on ring r after `steps` recorded steps, on the engine's stream
static void hlu_finish(ENGINE* base, const HluRing* r, uint64_t steps, const char* who, int buffer, float gamma, float lam, const float* d_bootstrap_value) {
  LL_CHECK(buffer >= 0 && buffer < r->nbuf, "buffer index out of range");
  const uint64_t L = (uint64_t)r->L;
  const float* boot = d_bootstrap_value;
  size_t bstride = 1;
  if (!boot) {
    // the newest complete unroll k of this block; its V_T is V of time step 0 of unroll k + 1, which the post-step record of step (k + 1) L writes
    const int64_t done_unrolls = (int64_t)(steps / L);
    int64_t k = done_unrolls - 1;
    while (k >= 0 && k % r->nbuf != buffer) k--;
    if (k < 0) throw PmcError(LL_ESTATE, std::string(who) + ": block " + std::to_string(buffer) + " holds no complete unroll yet; pass d_bootstrap_value to finish it anyway");
    if (steps < (uint64_t)(k + 1) * L + 1)
      throw PmcError(LL_ESTATE, std::string(who) + ": the first step of the next unroll, whose value bootstraps this one, has not run; step once more or pass "
                                "d_bootstrap_value");
    const int nb = (int)((k + 1) % r->nbuf);
    boot = r->d_base + (size_t)nb * r->n_rows * r->L * r->RF + (r->kind == LLH_EPMC ? HluRow<LLH_EPMC>::V_OFF : HluRow<LLH_SEPMC>::V_OFF);
    bstride = (size_t)r->L * r->RF;
  }
  base->bk.use();
  hipStream_t st = (hipStream_t)base->bk.stream_handle();
  hipLaunchKernelGGL(hl_unroll_gae_kernel, dim3((r->n_rows + 255) / 256), dim3(256), 0, st, r->d_base + (size_t)buffer * r->n_rows * r->L * r->RF, r->n_rows, r->L,
                     r->RF, r->kind == LLH_EPMC ? HluRow<LLH_EPMC>::R_OFF : HluRow<LLH_SEPMC>::R_OFF, gamma, lam, boot, bstride);
  HIPCHK(hipGetLastError());
}

extern "C" {

int ll_hl_unroll_create_epmc(ll_epmc_engine* e, ll_hl_policy* p, int unroll_length, int n_buffers, ll_hl_unroll** out) {
  return hlu_create(LLH_EPMC, e, nullptr, p, unroll_length, n_buffers, out);
}

int ll_hl_unroll_create_sepmc(ll_sepmc_engine* e, ll_hl_policy* p, int unroll_length, int n_buffers, ll_hl_unroll** out) {
  return hlu_create(LLH_SEPMC, nullptr, e, p, unroll_length, n_buffers, out);
}

int ll_hl_unroll_destroy(ll_hl_unroll* r) {
  LL_TRY
  if (r) {
    (void)hipSetDevice(r->device);
    (void)hipDeviceSynchronize();          // a record launch in flight still writes the blocks
    (void)hipFree(r->d_base);
    (void)hipFree(r->d_out);
    delete r;
  }
  LL_CATCH
}

int ll_hl_unroll_layout(ll_hl_unroll* r, ll_hl_unroll_layout_t* out) {
  LL_TRY
  LL_CHECK(r && out, "null argument");
  const HluRing ring = {r->kind, r->n_rows, r->L, r->nbuf, r->RF, r->d_base, r->n_bytes};
  hlu_fill_layout(&ring, out);
  LL_CATCH
}

int ll_hl_unroll_steps(ll_hl_unroll* r, uint64_t seed, int sample, int n_steps) {
  LL_TRY
  LL_CHECK(r, "null recorder");
  LL_CHECK(n_steps > 0, "n_steps must be positive");
  if ((uint64_t)n_steps > (uint64_t)r->L * (uint64_t)r->nbuf)
    throw PmcError(LL_EINVAL, "ll_hl_unroll_steps: " + std::to_string(n_steps) + " steps do not fit the unroll ring of " + std::to_string(r->L) + " x " +
                                  std::to_string(r->nbuf) + " rows per robot");
  if (!(r->ee ? r->ee->e->have_reset : r->se->e->have_reset)) throw PmcError(LL_ESTATE, "the engine must be reset before ll_hl_unroll_steps");
  r->base->need_launchable(r->kind == LLH_EPMC ? LL_ENGINE_EPMC : LL_ENGINE_SEPMC);
  r->base->bk.use();
  hipStream_t st = (hipStream_t)r->base->bk.stream_handle();
  const StepParams& P = r->base->P;
  hlu_launch_record(r, st, -1, (int64_t)r->steps);
  for (int i = 0; i < n_steps; i++) {
    const int rc = ll_hl_policy_act_pg(r->pol, P.obs, P.obs_dim, P.done, r->base->d_actions, r->d_code, r->kind == LLH_SEPMC ? r->d_heading : nullptr, r->d_neglogp,
                                       r->d_value, seed, r->steps, sample, r->n_rows, (void*)st);
    if (rc != 0) throw PmcError(rc, g_ll_err);
    if (r->ee) r->ee->e->step(nullptr);
    else r->se->e->step(nullptr);
    hlu_launch_record(r, st, (int64_t)r->steps, i + 1 < n_steps ? (int64_t)r->steps + 1 : -1);
    r->steps += 1;
  }
  LL_CATCH
}

int ll_hl_unroll_position(ll_hl_unroll* r, int64_t* unroll_index, int* time_step) {
  LL_TRY
  LL_CHECK(r && unroll_index && time_step, "null argument");
  *unroll_index = (int64_t)(r->steps / (uint64_t)r->L);
  *time_step = (int)(r->steps % (uint64_t)r->L);
  LL_CATCH
}

int ll_hl_unroll_finish(ll_hl_unroll* r, int buffer, float gamma, float lam, const float* d_bootstrap_value) {
  LL_TRY
  LL_CHECK(r, "null recorder");
  const HluRing ring = {r->kind, r->n_rows, r->L, r->nbuf, r->RF, r->d_base, r->n_bytes};
  hlu_finish(r->base, &ring, r->steps, "ll_hl_unroll_finish", buffer, gamma, lam, d_bootstrap_value);
  LL_CATCH
}

}  // extern "C"

// hl_loss.inc -- the PPO loss of a scored unroll block, its statistics and its gradient with respect to the scorer's output columns
// (include/hl/llenv_hl_loss.h).  Included after hl_score.inc: it reads the rows of hl_unroll.inc (HluRow) and the rows hl_score_kernel wrote, and calls
// none of hl_policy.inc's device functions.
//
// Everything is float64 from the float32 inputs; only the gradient is rounded to float32, once.  Kernels of its own, all streaming:
//   hl_loss_returns_kernel   LLL_PPO2 only: one lane per row walks its unroll backwards (as hl_unroll_gae_kernel) and leaves the lambda-returns of the
//                            scored V in d_work;
//   hl_loss_stats_kernel     sweep 1, one lane per sample: who is valid, and the sums the advantage statistics and the means need;
//   hl_loss_terms_kernel     sweep 2, one lane per sample: every workgroup first folds sweep 1's partials (the same order in each, so each gets the same
//                            bits), then the surrogate, value and entropy terms, the gradient row, and the sums of the statistics;
//   hl_loss_fold_kernel      one workgroup folds both sets of partials and writes d_stats.
// A sweep runs at most HLL_MAX_GROUPS workgroups (a lane strides over the samples), so there are at most that many partial rows and folding them inside
// every workgroup of sweep 2 stays cheap.  Sums go lane -> wave (cross-lane moves) -> workgroup (LDS) -> d_work, and the partial rows are added in
// index order by whoever reads them: no atomics, no ticket, and the same bits on every call.
#include "../../include/hl/llenv_hl_loss.h"

#define HLL_THREADS 256
#define HLL_WAVES (HLL_THREADS / 64)
#define HLL_MAX_GROUPS 1024              // workgroups of a sweep, and rows of partials in d_work; a fold pass takes HLL_THREADS of them
#define HLL_P1 7                         // sweep 1: W | sum w adv | sum w adv^2 | sum w R | sum w v | excluded by weight | excluded non-finite
#define HLL_P2 13                        // sweep 2: pg | value | entropy[3] | kl[3] | clip[3] | sum w (R - mean)^2 | sum w ((R - v) - mean)^2
#define HLL_MAX_LOG_RATIO 709.0          // above it exp() leaves float64
static_assert(LLS_OUT_FLOATS == 8, "a scored row is two 16-byte accesses");

struct HllArgs {
  const float *rows, *score, *weight;
  float* grad;
  double* stats;
  double *part1, *part2, *ret;           // d_work: [HLL_MAX_GROUPS][HLL_P1] | [HLL_MAX_GROUPS][HLL_P2] | [n_rows][L]
  long n_cells;                          // n_rows * L
  int n_rows, L, n_groups;
  int mode, merge, norm;
  double clip_lo, clip_hi;               // 1 - lower, 1 + upper
  double vf_clip, vf_coef, ent_coef, gamma, lam, adv_eps;
};

enum { HLL_VALID = 0, HLL_BAD_WEIGHT = 1, HLL_NONFINITE = 2, HLL_NO_SAMPLE = 3 };

template <int NH>
struct HllSample {
  double n[NH], e[NH], o[NH], v, R, vold, w, adv;
  int state;
};

// v[i] summed over the workgroup, in the fixed order lane tree -> waves 0 .. 3; the totals are lds[HLL_WAVES * NV + i].  lds: (HLL_WAVES + 1) * NV doubles.
template <int NV>
__device__ __forceinline__ void hll_block_sum(const double (&v)[NV], double* lds) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < NV; i++) {
    double x = v[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off);
    if (lane == 0) lds[wave * NV + i] = x;
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    double t = lds[threadIdx.x];
    for (int w = 1; w < HLL_WAVES; w++) t += lds[w * NV + threadIdx.x];
    lds[HLL_WAVES * NV + threadIdx.x] = t;
  }
  __syncthreads();
}

// n_groups rows of NV partials folded by the workgroup: thread i takes rows i, i + HLL_THREADS, .. in that order, then hll_block_sum
template <int NV>
__device__ __forceinline__ void hll_fold(const double* part, int n_groups, double* lds) {
  double acc[NV];
#pragma unroll
  for (int i = 0; i < NV; i++) acc[i] = 0.0;
  for (int p = threadIdx.x; p < n_groups; p += HLL_THREADS) {
#pragma unroll
    for (int i = 0; i < NV; i++) acc[i] += part[(size_t)p * NV + i];
  }
  hll_block_sum<NV>(acc, lds);
}

struct HllMoments {
  double W, adv_mean, adv_var, ret_mean, val_mean, n_bad_weight, n_nonfinite;
};

// sweep 1's partials folded: what sweep 2 needs before its first term, and what the last launch reports
__device__ __forceinline__ HllMoments hll_moments(const HllArgs& a, double* lds) {
#pragma clang fp contract(off)
  hll_fold<HLL_P1>(a.part1, a.n_groups, lds);
  const double* t = lds + HLL_WAVES * HLL_P1;
  HllMoments m = {t[0], 0.0, 0.0, 0.0, 0.0, t[5], t[6]};
  if (m.W > 0.0) {
    m.adv_mean = t[1] / m.W;
    const double var = t[2] / m.W - m.adv_mean * m.adv_mean;
    m.adv_var = var > 0.0 ? var : 0.0;
    m.ret_mean = t[3] / m.W;
    m.val_mean = t[4] / m.W;
  }
  return m;
}

// Sample s of the block (s = row * L + t: rows, scored rows and weights are dense) with its verdict.  Both sweeps decide through this one function.
template <int KIND>
__device__ __forceinline__ HllSample<HluRow<KIND>::NH> hll_load(const HllArgs& a, long s) {
#pragma clang fp contract(off)
  typedef HluRow<KIND> Y;
  constexpr int NH = Y::NH;
  HllSample<NH> x;
  x.state = HLL_NO_SAMPLE;
  x.w = 0.0;
  if (a.mode == LLL_PPO2 && s % a.L == a.L - 1) return x;                     // the bootstrap step
  // a weight counts when it is a positive normal float32 (a subnormal one reads as zero on this device)
  const float wf = a.weight ? a.weight[s] : 1.0f;
  const uint32_t wb = __float_as_uint(wf), we = (wb >> 23) & 0xFFu;
  if ((wb >> 31) != 0u || we == 0u || we == 0xFFu) {
    x.state = HLL_BAD_WEIGHT;
    return x;
  }
  x.w = (double)wf;
  const float4 s0 = *reinterpret_cast<const float4*>(a.score + (size_t)s * LLS_OUT_FLOATS);
  const float4 s1 = *reinterpret_cast<const float4*>(a.score + (size_t)s * LLS_OUT_FLOATS + 4);
  const float sc[LLS_OUT_FLOATS] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
  const float* row = a.rows + (size_t)s * Y::RF;
  bool fin = true;
#pragma unroll
  for (int h = 0; h < NH; h++) {
    x.n[h] = (double)sc[h];
    x.e[h] = (double)sc[NH + h];
    x.o[h] = (double)row[Y::NL_OFF + h];
    fin = fin && __builtin_isfinite(x.n[h]) && __builtin_isfinite(x.e[h]) && __builtin_isfinite(x.o[h]);
  }
  x.v = (double)sc[2 * NH];
  if (a.mode == LLL_PPO) {
    x.R = (double)row[Y::R_OFF];
    x.vold = (double)row[Y::V_OFF];
    x.adv = x.R - x.vold;
    fin = fin && __builtin_isfinite(x.vold);
  } else {
    x.R = a.ret[s];
    x.vold = 0.0;
    x.adv = x.R - x.v;
  }
  fin = fin && __builtin_isfinite(x.v) && __builtin_isfinite(x.R);
  if (a.merge) {
    double so = x.o[0], sn = x.n[0];
#pragma unroll
    for (int h = 1; h < NH; h++) { so += x.o[h]; sn += x.n[h]; }
    fin = fin && (so - sn <= HLL_MAX_LOG_RATIO);
  } else {
#pragma unroll
    for (int h = 0; h < NH; h++) fin = fin && (x.o[h] - x.n[h] <= HLL_MAX_LOG_RATIO);
  }
  x.state = fin ? HLL_VALID : HLL_NONFINITE;
  return x;
}

// LLL_PPO2: R_t of the scored V, one lane per row, time step L - 2 down to 0; a term with a zero coefficient is left out
template <int KIND>
__global__ __launch_bounds__(HLL_THREADS) void hl_loss_returns_kernel(HllArgs a) {
#pragma clang fp contract(off)
  typedef HluRow<KIND> Y;
  constexpr int V_COL = 2 * Y::NH;
  const int r = blockIdx.x * HLL_THREADS + threadIdx.x;
  if (r >= a.n_rows) return;
  const float* row = a.rows + (size_t)r * a.L * Y::RF;
  const float* sc = a.score + (size_t)r * a.L * LLS_OUT_FLOATS + V_COL;
  double* ret = a.ret + (size_t)r * a.L;
  double vn = (double)sc[(size_t)(a.L - 1) * LLS_OUT_FLOATS], Rn = 0.0;
  for (int t = a.L - 2; t >= 0; t--) {
    const double rw = (double)row[(size_t)t * Y::RF + Y::RW_OFF], gd = a.gamma * (double)row[(size_t)t * Y::RF + Y::DC_OFF];
    double R = rw;
    if (gd != 0.0) {
      const double boot = (t == a.L - 2 || a.lam == 0.0) ? vn : a.lam == 1.0 ? Rn : (1.0 - a.lam) * vn + a.lam * Rn;
      R = rw + gd * boot;
    }
    ret[t] = R;
    Rn = R;
    vn = (double)sc[(size_t)t * LLS_OUT_FLOATS];
  }
}

template <int KIND>
__global__ __launch_bounds__(HLL_THREADS) void hl_loss_stats_kernel(HllArgs a) {
#pragma clang fp contract(off)
  __shared__ double lds[(HLL_WAVES + 1) * HLL_P1];
  double acc[HLL_P1];
#pragma unroll
  for (int i = 0; i < HLL_P1; i++) acc[i] = 0.0;
  for (long s = (long)blockIdx.x * HLL_THREADS + threadIdx.x; s < a.n_cells; s += (long)gridDim.x * HLL_THREADS) {
    const auto x = hll_load<KIND>(a, s);
    if (x.state == HLL_VALID) {
      acc[0] += x.w;
      acc[1] += x.w * x.adv;
      acc[2] += x.w * (x.adv * x.adv);
      acc[3] += x.w * x.R;
      acc[4] += x.w * x.v;
    } else if (x.state == HLL_BAD_WEIGHT) {
      acc[5] += 1.0;
    } else if (x.state == HLL_NONFINITE) {
      acc[6] += 1.0;
    }
  }
  hll_block_sum<HLL_P1>(acc, lds);
  if (threadIdx.x < HLL_P1) a.part1[(size_t)blockIdx.x * HLL_P1 + threadIdx.x] = lds[HLL_WAVES * HLL_P1 + threadIdx.x];
}

// -a rho against -a clip(rho): the term, whether the clipped branch is the active one (a tie goes to the unclipped one), and rho
__device__ __forceinline__ double hll_surrogate(const HllArgs& a, double ah, double log_ratio, bool& clipped, double& rho) {
#pragma clang fp contract(off)
  rho = exp(log_ratio);
  const double u = -ah * rho, c = -ah * fmin(fmax(rho, a.clip_lo), a.clip_hi);
  clipped = c > u;
  return clipped ? c : u;
}

template <int KIND>
__global__ __launch_bounds__(HLL_THREADS) void hl_loss_terms_kernel(HllArgs a) {
#pragma clang fp contract(off)
  typedef HluRow<KIND> Y;
  constexpr int NH = Y::NH, V_COL = 2 * NH;
  __shared__ double lds1[(HLL_WAVES + 1) * HLL_P1], lds[(HLL_WAVES + 1) * HLL_P2];
  const HllMoments m = hll_moments(a, lds1);
  const double sd = sqrt(m.adv_var + a.adv_eps), dif_mean = m.ret_mean - m.val_mean;
  double acc[HLL_P2];
#pragma unroll
  for (int i = 0; i < HLL_P2; i++) acc[i] = 0.0;
  for (long s = (long)blockIdx.x * HLL_THREADS + threadIdx.x; s < a.n_cells; s += (long)gridDim.x * HLL_THREADS) {
    const auto x = hll_load<KIND>(a, s);
    float g[LLS_OUT_FLOATS];
#pragma unroll
    for (int c = 0; c < LLS_OUT_FLOATS; c++) g[c] = 0.0f;
    if (x.state == HLL_VALID) {
      const double q = x.w / m.W;
      const double ah = a.norm ? (x.adv - m.adv_mean) / sd : x.adv;
      double pg = 0.0;
      if (a.merge) {
        double so = x.o[0], sn = x.n[0];
#pragma unroll
        for (int h = 1; h < NH; h++) { so += x.o[h]; sn += x.n[h]; }
        bool clipped;
        double rho;
        pg = hll_surrogate(a, ah, so - sn, clipped, rho);
        const float gn = clipped ? 0.0f : (float)(ah * rho * q);
#pragma unroll
        for (int h = 0; h < NH; h++) g[h] = gn;
        acc[8] += clipped ? x.w : 0.0;
      } else {
#pragma unroll
        for (int h = 0; h < NH; h++) {
          bool clipped;
          double rho;
          pg += hll_surrogate(a, ah, x.o[h] - x.n[h], clipped, rho);
          g[h] = clipped ? 0.0f : (float)(ah * rho * q);
          acc[8 + h] += clipped ? x.w : 0.0;
        }
      }
      const double dv = x.v - x.R;
      double vterm = dv * dv, gv = dv;
      if (a.mode == LLL_PPO && a.vf_clip > 0.0) {
        const double d = x.v - x.vold, dc = x.vold + fmin(fmax(d, -a.vf_clip), a.vf_clip) - x.R, cterm = dc * dc;
        if (cterm > vterm) {
          vterm = cterm;
          gv = (d > -a.vf_clip && d < a.vf_clip) ? dc : 0.0;
        }
      }
      vterm *= 0.5;
      acc[0] += x.w * pg;
      acc[1] += x.w * vterm;
#pragma unroll
      for (int h = 0; h < NH; h++) {
        const double dn = x.n[h] - x.o[h];
        acc[2 + h] += x.w * x.e[h];
        acc[5 + h] += x.w * (0.5 * (dn * dn));
        g[NH + h] = (float)(-a.ent_coef * q);
      }
      g[V_COL] = (float)(a.vf_coef * gv * q);
      const double dr = x.R - m.ret_mean, dd = (x.R - x.v) - dif_mean;
      acc[11] += x.w * (dr * dr);
      acc[12] += x.w * (dd * dd);
    }
    float4* out = reinterpret_cast<float4*>(a.grad + (size_t)s * LLS_OUT_FLOATS);
    out[0] = make_float4(g[0], g[1], g[2], g[3]);
    out[1] = make_float4(g[4], g[5], g[6], g[7]);
  }
  hll_block_sum<HLL_P2>(acc, lds);
  if (threadIdx.x < HLL_P2) a.part2[(size_t)blockIdx.x * HLL_P2 + threadIdx.x] = lds[HLL_WAVES * HLL_P2 + threadIdx.x];
}

__global__ __launch_bounds__(HLL_THREADS) void hl_loss_fold_kernel(HllArgs a) {
#pragma clang fp contract(off)
  __shared__ double lds1[(HLL_WAVES + 1) * HLL_P1], lds[(HLL_WAVES + 1) * HLL_P2];
  const HllMoments m = hll_moments(a, lds1);
  hll_fold<HLL_P2>(a.part2, a.n_groups, lds);
  if (threadIdx.x != 0) return;
  const double* t = lds + HLL_WAVES * HLL_P2;
  double* o = a.stats;
  for (int i = 0; i < LLL_N_STATS; i++) o[i] = 0.0;
  o[LLL_N_EXCLUDED_WEIGHT] = m.n_bad_weight;
  o[LLL_N_EXCLUDED_NONFINITE] = m.n_nonfinite;
  if (!(m.W > 0.0)) return;
  o[LLL_W] = m.W;
  o[LLL_ADV_MEAN] = m.adv_mean;
  o[LLL_ADV_STD] = sqrt(m.adv_var);
  const double pg = t[0] / m.W, vl = t[1] / m.W;
  double ent = 0.0;
  for (int h = 0; h < 3; h++) {
    const double e = t[2 + h] / m.W;
    o[LLL_ENTROPY + h] = e;
    o[LLL_APPROX_KL + h] = t[5 + h] / m.W;
    o[LLL_CLIP_FRAC + h] = t[8 + h] / m.W;
    ent += e;
  }
  o[LLL_PG_LOSS] = pg;
  o[LLL_VALUE_LOSS] = vl;
  o[LLL_LOSS] = pg + a.vf_coef * vl - a.ent_coef * ent;
  o[LLL_RETURN_MEAN] = m.ret_mean;
  o[LLL_VALUE_MEAN] = m.val_mean;
  const double var_r = t[11] / m.W, var_d = t[12] / m.W;
  o[LLL_EXPLAINED_VARIANCE] = var_r > 0.0 ? 1.0 - var_d / var_r : 0.0;
}

static uint64_t hll_workspace_bytes(int n_rows, int L) {
  return sizeof(double) * ((uint64_t)HLL_MAX_GROUPS * (HLL_P1 + HLL_P2) + (uint64_t)n_rows * (uint64_t)L);
}

// every argument check of a loss call, before the device is touched
static void hll_check(int kind, const ll_hl_loss_config_t* cfg, const float* d_rows, int n_rows, int L, const float* d_score, float* d_grad, double* d_stats,
                      void* d_work, uint64_t work_bytes) {
  LL_CHECK(cfg && d_rows && d_score && d_grad && d_stats && d_work, "null argument");
  if (kind != LLH_EPMC && kind != LLH_SEPMC) throw PmcError(LL_EINVAL, "kind: LLH_EPMC (1) or LLH_SEPMC (2)");
  LL_CHECK(cfg->mode == LLL_PPO || cfg->mode == LLL_PPO2, "mode: LLL_PPO (0) or LLL_PPO2 (1)");
  LL_CHECK(n_rows > 0 && L > 0, "n_rows and unroll_length must be positive");
  LL_CHECK(cfg->mode != LLL_PPO2 || L >= 2, "LLL_PPO2 needs an unroll_length of at least 2: the last time step is the bootstrap value");
  LL_CHECK(std::isfinite(cfg->clip_range) && cfg->clip_range >= 0.0f, "clip_range must be finite and not negative");
  LL_CHECK(std::isfinite(cfg->vf_coef) && cfg->vf_coef >= 0.0f, "vf_coef must be finite and not negative");
  LL_CHECK(std::isfinite(cfg->adv_eps) && cfg->adv_eps >= 0.0f, "adv_eps must be finite and not negative");
  LL_CHECK(std::isfinite(cfg->clip_range_lower) && std::isfinite(cfg->vf_clip) && std::isfinite(cfg->ent_coef), "clip_range_lower, vf_clip and ent_coef must be finite");
  LL_CHECK(cfg->gamma >= 0.0f && cfg->gamma <= 1.0f && cfg->lam >= 0.0f && cfg->lam <= 1.0f, "gamma and lam must lie in [0, 1]");
  const int rf = kind == LLH_EPMC ? LLU_EPMC_ROW_FLOATS : LLU_SEPMC_ROW_FLOATS;
  LL_CHECK((long long)L * rf <= 0x7FFFFFFFll, "unroll_length: a row's unroll must stay below 2^31 floats");
  if (work_bytes < hll_workspace_bytes(n_rows, L))
    throw PmcError(LL_EINVAL, "work_bytes " + std::to_string(work_bytes) + " is below ll_hl_loss_workspace_bytes (" + std::to_string(hll_workspace_bytes(n_rows, L)) + ")");
  LL_CHECK((reinterpret_cast<uintptr_t>(d_score) & 15) == 0 && (reinterpret_cast<uintptr_t>(d_grad) & 15) == 0, "d_score and d_grad must be 16-byte aligned");
  LL_CHECK((reinterpret_cast<uintptr_t>(d_stats) & 7) == 0 && (reinterpret_cast<uintptr_t>(d_work) & 7) == 0, "d_stats and d_work must be 8-byte aligned");
}

template <int KIND>
static void hll_launch_kind(const HllArgs& a, hipStream_t st) {
  const dim3 block(HLL_THREADS), sweep(a.n_groups);
  if (a.mode == LLL_PPO2) hipLaunchKernelGGL(hl_loss_returns_kernel<KIND>, dim3((a.n_rows + HLL_THREADS - 1) / HLL_THREADS), block, 0, st, a);
  hipLaunchKernelGGL(hl_loss_stats_kernel<KIND>, sweep, block, 0, st, a);
  hipLaunchKernelGGL(hl_loss_terms_kernel<KIND>, sweep, block, 0, st, a);
  hipLaunchKernelGGL(hl_loss_fold_kernel, dim3(1), block, 0, st, a);
}

// checked arguments -> the three or four launches on st
static void hll_launch(int kind, const ll_hl_loss_config_t* cfg, const float* d_rows, int n_rows, int L, const float* d_score, const float* d_weight, float* d_grad,
                       double* d_stats, void* d_work, hipStream_t st) {
  HllArgs a;
  a.rows = d_rows; a.score = d_score; a.weight = d_weight; a.grad = d_grad; a.stats = d_stats;
  a.part1 = static_cast<double*>(d_work);
  a.part2 = a.part1 + (size_t)HLL_MAX_GROUPS * HLL_P1;
  a.ret = a.part2 + (size_t)HLL_MAX_GROUPS * HLL_P2;
  a.n_cells = (long)n_rows * L; a.n_rows = n_rows; a.L = L;
  const long groups = (a.n_cells + HLL_THREADS - 1) / HLL_THREADS;
  a.n_groups = (int)(groups < HLL_MAX_GROUPS ? groups : HLL_MAX_GROUPS);
  a.mode = cfg->mode; a.merge = cfg->merge_heads != 0; a.norm = cfg->adv_normalize != 0;
  a.clip_lo = 1.0 - (double)(cfg->clip_range_lower > 0.0f ? cfg->clip_range_lower : cfg->clip_range);
  a.clip_hi = 1.0 + (double)cfg->clip_range;
  a.vf_clip = (double)cfg->vf_clip; a.vf_coef = (double)cfg->vf_coef; a.ent_coef = (double)cfg->ent_coef;
  a.gamma = (double)cfg->gamma; a.lam = (double)cfg->lam; a.adv_eps = (double)cfg->adv_eps;
  if (kind == LLH_EPMC) hll_launch_kind<LLH_EPMC>(a, st);
  else hll_launch_kind<LLH_SEPMC>(a, st);
  HIPCHK(hipGetLastError());
}

// block `buffer` of ring r after `steps` recorded steps, on the engine's stream: the block arithmetic and the LL_ESTATE rule of hls_score_ring
static void hll_loss_ring(ENGINE* base, const HluRing* r, uint64_t steps, const char* who, int buffer, const ll_hl_loss_config_t* cfg, const float* d_score,
                          const float* d_weight, float* d_grad, double* d_stats, void* d_work, uint64_t work_bytes) {
  hll_check(r->kind, cfg, r->d_base, r->n_rows, r->L, d_score, d_grad, d_stats, d_work, work_bytes);
  LL_CHECK(buffer >= 0 && buffer < r->nbuf, "buffer index out of range");
  if (steps / (uint64_t)r->L <= (uint64_t)buffer)
    throw PmcError(LL_ESTATE, std::string(who) + ": block " + std::to_string(buffer) + " holds no complete unroll yet");
  const float* d_rows = r->d_base + (size_t)buffer * r->n_rows * r->L * r->RF;
  base->bk.use();
  hll_launch(r->kind, cfg, d_rows, r->n_rows, r->L, d_score, d_weight, d_grad, d_stats, d_work, (hipStream_t)base->bk.stream_handle());
}

extern "C" {

int ll_hl_loss_default_config(ll_hl_loss_config_t* cfg) {
  LL_TRY
  LL_CHECK(cfg, "null argument");
  memset(cfg, 0, sizeof *cfg);
  cfg->mode = LLL_PPO; cfg->merge_heads = 1; cfg->adv_normalize = 1;
  cfg->clip_range = 0.2f; cfg->clip_range_lower = 0.0f; cfg->vf_clip = 0.0f;
  cfg->vf_coef = 1.0f; cfg->ent_coef = 0.0f; cfg->gamma = 0.95f; cfg->lam = 0.95f; cfg->adv_eps = 1e-8f;
  LL_CATCH
}

int ll_hl_loss_workspace_bytes(int n_rows, int unroll_length, uint64_t* out) {
  LL_TRY
  LL_CHECK(out, "null argument");
  LL_CHECK(n_rows > 0 && unroll_length > 0, "n_rows and unroll_length must be positive");
  *out = hll_workspace_bytes(n_rows, unroll_length);
  LL_CATCH
}

int ll_hl_loss_rows(int kind, const ll_hl_loss_config_t* cfg, const float* d_rows, int n_rows, int unroll_length, const float* d_score, const float* d_weight,
                    float* d_grad, double* d_stats, void* d_work, uint64_t work_bytes, void* hip_stream) {
  LL_TRY
  hll_check(kind, cfg, d_rows, n_rows, unroll_length, d_score, d_grad, d_stats, d_work, work_bytes);
  int nd = 0;
  if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) {
    (void)hipGetLastError();
    throw PmcError(LL_ENODEV, "no HIP device available: the loss has no CPU path");
  }
  hll_launch(kind, cfg, d_rows, n_rows, unroll_length, d_score, d_weight, d_grad, d_stats, d_work, (hipStream_t)hip_stream);
  LL_CATCH
}

int ll_hl_loss_unroll(ll_hl_unroll* rec, int buffer, const ll_hl_loss_config_t* cfg, const float* d_score, const float* d_weight, float* d_grad, double* d_stats,
                      void* d_work, uint64_t work_bytes) {
  LL_TRY
  LL_CHECK(rec, "null recorder");
  const HluRing ring = {rec->kind, rec->n_rows, rec->L, rec->nbuf, rec->RF, rec->d_base, rec->n_bytes};
  hll_loss_ring(rec->base, &ring, rec->steps, "ll_hl_loss_unroll", buffer, cfg, d_score, d_weight, d_grad, d_stats, d_work, work_bytes);
  LL_CATCH
}

int ll_hl_loss_league(ll_hl_league* lg, int buffer, const ll_hl_loss_config_t* cfg, const float* d_score, const float* d_weight, float* d_grad, double* d_stats,
                      void* d_work, uint64_t work_bytes) {
  LL_TRY
  LL_CHECK(lg, "null league");
  hll_loss_ring(lg->base, &lg->ring, lg->steps, "ll_hl_loss_league", buffer, cfg, d_score, d_weight, d_grad, d_stats, d_work, work_bytes);
  LL_CATCH
}

}  // extern "C"

/*
 * llenv_hl_loss.h -- C ABI of the PPO loss of a scored EPMC / SEPMC unroll block: the loss, its statistics and its gradient with respect to the
 * eight output columns of llenv_hl_score.h, on the device.
 *
 * What the reference's learner does next with the scorer's numbers (epmc_net.py:278-418): from the fed neglogp, the entropies and vpred, the
 * recorded neglogp, R and V, and -- in the ppo2 form -- r and discount through lambda-returns of the NEW value, it builds pg_loss, value_loss and
 * the head entropies.  Here that is one call on a block of llenv_hl_unroll.h rows and the matching block of scored rows; d_grad is dloss / d(d_score),
 * the seed of a backward pass through the networks (which this library does not have).
 *
 * An assumption, stated as llenv.h states its own: the (absent) tpolicies package owns tp_losses.ppo_loss, ppo2_loss and multistep_forward_view;
 * the formulas below are this build's statement of them.  What epmc_net.py shows is followed as written: the per-head sum of ppo2, the [:-1] / [1:]
 * alignment, 0.5 square(R - vpred), the stop-gradients and the means over all samples.  tests/hl_loss_ref.py is the normative float64 statement.
 *
 * Samples.  LLL_PPO: every (row, t).  LLL_PPO2: t = 0 .. L - 2 of every row; time step L - 1 only supplies the bootstrap value, its d_grad row is zero.
 * Per sample, h = head in scorer order: new neglogp n_h, entropy e_h and v from d_score; old neglogp o_h, R, V_old, r and d = discount from the row.
 *   LLL_PPO    adv = R - V_old.  R is read as it stands: running ll_hl_unroll_finish / ll_hl_league_finish first is the caller's business.
 *   LLL_PPO2   per row, backwards: R_{L-2} = r + gamma d v_{L-1};  R_t = r_t + gamma d_t ((1 - lam) v_{t+1} + lam R_{t+1});  adv_t = R_t - v_t.
 *              A term whose coefficient is exactly zero is left out, not multiplied: gamma d_t = 0 gives R_t = r_t, lam = 0 leaves R_{t+1} out,
 *              lam = 1 leaves v_{t+1} out.  R and the v inside adv are constants for the gradient.
 *   adv_normalize   a = (adv - mean) / sqrt(var + adv_eps), weighted mean and population variance over the valid samples; otherwise a = adv.
 *              The statistics are constants for the gradient.
 *   surrogate  merge_heads: rho = exp(sum_h o_h - sum_h n_h), term = max(-a rho, -a clip(rho, 1 - lower, 1 + upper)); otherwise one rho_h =
 *              exp(o_h - n_h) and one such term per head, summed.  On a tie the unclipped branch is the active one.  d/dn_h = a rho (a rho_h) where
 *              the unclipped branch is active, 0 otherwise.
 *   value      LLL_PPO2, and LLL_PPO with vf_clip <= 0: 0.5 (v - R)^2, d/dv = v - R.  LLL_PPO with vf_clip > 0: 0.5 max((v - R)^2, (vc - R)^2),
 *              vc = V_old + clip(v - V_old, +-vf_clip); on a tie the unclipped branch is active; where the clipped branch is active d/dv =
 *              (vc - R) [v - V_old strictly inside +-vf_clip].
 *   loss       pg_loss, value_loss and entropy_h are weighted means over the valid samples, W = sum w;
 *              loss = pg_loss + vf_coef value_loss - ent_coef sum_h entropy_h.
 * d_grad holds dloss / d of the matching d_score column -- the neglogp columns, the entropy columns (-ent_coef w / W), the V column; pad columns are
 * zero -- and every entry carries its sample's w / W.
 *
 * Excluded samples.  By weight: a weight that is zero, negative or non-finite.  By value (only asked of a sample whose weight is good): any value the
 * sample uses is non-finite -- n_h, e_h, v, o_h, R as used (a ppo2 R that a NaN reached), V_old in LLL_PPO -- or a log ratio above 709 (rho would
 * not be a float64).  Both are counted, separately.  An excluded sample contributes to no statistic and its d_grad row is zero.  With no valid sample
 * every statistic is 0, the counts are right and d_grad is all zeros.  No NaN is ever written to d_stats or d_grad.
 *
 * Arithmetic is float64 from the float32 inputs: the per-sample terms, the ppo2 recursion and every sum; only d_grad is rounded to float32, once.
 * Sums are folded in a fixed order (lane, wave, workgroup, then the workgroups' partials in index order by the next launch): no floating-point
 * atomics, and two calls on the same inputs return the same bits.  A call is three launches (LLL_PPO) or four (LLL_PPO2), asynchronous: no host
 * synchronisation and no allocation inside.  d_rows and d_score are only read.
 *
 * Same conventions as llenv.h: 0 or a negative LL_E* code, ll_last_error() for the text.  Argument errors are LL_EINVAL and are checked before the
 * device is touched; there is no CPU path: LL_ENODEV without a HIP device.  These entry points add to the library and change no struct that crosses
 * it, so LL_ABI_VERSION stays as it is.
 */
#ifndef LLENV_HL_LOSS_H
#define LLENV_HL_LOSS_H

#include <stdint.h>

#include "llenv_hl_league.h"
#include "llenv_hl_score.h"
#include "llenv_hl_unroll.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LLL_PPO 0       /* epmc_net.py:292-306: recorded R and V, clipped surrogate */
#define LLL_PPO2 1      /* epmc_net.py:307-384: lambda-returns of the scored V over the first L-1 time steps */

/* d_stats: LLL_N_STATS float64.  Slots of a head the kind does not have (EPMC has two) are 0. */
#define LLL_W 0                         /* sum of the valid samples' weights */
#define LLL_N_EXCLUDED_WEIGHT 1
#define LLL_N_EXCLUDED_NONFINITE 2
#define LLL_ADV_MEAN 3                  /* before normalisation */
#define LLL_ADV_STD 4                   /* sqrt of the population variance, without adv_eps */
#define LLL_PG_LOSS 5
#define LLL_VALUE_LOSS 6
#define LLL_LOSS 7
#define LLL_ENTROPY 8                   /* [3] */
#define LLL_APPROX_KL 11                /* [3]: 0.5 mean((n_h - o_h)^2) */
#define LLL_CLIP_FRAC 14                /* [3]: weighted share of samples whose clipped branch is active; merge_heads: slot 0 only */
#define LLL_RETURN_MEAN 17              /* mean of R as used */
#define LLL_VALUE_MEAN 18               /* mean of v */
#define LLL_EXPLAINED_VARIANCE 19       /* 1 - Var(R - v) / Var(R), 0 where Var(R) = 0 */
#define LLL_N_STATS 20

typedef struct ll_hl_loss_config_t {
  int32_t mode;               /* LLL_PPO | LLL_PPO2 */
  int32_t merge_heads;        /* 1: one ratio from the summed neglogp of all heads; 0: one ratio and one surrogate per head, summed */
  int32_t adv_normalize;      /* 1: (adv - mean) / sqrt(var + adv_eps) over the valid samples of the block (population variance) */
  int32_t reserved;           /* 0 */
  float clip_range;           /* upper: ratio <= 1 + clip_range */
  float clip_range_lower;     /* ratio >= 1 - clip_range_lower; <= 0: clip_range */
  float vf_clip;              /* LLL_PPO only; <= 0: 0.5 (v - R)^2; > 0: 0.5 max((v - R)^2, (V_old + clip(v - V_old, +-vf_clip) - R)^2) */
  float vf_coef, ent_coef;
  float gamma, lam;           /* LLL_PPO2 only */
  float adv_eps;
} ll_hl_loss_config_t;

/* Host only.  mode LLL_PPO, merge_heads 1, adv_normalize 1, clip_range 0.2, clip_range_lower 0, vf_clip 0, vf_coef 1, ent_coef 0, gamma 0.95,
 * lam 0.95, adv_eps 1e-8 (vf_coef, ent_coef and lam as in example_epmc_train.sh).  LL_EINVAL for NULL. */
int ll_hl_loss_default_config(ll_hl_loss_config_t* cfg);
/* Host only: the size of d_work for a block of n_rows x unroll_length (any mode).  LL_EINVAL for NULL or a non-positive size. */
int ll_hl_loss_workspace_bytes(int n_rows, int unroll_length, uint64_t* out);
/*
 * kind: LLH_EPMC or LLH_SEPMC.  d_rows [n_rows][unroll_length][row_floats] in the row layout of llenv_hl_unroll.h, d_score [n_rows][unroll_length]
 * [LLS_OUT_FLOATS] as ll_hl_score_* wrote it, d_weight [n_rows][unroll_length] float32 or NULL for all ones -> d_grad [n_rows][unroll_length]
 * [LLS_OUT_FLOATS] float32 and d_stats [LLL_N_STATS] float64, both on the device; d_work: at least work_bytes >= ll_hl_loss_workspace_bytes bytes of
 * device memory, contents irrelevant.  d_score and d_grad must be 16-byte aligned, d_stats and d_work 8-byte.  Asynchronous on hip_stream (NULL:
 * the default stream).
 * LL_EINVAL: a NULL pointer other than d_weight, a non-positive n_rows or unroll_length, unroll_length < 2 in LLL_PPO2, an unknown kind or mode,
 * a non-finite or negative clip_range, vf_coef or adv_eps, a non-finite clip_range_lower, vf_clip or ent_coef, gamma or lam outside [0, 1],
 * work_bytes too small, a misaligned pointer, a block of 2^31 floats per row or more.
 */
int ll_hl_loss_rows(int kind, const ll_hl_loss_config_t* cfg, const float* d_rows, int n_rows, int unroll_length, const float* d_score,
                    const float* d_weight, float* d_grad, double* d_stats, void* d_work, uint64_t work_bytes, void* hip_stream);
/*
 * The same for block `buffer` of a recorder or of a league (its learner rows: n_rows = the arena count), queued on that engine's stream.  kind, n_rows
 * and unroll_length are the recorder's.  LL_EINVAL also for a buffer outside 0 .. n_buffers - 1; LL_ESTATE while the buffer holds no complete unroll,
 * decided on the host from the position as ll_hl_score_unroll does.  R is read as it stands: in LLL_PPO, call ll_hl_unroll_finish /
 * ll_hl_league_finish on the block first.  Neither the block nor the position is touched.
 */
int ll_hl_loss_unroll(ll_hl_unroll* rec, int buffer, const ll_hl_loss_config_t* cfg, const float* d_score, const float* d_weight, float* d_grad,
                      double* d_stats, void* d_work, uint64_t work_bytes);
int ll_hl_loss_league(ll_hl_league* lg, int buffer, const ll_hl_loss_config_t* cfg, const float* d_score, const float* d_weight, float* d_grad,
                      double* d_stats, void* d_work, uint64_t work_bytes);

#ifdef __cplusplus
}
#endif
#endif

/*
 * llenv_hl_policy.h -- C ABI of the on-device EPMC and SEPMC policies: the trained environmental-level and strategic-level
 * checkpoints acting on an engine's own buffers, their LSTM state kept on the device.
 *
 * The forward pass (argmax code, mean action) is the one oracle/epmc_policy.py (EpmcPolicy.act) and oracle/sepmc_policy.py
 * (SepmcPolicy.act) state in float64, restated as ONE fused kernel per call, 16 rows per workgroup:
 *   rms normalisation of prop (135 columns, clip +-5);
 *   the three percept encoders on VALU (2-D 25x13: 1x1 -> 4x4/2 -> 2x2/2 -> 2x2/1, 4 channels, SAME padding, 28 values each;
 *   1-D lidar with 4-column periodic padding and the [4:-4] crop: 32 values);
 *   the dense layers on the matrix cores (v_mfma_f32_16x16x4_f32, exact float32: the PMC kernel's pol_dense);
 *   the layer-normalised LSTM z = LN(x Wx) + LN(h Wh) + b, gates i, f, o, u, forget bias 1.0, h' = sigmoid(o) tanh(LN(c'));
 *   the first argmax of the 256 z logits, its code vector, and the low-level controller 96 -> 256 -> 256 -> 12.
 * SEPMC runs its high-level chain (own percept encoders, own LSTM) first; its heading, clipped to +-pi, becomes the mid-level's
 * target [cos, sin, control_spd].
 *
 * Rows: one per robot, the engine's row order (SEPMC: row = 2 arena + robot).  Each row has its own recurrent state, a device
 * buffer the policy owns: [max_rows][state_dim] float32,
 *   EPMC   state_dim  64:  c[32] | h[32]
 *   SEPMC  state_dim 128:  hlc c[32] | hlc h[32] | z c[32] | z h[32]
 *
 * Auto-reset: with auto_reset = 1 the EPMC / SEPMC step kernels re-seed a finished env (arena) INSIDE the step (epmc_step.hpp,
 * sepmc_step.hpp): they write done[row] = 1 and, into the obs row, the first observation of the new episode (history filled as at
 * a reset).  The SEPMC engine sets done on both rows of the arena.  So passing the engine's done buffer as d_reset (ll_device_ptrs_t.done
 * of ll_epmc_device_ptrs / ll_sepmc_device_ptrs: one byte per row) starts exactly the re-seeded rows from zero state -- agent.reset
 * at an episode start -- and the actor loop  act ; step ; act ; step ...  needs no host involvement.
 *
 * Same conventions as llenv.h: 0 or a negative LL_E* code, ll_last_error() for the text.  Argument errors (kind, n_floats,
 * obs_stride, n_rows > max_rows) are LL_EINVAL and are checked before the device is touched; without a HIP device
 * ll_hl_policy_create fails with LL_ENODEV -- there is no CPU fallback.
 */
#ifndef LLENV_HL_POLICY_H
#define LLENV_HL_POLICY_H

#include <stdint.h>

#include "../llenv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LLH_EPMC 1             /* arrays 0, 1, 47..101 of environmental_level_*.model (57 arrays) */
#define LLH_SEPMC 2            /* arrays 0, 1, 51..151 of strategic_level.model (103 arrays) */
#define LLH_EPMC_N_FLOATS 208437
#define LLH_SEPMC_N_FLOATS 316806
#define LLH_EPMC_OBS_DIM 916   /* prop 99 | prop_a 36 | percep_2d 325 | percep_1d 128 | percep_front 325 | target 3 */
#define LLH_SEPMC_OBS_DIM 965  /* ... percept_front | percept_vec 5 | oppo_info 15 | oppo_info_cheat 15 | flag_info 7 | flag_info_cheat 7 | with_flag 2 | control_spd 1 */
#define LLH_ACT_DIM 12
#define LLH_EPMC_VF_N_FLOATS 137872    /* arrays 2..46 of environmental_level_*.model: the value branch */
#define LLH_SEPMC_VF_N_FLOATS 182864   /* arrays 2..50 of strategic_level.model */
#define LLH_EPMC_N_HEADS 2             /* neglogp columns: z, llc */
#define LLH_SEPMC_N_HEADS 3            /* hlc, z, llc */

typedef struct ll_hl_policy ll_hl_policy;

/* h_weights: the arrays of `kind`, float32, each row-major in its checkpoint shape, concatenated in checkpoint order
 * (tests/golden/epmc_policy_*.npz, sepmc_policy.npz).  The state of every row starts at zero. */
int ll_hl_policy_create(int kind, const float* h_weights, int n_floats, int max_rows, int device, ll_hl_policy** out);
int ll_hl_policy_destroy(ll_hl_policy* p);
int ll_hl_policy_state_dim(ll_hl_policy* p);
/*
 * One step of the policy for rows 0 .. n_rows-1, asynchronous on hip_stream (NULL: the default stream):
 *   d_obs      [n_rows][obs_stride]   obs_stride must be the kind's obs dim
 *   d_reset    (nullable) [n_rows] uint8: rows with d_reset[r] != 0 start this call from zero state
 *   d_actions  [n_rows][12]           mean action
 *   d_code     (nullable) [n_rows]    int32 index of the chosen z code
 *   d_heading  (nullable, SEPMC only) [n_rows]  the high-level heading angle
 * and the state of those rows advances.  Rows >= n_rows of every output and of the state are not written.
 */
int ll_hl_policy_act(ll_hl_policy* p, const float* d_obs, int obs_stride, const uint8_t* d_reset, float* d_actions, int32_t* d_code,
                     float* d_heading, int n_rows, void* hip_stream);
int ll_hl_policy_reset_state(ll_hl_policy* p, void* hip_stream);      /* every row to zero (the value state too, once attached), queued on hip_stream */
/* host copies of the whole state buffer [max_rows][state_dim]; both wait for the device to be idle first */
int ll_hl_policy_get_state(ll_hl_policy* p, float* h_state);
int ll_hl_policy_set_state(ll_hl_policy* p, const float* h_state);
/*
 * The PPO actor (the self-fed heads of the training scripts' actor_type=PPO, use_value_head: True).
 *
 * ll_hl_policy_attach_value uploads the value branch, h_vf_weights = arrays 2..46 (EPMC, LLH_EPMC_VF_N_FLOATS) or 2..50 (SEPMC,
 * LLH_SEPMC_VF_N_FLOATS) of the checkpoint in checkpoint order (tests/golden/epmc_value_*.npz, sepmc_value.npz), and gives every row a
 * zeroed value LSTM state [max_rows][64] (c | h).  Attaching again replaces the weights and zeroes that state.
 *
 * ll_hl_policy_act_pg is ll_hl_policy_act with, for every row:
 *   sample != 0  every head sampled with Philox4x32-10, key (seed lo, seed hi), counter (row * G + g, step lo, step hi, salt), one salt per head;
 *                the draws depend on (seed, step, row) only:
 *                  SEPMC heading  mu + exp(logstd) eps, mu = the clipped mean, the sample itself not clipped (G 1, one Box-Muller normal);
 *                  z code         Gumbel-max argmax(logit - log(-log u)) over the 256 logits (G 64: word j of block g is code 4 g + j,
 *                                 u = ((w >> 8) + 0.5) 2^-24), and the low-level controller runs at the sampled code;
 *                  action         mean + exp(logstd) eps, twelve Box-Muller normals (G 3, as ll_policy_act_pg);
 *   sample == 0  the modes: the argmax code, the mean action, the clipped mean heading (what ll_hl_policy_act emits).
 *   d_neglogp    (nullable) [n_rows][n_heads] -log p of each emitted head, columns in action-space order: EPMC z, llc; SEPMC hlc, z, llc.
 *                Categorical: logsumexp(logits) - logits[code]; Gaussian: 0.5 sum eps^2 + 0.5 d log(2 pi) + sum logstd.
 *   d_value      (nullable) [n_rows] the value head; needs an attached branch (LL_EINVAL otherwise, before any launch).  The value state of
 *                rows < n_rows advances on the calls that compute a value; d_reset zeroes it like the policy state.
 * The policy state advances exactly as in ll_hl_policy_act.  The value branch runs as a second set of workgroups of the same launch.
 */
int ll_hl_policy_attach_value(ll_hl_policy* p, const float* h_vf_weights, int n_floats);
int ll_hl_policy_act_pg(ll_hl_policy* p, const float* d_obs, int obs_stride, const uint8_t* d_reset, float* d_actions, int32_t* d_code, float* d_heading,
                        float* d_neglogp, float* d_value, uint64_t seed, uint64_t step, int sample, int n_rows, void* hip_stream);
/* host copies of the value state [max_rows][64] (c | h); LL_EINVAL without an attached branch; both wait for the device to be idle first */
int ll_hl_policy_get_value_state(ll_hl_policy* p, float* h_state);
int ll_hl_policy_set_value_state(ll_hl_policy* p, const float* h_state);
/*
 * A new model for a policy in use: replaces the weights (and, when a value branch is attached, the branch: h_vf_weights is then required;
 * without a branch it must be NULL) and touches no recurrent state -- the actor's pull of fresh weights every update_model_freq steps
 * (distill_actor.py:294-308).  Same float counts as create / attach_value.  The upload is ordered on hip_stream, from a pinned staging
 * buffer the policy owns: the call neither waits for the device nor races a launch queued on that stream before it; a second call waits
 * for the first upload only.
 */
int ll_hl_policy_set_weights(ll_hl_policy* p, const float* h_weights, int n_floats, const float* h_vf_weights, int n_vf_floats, void* hip_stream);
/* HIP-event time of the ll_hl_policy_act and ll_hl_policy_act_pg launches since the last call (like ll_policy_time_ms) */
int ll_hl_policy_enable_timing(ll_hl_policy* p, int on);
int ll_hl_policy_time_ms(ll_hl_policy* p, double* avg_ms, int* n_launches);

#ifdef __cplusplus
}
#endif
#endif

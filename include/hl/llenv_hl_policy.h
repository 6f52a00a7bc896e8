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
int ll_hl_policy_reset_state(ll_hl_policy* p, void* hip_stream);      /* every row to zero, queued on hip_stream */
/* host copies of the whole state buffer [max_rows][state_dim]; both wait for the device to be idle first */
int ll_hl_policy_get_state(ll_hl_policy* p, float* h_state);
int ll_hl_policy_set_state(ll_hl_policy* p, const float* h_state);
/* HIP-event time of the ll_hl_policy_act launches since the last call (like ll_policy_time_ms) */
int ll_hl_policy_enable_timing(ll_hl_policy* p, int on);
int ll_hl_policy_time_ms(ll_hl_policy* p, double* avg_ms, int* n_launches);

#ifdef __cplusplus
}
#endif
#endif

/*
 * llenv_hl_unroll.h -- C ABI of the unroll recorder of the on-device EPMC and SEPMC actors: the loop  act_pg ; step  of
 * llenv_hl_policy.h, run on the engine's stream, with every transition packed into learner-ready unroll blocks in device memory.
 *
 * The reference trains both environments with actor_type=PPO, unroll_length 128, gamma 0.95, lam 0.95, use_lstm: True; its network
 * consumes the tuple X, A, neglogp, R, V, discount, r, S, M (epmc_net_data.py).  A recorder binds ONE engine to ONE ll_hl_policy with an
 * attached value branch and leaves exactly those fields, one float32 row per robot and control step:
 *
 *   field     width (EPMC / SEPMC)   content
 *   X         916 / 965              the observation the action was chosen on, in the engine's own column order (what ll_hl_policy_act reads)
 *   A         13 / 14                [heading (SEPMC only)] | z code as a float value | action[12]: the heads exactly as ll_hl_policy_act_pg emitted them
 *   neglogp   2 / 3                  per head, action-space order (LLH_EPMC_N_HEADS / LLH_SEPMC_N_HEADS)
 *   R         1                      TD(lambda) return, written by ll_hl_unroll_finish only
 *   V         1                      the value head's output for X
 *   r         1                      the engine's reward of this step
 *   discount  1                      1 - done of this step
 *   S         192 / 256              the recurrent state the LSTMs STARTED this step from, in the reference network's S layout: each LSTM's 64 values
 *                                    c | h;  EPMC: vf | pi (zeros: llc_light has no LSTM) | z;  SEPMC: vf | pi | z | hlc.  Zeros in a row that d_reset restarted
 *   M         1                      the mask: the d_reset flag of the step's act_pg call for time steps > 0 of an unroll, 0 for time step 0 (the first
 *                                    frame of an unroll carries the state itself and no mask: distill_actor.py:121-124,138-140)
 *   pad       0 / 1                  zeros, so that row_floats is a multiple of 4 (every row starts 16-byte aligned)
 * row_floats = 1128 (EPMC), 1244 (SEPMC).
 *
 * Rows are the engine's rows (EPMC: one per env; SEPMC: 2 arena + robot; both robots act with the same policy).  The blocks are ONE device
 * allocation [n_buffers][n_rows][unroll_length][row_floats]: the recorder's step s (counted from ll_hl_unroll_create) goes to time step
 * s % unroll_length of block (s / unroll_length) % n_buffers -- the ring arithmetic of ll_enable_unrolls -- so one robot's unroll is
 * unroll_length consecutive rows, and a finished block can be shipped from d_base while the next one fills.
 *
 * Two assumptions, stated as llenv.h states them for the PMC row: the (absent) tleague package owns the real flatten order of the data structure,
 * the field order above is that of the network's input tuple with r and discount behind V as in the PMC row; and X keeps the engine's column
 * order rather than the sorted-key order of the observation dict.
 *
 * Every act_pg of the loop passes the engine's done buffer as d_reset (the auto-reset loop of llenv_hl_policy.h), and its Philox `step` is the
 * recorder's own count of steps since create: a given (seed, n) reproduces exactly.
 *
 * The recorder launches kernels of its own around the policy and step kernels; it changes none of them, and it owns the small buffers the
 * policy writes code, heading, neglogp and value into.  S is captured before act_pg advances the state; A, neglogp, V after it; r and
 * discount after the step.
 *
 * Same conventions as llenv.h: 0 or a negative LL_E* code, ll_last_error() for the text.  Argument errors are LL_EINVAL and are checked before
 * the device is touched; there is no CPU fallback: LL_ENODEV without a HIP device.
 */
#ifndef LLENV_HL_UNROLL_H
#define LLENV_HL_UNROLL_H

#include <stdint.h>

#include "../llenv_epmc.h"
#include "../llenv_sepmc.h"
#include "llenv_hl_policy.h"

#ifdef __cplusplus
extern "C" {
#endif

/* fields of a row, the index into ll_hl_unroll_layout_t.off / .dim */
#define LLU_X 0
#define LLU_A 1
#define LLU_NEGLOGP 2
#define LLU_R 3
#define LLU_V 4
#define LLU_REWARD 5
#define LLU_DISCOUNT 6
#define LLU_S 7
#define LLU_M 8
#define LLU_PAD 9
#define LLU_N_FIELDS 10
#define LLU_EPMC_ROW_FLOATS 1128
#define LLU_SEPMC_ROW_FLOATS 1244

typedef struct ll_hl_unroll ll_hl_unroll;

typedef struct ll_hl_unroll_layout_t {
  int32_t kind;                 /* LLH_EPMC or LLH_SEPMC */
  int32_t row_floats;
  int32_t n_rows;
  int32_t unroll_length;
  int32_t n_buffers;
  int32_t reserved;             /* 0 */
  int32_t off[LLU_N_FIELDS];    /* first column of every field */
  int32_t dim[LLU_N_FIELDS];    /* its width (pad: may be 0) */
  float* d_base;                /* [n_buffers][n_rows][unroll_length][row_floats] */
  uint64_t n_bytes;             /* size of the allocation */
} ll_hl_unroll_layout_t;

/*
 * LL_EINVAL when the policy has no value branch attached, when its kind does not match the engine (EPMC engine: LLH_EPMC, SEPMC engine:
 * LLH_SEPMC), when its max_rows is smaller than the engine's row count, when it lives on another device, or when unroll_length or n_buffers
 * is not positive.  The blocks are one hipMalloc; LL_ENOMEM names the size that failed.  Unroll 0 starts with the first step of
 * ll_hl_unroll_steps, whatever the engine and the policy did before.  The engine and the policy must outlive the recorder.
 */
int ll_hl_unroll_create_epmc(ll_epmc_engine* e, ll_hl_policy* p, int unroll_length, int n_buffers, ll_hl_unroll** out);
int ll_hl_unroll_create_sepmc(ll_sepmc_engine* e, ll_hl_policy* p, int unroll_length, int n_buffers, ll_hl_unroll** out);
int ll_hl_unroll_destroy(ll_hl_unroll* rec);
int ll_hl_unroll_layout(ll_hl_unroll* rec, ll_hl_unroll_layout_t* out);
/*
 * n_steps x { record X, S, M ; ll_hl_policy_act_pg(d_reset = the engine's done buffer, step = steps since create) ; engine step ;
 * record A, neglogp, V, r, discount } on the engine's stream, asynchronous: no host synchronisation inside.  sample as in ll_hl_policy_act_pg.
 * The engine must have been reset (LL_ESTATE).  n_steps > unroll_length x n_buffers would overwrite rows of the call's own: LL_EINVAL
 * (as ll_step_random_n).  A call may run from one unroll into the next; the block it runs into must have been handed over by then.
 */
int ll_hl_unroll_steps(ll_hl_unroll* rec, uint64_t seed, int sample, int n_steps);
/* Where the NEXT step writes: the index of its unroll (counted from create) and its time step inside it, as ll_unroll_position.  Unroll k
 * lives in block k % n_buffers and is complete when this reports unroll_index = k + 1, time_step = 0. */
int ll_hl_unroll_position(ll_hl_unroll* rec, int64_t* unroll_index, int* time_step);
/*
 * TD(lambda) returns of the newest complete unroll in block `buffer`, the recursion of ll_finish_unroll:
 *   delta_t = r_t + gamma V_{t+1} m_t - V_t,   A_t = delta_t + gamma lam m_t A_{t+1},   R_t = A_t + V_t,   m_t = discount_t,
 * V_T = d_bootstrap_value[row] ([n_rows] floats on the device; always accepted).  With NULL, V_T is the V field of time step 0 of the NEXT
 * unroll -- the actor loop computes it as its next act_pg; no other evaluation is possible without advancing the LSTM -- and the call fails
 * with LL_ESTATE, decided on the host from the recorder's position, while the step that writes it has not run (or `buffer` holds no
 * complete unroll).  Asynchronous on the engine's stream.
 */
int ll_hl_unroll_finish(ll_hl_unroll* rec, int buffer, float gamma, float lam, const float* d_bootstrap_value);

#ifdef __cplusplus
}
#endif
#endif

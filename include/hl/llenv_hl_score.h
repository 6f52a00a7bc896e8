/*
 * llenv_hl_score.h -- C ABI of the teacher-forced scorer of recorded EPMC / SEPMC unrolls: a block of llenv_hl_unroll.h rows evaluated
 * under ANY weights, on the device, in one launch.
 *
 * What the reference's learner computes first from an unroll (epmc_net.py:278-410: outer_fed_head_neglogp, vpred, entropy_loss): for every
 * recorded time step the neglogp of the RECORDED action of every head, the entropy of every head and the value prediction, the LSTMs
 * starting from the S of the unroll's first frame and re-zeroed where M says so.  The same pass tells an actor how stale its weights were,
 * and a block scored under the weights it was recorded with gives back its own neglogp and V.
 *
 * The weights come from an ordinary ll_hl_policy with an attached value branch, the "weight carrier": create it with any weights, renew
 * them with ll_hl_policy_set_weights.  Its recurrent state, its value state and its max_rows play no part: scoring neither reads nor writes
 * them, and n_rows may exceed max_rows.
 *
 * Per row (one robot's unroll, time steps t = 0 .. unroll_length - 1, the row layout of llenv_hl_unroll.h):
 *   state at t = 0     the value LSTM starts from S[0:64], the z LSTM from S[128:192], SEPMC's hlc LSTM from S[192:256] (each c[32] | h[32]:
 *                      the inverse of the recorder's mapping); M of time step 0 is ignored;
 *   state at t > 0     what time step t - 1 left, set to zero first where M_t != 0; S_t is not read;
 *   SEPMC heading      the hlc chain to its clipped mean mu; for the recorded heading h = A[0]:
 *                      neglogp = 0.5 ((h - mu) / sigma)^2 + 0.5 log(2 pi) + logstd, entropy = 0.5 (1 + log(2 pi)) + logstd;
 *                      the mid level's target is cos h, sin h, X[964]: the RECORDED heading, not mu;
 *   z head             the 256 logits and the recorded code c = (int)A[z]: neglogp = logsumexp - logit[c], entropy = logsumexp - sum softmax x logit.
 *                      For a code outside 0 .. 255 (a corrupt block) nothing is read out of bounds; neglogp and entropy of the z and of the llc
 *                      head of that time step are NaN, and every other value of the row is what it would have been;
 *   controller         runs at the recorded code; for the recorded action a: neglogp = 0.5 sum ((a - mean) / exp(logstd))^2 + 6 log(2 pi) + sum logstd,
 *                      entropy = 6 (1 + log(2 pi)) + sum logstd;
 *   value              the value branch on the same X.
 * The Gaussian heads are formed as eps = (a - mean) / exp(logstd) fed into the sum ll_hl_policy_act_pg uses, the logsumexp is reduced as
 * there: a block recorded with sample = 0 scores, under the recording weights, to its own neglogp and V bit for bit, one recorded with
 * sample = 1 to its own V and z neglogp.
 *
 * One output row of LLS_OUT_FLOATS = 8 float32 per recorded row (heads in action-space order as in ll_hl_policy_act_pg):
 *   kind                 neglogp   entropy   V   zero pad
 *   EPMC  (n_heads 2)    0 .. 1    2 .. 3    4   5 .. 7         heads z, llc
 *   SEPMC (n_heads 3)    0 .. 2    3 .. 5    6   7              heads hlc, z, llc
 *
 * One kernel launch per block: the time loop runs inside the kernel and the LSTM state never leaves the chip.  Only X, A, S (time step 0)
 * and M of the block are read and nothing but d_out is written.
 *
 * Same conventions as llenv.h: 0 or a negative LL_E* code, ll_last_error() for the text.  Argument errors are LL_EINVAL and are checked
 * before the device is touched; there is no CPU path: LL_ENODEV without a HIP device.  These entry points add to the library and change
 * no struct that crosses it, so LL_ABI_VERSION (the layout of the config structs, llenv.h) stays as it is -- as it did for
 * llenv_hl_policy.h, llenv_hl_unroll.h and llenv_hl_league.h.
 */
#ifndef LLENV_HL_SCORE_H
#define LLENV_HL_SCORE_H

#include <stdint.h>

#include "llenv_hl_league.h"
#include "llenv_hl_policy.h"
#include "llenv_hl_unroll.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LLS_OUT_FLOATS 8
/* fields of an output row, the index into ll_hl_score_layout_t.off / .dim */
#define LLS_NEGLOGP 0
#define LLS_ENTROPY 1
#define LLS_V 2
#define LLS_PAD 3
#define LLS_N_FIELDS 4

typedef struct ll_hl_score_layout_t {
  int32_t kind;                 /* LLH_EPMC or LLH_SEPMC */
  int32_t n_heads;              /* LLH_EPMC_N_HEADS / LLH_SEPMC_N_HEADS */
  int32_t out_floats;           /* LLS_OUT_FLOATS */
  int32_t reserved;             /* 0 */
  int32_t off[LLS_N_FIELDS];    /* first column of every field */
  int32_t dim[LLS_N_FIELDS];    /* its width */
} ll_hl_score_layout_t;

/* Host only.  LL_EINVAL for a kind that is neither LLH_EPMC nor LLH_SEPMC. */
int ll_hl_score_layout(int kind, ll_hl_score_layout_t* out);
/*
 * d_rows [n_rows][unroll_length][row_floats] in the row layout of llenv_hl_unroll.h for w's kind (1128 / 1244 floats) -> d_out
 * [n_rows][unroll_length][LLS_OUT_FLOATS], asynchronous on hip_stream (NULL: the default stream).  LL_EINVAL for a NULL argument, a
 * non-positive n_rows or unroll_length, a block of 2^31 floats per row or more, or a carrier without a value branch.
 */
int ll_hl_score_rows(ll_hl_policy* w, const float* d_rows, int n_rows, int unroll_length, float* d_out, void* hip_stream);
/*
 * The same for block `buffer` of a recorder or of a league (its learner rows: n_rows = the arena count), queued on that engine's stream
 * behind the steps that filled it; d_out [n_rows][unroll_length][LLS_OUT_FLOATS].  LL_EINVAL for a carrier of another kind (a league's
 * is LLH_SEPMC) or on another device, or a buffer outside 0 .. n_buffers - 1; LL_ESTATE while the buffer holds no complete unroll, decided
 * on the host from the position as the finish calls do.  Neither the block, nor the position, nor R is touched.
 */
int ll_hl_score_unroll(ll_hl_policy* w, ll_hl_unroll* rec, int buffer, float* d_out);
int ll_hl_score_league(ll_hl_policy* w, ll_hl_league* lg, int buffer, float* d_out);

#ifdef __cplusplus
}
#endif
#endif

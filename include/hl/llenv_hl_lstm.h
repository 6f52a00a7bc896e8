/*
 * llenv_hl_lstm.h -- C ABI of the layer-normalised LSTM core that the five recurrent networks of the EPMC / SEPMC policies share, with its linear
 * head: the forward over an unroll, leaving a tape, and the backward through time, on the device.
 *
 * The EPMC z policy and value and the SEPMC hlc, z and value networks each end in the same cell -- 256 inputs -> 128 layer-normalised gate
 * pre-activations -> 32 units, nine arrays k0 .. k0 + 8 in the same order (csrc/hl_policy.inc hl_lstm) -- followed by one linear head 32 -> D:
 *
 *   branch        k0    head arrays   D
 *   EPMC z        79    88, 89        256
 *   EPMC value    36    45, 46        1
 *   SEPMC hlc     85    94, 95        1
 *   SEPMC z       129   138, 139      256
 *   SEPMC value   40    49, 50        1
 *
 * The cell is the only state-dependent part of these networks; their feed-forward fronts are batched over n x L independent frames and are the
 * caller's.  This header is the cell and its head, generic over D; the branches differ only in which arrays are passed.  tests/hl_lstm_ref.py is the
 * normative statement.
 *
 * Weights, eleven arrays: wx [256][128], wh [32][128], b [128], beta_x, gamma_x, beta_h, gamma_h [128], beta_c, gamma_c [32], wo [32][D], bo [D],
 * 1 <= D <= 256.  LN(x; beta, gamma) = (x - mean) (var + 1e-12)^-1/2 gamma + beta with the population variance.
 *
 * Forward, per row, t = 0 .. L - 1.  At t = 0 (c, h) = S0[0:32] | S0[32:64]; at t > 0 it is what step t - 1 left, set to zero first where
 * M[t] != 0 (any non-zero value counts, and so does NaN); M[0] is not read -- the scorer's rules (llenv_hl_score.h).
 *   u = E_t wx;  v = h wh;  z = LN(u; beta_x, gamma_x) + LN(v; beta_h, gamma_h) + b;  i, f, o, g = split(z)
 *   c' = sigmoid(f + 1) c + sigmoid(i) tanh(g);  n = LN(c'; beta_c, gamma_c);  h' = sigmoid(o) tanh(n);  y_t = h' wo + bo
 * Outputs: Y [n][L][D] and S_end [n][64] = c | h after the last step.
 *
 * Backward: the exact derivative of sum(Y dY) + sum(S_end dS_end) with respect to E, S0 and the weights.  Where M[t] != 0 (t > 0) nothing flows from
 * step t into the state of step t - 1.  LN backward, x^ and r from the forward: dgamma = sum dy x^, dbeta = sum dy,
 * dx = r (dx^ - mean(dx^) - x^ mean(dx^ x^)), dx^ = dy gamma.  Two consequences:
 *   - d b, d beta_x and d beta_h are the same numbers (all three are the sum of the gradient at z).
 *   - A step that starts from h = 0 (a zero S0, or a reset) has v = 0; its LN has r = 10^6, so dS0[32:64] of a zero-state row is large by the formula.
 *     That value is the derivative, not an error.  d wh gets nothing from that step.
 * The weight gradient is one packed float32 array in the order above, 37568 + 33 D floats (ll_hl_lstm_weight_layout).
 *
 * Arithmetic: the LNs and the gates are float32 with the rsqrt / 1 / (1 + exp(-x)) / tanhf forms of hl_lstm; every dot product multiplies float32 values exactly
 * and adds them in float64, rounding once.  Sums over frames go workgroup partial -> one fold launch that adds the partials in index order in float64 and
 * rounds once: no floating-point atomics, no ticket, and two calls on the same inputs return the same bits.
 * A row's Y, S_end, dE and dS0 do not depend on which other rows are in the call.  Calls are asynchronous: no host synchronisation and no allocation.
 *
 * Same conventions as llenv_hl_loss.h: 0 or a negative LL_E* code, ll_last_error() for the text.  Argument errors are LL_EINVAL and are decided
 * before the device is touched; there is no CPU path: LL_ENODEV without a HIP device.  Additive entry points: LL_ABI_VERSION stays as it is.
 */
#ifndef LLENV_HL_LSTM_H
#define LLENV_HL_LSTM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LLT_N_IN 256
#define LLT_N_GATES 128
#define LLT_N_UNITS 32
#define LLT_STATE_FLOATS 64       /* c | h */
#define LLT_MAX_OUT 256
#define LLT_N_WEIGHTS 11
#define LLT_TAPE_FLOATS 356       /* per frame */

typedef struct ll_hl_lstm_weights_t {
  const float* wx;        /* [256][128] */
  const float* wh;        /* [32][128] */
  const float* b;         /* [128] */
  const float* beta_x;    /* [128] */
  const float* gamma_x;   /* [128] */
  const float* beta_h;    /* [128] */
  const float* gamma_h;   /* [128] */
  const float* beta_c;    /* [32] */
  const float* gamma_c;   /* [32] */
  const float* wo;        /* [32][n_out] */
  const float* bo;        /* [n_out] */
  int32_t n_out;          /* D, 1 .. 256 */
  int32_t reserved;       /* 0 */
} ll_hl_lstm_weights_t;

/* Host only.  The packed order of the weight gradient: off[i], dim[i] floats of array i (the order of the struct), *total = 37568 + 33 n_out.  Any of
 * the three outputs may be NULL.  LL_EINVAL for n_out outside 1 .. 256. */
int ll_hl_lstm_weight_layout(int n_out, uint64_t off[LLT_N_WEIGHTS], uint64_t dim[LLT_N_WEIGHTS], uint64_t* total);
/* Host only.  The sizes of d_tape (forward, backward) and d_work (backward) for n_rows x L frames; either output may be NULL.  LL_EINVAL for
 * non-positive sizes, n_out outside 1 .. 256, n_rows x L >= 2^31. */
int ll_hl_lstm_workspace_bytes(int n_rows, int L, int n_out, uint64_t* tape_bytes, uint64_t* work_bytes);
/*
 * d_e [n_rows][L][256] dense.  S0 of row r: d_s0 + r * s0_row_stride, 64 floats (s0_row_stride >= 64).  M of (r, t): d_m[r * m_row_stride +
 * t * m_step_stride]; strides in floats, so S0 and M can be read straight out of a recorded block of llenv_hl_unroll.h (S0: the value, z or hlc slice
 * of S of the first frame, row stride L * row_floats; M: the M field, step stride row_floats, row stride L * row_floats).  m_step_stride >= 1,
 * m_row_stride >= 1.  -> d_y: frame (r, t) at d_y + (r * L + t) * y_stride, n_out floats (y_stride >= n_out); d_s_end [n_rows][64] or NULL;
 * d_tape: tape_bytes >= ll_hl_lstm_workspace_bytes' tape_bytes, or NULL (inference only: no backward can follow).
 * LL_EINVAL: a NULL pointer other than d_s_end and d_tape, non-positive sizes, n_out outside 1 .. 256, a stride smaller than its field,
 * n_rows x L >= 2^31, a tape too small, d_e or d_tape not 16-byte aligned, a non-zero reserved.
 */
int ll_hl_lstm_forward(const ll_hl_lstm_weights_t* w, const float* d_e, const float* d_s0, int64_t s0_row_stride, const float* d_m, int64_t m_row_stride,
                       int64_t m_step_stride, int n_rows, int L, float* d_y, int64_t y_stride, float* d_s_end, float* d_tape, uint64_t tape_bytes,
                       void* hip_stream);
/*
 * d_tape as ll_hl_lstm_forward left it for the same w, d_e, d_m, n_rows and L.  d_dy: frame (r, t) at d_dy + (r * L + t) * dy_stride (dy_stride >=
 * n_out; 8 takes the V column of the loss's d_grad without a copy); d_ds_end [n_rows][64] or NULL for zero -> d_de [n_rows][L][256], d_ds0
 * [n_rows][64] or NULL, d_wgrad [37568 + 33 n_out].  d_work: work_bytes >= ll_hl_lstm_workspace_bytes' work_bytes, contents irrelevant.
 * LL_EINVAL as above, and for d_de or d_work not 16-byte aligned or a workspace too small.
 */
int ll_hl_lstm_backward(const ll_hl_lstm_weights_t* w, const float* d_e, const float* d_m, int64_t m_row_stride, int64_t m_step_stride, int n_rows, int L,
                        const float* d_tape, uint64_t tape_bytes, const float* d_dy, int64_t dy_stride, const float* d_ds_end, float* d_de, float* d_ds0,
                        float* d_wgrad, void* d_work, uint64_t work_bytes, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif

// hl_policy.inc -- the fused EPMC / SEPMC policy kernels and the C ABI of include/hl/llenv_hl_policy.h (included by llenv.hip after
// pmc_policy.inc, whose pol_dense runs every dense layer here).
//
// One workgroup = 16 rows (the M of every matrix product), 8 wavefronts.  Activations live in LDS k-major ([k][16 rows]) as in the
// PMC kernel.  The percept encoders (about 60 k MACs a row, 4-channel tiles) run on VALU: one lane = one output position of one row,
// all output channels in registers; the 1x1 first layer of a 2-D stack and the periodic first layer of the 1-D stack are folded into
// the layer that reads them, so only two intermediate maps per stack ever exist (<= 7872 floats, in the two activation buffers).
// Layer norms and the LSTM cell: 32 lanes per row (lane j holds gates i, f, o, u of unit j), reductions by shuffles within the half-wave.
// The recurrent state is read from and written back to the policy's [max_rows][state_dim] buffer by the same launch.
#include "../../include/hl/llenv_hl_policy.h"

#define HL_MAX_ARRAY 152          // checkpoint array numbers 0..151; the kernel addresses weights by them
#define HL_PI 3.14159265358979323846f

struct HlW {
  const float* a[HL_MAX_ARRAY];   // a[k]: checkpoint array k (null where the kind does not carry it)
  const float* zero;              // 256 zeros: the bias of the LSTM's two bias-free products
};

// Which rows the 16 columns of a workgroup are.  row(m): the row whose observation, reset flag, outputs and Philox counters column m carries;
// srow(m): where that column's recurrent state and value live; live(m): the column holds a row at all.  HlDense is rows row0 .. row0 + 15 of
// n_rows (ll_hl_policy_act / _act_pg); hl_league.inc has the list map.  The helpers below also take the weights as a type: anything with
// a[k] and zero.
struct HlDense {
  int row0, n_rows;
  __device__ __forceinline__ int row(int m) const { return row0 + m; }
  __device__ __forceinline__ int srow(int m) const { return row0 + m; }
  __device__ __forceinline__ bool live(int m) const { return row0 + m < n_rows; }
};

__host__ __device__ constexpr int hl_same_out(int n, int s) { return (n + s - 1) / s; }
// tf SAME padding: pad_total = max((out - 1) s + k - n, 0), the smaller half in front (oracle/epmc_policy.py _same_pad)
__host__ __device__ constexpr int hl_same_front(int n, int k, int s) {
  return ((hl_same_out(n, s) - 1) * s + k - n > 0 ? (hl_same_out(n, s) - 1) * s + k - n : 0) / 2;
}

// out(m, p, acc[CO]) <- relu-free SAME cross-correlation of an [H][W][CI] map of each of the 16 rows, stride S; in(m, y, x, v[CI]) supplies
// one in-range input pixel.  Weights [KH][KW][CI][CO] (tf.contrib conv2d); taps in the padding contribute nothing.
template <int H, int W, int CI, int CO, int KH, int KW, int S, class In, class Out>
__device__ __forceinline__ void hl_conv(In in, const float* __restrict__ w, const float* __restrict__ b, Out out, int tid) {
  constexpr int OH = hl_same_out(H, S), OW = hl_same_out(W, S), PT = hl_same_front(H, KH, S), PL = hl_same_front(W, KW, S);
  for (int t = tid; t < POL_M * OH * OW; t += POL_THREADS) {
    const int m = t / (OH * OW), p = t - m * (OH * OW), oy = p / OW, ox = p - oy * OW;
    float acc[CO];
#pragma unroll
    for (int co = 0; co < CO; co++) acc[co] = b[co];
#pragma unroll
    for (int ky = 0; ky < KH; ky++) {
      const int y = oy * S - PT + ky;
      if (y < 0 || y >= H) continue;
#pragma unroll
      for (int kx = 0; kx < KW; kx++) {
        const int x = ox * S - PL + kx;
        if (x < 0 || x >= W) continue;
        float v[CI];
        in(m, y, x, v);
#pragma unroll
        for (int ci = 0; ci < CI; ci++)
#pragma unroll
          for (int co = 0; co < CO; co++) acc[co] = fmaf(v[ci], w[((ky * KW + kx) * CI + ci) * CO + co], acc[co]);
      }
    }
    out(m, p, acc);
  }
}

// percep_2d_encoder (epmc_net.py): 25x13x1 -> relu 1x1 (4) -> relu 4x4/2 (13x7x4) -> relu 2x2/2 (7x4x4) -> relu 2x2/1 (7x4x1) = 28 values,
// written to feat rows f0 .. f0 + 27.  Weights: arrays k .. k + 7.  scr: >= 7616 floats of LDS.
template <class WT, class RM>
__device__ __forceinline__ void hl_enc2d(const WT& W, int k, const float* __restrict__ obs, int stride, int col, const RM& R, float* scr, float* feat, int f0,
                                         int tid) {
  float* s1 = scr;                       // [16][13 * 7][4]
  float* s2 = scr + POL_M * 91 * 4;      // [16][7 * 4][4]
  const float *w1 = W.a[k], *b1 = W.a[k + 1];
  hl_conv<25, 13, 4, 4, 4, 4, 2>(
      [&](int m, int y, int x, float* v) {
        const int r = R.row(m);
        const float g = R.live(m) ? obs[(long)r * stride + col + y * 13 + x] : 0.0f;
#pragma unroll
        for (int c = 0; c < 4; c++) v[c] = fmaxf(fmaf(g, w1[c], b1[c]), 0.0f);
      },
      W.a[k + 2], W.a[k + 3], [&](int m, int p, const float* acc) {
#pragma unroll
        for (int c = 0; c < 4; c++) s1[(m * 91 + p) * 4 + c] = fmaxf(acc[c], 0.0f);
      }, tid);
  __syncthreads();
  hl_conv<13, 7, 4, 4, 2, 2, 2>(
      [&](int m, int y, int x, float* v) {
#pragma unroll
        for (int c = 0; c < 4; c++) v[c] = s1[(m * 91 + y * 7 + x) * 4 + c];
      },
      W.a[k + 4], W.a[k + 5], [&](int m, int p, const float* acc) {
#pragma unroll
        for (int c = 0; c < 4; c++) s2[(m * 28 + p) * 4 + c] = fmaxf(acc[c], 0.0f);
      }, tid);
  __syncthreads();
  hl_conv<7, 4, 4, 1, 2, 2, 1>(
      [&](int m, int y, int x, float* v) {
#pragma unroll
        for (int c = 0; c < 4; c++) v[c] = s2[(m * 28 + y * 4 + x) * 4 + c];
      },
      W.a[k + 6], W.a[k + 7], [&](int m, int p, const float* acc) { feat[(f0 + p) * POL_M + m] = fmaxf(acc[0], 0.0f); }, tid);
}

// percep_1d_encoder: 128 lidar values, periodic padding by 4 on both sides, relu conv 4 (1 -> 4) cropped back to 128, relu 4/2 (64x4),
// relu 4/2 (32x4), relu 4/1 (32x1) -> feat rows f0 .. f0 + 31.  Weights: arrays k .. k + 7.  The first layer is evaluated where the
// second reads it: on the 136-column padded input its SAME front pad is 1, so cropped position q sees lidar columns q - 1 .. q + 2 mod 128.
template <class WT, class RM>
__device__ __forceinline__ void hl_enc1d(const WT& W, int k, const float* __restrict__ obs, int stride, int col, const RM& R, float* scr, float* feat, int f0,
                                         int tid) {
  float* s1 = scr;                       // [16][64][4]
  float* s2 = scr + POL_M * 91 * 4;      // [16][32][4]
  const float *wa = W.a[k], *ba = W.a[k + 1];
  hl_conv<1, 128, 4, 4, 1, 4, 2>(
      [&](int m, int y, int q, float* v) {
        const int r = R.row(m);
        const bool live = R.live(m);
        float g[4];
#pragma unroll
        for (int t = 0; t < 4; t++) g[t] = live ? obs[(long)r * stride + col + ((q + t + 127) & 127)] : 0.0f;
#pragma unroll
        for (int c = 0; c < 4; c++) {
          float a = ba[c];
#pragma unroll
          for (int t = 0; t < 4; t++) a = fmaf(g[t], wa[t * 4 + c], a);
          v[c] = fmaxf(a, 0.0f);
        }
      },
      W.a[k + 2], W.a[k + 3], [&](int m, int p, const float* acc) {
#pragma unroll
        for (int c = 0; c < 4; c++) s1[(m * 64 + p) * 4 + c] = fmaxf(acc[c], 0.0f);
      }, tid);
  __syncthreads();
  hl_conv<1, 64, 4, 4, 1, 4, 2>(
      [&](int m, int y, int x, float* v) {
#pragma unroll
        for (int c = 0; c < 4; c++) v[c] = s1[(m * 64 + x) * 4 + c];
      },
      W.a[k + 4], W.a[k + 5], [&](int m, int p, const float* acc) {
#pragma unroll
        for (int c = 0; c < 4; c++) s2[(m * 32 + p) * 4 + c] = fmaxf(acc[c], 0.0f);
      }, tid);
  __syncthreads();
  hl_conv<1, 32, 4, 1, 1, 4, 1>(
      [&](int m, int y, int x, float* v) {
#pragma unroll
        for (int c = 0; c < 4; c++) v[c] = s2[(m * 32 + x) * 4 + c];
      },
      W.a[k + 6], W.a[k + 7], [&](int m, int p, const float* acc) { feat[(f0 + p) * POL_M + m] = fmaxf(acc[0], 0.0f); }, tid);
}

// the three percept stacks of one encoder (weights k: 2-D k .. k+7, 1-D k+8 .. k+15, front k+16 .. k+23) -> feat rows
// f0 .. f0+27 | f0+28 .. f0+59 | f0+60 .. f0+87.  Ends with a barrier.
template <class WT, class RM>
__device__ __forceinline__ void hl_percepts(const WT& W, int k, const float* __restrict__ obs, int stride, const RM& R, float* scr, float* feat, int f0, int tid) {
  hl_enc2d(W, k, obs, stride, 135, R, scr, feat, f0, tid);
  __syncthreads();
  hl_enc1d(W, k + 8, obs, stride, 460, R, scr, feat, f0 + 28, tid);
  __syncthreads();
  hl_enc2d(W, k + 16, obs, stride, 588, R, scr, feat, f0 + 60, tid);
  __syncthreads();
}

__device__ __forceinline__ float hl_sum32(float v) {     // sum over the 32 lanes of a half-wavefront (one row)
#pragma unroll
  for (int o = 16; o >= 1; o >>= 1) v += __shfl_xor(v, o, 32);
  return v;
}

__device__ __forceinline__ float hl_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// The state of one LSTM (c at st[0..31], h at st[32..63] of a row's state) into LDS k-major: cs, hs [32][16]; columns without a row and rows
// flagged in reset start from zero.
template <class RM>
__device__ __forceinline__ void hl_load_state(const float* __restrict__ state, int sdim, int off, const uint8_t* __restrict__ reset, const RM& R, float* cs,
                                              float* hs, int tid) {
  const int m = tid >> 5, j = tid & 31, r = R.srow(m);
  const bool live = R.live(m) && !(reset && reset[R.row(m)]);
  cs[j * POL_M + m] = live ? state[(long)r * sdim + off + j] : 0.0f;
  hs[j * POL_M + m] = live ? state[(long)r * sdim + off + 32 + j] : 0.0f;
}

// tpolicies lstm_embed_block, one step (oracle/epmc_policy.py): x [256][16] k-major in `x`; weights k0 .. k0+8 = wx, wh, b, beta_x, gamma_x,
// beta_h, gamma_h, beta_c, gamma_c.  zbuf: 256 x 16 floats of scratch.  Leaves c', h' in cs, hs and in the state buffer; returns h'_j of
// this lane's (row, unit).  Starts and ends at a barrier.  ONCHIP (the scorer, hl_score.inc): c', h' stay in cs, hs alone and `state` is not touched.
template <bool ONCHIP = false, class WT, class RM>
__device__ __forceinline__ float hl_lstm(const WT& W, int k0, const float* x, float* zbuf, float* cs, float* hs, float* __restrict__ state, int sdim, int off,
                                         const RM& R, int wave, int lane, int tid) {
  pol_dense(x, 256, W.a[k0], W.zero, 128, zbuf, 0, wave, lane);                     // x Wx   rows 0..127
  pol_dense(hs, 32, W.a[k0 + 1], W.zero, 128, zbuf + 128 * POL_M, 0, wave, lane);    // h Wh   rows 128..255
  __syncthreads();
  const int m = tid >> 5, j = tid & 31, r = R.srow(m);
  float zx[4], zh[4];
#pragma unroll
  for (int g = 0; g < 4; g++) { zx[g] = zbuf[(32 * g + j) * POL_M + m]; zh[g] = zbuf[(128 + 32 * g + j) * POL_M + m]; }
  const float mx = hl_sum32(zx[0] + zx[1] + zx[2] + zx[3]) * (1.0f / 128.0f), mh = hl_sum32(zh[0] + zh[1] + zh[2] + zh[3]) * (1.0f / 128.0f);
  float vx = 0.0f, vh = 0.0f;
#pragma unroll
  for (int g = 0; g < 4; g++) { vx += (zx[g] - mx) * (zx[g] - mx); vh += (zh[g] - mh) * (zh[g] - mh); }
  const float rx = rsqrtf(hl_sum32(vx) * (1.0f / 128.0f) + 1e-12f), rh = rsqrtf(hl_sum32(vh) * (1.0f / 128.0f) + 1e-12f);
  float z[4];
#pragma unroll
  for (int g = 0; g < 4; g++) {
    const int n = 32 * g + j;
    z[g] = ((zx[g] - mx) * rx * W.a[k0 + 4][n] + W.a[k0 + 3][n]) + ((zh[g] - mh) * rh * W.a[k0 + 6][n] + W.a[k0 + 5][n]) + W.a[k0 + 2][n];
  }
  const float c = hl_sigmoid(z[1] + 1.0f) * cs[j * POL_M + m] + hl_sigmoid(z[0]) * tanhf(z[3]);       // i, f, o, u; forget bias 1.0
  const float mc = hl_sum32(c) * (1.0f / 32.0f);
  const float rc = rsqrtf(hl_sum32((c - mc) * (c - mc)) * (1.0f / 32.0f) + 1e-12f);
  const float h = hl_sigmoid(z[2]) * tanhf((c - mc) * rc * W.a[k0 + 8][j] + W.a[k0 + 7][j]);
  cs[j * POL_M + m] = c;
  hs[j * POL_M + m] = h;
  if constexpr (!ONCHIP) {
    if (R.live(m)) { state[(long)r * sdim + off + j] = c; state[(long)r * sdim + off + 32 + j] = h; }
  }
  __syncthreads();
  return h;
}

// PPO actor draws (ll_hl_policy_act_pg): key (seed lo, seed hi), counter (row * G + g, step lo, step hi, salt), one salt per head
#define HL_HEADING_SALT 0x4EAD1Cu    // SEPMC heading: G 1, the first Box-Muller normal of the block
#define HL_Z_SALT 0x2C0DE5u          // z code: G 64, word j of block g perturbs code 4 g + j
#define HL_LLC_SALT 0x11C5A7u        // low-level action: G 3, four normals per block (as policy_noise)
#define HL_LOG_2PI 1.8378770664093453f

// four standard normals of one Philox block, formed as policy_noise (pmc_policy.inc) forms them
__device__ __forceinline__ void hl_normals4(uint64_t seed, uint64_t step, uint32_t ctr, uint32_t salt, float* eps) {
  uint32_t r[4];
  philox4x32(ctr, (uint32_t)step, (uint32_t)(step >> 32), salt, (uint32_t)seed, (uint32_t)(seed >> 32), r);
  const float k = 2.3283064365386963e-10f;   // 2^-32
  const float u1 = fminf(((float)r[0] + 1.0f) * k, 1.0f), u2 = (float)r[1] * k, u3 = fminf(((float)r[2] + 1.0f) * k, 1.0f), u4 = (float)r[3] * k;
  const float m1 = sqrtf(-2.0f * logf(u1)), m2 = sqrtf(-2.0f * logf(u3));
  eps[0] = m1 * cosf(6.283185307179586f * u2); eps[1] = m1 * sinf(6.283185307179586f * u2);
  eps[2] = m2 * cosf(6.283185307179586f * u4); eps[3] = m2 * sinf(6.283185307179586f * u4);
}

// Gumbel noise -log(-log u) of the 24-bit open-interval uniform u = ((w >> 8) + 0.5) 2^-24.  u is never rounded: below 1/2 it is exact in
// float32 and -log u = -logf(u); above, 1 - u = ((2^24 - 1 - (w >> 8)) + 0.5) 2^-24 is exact and -log u = -log1pf(-(1 - u)).
__device__ __forceinline__ float hl_gumbel(uint32_t w) {
  const uint32_t k = w >> 8;
  const float t = k < (1u << 23) ? -logf(((float)k + 0.5f) * 5.9604644775390625e-8f)
                                 : -log1pf(-(((float)(0xFFFFFFu - k) + 0.5f) * 5.9604644775390625e-8f));
  return -logf(t);
}

// what the PG launch hands the mid level: draws, the neglogp output and its column count, LDS for the z logits' logsumexp
struct HlPg {
  uint64_t seed, step;
  int sample, nh;
  float* neglogp;
  float *pm, *ps;      // [16][16]: per-part max and sum of exp of the z logits
};

// what the scoring launch (hl_score.inc) hands the policy chain in place of draws: the recorded heads of one time step and where their neglogp and
// entropy go.  Row r's A field ([heading (SEPMC)] | z code | action[12]) is a + r * astride, its output row (LLS_OUT_FLOATS columns: neglogp[nh] |
// entropy[nh] | ..) out + r * ostride.  hcs, hhs: LDS [32][16], SEPMC's high-level LSTM state (the mid level's own lives in HlLds::cs, hs).
struct HlFed {
  const float* a;
  float* out;
  long astride, ostride;
  float *hcs, *hhs;
};

struct HlLds {
  float big[2 * 256 * POL_M];   // two activation buffers b0 | b1; the percept stacks' intermediate maps while those run
  float xs[136 * POL_M];        // normalised prop (135)
  float feat[128 * POL_M];      // the percept features (and the vector feature in front of them)
  float cs[32 * POL_M], hs[32 * POL_M];
  float vin[32 * POL_M];        // SEPMC: percept_vec | oppo_info | flag_info | with_flag (29); the 3-value target in rows 0..2 for the mid level
  float pv[16 * POL_M];
  int pi[16 * POL_M];
  int best[POL_M];
};

// The mid level (EPMC's whole policy; SEPMC's mlc_encoder and llc) with the EPMC checkpoint's array numbers; the SEPMC arrays are OFF = 50
// further on.  On entry: xs, and the target [3][16] in L.vin.  Writes actions / code of the map's rows.
// PG: the PPO actor's heads (HlPg): the code and the action sampled when g.sample, neglogp of both when g.neglogp.
// FED (with PG; the scorer, hl_score.inc): nothing is chosen or drawn.  The z code and the action are the recorded ones of HlFed, the controller runs at
// that code, and neglogp and entropy of both heads go to HlFed::out; the LSTM state is what L.cs, L.hs hold on entry and stays there (state, reset,
// actions, code_out: unused).  A code outside 0..255 reads nothing out of range and makes the four values of that row NaN.
template <int OFF, bool PG = false, bool FED = false, class WT, class RM>
__device__ __forceinline__ void hl_mid(const WT& W, HlLds& L, const float* __restrict__ obs, int stride, const uint8_t* __restrict__ reset, float* __restrict__ state,
                                       int sdim, int soff, float* __restrict__ actions, int32_t* __restrict__ code_out, const RM& R, int wave, int lane, int tid,
                                       const HlPg& g = HlPg(), const HlFed& f = HlFed()) {
  static_assert(PG || !FED, "the fed heads are the PPO actor's");
  constexpr int AZ = OFF ? 1 : 0;                                                                  // the z code's column of A: behind SEPMC's heading
  float *b0 = L.big, *b1 = L.big + 256 * POL_M;
  if constexpr (!FED) hl_load_state(state, sdim, soff, reset, R, L.cs, L.hs, tid);
  hl_percepts(W, OFF + 49, obs, stride, R, L.big, L.feat, 32, tid);                                // usr_cmd_encoder: e2d | e1d | efr at 32..119
  pol_dense(L.vin, 3, W.a[OFF + 73], W.a[OFF + 74], 32, L.feat, 1, wave, lane);                   //                  vec at 0..31
  pol_dense(L.xs, 135, W.a[OFF + 47], W.a[OFF + 48], 64, b1, 1, wave, lane);                      // mlc_encoder prop embed: rows 0..63
  __syncthreads();
  pol_dense(L.feat, 120, W.a[OFF + 75], W.a[OFF + 76], 64, b1 + 64 * POL_M, 1, (wave + 4) & 7, lane);   // usr: rows 64..127 (the other four waves)
  __syncthreads();
  pol_dense(b1, 128, W.a[OFF + 77], W.a[OFF + 78], 256, b0, 1, wave, lane);                      // embed
  __syncthreads();
  hl_lstm<FED>(W, OFF + 79, b0, b1, L.cs, L.hs, state, sdim, soff, R, wave, lane, tid);
  pol_dense(L.hs, 32, W.a[OFF + 88], W.a[OFF + 89], 256, b0, 0, wave, lane);                     // z logits
  __syncthreads();
  if constexpr (FED) {  // max and sum of exp of 16 logits in the PG branch's order, and (in L.pv, which holds no maximum here) the sum of exp x logit for the entropy
    if (tid < 256) {
      const int m = tid & 15, part = tid >> 4;
      float mx = -3.0e38f, se = 0.0f, sw = 0.0f;
      for (int q = 0; q < 16; q++) mx = fmaxf(mx, b0[(part * 16 + q) * POL_M + m]);
      for (int q = 0; q < 16; q++) {
        const float v = b0[(part * 16 + q) * POL_M + m], e = expf(v - mx);
        se += e;
        sw += e * v;
      }
      g.pm[part * POL_M + m] = mx; g.ps[part * POL_M + m] = se; L.pv[part * POL_M + m] = sw;
    }
  } else if constexpr (PG) {   // first maximum of logit (+ Gumbel noise when sampling) per row; max and sum of exp of 16 logits for the logsumexp
    if (tid < 256) {
      const int m = tid & 15, part = tid >> 4;
      float mx = -3.0e38f, se = 0.0f, bv = -3.0e38f;
      int bi = 0;
      for (int q = 0; q < 16; q++) mx = fmaxf(mx, b0[(part * 16 + q) * POL_M + m]);
      for (int blk = 0; blk < 4; blk++) {
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        if (g.sample)
          philox4x32((uint32_t)R.row(m) * 64u + (uint32_t)(part * 4 + blk), (uint32_t)g.step, (uint32_t)(g.step >> 32), HL_Z_SALT, (uint32_t)g.seed,
                     (uint32_t)(g.seed >> 32), w);
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const int c = part * 16 + blk * 4 + q;
          const float v = b0[c * POL_M + m];
          se += expf(v - mx);
          const float pv = g.sample ? v + hl_gumbel(w[q]) : v;
          if (pv > bv) { bv = pv; bi = c; }
        }
      }
      L.pv[part * POL_M + m] = bv; L.pi[part * POL_M + m] = bi;
      g.pm[part * POL_M + m] = mx; g.ps[part * POL_M + m] = se;
    }
  } else {   // first maximum over the 256 logits of each row (as in pmc_policy_kernel)
    const int m = tid & 15, part = (tid >> 4) & 15;
    float bv = -3.0e38f;
    int bi = 0;
    for (int q = 0; q < 16; q++) {
      const int c = part * 16 + q;
      const float v = b0[c * POL_M + m];
      if (v > bv) { bv = v; bi = c; }
    }
    if (tid < 256) { L.pv[part * POL_M + m] = bv; L.pi[part * POL_M + m] = bi; }
  }
  __syncthreads();
  if constexpr (FED) {
    if (tid < POL_M) {                                                                            // the recorded code; L.pi[row]: it is one
      const bool live = R.live(tid);
      const float cf = live ? f.a[(long)R.row(tid) * f.astride + AZ] : 0.0f;
      const bool ok = cf >= 0.0f && cf < 256.0f;                                                  // (a NaN is neither)
      const int bi = ok ? (int)cf : 0;
      L.best[tid] = bi;
      L.pi[tid] = ok ? 1 : 0;
      if (live) {                                                                                 // logsumexp as below; entropy = logsumexp - sum softmax x logit
        float mx = g.pm[tid];
        for (int p = 1; p < 16; p++) mx = fmaxf(mx, g.pm[p * POL_M + tid]);
        float se = 0.0f, sw = 0.0f;
        for (int p = 0; p < 16; p++) {
          const float w = expf(g.pm[p * POL_M + tid] - mx);
          se += g.ps[p * POL_M + tid] * w;
          sw += L.pv[p * POL_M + tid] * w;
        }
        const float lse = mx + logf(se), nan = __builtin_nanf("");
        float* o = f.out + (long)R.row(tid) * f.ostride;
        o[g.nh - 2] = ok ? lse - b0[bi * POL_M + tid] : nan;
        o[2 * g.nh - 2] = ok ? lse - sw / se : nan;
      }
    }
  } else if (tid < POL_M) {
    float bv = L.pv[tid];
    int bi = L.pi[tid];
    for (int p = 1; p < 16; p++)
      if (L.pv[p * POL_M + tid] > bv) { bv = L.pv[p * POL_M + tid]; bi = L.pi[p * POL_M + tid]; }
    L.best[tid] = bi;
    if (code_out && R.live(tid)) code_out[R.row(tid)] = bi;
    if constexpr (PG) {
      if (g.neglogp && R.live(tid)) {                                                           // logsumexp(logits) - logits[code]
        float mx = g.pm[tid];
        for (int p = 1; p < 16; p++) mx = fmaxf(mx, g.pm[p * POL_M + tid]);
        float se = 0.0f;
        for (int p = 0; p < 16; p++) se += g.ps[p * POL_M + tid] * expf(g.pm[p * POL_M + tid] - mx);
        g.neglogp[(long)R.row(tid) * g.nh + g.nh - 2] = mx + logf(se) - b0[bi * POL_M + tid];
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < 32 * POL_M; i += POL_THREADS) {                                          // zq = w90.T[code]: rows 96..127 of b1
    const int k = i >> 4, m = i & 15;
    b1[(96 + k) * POL_M + m] = W.a[OFF + 90][k * 256 + L.best[m]];
  }
  __syncthreads();
  pol_dense(L.xs, 135, W.a[OFF + 91], W.a[OFF + 92], 64, b0, 1, wave, lane);                     // llc: relu(prop) rows 0..63
  pol_dense(b1 + 96 * POL_M, 32, W.a[OFF + 93], W.a[OFF + 94], 32, b0 + 64 * POL_M, 1, (wave + 4) & 7, lane);   // relu(zq) rows 64..95
  __syncthreads();
  pol_dense(b0, 96, W.a[OFF + 95], W.a[OFF + 96], 256, b1, 1, wave, lane);
  __syncthreads();
  pol_dense(b1, 256, W.a[OFF + 97], W.a[OFF + 98], 256, b0, 1, wave, lane);
  __syncthreads();
  pol_dense(b0, 256, W.a[OFF + 99], W.a[OFF + 100], 12, b1, 0, wave, lane);                      // mean action: rows 0..11 of b1
  __syncthreads();
  if constexpr (FED) {
    if (tid < 64) {     // as below with eps = (a - mean) / exp(logstd) of the recorded action; entropy = 6 (1 + log 2 pi) + sum logstd
      const int grp = lane >> 4, m = lane & 15;
      const bool live = R.live(m);
      const float* a = f.a + (long)R.row(m) * f.astride + AZ + 1;
      float nl = 0.0f, sl = 0.0f;
      if (grp < 3) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const int c = 4 * grp + q;
          const float ls = W.a[OFF + 101][c];
          const float eps = ((live ? a[c] : 0.0f) - b1[c * POL_M + m]) / expf(ls);
          nl += 0.5f * eps * eps + ls;
          sl += ls;
        }
      }
      nl += __shfl(nl, lane + 16) + __shfl(nl, lane + 32);
      sl += __shfl(sl, lane + 16) + __shfl(sl, lane + 32);
      if (grp == 0 && live) {
        float* o = f.out + (long)R.row(m) * f.ostride;
        const bool ok = L.pi[m] != 0;
        o[g.nh - 1] = ok ? nl + 0.5f * HL_LOG_2PI * LLH_ACT_DIM : __builtin_nanf("");
        o[2 * g.nh - 1] = ok ? sl + 0.5f * (1.0f + HL_LOG_2PI) * LLH_ACT_DIM : __builtin_nanf("");
      }
    }
  } else if constexpr (PG) {
    if (tid < 64) {     // wavefront 0, lane = group * 16 + row: a = mean + exp(logstd) eps (logstd: array OFF + 101), neglogp summed over the groups
      const int grp = lane >> 4, m = lane & 15, r = R.row(m);
      const bool live = R.live(m);
      float eps[4] = {0.0f, 0.0f, 0.0f, 0.0f}, nl = 0.0f;
      if (grp < 3) {
        if (g.sample) hl_normals4(g.seed, g.step, (uint32_t)r * 3u + (uint32_t)grp, HL_LLC_SALT, eps);
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const int c = 4 * grp + q;
          const float ls = W.a[OFF + 101][c];
          if (live) actions[(long)r * LLH_ACT_DIM + c] = b1[c * POL_M + m] + expf(ls) * eps[q];
          nl += 0.5f * eps[q] * eps[q] + ls;
        }
      }
      nl += __shfl(nl, lane + 16) + __shfl(nl, lane + 32);
      if (g.neglogp && grp == 0 && live) g.neglogp[(long)r * g.nh + g.nh - 1] = nl + 0.5f * HL_LOG_2PI * LLH_ACT_DIM;
    }
  } else {
    for (int i = tid; i < POL_M * LLH_ACT_DIM; i += POL_THREADS) {
      const int m = i / LLH_ACT_DIM, c = i - m * LLH_ACT_DIM;
      if (R.live(m)) actions[(long)R.row(m) * LLH_ACT_DIM + c] = b1[c * POL_M + m];
    }
  }
}

template <int KIND>
__global__ __launch_bounds__(POL_THREADS) void hl_policy_kernel(HlW W, const float* __restrict__ obs, int stride, const uint8_t* __restrict__ reset,
                                                                float* __restrict__ state, float* __restrict__ actions, int32_t* __restrict__ code_out,
                                                                float* __restrict__ heading_out, int n_rows) {
  __shared__ HlLds L;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const HlDense R = {(int)blockIdx.x * POL_M, n_rows};
  for (int i = tid; i < POL_M * 135; i += POL_THREADS) {        // rms normalisation + clip to +-5 (layers.py:55)
    const int m = i / 135, k = i - m * 135, r = R.row(m);
    const float x = R.live(m) ? obs[(long)r * stride + k] : 0.0f;
    L.xs[k * POL_M + m] = fminf(fmaxf((x - W.a[0][k]) / (W.a[1][k] + 1e-8f), -5.0f), 5.0f);
  }
  if (KIND == LLH_EPMC) {
    if (tid < 3 * POL_M) {                                       // target (913..915)
      const int k = tid >> 4, m = tid & 15, r = R.row(m);
      L.vin[k * POL_M + m] = R.live(m) ? obs[(long)r * stride + 913 + k] : 0.0f;
    }
    __syncthreads();
    hl_mid<0>(W, L, obs, stride, reset, state, 64, 0, actions, code_out, R, wave, lane, tid);
  } else {
    float *b0 = L.big, *b1 = L.big + 256 * POL_M;
    if (tid < 29 * POL_M) {                                      // percept_vec 913..917 | oppo_info 918..932 | flag_info 948..954 | with_flag 962..963
      const int k = tid >> 4, m = tid & 15, r = R.row(m);
      const int col = k < 20 ? 913 + k : (k < 27 ? 948 + k - 20 : 962 + k - 27);
      L.vin[k * POL_M + m] = R.live(m) ? obs[(long)r * stride + col] : 0.0f;
    }
    hl_load_state(state, 128, 0, reset, R, L.cs, L.hs, tid);
    __syncthreads();
    hl_percepts(W, 53, obs, stride, R, L.big, L.feat, 0, tid);                        // hlc_encoder percepts -> feat 0..87
    pol_dense(L.xs, 135, W.a[51], W.a[52], 64, b1, 1, wave, lane);                      // embed input: prop 0..63 | percepts 64..127 | vector 128..191
    pol_dense(L.feat, 88, W.a[77], W.a[78], 64, b1 + 64 * POL_M, 1, (wave + 4) & 7, lane);
    pol_dense(L.vin, 29, W.a[79], W.a[80], 64, b0, 1, wave, lane);
    __syncthreads();
    pol_dense(b0, 64, W.a[81], W.a[82], 64, b1 + 128 * POL_M, 1, (wave + 4) & 7, lane);
    __syncthreads();
    pol_dense(b1, 192, W.a[83], W.a[84], 256, b0, 1, wave, lane);
    __syncthreads();
    const float h = hl_lstm(W, 85, b0, b1, L.cs, L.hs, state, 128, 0, R, wave, lane, tid);
    const int m = tid >> 5, j = tid & 31, r = R.row(m);
    const float hd = fminf(fmaxf(hl_sum32(h * W.a[94][j]) + W.a[95][0], -HL_PI), HL_PI);   // the Gaussian head's mean, clipped to +-pi
    if (j == 0) {                                                                       // the mid level's target: cos, sin, control_spd
      L.vin[0 * POL_M + m] = cosf(hd);
      L.vin[1 * POL_M + m] = sinf(hd);
      L.vin[2 * POL_M + m] = R.live(m) ? obs[(long)r * stride + 964] : 0.0f;
      if (heading_out && R.live(m)) heading_out[r] = hd;
    }
    __syncthreads();
    hl_mid<50>(W, L, obs, stride, reset, state, 128, 64, actions, code_out, R, wave, lane, tid);
  }
}

// The value branch's view of the policy kernel's LDS (a union with HlLds in the PG launch): a 512-row and a 256-row activation buffer.
struct HlVLds {
  float a[512 * POL_M];         // the percept stacks' intermediate maps, then the dense layers' outputs; the LSTM's scratch
  float b[256 * POL_M];         // percept features (rows 0..119), normalised prop (rows 120..255); then the LSTM input
  float cs[32 * POL_M], hs[32 * POL_M];
  float vin[32 * POL_M];        // EPMC: target (3); SEPMC: percept_vec | oppo_info_cheat | flag_info_cheat | with_flag (29)
};

struct HlPgLds {
  union {
    HlLds P;
    HlVLds V;
  } u;
  float pm[16 * POL_M], ps[16 * POL_M];
};

// The value branch (epmc_net.py:226-244, sepmc_net.py:271-292) of 16 rows on the checkpoint's arrays 2..46 (EPMC) / 2..50 (SEPMC); its LSTM
// state [max_rows][64] (c | h) in vstate, zeroed by reset like the policy's.  value[R.srow(m)] <- the value of the map's rows.
// ONCHIP (the scorer, hl_score.inc): the state is what V.cs, V.hs hold on entry and stays there (vstate, reset: unused).
template <int KIND, bool ONCHIP = false, class WT, class RM>
__device__ __forceinline__ void hl_value(const WT& W, HlVLds& V, const float* __restrict__ obs, int stride, const uint8_t* __restrict__ reset,
                                         float* __restrict__ vstate, float* __restrict__ value, const RM& R, int wave, int lane, int tid) {
  float *a = V.a, *b = V.b, *xs = V.b + 120 * POL_M;
  for (int i = tid; i < POL_M * 135; i += POL_THREADS) {        // the policy's rms normalisation (arrays 0, 1)
    const int m = i / 135, k = i - m * 135, r = R.row(m);
    const float x = R.live(m) ? obs[(long)r * stride + k] : 0.0f;
    xs[k * POL_M + m] = fminf(fmaxf((x - W.a[0][k]) / (W.a[1][k] + 1e-8f), -5.0f), 5.0f);
  }
  if (KIND == LLH_EPMC) {
    if (tid < 3 * POL_M) {                                       // target (913..915)
      const int k = tid >> 4, m = tid & 15, r = R.row(m);
      V.vin[k * POL_M + m] = R.live(m) ? obs[(long)r * stride + 913 + k] : 0.0f;
    }
  } else if (tid < 29 * POL_M) {                                 // percept_vec 913..917 | oppo_info_cheat 933..947 | flag_info_cheat 955..961 | with_flag 962..963
    const int k = tid >> 4, m = tid & 15, r = R.row(m);
    const int col = k < 5 ? 913 + k : (k < 20 ? 933 + k - 5 : (k < 27 ? 955 + k - 20 : 962 + k - 27));
    V.vin[k * POL_M + m] = R.live(m) ? obs[(long)r * stride + col] : 0.0f;
  }
  if constexpr (!ONCHIP) hl_load_state(vstate, 64, 0, reset, R, V.cs, V.hs, tid);
  __syncthreads();
  float h;
  int kv;
  if (KIND == LLH_EPMC) {
    hl_percepts(W, 4, obs, stride, R, a, b, 32, tid);                              // usr_cmd_encoder: e2d | e1d | efr -> b rows 32..119
    pol_dense(V.vin, 3, W.a[28], W.a[29], 32, b, 1, wave, lane);                     //                  vec -> b rows 0..31
    pol_dense(xs, 135, W.a[2], W.a[3], 128, a + 128 * POL_M, 2, wave, lane);         // fc1, tanh -> a rows 128..255
    __syncthreads();
    pol_dense(b, 120, W.a[30], W.a[31], 64, a, 1, wave, lane);                       // bottleneck -> a rows 0..63
    __syncthreads();
    pol_dense(a, 64, W.a[32], W.a[33], 128, a + 256 * POL_M, 2, wave, lane);         // fc2, tanh -> a rows 256..383
    __syncthreads();
    pol_dense(a + 128 * POL_M, 256, W.a[34], W.a[35], 256, b, 2, wave, lane);        // fc3 of [fc1 | fc2], tanh -> b
    __syncthreads();
    h = hl_lstm<ONCHIP>(W, 36, b, a, V.cs, V.hs, vstate, 64, 0, R, wave, lane, tid);
    kv = 45;
  } else {
    hl_percepts(W, 4, obs, stride, R, a, b, 0, tid);                               // mlc_usr_cmd_encoder: e2d | e1d | efr -> b rows 0..87
    pol_dense(b, 88, W.a[28], W.a[29], 64, a, 1, wave, lane);                        // bottleneck -> a rows 0..63
    pol_dense(V.vin, 29, W.a[32], W.a[33], 64, a + 64 * POL_M, 1, (wave + 4) & 7, lane);   // hlc_usr_cmd_encoder 1 -> a rows 64..127
    pol_dense(xs, 135, W.a[2], W.a[3], 128, a + 128 * POL_M, 2, wave, lane);         // fc1, tanh -> a rows 128..255
    __syncthreads();
    pol_dense(a, 64, W.a[30], W.a[31], 128, a + 256 * POL_M, 2, wave, lane);         // fc2, tanh -> a rows 256..383
    pol_dense(a + 64 * POL_M, 64, W.a[34], W.a[35], 64, b, 1, (wave + 4) & 7, lane); // hlc_usr_cmd_encoder 2 -> b rows 0..63
    __syncthreads();
    pol_dense(b, 64, W.a[36], W.a[37], 128, a + 384 * POL_M, 2, wave, lane);         // fc3, tanh -> a rows 384..511
    __syncthreads();
    pol_dense(a + 128 * POL_M, 384, W.a[38], W.a[39], 256, b, 2, wave, lane);        // fc4 of [fc1 | fc2 | fc3], tanh -> b
    __syncthreads();
    h = hl_lstm<ONCHIP>(W, 40, b, a, V.cs, V.hs, vstate, 64, 0, R, wave, lane, tid);
    kv = 49;
  }
  const int m = tid >> 5, j = tid & 31;
  const float v = hl_sum32(h * W.a[kv][j]) + W.a[kv + 1][0];                         // value dense, linear
  if (j == 0 && R.live(m)) value[R.srow(m)] = v;
}

// The policy of hl_policy_kernel with its heads sampled / scored (HlPg) for the 16 rows of R: what blockIdx.y 0 of the PPO actor launch runs.
// FED (the scorer, hl_score.inc): one time step of a recorded unroll.  The heads are those of HlFed (hl_mid), the mid level's target is the recorded
// heading, and the LSTM states are what L.cs, L.hs and f.hcs, f.hhs hold on entry and stay there; of the pointers, only obs is used.
template <int KIND, bool FED = false, class WT, class RM>
__device__ __forceinline__ void hl_pg_policy(const WT& W, const RM& R, HlPgLds& S, const float* __restrict__ obs, int stride, const uint8_t* __restrict__ reset,
                                             float* __restrict__ state, float* __restrict__ actions, int32_t* __restrict__ code_out, float* __restrict__ heading_out,
                                             float* __restrict__ neglogp, uint64_t seed, uint64_t step, int sample, int wave, int lane, int tid,
                                             const HlFed& f = HlFed()) {
  HlLds& L = S.u.P;
  HlPg g;
  g.seed = seed; g.step = step; g.sample = sample; g.neglogp = neglogp; g.pm = S.pm; g.ps = S.ps;
  g.nh = KIND == LLH_EPMC ? LLH_EPMC_N_HEADS : LLH_SEPMC_N_HEADS;
  for (int i = tid; i < POL_M * 135; i += POL_THREADS) {        // rms normalisation + clip to +-5 (layers.py:55)
    const int m = i / 135, k = i - m * 135, r = R.row(m);
    const float x = R.live(m) ? obs[(long)r * stride + k] : 0.0f;
    L.xs[k * POL_M + m] = fminf(fmaxf((x - W.a[0][k]) / (W.a[1][k] + 1e-8f), -5.0f), 5.0f);
  }
  if (KIND == LLH_EPMC) {
    if (tid < 3 * POL_M) {                                       // target (913..915)
      const int k = tid >> 4, m = tid & 15, r = R.row(m);
      L.vin[k * POL_M + m] = R.live(m) ? obs[(long)r * stride + 913 + k] : 0.0f;
    }
    __syncthreads();
    hl_mid<0, true, FED>(W, L, obs, stride, reset, state, 64, 0, actions, code_out, R, wave, lane, tid, g, f);
  } else {
    float *b0 = L.big, *b1 = L.big + 256 * POL_M;
    if (tid < 29 * POL_M) {                                      // percept_vec 913..917 | oppo_info 918..932 | flag_info 948..954 | with_flag 962..963
      const int k = tid >> 4, m = tid & 15, r = R.row(m);
      const int col = k < 20 ? 913 + k : (k < 27 ? 948 + k - 20 : 962 + k - 27);
      L.vin[k * POL_M + m] = R.live(m) ? obs[(long)r * stride + col] : 0.0f;
    }
    if constexpr (!FED) hl_load_state(state, 128, 0, reset, R, L.cs, L.hs, tid);
    __syncthreads();
    hl_percepts(W, 53, obs, stride, R, L.big, L.feat, 0, tid);
    pol_dense(L.xs, 135, W.a[51], W.a[52], 64, b1, 1, wave, lane);
    pol_dense(L.feat, 88, W.a[77], W.a[78], 64, b1 + 64 * POL_M, 1, (wave + 4) & 7, lane);
    pol_dense(L.vin, 29, W.a[79], W.a[80], 64, b0, 1, wave, lane);
    __syncthreads();
    pol_dense(b0, 64, W.a[81], W.a[82], 64, b1 + 128 * POL_M, 1, (wave + 4) & 7, lane);
    __syncthreads();
    pol_dense(b1, 192, W.a[83], W.a[84], 256, b0, 1, wave, lane);
    __syncthreads();
    const float h = hl_lstm<FED>(W, 85, b0, b1, FED ? f.hcs : L.cs, FED ? f.hhs : L.hs, state, 128, 0, R, wave, lane, tid);
    const int m = tid >> 5, j = tid & 31, r = R.row(m);
    const float mu = fminf(fmaxf(hl_sum32(h * W.a[94][j]) + W.a[95][0], -HL_PI), HL_PI);   // the Gaussian head's mean, clipped to +-pi
    if constexpr (FED) {
      if (j == 0) {   // eps = (heading - mu) / exp(a96) of the recorded heading, which is the mid level's target; entropy = 0.5 (1 + log 2 pi) + a96
        const bool live = R.live(m);
        const float ls = W.a[96][0], hd = live ? f.a[(long)r * f.astride] : 0.0f, eps = (hd - mu) / expf(ls);
        L.vin[0 * POL_M + m] = cosf(hd);
        L.vin[1 * POL_M + m] = sinf(hd);
        L.vin[2 * POL_M + m] = live ? obs[(long)r * stride + 964] : 0.0f;
        if (live) {
          float* o = f.out + (long)r * f.ostride;
          o[0] = 0.5f * eps * eps + 0.5f * HL_LOG_2PI + ls;
          o[LLH_SEPMC_N_HEADS] = 0.5f * (1.0f + HL_LOG_2PI) + ls;
        }
      }
    } else if (j == 0) {   // heading = mu + exp(a96) eps, not clipped (a96, 'logvar' in sepmc_net.py, is the DiagGaussian's logstd half); the mid level's target
      float eps[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      if (sample) hl_normals4(seed, step, (uint32_t)r, HL_HEADING_SALT, eps);
      const float ls = W.a[96][0], hd = mu + expf(ls) * eps[0];
      L.vin[0 * POL_M + m] = cosf(hd);
      L.vin[1 * POL_M + m] = sinf(hd);
      L.vin[2 * POL_M + m] = R.live(m) ? obs[(long)r * stride + 964] : 0.0f;
      if (heading_out && R.live(m)) heading_out[r] = hd;
      if (neglogp && R.live(m)) neglogp[(long)r * LLH_SEPMC_N_HEADS] = 0.5f * eps[0] * eps[0] + 0.5f * HL_LOG_2PI + ls;
    }
    __syncthreads();
    hl_mid<50, true, FED>(W, L, obs, stride, reset, state, 128, 64, actions, code_out, R, wave, lane, tid, g, f);
  }
}

// The PPO actor launch: blockIdx.y 0 = hl_pg_policy; blockIdx.y 1 (launched only when a value is asked for) = the value branch of the same rows.
// Neither waits on the other.
template <int KIND>
__global__ __launch_bounds__(POL_THREADS) void hl_policy_pg_kernel(HlW W, const float* __restrict__ obs, int stride, const uint8_t* __restrict__ reset,
                                                                   float* __restrict__ state, float* __restrict__ vstate, float* __restrict__ actions,
                                                                   int32_t* __restrict__ code_out, float* __restrict__ heading_out, float* __restrict__ neglogp,
                                                                   float* __restrict__ value, uint64_t seed, uint64_t step, int sample, int n_rows) {
  __shared__ HlPgLds S;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const HlDense R = {(int)blockIdx.x * POL_M, n_rows};
  if (blockIdx.y == 1) {
    hl_value<KIND>(W, S.u.V, obs, stride, reset, vstate, value, R, wave, lane, tid);
    return;
  }
  hl_pg_policy<KIND>(W, R, S, obs, stride, reset, state, actions, code_out, heading_out, neglogp, seed, step, sample, wave, lane, tid);
}

struct ll_hl_policy {
  int kind, device, max_rows, state_dim;
  float *d_w, *d_state;
  float *d_vw, *d_vstate;        // the value branch (ll_hl_policy_attach_value) and its state [max_rows][64]; null until attached
  HlW W;
  float* h_stage;                // pinned [n_floats + n_vf_floats]: what ll_hl_policy_set_weights uploads from; null until its first call
  hipEvent_t up_ev;              // the last upload from h_stage
  bool up_pending;
  bool timing;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> evs;
  size_t ev_used;
};

// array sizes of the mid level, EPMC numbers 47..101 (SEPMC 97..151), and of SEPMC's high level 51..96
static const int HL_MID_SIZES[55] = {8640, 64, 4, 4, 256, 4, 64, 4, 16, 1, 16, 4, 64, 4, 64, 4, 16, 1, 4, 4, 256, 4, 64, 4, 16, 1, 96, 32,
                                     7680, 64, 32768, 256, 32768, 4096, 128, 128, 128, 128, 128, 32, 32, 8192, 256, 8192, 8640, 64, 1024, 32,
                                     24576, 256, 65536, 256, 3072, 12, 12};
static const int HL_HLC_SIZES[46] = {8640, 64, 4, 4, 256, 4, 64, 4, 16, 1, 16, 4, 64, 4, 64, 4, 16, 1, 4, 4, 256, 4, 64, 4, 16, 1,
                                     5632, 64, 1856, 64, 4096, 64, 49152, 256, 32768, 4096, 128, 128, 128, 128, 128, 32, 32, 32, 1, 1};

// array sizes of the value branches: EPMC 2..46, SEPMC 2..50
static const int HL_VF_EPMC_SIZES[45] = {17280, 128, 4, 4, 256, 4, 64, 4, 16, 1, 16, 4, 64, 4, 64, 4, 16, 1, 4, 4, 256, 4, 64, 4, 16, 1, 96, 32, 7680, 64,
                                         8192, 128, 65536, 256, 32768, 4096, 128, 128, 128, 128, 128, 32, 32, 32, 1};
static const int HL_VF_SEPMC_SIZES[49] = {17280, 128, 4, 4, 256, 4, 64, 4, 16, 1, 16, 4, 64, 4, 64, 4, 16, 1, 4, 4, 256, 4, 64, 4, 16, 1, 5632, 64, 8192,
                                          128, 1856, 64, 4096, 64, 8192, 128, 98304, 256, 32768, 4096, 128, 128, 128, 128, 128, 32, 32, 32, 1};

static void hl_check(ll_hl_policy* p) {
  if (!p) throw PmcError(LL_EINVAL, "null policy");
}

extern "C" {

int ll_hl_policy_create(int kind, const float* h_weights, int n_floats, int max_rows, int device, ll_hl_policy** out) {
  LL_TRY
  LL_CHECK(h_weights && out, "null argument");
  *out = nullptr;
  if (kind != LLH_EPMC && kind != LLH_SEPMC) throw PmcError(LL_EINVAL, "kind: LLH_EPMC (1) or LLH_SEPMC (2)");
  const int want = kind == LLH_EPMC ? LLH_EPMC_N_FLOATS : LLH_SEPMC_N_FLOATS;
  if (n_floats != want)
    throw PmcError(LL_EINVAL, kind == LLH_EPMC ? "weights: expected arrays 0, 1, 47..101 of an EPMC checkpoint (208437 floats)"
                                               : "weights: expected arrays 0, 1, 51..151 of the SEPMC checkpoint (316806 floats)");
  if (max_rows <= 0 || max_rows > (1 << 24)) throw PmcError(LL_EINVAL, "max_rows out of range");
  int nd = 0;
  if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) throw PmcError(LL_ENODEV, "no HIP device available: the policy kernel has no CPU fallback");
  if (device < 0 || device >= nd) throw PmcError(LL_EINVAL, "device ordinal out of range");
  HIPCHK(hipSetDevice(device));
  std::vector<int> nums, sizes;                        // checkpoint array number and size, in packing order
  nums.push_back(0); sizes.push_back(135);
  nums.push_back(1); sizes.push_back(135);
  if (kind == LLH_SEPMC)
    for (int i = 0; i < 46; i++) { nums.push_back(51 + i); sizes.push_back(HL_HLC_SIZES[i]); }
  for (int i = 0; i < 55; i++) { nums.push_back((kind == LLH_EPMC ? 47 : 97) + i); sizes.push_back(HL_MID_SIZES[i]); }
  size_t tot = 0;
  for (int s : sizes) tot += (size_t)s;
  if (tot != (size_t)want) throw PmcError(LL_EINVAL, "internal: array size table");
  ll_hl_policy* p = new ll_hl_policy();
  p->kind = kind; p->device = device; p->max_rows = max_rows; p->state_dim = kind == LLH_EPMC ? 64 : 128;
  p->timing = false; p->ev_used = 0; p->d_w = nullptr; p->d_state = nullptr; p->d_vw = nullptr; p->d_vstate = nullptr;
  p->h_stage = nullptr; p->up_ev = nullptr; p->up_pending = false;
  const size_t sbytes = (size_t)max_rows * p->state_dim * sizeof(float);
  if (hipMalloc(&p->d_w, ((size_t)want + 256) * sizeof(float)) != hipSuccess || hipMalloc(&p->d_state, sbytes) != hipSuccess) {
    if (p->d_w) (void)hipFree(p->d_w);
    delete p;
    throw PmcError(LL_ENOMEM, "hipMalloc failed");
  }
  try {
    HIPCHK(hipMemcpy(p->d_w, h_weights, (size_t)want * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(p->d_w + want, 0, 256 * sizeof(float)));
    HIPCHK(hipMemset(p->d_state, 0, sbytes));
    HIPCHK(hipDeviceSynchronize());
  } catch (...) {
    (void)hipFree(p->d_w); (void)hipFree(p->d_state);
    delete p;
    throw;
  }
  for (int i = 0; i < HL_MAX_ARRAY; i++) p->W.a[i] = nullptr;
  size_t off = 0;
  for (size_t i = 0; i < nums.size(); i++) { p->W.a[nums[i]] = p->d_w + off; off += (size_t)sizes[i]; }
  p->W.zero = p->d_w + want;
  *out = p;
  LL_CATCH
}

int ll_hl_policy_destroy(ll_hl_policy* p) {
  LL_TRY
  if (p) {
    (void)hipSetDevice(p->device);
    for (auto& e : p->evs) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    (void)hipFree(p->d_w);
    (void)hipFree(p->d_state);
    if (p->d_vw) (void)hipFree(p->d_vw);
    if (p->d_vstate) (void)hipFree(p->d_vstate);
    if (p->h_stage) { (void)hipDeviceSynchronize(); (void)hipHostFree(p->h_stage); }
    if (p->up_ev) (void)hipEventDestroy(p->up_ev);
    delete p;
  }
  LL_CATCH
}

int ll_hl_policy_state_dim(ll_hl_policy* p) {
  if (!p) return LL_EINVAL;
  return p->state_dim;
}

}  // extern "C"

// the start event of a timed launch (null when timing is off or un-polled timing has stopped recording)
static std::pair<hipEvent_t, hipEvent_t>* hl_timing_begin(ll_hl_policy* p, hipStream_t st) {
  if (!p->timing || p->ev_used >= 16384) return nullptr;
  if (p->ev_used == p->evs.size()) {
    hipEvent_t a, b;
    HIPCHK(hipEventCreate(&a));
    HIPCHK(hipEventCreate(&b));
    p->evs.push_back(std::make_pair(a, b));
  }
  std::pair<hipEvent_t, hipEvent_t>* ev = &p->evs[p->ev_used++];
  HIPCHK(hipEventRecord(ev->first, st));
  return ev;
}

extern "C" {

int ll_hl_policy_act(ll_hl_policy* p, const float* d_obs, int obs_stride, const uint8_t* d_reset, float* d_actions, int32_t* d_code, float* d_heading,
                     int n_rows, void* hip_stream) {
  LL_TRY
  hl_check(p);
  LL_CHECK(d_obs && d_actions, "null argument");
  LL_CHECK(n_rows > 0 && n_rows <= p->max_rows, "n_rows must be 1 .. max_rows");
  LL_CHECK(obs_stride == (p->kind == LLH_EPMC ? LLH_EPMC_OBS_DIM : LLH_SEPMC_OBS_DIM), "obs_stride is not the policy's obs dim (916 EPMC, 965 SEPMC)");
  LL_CHECK(!d_heading || p->kind == LLH_SEPMC, "d_heading: the EPMC policy has no heading");
  HIPCHK(hipSetDevice(p->device));
  hipStream_t st = (hipStream_t)hip_stream;
  std::pair<hipEvent_t, hipEvent_t>* ev = hl_timing_begin(p, st);     // un-polled timing stops recording instead of growing without bound
  const dim3 grid((n_rows + POL_M - 1) / POL_M), block(POL_THREADS);
  if (p->kind == LLH_EPMC)
    hipLaunchKernelGGL(hl_policy_kernel<LLH_EPMC>, grid, block, 0, st, p->W, d_obs, obs_stride, d_reset, p->d_state, d_actions, d_code, d_heading, n_rows);
  else
    hipLaunchKernelGGL(hl_policy_kernel<LLH_SEPMC>, grid, block, 0, st, p->W, d_obs, obs_stride, d_reset, p->d_state, d_actions, d_code, d_heading, n_rows);
  HIPCHK(hipGetLastError());
  if (ev) HIPCHK(hipEventRecord(ev->second, st));
  LL_CATCH
}

int ll_hl_policy_reset_state(ll_hl_policy* p, void* hip_stream) {
  LL_TRY
  hl_check(p);
  HIPCHK(hipSetDevice(p->device));
  HIPCHK(hipMemsetAsync(p->d_state, 0, (size_t)p->max_rows * p->state_dim * sizeof(float), (hipStream_t)hip_stream));
  if (p->d_vstate) HIPCHK(hipMemsetAsync(p->d_vstate, 0, (size_t)p->max_rows * 64 * sizeof(float), (hipStream_t)hip_stream));
  LL_CATCH
}

int ll_hl_policy_attach_value(ll_hl_policy* p, const float* h_vf_weights, int n_floats) {
  LL_TRY
  hl_check(p);
  LL_CHECK(h_vf_weights, "null argument");
  const bool ep = p->kind == LLH_EPMC;
  const int want = ep ? LLH_EPMC_VF_N_FLOATS : LLH_SEPMC_VF_N_FLOATS, n_arr = ep ? 45 : 49;
  const int* sizes = ep ? HL_VF_EPMC_SIZES : HL_VF_SEPMC_SIZES;
  if (n_floats != want)
    throw PmcError(LL_EINVAL, ep ? "value weights: expected arrays 2..46 of an EPMC checkpoint (137872 floats)"
                                 : "value weights: expected arrays 2..50 of the SEPMC checkpoint (182864 floats)");
  size_t tot = 0;
  for (int i = 0; i < n_arr; i++) tot += (size_t)sizes[i];
  if (tot != (size_t)want) throw PmcError(LL_EINVAL, "internal: value array size table");
  HIPCHK(hipSetDevice(p->device));
  HIPCHK(hipDeviceSynchronize());                 // a launch in flight may still read the branch being replaced
  if (!p->d_vw) {
    const size_t sbytes = (size_t)p->max_rows * 64 * sizeof(float);
    if (hipMalloc(&p->d_vw, (size_t)want * sizeof(float)) != hipSuccess) { p->d_vw = nullptr; throw PmcError(LL_ENOMEM, "hipMalloc failed"); }
    if (hipMalloc(&p->d_vstate, sbytes) != hipSuccess) {
      (void)hipFree(p->d_vw);
      p->d_vw = nullptr; p->d_vstate = nullptr;
      throw PmcError(LL_ENOMEM, "hipMalloc failed");
    }
  }
  HIPCHK(hipMemcpy(p->d_vw, h_vf_weights, (size_t)want * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(hipMemset(p->d_vstate, 0, (size_t)p->max_rows * 64 * sizeof(float)));
  HIPCHK(hipDeviceSynchronize());
  size_t off = 0;
  for (int i = 0; i < n_arr; i++) { p->W.a[2 + i] = p->d_vw + off; off += (size_t)sizes[i]; }
  LL_CATCH
}

int ll_hl_policy_act_pg(ll_hl_policy* p, const float* d_obs, int obs_stride, const uint8_t* d_reset, float* d_actions, int32_t* d_code, float* d_heading,
                        float* d_neglogp, float* d_value, uint64_t seed, uint64_t step, int sample, int n_rows, void* hip_stream) {
  LL_TRY
  hl_check(p);
  LL_CHECK(d_obs && d_actions, "null argument");
  LL_CHECK(n_rows > 0 && n_rows <= p->max_rows, "n_rows must be 1 .. max_rows");
  LL_CHECK(obs_stride == (p->kind == LLH_EPMC ? LLH_EPMC_OBS_DIM : LLH_SEPMC_OBS_DIM), "obs_stride is not the policy's obs dim (916 EPMC, 965 SEPMC)");
  LL_CHECK(!d_heading || p->kind == LLH_SEPMC, "d_heading: the EPMC policy has no heading");
  LL_CHECK(!d_value || p->d_vw, "d_value: no value branch attached (ll_hl_policy_attach_value)");
  HIPCHK(hipSetDevice(p->device));
  hipStream_t st = (hipStream_t)hip_stream;
  std::pair<hipEvent_t, hipEvent_t>* ev = hl_timing_begin(p, st);
  const dim3 grid((n_rows + POL_M - 1) / POL_M, d_value ? 2 : 1), block(POL_THREADS);
  if (p->kind == LLH_EPMC)
    hipLaunchKernelGGL(hl_policy_pg_kernel<LLH_EPMC>, grid, block, 0, st, p->W, d_obs, obs_stride, d_reset, p->d_state, p->d_vstate, d_actions, d_code, d_heading,
                       d_neglogp, d_value, seed, step, sample, n_rows);
  else
    hipLaunchKernelGGL(hl_policy_pg_kernel<LLH_SEPMC>, grid, block, 0, st, p->W, d_obs, obs_stride, d_reset, p->d_state, p->d_vstate, d_actions, d_code, d_heading,
                       d_neglogp, d_value, seed, step, sample, n_rows);
  HIPCHK(hipGetLastError());
  if (ev) HIPCHK(hipEventRecord(ev->second, st));
  LL_CATCH
}

int ll_hl_policy_set_weights(ll_hl_policy* p, const float* h_weights, int n_floats, const float* h_vf_weights, int n_vf_floats, void* hip_stream) {
  LL_TRY
  hl_check(p);
  LL_CHECK(h_weights, "null argument");
  const bool ep = p->kind == LLH_EPMC;
  const int want = ep ? LLH_EPMC_N_FLOATS : LLH_SEPMC_N_FLOATS, vwant = ep ? LLH_EPMC_VF_N_FLOATS : LLH_SEPMC_VF_N_FLOATS;
  LL_CHECK(n_floats == want, "weights: not the float count ll_hl_policy_create takes for this kind");
  if (p->d_vw) {
    LL_CHECK(h_vf_weights, "h_vf_weights: the policy has a value branch attached, a new model replaces both");
    LL_CHECK(n_vf_floats == vwant, "value weights: not the float count ll_hl_policy_attach_value takes for this kind");
  } else {
    LL_CHECK(!h_vf_weights, "h_vf_weights: no value branch attached (ll_hl_policy_attach_value)");
  }
  HIPCHK(hipSetDevice(p->device));
  hipStream_t st = (hipStream_t)hip_stream;
  if (!p->h_stage) {
    if (hipHostMalloc((void**)&p->h_stage, ((size_t)want + vwant) * sizeof(float), hipHostMallocDefault) != hipSuccess) {
      p->h_stage = nullptr;
      throw PmcError(LL_ENOMEM, "hipHostMalloc of the weight staging buffer failed");
    }
    HIPCHK(hipEventCreateWithFlags(&p->up_ev, hipEventDisableTiming));
  }
  if (p->up_pending) HIPCHK(hipEventSynchronize(p->up_ev));      // the staging buffer is free once the previous upload has left it
  memcpy(p->h_stage, h_weights, (size_t)want * sizeof(float));
  HIPCHK(hipMemcpyAsync(p->d_w, p->h_stage, (size_t)want * sizeof(float), hipMemcpyHostToDevice, st));
  if (h_vf_weights) {
    memcpy(p->h_stage + want, h_vf_weights, (size_t)vwant * sizeof(float));
    HIPCHK(hipMemcpyAsync(p->d_vw, p->h_stage + want, (size_t)vwant * sizeof(float), hipMemcpyHostToDevice, st));
  }
  HIPCHK(hipEventRecord(p->up_ev, st));
  p->up_pending = true;
  LL_CATCH
}

// host <-> the value state [max_rows][64]
static int hl_value_state_copy(ll_hl_policy* p, void* h_state, bool to_host) {
  LL_TRY
  hl_check(p);
  LL_CHECK(h_state, "null argument");
  LL_CHECK(p->d_vstate, "no value branch attached (ll_hl_policy_attach_value)");
  HIPCHK(hipSetDevice(p->device));
  HIPCHK(hipDeviceSynchronize());
  const size_t bytes = (size_t)p->max_rows * 64 * sizeof(float);
  if (to_host)
    HIPCHK(hipMemcpy(h_state, p->d_vstate, bytes, hipMemcpyDeviceToHost));
  else
    HIPCHK(hipMemcpy(p->d_vstate, h_state, bytes, hipMemcpyHostToDevice));
  HIPCHK(hipDeviceSynchronize());
  LL_CATCH
}

int ll_hl_policy_get_value_state(ll_hl_policy* p, float* h_state) { return hl_value_state_copy(p, h_state, true); }

int ll_hl_policy_set_value_state(ll_hl_policy* p, const float* h_state) { return hl_value_state_copy(p, const_cast<float*>(h_state), false); }

int ll_hl_policy_get_state(ll_hl_policy* p, float* h_state) {
  LL_TRY
  hl_check(p);
  LL_CHECK(h_state, "null argument");
  HIPCHK(hipSetDevice(p->device));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(h_state, p->d_state, (size_t)p->max_rows * p->state_dim * sizeof(float), hipMemcpyDeviceToHost));
  LL_CATCH
}

int ll_hl_policy_set_state(ll_hl_policy* p, const float* h_state) {
  LL_TRY
  hl_check(p);
  LL_CHECK(h_state, "null argument");
  HIPCHK(hipSetDevice(p->device));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(p->d_state, h_state, (size_t)p->max_rows * p->state_dim * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(hipDeviceSynchronize());
  LL_CATCH
}

int ll_hl_policy_enable_timing(ll_hl_policy* p, int on) {
  LL_TRY
  hl_check(p);
  p->timing = on != 0;
  LL_CATCH
}

int ll_hl_policy_time_ms(ll_hl_policy* p, double* avg_ms, int* n_launches) {
  LL_TRY
  hl_check(p);
  LL_CHECK(avg_ms && n_launches, "null argument");
  HIPCHK(hipSetDevice(p->device));
  HIPCHK(hipDeviceSynchronize());
  double tot = 0;
  for (size_t i = 0; i < p->ev_used; i++) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, p->evs[i].first, p->evs[i].second));
    tot += ms;
  }
  *n_launches = (int)p->ev_used;
  *avg_ms = p->ev_used ? tot / p->ev_used : 0.0;
  p->ev_used = 0;
  LL_CATCH
}

}  // extern "C"

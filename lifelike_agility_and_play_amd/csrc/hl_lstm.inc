// hl_lstm.inc -- the layer-normalised LSTM core of the EPMC / SEPMC networks with its linear head (include/hl/llenv_hl_lstm.h): forward over an unroll
// leaving a tape, and backward through time.  Included after hl_loss.inc.  Its device functions are its own: nothing of pmc_policy.inc / hl_policy.inc
// is called (DESIGN 6.3: a new caller changes other kernels' machine code); the formulas and the rsqrtf / 1 / (1 + expf(-x)) / tanhf forms are hl_lstm's.
//
//   hl_lstm_fwd_kernel      HLS_FROWS = 16 rows per workgroup of 512 lanes, the time loop inside, c in registers and h in LDS.  Per step: u = E_t wx and v = h wh
//                           on the float64 matrix cores (a wave owns 16 gate columns and keeps its wx / wh operands in registers; E_t and M_t are fetched a step
//                           ahead), then thread (row, unit) holds the unit's four gates: the three LNs through 32-lane sums, the gates, the tape; then the head.
//                           It needs no workspace: the interface allows a call without a tape.
//   hl_lstm_bwd_seq_kernel  HLS_ROWS = 8 rows, time reversed, thread (row, unit): the step recomputed from the tape, dY wo^T added to the carried dh, the
//                           gradients at u and at v of every frame to the workspace, the vector gradients summed in float64 registers, dS0.
//   hl_lstm_bwd_de_kernel   HLS_DE_FRAMES frames per workgroup: dE = dU wx^T.
//   hl_lstm_bwd_dw_kernel   workgroup (g, y) sums chunks g, g + G, .. of HLS_CHUNK frames: y = 0, 1 the halves of d wx = E^T dU on the float64 matrix cores,
//                           y = 2 d wh = H_prev^T dV, d wo = H^T dY and d bo.
//   hl_lstm_fold_kernel     one thread per weight-gradient entry adds its partials in index order in float64, HLS_FOLD_PASS per pass, rounds once.
// Every dot product -- E wx, h wh, the head, dY wo^T, dV wh^T, dU wx^T and the sums over frames -- multiplies float32 values exactly and adds them in float64,
// rounding once: the bars of the tests are a small multiple of what NumPy's float32 pass loses, whose BLAS sums are blocked, and a float32 running sum of 256
// terms alone loses about as much as that whole pass.  What is left is the float32 arithmetic of the LNs and the gates, which is hl_lstm's.
// No atomics, no ticket, every loop bounded by L or a launch-time count; a row's Y, S_end, dE and dS0 are sums in a fixed order over that row alone.
#include "../../include/hl/llenv_hl_lstm.h"

#define HLS_THREADS 256
#define HLS_ROWS 8                       // rows of a backward sequential workgroup: one per 32 lanes
#define HLS_FTHREADS 512                 // the forward: sixteen rows, one 16 x 16 float64 matrix-core tile of u and of v per wave
#define HLS_FROWS 16
#define HLS_PAD 16                       // float64 padding of an LDS row read by matrix-core lanes (row k of four per 16 lanes)
#define HLS_DE_FRAMES 16                 // frames of a dE workgroup
#define HLS_CHUNK 64                     // frames a weight-gradient workgroup sums at a time
#define HLS_STAGE 8                      // ... staged in LDS this many at a time
#define HLS_MAX_GROUPS 80                // rows of partials; three workgroups each (two halves of wx, and the small arrays): 240 fit a 256-CU device in one round
#define HLS_FOLD_PASS 8                  // partial rows a fold pass adds
#define HLS_NV 448                       // vector partials of a row group: sum dz [128] | sum dz x^_x [128] | sum dz x^_h [128] | sum dn [32] | sum dn c^ [32]
#define HLS_WX (LLT_N_IN * LLT_N_GATES)          // 32768
#define HLS_WH (LLT_N_UNITS * LLT_N_GATES)       // 4096
#define HLS_VEC_OFF (HLS_WX + HLS_WH)            // 36864: b, beta_x, gamma_x, beta_h, gamma_h [128] each, beta_c, gamma_c [32] each
#define HLS_WO_OFF (HLS_VEC_OFF + 5 * 128 + 64)  // 37568
// tape, per frame
#define HLS_T_XX 0                       // x^ of LN_x [128]
#define HLS_T_XH 128                     // x^ of LN_h [128]
#define HLS_T_CP 256                     // c entering the step (after a reset) [32]
#define HLS_T_HP 288                     // h entering the step [32]
#define HLS_T_HN 320                     // h the step left [32]
#define HLS_T_RX 352                     // r of LN_x, r of LN_h, two pads
static_assert(HLS_T_RX + 4 == LLT_TAPE_FLOATS && LLT_TAPE_FLOATS <= 512 && LLT_TAPE_FLOATS % 4 == 0, "the tape of a frame");
static_assert(HLS_WO_OFF == 37568 && HLS_THREADS == HLS_ROWS * LLT_N_UNITS && HLS_THREADS == LLT_N_IN && HLS_FTHREADS == HLS_FROWS * LLT_N_UNITS, "one thread per (row, unit), and per input");

struct HlsW {
  const float *wx, *wh, *b, *bx, *gx, *bh, *gh, *bc, *gc, *wo, *bo;
  int D;
};

struct HlsFwd {
  HlsW w;
  const float *e, *s0, *m;
  long s0_rs, m_rs, m_ss, y_stride;
  int n, L;
  float *y, *s_end, *tape;
};

struct HlsBwd {
  HlsW w;
  const float *e, *m, *tape, *dy, *ds_end;
  long m_rs, m_ss, dy_stride, n_frames, pstride;
  int n, L, n_groups, n_rowgroups, total;
  float *de, *ds0, *wgrad;
  double *partv, *part;                  // d_work: [n_rowgroups][HLS_NV] float64 | dU [n_frames][128] | dV [n_frames][128] | part [n_groups][pstride] float64
  float *du, *dv;
};

typedef double hls_d4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float hls_sum32(float v) {      // over the 32 lanes of a row
#pragma unroll
  for (int o = 16; o >= 1; o >>= 1) v += __shfl_xor(v, o, 32);
  return v;
}
// M != 0 by its bits: any non-zero value counts, a NaN and a subnormal (which a float compare on this device reads as zero) included
__device__ __forceinline__ bool hls_is_reset(float m) { return (__float_as_uint(m) & 0x7FFFFFFFu) != 0u; }
__device__ __forceinline__ float hls_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// the per-lane slices of the vector weights: gate g of unit j is column 32 g + j
struct HlsLaneW {
  float bx[4], gx[4], bh[4], gh[4], b[4], bc, gc;
  __device__ __forceinline__ void load(const HlsW& w, int j) {
#pragma unroll
    for (int g = 0; g < 4; g++) {
      const int c = 32 * g + j;
      bx[g] = w.bx[c]; gx[g] = w.gx[c]; bh[g] = w.bh[c]; gh[g] = w.gh[c]; b[g] = w.b[c];
    }
    bc = w.bc[j]; gc = w.gc[j];
  }
};

// what a step computes from (x^_x, x^_h, c): forward and backward run this one function
struct HlsGates {
  float si, sf, so, tg, c2, ch, rc, tn, h2;
};
__device__ __forceinline__ HlsGates hls_gates(const HlsLaneW& W, const float (&xx)[4], const float (&xh)[4], float c) {
  float z[4];
#pragma unroll
  for (int g = 0; g < 4; g++) z[g] = (xx[g] * W.gx[g] + W.bx[g]) + (xh[g] * W.gh[g] + W.bh[g]) + W.b[g];
  HlsGates s;
  s.si = hls_sigmoid(z[0]); s.sf = hls_sigmoid(z[1] + 1.0f); s.so = hls_sigmoid(z[2]); s.tg = tanhf(z[3]);     // i, f, o, g; forget bias 1.0
  s.c2 = s.sf * c + s.si * s.tg;
  const float mc = hls_sum32(s.c2) * (1.0f / 32.0f), dc = s.c2 - mc;
  s.rc = rsqrtf(hls_sum32(dc * dc) * (1.0f / 32.0f) + 1e-12f);
  s.ch = dc * s.rc;
  s.tn = tanhf(s.ch * W.gc + W.bc);
  s.h2 = s.so * s.tn;
  return s;
}
// x [4] of this lane's row (128 values over 32 lanes) -> x^ and r
__device__ __forceinline__ float hls_ln128(const float (&x)[4], float (&xh)[4]) {
  const float m = hls_sum32(x[0] + x[1] + x[2] + x[3]) * (1.0f / 128.0f);
  float v = 0.0f;
#pragma unroll
  for (int g = 0; g < 4; g++) v += (x[g] - m) * (x[g] - m);
  const float r = rsqrtf(hls_sum32(v) * (1.0f / 128.0f) + 1e-12f);
#pragma unroll
  for (int g = 0; g < 4; g++) xh[g] = (x[g] - m) * r;
  return r;
}
// four float32 values to LDS as float64
__device__ __forceinline__ void hls_stage4(double* dst, float4 x) {
  reinterpret_cast<double2*>(dst)[0] = make_double2((double)x.x, (double)x.y);
  reinterpret_cast<double2*>(dst)[1] = make_double2((double)x.z, (double)x.w);
}
// dx = r (dx^ - mean(dx^) - x^ mean(dx^ x^)), dx^ = dy gamma
__device__ __forceinline__ void hls_ln128_bwd(const float (&dy)[4], const float (&gamma)[4], const float (&xh)[4], float r, float (&dx)[4]) {
  float d[4], s1 = 0.0f, s2 = 0.0f;
#pragma unroll
  for (int g = 0; g < 4; g++) { d[g] = dy[g] * gamma[g]; s1 += d[g]; s2 += d[g] * xh[g]; }
  const float m1 = hls_sum32(s1) * (1.0f / 128.0f), m2 = hls_sum32(s2) * (1.0f / 128.0f);
#pragma unroll
  for (int g = 0; g < 4; g++) dx[g] = r * (d[g] - m1 - xh[g] * m2);
}

__global__ __launch_bounds__(HLS_FTHREADS) void hl_lstm_fwd_kernel(HlsFwd a) {
  __shared__ __attribute__((aligned(16))) double se[HLS_FROWS][LLT_N_IN + HLS_PAD];        // E_t and h as float64: converted once where they are staged
  __shared__ __attribute__((aligned(16))) double sh[HLS_FROWS][LLT_N_UNITS + 4];
  __shared__ float su[HLS_FROWS][LLT_N_GATES], sv[HLS_FROWS][LLT_N_GATES];
  const int tid = threadIdx.x, m = tid >> 5, j = tid & 31, row0 = blockIdx.x * HLS_FROWS, row = row0 + m;
  const bool live = row < a.n;
  const long r = live ? row : a.n - 1;                 // a lane without a row computes the last row again and stores nothing
  const int wave = tid >> 6, li = tid & 15, lk = (tid & 63) >> 4, colw = 16 * wave + li, D = a.w.D;      // the wave's 16 columns of u and v
  HlsLaneW W;
  W.load(a.w, j);
  const int hd = tid & 255, hr0 = (tid >> 8) * 8;        // the head, D >= 32: thread = (output d, eight of the rows)
  // the wave's B operands stay in registers for the whole unroll: wx[4 s + lk][colw], wh[4 s + lk][colw]
  float wxr[LLT_N_IN / 4], whr[LLT_N_UNITS / 4];
#pragma unroll
  for (int s = 0; s < LLT_N_IN / 4; s++) wxr[s] = a.w.wx[(size_t)(4 * s + lk) * LLT_N_GATES + colw];
#pragma unroll
  for (int s = 0; s < LLT_N_UNITS / 4; s++) whr[s] = a.w.wh[(4 * s + lk) * LLT_N_GATES + colw];
  // E_t and M_t are fetched one step ahead: two float4 of the tile per thread
  static_assert(HLS_FROWS * (LLT_N_IN / 4) == 2 * HLS_FTHREADS, "two float4 of E per thread and step");
  const float* ep[2];
#pragma unroll
  for (int i = 0; i < 2; i++) {
    const int q = tid + i * HLS_FTHREADS, rr = q >> 6;
    const long er = row0 + rr < a.n ? row0 + rr : a.n - 1;
    ep[i] = a.e + er * a.L * LLT_N_IN + 4 * (q & 63);
  }
  float4 e_next[2] = {*reinterpret_cast<const float4*>(ep[0]), *reinterpret_cast<const float4*>(ep[1])};
  float m_next = 0.0f;
  float c = a.s0[r * a.s0_rs + j], h = a.s0[r * a.s0_rs + 32 + j];
  for (int t = 0; t < a.L; t++) {
    if (t > 0 && hls_is_reset(m_next)) { c = 0.0f; h = 0.0f; }
    sh[m][j] = (double)h;
#pragma unroll
    for (int i = 0; i < 2; i++) {
      const int q = tid + i * HLS_FTHREADS;
      hls_stage4(&se[q >> 6][4 * (q & 63)], e_next[i]);
    }
    if (t + 1 < a.L) {
#pragma unroll
      for (int i = 0; i < 2; i++) e_next[i] = *reinterpret_cast<const float4*>(ep[i] + (size_t)(t + 1) * LLT_N_IN);
      m_next = a.m[r * a.m_rs + (long)(t + 1) * a.m_ss];
    }
    float* tp = a.tape + (r * a.L + t) * LLT_TAPE_FLOATS;
    const bool rec = a.tape != nullptr && live;
    if (rec) { tp[HLS_T_CP + j] = c; tp[HLS_T_HP + j] = h; }
    __syncthreads();
    // u = E_t wx and v = h wh on the matrix cores in float64: A[row = li][k = lk], B[k = lk][column = li], four k per instruction
    hls_d4 cu = {0.0, 0.0, 0.0, 0.0}, cv = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < LLT_N_IN / 4; s++) {
      float wf = wxr[s];
      asm volatile("" : "+v"(wf));          // converted here, every step: 64 float64 copies kept across the loop would not fit the registers
      cu = __builtin_amdgcn_mfma_f64_16x16x4f64(se[li][4 * s + lk], (double)wf, cu, 0, 0, 0);
    }
#pragma unroll
    for (int s = 0; s < LLT_N_UNITS / 4; s++) cv = __builtin_amdgcn_mfma_f64_16x16x4f64(sh[li][4 * s + lk], (double)whr[s], cv, 0, 0, 0);
#pragma unroll
    for (int q = 0; q < 4; q++) { su[lk + 4 * q][colw] = (float)cu[q]; sv[lk + 4 * q][colw] = (float)cv[q]; }      // D: row = lk + 4 q, column = li
    __syncthreads();
    float u[4], v[4], xx[4], xh[4];
#pragma unroll
    for (int g = 0; g < 4; g++) { u[g] = su[m][32 * g + j]; v[g] = sv[m][32 * g + j]; }
    const float rx = hls_ln128(u, xx), rh = hls_ln128(v, xh);
    const HlsGates s = hls_gates(W, xx, xh, c);
    c = s.c2; h = s.h2;
    sh[m][j] = (double)h;
    if (rec) {
#pragma unroll
      for (int g = 0; g < 4; g++) { tp[HLS_T_XX + 32 * g + j] = xx[g]; tp[HLS_T_XH + 32 * g + j] = xh[g]; }
      tp[HLS_T_HN + j] = h;
      if (j == 0) { tp[HLS_T_RX] = rx; tp[HLS_T_RX + 1] = rh; tp[HLS_T_RX + 2] = 0.0f; tp[HLS_T_RX + 3] = 0.0f; }
    }
    __syncthreads();
    if (D >= 32) {                                      // the head: y = h' wo + bo
      if (hd < D) {
        const double bo = (double)a.w.bo[hd];
        double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 8
        for (int k = 0; k < LLT_N_UNITS; k++) {
          const double wk = (double)a.w.wo[k * D + hd];
#pragma unroll
          for (int i = 0; i < 8; i++) acc[i] += sh[hr0 + i][k] * wk;
        }
#pragma unroll
        for (int i = 0; i < 8; i++)
          if (row0 + hr0 + i < a.n) a.y[((long)(row0 + hr0 + i) * a.L + t) * a.y_stride + hd] = (float)(acc[i] + bo);
      }
    } else {
      for (int i = tid; i < HLS_FROWS * D; i += HLS_FTHREADS) {
        const int mm = i / D, d = i - mm * D;
        if (row0 + mm < a.n) {
          double acc = 0.0;
          for (int k = 0; k < LLT_N_UNITS; k++) acc += sh[mm][k] * (double)a.w.wo[k * D + d];
          a.y[((long)(row0 + mm) * a.L + t) * a.y_stride + d] = (float)(acc + (double)a.w.bo[d]);
        }
      }
    }
    __syncthreads();
  }
  if (a.s_end && live) { a.s_end[r * LLT_STATE_FLOATS + j] = c; a.s_end[r * LLT_STATE_FLOATS + 32 + j] = h; }
}

__global__ __launch_bounds__(HLS_THREADS) void hl_lstm_bwd_seq_kernel(HlsBwd a) {
  __shared__ __attribute__((aligned(16))) float swo[LLT_MAX_OUT * LLT_N_UNITS];       // wo^T [d][32]; at the end HLS_ROWS x HLS_NV float64
  __shared__ float swh[LLT_N_UNITS][LLT_N_GATES + 1];
  __shared__ double sdv[HLS_ROWS][LLT_N_GATES];
  static_assert(sizeof(double) * HLS_ROWS * HLS_NV <= sizeof(float) * LLT_MAX_OUT * LLT_N_UNITS, "the vector partials fit the head's LDS");
  const int tid = threadIdx.x, m = tid >> 5, j = tid & 31, row = blockIdx.x * HLS_ROWS + m, D = a.w.D;
  const bool live = row < a.n;
  const long r = live ? row : a.n - 1;
  for (int i = tid; i < LLT_N_UNITS * D; i += HLS_THREADS) { const int k = i / D, d = i - k * D; swo[d * LLT_N_UNITS + k] = a.w.wo[i]; }
  for (int i = tid; i < HLS_WH; i += HLS_THREADS) swh[i >> 7][i & 127] = a.w.wh[i];
  HlsLaneW W;
  W.load(a.w, j);
  float dc = a.ds_end ? a.ds_end[r * LLT_STATE_FLOATS + j] : 0.0f, dh = a.ds_end ? a.ds_end[r * LLT_STATE_FLOATS + 32 + j] : 0.0f;
  double acc[14];
#pragma unroll
  for (int i = 0; i < 14; i++) acc[i] = 0.0;
  __syncthreads();
  for (int t = a.L - 1; t >= 0; t--) {
    const long f = r * a.L + t;
    const float* tp = a.tape + f * LLT_TAPE_FLOATS;
    float xx[4], xh[4];
#pragma unroll
    for (int g = 0; g < 4; g++) { xx[g] = tp[HLS_T_XX + 32 * g + j]; xh[g] = tp[HLS_T_XH + 32 * g + j]; }
    const float cp = tp[HLS_T_CP + j], rx = tp[HLS_T_RX], rh = tp[HLS_T_RX + 1];
    const HlsGates s = hls_gates(W, xx, xh, cp);
    const float* dyp = a.dy + f * a.dy_stride;
    double hd = 0.0;
#pragma unroll 4
    for (int d = 0; d < D; d++) hd += (double)dyp[d] * (double)swo[d * LLT_N_UNITS + j];
    dh += (float)hd;
    const float dn = dh * s.so * (1.0f - s.tn * s.tn);
    float dz[4];
    dz[2] = dh * s.tn * s.so * (1.0f - s.so);
    const float dch = dn * W.gc;
    const float m1 = hls_sum32(dch) * (1.0f / 32.0f), m2 = hls_sum32(dch * s.ch) * (1.0f / 32.0f);
    dc += s.rc * (dch - m1 - s.ch * m2);
    dz[0] = dc * s.tg * s.si * (1.0f - s.si);
    dz[1] = dc * cp * s.sf * (1.0f - s.sf);
    dz[3] = dc * s.si * (1.0f - s.tg * s.tg);
    if (live) {
#pragma unroll
      for (int g = 0; g < 4; g++) { acc[g] += (double)dz[g]; acc[4 + g] += (double)dz[g] * (double)xx[g]; acc[8 + g] += (double)dz[g] * (double)xh[g]; }
      acc[12] += (double)dn;
      acc[13] += (double)dn * (double)s.ch;
    }
    float du[4], dv[4];
    hls_ln128_bwd(dz, W.gx, xx, rx, du);
    hls_ln128_bwd(dz, W.gh, xh, rh, dv);
    if (live) {
#pragma unroll
      for (int g = 0; g < 4; g++) { a.du[f * LLT_N_GATES + 32 * g + j] = du[g]; a.dv[f * LLT_N_GATES + 32 * g + j] = dv[g]; }
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < 4; g++) sdv[m][32 * g + j] = (double)dv[g];
    __syncthreads();
    double dhp = 0.0;
#pragma unroll 8
    for (int cc = 0; cc < LLT_N_GATES; cc++) dhp += sdv[m][cc] * (double)swh[j][cc];
    const bool cut = t > 0 && hls_is_reset(a.m[r * a.m_rs + (long)t * a.m_ss]);       // the step started from zero: nothing flows further back
    dc = cut ? 0.0f : dc * s.sf;
    dh = cut ? 0.0f : (float)dhp;
  }
  if (a.ds0 && live) { a.ds0[r * LLT_STATE_FLOATS + j] = dc; a.ds0[r * LLT_STATE_FLOATS + 32 + j] = dh; }
  __syncthreads();
  double* sd = reinterpret_cast<double*>(swo);
#pragma unroll
  for (int g = 0; g < 4; g++) {
    sd[m * HLS_NV + 32 * g + j] = acc[g];
    sd[m * HLS_NV + 128 + 32 * g + j] = acc[4 + g];
    sd[m * HLS_NV + 256 + 32 * g + j] = acc[8 + g];
  }
  sd[m * HLS_NV + 384 + j] = acc[12];
  sd[m * HLS_NV + 416 + j] = acc[13];
  __syncthreads();
  for (int i = tid; i < HLS_NV; i += HLS_THREADS) {
    double t = sd[i];
    for (int mm = 1; mm < HLS_ROWS; mm++) t += sd[mm * HLS_NV + i];
    a.partv[(size_t)blockIdx.x * HLS_NV + i] = t;
  }
}

// dE[f][k] = sum over columns, in column order, of dU[f][col] wx[k][col]; thread = k, wx staged 32 columns at a time
__global__ __launch_bounds__(HLS_THREADS) void hl_lstm_bwd_de_kernel(HlsBwd a) {
  __shared__ __attribute__((aligned(16))) double sdu[HLS_DE_FRAMES][LLT_N_GATES];
  __shared__ float swx[LLT_N_IN][33];
  const int tid = threadIdx.x;
  const long f0 = (long)blockIdx.x * HLS_DE_FRAMES;
  for (int q = tid; q < HLS_DE_FRAMES * (LLT_N_GATES / 4); q += HLS_THREADS) {
    const int fr = q >> 5;
    const float4 x = f0 + fr < a.n_frames ? reinterpret_cast<const float4*>(a.du + (f0 + fr) * LLT_N_GATES)[q & 31] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    double2* dst = reinterpret_cast<double2*>(&sdu[fr][4 * (q & 31)]);
    dst[0] = make_double2((double)x.x, (double)x.y);
    dst[1] = make_double2((double)x.z, (double)x.w);
  }
  double acc[HLS_DE_FRAMES];
#pragma unroll
  for (int q = 0; q < HLS_DE_FRAMES; q++) acc[q] = 0.0;
  for (int c0 = 0; c0 < LLT_N_GATES; c0 += 32) {
    __syncthreads();
    for (int i = tid; i < LLT_N_IN * 32; i += HLS_THREADS) swx[i >> 5][i & 31] = a.w.wx[(size_t)(i >> 5) * LLT_N_GATES + c0 + (i & 31)];
    __syncthreads();
    for (int cc = 0; cc < 32; cc++) {
      const double w = (double)swx[tid][cc];
#pragma unroll
      for (int q = 0; q < HLS_DE_FRAMES; q++) acc[q] += sdu[q][c0 + cc] * w;
    }
  }
#pragma unroll
  for (int q = 0; q < HLS_DE_FRAMES; q++)
    if (f0 + q < a.n_frames) a.de[(f0 + q) * LLT_N_IN + tid] = (float)acc[q];
}

// Partials of the matrix gradients: workgroup (g, y) takes chunks g, g + gridDim.x, .. of HLS_CHUNK frames, HLS_STAGE frames at a time through LDS.
// y = 0, 1: d wx = E^T dU for columns 64 y .. 64 y + 63 on the matrix cores in float64 -- wave w holds inputs 64 w .. 64 w + 63, sixteen 16 x 16 tiles;
// y = 2: d wh, d wo and d bo.
__global__ __launch_bounds__(HLS_THREADS) void hl_lstm_bwd_dw_kernel(HlsBwd a) {
  __shared__ __attribute__((aligned(16))) double se[HLS_STAGE][LLT_N_IN + HLS_PAD];           // E; then dY.  All float64: converted once where they are staged
  __shared__ __attribute__((aligned(16))) double sdu[HLS_STAGE][LLT_N_GATES + HLS_PAD];       // dU; then dV
  __shared__ __attribute__((aligned(16))) double shp[HLS_STAGE][LLT_N_UNITS], shn[HLS_STAGE][LLT_N_UNITS];
  const int tid = threadIdx.x, D = a.w.D;
  const long n_chunks = (a.n_frames + HLS_CHUNK - 1) / HLS_CHUNK;
  double* out = a.part + (size_t)blockIdx.x * a.pstride;
  const float4 zero4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (blockIdx.y < 2) {
    const int wave = tid >> 6, li = tid & 15, lk = (tid & 63) >> 4, kb = 64 * wave, cb = 64 * blockIdx.y;
    hls_d4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int c = 0; c < 4; c++) acc[i][c] = hls_d4{0.0, 0.0, 0.0, 0.0};
    static_assert(HLS_STAGE * (LLT_N_IN / 4) == 2 * HLS_THREADS && HLS_STAGE * (LLT_N_GATES / 4) == HLS_THREADS, "two float4 of E and one of dU per thread and stage");
    float4 pe[2], pu;
    bool have = false;
    auto load = [&](long f0) {      // the thread's share of the stage that starts at frame f0, into registers
#pragma unroll
      for (int i = 0; i < 2; i++) {
        const long f = f0 + (tid >> 6) + 4 * i;
        pe[i] = f < a.n_frames ? reinterpret_cast<const float4*>(a.e + f * LLT_N_IN)[tid & 63] : zero4;
      }
      const long f = f0 + (tid >> 5);
      pu = f < a.n_frames ? reinterpret_cast<const float4*>(a.du + f * LLT_N_GATES)[tid & 31] : zero4;
    };
    for (long ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
      for (int s = 0; s < HLS_CHUNK; s += HLS_STAGE) {
        const long f0 = ch * HLS_CHUNK + s;
        if (f0 >= a.n_frames) break;
        if (!have) load(f0);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 2; i++) hls_stage4(&se[(tid >> 6) + 4 * i][4 * (tid & 63)], pe[i]);
        hls_stage4(&sdu[tid >> 5][4 * (tid & 31)], pu);
        __syncthreads();
        {  // the stage after this one: the next of the chunk, or the first of the workgroup's next chunk
          const long fn = s + HLS_STAGE < HLS_CHUNK ? f0 + HLS_STAGE : (ch + gridDim.x) * HLS_CHUNK;
          have = fn < a.n_frames && (s + HLS_STAGE < HLS_CHUNK || ch + gridDim.x < n_chunks);
          if (have) load(fn);
        }
#pragma unroll
        for (int fs = 0; fs < HLS_STAGE; fs += 4) {       // A[input = li][frame = lk], B[frame = lk][column = li]
          double av[4], bv[4];
#pragma unroll
          for (int i = 0; i < 4; i++) { av[i] = se[fs + lk][kb + 16 * i + li]; bv[i] = sdu[fs + lk][cb + 16 * i + li]; }
#pragma unroll
          for (int i = 0; i < 4; i++)
#pragma unroll
            for (int c = 0; c < 4; c++) acc[i][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[i], bv[c], acc[i][c], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int c = 0; c < 4; c++)
#pragma unroll
        for (int q = 0; q < 4; q++) out[(kb + 16 * i + lk + 4 * q) * LLT_N_GATES + cb + 16 * c + li] = acc[i][c][q];      // D: row = lk + 4 q, column = li
  } else {  // d wh: thread = 16 units x 1 column; d wo, d bo: thread = output d
    const int col = tid & 127, k0 = (tid >> 7) * 16;
    double awh[16], awo[LLT_N_UNITS], abo = 0.0;
#pragma unroll
    for (int i = 0; i < 16; i++) awh[i] = 0.0;
#pragma unroll
    for (int k = 0; k < LLT_N_UNITS; k++) awo[k] = 0.0;
    for (long ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
      for (int s = 0; s < HLS_CHUNK; s += HLS_STAGE) {
        const long f0 = ch * HLS_CHUNK + s;
        if (f0 >= a.n_frames) break;
        __syncthreads();
        {
          const int fr = tid >> 5, k = tid & 31;
          const bool in = f0 + fr < a.n_frames;
          const float* tp = a.tape + (f0 + fr) * LLT_TAPE_FLOATS;
          shp[fr][k] = in ? (double)tp[HLS_T_HP + k] : 0.0;
          shn[fr][k] = in ? (double)tp[HLS_T_HN + k] : 0.0;
          hls_stage4(&sdu[fr][4 * k], in ? reinterpret_cast<const float4*>(a.dv + (f0 + fr) * LLT_N_GATES)[k] : zero4);
        }
        if (tid < D) {
          for (int fr = 0; fr < HLS_STAGE; fr++) se[fr][tid] = f0 + fr < a.n_frames ? (double)a.dy[(f0 + fr) * a.dy_stride + tid] : 0.0;
        }
        __syncthreads();
#pragma unroll 2
        for (int q = 0; q < HLS_STAGE; q++) {
          const double dvq = sdu[q][col];
#pragma unroll
          for (int i = 0; i < 16; i++) awh[i] += shp[q][k0 + i] * dvq;
          if (tid < D) {
            const double dyq = se[q][tid];
            abo += dyq;
#pragma unroll
            for (int k = 0; k < LLT_N_UNITS; k++) awo[k] += shn[q][k] * dyq;
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 16; i++) out[HLS_WX + (k0 + i) * LLT_N_GATES + col] = awh[i];
    if (tid < D) {
#pragma unroll
      for (int k = 0; k < LLT_N_UNITS; k++) out[HLS_VEC_OFF + k * D + tid] = awo[k];
      out[HLS_VEC_OFF + LLT_N_UNITS * D + tid] = abo;
    }
  }
}

// entry idx of the packed gradient: its partials added in index order in float64, HLS_FOLD_PASS rows per pass, rounded once
__global__ __launch_bounds__(HLS_THREADS) void hl_lstm_fold_kernel(HlsBwd a) {
#pragma clang fp contract(off)
  const int idx = blockIdx.x * HLS_THREADS + threadIdx.x;
  if (idx >= a.total) return;
  double s = 0.0;
  if (idx >= HLS_VEC_OFF && idx < HLS_WO_OFF) {          // b, beta_x and beta_h are the same sum
    const int o = idx - HLS_VEC_OFF;
    int src;
    if (o < 640) { const int which = o >> 7, c = o & 127; src = (which == 2 ? 128 : which == 4 ? 256 : 0) + c; }
    else src = 384 + (o - 640);
    for (int p0 = 0; p0 < a.n_rowgroups; p0 += HLS_FOLD_PASS)
      for (int i = 0; i < HLS_FOLD_PASS && p0 + i < a.n_rowgroups; i++) s += a.partv[(size_t)(p0 + i) * HLS_NV + src];
  } else {
    const int src = idx < HLS_VEC_OFF ? idx : idx - (HLS_WO_OFF - HLS_VEC_OFF);
    for (int p0 = 0; p0 < a.n_groups; p0 += HLS_FOLD_PASS)
      for (int i = 0; i < HLS_FOLD_PASS && p0 + i < a.n_groups; i++) s += a.part[(size_t)(p0 + i) * a.pstride + src];
  }
  a.wgrad[idx] = (float)s;
}

struct HlsSizes {
  uint64_t frames, rowgroups, groups, pstride, total, tape_bytes, partv_bytes, frame_bytes, work_bytes;
};
static HlsSizes hls_sizes(int n_rows, int L, int n_out) {
  HlsSizes z;
  z.frames = (uint64_t)n_rows * (uint64_t)L;
  z.rowgroups = ((uint64_t)n_rows + HLS_ROWS - 1) / HLS_ROWS;
  const uint64_t chunks = (z.frames + HLS_CHUNK - 1) / HLS_CHUNK;
  z.groups = chunks < HLS_MAX_GROUPS ? chunks : HLS_MAX_GROUPS;
  z.pstride = (uint64_t)HLS_VEC_OFF + 33u * (uint64_t)n_out;
  z.total = (uint64_t)HLS_WO_OFF + 33u * (uint64_t)n_out;
  z.tape_bytes = z.frames * LLT_TAPE_FLOATS * sizeof(float);
  z.partv_bytes = z.rowgroups * HLS_NV * sizeof(double);
  z.frame_bytes = z.frames * LLT_N_GATES * sizeof(float);
  z.work_bytes = z.partv_bytes + 2 * z.frame_bytes + z.groups * z.pstride * sizeof(double);
  return z;
}

static void hls_check_shape(int n_rows, int L, int n_out) {
  LL_CHECK(n_rows > 0 && L > 0, "n_rows and L must be positive");
  LL_CHECK(n_out >= 1 && n_out <= LLT_MAX_OUT, "n_out must lie in 1 .. 256");
  LL_CHECK((long long)n_rows * (long long)L < 0x80000000ll, "n_rows x L must stay below 2^31");
}
static bool hls_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static HlsW hls_weights(const ll_hl_lstm_weights_t* w) {
  LL_CHECK(w, "null argument");
  LL_CHECK(w->wx && w->wh && w->b && w->beta_x && w->gamma_x && w->beta_h && w->gamma_h && w->beta_c && w->gamma_c && w->wo && w->bo, "null weight array");
  LL_CHECK(w->reserved == 0, "reserved must be 0");
  LL_CHECK(w->n_out >= 1 && w->n_out <= LLT_MAX_OUT, "n_out must lie in 1 .. 256");
  const HlsW r = {w->wx, w->wh, w->b, w->beta_x, w->gamma_x, w->beta_h, w->gamma_h, w->beta_c, w->gamma_c, w->wo, w->bo, w->n_out};
  return r;
}
static void hls_need_device() {
  int nd = 0;
  if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) {
    (void)hipGetLastError();
    throw PmcError(LL_ENODEV, "no HIP device available: the LSTM core has no CPU path");
  }
}

extern "C" {

int ll_hl_lstm_weight_layout(int n_out, uint64_t* off, uint64_t* dim, uint64_t* total) {
  LL_TRY
  LL_CHECK(n_out >= 1 && n_out <= LLT_MAX_OUT, "n_out must lie in 1 .. 256");
  const uint64_t d[LLT_N_WEIGHTS] = {HLS_WX, HLS_WH, 128, 128, 128, 128, 128, 32, 32, 32u * (uint64_t)n_out, (uint64_t)n_out};
  uint64_t at = 0;
  for (int i = 0; i < LLT_N_WEIGHTS; i++) {
    if (off) off[i] = at;
    if (dim) dim[i] = d[i];
    at += d[i];
  }
  if (total) *total = at;
  LL_CATCH
}

int ll_hl_lstm_workspace_bytes(int n_rows, int L, int n_out, uint64_t* tape_bytes, uint64_t* work_bytes) {
  LL_TRY
  hls_check_shape(n_rows, L, n_out);
  const HlsSizes z = hls_sizes(n_rows, L, n_out);
  if (tape_bytes) *tape_bytes = z.tape_bytes;
  if (work_bytes) *work_bytes = z.work_bytes;
  LL_CATCH
}

int ll_hl_lstm_forward(const ll_hl_lstm_weights_t* w, const float* d_e, const float* d_s0, int64_t s0_row_stride, const float* d_m, int64_t m_row_stride,
                       int64_t m_step_stride, int n_rows, int L, float* d_y, int64_t y_stride, float* d_s_end, float* d_tape, uint64_t tape_bytes,
                       void* hip_stream) {
  LL_TRY
  HlsFwd a;
  a.w = hls_weights(w);
  LL_CHECK(d_e && d_s0 && d_m && d_y, "null argument");
  hls_check_shape(n_rows, L, a.w.D);
  LL_CHECK(s0_row_stride >= LLT_STATE_FLOATS && m_row_stride >= 1 && m_step_stride >= 1 && y_stride >= a.w.D, "a stride is smaller than its field");
  const HlsSizes z = hls_sizes(n_rows, L, a.w.D);
  if (d_tape && tape_bytes < z.tape_bytes)
    throw PmcError(LL_EINVAL, "tape_bytes " + std::to_string(tape_bytes) + " is below ll_hl_lstm_workspace_bytes (" + std::to_string(z.tape_bytes) + ")");
  LL_CHECK(hls_aligned16(d_e) && hls_aligned16(d_tape), "d_e and d_tape must be 16-byte aligned");
  hls_need_device();
  a.e = d_e; a.s0 = d_s0; a.m = d_m;
  a.s0_rs = s0_row_stride; a.m_rs = m_row_stride; a.m_ss = m_step_stride; a.y_stride = y_stride;
  a.n = n_rows; a.L = L; a.y = d_y; a.s_end = d_s_end; a.tape = d_tape;
  hipLaunchKernelGGL(hl_lstm_fwd_kernel, dim3((unsigned)(((uint64_t)n_rows + HLS_FROWS - 1) / HLS_FROWS)), dim3(HLS_FTHREADS), 0, (hipStream_t)hip_stream, a);
  HIPCHK(hipGetLastError());
  LL_CATCH
}

int ll_hl_lstm_backward(const ll_hl_lstm_weights_t* w, const float* d_e, const float* d_m, int64_t m_row_stride, int64_t m_step_stride, int n_rows, int L,
                        const float* d_tape, uint64_t tape_bytes, const float* d_dy, int64_t dy_stride, const float* d_ds_end, float* d_de, float* d_ds0,
                        float* d_wgrad, void* d_work, uint64_t work_bytes, void* hip_stream) {
  LL_TRY
  HlsBwd a;
  a.w = hls_weights(w);
  LL_CHECK(d_e && d_m && d_tape && d_dy && d_de && d_wgrad && d_work, "null argument");
  hls_check_shape(n_rows, L, a.w.D);
  LL_CHECK(m_row_stride >= 1 && m_step_stride >= 1 && dy_stride >= a.w.D, "a stride is smaller than its field");
  const HlsSizes z = hls_sizes(n_rows, L, a.w.D);
  if (tape_bytes < z.tape_bytes)
    throw PmcError(LL_EINVAL, "tape_bytes " + std::to_string(tape_bytes) + " is below ll_hl_lstm_workspace_bytes (" + std::to_string(z.tape_bytes) + ")");
  if (work_bytes < z.work_bytes)
    throw PmcError(LL_EINVAL, "work_bytes " + std::to_string(work_bytes) + " is below ll_hl_lstm_workspace_bytes (" + std::to_string(z.work_bytes) + ")");
  LL_CHECK(hls_aligned16(d_e) && hls_aligned16(d_de) && hls_aligned16(d_tape) && hls_aligned16(d_work), "d_e, d_de, d_tape and d_work must be 16-byte aligned");
  hls_need_device();
  a.e = d_e; a.m = d_m; a.tape = d_tape; a.dy = d_dy; a.ds_end = d_ds_end;
  a.m_rs = m_row_stride; a.m_ss = m_step_stride; a.dy_stride = dy_stride; a.n_frames = (long)z.frames; a.pstride = (long)z.pstride;
  a.n = n_rows; a.L = L; a.n_groups = (int)z.groups; a.n_rowgroups = (int)z.rowgroups; a.total = (int)z.total;
  a.de = d_de; a.ds0 = d_ds0; a.wgrad = d_wgrad;
  char* p = static_cast<char*>(d_work);
  a.partv = reinterpret_cast<double*>(p);
  a.du = reinterpret_cast<float*>(p + z.partv_bytes);
  a.dv = reinterpret_cast<float*>(p + z.partv_bytes + z.frame_bytes);
  a.part = reinterpret_cast<double*>(p + z.partv_bytes + 2 * z.frame_bytes);
  const hipStream_t st = (hipStream_t)hip_stream;
  const dim3 block(HLS_THREADS);
  hipLaunchKernelGGL(hl_lstm_bwd_seq_kernel, dim3((unsigned)z.rowgroups), block, 0, st, a);
  hipLaunchKernelGGL(hl_lstm_bwd_de_kernel, dim3((unsigned)((z.frames + HLS_DE_FRAMES - 1) / HLS_DE_FRAMES)), block, 0, st, a);
  hipLaunchKernelGGL(hl_lstm_bwd_dw_kernel, dim3((unsigned)z.groups, 3), block, 0, st, a);
  hipLaunchKernelGGL(hl_lstm_fold_kernel, dim3((unsigned)((z.total + HLS_THREADS - 1) / HLS_THREADS)), block, 0, st, a);
  HIPCHK(hipGetLastError());
  LL_CATCH
}

}  // extern "C"

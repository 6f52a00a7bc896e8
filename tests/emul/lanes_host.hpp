// lanes_host.hpp -- TEST INFRASTRUCTURE: a 16-wide host stand-in for one DPP row of GPU lanes (one environment), so
// that the kernel body (lifelike_agility_and_play_amd/csrc/pmc_step.hpp) can be executed, one environment at a time,
// on a machine without a GPU.  It exists to debug the kernel's logic against the oracle here; it is compiled only by
// the tests and is never linked into, or reachable from, the product library.
#pragma once
#include <math.h>
#include <stdint.h>
#include <atomic>
#include <thread>
#include <vector>

#define EW 16
struct bN { bool v[EW]; };
struct fN {
  float v[EW];
  fN() {}
  explicit fN(float x) { for (int i = 0; i < EW; i++) v[i] = x; }
};
struct iN {
  int v[EW];
  iN() {}
  iN(int x) { for (int i = 0; i < EW; i++) v[i] = x; }
};
struct dN {
  double v[EW];
  dN() {}
  explicit dN(double x) { for (int i = 0; i < EW; i++) v[i] = x; }
};

#define EMU_BIN(T, OP) \
  inline T operator OP(const T& a, const T& b) { T r; for (int i = 0; i < EW; i++) r.v[i] = a.v[i] OP b.v[i]; return r; }
#define EMU_BIN_S(T, S, OP) \
  inline T operator OP(const T& a, S b) { T r; for (int i = 0; i < EW; i++) r.v[i] = a.v[i] OP b; return r; } \
  inline T operator OP(S a, const T& b) { T r; for (int i = 0; i < EW; i++) r.v[i] = a OP b.v[i]; return r; }
#define EMU_CMP(T, OP) \
  inline bN operator OP(const T& a, const T& b) { bN r; for (int i = 0; i < EW; i++) r.v[i] = a.v[i] OP b.v[i]; return r; }
#define EMU_CMP_S(T, S, OP) \
  inline bN operator OP(const T& a, S b) { bN r; for (int i = 0; i < EW; i++) r.v[i] = a.v[i] OP b; return r; }
EMU_BIN(fN, +) EMU_BIN(fN, -) EMU_BIN(fN, *) EMU_BIN(fN, /)
EMU_BIN_S(fN, float, +) EMU_BIN_S(fN, float, -) EMU_BIN_S(fN, float, *) EMU_BIN_S(fN, float, /)
EMU_CMP(fN, <) EMU_CMP(fN, >) EMU_CMP(fN, <=) EMU_CMP(fN, >=)
EMU_CMP_S(fN, float, <) EMU_CMP_S(fN, float, >) EMU_CMP_S(fN, float, <=) EMU_CMP_S(fN, float, >=)
EMU_BIN(iN, +) EMU_BIN(iN, -) EMU_BIN(iN, *)
EMU_BIN_S(iN, int, +) EMU_BIN_S(iN, int, -) EMU_BIN_S(iN, int, *)
EMU_CMP(iN, <) EMU_CMP(iN, >)
EMU_CMP_S(iN, int, <) EMU_CMP_S(iN, int, >)
EMU_BIN(dN, +) EMU_BIN(dN, -) EMU_BIN(dN, *)
EMU_BIN_S(dN, double, +) EMU_BIN_S(dN, double, -) EMU_BIN_S(dN, double, *)

namespace lm {
#define EMU_UN(NAME, FN) inline fN NAME(const fN& a) { fN r; for (int i = 0; i < EW; i++) r.v[i] = FN(a.v[i]); return r; }
EMU_UN(sqrt_, sqrtf) EMU_UN(abs_, fabsf) EMU_UN(rint_, rintf)
inline fN atan2_(const fN& y, const fN& x) { fN r; for (int i = 0; i < EW; i++) r.v[i] = atan2f(y.v[i], x.v[i]); return r; }
EMU_UN(sin_, sinf) EMU_UN(cos_, cosf)
inline fN nfma_(const fN& a, const fN& b, const fN& c) { fN r; for (int i = 0; i < EW; i++) r.v[i] = fmaf(-a.v[i], b.v[i], c.v[i]); return r; }
inline fN rsqrt_(const fN& a) { fN r; for (int i = 0; i < EW; i++) r.v[i] = 1.0f / sqrtf(a.v[i]); return r; }
inline fN min_(const fN& a, const fN& b) { fN r; for (int i = 0; i < EW; i++) r.v[i] = fminf(a.v[i], b.v[i]); return r; }
inline fN max_(const fN& a, const fN& b) { fN r; for (int i = 0; i < EW; i++) r.v[i] = fmaxf(a.v[i], b.v[i]); return r; }
inline fN med3_(const fN& x, const fN& lo, const fN& hi) { fN r; for (int i = 0; i < EW; i++) r.v[i] = fminf(fmaxf(x.v[i], lo.v[i]), hi.v[i]); return r; }
inline fN sel(const bN& m, const fN& a, const fN& b) { fN r; for (int i = 0; i < EW; i++) r.v[i] = m.v[i] ? a.v[i] : b.v[i]; return r; }
inline iN sel(const bN& m, const iN& a, const iN& b) { iN r; for (int i = 0; i < EW; i++) r.v[i] = m.v[i] ? a.v[i] : b.v[i]; return r; }
inline bN and_(const bN& a, const bN& b) { bN r; for (int i = 0; i < EW; i++) r.v[i] = a.v[i] && b.v[i]; return r; }
inline bN or_(const bN& a, const bN& b) { bN r; for (int i = 0; i < EW; i++) r.v[i] = a.v[i] || b.v[i]; return r; }
inline bN not_(const bN& a) { bN r; for (int i = 0; i < EW; i++) r.v[i] = !a.v[i]; return r; }
inline bN odd_(const iN& k) { bN r; for (int i = 0; i < EW; i++) r.v[i] = (k.v[i] & 1) != 0; return r; }
inline bN bit1_(const iN& k) { bN r; for (int i = 0; i < EW; i++) r.v[i] = (k.v[i] & 2) != 0; return r; }
}  // namespace lm

// Two robots of one SEPMC arena run as two host threads; peer() is their rendezvous (on the GPU: the neighbouring 16-lane row
// of the same wave, v_permlane16_swap).  Both sides must make the same sequence of peer() calls.
struct PairLink {
  fN box[2];
  std::atomic<int> arrived{0};
  std::atomic<int> phase{0};
  void barrier() {
    const int ph = phase.load(std::memory_order_acquire);
    if (arrived.fetch_add(1, std::memory_order_acq_rel) == 1) {
      arrived.store(0, std::memory_order_relaxed);
      phase.store(ph + 1, std::memory_order_release);
    } else {
      while (phase.load(std::memory_order_acquire) == ph) std::this_thread::yield();
    }
  }
};

struct HostLanes {
  static constexpr bool kHoldLink = false;
  typedef fN F;
  typedef iN I;
  typedef dN D;
  typedef bN B;
  struct F2 { fN x, y; };
  static F2 pair(const F& a, const F& b) { F2 r; r.x = a; r.y = b; return r; }
  const float* candc_;    // [words][16]

  PairLink* link_ = nullptr;
  int side_ = 0;

  explicit HostLanes(const float* candc) : candc_(candc) {}
  F peer(const F& x) const {
    link_->box[side_] = x;
    link_->barrier();
    F r = link_->box[1 - side_];
    link_->barrier();
    return r;
  }
  float peer_u(float x) const { return peer(fN(x)).v[0]; }
  void refresh_consts() const {}
  void new_step() {}
  static constexpr int kParamsReload = 0;
  static constexpr bool kPrefetchShapes = true;     // (the host build runs the read-ahead variant: it reads one record past the list)
  template <class T>
  const T& params(const T& as_passed) const { return as_passed; }
  bool lane0() const { return true; }
  int ray_first() const { return 0; }
  int ray_stride() const { return 1; }
  static constexpr int kRayChunk = 7;           // (the host build runs the chunked ray loops of the one-wave-per-SIMD kernels)
  uint32_t row_ballot(bool pred) const { return pred ? 1u : 0u; }      // (per-env scalar code runs once here: a "row" of one lane)
  void row_sync() const {}
  // (really through the scratch, so that step_env<PARK = true> -- LL_EMUL_PARK=1 -- checks on the host that nothing the substep loop changes is lost)
  void park_row(const float* v, int n, int at) const { for (int i = 0; i < n; i++) scratch_[at + i] = v[i]; }
  void unpark_row(float* v, int n, int at) const { for (int i = 0; i < n; i++) v[i] = scratch_[at + i]; }
  const float* stage_row(const float* g, int) const { return g; }
  alignas(16) mutable float scratch_[688];   // = PMC_ROW_SCRATCH (lanes.hpp, included later); checked below
  float* row_scratch() const { return scratch_; }
  static constexpr bool kConeInLds = false;          // (lanes.hpp WithConeInLds; emul.cpp runs that variant under LL_EMUL_PARK)
  static constexpr int kConeLdsAt = 64;              // = CONE_LDS_AT (lanes.hpp, included later); checked in emul.cpp
  void cone_store(int kind, int S, const F& a, const F& b, const F& c, const F& d) const {
    for (int i = 0; i < EW; i++) { float* w = scratch_ + kConeLdsAt + ((kind * 4 + S) * 16 + i) * 4; w[0] = a.v[i]; w[1] = b.v[i]; w[2] = c.v[i]; w[3] = d.v[i]; }
  }
  void cone_load(int kind, int S, F& a, F& b, F& c, F& d) const {
    for (int i = 0; i < EW; i++) { const float* w = scratch_ + kConeLdsAt + ((kind * 4 + S) * 16 + i) * 4; a.v[i] = w[0]; b.v[i] = w[1]; c.v[i] = w[2]; d.v[i] = w[3]; }
  }
  void prepare_turn_masks() const {}
  I leg() const { iN r; for (int i = 0; i < EW; i++) r.v[i] = i >> 2; return r; }
  I sub() const { iN r; for (int i = 0; i < EW; i++) r.v[i] = i & 3; return r; }
  F legf() const { fN r; for (int i = 0; i < EW; i++) r.v[i] = (float)(i >> 2); return r; }
  B is_leg(int l) const { bN r; for (int i = 0; i < EW; i++) r.v[i] = ((i >> 2) == l); return r; }
  B is_sub(int k) const { bN r; for (int i = 0; i < EW; i++) r.v[i] = ((i & 3) == k); return r; }
  B is_lane(int L) const { bN r; for (int i = 0; i < EW; i++) r.v[i] = (i == L); return r; }
  F lane_f(float x) const { return fN(x); }
  // How close this twin is to GpuLanes, one primitive at a time, is recorded in the class table of tests/lane_prims_common.py and held by tests/test_gpu_lane_prims.py:
  //   * moves (broadcasts, gathers, selects, mins, loads / stores) and the plain sums below are the GPU's bit for bit: qsum, subsum, rsum6, qsum6, subsum3 and sufsum*
  //     follow the association of the DPP trees in lanes.hpp, and an add rounds once on both sides;
  //   * whatever multiplies and adds (fmac_rbcast, gram*, turns*, cone_turns4, vel_*) is the GPU's only to rounding: every multiply-add here is a product and a sum
  //     (-ffp-contract=off), the GPU's v_fmac / v_fma / MFMA round once.  On inputs whose products and sums are exact the two agree bit for bit.
  static float qsum(const F& x) { return (x.v[0] + x.v[8]) + (x.v[4] + x.v[12]); }                 // over legs, leg-uniform input
  static F subsum(const F& x) { fN r; for (int q = 0; q < 4; q++) { float s = (x.v[4 * q] + x.v[4 * q + 1]) + (x.v[4 * q + 2] + x.v[4 * q + 3]); for (int k = 0; k < 4; k++) r.v[4 * q + k] = s; } return r; }
  static F submin(const F& x) { fN r; for (int q = 0; q < 4; q++) { float s = fminf(fminf(x.v[4 * q], x.v[4 * q + 1]), fminf(x.v[4 * q + 2], x.v[4 * q + 3])); for (int k = 0; k < 4; k++) r.v[4 * q + k] = s; } return r; }
  static void rsum6(const F* x, float* out) { for (int i = 0; i < 6; i++) out[i] = qsum(subsum(x[i])); }
  static void qsum6(const F* x, float* out) { for (int i = 0; i < 6; i++) out[i] = qsum(x[i]); }
  static void subsum3(const F* x, F* out) { for (int i = 0; i < 3; i++) out[i] = subsum(x[i]); }
  template <int L_> static float rbcast(const F& x) { return x.v[L_]; }
  // work split over the sub-lanes by link (lanes.hpp): suffix sums over the sub-lanes (sub-lane 3 holds zero), broadcasts of a sub-lane's values
  static void sufsum6(F* x) { for (int i = 0; i < 6; i++) sufsum1(x[i]); }
  static void sufsum4(F* x) { for (int i = 0; i < 4; i++) sufsum1(x[i]); }
  static void sufsum1(F& x) {
    fN t, r;
    static const int p1[4] = {1, 2, 3, 3}, p2[4] = {2, 3, 3, 3};
    for (int i = 0; i < EW; i++) t.v[i] = x.v[(i & ~3) | p1[i & 3]] + x.v[i];
    for (int i = 0; i < EW; i++) r.v[i] = t.v[(i & ~3) | p2[i & 3]] + t.v[i];
    x = r;
  }
  template <int K_> static void subbcast6(const F* x, F* out) { for (int i = 0; i < 6; i++) out[i] = subbcast<K_>(x[i]); }
  template <int K_> static void subbcast6_after(const F* x, F* out, const F&) { subbcast6<K_>(x, out); }
  static void gather_tri3(const F* d, F* m) {
    m[0] = subbcast<0>(d[0]); m[1] = subbcast<1>(d[0]); m[2] = subbcast<1>(d[1]); m[3] = subbcast<2>(d[0]); m[4] = subbcast<2>(d[1]); m[5] = subbcast<2>(d[2]);
  }
  static void spread3(const F& x, F* out) { out[0] = subbcast<0>(x); out[1] = subbcast<1>(x); out[2] = subbcast<2>(x); }
  template <int K_> static F subbcast(const F& x) { fN r; for (int i = 0; i < EW; i++) r.v[i] = x.v[(i & ~3) | K_]; return r; }
  template <int LEG_> static float bcast(const F& x) { return x.v[4 * LEG_]; }
  template <int L_> static void fmac_rbcast(F& acc, const F& x, const F& k) { for (int i = 0; i < EW; i++) acc.v[i] = acc.v[i] + x.v[L_] * k.v[i]; }
  template <int L_> static void fmac_rbcast_settled(F& acc, const F& x, const F& k) { fmac_rbcast<L_>(acc, x, k); }
  static F settle(const F& x) { return x; }
  static constexpr bool kGram16 = false;       // (as the shipped GPU build: lanes.hpp LL_MFMA_GRAM)
  static void gram16(const F* x, const F* y, F* g) {     // lanes.hpp GpuLanes::gram16: g[L] = sum_i y[i] * (x[i] of lane L), in the order the MFMA chain accumulates (i = 0 .. 5) but with product and sum rounded separately
    for (int L_ = 0; L_ < EW; L_++) {
      for (int l = 0; l < EW; l++) g[L_].v[l] = 0.0f;
      for (int i = 0; i < 6; i++) for (int l = 0; l < EW; l++) g[L_].v[l] = g[L_].v[l] + x[i].v[L_] * y[i].v[l];
    }
  }
  // lanes.hpp GpuLanes::gram_mfma / gram_collect (WithGramPipe): the same sums, one k at a time, in the order the MFMA chain accumulates (unfused, as gram16 above)
  static constexpr bool kGramPipe = false;           // (emul.cpp runs the piped variant under LL_EMUL_GRAM_PIPE)
  struct GramAcc { fN g[EW]; };
  template <int K_> static void gram_mfma(GramAcc& a, const F& x, const F& y) {
    for (int L_ = 0; L_ < EW; L_++) for (int l = 0; l < EW; l++) a.g[L_].v[l] = (K_ == 0 ? 0.0f : a.g[L_].v[l]) + x.v[L_] * y.v[l];
  }
  static void gram_collect(const GramAcc& a, F* g) { for (int L_ = 0; L_ < EW; L_++) g[L_] = a.g[L_]; }
  template <int S_> static void gram4(const F* x, const F* y, F* g) {
    for (int t = 0; t < 4; t++) {
      const int L_ = 4 * t + S_;
      for (int i = 0; i < 6; i++) for (int l = 0; l < EW; l++) g[L_].v[l] = g[L_].v[l] + x[i].v[L_] * y[i].v[l];
    }
  }
  template <int S_, bool NEG_LO = false> static void turns4(F& u, F& dl, const F& lo_in, const F& hi, const F& k0, const F& k1, const F& k2, const F& k3) {
    const F* ks[4] = {&k0, &k1, &k2, &k3};
    fN lo = lo_in;
    if (NEG_LO) for (int l = 0; l < EW; l++) lo.v[l] = -lo_in.v[l];      // the negation the GPU takes (lo = 0 gives -0, and med3 hands that sign on), not 0 - lo
    for (int t = 0; t < 4; t++) {
      const int L_ = 4 * t + S_;
      fN d = lm::med3_(u, lo, hi);
      dl.v[L_] = d.v[L_];
      for (int l = 0; l < EW; l++) u.v[l] = u.v[l] + d.v[L_] * ks[t]->v[l];
    }
  }
  template <int H_, bool NEG_LO = false> static void turns8(F& u, F& dl, const F& lo_in, const F& hi, const F* nk) {
    fN lo = lo_in;
    if (NEG_LO) for (int l = 0; l < EW; l++) lo.v[l] = -lo_in.v[l];      // the negation the GPU takes (lo = 0 gives -0, and med3 hands that sign on), not 0 - lo
    const int order[2][8] = {{0, 4, 8, 12, 1, 5, 9, 13}, {2, 6, 10, 14, 3, 7, 11, 15}};
    for (int t = 0; t < 8; t++) {
      const int L_ = order[H_][t];
      fN d = lm::med3_(u, lo, hi);
      dl.v[L_] = d.v[L_];
      for (int l = 0; l < EW; l++) u.v[l] = u.v[l] + d.v[L_] * nk[L_].v[l];
    }
  }
  // four cone-coupled friction turns (lanes.hpp cone_turns4): v_mul_legacy (0 * anything = 0) with clamp, v_rsq(0) = inf
  template <int S_> static void cone_turns4(F& S1, F& S2, F& d1, F& d2, const F& lam1, const F& lam2, const F& lim, const F* k11, const F* k12, const F* k21, const F* k22) {
    for (int t = 0; t < 4; t++) {
      const int L_ = 4 * t + S_;
      fN e1, e2;
      for (int l = 0; l < EW; l++) {
        const float len2 = fmaf(S1.v[l], S1.v[l], S2.v[l] * S2.v[l]);
        const float r = len2 > 0.0f ? 1.0f / sqrtf(len2) : INFINITY;
        const float sc = (lim.v[l] == 0.0f || r == 0.0f) ? 0.0f : fminf(fmaxf(lim.v[l] * r, 0.0f), 1.0f);
        e1.v[l] = fmaf(S1.v[l], sc, -lam1.v[l]); e2.v[l] = fmaf(S2.v[l], sc, -lam2.v[l]);
      }
      d1.v[L_] = e1.v[L_]; d2.v[L_] = e2.v[L_];
      for (int l = 0; l < EW; l++) {
        S1.v[l] = (S1.v[l] + e1.v[L_] * k11[L_].v[l]) + e2.v[L_] * k12[L_].v[l];
        S2.v[l] = (S2.v[l] + e1.v[L_] * k21[L_].v[l]) + e2.v[L_] * k22[L_].v[l];
      }
    }
  }
  // the solver's scattered velocity state (lanes.hpp): VA[l] = dx[l & 3], VB[l] = dx[4 + (l & 1)], VJ[l] = dq_leg[l & 3];
  // ca[k][l] = gt[(l & 3) ^ k], cb[k][l] = gt[4 + (((l & 3) ^ k) & 1)], cj[k][l] = jt[(l & 3) ^ k]
  static F vel_dot(const F& c, const F2& ca01, const F2& ca23, const F2& cb01, const F2& cj01, const F2& cj23, const F& VA, const F& VB, const F& VJ) {
    const fN* ca[4] = {&ca01.x, &ca01.y, &ca23.x, &ca23.y};
    const fN* cb[2] = {&cb01.x, &cb01.y};
    const fN* cj[4] = {&cj01.x, &cj01.y, &cj23.x, &cj23.y};
    fN w;
    for (int l = 0; l < EW; l++) {
      float a = ca[0]->v[l] * VA.v[l] + c.v[l];
      a += cb[0]->v[l] * VB.v[l];
      a += cj[0]->v[l] * VJ.v[l];
      for (int k = 1; k < 4; k++) a += ca[k]->v[l] * VA.v[l ^ k];
      a += cb[1]->v[l] * VB.v[l ^ 1];
      for (int k = 1; k < 4; k++) a += cj[k]->v[l] * VJ.v[l ^ k];
      w.v[l] = a;
    }
    return w;
  }
  // (the sixteen products of a value are summed in LANE ORDER here; the GPU reduces them in a quad-exchange tree followed by row_ror 4 and 8 -- another association: equal to rounding only)
  static void vel_commit(const F& dl, F& lam, const F2& ca01, const F2& ca23, const F2& cb01, const F2& cj01, const F2& cj23, F& VA, F& VB, F& VJ) {
    const fN* ca[4] = {&ca01.x, &ca01.y, &ca23.x, &ca23.y};
    const fN* cb[2] = {&cb01.x, &cb01.y};
    const fN* cj[4] = {&cj01.x, &cj01.y, &cj23.x, &cj23.y};
    float tA[4] = {0, 0, 0, 0}, tB[2] = {0, 0}, tJ[4][4] = {{0}};
    lam = lam + dl;
    for (int l = 0; l < EW; l++) {
      const int s = l & 3;
      for (int k = 0; k < 4; k++) { tA[s ^ k] += ca[k]->v[l] * dl.v[l]; tJ[l >> 2][s ^ k] += cj[k]->v[l] * dl.v[l]; }
      for (int k = 0; k < 2; k++) tB[(s ^ k) & 1] += cb[k]->v[l] * dl.v[l];
    }
    for (int l = 0; l < EW; l++) { VA.v[l] += tA[l & 3]; VB.v[l] += tB[l & 1]; VJ.v[l] += tJ[l >> 2][l & 3]; }
  }
  static void vel_commit2(const F& dl1, F& lam1, const F2& a01, const F2& a23, const F2& b01, const F2& j01, const F2& j23,
                          const F& dl2, F& lam2, const F2& c01, const F2& c23, const F2& e01, const F2& k01, const F2& k23, F& VA, F& VB, F& VJ) {
    vel_commit(dl1, lam1, a01, a23, b01, j01, j23, VA, VB, VJ);
    vel_commit(dl2, lam2, c01, c23, e01, k01, k23, VA, VB, VJ);
  }
  template <int I_> static float vel_dx(const F& VA, const F& VB) { return I_ < 4 ? VA.v[I_ & 3] : VB.v[I_ & 1]; }
  template <int J_> static F vel_dq(const F& VJ) { fN r; for (int i = 0; i < EW; i++) r.v[i] = VJ.v[(i & ~3) | J_]; return r; }
  static F from_prev_leg(const F& x) { fN r; for (int i = 0; i < EW; i++) r.v[i] = x.v[(i + 12) & 15]; return r; }
  static F from_next_leg(const F& x) { fN r; for (int i = 0; i < EW; i++) r.v[i] = x.v[(i + 4) & 15]; return r; }
  static F from_leg2(const F& x) { fN r; for (int i = 0; i < EW; i++) r.v[i] = x.v[(i + 8) & 15]; return r; }
  static float rmin(const F& x) { float m = x.v[0]; for (int i = 1; i < EW; i++) m = fminf(m, x.v[i]); return m; }
  static bool any(const B& m) { for (int i = 0; i < EW; i++) if (m.v[i]) return true; return false; }
  F legc(const float* tbl, int field) const { fN r; for (int i = 0; i < EW; i++) r.v[i] = tbl[field * 4 + (i >> 2)]; return r; }
  float basec(const float* bc, int i) const { return bc[i]; }
  F candc(int word) const { fN r; for (int i = 0; i < EW; i++) r.v[i] = candc_[word * 16 + i]; return r; }
  F candc_of(const I& sub2, const I& word) const { fN r; for (int i = 0; i < EW; i++) r.v[i] = candc_[word.v[i] * 16 + (i & ~3) + sub2.v[i]]; return r; }
  F pick3(float x, float y, float z) const { fN r; for (int i = 0; i < EW; i++) r.v[i] = (i >> 2) == 0 ? x : ((i >> 2) == 1 ? y : z); return r; }
  F ldl(const float* p, long base, long stride) const { fN r; for (int i = 0; i < EW; i++) r.v[i] = p[base + stride * (i >> 2)]; return r; }
  void stl(float* p, long base, long stride, const F& v) const { for (int i = 0; i < EW; i += 4) p[base + stride * (i >> 2)] = v.v[i]; }
  void stl_if(const B& m, float* p, long base, long stride, const F& v) const { for (int i = 0; i < EW; i += 4) if (m.v[i]) p[base + stride * (i >> 2)] = v.v[i]; }
  void copy16(float* dst, const float* src, int i0, int n) const { for (int i = i0; i < i0 + EW && i < n; i++) dst[i] = src[i]; }
  F ld16(const float* src, int i0, int n) const { fN r; for (int i = 0; i < EW; i++) r.v[i] = (i0 + i < n) ? src[i0 + i] : 0.0f; return r; }
  void st16(float* dst, int i0, int n, const F& v) const { for (int i = 0; i < EW; i++) if (i0 + i < n) dst[i0 + i] = v.v[i]; }
  void st16_rot(float* dst, int i0, int n, int split, const F& v) const { for (int k = 0; k < EW; k++) { const int i = i0 + k; if (i < n) dst[i < split ? i + (n - split) : i - split] = v.v[k]; } }
  int count_le16(const double* p, int n, double u) const { int c = 0; for (int i = 0; i < n; i++) c += (p[i] <= u) ? 1 : 0; return c; }
  I pick4i(int a, int b, int c, int d) const { const int v[4] = {a, b, c, d}; iN r; for (int i = 0; i < EW; i++) r.v[i] = v[i >> 2]; return r; }
  D pick4d(double a, double b, double c, double d) const { const double v[4] = {a, b, c, d}; dN r; for (int i = 0; i < EW; i++) r.v[i] = v[i >> 2]; return r; }
  D ldd_idx(const double* p, const I& idx) const { dN r; for (int i = 0; i < EW; i++) r.v[i] = p[idx.v[i]]; return r; }
  D lddl(const double* p, long base, long stride) const { dN r; for (int i = 0; i < EW; i++) r.v[i] = p[base + stride * (i >> 2)]; return r; }
  static F d2f(const D& x) { fN r; for (int i = 0; i < EW; i++) r.v[i] = (float)x.v[i]; return r; }
  static F i2f(const I& x) { fN r; for (int i = 0; i < EW; i++) r.v[i] = (float)x.v[i]; return r; }
  static I f2i(const F& x) { iN r; for (int i = 0; i < EW; i++) r.v[i] = (int)x.v[i]; return r; }
};

// lanes.hpp WithGramPipe for the host lanes (emul.cpp: LL_EMUL_GRAM_PIPE runs the contact rows through the piped Gram statement)
template <class Base>
struct WithGramPipeHost : Base {
  using Base::Base;
  static constexpr bool kGramPipe = true;
};

// lanes.hpp WithConeInLds for the host lanes (emul.cpp: LL_EMUL_PARK runs the cone round's cross scalars through the row scratch)
template <class Base>
struct WithConeInLdsHost : Base {
  using Base::Base;
  static constexpr bool kConeInLds = true;
};

// Device helpers for the backward pass.
//
// bwd_through_store: a gradient wrt the previous stage's OUTPUT element (b, y, x, c) is
// multiplied by that stage's (regenerated) dropout mask and ReLU mask (from its saved
// output) and stored AT THE SAME RESOLUTION.  For a max-pooled stage this is dP, the
// gradient at pooled resolution; the full-resolution gradient dY is never materialised:
// consumers rebuild it on load from (dP, argmax code) -- see unpool_load8.
#pragma once
#include <type_traits>

#include "args.h"

__device__ __forceinline__ void bwd_through_store(const BwdThrough& t, int b, int y, int x, int c,
                                                  float g, uint32_t step) {
  if (c >= t.pCs) return;
  const size_t qi = ((size_t)b * t.pH + y) * t.pW + x;
  if (c >= t.pC) {
    g = 0.f;
  } else {
    if (t.drop_thr) {
      const uint32_t idx = (uint32_t)(qi * (size_t)t.pC + c);
      g = dropout_keep(idx, t.seed, t.stream_id, step, t.drop_thr) ? g * t.drop_scale : 0.f;
    }
    if (t.prev_relu) {
      const float a = bf2f(t.prev_out[qi * t.pCs + c]);
      if (!(a > 0.f)) g = 0.f;
    }
  }
  t.dy[qi * t.pCs + c] = f2bf(g);
}

// Where bwd_through_store8 reads the geometry of the previous stage (CV_BT_INTS, args.h):
// BtGeoRt the BwdThrough fields; the fixed form is part of CvGeoFix (conv_halo_body.h).  The
// pointers and the dropout threshold / scale / seed / stream id always come from BwdThrough.
struct BtGeoRt {
#define F(n) \
  __device__ __forceinline__ static int n(const BwdThrough& t) { return t.n; }
  CV_BT_INTS(F)
#undef F
};

// Vectorised form: 8 consecutive channels [c0, c0+8) of output pixel qi (flat index over
// the previous stage's output grid); one 16-byte load of the saved output, one 16-byte store
// (bwd_through_store8, below).
// The two halves of it, for callers that know (qi, c0) long before they have the gradient: the
// load of the saved output needs nothing the kernel computes, so it can be in flight while the
// MFMAs run and only arithmetic and the store remain behind them.
//
// fetch8: the saved output's 8 values (zeros without a ReLU mask).  Branch-free: the load is
// always issued, so (qi, c0) must be an in-range chunk -- callers clamp.  (The _at forms take the
// element offset o = qi * pCs + c0, which store8 computes once for both halves; ALWAYS false: the
// load sits under the prev_relu test, the form bwd_through_store8 has always had.)
template <class G, bool ALWAYS>
__device__ __forceinline__ bf16x8 bwd_through_fetch8_at(const BwdThrough& t, size_t o) {
  if (ALWAYS) {
    const bf16x8 v = load_bf16x8(t.prev_out + o);
    return G::prev_relu(t) ? v : zero_bf16x8();
  }
  bf16x8 prev = zero_bf16x8();
  if (G::prev_relu(t)) prev = load_bf16x8(t.prev_out + o);
  return prev;
}
template <class G = BtGeoRt>
__device__ __forceinline__ bf16x8 bwd_through_fetch8(const BwdThrough& t, size_t qi, int c0) {
  return bwd_through_fetch8_at<G, true>(t, qi * G::pCs(t) + c0);
}

// finish8: dropout scale, then ReLU mask (prev: fetch8's value), then f2bf and the store.
// WHOLE: the caller has proved c0 + 8 <= pC (== pCs), no channel test is compiled.  HOIST: the
// dropout threshold is tested once per chunk instead of around each element's hash.
// (DROP 1 / 0: the chunk's dropout is known on / off, -1: the threshold is tested per element)
template <class G, bool WHOLE, int DROP>
__device__ __forceinline__ bf16x8 bwd_through_mask8(const BwdThrough& t, size_t qi, int c0, const float* g,
                                                    const bf16x8 prev, uint32_t step) {
  bf16x8 outv;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int c = c0 + k;
    float v = g[k];
    if (!WHOLE && c >= G::pC(t)) {
      v = 0.f;
    } else {
      if (DROP > 0 || (DROP < 0 && t.drop_thr))
        v = dropout_keep((uint32_t)(qi * (size_t)G::pC(t) + c), t.seed, t.stream_id, step, t.drop_thr) ? v * t.drop_scale
                                                                                                      : 0.f;
      if (G::prev_relu(t) && !(bf2f(prev[k]) > 0.f)) v = 0.f;
    }
    outv[k] = f2bf(v);
  }
  return outv;
}
template <class G, bool WHOLE, bool HOIST>
__device__ __forceinline__ void bwd_through_finish8_at(const BwdThrough& t, size_t qi, int c0, size_t o, const float* g,
                                                       const bf16x8 prev, uint32_t step) {
  bf16x8 outv;
  if (!HOIST) outv = bwd_through_mask8<G, WHOLE, -1>(t, qi, c0, g, prev, step);
  else if (t.drop_thr) outv = bwd_through_mask8<G, WHOLE, 1>(t, qi, c0, g, prev, step);
  else outv = bwd_through_mask8<G, WHOLE, 0>(t, qi, c0, g, prev, step);
  if (G::wt(t)) st_wt16(t.dy, (unsigned)(o * 2), __builtin_bit_cast(u32x4, outv));
  else *reinterpret_cast<bf16x8*>(t.dy + o) = outv;
}
template <class G, bool WHOLE>
__device__ __forceinline__ void bwd_through_finish8(const BwdThrough& t, size_t qi, int c0, const float* g,
                                                    const bf16x8 prev, uint32_t step) {
  bwd_through_finish8_at<G, WHOLE, true>(t, qi, c0, qi * G::pCs(t) + c0, g, prev, step);
}

// The composition (the load under the prev_relu test, the channel tests, the threshold tested
// per element: the form every run-time-geometry caller has always had).
template <class G = BtGeoRt>
__device__ __forceinline__ void bwd_through_store8(const BwdThrough& t, size_t qi, int c0, const float* g,
                                                   uint32_t step) {
  if (c0 >= G::pCs(t)) return;
  const size_t o = qi * G::pCs(t) + c0;
  bwd_through_finish8_at<G, false, false>(t, qi, c0, o, g, bwd_through_fetch8_at<G, false>(t, o), step);
}

// Full-resolution gradient of a max-pooled conv at pixel (y, x), channels [c, c+8), rebuilt
// from the pooled gradient dP [Hp][Wp][Cs] and the forward argmax codes (same layout).
// Pixels outside the 2*Hp x 2*Wp pooled area get no gradient (Keras 'valid' pooling).
// Branch-free: `ok` false (or a pixel outside the pooled area) yields zeros; the loads are
// always issued (from a clamped in-range address) so batches of them stay in flight.
__device__ __forceinline__ bf16x8 unpool_load8(const bf16* dP, const uint8_t* code, int Hp, int Wp, int Cs,
                                               int y, int x, int c, bool ok = true) {
  const int wy = y >> 1, wx = x >> 1;
  ok = ok && wy < Hp && wx < Wp && y >= 0 && x >= 0;
  const size_t o = ok ? ((size_t)wy * Wp + wx) * Cs + c : 0;
  const uint4 raw = *reinterpret_cast<const uint4*>(dP + o);
  const uint2 cw = *reinterpret_cast<const uint2*>(code + o);
  const uint32_t pos = ok ? (uint32_t)(((y & 1) << 1) | (x & 1)) : 0xFFu;
  // per 16-bit lane mask: keep element j iff code byte j == pos
  uint32_t m[4];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const uint32_t w = h ? cw.y : cw.x;
    const uint32_t k0 = ((w & 0xFF) == pos) ? 0x0000FFFFu : 0u;
    const uint32_t k1 = (((w >> 8) & 0xFF) == pos) ? 0xFFFF0000u : 0u;
    const uint32_t k2 = (((w >> 16) & 0xFF) == pos) ? 0x0000FFFFu : 0u;
    const uint32_t k3 = (((w >> 24) & 0xFF) == pos) ? 0xFFFF0000u : 0u;
    m[2 * h] = k0 | k1;
    m[2 * h + 1] = k2 | k3;
  }
  const uint4 v = {raw.x & m[0], raw.y & m[1], raw.z & m[2], raw.w & m[3]};
  return *reinterpret_cast<const bf16x8*>(&v);
}

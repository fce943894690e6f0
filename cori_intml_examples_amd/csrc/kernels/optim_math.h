// Keras-2.2 optimizer update of ONE element (Adam / AMSGrad / Adamax / Nadam / Adadelta / Adagrad /
// RMSprop / SGD with momentum / Nesterov), shared by the multi-tensor optimizer, the fused reduce+optimizer
// and the fused xGMI all-reduce+optimizer kernels.  Per-step scalars (bias-corrected LR,
// Nadam schedule) come from the device StepState written by the step bookkeeping.
#pragma once
#include "args.h"

template <int KIND>
__device__ __forceinline__ void opt_update(const OptimArgs& a, const StepState* st, float& p, float g, float* s0,
                                           float* s1, float* s2 = nullptr) {
  // The three kinds below run in optim_kernel (data-parallel step, fuse_optim=0) and in
  // reduce_optim_kernel (single-GPU step): no fp contraction, so both give the same bits
  // whatever the surrounding code lets the compiler fuse
  if (KIND == OPT_AMSGRAD) {          // s2: the running maximum of v (only this kind touches it)
#pragma clang fp contract(off)
    const float m = a.beta1 * *s0 + (1.f - a.beta1) * g;
    const float v = a.beta2 * *s1 + (1.f - a.beta2) * g * g;
    const float vhat = fmaxf(*s2, v);
    *s0 = m;
    *s1 = v;
    *s2 = vhat;
    p -= st->s[0] * m / (sqrtf(vhat) + a.eps);
  } else if (KIND == OPT_ADAMAX) {    // st->s[0] = lr / (1 - beta1^t)
#pragma clang fp contract(off)
    const float m = a.beta1 * *s0 + (1.f - a.beta1) * g;
    const float u = fmaxf(a.beta2 * *s1, fabsf(g));
    *s0 = m;
    *s1 = u;
    p -= st->s[0] * m / (u + a.eps);
  } else if (KIND == OPT_ADAGRAD) {
#pragma clang fp contract(off)
    const float acc = *s0 + g * g;
    *s0 = acc;
    p -= st->s[0] * g / (sqrtf(acc) + a.eps);
  } else if (KIND == OPT_ADAM) {
    const float m = a.beta1 * *s0 + (1.f - a.beta1) * g;
    const float v = a.beta2 * *s1 + (1.f - a.beta2) * g * g;
    *s0 = m;
    *s1 = v;
    p -= st->s[0] * m / (sqrtf(v) + a.eps);
  } else if (KIND == OPT_NADAM) {
    const float mc_t = st->s[0], mc_t1 = st->s[1];
    const float gp = g * st->s[2];
    const float m = a.beta1 * *s0 + (1.f - a.beta1) * g;
    const float v = a.beta2 * *s1 + (1.f - a.beta2) * g * g;
    *s0 = m;
    *s1 = v;
    const float mp = m * st->s[3];
    const float vp = v * st->s[4];
    const float mbar = (1.f - mc_t) * gp + mc_t1 * mp;
    p -= st->s[5] * mbar / (sqrtf(vp) + a.eps);
  } else if (KIND == OPT_ADADELTA) {
    const float acc = a.rho * *s0 + (1.f - a.rho) * g * g;
    const float upd = g * sqrtf(*s1 + a.eps) / sqrtf(acc + a.eps);
    *s0 = acc;
    p -= st->s[0] * upd;
    *s1 = a.rho * *s1 + (1.f - a.rho) * upd * upd;
  } else if (KIND == OPT_RMSPROP) {
    const float acc = a.rho * *s0 + (1.f - a.rho) * g * g;
    *s0 = acc;
    p -= st->s[0] * g / (sqrtf(acc) + a.eps);
  } else {   // SGD (+momentum / nesterov)
    const float lr = st->s[0];
    if (a.momentum != 0.f) {
      const float v = a.momentum * *s0 - lr * g;
      *s0 = v;
      p += a.nesterov ? (a.momentum * v - lr * g) : v;
    } else {
      p -= lr * g;
    }
  }
}

// Keras gradient clipping of ONE element (Optimizer.get_gradients): the global-norm factor
// first (c / norm when norm >= c, else exactly 1: the quotient is formed once per step by
// grad_sqnorm_kernel), then the clamp to [-v, v] when v > 0.  Comparisons, not fminf / fmaxf:
// a NaN gradient stays NaN.  No fp contraction: the product is a rounding of its own whatever
// consumes it, so a factor of 1 and v = inf-like bounds leave the update's bits unchanged.
__device__ __forceinline__ float clip_elem(float g, float factor, float v) {
#pragma clang fp contract(off)
  g = g * factor;
  if (v > 0.f) g = g < -v ? -v : (g > v ? v : g);
  return g;
}
// the clip factor and bound of a launch (CLIP instances): read once per thread
__device__ __forceinline__ float clip_factor(const OptimArgs& a) { return a.clip ? a.clip[CLIP_FACTOR] : 1.f; }
__device__ __forceinline__ float4 clip4(const OptimArgs& a, float4 g, float factor) {
  const float v = a.clipvalue;
  g.x = clip_elem(g.x, factor, v);
  g.y = clip_elem(g.y, factor, v);
  g.z = clip_elem(g.z, factor, v);
  g.w = clip_elem(g.w, factor, v);
  return g;
}

// The same for four consecutive elements at e (16-byte aligned): load p and the state (s0 / s1
// optional; s2 is touched by the OPT_AMSGRAD instances only and dead in every other one; with
// g also the gradient at a.g + e), update with the gradient scaled by grad_scale, store back.
template <int KIND>
__device__ __forceinline__ void opt_load4(const OptimArgs& a, long long e, float4& p, float4& s0, float4& s1,
                                          float4& s2, float4* g = nullptr) {
  p = *reinterpret_cast<const float4*>(a.p + e);
  if (g) *g = *reinterpret_cast<const float4*>(a.g + e);
  s0 = a.s0 ? *reinterpret_cast<const float4*>(a.s0 + e) : float4{0.f, 0.f, 0.f, 0.f};
  s1 = a.s1 ? *reinterpret_cast<const float4*>(a.s1 + e) : float4{0.f, 0.f, 0.f, 0.f};
  s2 = {0.f, 0.f, 0.f, 0.f};
  if constexpr (KIND == OPT_AMSGRAD) s2 = *reinterpret_cast<const float4*>(a.s2 + e);
}
template <int KIND>
__device__ __forceinline__ void opt_update4(const OptimArgs& a, const StepState* st, float4& p, const float4& g,
                                            float4& s0, float4& s1, float4& s2) {
  const float gs = a.grad_scale;
  opt_update<KIND>(a, st, p.x, g.x * gs, &s0.x, &s1.x, &s2.x);
  opt_update<KIND>(a, st, p.y, g.y * gs, &s0.y, &s1.y, &s2.y);
  opt_update<KIND>(a, st, p.z, g.z * gs, &s0.z, &s1.z, &s2.z);
  opt_update<KIND>(a, st, p.w, g.w * gs, &s0.w, &s1.w, &s2.w);
}
template <int KIND>
__device__ __forceinline__ void opt_store4(const OptimArgs& a, long long e, const float4& p, const float4& s0,
                                             const float4& s1, const float4& s2) {
  *reinterpret_cast<float4*>(a.p + e) = p;
  if (a.s0) *reinterpret_cast<float4*>(a.s0 + e) = s0;
  if (a.s1) *reinterpret_cast<float4*>(a.s1 + e) = s1;
  if constexpr (KIND == OPT_AMSGRAD) *reinterpret_cast<float4*>(a.s2 + e) = s2;
}

// ---------------------------------------------------------------------------------------
// bf16 copies of updated master elements into the fragment packs (routes: PackRoute, args.h).
// Fragment layout: pack[((ks*NT + nt)*64 + lane)*8 + j] = B[k = 32ks + 8(lane>>4) + j][n = 16nt + (lane&15)].
__device__ __forceinline__ long long frag_off(int k, int n, int NT) {
  return (long long)(((k >> 5) * NT + (n >> 4)) * 64 + ((((k >> 3) & 3) << 4) | (n & 15))) * 8 + (k & 7);
}

// element (outer o, inner c) of route R -> fwd (kf, c) and bwd (kb + c, nb) pack coordinates
__device__ __forceinline__ void route_coords(const PackRoute& R, int o, int& kf, int& kb, int& nb) {
  const int tap = o / R.Cin, ci = o - tap * R.Cin;
  kf = tap * R.Cs + ci;
  if (R.kind == 1) { kb = (R.KHW - 1 - tap) * R.Csb; nb = ci; }
  else { kb = 0; nb = kf; }
}

// one element e with its new value p
__device__ __forceinline__ void pack_write(const OptimArgs& a, int e, float p) {
  for (int r = 0; r < a.nroutes; ++r) {            // uniform loop: scalar loads of the route
    const PackRoute R = a.routes[r];
    if (e < R.lo || e >= R.hi) continue;
    const int le = e - R.lo, o = le / R.Cout, c = le - o * R.Cout;
    int kf, kb, nb;
    route_coords(R, o, kf, kb, nb);
    const bf16 v = f2bf(p);
    if (R.fwd >= 0) a.arena[R.fwd + frag_off(kf, c, R.NT)] = v;
    if (R.bwd >= 0) a.arena[R.bwd + frag_off(kb + c, nb, R.NTb)] = v;
  }
}

// four consecutive elements [e, e+4) (e % 4 == 0): one coordinate split when the group is one
// route's row run (Cout % 4 == 0, route start % 4 == 0): four 2-byte forward stores (n .. n+3:
// consecutive lanes of one fragment) and ONE 8-byte backward store (k .. k+3: consecutive j;
// the host sets a backward route only when its k base Csb is a multiple of 4)
__device__ __forceinline__ void pack_write4(const OptimArgs& a, int e, const float4& p) {
  for (int r = 0; r < a.nroutes; ++r) {
    const PackRoute R = a.routes[r];
    if (e + 4 <= R.lo || e >= R.hi) continue;
    if (e < R.lo || e + 4 > R.hi || ((R.Cout | (e - R.lo)) & 3)) {   // straddles / unaligned: per element
      const float v4[4] = {p.x, p.y, p.z, p.w};
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int eu = e + u;
        if (eu < R.lo || eu >= R.hi) continue;
        const int le = eu - R.lo, o = le / R.Cout, c = le - o * R.Cout;
        int kf, kb, nb;
        route_coords(R, o, kf, kb, nb);
        const bf16 v = f2bf(v4[u]);
        if (R.fwd >= 0) a.arena[R.fwd + frag_off(kf, c, R.NT)] = v;
        if (R.bwd >= 0) a.arena[R.bwd + frag_off(kb + c, nb, R.NTb)] = v;
      }
      continue;
    }
    const int le = e - R.lo, o = le / R.Cout, c = le - o * R.Cout;
    int kf, kb, nb;
    route_coords(R, o, kf, kb, nb);
    if (R.fwd >= 0) {
      bf16* d = a.arena + R.fwd + frag_off(kf, c, R.NT);
      d[0] = f2bf(p.x);
      d[8] = f2bf(p.y);
      d[16] = f2bf(p.z);
      d[24] = f2bf(p.w);
    }
    if (R.bwd >= 0) {
      bf16x4 v;
      v[0] = f2bf(p.x); v[1] = f2bf(p.y); v[2] = f2bf(p.z); v[3] = f2bf(p.w);
      *reinterpret_cast<bf16x4*>(a.arena + R.bwd + frag_off(kb + c, nb, R.NTb)) = v;
    }
  }
}

// Element-wise hidden activations of a Conv2D / Dense stage (Keras 2.2.4 keras/activations.py,
// LeakyReLU and ELU layers), as one streaming launch per direction behind the stage's linear
// kernels:
//
//   act_fwd_kernel   x = bf16(dropout(A(float(x))))            in place on the stage output
//   act_bwd_kernel   g = bf16(float(g) * A'(float(y) * y_scale))   in place on the stage's gradient
//
//   tanh          tanh(x)                               max(0, 1 - y^2)
//   sigmoid       1 / (1 + e^-x)                        max(0, y (1 - y))
//   hard_sigmoid  clip(0.2 x + 0.5, 0, 1)               0.2 if 0 < y < 1 else 0
//   elu           x > 0 ? x : alpha (e^x - 1)           y > 0 ? 1 : max(0, y + alpha)
//   selu          s elu(x, a)                           y > 0 ? s : max(0, y + s a)
//   softplus      max(x, 0) + log1p(e^-|x|)             max(0, -expm1(-y))
//   softsign      x / (1 + |x|)                         (1 - min(|y|, 1))^2
//   leaky_relu    x > 0 ? x : alpha x                   y > 0 ? 1 : alpha
//
// Every derivative is a function of the OUTPUT y and clamped to >= 0 (the clamp only acts on
// outputs that un-scaling a dropout-scaled bf16 value pushed out of the function's range).  The
// math library's tanhf / expm1f / log1pf / expf are used as they are: the cancellation forms
// (1 - 2 / (1 + e^2x), e^x - 1, 1 - e^-y) are wrong by thousands of bf16 ulps near zero.
//
// One thread per 8 channels: one 16-byte load (two in the backward), one 16-byte store, no LDS.
// Channels >= C go back bit for bit: they hold the zeros the next layer's MFMA k-padding reads,
// and A(0) != 0 for half of the table.
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>

#include "args.h"

#define ACT_THREADS 256
constexpr float SELU_SCALE = 1.0507009873554805f;
constexpr float SELU_ALPHA = 1.6732632423543772f;
constexpr float SELU_SA = (float)(1.0507009873554805 * 1.6732632423543772);

template <int ACT>
__device__ __forceinline__ float act_value(float x, float alpha) {
  if (ACT == ACT_TANH) return tanhf(x);
  if (ACT == ACT_SIGMOID) return 1.f / (1.f + expf(-x));
  if (ACT == ACT_HARD_SIGMOID) {
    const float v = 0.2f * x + 0.5f;          // (comparisons, not fminf / fmaxf: NaN stays NaN)
    return v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
  }
  if (ACT == ACT_ELU) return x > 0.f ? x : alpha * expm1f(x);
  if (ACT == ACT_SELU) return SELU_SCALE * (x > 0.f ? x : SELU_ALPHA * expm1f(x));
  if (ACT == ACT_SOFTPLUS) return (x > 0.f ? x : (x < 0.f ? 0.f : x)) + log1pf(expf(-fabsf(x)));
  if (ACT == ACT_SOFTSIGN) return isinf(x) ? copysignf(1.f, x) : x / (1.f + fabsf(x));
  // ACT_LEAKY_RELU (alpha = 0 is relu: 0 for every negative input, -inf included)
  return x > 0.f ? x : ((alpha == 0.f && x < 0.f) ? 0.f : alpha * x);
}

template <int ACT>
__device__ __forceinline__ float act_slope(float y, float alpha) {
  if (ACT == ACT_TANH) return fmaxf(0.f, 1.f - y * y);
  if (ACT == ACT_SIGMOID) return fmaxf(0.f, y * (1.f - y));
  if (ACT == ACT_HARD_SIGMOID) return (y > 0.f && y < 1.f) ? 0.2f : 0.f;
  if (ACT == ACT_ELU) return y > 0.f ? 1.f : fmaxf(0.f, y + alpha);
  if (ACT == ACT_SELU) return y > 0.f ? SELU_SCALE : fmaxf(0.f, y + SELU_SA);
  if (ACT == ACT_SOFTPLUS) return fmaxf(0.f, -expm1f(-y));
  if (ACT == ACT_SOFTSIGN) {
    const float d = 1.f - fminf(fabsf(y), 1.f);
    return d * d;
  }
  return y > 0.f ? 1.f : alpha;
}

// this thread's 8-channel group: row and first channel (false: past the end)
__device__ __forceinline__ bool act_group(const ActArgs& a, long long& row, int& c0, long long& off) {
  const unsigned gpr = (unsigned)a.Cs >> 3;
  const long long gi = (long long)blockIdx.x * ACT_THREADS + threadIdx.x;
  if (gi >= a.rows * gpr) return false;
  row = (gi >> 32) ? gi / gpr : (long long)((uint32_t)gi / gpr);
  c0 = (int)(gi - row * gpr) * 8;
  off = gi * 8;
  return true;
}

template <int ACT>
__global__ __launch_bounds__(ACT_THREADS) void act_fwd_kernel(const ActArgs a) {
  long long row, off;
  int c0;
  if (!act_group(a, row, c0, off)) return;
  const uint32_t step = a.st ? (uint32_t)a.st->t : 0u;
  const bf16x8 in = load_bf16x8(a.x + off);
  bf16x8 out = in;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int c = c0 + k;
    if (c < a.C) {
      float v = act_value<ACT>(bf2f(in[k]), a.alpha);
      if (a.drop_thr)
        v = dropout_keep((uint32_t)(row * a.C + c), a.seed, a.stream_id, step, a.drop_thr) ? v * a.drop_scale : 0.f;
      out[k] = f2bf(v);
    }
  }
  *reinterpret_cast<bf16x8*>(a.x + off) = out;
}

template <int ACT>
__global__ __launch_bounds__(ACT_THREADS) void act_bwd_kernel(const ActArgs a) {
  long long row, off;
  int c0;
  if (!act_group(a, row, c0, off)) return;
  const bf16x8 g = load_bf16x8(a.x + off);
  const bf16x8 y = load_bf16x8(a.y + off);
  bf16x8 out = g;
#pragma unroll
  for (int k = 0; k < 8; ++k)
    if (c0 + k < a.C) out[k] = f2bf(bf2f(g[k]) * act_slope<ACT>(bf2f(y[k]) * a.y_scale, a.alpha));
  *reinterpret_cast<bf16x8*>(a.x + off) = out;
}

static const ActRow* act_row(int act) {
  for (const ActRow& r : ACT_KINDS)
    if (r.id == act) return &r;
  return nullptr;
}

// the checks both launchers share; returns the workgroups of the launch (0: nothing to do)
static unsigned act_check(const ActArgs& a, const char* what, bool bwd) {
  const std::string w(what);
  const ActRow* r = act_row(a.act);
  if (!r) throw std::invalid_argument(w + ": unknown activation code " + std::to_string(a.act));
  if (r->has_alpha && !(a.alpha >= 0.f && std::isfinite(a.alpha)))
    throw std::invalid_argument(w + ": " + r->name + " needs a finite alpha >= 0");
  if (a.Cs <= 0 || a.Cs % 8) throw std::invalid_argument(w + ": the channel stride must be a positive multiple of 8");
  if (a.C <= 0 || a.C > a.Cs) throw std::invalid_argument(w + ": channels must be in [1, Cs]");
  if (a.rows < 0) throw std::invalid_argument(w + ": negative row count");
  if (!a.x || (reinterpret_cast<uintptr_t>(a.x) & 15)) throw std::invalid_argument(w + ": buffer pointer (null or not 16-byte aligned)");
  if (bwd && (!a.y || (reinterpret_cast<uintptr_t>(a.y) & 15)))
    throw std::invalid_argument(w + ": saved output pointer (null or not 16-byte aligned)");
  if (bwd && !(a.y_scale > 0.f && a.y_scale <= 1.f)) throw std::invalid_argument(w + ": y_scale must be in (0, 1]");
  if (!bwd && a.drop_thr && !(a.drop_scale >= 1.f && std::isfinite(a.drop_scale)))
    throw std::invalid_argument(w + ": dropout scale");
  const long long groups = a.rows * (a.Cs / 8);
  const long long blocks = (groups + ACT_THREADS - 1) / ACT_THREADS;
  if (blocks > 0x7fffffffLL) throw std::invalid_argument(w + ": buffer too large for one launch");
  return (unsigned)blocks;
}

#define ACT_DISPATCH(kernel)                                                                      \
  switch (a.act) {                                                                                \
    case ACT_TANH: hipLaunchKernelGGL(kernel<ACT_TANH>, grid, block, 0, s, a); break;             \
    case ACT_SIGMOID: hipLaunchKernelGGL(kernel<ACT_SIGMOID>, grid, block, 0, s, a); break;       \
    case ACT_HARD_SIGMOID: hipLaunchKernelGGL(kernel<ACT_HARD_SIGMOID>, grid, block, 0, s, a); break; \
    case ACT_ELU: hipLaunchKernelGGL(kernel<ACT_ELU>, grid, block, 0, s, a); break;               \
    case ACT_SELU: hipLaunchKernelGGL(kernel<ACT_SELU>, grid, block, 0, s, a); break;             \
    case ACT_SOFTPLUS: hipLaunchKernelGGL(kernel<ACT_SOFTPLUS>, grid, block, 0, s, a); break;     \
    case ACT_SOFTSIGN: hipLaunchKernelGGL(kernel<ACT_SOFTSIGN>, grid, block, 0, s, a); break;     \
    default: hipLaunchKernelGGL(kernel<ACT_LEAKY_RELU>, grid, block, 0, s, a); break;             \
  }

void launch_act_fwd(const ActArgs& a, hipStream_t s) {
  const unsigned blocks = act_check(a, "act_fwd", false);
  if (!blocks) return;
  const dim3 grid(blocks), block(ACT_THREADS);
  ACT_DISPATCH(act_fwd_kernel)
}

void launch_act_bwd(const ActArgs& a, hipStream_t s) {
  const unsigned blocks = act_check(a, "act_bwd", true);
  if (!blocks) return;
  const dim3 grid(blocks), block(ACT_THREADS);
  ACT_DISPATCH(act_bwd_kernel)
}

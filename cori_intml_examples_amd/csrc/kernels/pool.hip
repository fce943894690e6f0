// Keras AveragePooling2D (2x2 / stride 2 / 'valid'), GlobalAveragePooling2D and GlobalMaxPooling2D,
// as one streaming launch per direction around the stage's other kernels (PoolArgs, args.h):
//
//   pool_fwd, POOL_AVG2   out[b, hp, wp, c] = bf16(dropout(0.25 * ((a + b) + (c + d))))
//                         a b / c d the window of the stage's un-pooled stored activation x in
//                         row-major order; an odd leftover row / column is never read
//   pool_fwd, POOL_GAVG   out[b, c] = bf16(dropout(s * fp32(1 / (H * W))))
//                         s = (..((x[0] + x[1]) + x[2]) + ..) + x[H*W-1]: ONE fp32 chain over the map in
//                         row-major (y, x) order, started at x[0]
//   pool_fwd, POOL_GMAX   out[b, c] = bf16(dropout(max)), idx[b, c] = flat y * W + x of the FIRST maximum
//                         in row-major order (strict > against an accumulator started at x[0]: an
//                         all-negative channel returns its true maximum)
//   pool_bwd, POOL_AVG2   dz[b, y, x, c] = bf16(0.25 * dp[b, y / 2, x / 2, c] * (relu ? lin[b, y, x, c] > 0 : 1)),
//                         zero in the leftover odd row / column
//   pool_bwd, POOL_GAVG / POOL_GMAX   for every element (b, y, x, c) of the feeding stage's output grid
//                         g = dp[b, c] * fp32(1 / (H * W))   /   g = idx[b, c] == y * W + x ? dp[b, c] : 0
//                         handed to bwd_through_store8 with the feeding stage's BwdThrough (its dropout,
//                         relu mask and rounding, like any other consumer's gradient)
//
// One thread per 8 channels of one OUTPUT element: 16-byte loads and stores, fp32 arithmetic, one
// bf16 rounding per stored value, no LDS, no atomics, nothing shared between threads -- repeated
// launches are bit-identical.  The global forward's thread walks its WHOLE map alone (H * W loads,
// four in flight, added in order): there is no chunk length and no cross-thread combination, and
// the maps it is built for are the few hundred pixels behind a conv stack.  Channels >= C are
// written as zeros.  The dropout is the fused epilogues' counter at element row_out * C + c.
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>

#include "args.h"
#include "bwd_through.h"

#define POOL_THREADS 256

// this thread's (row, 8-channel group) of ``rows`` rows (false: past the end)
__device__ __forceinline__ bool pool_group(long long rows, int Cs, long long& row, int& c0) {
  const unsigned gpr = (unsigned)Cs >> 3;
  const long long gi = (long long)blockIdx.x * POOL_THREADS + threadIdx.x;
  if (gi >= rows * gpr) return false;
  row = (gi >> 32) ? gi / gpr : (long long)((uint32_t)gi / gpr);
  c0 = (int)(gi - row * gpr) * 8;
  return true;
}

// bf16(dropout(v[k])) of output row ``row``, channels [c0, c0 + 8); zeros at channels >= C
__device__ __forceinline__ bf16x8 pool_finish(const PoolArgs& a, long long row, int c0, const float* v) {
  const uint32_t step = a.st ? (uint32_t)a.st->t : 0u;
  bf16x8 out;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int c = c0 + k;
    float r = v[k];
    if (c >= a.C) {
      r = 0.f;
    } else if (a.drop_thr) {
      r = dropout_keep((uint32_t)(row * a.C + c), a.seed, a.stream_id, step, a.drop_thr) ? r * a.drop_scale : 0.f;
    }
    out[k] = f2bf(r);
  }
  return out;
}

__global__ __launch_bounds__(POOL_THREADS) void pool_avg2_fwd_kernel(const PoolArgs a) {
  const int Hp = a.H >> 1, Wp = a.W >> 1;
  long long q;
  int c0;
  if (!pool_group((long long)a.B * Hp * Wp, a.Cs, q, c0)) return;
  const int wp = (int)(q % Wp);
  const long long t = q / Wp;
  const int hp = (int)(t % Hp);
  const long long b = t / Hp;
  const long long base = ((b * a.H + 2 * hp) * a.W + 2 * wp) * a.Cs + c0;
  const bf16x8 p0 = load_bf16x8(a.x + base);
  const bf16x8 p1 = load_bf16x8(a.x + base + a.Cs);
  const bf16x8 p2 = load_bf16x8(a.x + base + (long long)a.W * a.Cs);
  const bf16x8 p3 = load_bf16x8(a.x + base + (long long)a.W * a.Cs + a.Cs);
  float v[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = 0.25f * ((bf2f(p0[k]) + bf2f(p1[k])) + (bf2f(p2[k]) + bf2f(p3[k])));
  *reinterpret_cast<bf16x8*>(a.out + q * a.Cs + c0) = pool_finish(a, q, c0, v);
}

template <int MODE>
__global__ __launch_bounds__(POOL_THREADS) void pool_global_fwd_kernel(const PoolArgs a) {
  long long b;
  int c0;
  if (!pool_group(a.B, a.Cs, b, c0)) return;
  const int n = a.H * a.W;
  const bf16* p = a.x + b * n * a.Cs + c0;
  const long long ld = a.Cs;
  float acc[8];
  int at[8];
  {
    const bf16x8 x0 = load_bf16x8(p);      // (no accumulator starts at zero)
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = bf2f(x0[k]), at[k] = 0;
  }
  auto take = [&](const bf16x8& x, int i) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float f = bf2f(x[k]);
      if (MODE == POOL_GAVG) {
        acc[k] += f;
      } else if (f > acc[k]) {             // strict: the FIRST maximum keeps the index
        acc[k] = f;
        at[k] = i;
      }
    }
  };
  int i = 1;
  for (; i + 4 <= n; i += 4) {             // four loads in flight, taken in order
    const bf16x8 x0 = load_bf16x8(p + (i + 0) * ld), x1 = load_bf16x8(p + (i + 1) * ld);
    const bf16x8 x2 = load_bf16x8(p + (i + 2) * ld), x3 = load_bf16x8(p + (i + 3) * ld);
    take(x0, i), take(x1, i + 1), take(x2, i + 2), take(x3, i + 3);
  }
  for (; i < n; ++i) take(load_bf16x8(p + i * ld), i);
  if (MODE == POOL_GAVG) {
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] *= a.inv_n;
  }
  *reinterpret_cast<bf16x8*>(a.out + b * a.Cs + c0) = pool_finish(a, b, c0, acc);
  if (MODE == POOL_GMAX && a.idx) {
    int4 lo, hi;
    lo.x = c0 + 0 < a.C ? at[0] : 0, lo.y = c0 + 1 < a.C ? at[1] : 0;
    lo.z = c0 + 2 < a.C ? at[2] : 0, lo.w = c0 + 3 < a.C ? at[3] : 0;
    hi.x = c0 + 4 < a.C ? at[4] : 0, hi.y = c0 + 5 < a.C ? at[5] : 0;
    hi.z = c0 + 6 < a.C ? at[6] : 0, hi.w = c0 + 7 < a.C ? at[7] : 0;
    int4* dst = reinterpret_cast<int4*>(a.idx + b * a.Cs + c0);
    dst[0] = lo;
    dst[1] = hi;
  }
}

__global__ __launch_bounds__(POOL_THREADS) void pool_avg2_bwd_kernel(const PoolArgs a) {
  const int Hp = a.H >> 1, Wp = a.W >> 1;
  long long r;
  int c0;
  if (!pool_group((long long)a.B * a.H * a.W, a.Cs, r, c0)) return;
  const int x = (int)(r % a.W);
  const long long t = r / a.W;
  const int y = (int)(t % a.H);
  const long long b = t / a.H;
  bf16x8 out = zero_bf16x8();
  if (y < 2 * Hp && x < 2 * Wp) {          // (a leftover odd row / column gets zeros)
    const bf16x8 g = load_bf16x8(a.dp + ((b * Hp + (y >> 1)) * Wp + (x >> 1)) * a.Cs + c0);
    bf16x8 lin = zero_bf16x8();
    if (a.relu) lin = load_bf16x8(a.lin + r * a.Cs + c0);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      float v = 0.25f * bf2f(g[k]);
      if (c0 + k >= a.C || (a.relu && !(bf2f(lin[k]) > 0.f))) v = 0.f;
      out[k] = f2bf(v);
    }
  }
  *reinterpret_cast<bf16x8*>(a.dz + r * a.Cs + c0) = out;
}

template <int MODE>
__global__ __launch_bounds__(POOL_THREADS) void pool_global_bwd_kernel(const PoolArgs a) {
  const int n = a.H * a.W;
  long long q;
  int c0;
  if (!pool_group((long long)a.B * n, a.Cs, q, c0)) return;
  const long long b = q / n;
  const int pos = (int)(q - b * n);
  const bf16x8 g = load_bf16x8(a.dp + b * a.Cs + c0);
  float v[8];
  if (MODE == POOL_GAVG) {
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = bf2f(g[k]) * a.inv_n;
  } else {
    const int4* src = reinterpret_cast<const int4*>(a.idx + b * a.Cs + c0);
    const int4 lo = src[0], hi = src[1];
    const int at[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = at[k] == pos ? bf2f(g[k]) : 0.f;
  }
  const uint32_t step = a.st ? (uint32_t)a.st->t : 0u;
  bwd_through_store8(a.bt, (size_t)q, c0, v, step);
}

static bool pool_bad_ptr(const void* p) { return !p || (reinterpret_cast<uintptr_t>(p) & 15); }

// the checks both launchers share; returns the workgroups of a launch over ``rows`` rows
static unsigned pool_check(const PoolArgs& a, const char* what, long long rows) {
  const std::string w(what);
  if (a.mode != POOL_AVG2 && a.mode != POOL_GAVG && a.mode != POOL_GMAX)
    throw std::invalid_argument(w + ": unknown pooling mode " + std::to_string(a.mode));
  if (a.Cs <= 0 || a.Cs % 8) throw std::invalid_argument(w + ": the channel stride must be a positive multiple of 8");
  if (a.C <= 0 || a.C > a.Cs) throw std::invalid_argument(w + ": channels must be in [1, Cs]");
  if (a.B < 0) throw std::invalid_argument(w + ": negative batch size");
  if (a.H <= 0 || a.W <= 0 || (long long)a.H * a.W > 0x7fffffffLL)
    throw std::invalid_argument(w + ": the input grid must be positive (and H * W below 2^31)");
  if (a.mode == POOL_AVG2 && (a.H < 2 || a.W < 2)) throw std::invalid_argument(w + ": a 2x2 window needs H, W >= 2");
  const long long groups = rows * (a.Cs / 8);
  const long long blocks = (groups + POOL_THREADS - 1) / POOL_THREADS;
  if (blocks > 0x7fffffffLL) throw std::invalid_argument(w + ": buffer too large for one launch");
  return (unsigned)blocks;
}

void launch_pool_fwd(const PoolArgs& a, hipStream_t s) {
  const char* w = "pool_fwd";
  const bool avg2 = a.mode == POOL_AVG2;
  const unsigned blocks = pool_check(a, w, avg2 ? (long long)a.B * (a.H / 2) * (a.W / 2) : (long long)a.B);
  if (pool_bad_ptr(a.x)) throw std::invalid_argument(std::string(w) + ": input pointer (null or not 16-byte aligned)");
  if (pool_bad_ptr(a.out)) throw std::invalid_argument(std::string(w) + ": output pointer (null or not 16-byte aligned)");
  if (a.idx && (a.mode != POOL_GMAX || (reinterpret_cast<uintptr_t>(a.idx) & 15)))
    throw std::invalid_argument(std::string(w) + ": index pointer (only POOL_GMAX takes one; 16-byte aligned)");
  if (a.drop_thr && !(a.drop_scale >= 1.f && std::isfinite(a.drop_scale)))
    throw std::invalid_argument(std::string(w) + ": dropout scale");
  if (!blocks) return;
  const dim3 grid(blocks), block(POOL_THREADS);
  PoolArgs k = a;
  k.inv_n = 1.f / (float)(a.H * a.W);
  if (avg2) hipLaunchKernelGGL(pool_avg2_fwd_kernel, grid, block, 0, s, k);
  else if (a.mode == POOL_GAVG) hipLaunchKernelGGL(pool_global_fwd_kernel<POOL_GAVG>, grid, block, 0, s, k);
  else hipLaunchKernelGGL(pool_global_fwd_kernel<POOL_GMAX>, grid, block, 0, s, k);
}

void launch_pool_bwd(const PoolArgs& a, hipStream_t s) {
  const std::string w("pool_bwd");
  const unsigned blocks = pool_check(a, "pool_bwd", (long long)a.B * a.H * a.W);
  if (pool_bad_ptr(a.dp)) throw std::invalid_argument(w + ": gradient pointer (null or not 16-byte aligned)");
  if (a.mode == POOL_AVG2) {
    if (pool_bad_ptr(a.dz)) throw std::invalid_argument(w + ": dz pointer (null or not 16-byte aligned)");
    if (a.relu && pool_bad_ptr(a.lin))
      throw std::invalid_argument(w + ": the relu mask needs the un-pooled activation (null or not 16-byte aligned)");
  } else {
    const BwdThrough& t = a.bt;
    if (t.pH != a.H || t.pW != a.W || t.pC != a.C || t.pCs != a.Cs)
      throw std::invalid_argument(w + ": the feeding stage's BwdThrough geometry differs from the pooled grid");
    if (pool_bad_ptr(t.dy)) throw std::invalid_argument(w + ": BwdThrough dy (null or not 16-byte aligned)");
    if (t.prev_relu && pool_bad_ptr(t.prev_out))
      throw std::invalid_argument(w + ": BwdThrough prev_out (null or not 16-byte aligned)");
    if (t.wt && (long long)a.B * a.H * a.W * a.Cs * 2 >= (1LL << 31))
      throw std::invalid_argument(w + ": write-through stores need a gradient buffer below 2 GB");
    if (t.drop_thr && !(t.drop_scale >= 1.f && std::isfinite(t.drop_scale)))
      throw std::invalid_argument(w + ": BwdThrough dropout scale");
    if (a.mode == POOL_GMAX && pool_bad_ptr(a.idx))
      throw std::invalid_argument(w + ": index pointer (null or not 16-byte aligned)");
  }
  if (!blocks) return;
  const dim3 grid(blocks), block(POOL_THREADS);
  PoolArgs k = a;
  k.inv_n = 1.f / (float)(a.H * a.W);
  if (a.mode == POOL_AVG2) hipLaunchKernelGGL(pool_avg2_bwd_kernel, grid, block, 0, s, k);
  else if (a.mode == POOL_GAVG) hipLaunchKernelGGL(pool_global_bwd_kernel<POOL_GAVG>, grid, block, 0, s, k);
  else hipLaunchKernelGGL(pool_global_bwd_kernel<POOL_GMAX>, grid, block, 0, s, k);
}

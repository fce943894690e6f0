// Keras BatchNormalization (axis -1) of a Conv2D / hidden Dense stage, as four launches around the
// stage's linear kernels, which store the un-pooled pre-activation z [rows][Cs] in bf16:
//
//   bn_stats_kernel      per row chunk and channel: the chunk's mean and its sum of squares ABOUT
//                        that mean (two passes over the chunk; never E[z^2] - E[z]^2)
//   bn_apply_fwd_kernel  every workgroup combines the chunk partials pairwise in one fixed order
//                        (Chan et al.: n, mean, M2), so all of them hold bit-identical statistics
//                        with no wait between workgroups; workgroup x = 0 stores mean / invstd for
//                        the backward and makes the moving update.  Then
//                          u = gamma * ((z - mean) * invstd) + beta,  [relu],  [2x2/2 max-pool with
//                          first-maximum codes (conv_code's format)],  [dropout],  ONE bf16 rounding
//                        The evaluation form reads the moving statistics instead (no bn_stats).
//   bn_bwd_reduce_kernel per row chunk and channel: partial dbeta = sum du, dgamma = sum du * xhat,
//                        du the pooled gradient routed to each window's argmax (zero elsewhere, the
//                        rows / columns an odd size leaves outside every window included).  The
//                        partials are slabs [chunk][dgamma[C], dbeta[C]] of an ordinary bias-like
//                        reduction (RedDesc) over gamma and beta, adjacent in the parameter store.
//   bn_bwd_apply_kernel  every workgroup sums the slabs in one fixed order, then
//                          dz = gamma * invstd * (du - dbeta / m - xhat * dgamma / m)   (bf16, dense)
//
// Thread map (all four): GP = the power of two >= min(Cs / 8, 32) channel groups side by side in
// a workgroup (consecutive lanes load consecutive 16-byte groups of a row), 256 / GP row lanes;
// blockIdx.y steps over blocks of GP groups.  Every cross-thread sum is a tree over the row lanes
// in LDS, in an order fixed by the geometry: no float atomics, launches repeat bit for bit.
// Channels >= C (z holds zeros there) get gamma = beta = 0, so every output keeps the zeros the
// next layer's MFMA k-padding reads.
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>

#include "args.h"

struct BnMap {
  int R;        // row lanes
  int gl, rl;   // this thread's group within the block, its row lane
  int c0;       // its first channel
  bool on;      // c0 < Cs
};

__device__ __forceinline__ BnMap bn_map(const BnArgs& a) {
  BnMap m;
  const int tid = threadIdx.x;
  m.R = BN_THREADS >> a.gp_log2;
  m.gl = tid & ((1 << a.gp_log2) - 1);
  m.rl = tid >> a.gp_log2;
  m.c0 = ((int)blockIdx.y * (1 << a.gp_log2) + m.gl) * 8;
  m.on = m.c0 < a.Cs;
  return m;
}

// v[k] summed over the row lanes of this thread's group; every thread gets its group's totals.
// lds: 8 * BN_THREADS floats.  The order is fixed: lane t adds lane t + s for s = 128, 64, .., GP.
__device__ __forceinline__ void bn_tree_sum(float (&v)[8], float* lds, int gp) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < 8; ++k) lds[k * BN_THREADS + tid] = v[k];
  __syncthreads();
  for (int s = BN_THREADS / 2; s >= gp; s >>= 1) {
    if (tid < s) {
#pragma unroll
      for (int k = 0; k < 8; ++k) lds[k * BN_THREADS + tid] += lds[k * BN_THREADS + tid + s];
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = lds[k * BN_THREADS + (tid & (gp - 1))];
  __syncthreads();
}

// (na, ma, qa) <- combined with (nb, mb, qb): counts, means, sums of squares about the mean
__device__ __forceinline__ void bn_chan(float& na, float (&ma)[8], float (&qa)[8], float nb, const float (&mb)[8],
                                        const float (&qb)[8]) {
  if (nb == 0.f) return;
  const float n = na + nb, f = nb / n, w = na * f;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float d = mb[k] - ma[k];
    ma[k] += d * f;
    qa[k] += qb[k] + d * d * w;
  }
  na = n;
}

__device__ __forceinline__ void bn_load8(const float* p, float (&v)[8]) {
  const float4 lo = *reinterpret_cast<const float4*>(p), hi = *reinterpret_cast<const float4*>(p + 4);
  v[0] = lo.x, v[1] = lo.y, v[2] = lo.z, v[3] = lo.w, v[4] = hi.x, v[5] = hi.y, v[6] = hi.z, v[7] = hi.w;
}

__device__ __forceinline__ void bn_store8(float* p, const float (&v)[8]) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
}

__global__ __launch_bounds__(BN_THREADS) void bn_stats_kernel(const BnArgs a) {
  __shared__ float lds[8 * BN_THREADS];
  const BnMap m = bn_map(a);
  const int gp = 1 << a.gp_log2;
  const long long r0 = (long long)blockIdx.x * a.chunk;
  const long long r1 = r0 + a.chunk < a.rows ? r0 + a.chunk : a.rows;
  const bf16* zp = a.z + (m.on ? m.c0 : 0);
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (m.on)
    for (long long r = r0 + m.rl; r < r1; r += m.R) {
      const bf16x8 v = load_bf16x8(zp + r * a.Cs);
#pragma unroll
      for (int k = 0; k < 8; ++k) s[k] += bf2f(v[k]);
    }
  bn_tree_sum(s, lds, gp);
  const float n = (float)(r1 - r0);
  float mean[8], q[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) mean[k] = s[k] / n, q[k] = 0.f;
  if (m.on)
    for (long long r = r0 + m.rl; r < r1; r += m.R) {
      const bf16x8 v = load_bf16x8(zp + r * a.Cs);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float d = bf2f(v[k]) - mean[k];
        q[k] += d * d;
      }
    }
  bn_tree_sum(q, lds, gp);
  if (m.on && m.rl == 0) {
    bn_store8(a.part + (size_t)blockIdx.x * a.Cs + m.c0, mean);
    bn_store8(a.part + ((size_t)a.nchunks + blockIdx.x) * a.Cs + m.c0, q);
  }
}

// The batch statistics of this thread's 8 channels from the chunk partials (lds: 17 * BN_THREADS floats)
__device__ __forceinline__ void bn_combine(const BnArgs& a, const BnMap& m, float* lds, float (&mean)[8],
                                           float (&var)[8]) {
  const int tid = threadIdx.x, gp = 1 << a.gp_log2;
  float n = 0.f, mu[8], q[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) mu[k] = 0.f, q[k] = 0.f;
  if (m.on)
    for (int c = m.rl; c < a.nchunks; c += m.R) {
      const long long r0 = (long long)c * a.chunk;
      const long long r1 = r0 + a.chunk < a.rows ? r0 + a.chunk : a.rows;
      float mb[8], qb[8];
      bn_load8(a.part + (size_t)c * a.Cs + m.c0, mb);
      bn_load8(a.part + ((size_t)a.nchunks + c) * a.Cs + m.c0, qb);
      bn_chan(n, mu, q, (float)(r1 - r0), mb, qb);
    }
  float* ln = lds + 16 * BN_THREADS;
  ln[tid] = n;
#pragma unroll
  for (int k = 0; k < 8; ++k) lds[k * BN_THREADS + tid] = mu[k], lds[(8 + k) * BN_THREADS + tid] = q[k];
  __syncthreads();
  for (int s = BN_THREADS / 2; s >= gp; s >>= 1) {
    if (tid < s) {
      float mb[8], qb[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) mb[k] = lds[k * BN_THREADS + tid + s], qb[k] = lds[(8 + k) * BN_THREADS + tid + s];
      bn_chan(n, mu, q, ln[tid + s], mb, qb);
      ln[tid] = n;
#pragma unroll
      for (int k = 0; k < 8; ++k) lds[k * BN_THREADS + tid] = mu[k], lds[(8 + k) * BN_THREADS + tid] = q[k];
    }
    __syncthreads();
  }
  const float rows = (float)a.rows;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    mean[k] = lds[k * BN_THREADS + m.gl];
    var[k] = lds[(8 + k) * BN_THREADS + m.gl] / rows;
  }
  __syncthreads();
}

__global__ __launch_bounds__(BN_THREADS) void bn_apply_fwd_kernel(const BnArgs a) {
  __shared__ float lds[17 * BN_THREADS];
  const BnMap m = bn_map(a);
  float mean[8], var[8], inv[8], ga[8], be[8];
  if (a.training) {
    bn_combine(a, m, lds, mean, var);
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const bool real = m.on && m.c0 + k < a.C;
      mean[k] = real ? a.moving_mean[m.c0 + k] : 0.f;
      var[k] = real ? a.moving_var[m.c0 + k] : 1.f;
    }
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const bool real = m.on && m.c0 + k < a.C;
    inv[k] = 1.f / sqrtf(var[k] + a.eps);
    ga[k] = real ? (a.gamma ? a.gamma[m.c0 + k] : 1.f) : 0.f;
    be[k] = (real && a.beta) ? a.beta[m.c0 + k] : 0.f;
  }
  if (!m.on) return;
  if (a.training && blockIdx.x == 0 && m.rl == 0) {
    bn_store8(a.saved + m.c0, mean);
    bn_store8(a.saved + a.Cs + m.c0, inv);
    const float keep = 1.f - a.momentum;
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (m.c0 + k < a.C) {
        const int c = m.c0 + k;
        a.moving_mean[c] = a.moving_mean[c] * a.momentum + mean[k] * keep;
        a.moving_var[c] = a.moving_var[c] * a.momentum + (var[k] * a.unbias) * keep;
      }
  }
  const uint32_t step = a.st ? (uint32_t)a.st->t : 0u;
  const int rows_out = a.pool ? a.B * a.Hp * a.Wp : (int)a.rows;
  for (int ro = (int)blockIdx.x * m.R + m.rl; ro < rows_out; ro += (int)gridDim.x * m.R) {
    float best[8];
    u16x8 code = {0, 0, 0, 0, 0, 0, 0, 0};
    if (a.pool) {
      const int wp = ro % a.Wp, t = ro / a.Wp, hp = t % a.Hp, b = t / a.Hp;
      const long long base = (((long long)b * a.Ho + 2 * hp) * a.Wo + 2 * wp) * a.Cs + m.c0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bf16x8 z = load_bf16x8(a.z + base + ((long long)(j >> 1) * a.Wo + (j & 1)) * a.Cs);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float u = ga[k] * ((bf2f(z[k]) - mean[k]) * inv[k]) + be[k];
          if (j == 0 || u > best[k]) best[k] = u, code[k] = (unsigned short)j;   // the FIRST maximum wins
        }
      }
    } else {
      const bf16x8 z = load_bf16x8(a.z + (long long)ro * a.Cs + m.c0);
#pragma unroll
      for (int k = 0; k < 8; ++k) best[k] = ga[k] * ((bf2f(z[k]) - mean[k]) * inv[k]) + be[k];
    }
    bf16x8 out;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      float v = best[k];
      if (a.relu) v = v > 0.f ? v : (v <= 0.f ? 0.f : v);   // (NaN stays NaN)
      const int c = m.c0 + k;
      if (a.drop_thr && c < a.C)
        v = dropout_keep((uint32_t)((long long)ro * a.C + c), a.seed, a.stream_id, step, a.drop_thr) ? v * a.drop_scale
                                                                                                      : 0.f;
      out[k] = f2bf(v);
    }
    *reinterpret_cast<bf16x8*>(a.out + (long long)ro * a.Cs + m.c0) = out;
    if (a.pool) {
      uint2 cw;
      cw.x = code[0] | (code[1] << 8) | (code[2] << 16) | ((unsigned)code[3] << 24);
      cw.y = code[4] | (code[5] << 8) | (code[6] << 16) | ((unsigned)code[7] << 24);
      *reinterpret_cast<uint2*>(a.code + (long long)ro * a.Cs + m.c0) = cw;
    }
  }
}

// du of un-pooled row r, channels [c0, c0 + 8): the pooled gradient at the window's argmax, else 0
__device__ __forceinline__ void bn_du(const BnArgs& a, long long r, int c0, float (&du)[8]) {
  if (!a.pool) {
    const bf16x8 g = load_bf16x8(a.dp + r * a.Cs + c0);
#pragma unroll
    for (int k = 0; k < 8; ++k) du[k] = bf2f(g[k]);
    return;
  }
  const int ri = (int)r;
  const int w = ri % a.Wo, t = ri / a.Wo, h = t % a.Ho, b = t / a.Ho;
  const bool in = h < 2 * a.Hp && w < 2 * a.Wp;
  // (a row or column outside every window: a clamped, discarded load keeps the loads branch-free)
  const int hp = in ? h >> 1 : 0, wp = in ? w >> 1 : 0;
  const long long po = (((long long)b * a.Hp + hp) * a.Wp + wp) * a.Cs + c0;
  const bf16x8 g = load_bf16x8(a.dp + po);
  const uint2 cw = *reinterpret_cast<const uint2*>(a.code + po);
  const unsigned pos = (unsigned)((h & 1) * 2 + (w & 1));
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const unsigned c = ((k < 4 ? cw.x : cw.y) >> (8 * (k & 3))) & 0xffu;
    du[k] = (in && c == pos) ? bf2f(g[k]) : 0.f;
  }
}

__global__ __launch_bounds__(BN_THREADS) void bn_bwd_reduce_kernel(const BnArgs a) {
  __shared__ float lds[8 * BN_THREADS];
  const BnMap m = bn_map(a);
  const int gp = 1 << a.gp_log2;
  const long long r0 = (long long)blockIdx.x * a.chunk;
  const long long r1 = r0 + a.chunk < a.rows ? r0 + a.chunk : a.rows;
  float mean[8], inv[8], sb[8], sg[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) mean[k] = 0.f, inv[k] = 0.f, sb[k] = 0.f, sg[k] = 0.f;
  if (m.on) {
    bn_load8(a.saved + m.c0, mean);
    bn_load8(a.saved + a.Cs + m.c0, inv);
    for (long long r = r0 + m.rl; r < r1; r += m.R) {
      float du[8];
      bn_du(a, r, m.c0, du);
      const bf16x8 z = load_bf16x8(a.z + r * a.Cs + m.c0);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        sb[k] += du[k];
        sg[k] += du[k] * ((bf2f(z[k]) - mean[k]) * inv[k]);
      }
    }
  }
  bn_tree_sum(sb, lds, gp);
  bn_tree_sum(sg, lds, gp);
  // the slab of this chunk: dgamma[C] then dbeta[C], packed like gamma and beta in the parameter
  // store, so that both are ONE bias-like reduction
  if (m.on && m.rl == 0) {
    float* slab = a.slab + (size_t)blockIdx.x * 2 * a.C;
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (m.c0 + k < a.C) slab[m.c0 + k] = sg[k], slab[a.C + m.c0 + k] = sb[k];
  }
}

__global__ __launch_bounds__(BN_THREADS) void bn_bwd_apply_kernel(const BnArgs a) {
  __shared__ float lds[8 * BN_THREADS];
  const BnMap m = bn_map(a);
  const int gp = 1 << a.gp_log2;
  float sb[8], sg[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) sb[k] = 0.f, sg[k] = 0.f;
  if (m.on)
    for (int c = m.rl; c < a.nchunks; c += m.R) {
      const float* slab = a.slab + (size_t)c * 2 * a.C;
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (m.c0 + k < a.C) sg[k] += slab[m.c0 + k], sb[k] += slab[a.C + m.c0 + k];
    }
  bn_tree_sum(sb, lds, gp);
  bn_tree_sum(sg, lds, gp);
  if (!m.on) return;
  float mean[8], inv[8], gi[8];
  bn_load8(a.saved + m.c0, mean);
  bn_load8(a.saved + a.Cs + m.c0, inv);
  const float rows = (float)a.rows;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const bool real = m.c0 + k < a.C;
    gi[k] = real ? (a.gamma ? a.gamma[m.c0 + k] : 1.f) * inv[k] : 0.f;
    sb[k] = sb[k] / rows;
    sg[k] = sg[k] / rows;
  }
  for (long long r = (long long)blockIdx.x * m.R + m.rl; r < a.rows; r += (long long)gridDim.x * m.R) {
    float du[8];
    bn_du(a, r, m.c0, du);
    const bf16x8 z = load_bf16x8(a.z + r * a.Cs + m.c0);
    bf16x8 out;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float xhat = (bf2f(z[k]) - mean[k]) * inv[k];
      out[k] = f2bf(gi[k] * (du[k] - sb[k] - xhat * sg[k]));
    }
    *reinterpret_cast<bf16x8*>(a.dz + r * a.Cs + m.c0) = out;
  }
}

// ---------------------------------------------------------------------------------------------
// host side
void bn_plan(long long rows, int Cs, int* chunk, int* nchunks, int* gp_log2) {
  if (rows < 1 || Cs < 8 || Cs % 8) throw std::invalid_argument("bn_plan: rows >= 1 and Cs a positive multiple of 8");
  long long ch = (rows + BN_MAX_CHUNKS - 1) / BN_MAX_CHUNKS;
  if (ch < BN_MIN_CHUNK) ch = BN_MIN_CHUNK;
  if (ch > 0x7fffffffLL) throw std::invalid_argument("bn_plan: too many rows");
  *chunk = (int)ch;
  *nchunks = (int)((rows + ch - 1) / ch);
  int lg = 0;
  while ((1 << lg) < Cs / 8 && lg < 5) ++lg;
  *gp_log2 = lg;
}

static bool bad16(const void* p) { return !p || (reinterpret_cast<uintptr_t>(p) & 15); }

// the checks the four launchers share; what: which buffers this launch touches
enum { BN_STATS = 1, BN_FWD = 2, BN_BWD_RED = 4, BN_BWD_APPLY = 8 };
static void bn_check(const BnArgs& a, const char* name, int what) {
  const std::string w(name);
  if (a.Cs <= 0 || a.Cs % 8) throw std::invalid_argument(w + ": the channel stride must be a positive multiple of 8");
  if (a.C <= 0 || a.C > a.Cs) throw std::invalid_argument(w + ": channels must be in [1, Cs]");
  if (a.rows < 1 || a.rows > 0x7fffffffLL) throw std::invalid_argument(w + ": rows must be in [1, 2^31)");
  int chunk, nchunks, lg;
  bn_plan(a.rows, a.Cs, &chunk, &nchunks, &lg);
  if (a.chunk != chunk || a.nchunks != nchunks || a.gp_log2 != lg)
    throw std::invalid_argument(w + ": chunk / nchunks / gp_log2 are not bn_plan's for these rows and Cs");
  if (bad16(a.z)) throw std::invalid_argument(w + ": z (null or not 16-byte aligned)");
  if (a.pool) {
    if (a.B < 1 || a.Ho < 2 || a.Wo < 2 || a.Hp != a.Ho / 2 || a.Wp != a.Wo / 2 ||
        (long long)a.B * a.Ho * a.Wo != a.rows)
      throw std::invalid_argument(w + ": pooled geometry (rows = B * Ho * Wo, Hp = Ho / 2, Wp = Wo / 2, Ho, Wo >= 2)");
    if ((what & (BN_FWD | BN_BWD_RED | BN_BWD_APPLY)) && (!a.code || (reinterpret_cast<uintptr_t>(a.code) & 7)))
      throw std::invalid_argument(w + ": code (null or not 8-byte aligned)");
  }
  const bool training = (what != BN_FWD) || a.training;
  if (training && bad16(a.saved)) throw std::invalid_argument(w + ": saved (null or not 16-byte aligned)");
  if ((what & BN_STATS) || ((what & BN_FWD) && a.training))
    if (bad16(a.part)) throw std::invalid_argument(w + ": part (null or not 16-byte aligned)");
  if (what & BN_FWD) {
    if (!a.moving_mean || !a.moving_var) throw std::invalid_argument(w + ": moving statistics pointers");
    if (!(a.eps > 0.f)) throw std::invalid_argument(w + ": epsilon must be > 0");
    if (!(a.momentum >= 0.f && a.momentum < 1.f)) throw std::invalid_argument(w + ": momentum must be in [0, 1)");
    if (bad16(a.out)) throw std::invalid_argument(w + ": out (null or not 16-byte aligned)");
    if (a.drop_thr && !(a.drop_scale >= 1.f && std::isfinite(a.drop_scale)))
      throw std::invalid_argument(w + ": dropout scale");
  }
  if (what & (BN_BWD_RED | BN_BWD_APPLY)) {
    if (bad16(a.dp)) throw std::invalid_argument(w + ": dp (null or not 16-byte aligned)");
    if (!a.slab || (reinterpret_cast<uintptr_t>(a.slab) & 3)) throw std::invalid_argument(w + ": slab (null or unaligned)");
  }
  if ((what & BN_BWD_APPLY) && bad16(a.dz)) throw std::invalid_argument(w + ": dz (null or not 16-byte aligned)");
}

static unsigned bn_gy(const BnArgs& a) { return (unsigned)((a.Cs / 8 + (1 << a.gp_log2) - 1) >> a.gp_log2); }

// workgroups in x of the two element-wise launches over n rows: one row per thread, four for large n
static unsigned bn_gx(const BnArgs& a, long long n) {
  const long long R = BN_THREADS >> a.gp_log2;
  const long long per = n > 65536 ? 4 * R : R;
  return (unsigned)((n + per - 1) / per);
}

void launch_bn_stats(const BnArgs& a, hipStream_t s) {
  bn_check(a, "bn_stats", BN_STATS);
  hipLaunchKernelGGL(bn_stats_kernel, dim3(a.nchunks, bn_gy(a)), dim3(BN_THREADS), 0, s, a);
}

void launch_bn_apply_fwd(const BnArgs& a, hipStream_t s) {
  bn_check(a, "bn_apply_fwd", BN_FWD);
  const long long n = a.pool ? (long long)a.B * a.Hp * a.Wp : a.rows;
  hipLaunchKernelGGL(bn_apply_fwd_kernel, dim3(bn_gx(a, n), bn_gy(a)), dim3(BN_THREADS), 0, s, a);
}

void launch_bn_bwd_reduce(const BnArgs& a, hipStream_t s) {
  bn_check(a, "bn_bwd_reduce", BN_BWD_RED);
  hipLaunchKernelGGL(bn_bwd_reduce_kernel, dim3(a.nchunks, bn_gy(a)), dim3(BN_THREADS), 0, s, a);
}

void launch_bn_bwd_apply(const BnArgs& a, hipStream_t s) {
  bn_check(a, "bn_bwd_apply", BN_BWD_APPLY);
  hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(bn_gx(a, a.rows), bn_gy(a)), dim3(BN_THREADS), 0, s, a);
}

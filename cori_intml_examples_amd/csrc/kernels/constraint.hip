// Keras-2.2.4 weight constraints (keras/constraints.py) on the flat fp32 master weights, behind the
// step's optimizer update: every constrained tensor is a row-major [R, M] matrix, a group is one column,
// and a column is rescaled by a function of its L2 norm n = sqrt(sum over the rows of w * w):
//   MaxNorm     w *= clip(n, 0, max) / (1e-7 + n)
//   NonNeg      w *= (w >= 0)
//   UnitNorm    w /= (1e-7 + n)
//   MinMaxNorm  w *= (rate * clip(n, min, max) + (1 - rate) * n) / (1e-7 + n)
// in fp32 without contraction, in exactly that operation order.  ONE descriptor table (ConArgs) holds
// all tensors of a model; a step adds constraint_apply_kernel, and constraint_norms_kernel ahead of
// it when a tensor's rows are split over workgroups -- never a launch per tensor.
//
// Work split (con_plan, from the table): the CON_THREADS threads of a workgroup form a
// [row lanes][column groups] grid, 1 << cg_log2 column groups wide -- as wide as the tensor's columns
// need, at most the whole workgroup.  A thread owns one column, or four adjacent ones as one 16-byte
// access where M % 4 == 0 and the tensor starts on a 16-byte line, and walks the rows r0 + lane,
// r0 + lane + lanes, ... of its workgroup's row chunk:
//   short and wide (a conv kernel at axis 0: R = kh, M in the thousands): 256 column groups, one row
//     lane -- a thread sums its columns' few rows in registers, no LDS traffic that matters;
//   tall and narrow (a dense kernel, 4096 x 128): 32 column groups x 8 row lanes, the rows cut into
//     chunks of max(CON_MIN_CHUNK_ROWS, ceil(R / CON_MAX_CHUNKS)) rows, one workgroup per chunk;
//   M = 1 (a bias): one column group, 256 row lanes -- one whole-vector norm.
// The sum of a column is fixed-order throughout: a thread adds its rows in ascending order, the row
// lanes' partial sums meet in LDS and are added in ascending lane order, and the chunks of a split
// tensor are added in ascending chunk order from the partials buffer (one word per (chunk, column),
// written by the norms launch, read by the apply launch: the launch boundary is the only
// synchronisation).  No atomics, so two runs from the same state give the same bits.
//
// The apply launch writes every rescaled weight's bf16 copies into the fragment packs through the
// optimizer's pack routes (con_pack: pack_write's addresses, optim_math.h) -- the update wrote the unconstrained value there --
// or, without routes, marks the packs stale for the next prologue, as the optimizer launches do.
// Elements outside the tensors are neither read nor written.
#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>

#include "args.h"
#include "optim_math.h"

#define CON_EPS 1e-7f                    // K.epsilon()

// NaN stays NaN (K.clip), unlike fminf / fmaxf
__device__ __forceinline__ float con_clip(float n, float lo, float hi) { return n < lo ? lo : (n > hi ? hi : n); }

// one element of a column of norm n; den = 1e-7 + n and f = numerator / den are formed once per column
__device__ __forceinline__ void con_column(const ConDesc& d, float sumsq, float& f, float& den) {
#pragma clang fp contract(off)
  const float n = sqrtf(sumsq);
  den = CON_EPS + n;
  float num = con_clip(n, 0.f, d.p1);                              // CON_MAX_NORM
  if (d.kind == CON_MIN_MAX_NORM) num = d.p2 * con_clip(n, d.p0, d.p1) + (1.f - d.p2) * n;
  f = num / den;
}
__device__ __forceinline__ float con_elem(int kind, float w, float f, float den) {
#pragma clang fp contract(off)
  if (kind == CON_NON_NEG) return w * (w >= 0.f ? 1.f : 0.f);
  if (kind == CON_UNIT_NORM) return w / den;
  return w * f;
}

// the descriptor and the (chunk, tile) of a workgroup: NORMS picks the norms launch's numbering
template <bool NORMS>
__device__ __forceinline__ int con_find(const ConArgs& a, int blk, int& chunk, int& tile) {
  int di = 0, b0 = 0;
  for (int i = 0; i < a.ndesc; ++i) {                              // workgroup-uniform
    const int s = NORMS ? a.d[i].nb0 : a.d[i].b0;
    if (s >= 0 && blk >= s) { di = i; b0 = s; }
  }
  const int local = blk - b0, nt = a.d[di].ntile;
  chunk = local / nt;
  tile = local - chunk * nt;
  return di;
}

// The row lanes' sums of squares of this workgroup's columns over the rows [r0, r1), combined in LDS:
// tot[c] for the tile's columns c in [0, (1 << cg_log2) * V).  sh: CON_THREADS * V words.
template <int V>
__device__ __forceinline__ void con_tile_sums(const float* __restrict__ w, const ConDesc& d, int r0, int r1, int col,
                                              bool active, float* sh, float* tot) {
#pragma clang fp contract(off)
  const int CG = 1 << d.cg_log2, RL = CON_THREADS >> d.cg_log2, CGV = CG * V;
  const int cg = threadIdx.x & (CG - 1), rl = threadIdx.x >> d.cg_log2;
  float acc[V];
#pragma unroll
  for (int u = 0; u < V; ++u) acc[u] = 0.f;
  if (active) {
#pragma unroll 4
    for (int r = r0 + rl; r < r1; r += RL) {
      const float* src = w + (long long)r * d.M + col;
      if constexpr (V == 4) {
        const float4 x = *reinterpret_cast<const float4*>(src);
        acc[0] += x.x * x.x;
        acc[1] += x.y * x.y;
        acc[2] += x.z * x.z;
        acc[3] += x.w * x.w;
      } else {
        const float x = *src;
        acc[0] += x * x;
      }
    }
  }
#pragma unroll
  for (int u = 0; u < V; ++u) sh[rl * CGV + cg * V + u] = acc[u];
  __syncthreads();
  for (int c = threadIdx.x; c < CGV; c += CON_THREADS) {
    float s = 0.f;
    for (int l = 0; l < RL; ++l) s += sh[l * CGV + c];             // ascending lane order
    tot[c] = s;
  }
  __syncthreads();
}

// a workgroup's place in its tensor
struct ConPlace {
  int r0, r1, col, cg, rl, tcol0;
  bool active;
};
template <int V>
__device__ __forceinline__ ConPlace con_place(const ConDesc& d, int chunk, int tile) {
  ConPlace p;
  const int CG = 1 << d.cg_log2;
  p.cg = threadIdx.x & (CG - 1);
  p.rl = threadIdx.x >> d.cg_log2;
  p.r0 = chunk * d.rchunk;
  p.r1 = min(p.r0 + d.rchunk, d.R);
  p.tcol0 = tile * CG * V;
  p.col = p.tcol0 + p.cg * V;
  p.active = p.col < d.M;                                          // (V == 4: M % 4 == 0, all four or none)
  return p;
}

template <int V>
__device__ __forceinline__ void con_norms_body(const ConArgs& a, const ConDesc& d, int chunk, int tile, float* sh,
                                               float* tot) {
  const ConPlace p = con_place<V>(d, chunk, tile);
  con_tile_sums<V>(a.p + d.off, d, p.r0, p.r1, p.col, p.active, sh, tot);
  const int CGV = (1 << d.cg_log2) * V;
  float* dst = a.partials + d.part0 + (long long)chunk * d.M;
  for (int c = threadIdx.x; c < CGV; c += CON_THREADS)
    if (p.tcol0 + c < d.M) dst[p.tcol0 + c] = tot[c];
}

__global__ __launch_bounds__(CON_THREADS) void constraint_norms_kernel(const ConArgs a) {
  __shared__ __attribute__((aligned(16))) float sh[CON_THREADS * 4];
  __shared__ __attribute__((aligned(16))) float tot[CON_THREADS * 4];
  int chunk, tile;
  const ConDesc& d = a.d[con_find<true>(a, blockIdx.x, chunk, tile)];
  if (d.vec) con_norms_body<4>(a, d, chunk, tile, sh, tot);
  else con_norms_body<1>(a, d, chunk, tile, sh, tot);
}

#define CON_ROWS_IN_FLIGHT 4

// The bf16 copies of the V consecutive elements [e, e + V) of route R with their new values v: the
// coordinates and stores of pack_write / pack_write4 (optim_math.h) for one known route.
template <int V>
__device__ __forceinline__ void con_pack(const PackRoute& R, bf16* arena, int e, const float (&v)[V]) {
  int kf, kb, nb;
  if (V == 4 && e >= R.lo && e + 4 <= R.hi && !((R.Cout | (e - R.lo)) & 3)) {   // one row run: see pack_write4
    const int le = e - R.lo, o = le / R.Cout, c = le - o * R.Cout;
    route_coords(R, o, kf, kb, nb);
    if (R.fwd >= 0) {
      bf16* dst = arena + R.fwd + frag_off(kf, c, R.NT);
      dst[0] = f2bf(v[0]);
      dst[8] = f2bf(v[1]);
      dst[16] = f2bf(v[2]);
      dst[24] = f2bf(v[3]);
    }
    if (R.bwd >= 0) {
      bf16x4 q;
      q[0] = f2bf(v[0]); q[1] = f2bf(v[1]); q[2] = f2bf(v[2]); q[3] = f2bf(v[3]);
      *reinterpret_cast<bf16x4*>(arena + R.bwd + frag_off(kb + c, nb, R.NTb)) = q;
    }
    return;
  }
#pragma unroll
  for (int u = 0; u < V; ++u) {
    const int eu = e + u;
    if (eu < R.lo || eu >= R.hi) continue;
    const int le = eu - R.lo, o = le / R.Cout, c = le - o * R.Cout;
    route_coords(R, o, kf, kb, nb);
    const bf16 b = f2bf(v[u]);
    if (R.fwd >= 0) arena[R.fwd + frag_off(kf, c, R.NT)] = b;
    if (R.bwd >= 0) arena[R.bwd + frag_off(kb + c, nb, R.NTb)] = b;
  }
}

template <int V>
__device__ __forceinline__ void con_apply_body(const ConArgs& a, const ConDesc& d, int chunk, int tile, float* sh,
                                               float* tot) {
  const ConPlace p = con_place<V>(d, chunk, tile);
  const int RL = CON_THREADS >> d.cg_log2, CGV = (1 << d.cg_log2) * V;
  float* w = a.p + d.off;
  float f[V], den[V];
#pragma unroll
  for (int u = 0; u < V; ++u) f[u] = den[u] = 0.f;
  if (d.kind != CON_NON_NEG) {
    if (d.part0 >= 0) {
      // a split tensor: the chunks of each of the tile's columns in ascending chunk order
      for (int c = threadIdx.x; c < CGV; c += CON_THREADS) {
        float s = 0.f;
        if (p.tcol0 + c < d.M)
          for (int k = 0; k < d.nchunk; ++k) {
#pragma clang fp contract(off)
            s += a.partials[d.part0 + (long long)k * d.M + p.tcol0 + c];
          }
        tot[c] = s;
      }
      __syncthreads();
    } else {
      con_tile_sums<V>(w, d, 0, d.R, p.col, p.active, sh, tot);
    }
#pragma unroll
    for (int u = 0; u < V; ++u) con_column(d, tot[p.cg * V + u], f[u], den[u]);
  }
  if (!p.active) return;
  // the tensor's pack route, read once (a route covers one whole packed tensor; a bias or an unpacked
  // stage's kernel has none)
  PackRoute R = {};
  bool routed = false;
  for (int i = 0; i < a.nroutes; ++i)                                // workgroup-uniform
    if (d.off >= a.routes[i].lo && d.off < a.routes[i].hi) {
      R = a.routes[i];
      routed = true;
    }
  // CON_ROWS_IN_FLIGHT rows are loaded before the first of them is stored: the loads of a thread's rows
  // do not wait behind its own stores
  for (int rb = p.r0 + p.rl; rb < p.r1; rb += RL * CON_ROWS_IN_FLIGHT) {
    float x[CON_ROWS_IN_FLIGHT][V];
#pragma unroll
    for (int i = 0; i < CON_ROWS_IN_FLIGHT; ++i) {
      const int r = rb + i * RL;
      if (r >= p.r1) continue;
      const float* src = w + (long long)r * d.M + p.col;
      if constexpr (V == 4) {
        const float4 v = *reinterpret_cast<const float4*>(src);
        x[i][0] = v.x; x[i][1] = v.y; x[i][2] = v.z; x[i][3] = v.w;
      } else {
        x[i][0] = *src;
      }
    }
#pragma unroll
    for (int i = 0; i < CON_ROWS_IN_FLIGHT; ++i) {
      const int r = rb + i * RL;
      if (r >= p.r1) continue;
      const long long le = (long long)r * d.M + p.col;
#pragma unroll
      for (int u = 0; u < V; ++u) x[i][u] = con_elem(d.kind, x[i][u], f[u], den[u]);
      if constexpr (V == 4) *reinterpret_cast<float4*>(w + le) = float4{x[i][0], x[i][1], x[i][2], x[i][3]};
      else w[le] = x[i][0];
      if (routed) con_pack<V>(R, a.arena, d.off + (int)le, x[i]);
    }
  }
}

__global__ __launch_bounds__(CON_THREADS) void constraint_apply_kernel(const ConArgs a) {
  __shared__ __attribute__((aligned(16))) float sh[CON_THREADS * 4];
  __shared__ __attribute__((aligned(16))) float tot[CON_THREADS * 4];
  if (!a.nroutes && a.st && blockIdx.x == 0 && threadIdx.x == 0) a.st->packs_stale = 1;
  int chunk, tile;
  const ConDesc& d = a.d[con_find<false>(a, blockIdx.x, chunk, tile)];
  if (d.vec) con_apply_body<4>(a, d, chunk, tile, sh, tot);
  else con_apply_body<1>(a, d, chunk, tile, sh, tot);
}

void con_set_tensors(ConArgs& a, const int* off, const int* R, const int* M, const int* kind, const float* p0,
                     const float* p1, const float* p2, int count) {
  if (count > MAX_CON)
    throw std::invalid_argument("constraint: " + std::to_string(count) + " constrained tensors, the kernel takes at most "
                                "MAX_CON = " + std::to_string(MAX_CON));
  long long prev = 0;
  for (int i = 0; i < count; ++i) {
    if (R[i] <= 0 || M[i] <= 0 || off[i] < prev || (long long)off[i] + (long long)R[i] * M[i] > 0x7fffffffLL)
      throw std::invalid_argument("constraint: tensors must be non-empty, ascending and disjoint");
    if (kind[i] < CON_MAX_NORM || kind[i] > CON_MIN_MAX_NORM) throw std::invalid_argument("constraint: kind");
    a.d[i] = ConDesc{off[i], R[i], M[i], kind[i], p0[i], p1[i], p2[i], 0, 0, 0, 0, 0, -1, -1, -1};
    prev = (long long)off[i] + (long long)R[i] * M[i];
  }
  a.ndesc = count;
}

// Every descriptor's work split for a's weight pointer (its alignment decides the float4 path), the two
// launches' workgroup numbering and the partials' layout; returns the partials words needed.
int con_plan(ConArgs& a) {
  int nb = 0, ab = 0, words = 0;
  for (int i = 0; i < a.ndesc; ++i) {
    ConDesc& d = a.d[i];
    d.vec = d.M % 4 == 0 && (((reinterpret_cast<uintptr_t>(a.p) >> 2) + (uintptr_t)d.off) & 3) == 0;
    const int V = d.vec ? 4 : 1, groups = (d.M + V - 1) / V;
    d.cg_log2 = 0;
    while ((1 << d.cg_log2) < groups && d.cg_log2 < 8) ++d.cg_log2;
    d.rchunk = std::max(CON_MIN_CHUNK_ROWS, (d.R + CON_MAX_CHUNKS - 1) / CON_MAX_CHUNKS);
    d.nchunk = (d.R + d.rchunk - 1) / d.rchunk;
    d.ntile = (groups + (1 << d.cg_log2) - 1) >> d.cg_log2;
    d.b0 = ab;
    ab += d.nchunk * d.ntile;
    d.nb0 = d.part0 = -1;
    if (d.kind != CON_NON_NEG && d.nchunk > 1) {
      d.nb0 = nb;
      nb += d.nchunk * d.ntile;
      d.part0 = words;
      words += d.nchunk * d.M;
    }
  }
  a.norm_blocks = nb;
  a.apply_blocks = ab;
  return words;
}

static ConArgs con_checked(const ConArgs& in) {
  ConArgs a = in;
  if (!a.p || (reinterpret_cast<uintptr_t>(a.p) & 3) || a.ndesc <= 0 || a.ndesc > MAX_CON)
    throw std::invalid_argument("constraint: weight pointer / no constrained tensor (a model without constraints "
                                "launches nothing)");
  for (int i = 0; i < a.ndesc; ++i) {
    const ConDesc& d = a.d[i];
    const long long hi = (long long)d.off + (long long)d.R * d.M;
    if (d.off < 0 || d.R <= 0 || d.M <= 0 || hi > a.n || (i && d.off < a.d[i - 1].off + a.d[i - 1].R * a.d[i - 1].M))
      throw std::invalid_argument("constraint: tensors must be ascending, disjoint and inside [0, n)");
  }
  const int words = con_plan(a);
  if (words > 0 && (!a.partials || a.npartials < words))
    throw std::invalid_argument("constraint: partials buffer too small");
  if (a.nroutes < 0 || a.nroutes > MAX_ROUTES || (a.nroutes && (!a.routes || !a.arena)))
    throw std::invalid_argument("constraint: pack routes");
  return a;
}

// the norms launch of the tensors whose rows are split over workgroups (nothing without one)
void launch_constraint_norms(const ConArgs& in, hipStream_t s) {
  const ConArgs a = con_checked(in);
  if (a.norm_blocks > 0)
    hipLaunchKernelGGL(constraint_norms_kernel, dim3(a.norm_blocks), dim3(CON_THREADS), 0, s, a);
}

void launch_constraint_apply(const ConArgs& in, hipStream_t s) {
  const ConArgs a = con_checked(in);
  hipLaunchKernelGGL(constraint_apply_kernel, dim3(a.apply_blocks), dim3(CON_THREADS), 0, s, a);
}

// Keras-2.2 L1 / L2 weight regularizers (keras/regularizers.py L1L2) on the flat master weights
// and the flat reduced gradient, ONE launch per step.
//
// weight_reg_kernel: for every element w of a regularized range {lo, hi, l1, l2x2, l2}
//   g = g + (l1 * sgn(w) + l2x2 * w)          (sgn(0) = 0; stored only when add_grad)
//   P += l1 * |w| + l2 * (w * w)
// in fp32 without contraction, in exactly that operation order.  Elements outside every range
// are neither read into the sum nor written.
//
// The sum is bit-reproducible, built like grad_sqnorm_kernel's (clip.hip): workgroup b takes one
// fixed chunk of REG_CHUNK elements of the 16-byte-aligned view of the buffers (the launch covers
// only the chunks that touch a range: reg_plan), every thread its REG_VEC_PER_THREAD groups of
// four in a fixed order, a fixed cross-lane / LDS tree, a partial per workgroup, a ticket drawn
// with a device-scope atomic.  The workgroup that draws the last ticket re-reads ALL partials and
// sums them in an order that depends on their index only, writes P, adds P * rows to the step's
// loss words (the head's 64-bit fixed point) and zeroes the ticket for the next launch / graph
// replay.  No workgroup waits for another one: no spin, no grid barrier.
//
// A group of four is loaded and stored as one float4 where it lies inside ONE range (and with it
// inside the aligned view); groups on a range border -- a bias follows its kernel at an arbitrary
// element -- take 4-byte accesses of the elements inside a range.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>

#include "args.h"

// fixed-order sum over the workgroup's 256 threads: xor butterfly inside each wave (every lane
// ends with the same bits), then the four wave sums in wave order; sh[0..3] is scratch
__device__ __forceinline__ float reg_block_sum(float v, float* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int wave = threadIdx.x >> 6;
  __syncthreads();                       // (sh may still be read from an earlier call)
  if ((threadIdx.x & 63) == 0) sh[wave] = v;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// one element: the gradient with the regularizer's term, and the element's penalty term
__device__ __forceinline__ float reg_grad(float g, float w, float l1, float l2x2) {
#pragma clang fp contract(off)
  const float sg = (w > 0.f ? 1.f : 0.f) - (w < 0.f ? 1.f : 0.f);
  return g + (l1 * sg + l2x2 * w);
}
__device__ __forceinline__ float reg_term(float w, float l1, float l2) {
#pragma clang fp contract(off)
  return l1 * fabsf(w) + l2 * (w * w);
}

__global__ __launch_bounds__(REG_THREADS) void weight_reg_kernel(const RegArgs a) {
#pragma clang fp contract(off)
  __shared__ float sh[8];                // [0..3] wave sums, [4] "this workgroup drew the last ticket"
  // the 16-byte-aligned view: element i of the view is p[i - mis] (g shares the offset: host check)
  const int mis = (int)((reinterpret_cast<uintptr_t>(a.p) >> 2) & 3);
  const float* pb = a.p - mis;
  float* gb = a.g - mis;
  // this workgroup's chunk (the launch skips the chunks no range touches)
  int chunk = 0;
  for (int s = 0; s < a.nseg; ++s)
    if ((int)blockIdx.x >= a.seg_b0[s]) chunk = a.seg_c0[s] + ((int)blockIdx.x - a.seg_b0[s]);
  const long long c0 = (long long)chunk * REG_CHUNK, c1 = c0 + REG_CHUNK;
  // the ranges that touch it (workgroup-uniform)
  unsigned touch = 0;
  for (int r = 0; r < a.nranges; ++r)
    if ((long long)a.r[r].lo + mis < c1 && (long long)a.r[r].hi + mis > c0) touch |= 1u << r;
  const bool add = a.add_grad != 0;
  float t[REG_VEC_PER_THREAD][4];
#pragma unroll
  for (int i = 0; i < REG_VEC_PER_THREAD; ++i) t[i][0] = t[i][1] = t[i][2] = t[i][3] = 0.f;
  for (unsigned m = touch; m; m &= m - 1) {
    const int r = __ffs(m) - 1;
    const long long lo = (long long)a.r[r].lo + mis, hi = (long long)a.r[r].hi + mis;
    const float l1 = a.r[r].l1, l2x2 = a.r[r].l2x2, l2 = a.r[r].l2;
#pragma unroll
    for (int i = 0; i < REG_VEC_PER_THREAD; ++i) {
      const long long e = c0 + ((long long)i * REG_THREADS + threadIdx.x) * 4;
      if (e >= lo && e + 4 <= hi) {
        const float4 w = *reinterpret_cast<const float4*>(pb + e);
        if (add) {
          float4 g = *reinterpret_cast<const float4*>(gb + e);
          g.x = reg_grad(g.x, w.x, l1, l2x2);
          g.y = reg_grad(g.y, w.y, l1, l2x2);
          g.z = reg_grad(g.z, w.z, l1, l2x2);
          g.w = reg_grad(g.w, w.w, l1, l2x2);
          *reinterpret_cast<float4*>(gb + e) = g;
        }
        t[i][0] = reg_term(w.x, l1, l2);
        t[i][1] = reg_term(w.y, l1, l2);
        t[i][2] = reg_term(w.z, l1, l2);
        t[i][3] = reg_term(w.w, l1, l2);
      } else if (e + 4 > lo && e < hi) {   // a border group: 4-byte accesses of the elements inside
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (e + u >= lo && e + u < hi) {
            const float w = pb[e + u];
            if (add) gb[e + u] = reg_grad(gb[e + u], w, l1, l2x2);
            t[i][u] = reg_term(w, l1, l2);
          }
      }
    }
  }
  float acc = 0.f;
#pragma unroll
  for (int i = 0; i < REG_VEC_PER_THREAD; ++i) acc += (t[i][0] + t[i][1]) + (t[i][2] + t[i][3]);
  const float part = reg_block_sum(acc, sh);
  unsigned* ticket = reinterpret_cast<unsigned*>(a.state + REG_TICKET);
  if (threadIdx.x == 0) {
    // publish the partial (write-through store, agent-scope release, drained) before the ticket;
    // the explicit waits repeat the fences' own and keep the order in the source (see clip.hip)
    __hip_atomic_store(a.partials + blockIdx.x, part, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned tk = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool last = tk == gridDim.x - 1;
    if (last) {                          // acquire: drop this CU's stale lines of the partials
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    sh[4] = last ? 1.f : 0.f;
  }
  __syncthreads();
  if (sh[4] == 0.f) return;
  float s = 0.f;
  for (int k = threadIdx.x; k < (int)gridDim.x; k += REG_THREADS)
    s += __hip_atomic_load(a.partials + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const float total = reg_block_sum(s, sh);
  if (threadIdx.x == 0) {
    a.state[REG_PENALTY] = total;
    if (a.st) {
      // the batch's loss words take rows * P (the epoch loss is sum_b(M_b * loss_b) / N), in the
      // head's fixed point and with its overflow rule: the spare word makes the host report NaN
      long long* slot = a.st->metric_slots[0];
      const double v = (double)total * a.rows;
      if (isfinite(v) && v < 1073741824.0)
        atomicAdd((unsigned long long*)&slot[0], (unsigned long long)llrint(v * 4294967296.0));
      else
        atomicAdd((unsigned long long*)&slot[3], 1ull);
    }
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// Fills a's chunk segments for its pointers' alignment; returns the workgroups (= partials) of
// the launch.  Chunks of the aligned view that no range touches get no workgroup.
int reg_plan(RegArgs& a) {
  const long long mis = (long long)((reinterpret_cast<uintptr_t>(a.p) >> 2) & 3);
  a.nseg = 0;
  int blocks = 0;
  long long next = -1;                   // the first chunk not yet covered
  for (int r = 0; r < a.nranges; ++r) {
    if (a.r[r].hi <= a.r[r].lo) continue;
    long long f = (a.r[r].lo + mis) / REG_CHUNK;
    const long long l = (a.r[r].hi + mis - 1) / REG_CHUNK;
    f = std::max(f, next);
    if (f > l) continue;
    if (a.nseg && f == next) {           // continues the previous segment
      blocks += (int)(l - f + 1);
    } else {
      a.seg_b0[a.nseg] = blocks;
      a.seg_c0[a.nseg] = (int)f;
      ++a.nseg;
      blocks += (int)(l - f + 1);
    }
    next = l + 1;
    a.seg_b0[a.nseg] = blocks;
  }
  return blocks;
}

int reg_blocks(const RegArgs& a) {
  RegArgs b = a;
  return reg_plan(b);
}

void reg_set_ranges(RegArgs& a, const int* lo, const int* hi, const float* l1, const float* l2, int count) {
  if (count > MAX_REG_RANGES)
    throw std::invalid_argument("weight_reg: " + std::to_string(count) + " regularized ranges, the kernel takes at most "
                                "MAX_REG_RANGES = " + std::to_string(MAX_REG_RANGES));
  int prev = 0;
  for (int i = 0; i < count; ++i) {
    if (lo[i] < prev || hi[i] < lo[i])
      throw std::invalid_argument("weight_reg: ranges must be ascending and disjoint");
    if (!(l1[i] >= 0.f) || !(l2[i] >= 0.f) || !std::isfinite(l1[i]) || !std::isfinite(l2[i]) || !std::isfinite(2.f * l2[i]))
      throw std::invalid_argument("weight_reg: coefficients must be finite and >= 0");
    a.r[i] = RegRange{lo[i], hi[i], l1[i], 2.f * l2[i], l2[i]};
    prev = hi[i];
  }
  a.nranges = count;
}

void launch_weight_reg(const RegArgs& in, hipStream_t s) {
  RegArgs a = in;
  const uintptr_t pp = reinterpret_cast<uintptr_t>(a.p), gp = reinterpret_cast<uintptr_t>(a.g);
  if (!a.p || !a.state || a.n < 0 || (pp & 3) || (reinterpret_cast<uintptr_t>(a.state) & 15))
    throw std::invalid_argument("weight_reg: weight / reg state pointers");
  if (a.add_grad && (!a.g || (gp & 3) || ((gp >> 2) & 3) != ((pp >> 2) & 3)))
    throw std::invalid_argument("weight_reg: the gradient must share the weights' offset in a 16-byte line");
  if (a.nranges < 0 || a.nranges > MAX_REG_RANGES) throw std::invalid_argument("weight_reg: range count");
  for (int r = 0; r < a.nranges; ++r)
    if (a.r[r].lo < 0 || a.r[r].hi > a.n || a.r[r].hi < a.r[r].lo || (r && a.r[r].lo < a.r[r - 1].hi))
      throw std::invalid_argument("weight_reg: ranges must be ascending, disjoint and inside [0, n)");
  if (!a.add_grad) a.g = const_cast<float*>(a.p);      // (never dereferenced: add_grad = 0)
  const int blocks = reg_plan(a);
  if (blocks == 0) throw std::invalid_argument("weight_reg: no regularized element (a model without regularizers "
                                               "launches nothing)");
  if (!a.partials || a.npartials < blocks) throw std::invalid_argument("weight_reg: partials buffer too small");
  hipLaunchKernelGGL(weight_reg_kernel, dim3(blocks), dim3(REG_THREADS), 0, s, a);
}

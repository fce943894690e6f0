// Keras-2.2 gradient clipping (Optimizer.get_gradients: clipnorm over the GLOBAL norm of every
// trainable parameter's gradient, then clipvalue) on the flat reduced gradient.
//
// grad_sqnorm_kernel: sum of squares of g[0, n) in ONE launch, bit-reproducible.  Workgroup b
// sums the fixed contiguous chunk [b * CLIP_CHUNK, (b + 1) * CLIP_CHUNK) of the 16-byte-aligned
// view of the buffer (fixed per-thread order, fixed cross-lane / LDS tree), stores its partial
// and draws a ticket with a device-scope atomic.  The workgroup that draws the last ticket
// re-reads ALL partials and sums them in an order that depends on their index only (thread t:
// partials t, t + 256, ... ascending; then the same tree), so the result does not depend on
// which workgroup came last; it writes the norm and the clip factor and zeroes the ticket for
// the next launch / graph replay.  No workgroup waits for another one: no spin, no grid barrier.
//
// grad_clip_apply_kernel: g = clip_elem(g) in place (the data-parallel step clips the local
// gradient in memory ahead of the all-reduce); the single-GPU step applies the same element
// function on the fly inside the optimizer launch (optim_clip_kernel, misc.hip).
#include <algorithm>
#include <cstdint>

#include "optim_math.h"

// fixed-order sum over the workgroup's 256 threads: xor butterfly inside each wave (every lane
// ends with the same bits), then the four wave sums in wave order; sh[0..3] is scratch
__device__ __forceinline__ float clip_block_sum(float v, float* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int wave = threadIdx.x >> 6;
  __syncthreads();                       // (sh may still be read from an earlier call)
  if ((threadIdx.x & 63) == 0) sh[wave] = v;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

__global__ __launch_bounds__(CLIP_THREADS) void grad_sqnorm_kernel(const ClipArgs a) {
  __shared__ float sh[8];                // [0..3] wave sums, [4] "this workgroup drew the last ticket"
  // the 16-byte-aligned view: element i of the view is g[i - mis]; the range is [mis, mis + n)
  const int mis = (int)((reinterpret_cast<uintptr_t>(a.g) >> 2) & 3);
  const float* gb = a.g - mis;
  const long long lo = mis, hi = (long long)mis + a.n;
  const long long c0 = (long long)blockIdx.x * CLIP_CHUNK;
  float acc = 0.f;
#pragma unroll
  for (int i = 0; i < CLIP_VEC_PER_THREAD; ++i) {
    const long long e = c0 + ((long long)i * CLIP_THREADS + threadIdx.x) * 4;
    float x = 0.f, y = 0.f, z = 0.f, w = 0.f;
    if (e >= lo && e + 4 <= hi) {
      const float4 v = *reinterpret_cast<const float4*>(gb + e);
      x = v.x; y = v.y; z = v.z; w = v.w;
    } else if (e + 4 > lo && e < hi) {   // a boundary group: 4-byte loads of the elements inside
      if (e >= lo) x = gb[e];
      if (e + 1 >= lo && e + 1 < hi) y = gb[e + 1];
      if (e + 2 >= lo && e + 2 < hi) z = gb[e + 2];
      if (e + 3 < hi) w = gb[e + 3];
    }
    acc += (x * x + y * y) + (z * z + w * w);
  }
  const float part = clip_block_sum(acc, sh);
  unsigned* ticket = reinterpret_cast<unsigned*>(a.state + CLIP_TICKET);
  if (threadIdx.x == 0) {
    // publish the partial (write-through store, agent-scope release, drained) before the ticket.
    // The explicit waits behind the fences repeat the fences' own (the compiler emits both today):
    // they cost nothing and keep the order "partial drained, then ticket" / "invalidate done, then
    // barrier" in the source, whatever wait a compiler version attaches to the fence itself
    __hip_atomic_store(a.partials + blockIdx.x, part, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool last = t == gridDim.x - 1;
    if (last) {                          // acquire: drop this CU's stale lines of the partials
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    sh[4] = last ? 1.f : 0.f;
  }
  __syncthreads();
  if (sh[4] == 0.f) return;
  float s = 0.f;
  for (int k = threadIdx.x; k < (int)gridDim.x; k += CLIP_THREADS) s += a.partials[k];
  const float total = clip_block_sum(s, sh);
  if (threadIdx.x == 0) {
    const float norm = sqrtf(total);
    // (a zero norm and a NaN norm both fail the comparison: no division, factor 1)
    const float factor = (a.clipnorm > 0.f && norm >= a.clipnorm) ? a.clipnorm / norm : 1.f;
    a.state[CLIP_NORM] = norm;
    a.state[CLIP_FACTOR] = factor;
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ __launch_bounds__(CLIP_THREADS) void grad_clip_apply_kernel(const ClipArgs a) {
  const int mis = (int)((reinterpret_cast<uintptr_t>(a.g) >> 2) & 3);
  float* gb = a.g - mis;
  const long long lo = mis, hi = (long long)mis + a.n;
  const long long e = ((long long)blockIdx.x * CLIP_THREADS + threadIdx.x) * 4;
  if (e >= hi) return;
  const float f = a.use_norm ? a.state[CLIP_FACTOR] : 1.f;
  const float v = a.clipvalue;
  if (e >= lo && e + 4 <= hi) {
    float4 g = *reinterpret_cast<const float4*>(gb + e);
    g.x = clip_elem(g.x, f, v);
    g.y = clip_elem(g.y, f, v);
    g.z = clip_elem(g.z, f, v);
    g.w = clip_elem(g.w, f, v);
    *reinterpret_cast<float4*>(gb + e) = g;
  } else {
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (e + u >= lo && e + u < hi) gb[e + u] = clip_elem(gb[e + u], f, v);
  }
}

int clip_blocks(const ClipArgs& a) {     // workgroups (= partials) of grad_sqnorm for this range
  const long long span = (long long)((reinterpret_cast<uintptr_t>(a.g) >> 2) & 3) + a.n;
  return (int)std::max<long long>(1, (span + CLIP_CHUNK - 1) / CLIP_CHUNK);
}

static void check_clip(const ClipArgs& a, const char* what) {
  if (!a.g || a.n < 0 || !a.state || (reinterpret_cast<uintptr_t>(a.g) & 3) || (reinterpret_cast<uintptr_t>(a.state) & 15))
    throw std::invalid_argument(std::string(what) + ": gradient / clip state pointers");
}

void launch_grad_sqnorm(const ClipArgs& a, hipStream_t s) {
  check_clip(a, "grad_sqnorm");
  const int blocks = clip_blocks(a);
  if (!a.partials || a.npartials < blocks) throw std::invalid_argument("grad_sqnorm: partials buffer too small");
  hipLaunchKernelGGL(grad_sqnorm_kernel, dim3(blocks), dim3(CLIP_THREADS), 0, s, a);
}

void launch_grad_clip_apply(const ClipArgs& a, hipStream_t s) {
  check_clip(a, "grad_clip_apply");
  if (a.n == 0 || (!a.use_norm && !(a.clipvalue > 0.f))) return;
  const long long span = (long long)((reinterpret_cast<uintptr_t>(a.g) >> 2) & 3) + a.n;
  const long long blocks = ((span + 3) / 4 + CLIP_THREADS - 1) / CLIP_THREADS;
  hipLaunchKernelGGL(grad_clip_apply_kernel, dim3((unsigned)blocks), dim3(CLIP_THREADS), 0, s, a);
}

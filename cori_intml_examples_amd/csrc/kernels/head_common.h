// What the two output-head kernels share (head.hip: the three classic (activation, loss) pairs,
// also absorbing the last dense layer's epilogue; loss_head.hip: every other pair of the loss
// table): the staging of targets / bias / sample weights, the logit dot products, the metric
// atomics, the dW / db partial slabs and the dh back-projection.
#pragma once
#include "bwd_through.h"

// Keras' probability clip (tf.clip_by_value) propagates a NaN; fminf/fmaxf would replace it
// by a bound and turn a diverged model's loss into a finite value
__device__ __forceinline__ float clip_nan(float q, float lo, float hi) {
  return q != q ? q : fminf(fmaxf(q, lo), hi);
}

#define HEAD_RB 4
#define HEAD_W_LDS 2048     // head weights staged in LDS up to this many floats

// 16-lane group reductions (lanes 0..15 of a wave; xor offsets < 16 stay inside the group)
__device__ __forceinline__ float grp16_sum(float v) {
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
// max value and its lowest index (the serial loop's strict '>' keeps the first maximum)
__device__ __forceinline__ void grp16_argmax(float& v, int& i) {
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) {
    const float ov = __shfl_xor(v, off);
    const int oi = __shfl_xor(i, off);
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
  }
}

// The code blocks below are macros, not functions: head_kernel's instances are pinned at the code
// they compiled to before loss_head.hip existed (the launch that gates the RPV backward), and as
// force-inlined functions the same statements were scheduled and allocated differently.  They name
// the kernels' locals (a, tid, lane, row, row0, N, NM, wlds, wsh, ysh, bsh, dz_s, rows_here, step).

// The bias (threads 0..15) and the workgroup's RB_ target rows (threads 64..64 + 16 RB_) -> LDS
// (prologue-free step: the targets' dataset row, recorded by the conv stack)
#define HEAD_STAGE_TARGETS(RB_)                                                                              \
  if (tid < 16) bsh[tid] = (a.bias && tid < a.N) ? a.bias[tid] : 0.f;                                        \
  if (tid >= 64 && tid < 64 + RB_ * 16) {                                                                    \
    const int rl = (tid - 64) >> 4, n = (tid - 64) & 15;                                                     \
    const int m = row0 + rl;                                                                                 \
    const bool ok = a.y && n < a.N && m < a.M;                                                               \
    const float* yr = a.yidx ? reinterpret_cast<const float*>(a.st->data_y) + (size_t)a.yidx[ok ? m : 0] * a.st->data_C \
                             : a.y + (size_t)m * a.N;                                                        \
    ysh[rl][n] = ok ? yr[n] : 0.f;                                                                           \
  }

// The rows' weights, and nnz counted by every workgroup itself over all M weights (ballot +
// popcount: an exact integer, the same in every workgroup; no float atomics, no
// cross-workgroup wait).  Read after a barrier.
template <int RB>
__device__ __forceinline__ void head_stage_weights(const HeadArgs& a, int row0, int tid, float (&wrow)[RB],
                                                   int (&nnz_s)[4]) {
  const int wave = tid >> 6, lane = tid & 63;
  const float* dw = a.yidx ? reinterpret_cast<const float*>(a.st->data_w) : a.wb;
  int cnt = 0;
  for (int m0 = 0; m0 < a.M; m0 += 256) {
    const int m = m0 + tid;
    float wv = 0.f;
    if (m < a.M) wv = !dw ? 1.f : (a.yidx ? dw[a.yidx[m]] : dw[m]);
    cnt += __popcll(__ballot(wv != 0.f));
    if (m >= row0 && m < row0 + RB) wrow[m - row0] = wv;   // (rows >= M: 0)
  }
  if (lane == 0) nnz_s[wave] = cnt;
}
// this wave's row factor w_i * (M / nnz), nnz clamped to 1
template <int RB>
__device__ __forceinline__ float head_weight_factor(const HeadArgs& a, int rw, const float (&wrow)[RB],
                                                    const int (&nnz_s)[4]) {
  const int nnz = max((nnz_s[0] + nnz_s[1]) + (nnz_s[2] + nnz_s[3]), 1);
  return wrow[rw] * ((float)a.M / (float)nnz);
}

// Advance the data cursor the step prologue gathered from (it must not move while prologue
// workgroups read it) and mark the weight packs fresh (this step's prologue re-packed them if an
// optimizer ran; the next optimizer marks them stale again)
#define HEAD_ADVANCE_CURSOR()                     \
  if (a.st && blockIdx.x == 0 && tid == 0) {      \
    if (a.training) a.st->pos += a.M;             \
    else a.st->eval_pos += a.M;                   \
    a.st->packs_stale = 0;                        \
  }

// z[NM] (declared by the kernel): the row's logits without the bias.  K split across the wave's 64 lanes (HV_: the
// row's input at padded column kp, an expression over kp and the row pointer hr), then the NM
// cross-lane chains unconditionally (z[n >= N] is 0) and interleaved: 6 dependent rounds instead
// of N guarded chains of 6 (each chain's order is unchanged)
#define HEAD_LOGITS(ACTIVE_, HV_)                                                        \
  _Pragma("unroll") for (int n = 0; n < NM; ++n) z[n] = 0.f;                             \
  if (ACTIVE_) {                                                                         \
    const bf16* hr = a.h + (size_t)row * a.Ks;                                           \
    for (int k = lane; k < a.K; k += 64) {                                               \
      const int kp = a.flat_C ? flat_keras_to_padded(k, a.flat_C, a.flat_Cs) : k;        \
      const float hv = HV_;                                                              \
      _Pragma("unroll") for (int n = 0; n < NM; ++n)                                     \
        if (n < N) z[n] += hv * (wlds ? wsh[k * N + n] : a.w[(size_t)k * N + n]);        \
    }                                                                                    \
  }                                                                                      \
  _Pragma("unroll") for (int off = 32; off > 0; off >>= 1) {                             \
    _Pragma("unroll") for (int n = 0; n < NM; ++n) z[n] += __shfl_xor(z[n], off);        \
  }

// The workgroup's loss sum ls, correct count cs and row count into the metric slots:
// order-independent integer atomics spread over 16 slots (128 workgroups on one address
// serialise at the L2, ~2 us).  A non-finite loss (diverged trial) or one beyond the fixed-point
// range (|sum| >= 2^30 per workgroup) cannot be converted: count it in the slot's spare word
// instead, and the host reports the loss as NaN (llrint of NaN/inf is undefined and would read
// as finite)
__device__ __forceinline__ void head_metric_commit(const HeadArgs& a, float ls, float cs, int rows) {
  long long* slot = a.st->metric_slots[blockIdx.x & 15];
  const bool loss_ok = isfinite(ls) && fabsf(ls) < 1073741824.f;
  if (loss_ok) atomicAdd((unsigned long long*)&slot[0], (unsigned long long)llrint((double)ls * 4294967296.0));
  else atomicAdd((unsigned long long*)&slot[3], 1ull);
  atomicAdd((unsigned long long*)&slot[1], (unsigned long long)llrintf(cs));
  atomicAdd((unsigned long long*)&slot[2], (unsigned long long)rows);
}

// dW / db partial slabs of this workgroup's rows (HV_: row rl's input at padded column kp)
#define HEAD_STORE_SLABS(HV_)                                                            \
  float* ws = a.wslab + (size_t)blockIdx.x * a.K * N;                                    \
  for (int idx = tid; idx < a.K * N; idx += 256) {                                       \
    const int k = idx / N, n = idx - (idx / N) * N;                                      \
    const int kp = a.flat_C ? flat_keras_to_padded(k, a.flat_C, a.flat_Cs) : k;          \
    float s = 0.f;                                                                       \
    for (int rl = 0; rl < rows_here; ++rl)                                               \
      s += (HV_) * dz_s[rl][n];                                                          \
    ws[idx] = s;                                                                         \
  }                                                                                      \
  if (tid < N && a.bslab) {                                                              \
    float s = 0.f;                                                                       \
    for (int rl = 0; rl < rows_here; ++rl) s += dz_s[rl][tid];                           \
    a.bslab[(size_t)blockIdx.x * N + tid] = s;                                           \
  }

// dh = dz W^T of this workgroup's rows through the previous stage's masks (t: a.bt).  The
// variadic argument is a statement run for every element (rl, c, gs) ahead of the store: a kernel
// that holds the previous stage's output itself stores the element there and `continue`s.
#define HEAD_STORE_DH(...)                                                               \
  if (t.dy) {                                                                            \
    const int width = t.pH * t.pW * t.pCs;                                               \
    for (int idx = tid; idx < rows_here * width; idx += 256) {                           \
      const int rl = idx / width;                                                        \
      const int kp = idx - rl * width;                                                   \
      const int y = kp / (t.pW * t.pCs);                                                 \
      const int rem = kp - y * t.pW * t.pCs;                                             \
      const int x = rem / t.pCs;                                                         \
      const int c = rem - x * t.pCs;                                                     \
      float gs = 0.f;                                                                    \
      if (c < t.pC) {                                                                    \
        const int k = (y * t.pW + x) * t.pC + c;                                         \
        for (int n = 0; n < N; ++n) gs += dz_s[rl][n] * (wlds ? wsh[k * N + n] : a.w[(size_t)k * N + n]); \
      }                                                                                  \
      __VA_ARGS__                                                                        \
      bwd_through_store(t, row0 + rl, y, x, c, gs, step);                                \
    }                                                                                    \
  }

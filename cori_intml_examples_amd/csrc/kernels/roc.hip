// ROC / AUC, purity, efficiency and weighted metrics (args.h RocArgs).
//
// roc_accum_kernel: one thread per (row, class column) of a batch's probabilities.  The thread
// forms the score's key, the sign of its row for that class and the row's fixed-point weight, and
// adds them to the (set, class) block of the ROC state: one histogram word and one confusion word
// per set, for a softmax head also sum(w * correct) and sum(w) of the row.  Every sum is a 64-bit
// integer atomic, so the state is order-independent and bit-identical from run to run.  Before an
// atomic is issued the wave combines the lanes that hit the same word (wave_add): a batch whose
// rows all saturate into one bin costs one atomic per wave and word, not 64.  No LDS.
//
// roc_finish_kernel: one workgroup per (set, class); the exact int64 scan of the bins from the
// top and the Mann-Whitney sum (ties counted half) in a fixed order.
#include "args.h"

namespace {

__device__ __forceinline__ int roc_key(float s) {   // (valid scores only: 0 <= s <= 1)
  // (the sign bit is cleared: of the valid scores only -0.0 has it, and it counts as 0)
  if (s < 0.5f) return (int)((__float_as_uint(s) & 0x7FFFFFFFu) >> ROC_SHIFT);
  return 2 * ROC_H - (int)(__float_as_uint(1.0f - s) >> ROC_SHIFT);
}

__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// Adds v to state[idx] for every lane with idx >= 0.  Called by ALL lanes of the wave (no lane has
// left the kernel).  ROUNDS times: the lowest pending lane's word is broadcast and the lanes that hit
// the same word are counted by a ballot; the leader issues ONE atomic for all of them.  UNIT (every
// v is 0 or 1, the unweighted set): their sum is the count, no data crosses lanes at all.  Otherwise
// a group of more than one lane sums its values by a 64-bit butterfly, a group of one adds its own
// value.  What is still pending after the rounds goes out as per-lane atomics.  Integer sums: the
// combination changes nothing in the result.
template <int ROUNDS, bool UNIT>
__device__ __forceinline__ void wave_add(long long* state, int idx, long long v, int lane) {
  if (v == 0) idx = -1;
#pragma unroll 1
  for (int r = 0; r < ROUNDS; ++r) {
    const unsigned long long pending = __ballot(idx >= 0);
    if (!pending) return;                       // wave-uniform
    const int leader = __ffsll((long long)pending) - 1;
    const int lidx = __builtin_amdgcn_readlane(idx, leader);
    const bool mine = idx == lidx;
    const int cnt = __popcll(__ballot(mine));   // >= 1: the leader
    long long sum = UNIT ? (long long)cnt : v;
    if (!UNIT && cnt > 1) sum = wave_sum_i64(mine ? v : 0);     // (wave-uniform branch)
    if (lane == leader) atomicAdd(reinterpret_cast<unsigned long long*>(state + lidx), (unsigned long long)sum);
    if (mine) idx = -1;
  }
  if (idx >= 0) atomicAdd(reinterpret_cast<unsigned long long*>(state + idx), (unsigned long long)v);
}

template <bool WT>
__global__ __launch_bounds__(ROC_THREADS) void roc_accum_kernel(const RocArgs a) {
  const int lane = threadIdx.x & 63;
  const long long gid = (long long)blockIdx.x * ROC_THREADS + threadIdx.x;
  const int N = a.N;
  const bool live = gid < (long long)a.M * N;
  const int m = live ? (int)(gid / N) : 0, n = live ? (int)(gid % N) : 0;
  // this thread's words (-1: none) and values; q: the row's fixed-point weight in the weighted set
  int hist = -1, conf = -1, inval = -1;
  bool row_words = false;
  long long correct = 0, q = 0;
  if (live) {
    const size_t drow = a.yidx ? (size_t)a.yidx[m] : (size_t)m;
    const float* yr = a.yidx ? reinterpret_cast<const float*>(a.st->data_y) + drow * a.st->data_C
                             : a.y + (size_t)m * N;
    const float* pr = a.probs + (size_t)m * N;
    const float s = pr[n];
    bool pos;
    if (a.softmax) {
      // the head's own first-maximum rule (strict '>') on the target row and on the probabilities
      int ay = 0, am = 0;
      float ymx = yr[0], pmx = pr[0];
      for (int j = 1; j < N; ++j) {
        const float yv = yr[j], pv = pr[j];
        if (yv > ymx) { ymx = yv; ay = j; }
        if (pv > pmx) { pmx = pv; am = j; }
      }
      pos = n == ay;
      row_words = n == 0;
      correct = am == ay ? 1 : 0;
    } else {
      pos = yr[n] > 0.5f;
    }
    if constexpr (WT) {
      const float* dw = a.yidx ? reinterpret_cast<const float*>(a.st->data_w) : a.wb;
      const double w = dw ? (double)dw[drow] : 1.0;
      q = __double2ll_rn(w * __longlong_as_double(a.state[1]));
    }
    const bool valid = s >= 0.f && s <= 1.f;    // (NaN: false)
    if (valid) {
      hist = (pos ? 0 : ROC_BINS) + roc_key(s);
      const bool pred = s > 0.5f;
      conf = 2 * ROC_BINS + (pred ? (pos ? ROC_T_TP : ROC_T_FP) : (pos ? ROC_T_FN : ROC_T_TN));
    } else {
      inval = 2 * ROC_BINS + ROC_T_INVALID;
    }
  }
  const int b0 = ROC_HDR + n * ROC_BLOCK;                      // set 0, class n
  const int b1 = ROC_HDR + (N + n) * ROC_BLOCK;                // set 1, class n
  auto at = [](int base, int word) { return word < 0 ? -1 : base + word; };
  wave_add<4, true>(a.state, at(b0, hist), 1, lane);
  wave_add<4, true>(a.state, at(b0, conf), 1, lane);
  wave_add<1, true>(a.state, at(b0, inval), 1, lane);
  if (a.softmax) {
    wave_add<1, true>(a.state, row_words ? b0 + 2 * ROC_BINS + ROC_T_WC : -1, correct, lane);
    wave_add<1, true>(a.state, row_words ? b0 + 2 * ROC_BINS + ROC_T_WS : -1, 1, lane);
  }
  if constexpr (WT) {
    wave_add<4, false>(a.state, at(b1, hist), q, lane);
    wave_add<4, false>(a.state, at(b1, conf), q, lane);
    wave_add<1, true>(a.state, at(b1, inval), q > 0 ? 1 : 0, lane);
    if (a.softmax) {
      wave_add<1, false>(a.state, row_words ? b1 + 2 * ROC_BINS + ROC_T_WC : -1, correct * q, lane);
      wave_add<1, false>(a.state, row_words ? b1 + 2 * ROC_BINS + ROC_T_WS : -1, q, lane);
    }
  }
}

// Thread t owns the bins j in [t * CH, (t + 1) * CH) counted from the TOP (bin ROC_BINS - 1 - j).
__global__ __launch_bounds__(ROC_THREADS) void roc_finish_kernel(const RocArgs a) {
  constexpr int CH = (ROC_BINS + ROC_THREADS - 1) / ROC_THREADS;
  __shared__ long long psum[ROC_THREADS], nsum[ROC_THREADS];
  __shared__ double dsum[ROC_THREADS];
  const int t = threadIdx.x;
  const long long* blk = a.state + ROC_HDR + (size_t)blockIdx.x * ROC_BLOCK;
  const long long* pos = blk;
  const long long* neg = blk + ROC_BINS;
  const int j0 = t * CH, j1 = min(j0 + CH, ROC_BINS);
  long long ps = 0, ns = 0;
  for (int j = j0; j < j1; ++j) {
    ps += pos[ROC_BINS - 1 - j];
    ns += neg[ROC_BINS - 1 - j];
  }
  psum[t] = ps;
  nsum[t] = ns;
  __syncthreads();
  // positives above this thread's bins, and the totals (exact integers: any order)
  long long above = 0, P = 0, Nn = 0;
  for (int i = 0; i < ROC_THREADS; ++i) {
    if (i < t) above += psum[i];
    P += psum[i];
    Nn += nsum[i];
  }
  double acc = 0.0;
  for (int j = j0; j < j1; ++j) {
    const long long pb = pos[ROC_BINS - 1 - j], nb = neg[ROC_BINS - 1 - j];
    acc += (double)nb * (double)(2 * above + pb);
    above += pb;
  }
  dsum[t] = acc;
  __syncthreads();
  for (int off = ROC_THREADS / 2; off > 0; off >>= 1) {      // fixed tree order
    if (t < off) dsum[t] += dsum[t + off];
    __syncthreads();
  }
  long long* res = a.res + (size_t)blockIdx.x * ROC_RES_WORDS;
  if (t == 0) {
    const double auc = (P > 0 && Nn > 0) ? dsum[0] / (2.0 * (double)P * (double)Nn) : __longlong_as_double(0x7FF8000000000000LL);
    res[0] = __double_as_longlong(auc);
    res[1] = P;
    res[2] = Nn;
  }
  if (t < ROC_TAIL) res[3 + t] = blk[2 * ROC_BINS + t];
}

void roc_check(const RocArgs& a, const std::string& w) {
  if (a.N < 1 || a.N > ROC_MAX_N) throw std::invalid_argument(w + ": N must be 1.." + std::to_string(ROC_MAX_N));
  if (!a.state) throw std::invalid_argument(w + ": null state pointer");
  if (reinterpret_cast<uintptr_t>(a.state) & 7) throw std::invalid_argument(w + ": state pointer not 8-byte aligned");
}

}  // namespace

void launch_roc_accum(const RocArgs& a, hipStream_t s) {
  const std::string w("roc_accum");
  if (a.M < 1) throw std::invalid_argument(w + ": M must be >= 1");
  roc_check(a, w);
  if (!a.probs) throw std::invalid_argument(w + ": null probs pointer");
  if (!a.softmax && a.N != 1) throw std::invalid_argument(w + ": a sigmoid head has N == 1");
  if (a.softmax && a.N < 2) throw std::invalid_argument(w + ": a softmax head has N >= 2");
  if (a.yidx ? !a.st : !a.y) throw std::invalid_argument(w + ": null target pointer (y, or yidx with st)");
  if ((long long)a.M * a.N > (1LL << 31) - ROC_THREADS) throw std::invalid_argument(w + ": M * N too large");
  const dim3 grid((unsigned)(((long long)a.M * a.N + ROC_THREADS - 1) / ROC_THREADS)), block(ROC_THREADS);
  if (a.weighted) hipLaunchKernelGGL(roc_accum_kernel<true>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(roc_accum_kernel<false>, grid, block, 0, s, a);
}

void launch_roc_finish(const RocArgs& a, hipStream_t s) {
  const std::string w("roc_finish");
  roc_check(a, w);
  if (!a.res) throw std::invalid_argument(w + ": null result pointer");
  if (reinterpret_cast<uintptr_t>(a.res) & 7) throw std::invalid_argument(w + ": result pointer not 8-byte aligned");
  hipLaunchKernelGGL(roc_finish_kernel, dim3(2 * a.N), dim3(ROC_THREADS), 0, s, a);
}

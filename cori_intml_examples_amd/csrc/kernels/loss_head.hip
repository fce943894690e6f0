// The second output head: every (activation, loss) pair of the loss table that head_kernel
// (head.hip) does not run -- mse on a sigmoid / softmax output, mae, msle, logcosh, hinge,
// squared_hinge, categorical_hinge, kld, poisson on a linear / sigmoid / softmax output, and
// binary_crossentropy on a sigmoid output of more than one column (multi-label).
//   logits = h W + b  ->  p = A(logits)  ->  row loss l(p, y), g = dl/dp  ->  dz through A
// Four rows per workgroup, one wave per row, K split across the 64 lanes; after the logit
// reduction lane n of the row's first 16 lanes owns column n: p, l, g, the chain to the logits
// and the accuracy are per-lane code with 16-lane trees for the row sums and argmaxes.  The loss
// is a uniform run-time switch (HeadArgs::loss).  Metrics, probabilities, dW / db slabs and
// dh = dz W^T are head_kernel's, in the same layouts (head_common.h).  The input is always a
// stored bf16 buffer: this kernel never absorbs a split-K dense epilogue.
//
// Semantics are Keras 2.2.4 on the TF backend in fp32 (README, "Losses"): a maximum's tie gives
// the first argument the gradient, clips pass it on the closed interval, the FIRST row maximum
// takes categorical_hinge's whole gradient.  A NaN propagates into the loss (the metric commit
// then counts the workgroup in the non-finite word) and into dz.
#include <stdexcept>
#include <string>

#include "head_common.h"

// row sum / first argmax over the row's columns: identities for the one-column instance
template <int NM>
__device__ __forceinline__ float row_sum(float v) {
  if constexpr (NM == 1) return v;
  else return grp16_sum(v);
}
template <int NM>
__device__ __forceinline__ void row_argmax(float& v, int& i) {
  if constexpr (NM > 1) grp16_argmax(v, i);
}
// max(v, 0) that keeps a NaN (fmaxf would return the 0)
__device__ __forceinline__ float relu_nan(float v) { return v != v ? v : fmaxf(v, 0.f); }

// WT: the sample-weighted loss, as in head_kernel (row factor wf = w_i * M / nnz).
template <int NM, bool WT>
__global__ __launch_bounds__(256) void loss_head_kernel(const HeadArgs a) {
  __shared__ float dz_s[HEAD_RB][NM];
  __shared__ float met[HEAD_RB][2];
  __shared__ float wsh[HEAD_W_LDS];      // head weights [K][N] when they fit (read twice below)
  __shared__ float ysh[HEAD_RB][16], bsh[16];
  __shared__ float wrow[HEAD_RB];
  __shared__ int nnz_s[4];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const bool w_in_lds = a.K * a.N <= HEAD_W_LDS;
  if (w_in_lds)
    for (int i = tid; i < a.K * a.N; i += 256) wsh[i] = a.w[i];
  const int row0 = blockIdx.x * HEAD_RB;
  const int N = a.N;
  const uint32_t step = a.st ? (uint32_t)a.st->t : 0u;
  const int rw = wave, row = row0 + wave;
  HEAD_STAGE_TARGETS(HEAD_RB);
  if constexpr (WT) head_stage_weights<HEAD_RB>(a, row0, tid, wrow, nnz_s);
  HEAD_ADVANCE_CURSOR();
  __syncthreads();
  float wf = 1.f;
  if constexpr (WT) wf = head_weight_factor<HEAD_RB>(a, rw, wrow, nnz_s);
  const bool live = row < a.M;
  // (a branch per weight source, `wlds` a constant in each: the compiler rejects this kernel's
  // run-time select between an LDS and a global weight load)
  float z[NM];
  if (w_in_lds) {
    constexpr bool wlds = true;
    HEAD_LOGITS(live, bf2f(hr[kp]));
  } else {
    constexpr bool wlds = false;
    HEAD_LOGITS(live, bf2f(hr[kp]));
  }

  // lane n < 16 of the row's wave: column n
  const int n = lane & 15;
  const bool cls = live && lane < 16 && n < N;
  float zn = 0.f;
#pragma unroll
  for (int j = 0; j < NM; ++j)
    if (j == n) zn = z[j];
  zn += bsh[n];
  float p = zn;
  if (a.act == 1) {
    p = 1.f / (1.f + expf(-zn));
  } else if (a.act == 2) {
    float mx = cls ? zn : -__builtin_inff();
    int am = cls ? n : 1 << 20;
    row_argmax<NM>(mx, am);
    const float e = cls ? expf(zn - mx) : 0.f;
    p = e / row_sum<NM>(e);
  }
  if (!cls) p = 0.f;
  if (cls && a.probs) a.probs[(size_t)row * N + n] = p;
  float loss = 0.f, dzn = 0.f, correct = 0.f;
  if (a.y) {
    const float eps = 1e-7f;
    const float y = cls ? ysh[rw][n] : 0.f;
    const float fN = (float)N;
    float l = 0.f, g = 0.f;
    bool direct = false;               // g is already dl/dz (binary_crossentropy)
    switch (a.loss) {
      case LOSS_MSE: {
        const float d = p - y;
        l = d * d / fN;
        g = 2.f * d / fN;
      } break;
      case LOSS_MAE: {
        const float d = p - y;
        l = fabsf(d) / fN;
        g = (d > 0.f ? 1.f : d < 0.f ? -1.f : 0.f) / fN;
      } break;
      case LOSS_MSLE: {
        const float pm = p != p ? p : fmaxf(p, eps), ym = y != y ? y : fmaxf(y, eps);
        const float d = logf(pm + 1.f) - logf(ym + 1.f);
        l = d * d / fN;
        g = p >= eps ? 2.f * d / (pm + 1.f) / fN : 0.f;
      } break;
      case LOSS_LOGCOSH: {
        const float d = p - y, ad = fabsf(d);
        l = (ad + log1pf(expf(-2.f * ad)) - 0.69314718f) / fN;
        g = tanhf(d) / fN;
      } break;
      case LOSS_HINGE: {
        const float m = 1.f - y * p;
        l = relu_nan(m) / fN;
        g = m >= 0.f ? -y / fN : 0.f;
      } break;
      case LOSS_SQ_HINGE: {
        const float hm = relu_nan(1.f - y * p);
        l = hm * hm / fN;
        g = -2.f * y * hm / fN;
      } break;
      case LOSS_CAT_HINGE: {
        const float pos = row_sum<NM>(cls ? y * p : 0.f);
        float neg = cls ? (1.f - y) * p : -__builtin_inff();
        int m = cls ? n : 1 << 20;
        row_argmax<NM>(neg, m);
        const float v = neg - pos + 1.f;
        l = n == 0 ? relu_nan(v) : 0.f;
        g = v > 0.f ? (-y + (n == m ? 1.f - y : 0.f)) : (v != v ? v : 0.f);
      } break;
      case LOSS_KLD: {
        const float yc = clip_nan(y, eps, 1.f), pc = clip_nan(p, eps, 1.f);
        l = yc * logf(yc / pc);
        g = (p >= eps && p <= 1.f) ? -yc / pc : 0.f;
      } break;
      case LOSS_POISSON: {
        const float q = p + eps;
        l = (p - y * logf(q)) / fN;
        g = (1.f - y / q) / fN;
      } break;
      default: {   // LOSS_BCE on a sigmoid output: head_kernel's per-element formula, mean over the columns
        const bool inr = (p >= eps) && (p <= 1.f - eps);
        const float pc = clip_nan(p, eps, 1.f - eps);
        const float lg = logf(pc / (1.f - pc));
        l = (fmaxf(lg, 0.f) - lg * y + log1pf(expf(-fabsf(lg)))) / fN;
        g = inr ? (pc - y) / fN : 0.f;
        direct = true;
      } break;
    }
    if (p != p) g = p;                 // (the masks' comparisons are false for a NaN)
    if (!cls) { l = 0.f; g = 0.f; }
    if (direct || a.act == 0) dzn = g;
    else if (a.act == 1) dzn = g * p * (1.f - p);
    else dzn = p * (g - row_sum<NM>(p * g));
    loss = row_sum<NM>(l);
    if (NM == 1 || N == 1 || a.loss == LOSS_BCE) {
      // binary_accuracy: the row's count of correct ELEMENTS (the host divides by rows * N)
      correct = row_sum<NM>((cls && rintf(p) == y) ? 1.f : 0.f);
    } else {
      float pmx = cls ? p : -__builtin_inff(), ymx = cls ? y : -__builtin_inff();
      int ap = cls ? n : 1 << 20, ay = ap;
      row_argmax<NM>(pmx, ap);
      row_argmax<NM>(ymx, ay);
      correct = (live && ap == ay) ? 1.f : 0.f;
    }
  }
  if constexpr (WT) {
    dzn = dzn * a.inv_bs * wf;
    loss *= wf;
  } else {
    dzn = dzn * a.inv_bs;
  }
  if (lane < NM) dz_s[rw][lane] = cls ? dzn : 0.f;
  if (lane == 0) {
    met[rw][0] = live ? loss : 0.f;
    met[rw][1] = live ? correct : 0.f;
  }
  __syncthreads();
  const int rows_here = min(HEAD_RB, a.M - row0);
  if (tid == 0 && a.y && a.st) {
    float ls = 0.f, cs = 0.f;
    for (int r = 0; r < rows_here; ++r) { ls += met[r][0]; cs += met[r][1]; }
    head_metric_commit(a, ls, cs, rows_here);
  }
  if (!a.training) return;
  HEAD_STORE_SLABS(bf2f(a.h[(size_t)(row0 + rl) * a.Ks + kp]));
  const BwdThrough& t = a.bt;
  if (w_in_lds) {
    constexpr bool wlds = true;
    HEAD_STORE_DH();
  } else {
    constexpr bool wlds = false;
    HEAD_STORE_DH();
  }
}

template <bool WT>
static void launch_loss_head_wt(const HeadArgs& a, hipStream_t s) {
  const dim3 g4((a.M + HEAD_RB - 1) / HEAD_RB);
  if (a.N == 1) hipLaunchKernelGGL((loss_head_kernel<1, WT>), g4, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((loss_head_kernel<16, WT>), g4, dim3(256), 0, s, a);
}

void launch_loss_head(const HeadArgs& a, hipStream_t s) {
  const std::string w("loss_head");
  if (a.N < 1 || a.N > 16) throw std::invalid_argument(w + ": N must be in 1..16, got " + std::to_string(a.N));
  if (a.loss < 0 || a.loss >= LOSS_COUNT) throw std::invalid_argument(w + ": unknown loss code " + std::to_string(a.loss));
  if (a.act < 0 || a.act > 2) throw std::invalid_argument(w + ": unknown activation code " + std::to_string(a.act));
  if (a.loss == LOSS_BCE && a.act != 1)
    throw std::invalid_argument(w + ": binary_crossentropy needs a sigmoid output (act 1)");
  if (a.M < 1 || a.K < 1 || a.Ks < 1) throw std::invalid_argument(w + ": M, K and Ks must be positive");
  if ((long long)a.K * a.N > 0x7fffffffLL) throw std::invalid_argument(w + ": K * N must be below 2^31");
  if (!a.h || !a.w) throw std::invalid_argument(w + ": null input or weight pointer");
  if (a.epi.part != nullptr) throw std::invalid_argument(w + ": this head never absorbs a dense epilogue");
  if (a.training && (!a.y || !a.wslab)) throw std::invalid_argument(w + ": a training launch needs targets and slabs");
  if (a.yidx && !a.st) throw std::invalid_argument(w + ": dataset-row targets need the step state");
  if (a.wb != nullptr && a.y != nullptr) launch_loss_head_wt<true>(a, s);
  else launch_loss_head_wt<false>(a, s);
}

// The wide output head: 17..1024 columns, the three classic (activation, loss) pairs
//   softmax + (sparse_)categorical_crossentropy, sigmoid + binary_crossentropy (multi-label),
//   linear + mse
// with the formulas, clips and accuracy rules of head_kernel / loss_head_kernel (head.hip,
// loss_head.hip), on the matrix cores.  One workgroup per 16-row tile of the batch, at most
// WIDE_HEAD_MAX_SLABS workgroups: workgroup b walks tiles b, b + grid, ... in order and owns slab b
// of the dW / db partials (its first tile stores, its later tiles add to what it stored itself:
// one workgroup, program order, so the slabs are bit-identical from launch to launch).  No
// cross-workgroup wait, no float atomics.  Per tile:
//   1. Z = H W + b: the 16 x K input tile goes to LDS (bf16, K chunks of WIDE_HEAD_KC); wave w owns
//      the N-tiles w, w + 4, ... and keeps one 16 x 16 fp32 accumulator in registers over the
//      chunk's K loop (v_mfma_f32_16x16x32_bf16).  The B fragment -- 8 k of one column -- is read
//      from the fp32 MASTER directly and rounded to bf16 in registers: a weight is used by exactly
//      one wave of the tile, the master's offset in the parameter store is only 4-byte aligned
//      and a row of N floats is no multiple of 16 bytes for most N, so staging it through LDS
//      would be the same number of 4-byte loads plus a barrier pair per K step.  Z (+ bias) goes to
//      the LDS logit buffer [16][N] fp32 (64 KB at N = 1024: what fixes the width cap).
//   2. the row loss: wave w takes rows w, w + 4, ...; its 64 lanes stride over the row's columns
//      with wave-wide butterflies for the first maximum, the exp-sum, the loss and the accuracy
//      count.  dz / M replaces the logits in place (fp32: db's column sums) and goes to a second
//      LDS tile as bf16 (the two backward products' operand, rows >= M and columns >= N zero).
//   3. dh = dz W^T (reduction over N, 16x16x32): waves own 16-column tiles of the previous stage's
//      PADDED output; the B fragment, 8 consecutive n of row k of w, is contiguous in the master.
//      Every element goes through bwd_through_store.
//   4. dW slab = H^T dz (reduction over the tile's 16 rows, 16x16x16: no zero-padded half): waves
//      own K-tiles, A is H^T straight from global (rows >= M zero), B a transposed LDS read
//      (ds_read_b64_tr_b16) of the bf16 dz tile.
// Evaluation and predict plans run 1 and 2 only.
#include <stdexcept>
#include <string>

#include "head_common.h"

#define WIDE_HEAD_MAX_SLABS 16
#define WIDE_HEAD_MIN_N 17
#define WIDE_HEAD_MAX_N 1024
#define WIDE_HEAD_KC 1024      // input columns staged per K chunk

namespace {

// LDS: logits [16][ldz] fp32 | dz [16][ldd] bf16 | input chunk [16][ldh] bf16.  ldz = 4 mod 16
// (an accumulator's four row groups land in four different bank quarters), ldd and ldh multiples
// of 8 (16-byte fragment reads) that are 8 mod 64 / 8 mod 32.
struct WideLds {
  int ldz, ldd, ldh, kc;
  size_t off_dz, off_h, bytes;
};
__host__ __device__ inline WideLds wide_lds(int K, int N) {
  WideLds l;
  l.ldz = ((N + 15) & ~15) + 4;
  l.ldd = ((N + 31) & ~31) + 8;
  const int k32 = (K + 31) & ~31;
  l.kc = k32 < WIDE_HEAD_KC ? k32 : WIDE_HEAD_KC;
  l.ldh = l.kc + 8;
  l.off_dz = (size_t)16 * l.ldz * 4;
  l.off_h = l.off_dz + (size_t)16 * l.ldd * 2;
  l.bytes = l.off_h + (size_t)16 * l.ldh * 2;
  return l;
}

__device__ __forceinline__ bf16x4 wide_tr_read(const bf16* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4bf16(LDS_PTR(bf16x4, p));
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
// max value and its lowest index over the wave (grp16_argmax's rule: the first maximum wins)
__device__ __forceinline__ void wave_argmax(float& v, int& i) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(v, off);
    const int oi = __shfl_xor(i, off);
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
  }
}

// softmax_cce_lanes' gradient wrt the clipped, renormalised probability q = p / ps of one column
__device__ __forceinline__ float cce_gn(float p, float ps, float y) {
  const float eps = 1e-7f;
  const float q = p / ps;
  const bool inr = (q >= eps) && (q <= 1.f - eps);
  return inr ? -y / clip_nan(q, eps, 1.f - eps) : 0.f;
}

// The launch's arguments, re-read from the kernel-argument segment (HeadArgs is the kernel's ONE
// by-value argument: offset 0; the static_assert under the kernel pins that signature).  Each phase starts from a pointer the compiler cannot see through, so a
// phase's fields are scalar loads of its own and not ~100 SGPRs held live across the whole tile
// loop (which spilled 81..96 of them).
__device__ __forceinline__ const HeadArgs& wide_args() {
  typedef const __attribute__((address_space(4))) HeadArgs* KP;
  KP p = (KP)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return *(const HeadArgs*)p;
}

}  // namespace

// What every phase derives from the arguments it re-reads (names the kernel's smem)
#define WIDE_PHASE_LOCALS()                                                      \
  const HeadArgs& a = wide_args();                                               \
  const int N = a.N, K = a.K, M = a.M;                                           \
  const WideLds L = wide_lds(K, N);                                              \
  float* zs = reinterpret_cast<float*>(smem);                                    \
  bf16* dzs = reinterpret_cast<bf16*>(smem + L.off_dz);                          \
  bf16* hs = reinterpret_cast<bf16*>(smem + L.off_h);                            \
  const int NT = (N + 15) >> 4, NS = (N + 31) >> 5;                              \
  const int rows_here = min(16, M - row0);                                       \
  (void)zs; (void)dzs; (void)hs; (void)NT; (void)NS; (void)rows_here

// WT: the sample-weighted loss, as in head_kernel (row factor wf = w_i * M / max(nnz, 1), nnz
// counted by every workgroup itself).
template <bool WT>
__global__ __launch_bounds__(256) void wide_head_kernel(const HeadArgs) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ float met[16][2];
  __shared__ float wrow[16];
  __shared__ int nnz_s[4];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 15, g = lane >> 4;
  const HeadArgs& a = wide_args();
  const int tiles = (a.M + 15) >> 4;
  HEAD_ADVANCE_CURSOR();

  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int row0 = tile * 16;
    const bool first = tile == (int)blockIdx.x;      // this workgroup's first tile: its slab is stored
    __syncthreads();                                 // (the previous tile's readers of the LDS tiles)
    if constexpr (WT) head_stage_weights<16>(wide_args(), row0, tid, wrow, nnz_s);

    // ------------------------------------------------------------------ 1. logits
    {
    WIDE_PHASE_LOCALS();
    for (int kc0 = 0; kc0 < K; kc0 += L.kc) {
      const int ksteps = (min(L.kc, K - kc0) + 31) >> 5;
      // the input chunk: Keras column k of the row is padded column kp of h (a flattened conv's
      // padded channels are never read: they contribute nothing); rows >= M and columns >= K zero
      for (int r = wave; r < 16; r += 4) {
        const int row = row0 + r;
        const bf16* hr = a.h + (size_t)min(row, M - 1) * a.Ks;
        for (int kk = lane; kk < ksteps * 32; kk += 64) {
          const int k = kc0 + kk;
          const int kc = min(k, K - 1);
          const int kp = a.flat_C ? flat_keras_to_padded(kc, a.flat_C, a.flat_Cs) : kc;
          const bf16 v = hr[kp];
          hs[r * L.ldh + kk] = (row < M && k < K) ? v : f2bf(0.f);
        }
      }
      __syncthreads();
      for (int nt = wave; nt < NT; nt += 4) {
        const int n = nt * 16 + i;
        const bool ncol = n < N;
        const float* wc = a.w + (ncol ? n : 0);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int ks = 0; ks < ksteps; ++ks) {
          const bf16x8 afr = *reinterpret_cast<const bf16x8*>(hs + i * L.ldh + ks * 32 + 8 * g);
          bf16x8 bfr;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int k = kc0 + ks * 32 + 8 * g + j;
            const float v = wc[(size_t)min(k, K - 1) * N];     // (always loaded, then selected)
            bfr[j] = f2bf((ncol && k < K) ? v : 0.f);
          }
          acc = mfma16(afr, bfr, acc);
        }
        const float b0 = (kc0 == 0 && ncol && a.bias) ? a.bias[n] : 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float* z = zs + (4 * g + j) * L.ldz + n;
          *z = (kc0 == 0 ? b0 : *z) + acc[j];
        }
      }
      __syncthreads();
    }

    }
    // ------------------------------------------------------------------ 2. row loss
    {
    WIDE_PHASE_LOCALS();
    const float fN = (float)N, eps = 1e-7f;
    for (int r = wave; r < 16; r += 4) {
      const int row = row0 + r;
      float* zr = zs + r * L.ldz;
      bf16* dr = dzs + r * L.ldd;
      if (row >= M) {                                  // (wave-uniform)
        if (a.training) {
          for (int n = lane; n < N; n += 64) zr[n] = 0.f;
          for (int n = lane; n < NS * 32; n += 64) dr[n] = f2bf(0.f);
        }
        if (lane == 0) met[r][0] = met[r][1] = 0.f;
        continue;
      }
      const float* yr = nullptr;
      if (a.y)
        yr = a.yidx ? reinterpret_cast<const float*>(a.st->data_y) + (size_t)a.yidx[row] * a.st->data_C
                    : a.y + (size_t)row * N;
      float* pr = a.probs ? a.probs + (size_t)row * N : nullptr;
      float sc = a.inv_bs, wf = 1.f;                   // dz = dL/dz * sc
      if constexpr (WT) {
        wf = head_weight_factor<16>(a, r, wrow, nnz_s);
        sc = a.inv_bs * wf;
      }
      float loss = 0.f;
      int correct = 0;
      if (a.act == 2) {
        float mx = -__builtin_inff();
        int am = 1 << 20;
        for (int n = lane; n < N; n += 64)
          if (zr[n] > mx) { mx = zr[n]; am = n; }
        wave_argmax(mx, am);
        float s = 0.f;
        for (int n = lane; n < N; n += 64) {
          const float e = expf(zr[n] - mx);
          zr[n] = e;
          s += e;
        }
        s = wave_sum(s);
        float ps = 0.f;
        for (int n = lane; n < N; n += 64) {
          const float p = zr[n] / s;
          zr[n] = p;
          if (pr) pr[n] = p;
          ps += p;
        }
        ps = wave_sum(ps);
        if (yr) {
          float gq = 0.f, ymx = -__builtin_inff();
          int ay = 1 << 20;
          for (int n = lane; n < N; n += 64) {
            const float p = zr[n], yn = yr[n], q = p / ps;
            loss -= yn * logf(clip_nan(q, eps, 1.f - eps));
            gq += cce_gn(p, ps, yn) * q;
            if (yn > ymx) { ymx = yn; ay = n; }
          }
          loss = wave_sum(loss);
          gq = wave_sum(gq);
          wave_argmax(ymx, ay);
          correct = am == ay ? 1 : 0;
          if (a.training) {
            float pg = 0.f;
            for (int n = lane; n < N; n += 64) pg += zr[n] * ((cce_gn(zr[n], ps, yr[n]) - gq) / ps);
            pg = wave_sum(pg);
            for (int n = lane; n < N; n += 64) {
              const float p = zr[n];
              const float dzn = p * ((cce_gn(p, ps, yr[n]) - gq) / ps - pg) * sc;
              zr[n] = dzn;
              dr[n] = f2bf(dzn);
            }
          }
        }
      } else {
        for (int n = lane; n < N; n += 64) {
          const float z = zr[n];
          float p = z, l = 0.f, gz = 0.f;
          if (a.act == 1) p = 1.f / (1.f + expf(-z));
          if (pr) pr[n] = p;
          if (yr) {
            const float yn = yr[n];
            if (a.act == 1) {
              // loss_head_kernel's binary_crossentropy element (mean over the columns)
              const bool inr = (p >= eps) && (p <= 1.f - eps);
              const float pc = clip_nan(p, eps, 1.f - eps);
              const float lg = logf(pc / (1.f - pc));
              l = (fmaxf(lg, 0.f) - lg * yn + log1pf(expf(-fabsf(lg)))) / fN;
              gz = inr ? (pc - yn) / fN : 0.f;
              if (p != p) gz = p;
              correct += rintf(p) == yn ? 1 : 0;
            } else {
              const float d = z - yn;
              l = d * d / fN;
              gz = 2.f * d / fN;
            }
          }
          loss += l;
          if (a.training) {
            zr[n] = gz * sc;
            dr[n] = f2bf(gz * sc);
          }
        }
        loss = wave_sum(loss);
        correct = wave_sum(correct);
      }
      if (a.training)
        for (int n = N + lane; n < NS * 32; n += 64) dr[n] = f2bf(0.f);
      if constexpr (WT) loss *= wf;
      if (lane == 0) {
        met[r][0] = loss;
        met[r][1] = (float)correct;
      }
    }
    }
    __syncthreads();
    if (tid == 0 && a.y && a.st) {
      const int rows_here = min(16, a.M - row0);
      float ls = 0.f, cs = 0.f;
      for (int r = 0; r < rows_here; ++r) { ls += met[r][0]; cs += met[r][1]; }
      head_metric_commit(a, ls, cs, rows_here);
    }
    if (!a.training) continue;

    {
    WIDE_PHASE_LOCALS();
    // db slab: the fp32 dz tile's column sums in row order
    if (a.bslab)
      for (int n = tid; n < N; n += 256) {
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) s += zs[r * L.ldz + n];
        float* b = a.bslab + (size_t)blockIdx.x * N + n;
        *b = first ? s : *b + s;
      }

    // ------------------------------------------------------------------ 3. dh = dz W^T
    const BwdThrough& t = a.bt;
    const uint32_t step = a.st ? (uint32_t)a.st->t : 0u;
    if (t.dy) {
      const int width = t.pH * t.pW * t.pCs;
      for (int kt = wave; kt * 16 < width; kt += 4) {
        const int kp = kt * 16 + i;                    // this lane's padded column of the previous stage
        const int y = kp / (t.pW * t.pCs);
        const int rem = kp - y * t.pW * t.pCs;
        const int x = rem / t.pCs;
        const int c = rem - x * t.pCs;
        const bool kcol = kp < width && c < t.pC;
        const float* wr = a.w + (kcol ? (size_t)((y * t.pW + x) * t.pC + c) * N : 0);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int ns = 0; ns < NS; ++ns) {
          const bf16x8 afr = *reinterpret_cast<const bf16x8*>(dzs + i * L.ldd + ns * 32 + 8 * g);
          bf16x8 bfr;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int n = ns * 32 + 8 * g + j;
            const float v = wr[min(n, N - 1)];
            bfr[j] = f2bf((kcol && n < N) ? v : 0.f);
          }
          acc = mfma16(afr, bfr, acc);
        }
        if (kp < width) {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (4 * g + j < rows_here) bwd_through_store(t, row0 + 4 * g + j, y, x, c, acc[j], step);
        }
      }
    }

    }
    // ------------------------------------------------------------------ 4. dW slab = H^T dz
    WIDE_PHASE_LOCALS();
    float* ws = a.wslab + (size_t)blockIdx.x * K * N;
    for (int kt = wave; kt * 16 < K; kt += 4) {
      const int k = kt * 16 + i;                       // A[k][m = 4 g + j] = h[row0 + m][kp(k)]
      const int kc = min(k, K - 1);
      const int kp = a.flat_C ? flat_keras_to_padded(kc, a.flat_C, a.flat_Cs) : kc;
      bf16x4 afr;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = row0 + 4 * g + j;
        const bf16 v = a.h[(size_t)min(row, M - 1) * a.Ks + kp];
        afr[j] = (row < M && k < K) ? v : f2bf(0.f);
      }
      for (int nt = 0; nt < NT; ++nt) {
        const bf16x4 bfr = wide_tr_read(dzs + (4 * g + (i >> 2)) * L.ldd + nt * 16 + 4 * (i & 3));
        const f32x4 acc = mfma16k16(afr, bfr, f32x4{0.f, 0.f, 0.f, 0.f});
        const int n = nt * 16 + i;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int ko = kt * 16 + 4 * g + j;
          if (ko < K && n < N) {
            float* d = ws + (size_t)ko * N + n;
            *d = first ? acc[j] : *d + acc[j];
          }
        }
      }
    }
  }
}

// wide_args() reads the kernel-argument segment as a HeadArgs: the kernel takes exactly that, by value
static_assert(std::is_same<decltype(&wide_head_kernel<false>), void (*)(HeadArgs)>::value &&
                  std::is_same<decltype(&wide_head_kernel<true>), void (*)(HeadArgs)>::value,
              "wide_args() needs HeadArgs as the only, by-value kernel argument");

// workgroups of the launch = dW / db slabs it writes
int wide_head_slabs(int M) {
  const int tiles = (M + 15) / 16;
  return tiles < WIDE_HEAD_MAX_SLABS ? tiles : WIDE_HEAD_MAX_SLABS;
}
int wide_head_max_n() { return WIDE_HEAD_MAX_N; }

void launch_wide_head(const HeadArgs& a, hipStream_t s) {
  const std::string w("wide_head");
  if (a.N < WIDE_HEAD_MIN_N || a.N > WIDE_HEAD_MAX_N)
    throw std::invalid_argument(w + ": N must be in " + std::to_string(WIDE_HEAD_MIN_N) + ".." +
                                std::to_string(WIDE_HEAD_MAX_N) + ", got " + std::to_string(a.N));
  if (a.act < 0 || a.act > 2) throw std::invalid_argument(w + ": unknown activation code " + std::to_string(a.act));
  if (a.loss != (a.act == 2 ? LOSS_CCE : a.act == 1 ? LOSS_BCE : LOSS_MSE))
    throw std::invalid_argument(w + ": no instance for activation code " + std::to_string(a.act) + " with loss code " +
                                std::to_string(a.loss) + " (softmax + categorical_crossentropy, sigmoid + "
                                "binary_crossentropy, linear + mse)");
  if (a.M < 1 || a.K < 1 || a.Ks < 1) throw std::invalid_argument(w + ": M, K and Ks must be positive");
  if ((long long)a.K * a.N > 0x7fffffffLL) throw std::invalid_argument(w + ": K * N must be below 2^31");
  if (!a.h || !a.w) throw std::invalid_argument(w + ": null input or weight pointer");
  if (a.epi.part != nullptr) throw std::invalid_argument(w + ": this head never absorbs a dense epilogue");
  if (a.training && (!a.y || !a.wslab)) throw std::invalid_argument(w + ": a training launch needs targets and slabs");
  if (a.yidx && !a.st) throw std::invalid_argument(w + ": dataset-row targets need the step state");
  const size_t lds = wide_lds(a.K, a.N).bytes;
  const dim3 grid(wide_head_slabs(a.M));
  const bool wt = a.wb != nullptr && a.y != nullptr;
  const void* k = wt ? (const void*)wide_head_kernel<true> : (const void*)wide_head_kernel<false>;
  if (lds > 65536) (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (wt) hipLaunchKernelGGL(wide_head_kernel<true>, grid, dim3(256), lds, s, a);
  else hipLaunchKernelGGL(wide_head_kernel<false>, grid, dim3(256), lds, s, a);
}

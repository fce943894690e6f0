// Depthwise convolution, depth_multiplier 1 (Keras DepthwiseConv2D, the depthwise half of a
// SeparableConv2D): forward, the gradient to its input, the per-channel weight gradient (DwArgs, args.h).
//
//   dw_fwd    out[b, y, x, c] = bf16(A(bias[c] + sum_{ky, kx} w[ky, kx, c] * x[b, y*s + ky - pad_t, x*s + kx - pad_l, c]))
//   dw_dgrad  dx[b, y, x, c]  = sum_{ky, kx} w[ky, kx, c] * dt[b, (y + pad_t - ky) / s, (x + pad_l - kx) / s, c]
//             over the taps where both divisions are exact and in range, handed to the feeding stage's
//             BwdThrough (its dropout mask, relu mask and bf16 rounding)
//   dw_wgrad  dW[ky, kx, c]   = sum_{b, y, x} x[b, y*s + ky - pad_t, x*s + kx - pad_l, c] * dt[b, y, x, c]
//             db[c]           = sum_{b, y, x} dt[b, y, x, c]
//
// There is nothing to contract over -- KH * KW multiply-adds per output element and channel -- so no
// matrix instruction fits: the kernels are VALU fma and LDS-bandwidth work.  w is the fp32 master,
// rounded to bf16 as it is staged (no weight pack); every product and sum is fp32, in one fixed
// order, without atomics: two launches are bit-identical.
//
// dw_fwd / dw_dgrad (one kernel body, dw_conv_kernel): a workgroup takes one image, a block of R rows
// of its result and all channels.  It stages the weights [tap][Cs] (fp32, already rounded) and the
// input halo [rows][cols][Cs] (bf16) in LDS once; positions outside the image are ZEROS in LDS, so no
// tap branches.  dw_dgrad stages dt dilated by the stride (zeros between its pixels) and the taps
// flipped, which makes it a stride-1 correlation over that halo: the same body.  (For a strided layer
// this spends LDS and multiply-adds on the zeros; a parity-class form would not.)
// A thread owns VEC channels (8: one 16-byte LDS read; 4 when Cs == 4) of DW_PX consecutive pixels
// along x.  Per kernel row it walks each stride phase ph < s separately: the DW_PX input vectors of
// tap kx = ph stay in registers, and the step to tap kx + s shifts them by one pixel and loads ONE new
// vector -- a row of KW taps costs DW_PX + KW - s LDS reads at stride 1 instead of DW_PX * KW.  A pixel's
// chain order is ky, then ph, then kx = ph, ph + s, ...
//
// dw_wgrad: workgroup g takes the (image, row block) pairs [g * pairs_per_slab, ...), stages the x halo
// and the dt rows of each in LDS, and writes ONE slab row.  A work unit is (tap or bias, channel group,
// pixel slice): the unit sums its slice of the block's pixels in registers (pixel order) and adds the
// sum to an LDS cell that only it touches (pair order); at the end one thread per (tap, channel group)
// adds the slices' cells in slice order and stores the slab row.  Rows are laid out [tap][C] -- Keras'
// (kh, kw, C, 1) order -- then, on the next 16-byte boundary (dw_bias_off), [C]: the slab reduction takes
// both as bias-like (identity) descriptors.
#include <cstdint>
#include <stdexcept>
#include <string>

#include "args.h"
#include "bwd_through.h"

template <int VEC> struct DwVec;
template <> struct DwVec<8> {
  typedef bf16x8 T;
  __device__ __forceinline__ static T load_if(bool ok, const bf16* p, const bf16* safe) { return load_bf16x8_if(ok, p, safe); }
};
template <> struct DwVec<4> {
  typedef bf16x4 T;
  __device__ __forceinline__ static T load_if(bool ok, const bf16* p, const bf16* safe) { return load_bf16x4_if(ok, p, safe); }
};

__host__ __device__ __forceinline__ int dw_a16(int v) { return (v + 15) & ~15; }
__host__ __device__ __forceinline__ int dw_cdiv(int a, int b) { return (a + b - 1) / b; }

// the halo of a block of ``rows`` result rows: (rows, cols) in pixels
__host__ __device__ __forceinline__ void dw_halo(const DwArgs& a, int kind, int rows, int& hr, int& hc) {
  if (kind == DW_FWD) {
    hr = (rows - 1) * a.stride + a.KH;
    hc = (dw_cdiv(a.Wo, DW_PX) * DW_PX - 1) * a.stride + a.KW;
  } else if (kind == DW_DGRAD) {
    hr = rows + a.KH - 1;
    hc = dw_cdiv(a.W, DW_PX) * DW_PX - 1 + a.KW;
  } else {
    hr = (rows - 1) * a.stride + a.KH;
    hc = (a.Wo - 1) * a.stride + a.KW;
  }
}

// the channel stride of out / dt
__host__ __device__ __forceinline__ int dw_cs_out(const DwArgs& a) { return a.Cs_out ? a.Cs_out : a.Cs; }

// where the bias gradient starts in a slab row: behind the [tap][C] sums, on a 16-byte boundary
__host__ __device__ __forceinline__ int dw_bias_off(const DwArgs& a) { return (a.KH * a.KW * a.C + 3) & ~3; }

// wgrad work units: items = (taps + bias) * channel groups, each cut into nsl pixel slices
__host__ __device__ __forceinline__ void dw_units(const DwArgs& a, int& items, int& nsl) {
  const int vec = a.Cs == 4 ? 4 : 8;
  items = (a.KH * a.KW + (a.has_bias ? 1 : 0)) * (a.Cs / vec);
  nsl = DW_THREADS / items > 1 ? DW_THREADS / items : 1;
}

// Stage the halo of one block: pixel (r, c) of it is source pixel (y, x) = (r + oy, c + ox) of the
// grid [SH, SW], taken at (y / dil, x / dil) of ``src`` [.., sh, sw, scs] (its first Cs channels) where
// both divisions are exact; zeros elsewhere.
template <int VEC>
__device__ __forceinline__ void dw_stage(bf16* dst, const bf16* src, int scs, int hr, int hc, int Cs, int oy, int ox,
                                         int dil, int sh, int sw) {
  typedef typename DwVec<VEC>::T V;
  const int ncg = Cs / VEC;
  staged_copy<4, V>(
      hr * hc * ncg, (int)threadIdx.x, DW_THREADS,
      [&](int i) {
        const int t = i / ncg, cg = i - t * ncg;
        const int r = t / hc, c = t - r * hc;
        const int y = r + oy, x = c + ox;
        int sy = y, sx = x;
        bool ok = y >= 0 && x >= 0;
        if (dil > 1) {
          sy = y / dil, sx = x / dil;
          ok = ok && sy * dil == y && sx * dil == x;
        }
        ok = ok && sy < sh && sx < sw;
        return DwVec<VEC>::load_if(ok, src + ((size_t)sy * sw + sx) * scs + cg * VEC, src);
      },
      [&](int i, const V& v) { *reinterpret_cast<V*>(dst + (size_t)i * VEC) = v; });
}

template <int VEC, int KIND>
__global__ __launch_bounds__(DW_THREADS) void dw_conv_kernel(const DwArgs a) {
  typedef typename DwVec<VEC>::T V;
  extern __shared__ __attribute__((aligned(16))) unsigned char dw_smem[];
  const int ntaps = a.KH * a.KW, Cs = a.Cs, ncg = Cs / VEC, Cso = dw_cs_out(a);
  float* wl = reinterpret_cast<float*>(dw_smem);
  bf16* hx = reinterpret_cast<bf16*>(dw_smem + dw_a16(ntaps * Cs * 4));
  const int nrows = KIND == DW_FWD ? a.Ho : a.H, ncols = KIND == DW_FWD ? a.Wo : a.W;
  const int nrb = dw_cdiv(nrows, a.R);
  const int b = blockIdx.x / nrb, r0 = (blockIdx.x - b * nrb) * a.R;
  const int Rv = min(a.R, nrows - r0);
  const int s = KIND == DW_FWD ? a.stride : 1;
  int hr, hc;
  dw_halo(a, KIND, Rv, hr, hc);
  // the weights, rounded to bf16 (dgrad: the taps flipped); zeros in the padding lanes
  for (int i = threadIdx.x; i < ntaps * Cs; i += DW_THREADS) {
    const int tap = i / Cs, c = i - tap * Cs;
    const int src = KIND == DW_FWD ? tap : ntaps - 1 - tap;
    wl[i] = c < a.C ? bf2f(f2bf(a.w[src * a.C + c])) : 0.f;
  }
  if (KIND == DW_FWD)
    dw_stage<VEC>(hx, a.x + (size_t)b * a.H * a.W * Cs, Cs, hr, hc, Cs, r0 * s - a.pad_t, -a.pad_l, 1, a.H, a.W);
  else
    dw_stage<VEC>(hx, a.dt + (size_t)b * a.Ho * a.Wo * Cso, Cso, hr, hc, Cs, r0 + a.pad_t - (a.KH - 1),
                  a.pad_l - (a.KW - 1), a.stride, a.Ho, a.Wo);
  __syncthreads();
  const uint32_t step = a.st ? (uint32_t)a.st->t : 0u;
  const int nruns = dw_cdiv(ncols, DW_PX), items = Rv * nruns * ncg;
  const int nph = min(s, a.KW);
  for (int it = threadIdx.x; it < items; it += DW_THREADS) {
    const int t = it / ncg, c0 = (it - t * ncg) * VEC;
    const int r = t / nruns, x0 = (t - r * nruns) * DW_PX;
    float acc[DW_PX][VEC];
#pragma unroll
    for (int p = 0; p < DW_PX; ++p)
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc[p][k] = 0.f;
    for (int ky = 0; ky < a.KH; ++ky) {
      const bf16* rowp = hx + (size_t)(r * s + ky) * hc * Cs + c0;
      const float* wrow = wl + ky * a.KW * Cs + c0;
      for (int ph = 0; ph < nph; ++ph) {
        V v[DW_PX];
#pragma unroll
        for (int p = 0; p < DW_PX; ++p) v[p] = *reinterpret_cast<const V*>(rowp + ((x0 + p) * s + ph) * Cs);
        for (int kx = ph; kx < a.KW; kx += s) {
          float wv[VEC];
#pragma unroll
          for (int k = 0; k < VEC; k += 4) {
            const f32x4 q = *reinterpret_cast<const f32x4*>(wrow + kx * Cs + k);
            wv[k] = q[0], wv[k + 1] = q[1], wv[k + 2] = q[2], wv[k + 3] = q[3];
          }
#pragma unroll
          for (int p = 0; p < DW_PX; ++p)
#pragma unroll
            for (int k = 0; k < VEC; ++k) acc[p][k] = fmaf(bf2f(v[p][k]), wv[k], acc[p][k]);
          if (kx + s < a.KW) {
#pragma unroll
            for (int p = 0; p + 1 < DW_PX; ++p) v[p] = v[p + 1];
            v[DW_PX - 1] = *reinterpret_cast<const V*>(rowp + ((x0 + DW_PX - 1) * s + kx + s) * Cs);
          }
        }
      }
    }
    const int y = r0 + r;
    if (KIND == DW_FWD) {
      float bv[VEC];
#pragma unroll
      for (int k = 0; k < VEC; ++k) bv[k] = (a.bias && c0 + k < a.C) ? a.bias[c0 + k] : 0.f;
#pragma unroll
      for (int p = 0; p < DW_PX; ++p) {
        if (x0 + p >= ncols) continue;
        V o;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          float f = acc[p][k] + bv[k];
          if (a.relu) f = fmaxf(f, 0.f);
          if (c0 + k >= a.C) f = 0.f;
          o[k] = f2bf(f);
        }
        bf16* dst = a.out + (((size_t)b * a.Ho + y) * a.Wo + x0 + p) * Cso + c0;
        *reinterpret_cast<V*>(dst) = o;
        if (VEC == 4 && Cso == 8) {      // (a 4-lane input stored with 8 lanes: the upper four are padding)
#pragma unroll
          for (int k = 0; k < VEC; ++k) o[k] = f2bf(0.f);
          *reinterpret_cast<V*>(dst + 4) = o;
        }
      }
    } else {
#pragma unroll
      for (int p = 0; p < DW_PX; ++p) {
        if (x0 + p >= ncols) continue;
        if (VEC == 8) {
          bwd_through_store8(a.bt, ((size_t)b * a.H + y) * a.W + x0 + p, c0, acc[p], step);
        } else {
#pragma unroll
          for (int k = 0; k < VEC; ++k) bwd_through_store(a.bt, b, y, x0 + p, c0 + k, acc[p][k], step);
        }
      }
    }
  }
}

template <int VEC>
__global__ __launch_bounds__(DW_THREADS) void dw_wgrad_kernel(const DwArgs a) {
  typedef typename DwVec<VEC>::T V;
  extern __shared__ __attribute__((aligned(16))) unsigned char dw_smem[];
  const int ntaps = a.KH * a.KW, Cs = a.Cs, ncg = Cs / VEC, s = a.stride, Cso = dw_cs_out(a);
  int items, nsl;
  dw_units(a, items, nsl);
  const int U = items * nsl;
  int hr_max, hc;
  dw_halo(a, DW_WGRAD, a.R, hr_max, hc);
  float* accl = reinterpret_cast<float*>(dw_smem);                            // [U][VEC], cell u owned by unit u
  bf16* hx = reinterpret_cast<bf16*>(dw_smem + dw_a16(U * VEC * 4));          // [hr][hc][Cs]
  bf16* hd = hx + (size_t)hr_max * hc * Cs;                                   // [R][Wo][Cs]
  for (int i = threadIdx.x; i < U * VEC; i += DW_THREADS) accl[i] = 0.f;
  const int nrb = dw_cdiv(a.Ho, a.R);
  const long long npairs = (long long)a.B * nrb;
  const long long p_lo = (long long)blockIdx.x * a.pairs_per_slab;
  const long long p_hi = min(p_lo + a.pairs_per_slab, npairs);
  for (long long pr = p_lo; pr < p_hi; ++pr) {
    const int b = (int)(pr / nrb), r0 = (int)(pr - (long long)b * nrb) * a.R;
    const int Rv = min(a.R, a.Ho - r0);
    int hr, hcc;
    dw_halo(a, DW_WGRAD, Rv, hr, hcc);
    __syncthreads();      // (the previous pair's readers are done; the first pass: accl is zero)
    dw_stage<VEC>(hx, a.x + (size_t)b * a.H * a.W * Cs, Cs, hr, hc, Cs, r0 * s - a.pad_t, -a.pad_l, 1, a.H, a.W);
    dw_stage<VEC>(hd, a.dt + ((size_t)b * a.Ho + r0) * a.Wo * Cso, Cso, Rv, a.Wo, Cs, 0, 0, 1, Rv, a.Wo);
    __syncthreads();
    const int npix = Rv * a.Wo;
    for (int u = threadIdx.x; u < U; u += DW_THREADS) {
      const int sl = u / items, item = u - sl * items;
      const int tap = item / ncg, c0 = (item - tap * ncg) * VEC;
      const int ky = tap / a.KW, kx = tap - ky * a.KW;
      const bool is_bias = tap == ntaps;
      float acc[VEC];
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
      for (int pix = sl; pix < npix; pix += nsl) {
        const int y = pix / a.Wo, x = pix - y * a.Wo;
        const V d = *reinterpret_cast<const V*>(hd + (size_t)pix * Cs + c0);
        // (the bias unit: any in-range address; its x value is replaced by 1)
        const V xv = *reinterpret_cast<const V*>(hx + ((size_t)(is_bias ? 0 : (y * s + ky) * hc + x * s + kx)) * Cs + c0);
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] = fmaf(is_bias ? 1.f : bf2f(xv[k]), bf2f(d[k]), acc[k]);
      }
#pragma unroll
      for (int k = 0; k < VEC; ++k) accl[u * VEC + k] += acc[k];
    }
  }
  __syncthreads();
  float* row = a.slab + (size_t)blockIdx.x * a.slab_ld;
  for (int item = threadIdx.x; item < items; item += DW_THREADS) {
    const int tap = item / ncg, c0 = (item - tap * ncg) * VEC;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      float sum = accl[item * VEC + k];
      for (int sl = 1; sl < nsl; ++sl) sum += accl[(sl * items + item) * VEC + k];
      if (c0 + k < a.C) row[(tap == ntaps ? dw_bias_off(a) : tap * a.C) + c0 + k] = sum;
    }
  }
}

// ---------------------------------------------------------------------------------------------------
size_t dw_lds_bytes(const DwArgs& a, int kind, int R) {
  int hr, hc;
  dw_halo(a, kind, R, hr, hc);
  const size_t halo = (size_t)hr * hc * a.Cs * 2;
  if (kind == DW_WGRAD) {
    int items, nsl;
    dw_units(a, items, nsl);
    return dw_a16(items * nsl * (a.Cs == 4 ? 4 : 8) * 4) + halo + (size_t)R * a.Wo * a.Cs * 2;
  }
  return dw_a16(a.KH * a.KW * a.Cs * 4) + halo;
}

static void dw_check_geometry(const DwArgs& a, const std::string& w) {
  if (a.depth_multiplier != 1) throw std::invalid_argument(w + ": depth_multiplier must be 1");
  if (a.Cs != 4 && (a.Cs <= 0 || a.Cs % 8 || a.Cs > 2048))
    throw std::invalid_argument(w + ": the channel stride must be 4 or a multiple of 8 (at most 2048)");
  if (a.Cs_out && a.Cs_out != a.Cs && !(a.Cs == 4 && a.Cs_out == 8))
    throw std::invalid_argument(w + ": the output's channel stride must be the input's (or 8 behind a 4-lane input)");
  if (a.C <= 0 || a.C > a.Cs) throw std::invalid_argument(w + ": channels must be in [1, Cs]");
  if (a.B < 0 || a.H <= 0 || a.W <= 0 || a.Ho <= 0 || a.Wo <= 0) throw std::invalid_argument(w + ": batch / grid sizes");
  if (a.KH <= 0 || a.KW <= 0 || a.KH * a.KW > 1024 || a.stride <= 0)
    throw std::invalid_argument(w + ": kernel size / stride");
  if (a.pad_t < 0 || a.pad_l < 0 || a.pad_t >= a.KH || a.pad_l >= a.KW)
    throw std::invalid_argument(w + ": the top / left padding must be smaller than the kernel");
  if ((long long)(a.Ho - 1) * a.stride - a.pad_t >= a.H || (long long)(a.Wo - 1) * a.stride - a.pad_l >= a.W)
    throw std::invalid_argument(w + ": the output grid does not belong to the input grid");
  if ((long long)a.H * a.W * a.Cs > 0x7fffffffLL || (long long)a.Ho * a.Wo * dw_cs_out(a) > 0x7fffffffLL)
    throw std::invalid_argument(w + ": one image must stay below 2^31 elements");
}

// Rows per block: the fewest row blocks per image (balanced: each cdiv(rows, blocks) rows) whose LDS
// stage fits DW_LDS_BUDGET and that leave at least ``want`` workgroups; 1 where nothing gives that
// many; 0 where not even one row fits.
int dw_rows(const DwArgs& a, int kind, int want) {
  dw_check_geometry(a, "dw_rows");
  if (kind != DW_FWD && kind != DW_DGRAD && kind != DW_WGRAD) throw std::invalid_argument("dw_rows: kind");
  const int nrows = kind == DW_DGRAD ? a.H : a.Ho;
  if (dw_lds_bytes(a, kind, 1) > DW_LDS_BUDGET) return 0;
  for (int c = 1; c <= nrows; ++c) {
    const int R = dw_cdiv(nrows, c);
    if (dw_lds_bytes(a, kind, R) > DW_LDS_BUDGET) continue;
    if ((long long)a.B * dw_cdiv(nrows, R) < want) continue;
    return R;
  }
  return 1;
}

static bool dw_bad_ptr(const void* p, int Cs) { return !p || (reinterpret_cast<uintptr_t>(p) & (Cs == 4 ? 7 : 15)); }

static unsigned dw_check(const DwArgs& a, int kind, const std::string& w) {
  dw_check_geometry(a, w);
  const int nrows = kind == DW_DGRAD ? a.H : a.Ho;
  if (a.R <= 0 || a.R > nrows) throw std::invalid_argument(w + ": rows per block must be in [1, rows]");
  if (dw_lds_bytes(a, kind, a.R) > DW_LDS_BUDGET)
    throw std::invalid_argument(w + ": the block's LDS stage exceeds " + std::to_string(DW_LDS_BUDGET) + " bytes");
  if (!a.w || (reinterpret_cast<uintptr_t>(a.w) & 3)) throw std::invalid_argument(w + ": weight pointer");
  const long long blocks = (long long)a.B * dw_cdiv(nrows, a.R);
  if (blocks > 0x7fffffffLL) throw std::invalid_argument(w + ": too many blocks for one launch");
  return (unsigned)blocks;
}

void launch_dw_fwd(const DwArgs& a, hipStream_t s) {
  const std::string w("dw_fwd");
  const unsigned blocks = dw_check(a, DW_FWD, w);
  if (dw_bad_ptr(a.x, a.Cs)) throw std::invalid_argument(w + ": input pointer (null or misaligned)");
  if (dw_bad_ptr(a.out, a.Cs)) throw std::invalid_argument(w + ": output pointer (null or misaligned)");
  if (a.bias && (reinterpret_cast<uintptr_t>(a.bias) & 3)) throw std::invalid_argument(w + ": bias pointer");
  if (!blocks) return;
  const size_t lds = dw_lds_bytes(a, DW_FWD, a.R);
  if (a.Cs == 4) hipLaunchKernelGGL((dw_conv_kernel<4, DW_FWD>), dim3(blocks), dim3(DW_THREADS), lds, s, a);
  else hipLaunchKernelGGL((dw_conv_kernel<8, DW_FWD>), dim3(blocks), dim3(DW_THREADS), lds, s, a);
}

void launch_dw_dgrad(const DwArgs& a, hipStream_t s) {
  const std::string w("dw_dgrad");
  const unsigned blocks = dw_check(a, DW_DGRAD, w);
  if (dw_bad_ptr(a.dt, a.Cs)) throw std::invalid_argument(w + ": gradient pointer (null or misaligned)");
  const BwdThrough& t = a.bt;
  if (t.pH != a.H || t.pW != a.W || t.pC != a.C || t.pCs != a.Cs)
    throw std::invalid_argument(w + ": the feeding stage's BwdThrough geometry differs from the input grid");
  if (dw_bad_ptr(t.dy, a.Cs)) throw std::invalid_argument(w + ": BwdThrough dy (null or misaligned)");
  if (t.prev_relu && dw_bad_ptr(t.prev_out, a.Cs)) throw std::invalid_argument(w + ": BwdThrough prev_out (null or misaligned)");
  if (t.wt && (a.Cs == 4 || (long long)a.B * a.H * a.W * a.Cs * 2 >= (1LL << 31)))
    throw std::invalid_argument(w + ": write-through stores need Cs % 8 == 0 and a gradient buffer below 2 GB");
  if (t.drop_thr && !(t.drop_scale >= 1.f)) throw std::invalid_argument(w + ": BwdThrough dropout scale");
  if (!blocks) return;
  const size_t lds = dw_lds_bytes(a, DW_DGRAD, a.R);
  if (a.Cs == 4) hipLaunchKernelGGL((dw_conv_kernel<4, DW_DGRAD>), dim3(blocks), dim3(DW_THREADS), lds, s, a);
  else hipLaunchKernelGGL((dw_conv_kernel<8, DW_DGRAD>), dim3(blocks), dim3(DW_THREADS), lds, s, a);
}

void launch_dw_wgrad(const DwArgs& a, hipStream_t s) {
  const std::string w("dw_wgrad");
  const unsigned blocks = dw_check(a, DW_WGRAD, w);
  if (dw_bad_ptr(a.x, a.Cs)) throw std::invalid_argument(w + ": input pointer (null or misaligned)");
  if (dw_bad_ptr(a.dt, a.Cs)) throw std::invalid_argument(w + ": gradient pointer (null or misaligned)");
  if (!a.slab || (reinterpret_cast<uintptr_t>(a.slab) & 3)) throw std::invalid_argument(w + ": slab pointer");
  if (a.slab_ld < (a.has_bias ? dw_bias_off(a) + a.C : a.KH * a.KW * a.C)) throw std::invalid_argument(w + ": slab row stride");
  if (!blocks) {
    if (a.S) throw std::invalid_argument(w + ": slabs of an empty batch");
    return;
  }
  if (a.S <= 0 || a.pairs_per_slab <= 0 || (long long)a.S * a.pairs_per_slab < blocks ||
      (long long)(a.S - 1) * a.pairs_per_slab >= blocks)
    throw std::invalid_argument(w + ": S slabs of pairs_per_slab (image, row block) pairs must cover the pairs, none empty");
  const size_t lds = dw_lds_bytes(a, DW_WGRAD, a.R);
  if (a.Cs == 4) hipLaunchKernelGGL(dw_wgrad_kernel<4>, dim3(a.S), dim3(DW_THREADS), lds, s, a);
  else hipLaunchKernelGGL(dw_wgrad_kernel<8>, dim3(a.S), dim3(DW_THREADS), lds, s, a);
}

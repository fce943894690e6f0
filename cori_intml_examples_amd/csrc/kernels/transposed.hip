// Transposed convolution (Keras Conv2DTranspose, isotropic strides s in 1..4): forward, the gradient to
// its input, the weight and bias gradient (TconvArgs, args.h).  The kernel is w[ky][kx][n][c], OUTPUT
// channels n before input channels c, so c is the contiguous axis.
//
//   tconv_fwd    z[b, Y, X, n]  = bias[n] + sum over (i, ky), (j, kx), c with Y = i*s + ky - pad_t, X = j*s + kx - pad_l
//                                 of x[b, i, j, c] * w[ky, kx, n, c];  out = bf16(A(z))
//   tconv_dgrad  dx[b, i, j, c] = sum_{ky, kx, n} dt[b, i*s + ky - pad_t, j*s + kx - pad_l, n] * w[ky, kx, n, c]
//                handed to the feeding stage's BwdThrough (its dropout mask, relu mask and bf16 rounding)
//   tconv_wgrad  dW[ky, kx, n, c] = sum_{b, i, j} x[b, i, j, c] * dt[b, i*s + ky - pad_t, j*s + kx - pad_l, n]
//                db[n]            = sum_{b, Y, X} dt[b, Y, X, n]
//
// All three are implicit GEMMs on v_mfma_f32_16x16x32_bf16 over blocks of R INPUT rows.  w is the fp32
// master, rounded to bf16 as it is staged into LDS (no weight pack); accumulation is fp32 in one fixed
// order, without atomics: two launches are bit-identical.
//
// tconv_fwd, by output parity class.  With Yf = Y + pad_t, Xf = X + pad_l, an output pixel lies on the base
// grid at (q, p) = (Yf / s, Xf / s) in class (py, px) = (Yf % s, Xf % s), and sees only the taps
// ky = py + m*s, kx = px + n*s, of input pixel (q - m, p - n): each class is a dense stride-1 convolution
// with at most ty x tw = ceil(KH / s) x ceil(KW / s) taps, and the stride's zeros are never multiplied.  A
// workgroup takes one image, R rows of the base grid (the last block: also the ceil((Ho + pad_t) / s) - H
// border rows a kernel larger than the stride adds) and ntw n-tiles of Cout.  It stages the block's input
// rows and the ty - 1 rows above them ONCE ([rows][qw + tw - 1][xpix], zeros outside the input), then for
// each of the s*s classes: the class's halo offset table, the class's weights, M = the block's base pixels,
// K = (taps of the class) x Cin, and the epilogue stores pixel (q*s + py - pad_t, p*s + px - pad_l) where
// that lies inside the output.  A class without taps (k < s) has no k-steps: its outputs are A(bias).
//
// tconv_dgrad, a strided gather.  M = the block's input pixels, K = KH*KW x Cout, N = Cin.  It stages
// (R - 1)*s + KH rows x (W - 1)*s + KW columns of dt (zeros outside the output grid); tap (ky, kx) of
// pixel (r, j) is staged pixel (r*s + ky, j*s + kx).
//
// Both share one body (tconv_conv_kernel): [offset table][weight chunk][staged image] in LDS; one table
// entry per 8 consecutive k (one tap, 8 channels: a lane's fragment is ONE 16-byte read; 4-lane inputs: per
// 4 k, two 8-byte reads), the k padding pointing at the pixel itself with zero weights.  Weights are staged
// in fragment order [(ks, nt)][lane][8] in 8-element (4-element) vectors, one index decomposition per
// vector: the forward's vector is 8 consecutive c of one (tap, n) -- contiguous floats -- and the dgrad's
// is 8 consecutive n of one c, with the 16 lanes of a fragment row on 16 consecutive c.  K is walked in
// chunks of kc k-steps when a class's slice does not fit.  The MFMA runs transposed (weights as the A
// operand): a lane holds 4 consecutive channels of one pixel, one exchange with lane ^ 16 makes 8, and the
// even 16-lane groups store 16 bytes.  A wave keeps TC_MTW m-tiles x ntw n-tiles; larger blocks take passes.
//
// tconv_wgrad: M = (tap, n), N = c, K = pixels, so that a tile's columns are the contiguous axis of dW.
// Workgroup (g, my, nz) takes the (image, row block) pairs [g * pairs_per_slab, ...), stages of each pair
// (R - 1)*s + max(KH, s) rows x (W - 1)*s + max(KW, s) columns of dt -- the rows and columns the block OWNS
// (a partition of the output grid) besides the ones its taps reach -- and the block's x pixels ([pixel]
// [channel], zero rows up to a multiple of 32 pixels, zero columns up to a multiple of 16 channels).  Both
// operands need k = pixel runs per lane out of [pixel][channel] tiles: transposed LDS reads
// (ds_read_b64_tr_b16), the A operand at the lane's pixel (r*s, j*s) shifted by its row group's tap.  The
// bias gradient sums the owned dt pixels, contiguous in the staged image, with an all-ones B fragment:
// 16-channel tile (4 my + wave) * 4 + k, k < 4, in the waves of nz == 0.  One slab row per workgroup group:
// [KH][KW][Cout][Cin] (Keras order, unpadded), then on the next 16-byte boundary [Cout]; the slab reduction
// takes both as identity descriptors.
#include <cstdint>
#include <stdexcept>
#include <string>
#include <tuple>

#include "args.h"
#include "bwd_through.h"

template <int VEC> struct TcVec;
template <> struct TcVec<8> {
  typedef bf16x8 T;
  __device__ __forceinline__ static T load_if(bool ok, const bf16* p, const bf16* safe) { return load_bf16x8_if(ok, p, safe); }
};
template <> struct TcVec<4> {
  typedef bf16x4 T;
  __device__ __forceinline__ static T load_if(bool ok, const bf16* p, const bf16* safe) { return load_bf16x4_if(ok, p, safe); }
};

__host__ __device__ __forceinline__ int tc_a16(int v) { return (v + 15) & ~15; }
__host__ __device__ __forceinline__ int tc_cdiv(int a, int b) { return (a + b - 1) / b; }
__host__ __device__ __forceinline__ int tc_max(int a, int b) { return a > b ? a : b; }

// What a launch kind stages and produces: ``ck`` the staged image's channel stride, (ty, tw) the taps per
// axis it reaches back over (fwd: of the largest class; wgrad: at least the stride, the owned pixels),
// (qh, qw) the grid its m (fwd, dgrad) pixels run over, ``hc`` the staged columns, n / ns the result
// channels and their stride.
struct TcGeo {
  int ck, ty, tw, qh, qw, hc, n, ns;
};
__host__ __device__ __forceinline__ TcGeo tc_geo(const TconvArgs& a, int kind) {
  TcGeo g;
  const int s = a.stride;
  if (kind == TC_FWD) {
    g.ck = a.Cs_in, g.ty = tc_cdiv(a.KH, s), g.tw = tc_cdiv(a.KW, s);
    g.qh = tc_cdiv(a.Ho + a.pad_t, s), g.qw = tc_cdiv(a.Wo + a.pad_l, s);
    g.hc = g.qw + g.tw - 1, g.n = a.Cout, g.ns = a.Cs_out;
  } else {
    const bool wg = kind == TC_WGRAD;
    g.ck = a.Cs_out, g.ty = wg ? tc_max(a.KH, s) : a.KH, g.tw = wg ? tc_max(a.KW, s) : a.KW;
    g.qh = a.H, g.qw = a.W, g.hc = (a.W - 1) * s + g.tw, g.n = a.Cin, g.ns = a.Cs_in;
  }
  return g;
}
// staged rows of a block of R input rows (fwd: of the last block, the largest)
__host__ __device__ __forceinline__ int tc_rows(const TconvArgs& a, int kind, const TcGeo& G, int R) {
  return kind == TC_FWD ? R + (G.qh - a.H) + G.ty - 1 : (R - 1) * a.stride + G.ty;
}
// k-steps of the forward's largest class / of the dgrad
__host__ __device__ __forceinline__ int tc_ks(const TcGeo& G) { return tc_cdiv(G.ty * G.tw * G.ck, 32); }
// elements of a staged image, to a 16-byte boundary
__host__ __device__ __forceinline__ size_t tc_halo_elems(int hr, int hc, int xpix) { return ((size_t)hr * hc * xpix + 7) & ~(size_t)7; }
// tconv_wgrad's staged x pixels: all n-tiles' columns defined (zeros behind Cs_in), 16 bytes of padding
__host__ __device__ __forceinline__ int tc_xb(const TconvArgs& a) { return tc_a16(a.Cs_in) + 8; }
__host__ __device__ __forceinline__ int tc_bias_off(const TconvArgs& a) { return (a.KH * a.KW * a.Cin * a.Cout + 3) & ~3; }

// Stage hr * hc pixels: pixel (r, c) is source pixel (r + oy, c + ox) of [sh, sw, scs], its first ``ncg``
// VEC-channel groups (groups >= src_ncg and pixels outside the grid: zeros), at dst + pixel * dpix.
template <int VEC>
__device__ __forceinline__ void tc_stage(bf16* dst, int dpix, const bf16* src, int scs, int hr, int hc, int ncg, int src_ncg,
                                         int oy, int ox, int sh, int sw) {
  typedef typename TcVec<VEC>::T V;
  staged_copy<4, V>(
      hr * hc * ncg, (int)threadIdx.x, TC_THREADS,
      [&](int i) {
        const int t = i / ncg, cg = i - t * ncg;
        const int r = t / hc, c = t - r * hc;
        const int y = r + oy, x = c + ox;
        const bool ok = y >= 0 && x >= 0 && y < sh && x < sw && cg < src_ncg;
        return TcVec<VEC>::load_if(ok, src + ((size_t)y * sw + x) * scs + cg * VEC, src);
      },
      [&](int i, const V& v) {
        const int t = i / ncg, cg = i - t * ncg;
        *reinterpret_cast<V*>(dst + (size_t)t * dpix + cg * VEC) = v;
      });
}

// The launch's arguments, re-read from the kernel-argument segment (TconvArgs is the kernels' ONE by-value
// argument: offset 0).  A phase that starts from this pointer, which the compiler cannot see through, takes
// its fields as scalar loads of its own, not as scalar registers held live across the whole kernel (which
// spilled up to 27 of them).
__device__ __forceinline__ const TconvArgs& tc_args() {
  typedef const __attribute__((address_space(4))) TconvArgs* KP;
  KP p = (KP)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return *(const TconvArgs*)p;
}

template <bool CS4, int NTW, int KIND>
__global__ __launch_bounds__(TC_THREADS) void tconv_conv_kernel(const TconvArgs a0) {
  constexpr int VEC = CS4 ? 4 : 8, NV = 8 / VEC;
  constexpr bool FWD = KIND == TC_FWD;
  typedef typename TcVec<VEC>::T V;
  extern __shared__ __attribute__((aligned(16))) unsigned char tc_smem[];
  int* toff = reinterpret_cast<int*>(tc_smem);
  bf16 *wl, *hx;
  int b, r0, Rv, npix, ncls;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 15, g = lane >> 4;
  const int nbase = blockIdx.y * NTW * 16;
  {
  const TconvArgs& a = a0;
  const TcGeo G = tc_geo(a, KIND);
  const int s = a.stride, ck = G.ck, hc = G.hc;
  wl = reinterpret_cast<bf16*>(tc_smem + tc_a16(tc_ks(G) * 4 * NV * 4));
  hx = wl + (size_t)a.kc * NTW * 512;
  const int nrb = tc_cdiv(a.H, a.R), rb = blockIdx.x % nrb;
  b = blockIdx.x / nrb, r0 = rb * a.R;
  Rv = rb == nrb - 1 ? G.qh - r0 : a.R;      // (fwd: the last block takes the border rows)
  npix = Rv * G.qw, ncls = FWD ? s * s : 1;
  if (FWD)
    tc_stage<VEC>(hx, a.xpix, a.x + (size_t)b * a.H * a.W * a.Cs_in, a.Cs_in, Rv + G.ty - 1, hc, ck / VEC, ck / VEC,
                  r0 - (G.ty - 1), -(G.tw - 1), a.H, a.W);
  else
    tc_stage<VEC>(hx, a.xpix, a.dt + (size_t)b * a.Ho * a.Wo * a.Cs_out, a.Cs_out, (Rv - 1) * s + G.ty, hc, ck / VEC, ck / VEC,
                  r0 * s - a.pad_t, -a.pad_l, a.Ho, a.Wo);
  }
  // (every phase below re-reads the arguments it needs: tc_args)
  const int nmt = tc_cdiv(npix, 16);
  for (int cls = 0; cls < ncls; ++cls) {
    const TconvArgs& a = tc_args();
    const TcGeo G = tc_geo(a, KIND);
    const int s = a.stride, ck = G.ck, hc = G.hc;
    // the class's taps: ky = py + m * s, m < nty, kx = px + n * s, n < ntx (the dgrad: every tap)
    const int py = cls / s, px = cls - py * s;
    const int nty = FWD ? (py < a.KH ? tc_cdiv(a.KH - py, s) : 0) : a.KH;
    const int ntx = FWD ? (px < a.KW ? tc_cdiv(a.KW - px, s) : 0) : a.KW;
    const int ntc = nty * ntx, KS = tc_cdiv(ntc * ck, 32), nq = KS * 4 * NV;
    const int nchunks = tc_cdiv(KS, a.kc);
    __syncthreads();      // (the previous class's readers are done)
    // the staged offset of every VEC consecutive k, relative to the m pixel: the forward reaches BACK m rows
    // and n columns, the dgrad forward by the tap; the k padding: offset 0
    for (int q = tid; q < nq; q += TC_THREADS) {
      const int k0 = q * VEC, t = k0 / ck, m = t / ntx, n = t - m * ntx;
      toff[q] = t < ntc ? (FWD ? -(m * hc + n) : m * hc + n) * a.xpix + (k0 - t * ck) : 0;
    }
    for (int mt0 = 0; mt0 < nmt; mt0 += 4 * TC_MTW) {
      f32x4 acc[TC_MTW][NTW];
      int pixoff[TC_MTW], opix[TC_MTW];
#pragma unroll
      for (int u = 0; u < TC_MTW; ++u) {
        const TconvArgs& a = tc_args();
        const TcGeo G = tc_geo(a, KIND);
        const int s = a.stride, hc = G.hc;
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) acc[u][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
        int p = (mt0 + wave + 4 * u) * 16 + i;
        const bool in = p < npix;
        if (!in) p = 0;      // (a tail lane: any pixel of the block; its results are not stored)
        const int r = p / G.qw, c = p - r * G.qw;
        if (FWD) {
          pixoff[u] = ((r + G.ty - 1) * hc + c + G.tw - 1) * a.xpix;
          const int Y = (r0 + r) * s + py - a.pad_t, X = c * s + px - a.pad_l;
          opix[u] = in && Y >= 0 && X >= 0 && Y < a.Ho && X < a.Wo ? Y * a.Wo + X : -1;
        } else {
          pixoff[u] = (r * s * hc + c * s) * a.xpix;
          opix[u] = in ? r0 * a.W + p : -1;      // (a block's pixels are consecutive in the image)
        }
      }
      for (int ch = 0; ch < nchunks; ++ch) {
        const int kc = tc_args().kc, ks0 = ch * kc, kcn = min(kc, KS - ks0);
        if (nchunks > 1 || mt0 == 0) {
          __syncthreads();      // (the previous chunk's readers are done)
          // the weight chunk in fragment order, rounded to bf16: element j of lane (i, g) of (ks, nt) is
          // W[k = 32 ks + 8 g + j][n = nbase + 16 nt + i], zeros in the k and n padding; one vector of VEC
          // elements per thread and turn.  Thread order follows the master's contiguous axis c: the k groups
          // of one n for the forward, the 16 n (= c) of one k group for the dgrad.
          const TconvArgs& wa = tc_args();
          const int s = wa.stride, ck = FWD ? wa.Cs_in : wa.Cs_out, gn = FWD ? wa.Cout : wa.Cin;
          for (int e = tid; e < kcn * NTW * 64 * NV; e += TC_THREADS) {
            const int h = e & (NV - 1), f = e / NV, t = f >> 6;
            const int eg = FWD ? f & 3 : (f >> 4) & 3, ei = FWD ? (f >> 2) & 15 : f & 15;
            const int ksl = t / NTW, nt = t - ksl * NTW;
            const int k0 = (ks0 + ksl) * 32 + 8 * eg + h * VEC, n = nbase + nt * 16 + ei;
            const int tap = k0 / ck, c0 = k0 - tap * ck;
            V v;
#pragma unroll
            for (int j = 0; j < VEC; ++j) v[j] = f2bf(0.f);
            if (tap < ntc && n < gn) {
              const int m = tap / ntx, nn = tap - m * ntx;
              if (FWD) {
                const float* wp = wa.w + ((size_t)((py + m * s) * wa.KW + px + nn * s) * wa.Cout + n) * wa.Cin + c0;
#pragma unroll
                for (int j = 0; j < VEC; ++j)
                  if (c0 + j < wa.Cin) v[j] = f2bf(wp[j]);
              } else {
                const float* wp = wa.w + ((size_t)tap * wa.Cout + c0) * wa.Cin + n;
#pragma unroll
                for (int j = 0; j < VEC; ++j)
                  if (c0 + j < wa.Cout) v[j] = f2bf(wp[(size_t)j * wa.Cin]);
              }
            }
            *reinterpret_cast<V*>(wl + ((size_t)t * 64 + eg * 16 + ei) * 8 + h * VEC) = v;
          }
          __syncthreads();      // (first chunk: the table and the staged image too)
        }
        for (int ksl = 0; ksl < kcn; ++ksl) {
          bf16x8 wfr[NTW];
#pragma unroll
          for (int nt = 0; nt < NTW; ++nt) wfr[nt] = *reinterpret_cast<const bf16x8*>(wl + ((size_t)(ksl * NTW + nt) * 64 + lane) * 8);
          const int q = (ks0 + ksl) * 4 + g;
          int o0, o1 = 0;
          if (CS4) o0 = toff[2 * q], o1 = toff[2 * q + 1];
          else o0 = toff[q];
#pragma unroll
          for (int u = 0; u < TC_MTW; ++u) {
            bf16x8 xfr;
            if (CS4) {
              const bf16x4 lo = *reinterpret_cast<const bf16x4*>(hx + pixoff[u] + o0);
              const bf16x4 hi = *reinterpret_cast<const bf16x4*>(hx + pixoff[u] + o1);
              xfr = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
            } else {
              xfr = *reinterpret_cast<const bf16x8*>(hx + pixoff[u] + o0);
            }
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt) acc[u][nt] = mfma16(wfr[nt], xfr, acc[u][nt]);
          }
        }
      }
      // epilogue: lane (i, g) holds channels n0 + j of pixel i, n0 = 16 nt + 4 g; lane ^ 16 holds the other
      // half of the 8-channel chunk, and the even groups store it
      const TconvArgs& ea = tc_args();
      const int gn = FWD ? ea.Cout : ea.Cin, gns = FWD ? ea.Cs_out : ea.Cs_in;
      const uint32_t step = ea.st ? (uint32_t)ea.st->t : 0u;
#pragma unroll
      for (int nt = 0; nt < NTW; ++nt) {
        const int n0 = nbase + nt * 16 + 4 * g;
        float bv[4];
        uint32_t keep[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const bool in = n0 + j < gn;
          bv[j] = (FWD && ea.bias) ? ea.bias[in ? n0 + j : 0] : 0.f;
          keep[j] = in ? 0xffffffffu : 0u;
        }
#pragma unroll
        for (int u = 0; u < TC_MTW; ++u) {
          float v[8];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            float f = acc[u][nt][j];
            if (FWD) {
              f += bv[j];
              if (ea.relu) f = fmaxf(f, 0.f);
            }
            v[j] = __uint_as_float(__float_as_uint(f) & keep[j]);      // (padding channels: zeros)
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) v[4 + j] = __shfl_xor(v[j], 16);
          if ((g & 1) || opix[u] < 0 || n0 >= gns) continue;
          if (FWD) {
            bf16x8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = f2bf(v[j]);
            *reinterpret_cast<bf16x8*>(ea.out + ((size_t)b * ea.Ho * ea.Wo + opix[u]) * gns + n0) = o;
          } else {
            const size_t qi = (size_t)b * ea.H * ea.W + opix[u], o = qi * gns + n0;
            bwd_through_finish8_at<BtGeoRt, true, false>(ea.bt, qi, n0, o, v, bwd_through_fetch8_at<BtGeoRt, false>(ea.bt, o), step);
          }
        }
      }
    }
  }
}

__device__ __forceinline__ bf16x4 tc_tr_read(const bf16* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4bf16(LDS_PTR(bf16x4, p));
}

template <bool CS4, int NTW>
__global__ __launch_bounds__(TC_THREADS) void tconv_wgrad_kernel(const TconvArgs a0) {
  const TconvArgs& a = a0;
  constexpr int VEC = CS4 ? 4 : 8;
  extern __shared__ __attribute__((aligned(16))) unsigned char tc_smem[];
  const TcGeo G = tc_geo(a, TC_WGRAD);
  const int s = a.stride, cs = a.Cs_out, mtot = a.KH * a.KW * cs, hc = G.hc, xb = tc_xb(a);
  bf16* hd = reinterpret_cast<bf16*>(tc_smem);                                  // dt [rows][hc][xpix]
  bf16* hx = hd + tc_halo_elems(tc_rows(a, TC_WGRAD, G, a.R), hc, a.xpix);      // x [32-multiple of pixels][xb]
  bf16* hz = hx + (size_t)((a.R * a.W + 31) & ~31) * xb;                        // one pixel of zeros
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 15, g = lane >> 4;
  const int nbase = blockIdx.z * NTW * 16, mtb = blockIdx.y * 4 * TC_MTW + wave;
  const int ncols = tc_a16(a.Cs_in);      // the staged x columns
  for (int e = tid; e < a.xpix; e += TC_THREADS) hz[e] = f2bf(0.f);
  f32x4 acc[TC_MTW][NTW], bacc[4];
  int aoff[TC_MTW];
#pragma unroll
  for (int u = 0; u < TC_MTW; ++u) {
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt) acc[u][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    // the lane's 4 rows m of the tile, one tap's channels n .. n + 3: its tap shift in the staged dt (a
    // padding row: offset 0 -- in range, the row is not stored)
    const int m = (mtb + 4 * u) * 16 + 4 * (i & 3);
    const int tap = m / cs, ky = tap / a.KW, kx = tap - ky * a.KW;
    aoff[u] = m < mtot ? (ky * hc + kx) * a.xpix + (m - tap * cs) : 0;
  }
  // the bias gradient's 16-channel tiles of this wave, and the lane's 4 channels in them (past Cs_out:
  // channel 0 -- in range, those rows are not stored)
  const bool do_bias = a.has_bias && blockIdx.z == 0;
  int boff[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    bacc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int n = ((blockIdx.y * 4 + wave) * 4 + k) * 16 + 4 * (i & 3);
    boff[k] = n < cs ? n : 0;
  }
  bf16x8 ones;
#pragma unroll
  for (int j = 0; j < 8; ++j) ones[j] = f2bf(1.f);
  const int nrb = tc_cdiv(a.H, a.R);
  const long long npairs = (long long)a.B * nrb;
  const long long p_lo = (long long)blockIdx.x * a.pairs_per_slab;
  const long long p_hi = min(p_lo + a.pairs_per_slab, npairs);
  // (every phase below re-reads the arguments it needs: tc_args)
  for (long long pr = p_lo; pr < p_hi; ++pr) {
    const TconvArgs& a = tc_args();
    const TcGeo G = tc_geo(a, TC_WGRAD);
    const int s = a.stride, cs = a.Cs_out, hc = G.hc, xb = tc_xb(a), ncols = tc_a16(a.Cs_in);
    const int b = (int)(pr / nrb), rb = (int)(pr - (long long)b * nrb), r0 = rb * a.R;
    const int Rv = min(a.R, a.H - r0);
    const int npix = Rv * a.W, npix32 = (npix + 31) & ~31;
    const int hr = (Rv - 1) * s + G.ty;
    __syncthreads();      // (the previous pair's readers are done)
    tc_stage<8>(hd, a.xpix, a.dt + (size_t)b * a.Ho * a.Wo * cs, cs, hr, hc, cs / 8, cs / 8, r0 * s - a.pad_t, -a.pad_l, a.Ho, a.Wo);
    tc_stage<VEC>(hx, xb, a.x + ((size_t)b * a.H + r0) * a.W * a.Cs_in, a.Cs_in, 1, npix32, ncols / VEC, a.Cs_in / VEC, 0, 0, 1, npix);
    __syncthreads();
    for (int p0 = 0; p0 < npix32; p0 += 32) {
      // the lane's two pixels of the 32 (rows of the transposed reads); past the block: x rows of zeros
      // against any dt pixel of the block
      const int pl = p0 + 8 * g + (i >> 2), ph = pl + 4;
      const int al = pl < npix ? pl : 0, ah = ph < npix ? ph : 0;
      const int dl = ((al / a.W) * s * hc + (al % a.W) * s) * a.xpix, dh = ((ah / a.W) * s * hc + (ah % a.W) * s) * a.xpix;
      bf16x8 bfr[NTW];
#pragma unroll
      for (int nt = 0; nt < NTW; ++nt) {
        // (an n-tile past the staged columns: a defined address, the tile is not stored)
        const int col = nbase + nt * 16 < ncols ? nbase + nt * 16 + 4 * (i & 3) : 0;
        const bf16x4 lo = tc_tr_read(hx + (size_t)pl * xb + col);
        const bf16x4 hi = tc_tr_read(hx + (size_t)ph * xb + col);
        bfr[nt] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
      }
#pragma unroll
      for (int u = 0; u < TC_MTW; ++u) {
        const bf16x4 lo = tc_tr_read(hd + dl + aoff[u]);
        const bf16x4 hi = tc_tr_read(hd + dh + aoff[u]);
        const bf16x8 afr = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) acc[u][nt] = mfma16(afr, bfr[nt], acc[u][nt]);
      }
    }
    if (do_bias) {
      // the dt pixels the block owns: the first Rv * s staged rows (the last block: all of them), every
      // staged column -- contiguous; past them: the pixel of zeros
      const int nown = (rb == nrb - 1 ? hr : Rv * s) * hc;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (((blockIdx.y * 4 + wave) * 4 + k) * 16 >= cs) continue;
        for (int t0 = 0; t0 < nown; t0 += 32) {
          const int pl = t0 + 8 * g + (i >> 2), ph = pl + 4;
          const bf16x4 lo = tc_tr_read((pl < nown ? hd + (size_t)pl * a.xpix : hz) + boff[k]);
          const bf16x4 hi = tc_tr_read((ph < nown ? hd + (size_t)ph * a.xpix : hz) + boff[k]);
          bacc[k] = mfma16(__builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7), ones, bacc[k]);
        }
      }
    }
  }
  // lane (i, g) holds rows m = 16 mt + 4 g + j of column c = nbase + 16 nt + i
  const TconvArgs& ea = tc_args();
  float* row = ea.slab + (size_t)blockIdx.x * ea.slab_ld;
#pragma unroll
  for (int nt = 0; nt < NTW; ++nt) {
    const int c = nbase + nt * 16 + i;
    if (c >= ea.Cin) continue;
#pragma unroll
    for (int u = 0; u < TC_MTW; ++u) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int m = (mtb + 4 * u) * 16 + 4 * g + j;
        const int tap = m / ea.Cs_out, n = m - tap * ea.Cs_out;
        if (m < ea.KH * ea.KW * ea.Cs_out && n < ea.Cout) row[((size_t)tap * ea.Cout + n) * ea.Cin + c] = acc[u][nt][j];
      }
    }
  }
  if (do_bias && i == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int n = ((blockIdx.y * 4 + wave) * 4 + k) * 16 + 4 * g + j;
        if (n < ea.Cout) row[tc_bias_off(ea) + n] = bacc[k][j];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------
// n-tiles per workgroup for n result channels (tconv_dgrad: at most 2, its BwdThrough epilogue's registers)
int tconv_ntw(int n, int kind) { return n <= 16 ? 1 : (n <= 32 || kind == TC_DGRAD) ? 2 : 4; }

// LDS bytes of a launch with R input rows per block (fwd / dgrad: and kc k-steps of weights)
size_t tconv_lds_bytes(const TconvArgs& a, int kind, int R, int kc) {
  const TcGeo G = tc_geo(a, kind);
  const size_t halo = tc_halo_elems(tc_rows(a, kind, G, R), G.hc, a.xpix) * 2;
  if (kind == TC_WGRAD) return halo + (size_t)((R * a.W + 31) & ~31) * tc_xb(a) * 2 + (size_t)tc_a16(a.xpix) * 2;
  return (size_t)tc_a16(tc_ks(G) * (G.ck == 4 ? 8 : 4) * 4) + (size_t)kc * a.ntw * 1024 + halo;
}

static void tc_check_geometry(const TconvArgs& a, int kind, const std::string& w) {
  if (kind != TC_FWD && kind != TC_DGRAD && kind != TC_WGRAD) throw std::invalid_argument(w + ": kind");
  if (a.stride < 1 || a.stride > 4) throw std::invalid_argument(w + ": strides must be in 1..4");
  if (a.Cs_in != 4 && (a.Cs_in <= 0 || a.Cs_in % 8 || a.Cs_in > 2048))
    throw std::invalid_argument(w + ": the input's channel stride must be 4 or a multiple of 8 (at most 2048)");
  if (a.Cs_out <= 0 || a.Cs_out % 8 || a.Cs_out > 2048)
    throw std::invalid_argument(w + ": the output's channel stride must be a multiple of 8 (at most 2048)");
  if (a.Cin <= 0 || a.Cin > a.Cs_in || a.Cout <= 0 || a.Cout > a.Cs_out)
    throw std::invalid_argument(w + ": channels must be in [1, channel stride]");
  if (a.B < 0 || a.H <= 0 || a.W <= 0 || a.Ho <= 0 || a.Wo <= 0 || a.H > 32768 || a.W > 32768)
    throw std::invalid_argument(w + ": batch / grid sizes");
  if (a.KH <= 0 || a.KW <= 0 || a.KH * a.KW > 1024) throw std::invalid_argument(w + ": kernel size");
  // the output grid of TensorFlow's conv2d_transpose: H*s + max(k - s, 0) minus the padding, the top /
  // left part of which is at most the whole of it
  const int s = a.stride, eh = tc_max(a.KH - s, 0), ew = tc_max(a.KW - s, 0);
  if (a.pad_t < 0 || a.pad_l < 0 || a.Ho + a.pad_t < a.H * s || a.Ho + a.pad_t > a.H * s + eh || a.Wo + a.pad_l < a.W * s ||
      a.Wo + a.pad_l > a.W * s + ew)
    throw std::invalid_argument(w + ": the output grid and top / left padding must satisfy H*s <= Ho + pad <= H*s + max(k - s, 0)");
  if ((long long)a.H * a.W * a.Cs_in > 0x7fffffffLL || (long long)a.Ho * a.Wo * a.Cs_out > 0x7fffffffLL)
    throw std::invalid_argument(w + ": one image must stay below 2^31 elements");
  if ((long long)a.KH * a.KW * a.Cin * a.Cout > 0x7ffffff0LL) throw std::invalid_argument(w + ": kernel elements");
  if (a.ntw != 1 && a.ntw != 2 && a.ntw != 4) throw std::invalid_argument(w + ": n-tiles per workgroup must be 1, 2 or 4");
  if (kind == TC_DGRAD && a.ntw == 4) throw std::invalid_argument(w + ": tconv_dgrad takes 1 or 2 n-tiles per workgroup");
  if (kind == TC_WGRAD && a.Cs_in == 4 && a.ntw != 1)
    throw std::invalid_argument(w + ": a 4-lane input has one n-tile of input channels per workgroup");
  if (kind == TC_DGRAD && a.Cs_in == 4) throw std::invalid_argument(w + ": no input gradient for a 4-lane model input");
  const TcGeo G = tc_geo(a, kind);
  const int vec = G.ck == 4 ? 4 : 8;
  if (a.xpix < G.ck || a.xpix % vec || a.xpix > G.ck + 64)
    throw std::invalid_argument(w + ": the staged pixel stride must be a multiple of the vector width in [Ck, Ck + 64]");
}

// (R, kc): input rows per block -- the fewest row blocks per image (balanced) whose LDS stage fits
// TC_LDS_BUDGET (fwd / dgrad: with at least two k-steps of weights, or all of them) and that leave at
// least ``want`` workgroups; 1 where nothing gives that many; 0 where not even one row fits -- and the
// k-steps of weights that then fit (wgrad: 0).
std::tuple<int, int> tconv_cfg(const TconvArgs& a, int kind, int want) {
  tc_check_geometry(a, kind, "tconv_cfg");
  const TcGeo G = tc_geo(a, kind);
  const int KS = tc_ks(G), kmin = kind == TC_WGRAD ? 0 : (KS < 2 ? KS : 2);
  long long per = kind == TC_WGRAD ? (long long)tc_cdiv(tc_cdiv(a.KH * a.KW * a.Cs_out, 16), 4 * TC_MTW) : 1;
  per *= tc_cdiv(tc_cdiv(G.n, 16), a.ntw);
  int R = 0;
  if (tconv_lds_bytes(a, kind, 1, kmin) <= TC_LDS_BUDGET) {
    R = 1;
    for (int c = 1; c <= a.H; ++c) {
      const int r = tc_cdiv(a.H, c);
      if (tconv_lds_bytes(a, kind, r, kmin) > TC_LDS_BUDGET) continue;
      if ((long long)a.B * tc_cdiv(a.H, r) * per < want) continue;
      R = r;
      break;
    }
  }
  int kc = 0;
  if (R > 0 && kind != TC_WGRAD) {
    const size_t left = TC_LDS_BUDGET - tconv_lds_bytes(a, kind, R, 0);
    kc = (int)(left / ((size_t)a.ntw * 1024));
    if (kc > KS) kc = KS;
  }
  return std::make_tuple(R, kc);
}

static bool tc_bad_ptr(const void* p, int Cs) { return !p || (reinterpret_cast<uintptr_t>(p) & (Cs == 4 ? 7 : 15)); }

// the checks every launch shares; returns the grid's x (image, row block) count
static unsigned tc_check(const TconvArgs& a, int kind, const std::string& w) {
  tc_check_geometry(a, kind, w);
  if (a.R <= 0 || a.R > a.H) throw std::invalid_argument(w + ": rows per block must be in [1, rows]");
  if (kind != TC_WGRAD && (a.kc <= 0 || a.kc > tc_ks(tc_geo(a, kind))))
    throw std::invalid_argument(w + ": the weight chunk must be in [1, k-steps]");
  if (tconv_lds_bytes(a, kind, a.R, a.kc) > TC_LDS_BUDGET)
    throw std::invalid_argument(w + ": the block's LDS stage exceeds " + std::to_string(TC_LDS_BUDGET) + " bytes");
  if (!a.w || (reinterpret_cast<uintptr_t>(a.w) & 3)) throw std::invalid_argument(w + ": weight pointer (null or misaligned)");
  const long long blocks = (long long)a.B * tc_cdiv(a.H, a.R);
  if (blocks > 0x7fffffffLL) throw std::invalid_argument(w + ": too many blocks for one launch");
  return (unsigned)blocks;
}

template <class Kn>
static void tc_launch(Kn k, dim3 grid, size_t lds, hipStream_t s, const TconvArgs& a) {
  if (lds > 65536) (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(k, grid, dim3(TC_THREADS), lds, s, a);
}

template <bool CS4, int KIND>
static void tc_conv_launch(const TconvArgs& a, dim3 grid, size_t lds, hipStream_t s) {
  if (a.ntw == 1) tc_launch(tconv_conv_kernel<CS4, 1, KIND>, grid, lds, s, a);
  else if (a.ntw == 2) tc_launch(tconv_conv_kernel<CS4, 2, KIND>, grid, lds, s, a);
  else if constexpr (KIND != TC_DGRAD) tc_launch(tconv_conv_kernel<CS4, 4, KIND>, grid, lds, s, a);      // (tc_check: no 4 n-tile dgrad)
}

void launch_tconv_fwd(const TconvArgs& a, hipStream_t s) {
  const std::string w("tconv_fwd");
  const unsigned blocks = tc_check(a, TC_FWD, w);
  if (tc_bad_ptr(a.x, a.Cs_in)) throw std::invalid_argument(w + ": input pointer (null or misaligned)");
  if (tc_bad_ptr(a.out, a.Cs_out)) throw std::invalid_argument(w + ": output pointer (null or misaligned)");
  if (a.bias && (reinterpret_cast<uintptr_t>(a.bias) & 3)) throw std::invalid_argument(w + ": bias pointer (misaligned)");
  if (!blocks) return;
  const dim3 grid(blocks, tc_cdiv(tc_cdiv(a.Cout, 16), a.ntw));
  const size_t lds = tconv_lds_bytes(a, TC_FWD, a.R, a.kc);
  if (a.Cs_in == 4) tc_conv_launch<true, TC_FWD>(a, grid, lds, s);
  else tc_conv_launch<false, TC_FWD>(a, grid, lds, s);
}

void launch_tconv_dgrad(const TconvArgs& a, hipStream_t s) {
  const std::string w("tconv_dgrad");
  const unsigned blocks = tc_check(a, TC_DGRAD, w);
  if (tc_bad_ptr(a.dt, a.Cs_out)) throw std::invalid_argument(w + ": gradient pointer (null or misaligned)");
  const BwdThrough& t = a.bt;
  if (t.pH != a.H || t.pW != a.W || t.pC != a.Cin || t.pCs != a.Cs_in)
    throw std::invalid_argument(w + ": the feeding stage's BwdThrough geometry differs from the input grid");
  if (tc_bad_ptr(t.dy, a.Cs_in)) throw std::invalid_argument(w + ": BwdThrough dy (null or misaligned)");
  if (t.prev_relu && tc_bad_ptr(t.prev_out, a.Cs_in)) throw std::invalid_argument(w + ": BwdThrough prev_out (null or misaligned)");
  if (t.wt && (long long)a.B * a.H * a.W * a.Cs_in * 2 >= (1LL << 31))
    throw std::invalid_argument(w + ": write-through stores need a gradient buffer below 2 GB");
  if (t.drop_thr && !(t.drop_scale >= 1.f)) throw std::invalid_argument(w + ": BwdThrough dropout scale");
  if (!blocks) return;
  const dim3 grid(blocks, tc_cdiv(tc_cdiv(a.Cin, 16), a.ntw));
  tc_conv_launch<false, TC_DGRAD>(a, grid, tconv_lds_bytes(a, TC_DGRAD, a.R, a.kc), s);
}

void launch_tconv_wgrad(const TconvArgs& a, hipStream_t s) {
  const std::string w("tconv_wgrad");
  const unsigned blocks = tc_check(a, TC_WGRAD, w);
  if (tc_bad_ptr(a.x, a.Cs_in)) throw std::invalid_argument(w + ": input pointer (null or misaligned)");
  if (tc_bad_ptr(a.dt, a.Cs_out)) throw std::invalid_argument(w + ": gradient pointer (null or misaligned)");
  if (!a.slab || (reinterpret_cast<uintptr_t>(a.slab) & 3)) throw std::invalid_argument(w + ": slab pointer (null or misaligned)");
  if (a.slab_ld < (a.has_bias ? tc_bias_off(a) + a.Cout : a.KH * a.KW * a.Cin * a.Cout))
    throw std::invalid_argument(w + ": slab row stride");
  if (!blocks) {
    if (a.S) throw std::invalid_argument(w + ": slabs of an empty batch");
    return;
  }
  if (a.S <= 0 || a.pairs_per_slab <= 0 || (long long)a.S * a.pairs_per_slab < blocks ||
      (long long)(a.S - 1) * a.pairs_per_slab >= blocks)
    throw std::invalid_argument(w + ": S slabs of pairs_per_slab (image, row block) pairs must cover the pairs, none empty");
  const dim3 grid(a.S, tc_cdiv(tc_cdiv(a.KH * a.KW * a.Cs_out, 16), 4 * TC_MTW), tc_cdiv(tc_cdiv(a.Cin, 16), a.ntw));
  const size_t lds = tconv_lds_bytes(a, TC_WGRAD, a.R, 0);
  if (a.Cs_in == 4) tc_launch(tconv_wgrad_kernel<true, 1>, grid, lds, s, a);      // (tc_check_geometry: ntw == 1)
  else if (a.ntw == 1) tc_launch(tconv_wgrad_kernel<false, 1>, grid, lds, s, a);
  else if (a.ntw == 2) tc_launch(tconv_wgrad_kernel<false, 2>, grid, lds, s, a);
  else tc_launch(tconv_wgrad_kernel<false, 4>, grid, lds, s, a);
}

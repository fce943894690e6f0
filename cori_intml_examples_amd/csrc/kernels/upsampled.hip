// Up-sampled convolution (Keras UpSampling2D(s), nearest, folded into the stride-1 Conv2D behind it):
// forward, the gradient to the LOW-resolution input, the weight and bias gradient (UpArgs, args.h).
// The up-sampled tensor never exists: with up(u, v) = x[u // s, v // s] inside the virtual H*s x W*s grid
// and 0 outside it,
//
//   upconv_fwd    out[b, Y, X, n] = bf16(A(bias[n] + sum_{ky, kx, c} w[ky, kx, c, n] * up(Y + ky - pad_t, X + kx - pad_l)[c]))
//   upconv_dgrad  dx[b, i, j, c]  = sum_{du, dv < s} sum_{ky, kx, n} w[ky, kx, c, n] * dt[b, s*i + du + pad_t - ky, s*j + dv + pad_l - kx, n]
//                 handed to the feeding stage's BwdThrough (its dropout mask, relu mask, pool codes, bf16 rounding)
//   upconv_wgrad  dW[ky, kx, c, n] = sum_{b, Y, X} up(Y + ky - pad_t, X + kx - pad_l)[c] * dt[b, Y, X, n]
//                 db[n]            = sum_{b, Y, X} dt[b, Y, X, n]
//
// All three are implicit GEMMs on v_mfma_f32_16x16x32_bf16.  w is the fp32 master, rounded to bf16 as it
// is staged into LDS (no weight pack); every product is bf16(x) * bf16(w) of ONE master weight (taps that
// land on the same source pixel are not pre-summed); accumulation is fp32 in one fixed order, without
// atomics: two launches are bit-identical.
//
// Floor division makes the padding free: a virtual index lies inside the virtual grid exactly when its
// // s lies inside the source grid, so a LOW-resolution halo staged with zeros outside the source grid is
// the conv's zero padding.  With Y - pad_t = s * qy + py (0 <= py < s) tap ky reads source row
// qy + (py + ky) // s: a base that depends on the pixel, plus an offset that depends on its PHASE (py, px)
// and the tap alone -- a table in LDS, no division in the k loop.
//
// upconv_fwd / upconv_dgrad (one body, up_conv_kernel): M = result pixels, N = result channels, K padded to
// a multiple of 32.  A workgroup takes one image, a block of R result rows (grid x; R need not be a
// multiple of s) and a slice of ntw n-tiles (grid y).  LDS map: [offset tables][pixel table][weight chunk]
// [staged image].  The pixel table holds, per result pixel of the block, its base in the staged image and its
// phase in one int (filled once: the passes and the k loop divide nothing).
//   fwd    K = (tap, c).  Staged: source rows (Y0 - pad_t) // s .. (Y0 + R - 1 + kh - 1 - pad_t) // s, columns
//          (-pad_l) // s .. (Wo - 1 + kw - 1 - pad_l) // s, all channels, pixel stride xpix, ONCE.  Tables:
//          s * s phases x one offset per 8 consecutive k (Ck == 4: per 4 k).
//   dgrad  K = (du, dv, tap, n): as many multiply-adds as the forward.  Staged: dt rows
//          s * i0 + pad_t - (kh - 1) .. s * (i0 + R) + pad_t - 1, columns pad_l - (kw - 1) .. s * W + pad_l - 1
//          (zeros outside the dt grid); result pixel (i, j) is based at staged pixel (s * (i - i0), s * j),
//          and ONE table holds the offsets (du + kh - 1 - ky, dv + kw - 1 - kx).
//   The k padding points at offset 0 -- in range, and its weights are zeros.  Weights: kc k-steps x ntw
//   n-tiles in fragment order [(ks, nt)][lane][8], K walked in chunks of kc k-steps when the slice does not
//   fit.  The MFMA runs TRANSPOSED (weights as A, pixels as B): a lane holds 4 consecutive channels of ONE
//   pixel, one exchange with lane ^ 16 makes 8, the even 16-lane groups store 16 bytes.  A wave keeps
//   UP_MTW m-tiles x ntw n-tiles; larger blocks take further passes.  (dgrad: at most 2 n-tiles.)
//
// upconv_wgrad: M = (tap, c), N = Cout, K = OUTPUT pixels.  Workgroup (g, my, nz) takes the (image, block
// of R output rows) pairs [g * pairs_per_slab, ...), stages the forward's source block and the block's dt
// rows ([pixel][channel], zero rows up to a multiple of 32 pixels) of each pair and keeps its accumulators
// in registers across the pairs.  Both operands are k = pixel runs out of [pixel][channel] tiles:
// transposed LDS reads (ds_read_b64_tr_b16), each lane addressing ITS pixel's base plus the
// [phase][tap] table entry of its rows' tap.  The bias gradient is one more MFMA per n-tile with an
// all-ones A fragment (wave 3 of my == 0).  It writes ONE slab row: [KH][KW][Cin][Cout] (Keras order,
// unpadded), then on the next 16-byte boundary [Cout]; the slab reduction takes both as identity descriptors.
#include <cstdint>
#include <stdexcept>
#include <string>
#include <tuple>

#include "args.h"
#include "bwd_through.h"

template <int VEC> struct UpVec;
template <> struct UpVec<8> {
  typedef bf16x8 T;
  __device__ __forceinline__ static T load_if(bool ok, const bf16* p, const bf16* safe) { return load_bf16x8_if(ok, p, safe); }
};
template <> struct UpVec<4> {
  typedef bf16x4 T;
  __device__ __forceinline__ static T load_if(bool ok, const bf16* p, const bf16* safe) { return load_bf16x4_if(ok, p, safe); }
};

__host__ __device__ __forceinline__ int up_a16(int v) { return (v + 15) & ~15; }
__host__ __device__ __forceinline__ int up_cdiv(int a, int b) { return (a + b - 1) / b; }
// floor(a / s), s > 0
__host__ __device__ __forceinline__ int up_fdiv(int a, int s) { return a >= 0 ? a / s : -((s - 1 - a) / s); }

// What a launch kind contracts over and produces: the staged grid [sh, sw, scs] (x or dt) and its ck
// contraction channels, the result grid [rh, rw], the result channels n (their stride ns), the (block, tap)
// groups ntk of K, the offset tables nph, and the staged image's columns hc, the first at source column sx0.
struct UpGeo {
  int sh, sw, scs, ck, rh, rw, n, ns, ntk, nph, hc, sx0;
};
__host__ __device__ __forceinline__ UpGeo up_geo(const UpArgs& a, int kind) {
  UpGeo g;
  const int s = a.up;
  if (kind == UP_DGRAD) {
    g.sh = a.Ho, g.sw = a.Wo, g.scs = g.ck = a.Cs_out, g.rh = a.H, g.rw = a.W, g.n = a.Cin, g.ns = a.Cs_in;
    g.ntk = s * s * a.KH * a.KW, g.nph = 1;
    g.sx0 = a.pad_l - (a.KW - 1), g.hc = s * a.W + a.KW - 1;
  } else {
    g.sh = a.H, g.sw = a.W, g.scs = g.ck = a.Cs_in, g.rh = a.Ho, g.rw = a.Wo, g.n = a.Cout, g.ns = a.Cs_out;
    g.ntk = a.KH * a.KW, g.nph = s * s;
    g.sx0 = up_fdiv(-a.pad_l, s), g.hc = up_fdiv(a.Wo - 1 + a.KW - 1 - a.pad_l, s) - g.sx0 + 1;
  }
  return g;
}
// the staged rows of result rows [r0, r0 + rv): the first source row, and how many
__host__ __device__ __forceinline__ void up_rows(const UpArgs& a, int kind, int r0, int rv, int* sy0, int* hr) {
  if (kind == UP_DGRAD) {
    *sy0 = a.up * r0 + a.pad_t - (a.KH - 1), *hr = a.up * rv + a.KH - 1;
  } else {
    *sy0 = up_fdiv(r0 - a.pad_t, a.up), *hr = up_fdiv(r0 + rv - 1 + a.KH - 1 - a.pad_t, a.up) - *sy0 + 1;
  }
}
// the most rows any block of R result rows stages
__host__ __device__ __forceinline__ int up_max_rows(const UpArgs& a, int kind, int R) {
  return kind == UP_DGRAD ? a.up * R + a.KH - 1 : (R + a.KH - 1 + a.up - 2) / a.up + 1;
}
__host__ __device__ __forceinline__ int up_ks(const UpGeo& g) { return up_cdiv(g.ntk * g.ck, 32); }
// upconv_wgrad's staged dt rows: all n-tiles' columns defined (zeros behind Cs_out), 16 bytes of padding
__host__ __device__ __forceinline__ int up_dpix(const UpArgs& a) { return up_a16(a.Cs_out) + 8; }
// elements of a staged image, to a 16-byte boundary
__host__ __device__ __forceinline__ size_t up_img_elems(int hr, int hc, int xpix) { return ((size_t)hr * hc * xpix + 7) & ~(size_t)7; }
__host__ __device__ __forceinline__ int up_bias_off(const UpArgs& a) { return (a.KH * a.KW * a.Cin * a.Cout + 3) & ~3; }
// bytes of the offset tables: fwd / dgrad one int per (phase, VEC consecutive k), wgrad per (phase, tap)
__host__ __device__ __forceinline__ int up_table_bytes(const UpArgs& a, int kind) {
  const UpGeo g = up_geo(a, kind);
  return up_a16(4 * (kind == UP_WGRAD ? g.nph * a.KH * a.KW : g.nph * up_ks(g) * (g.ck == 4 ? 8 : 4)));
}
// bytes of the pixel table of a block of R result rows: one int per pixel, base | (phase * mul) << shift (the base
// stays below 2^17 elements: the LDS budget; upconv_wgrad keeps phase * taps < 2^14 beside it)
__host__ __device__ __forceinline__ int up_ptab_bytes(int R, int rw) { return up_a16(4 * R * rw); }
// Fill it for result rows [r0, r0 + rv) of the forward grid (upconv_fwd, upconv_wgrad): pixel (Y, X) with
// Y - pad_t = s * qy + py, X - pad_l = s * qx + px is based at staged pixel (qy - sy0, qx - sx0), phase py * s + px.
__device__ __forceinline__ void up_fill_ptab(int* ptab, const UpArgs& a, int r0, int npix, int sy0, int sx0, int hc, int mul, int shift) {
  const int s = a.up;
  for (int p = threadIdx.x; p < npix; p += UP_THREADS) {
    const int r = p / a.Wo, ty = r0 + r - a.pad_t, tx = p - r * a.Wo - a.pad_l;
    const int qy = up_fdiv(ty, s), qx = up_fdiv(tx, s);
    ptab[p] = (int)((unsigned)(((qy - sy0) * hc + (qx - sx0)) * a.xpix) | ((unsigned)(((ty - qy * s) * s + (tx - qx * s)) * mul) << shift));
  }
}

// Stage ``npx`` = hr * hc pixels: pixel (r, c) is source pixel (r + oy, c + ox) of [sh, sw, scs], its first
// ``ncg`` VEC-channel groups (groups >= src_ncg and pixels outside the grid: zeros), at dst + pixel * dpix.
template <int VEC>
__device__ __forceinline__ void up_stage(bf16* dst, int dpix, const bf16* src, int scs, int hr, int hc, int ncg,
                                         int src_ncg, int oy, int ox, int sh, int sw) {
  typedef typename UpVec<VEC>::T V;
  staged_copy<4, V>(
      hr * hc * ncg, (int)threadIdx.x, UP_THREADS,
      [&](int i) {
        const int t = i / ncg, cg = i - t * ncg;
        const int r = t / hc, c = t - r * hc;
        const int y = r + oy, x = c + ox;
        const bool ok = y >= 0 && x >= 0 && y < sh && x < sw && cg < src_ncg;
        return UpVec<VEC>::load_if(ok, src + ((size_t)y * sw + x) * scs + cg * VEC, src);
      },
      [&](int i, const V& v) {
        const int t = i / ncg, cg = i - t * ncg;
        *reinterpret_cast<V*>(dst + (size_t)t * dpix + cg * VEC) = v;
      });
}

template <bool CS4, int NTW, int KIND>
__global__ __launch_bounds__(UP_THREADS) void up_conv_kernel(const UpArgs a) {
  constexpr int VEC = CS4 ? 4 : 8;
  extern __shared__ __attribute__((aligned(16))) unsigned char up_smem[];
  const UpGeo G = up_geo(a, KIND);
  const int s = a.up, ntaps = a.KH * a.KW, ck = G.ck, hc = G.hc, KS = up_ks(G), nq = KS * (32 / VEC);
  int* toff = reinterpret_cast<int*>(up_smem);
  int* ptab = reinterpret_cast<int*>(up_smem + up_table_bytes(a, KIND));
  bf16* wl = reinterpret_cast<bf16*>(up_smem + up_table_bytes(a, KIND) + up_ptab_bytes(a.R, G.rw));
  bf16* hx = wl + (size_t)a.kc * NTW * 512;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 15, g = lane >> 4;
  const int nrb = up_cdiv(G.rh, a.R);
  const int b = blockIdx.x / nrb, r0 = (blockIdx.x - b * nrb) * a.R;
  const int Rv = min(a.R, G.rh - r0);
  int sy0, hr;
  up_rows(a, KIND, r0, Rv, &sy0, &hr);
  const int nbase = blockIdx.y * NTW * 16;
  // the staged offset of every VEC consecutive k -- per phase for the forward: tap (ky, kx) of a pixel of
  // phase (py, px) lies (py + ky) // s rows and (px + kx) // s columns behind the pixel's base; the padding: 0
  for (int e = tid; e < G.nph * nq; e += UP_THREADS) {
    const int ph = e / nq, q = e - ph * nq;
    const int k0 = q * VEC, grp = k0 / ck, c0 = k0 - grp * ck;
    const int blk = grp / ntaps, tap = grp - blk * ntaps, ky = tap / a.KW, kx = tap - ky * a.KW;
    int dy, dx;
    if (KIND == UP_FWD) {
      const int py = ph / s, px = ph - py * s;
      dy = (py + ky) / s, dx = (px + kx) / s;
    } else {
      const int du = blk / s, dv = blk - du * s;
      dy = du + a.KH - 1 - ky, dx = dv + a.KW - 1 - kx;
    }
    toff[e] = grp < G.ntk ? (dy * hc + dx) * a.xpix + c0 : 0;
  }
  const int npix = Rv * G.rw;
  if (KIND == UP_FWD) {
    up_fill_ptab(ptab, a, r0, npix, sy0, G.sx0, hc, 1, 28);
  } else {
    for (int p = tid; p < npix; p += UP_THREADS) {
      const int r = p / G.rw;
      ptab[p] = (s * r * hc + s * (p - r * G.rw)) * a.xpix;
    }
  }
  const bf16* src = KIND == UP_FWD ? a.x : a.dt;
  up_stage<VEC>(hx, a.xpix, src + (size_t)b * G.sh * G.sw * G.scs, G.scs, hr, hc, ck / VEC, ck / VEC, sy0, G.sx0, G.sh, G.sw);
  const uint32_t step = a.st ? (uint32_t)a.st->t : 0u;
  const int nmt = up_cdiv(npix, 16), nchunks = up_cdiv(KS, a.kc);
  __syncthreads();      // (the tables, the pixel table and the staged image)
  for (int mt0 = 0; mt0 < nmt; mt0 += 4 * UP_MTW) {
    f32x4 acc[UP_MTW][NTW];
    int pixoff[UP_MTW], tb[UP_MTW];
#pragma unroll
    for (int u = 0; u < UP_MTW; ++u) {
#pragma unroll
      for (int nt = 0; nt < NTW; ++nt) acc[u][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
      const int p = (mt0 + wave + 4 * u) * 16 + i;
      const unsigned e = (unsigned)ptab[p < npix ? p : 0];      // (a tail lane: any pixel of the block; its results are not stored)
      pixoff[u] = (int)(e & 0x0fffffffu);
      tb[u] = (int)(e >> 28) * nq;
    }
    for (int ch = 0; ch < nchunks; ++ch) {
      const int ks0 = ch * a.kc, kcn = min(a.kc, KS - ks0);
      if (nchunks > 1 || mt0 == 0) {
        __syncthreads();      // (the previous chunk's readers are done)
        // the weight chunk in fragment order, rounded to bf16: element j of lane (i, g) of (ks, nt) is
        // W[k = 32 ks + 8 g + j][n = nbase + 16 nt + i]; zeros in the k and n padding.  Thread order follows
        // the master's contiguous axis: n for the forward, the contraction channel for the dgrad.
        for (int e = tid; e < kcn * NTW * 512; e += UP_THREADS) {
          const int t = e >> 9;
          int ei, ej, eg;
          if (KIND == UP_FWD) ei = e & 15, ej = (e >> 4) & 7, eg = (e >> 7) & 3;
          else ej = e & 7, eg = (e >> 3) & 3, ei = (e >> 5) & 15;
          const int ksl = t / NTW, nt = t - ksl * NTW;
          const int k = (ks0 + ksl) * 32 + 8 * eg + ej, n = nbase + nt * 16 + ei;
          const int grp = k / ck, c = k - grp * ck, tap = grp % ntaps;
          float v = 0.f;
          if (grp < G.ntk && n < G.n) {
            if (KIND == UP_FWD) {
              if (c < a.Cin) v = a.w[((size_t)tap * a.Cin + c) * a.Cout + n];
            } else {
              if (c < a.Cout) v = a.w[((size_t)tap * a.Cin + n) * a.Cout + c];
            }
          }
          wl[((size_t)t * 64 + eg * 16 + ei) * 8 + ej] = f2bf(v);
        }
        __syncthreads();
      }
      for (int ksl = 0; ksl < kcn; ++ksl) {
        bf16x8 wfr[NTW];
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) wfr[nt] = *reinterpret_cast<const bf16x8*>(wl + ((size_t)(ksl * NTW + nt) * 64 + lane) * 8);
        const int q = (ks0 + ksl) * 4 + g;
#pragma unroll
        for (int u = 0; u < UP_MTW; ++u) {
          const int* tq = toff + (KIND == UP_FWD ? tb[u] : 0);
          bf16x8 xfr;
          if (CS4) {
            const bf16x4 lo = *reinterpret_cast<const bf16x4*>(hx + pixoff[u] + tq[2 * q]);
            const bf16x4 hi = *reinterpret_cast<const bf16x4*>(hx + pixoff[u] + tq[2 * q + 1]);
            xfr = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
          } else {
            xfr = *reinterpret_cast<const bf16x8*>(hx + pixoff[u] + tq[q]);
          }
#pragma unroll
          for (int nt = 0; nt < NTW; ++nt) acc[u][nt] = mfma16(wfr[nt], xfr, acc[u][nt]);
        }
      }
    }
    // epilogue: lane (i, g) holds channels n0 + j of pixel i, n0 = 16 nt + 4 g; lane ^ 16 holds the other
    // half of the 8-channel chunk, and the even groups store it.
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt) {
      const int n0 = nbase + nt * 16 + 4 * g;
      float bv[4];
      uint32_t keep[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool in = n0 + j < G.n;
        bv[j] = (KIND == UP_FWD && a.bias) ? a.bias[in ? n0 + j : 0] : 0.f;
        keep[j] = in ? 0xffffffffu : 0u;
      }
#pragma unroll
      for (int u = 0; u < UP_MTW; ++u) {
        const int p = (mt0 + wave + 4 * u) * 16 + i;      // (an m-tile past the block: every p >= npix)
        const size_t qi = ((size_t)b * G.rh + r0) * G.rw + p;      // (a block's pixels are consecutive in the image)
        float v[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float f = acc[u][nt][j];
          if (KIND == UP_FWD) {
            f += bv[j];
            if (a.relu) f = fmaxf(f, 0.f);
          }
          v[j] = __uint_as_float(__float_as_uint(f) & keep[j]);      // (padding channels: zeros)
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) v[4 + j] = __shfl_xor(v[j], 16);
        if ((g & 1) || p >= npix || n0 >= G.ns) continue;
        if (KIND == UP_FWD) {
          bf16x8 o;
#pragma unroll
          for (int j = 0; j < 8; ++j) o[j] = f2bf(v[j]);
          *reinterpret_cast<bf16x8*>(a.out + qi * G.ns + n0) = o;
        } else {
          // (the padding channels are zeros already: the form without the per-element channel test)
          const size_t o = qi * G.ns + n0;
          bwd_through_finish8_at<BtGeoRt, true, false>(a.bt, qi, n0, o, v, bwd_through_fetch8_at<BtGeoRt, false>(a.bt, o), step);
        }
      }
    }
  }
}

// The arguments, re-read from the kernel-argument segment: a phase that names them this way does not hold
// them in scalar registers across the loops before it (the device transposed.hip and wide_head.hip use).
__device__ __forceinline__ const UpArgs& up_args() {
  typedef const __attribute__((address_space(4))) UpArgs* KP;
  KP p = (KP)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return *(const UpArgs*)p;
}

__device__ __forceinline__ bf16x4 up_tr_read(const bf16* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4bf16(LDS_PTR(bf16x4, p));
}

template <bool CS4, int NTW>
__global__ __launch_bounds__(UP_THREADS) void up_wgrad_kernel(const UpArgs a) {
  constexpr int VEC = CS4 ? 4 : 8;
  extern __shared__ __attribute__((aligned(16))) unsigned char up_smem[];
  const UpGeo G = up_geo(a, UP_WGRAD);
  const int ntaps = a.KH * a.KW, cs = a.Cs_in, mtot = ntaps * cs, hc = G.hc, dpix = up_dpix(a);
  int* toff = reinterpret_cast<int*>(up_smem);                                   // [phase][tap]
  int* ptab = reinterpret_cast<int*>(up_smem + up_table_bytes(a, UP_WGRAD));     // [pixel of the block]
  bf16* hx = reinterpret_cast<bf16*>(up_smem + up_table_bytes(a, UP_WGRAD) + up_ptab_bytes(a.R, a.Wo));     // [hr][hc][xpix]
  bf16* hd = hx + up_img_elems(up_max_rows(a, UP_WGRAD, a.R), hc, a.xpix);       // [32-multiple of pixels][dpix]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 15, g = lane >> 4;
  const int nbase = blockIdx.z * NTW * 16, mtb = blockIdx.y * 4 * UP_MTW + wave;
  const int ncols = up_a16(a.Cs_out);      // the staged dt columns
  for (int e = tid; e < G.nph * ntaps; e += UP_THREADS) {
    const int ph = e / ntaps, tap = e - ph * ntaps, py = ph / a.up, px = ph - py * a.up, ky = tap / a.KW, kx = tap - ky * a.KW;
    toff[e] = (((py + ky) / a.up) * hc + (px + kx) / a.up) * a.xpix;
  }
  f32x4 acc[UP_MTW][NTW], bacc[NTW];
  int atap[UP_MTW], ac[UP_MTW];
#pragma unroll
  for (int u = 0; u < UP_MTW; ++u) {
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt) acc[u][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    // the lane's 4 rows m of the tile, one tap's channels c .. c + 3 (a padding row: tap 0, channel 0 -- in
    // range, the row is not stored)
    const int m = (mtb + 4 * u) * 16 + 4 * (i & 3);
    const int tap = m / cs;
    atap[u] = m < mtot ? tap : 0;
    ac[u] = m < mtot ? m - tap * cs : 0;
  }
#pragma unroll
  for (int nt = 0; nt < NTW; ++nt) bacc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int bias_wave = a.has_bias && blockIdx.y == 0 ? 3 : -1;
  bf16x8 ones;
#pragma unroll
  for (int j = 0; j < 8; ++j) ones[j] = f2bf(1.f);
  // (launch_upconv_wgrad: the pairs and S * pairs_per_slab stay below 2^32)
  const unsigned nrb = up_cdiv(a.Ho, a.R), npairs = (unsigned)a.B * nrb;
  const unsigned p_lo = blockIdx.x * (unsigned)a.pairs_per_slab, p_hi = min(p_lo + (unsigned)a.pairs_per_slab, npairs);
  for (unsigned pr = p_lo; pr < p_hi; ++pr) {
    const int b = (int)(pr / nrb), r0 = (int)(pr - b * nrb) * a.R;
    const int Rv = min(a.R, a.Ho - r0);
    const int npix = Rv * a.Wo, npix32 = (npix + 31) & ~31;
    int sy0, hr;
    up_rows(a, UP_WGRAD, r0, Rv, &sy0, &hr);
    __syncthreads();      // (the previous pair's readers are done; first pair: nothing)
    up_fill_ptab(ptab, a, r0, npix, sy0, G.sx0, hc, ntaps, 17);
    up_stage<VEC>(hx, a.xpix, a.x + (size_t)b * a.H * a.W * cs, cs, hr, hc, cs / VEC, cs / VEC, sy0, G.sx0, a.H, a.W);
    up_stage<8>(hd, dpix, a.dt + ((size_t)b * a.Ho + r0) * a.Wo * a.Cs_out, a.Cs_out, 1, npix32, ncols / 8, a.Cs_out / 8,
                0, 0, 1, npix);
    __syncthreads();      // (first pair: the table too)
    for (int p0 = 0; p0 < npix32; p0 += 32) {
      // the lane's two pixels of the 32 (rows of the transposed reads); past the block: dt rows of zeros
      // against any pixel of the block.  Each pixel: its base in the staged source block and its phase's table.
      const int pl = p0 + 8 * g + (i >> 2), ph = pl + 4;
      int xb[2], tp[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int p = h ? ph : pl;
        const unsigned e = (unsigned)ptab[p < npix ? p : 0];
        xb[h] = (int)(e & 0x1ffffu);
        tp[h] = (int)(e >> 17);
      }
      bf16x8 bfr[NTW];
#pragma unroll
      for (int nt = 0; nt < NTW; ++nt) {
        // (an n-tile past the staged columns: a defined address, the tile is not stored)
        const int col = nbase + nt * 16 < ncols ? nbase + nt * 16 + 4 * (i & 3) : 0;
        const bf16x4 lo = up_tr_read(hd + (size_t)pl * dpix + col);
        const bf16x4 hi = up_tr_read(hd + (size_t)ph * dpix + col);
        bfr[nt] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
      }
#pragma unroll
      for (int u = 0; u < UP_MTW; ++u) {
        const bf16x4 lo = up_tr_read(hx + xb[0] + toff[tp[0] + atap[u]] + ac[u]);
        const bf16x4 hi = up_tr_read(hx + xb[1] + toff[tp[1] + atap[u]] + ac[u]);
        const bf16x8 afr = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) acc[u][nt] = mfma16(afr, bfr[nt], acc[u][nt]);
      }
      if (wave == bias_wave) {
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) bacc[nt] = mfma16(ones, bfr[nt], bacc[nt]);
      }
    }
  }
  // lane (i, g) holds rows m = 16 mt + 4 g + j of column n = nbase + 16 nt + i
  const UpArgs& e = up_args();
  const int ecs = e.Cs_in, emtot = e.KH * e.KW * ecs;
  float* row = e.slab + (size_t)blockIdx.x * e.slab_ld;
#pragma unroll
  for (int nt = 0; nt < NTW; ++nt) {
    const int n = nbase + nt * 16 + i;
    if (n >= e.Cout) continue;
#pragma unroll
    for (int u = 0; u < UP_MTW; ++u) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int m = (mtb + 4 * u) * 16 + 4 * g + j;
        const int tap = m / ecs, c = m - tap * ecs;
        if (m < emtot && c < e.Cin) row[((size_t)tap * e.Cin + c) * e.Cout + n] = acc[u][nt][j];
      }
    }
    if (wave == bias_wave && g == 0) row[up_bias_off(e) + n] = bacc[nt][0];
  }
}

// ---------------------------------------------------------------------------------------------------
// n-tiles per workgroup for n result channels (upconv_dgrad: at most 2)
int up_ntw(int n, int kind) { return n <= 16 ? 1 : (n <= 32 || kind == UP_DGRAD) ? 2 : 4; }

// LDS bytes of a launch with R rows per block (fwd / dgrad: and kc k-steps of weights)
size_t up_lds_bytes(const UpArgs& a, int kind, int R, int kc) {
  const UpGeo G = up_geo(a, kind);
  const size_t img = up_img_elems(up_max_rows(a, kind, R), G.hc, a.xpix) * 2;
  const size_t tabs = (size_t)up_table_bytes(a, kind) + up_ptab_bytes(R, G.rw);
  if (kind == UP_WGRAD) return tabs + img + (size_t)((R * a.Wo + 31) & ~31) * up_dpix(a) * 2;
  return tabs + (size_t)kc * a.ntw * 1024 + img;
}

static void up_check_geometry(const UpArgs& a, int kind, const std::string& w) {
  if (kind != UP_FWD && kind != UP_DGRAD && kind != UP_WGRAD) throw std::invalid_argument(w + ": kind");
  if (a.up < 1 || a.up > 4) throw std::invalid_argument(w + ": the up-sampling size must be in 1..4");
  if (a.Cs_in != 4 && (a.Cs_in <= 0 || a.Cs_in % 8 || a.Cs_in > 2048))
    throw std::invalid_argument(w + ": the input's channel stride must be 4 or a multiple of 8 (at most 2048)");
  if (a.Cs_out <= 0 || a.Cs_out % 8 || a.Cs_out > 2048)
    throw std::invalid_argument(w + ": the output's channel stride must be a multiple of 8 (at most 2048)");
  if (a.Cin <= 0 || a.Cin > a.Cs_in || a.Cout <= 0 || a.Cout > a.Cs_out)
    throw std::invalid_argument(w + ": channels must be in [1, channel stride]");
  if (a.B < 0 || a.H <= 0 || a.W <= 0 || a.H > (1 << 20) || a.W > (1 << 20)) throw std::invalid_argument(w + ": batch / grid sizes");
  if (a.KH <= 0 || a.KW <= 0 || a.KH * a.KW > 1024) throw std::invalid_argument(w + ": kernel size");
  // the conv's output on the virtual H*s x W*s grid: 'valid' (no padding) or 'same' (Keras' split of k - 1)
  const int vh = a.H * a.up, vw = a.W * a.up;
  const bool valid = a.pad_t == 0 && a.pad_l == 0 && a.Ho == vh - a.KH + 1 && a.Wo == vw - a.KW + 1;
  const bool same = a.pad_t == (a.KH - 1) / 2 && a.pad_l == (a.KW - 1) / 2 && a.Ho == vh && a.Wo == vw;
  if (a.Ho <= 0 || a.Wo <= 0 || !(valid || same))
    throw std::invalid_argument(w + ": the output grid is not the layer's (a valid or same conv over the up-sampled grid)");
  if ((long long)a.H * a.W * a.Cs_in > 0x7fffffffLL || (long long)a.Ho * a.Wo * a.Cs_out > 0x7fffffffLL)
    throw std::invalid_argument(w + ": one image must stay below 2^31 elements");
  if ((long long)a.KH * a.KW * a.Cin * a.Cout > 0x7ffffff0LL) throw std::invalid_argument(w + ": kernel elements");
  if (a.ntw != 1 && a.ntw != 2 && a.ntw != 4) throw std::invalid_argument(w + ": n-tiles per workgroup must be 1, 2 or 4");
  const UpGeo G = up_geo(a, kind);
  const int vec = G.ck == 4 ? 4 : 8;
  if (kind != UP_WGRAD && G.ns > 16 * up_cdiv(G.n, 16))
    throw std::invalid_argument(w + ": the result's channel stride exceeds its channels rounded up to 16 (the n-tiles would leave chunks unwritten)");
  if (kind == UP_DGRAD && a.ntw == 4) throw std::invalid_argument(w + ": upconv_dgrad takes 1 or 2 n-tiles per workgroup");
  if (kind == UP_DGRAD && a.Cs_in == 4) throw std::invalid_argument(w + ": no input gradient for a 4-lane model input");
  if (a.xpix < G.ck || a.xpix % vec || a.xpix > G.ck + 64)
    throw std::invalid_argument(w + ": the staged pixel stride must be a multiple of the vector width in [Ck, Ck + 64]");
}

// (R, kc): rows per block -- the fewest row blocks per image (balanced) whose LDS stage fits UP_LDS_BUDGET
// (fwd / dgrad: with at least two k-steps of weights, or all of them) and that leave at least ``want``
// workgroups; 1 where nothing gives that many; 0 where not even one row fits -- and the k-steps of weights
// that then fit (wgrad: 0).
std::tuple<int, int> up_cfg(const UpArgs& a, int kind, int want) {
  up_check_geometry(a, kind, "up_cfg");
  const UpGeo G = up_geo(a, kind);
  const int KS = up_ks(G), kmin = kind == UP_WGRAD ? 0 : (KS < 2 ? KS : 2);
  long long per = kind == UP_WGRAD ? (long long)up_cdiv(up_cdiv(a.KH * a.KW * a.Cs_in, 16), 4 * UP_MTW) : 1;
  per *= up_cdiv(up_cdiv(G.n, 16), a.ntw);
  int R = 0;
  if (up_lds_bytes(a, kind, 1, kmin) <= UP_LDS_BUDGET) {
    R = 1;
    for (int c = 1; c <= G.rh; ++c) {
      const int r = up_cdiv(G.rh, c);
      if (up_lds_bytes(a, kind, r, kmin) > UP_LDS_BUDGET) continue;
      if ((long long)a.B * up_cdiv(G.rh, r) * per < want) continue;
      R = r;
      break;
    }
  }
  int kc = 0;
  if (R > 0 && kind != UP_WGRAD) {
    const size_t left = UP_LDS_BUDGET - up_lds_bytes(a, kind, R, 0);
    kc = (int)(left / ((size_t)a.ntw * 1024));
    if (kc > KS) kc = KS;
  }
  return std::make_tuple(R, kc);
}

static bool up_bad_ptr(const void* p, int Cs) { return !p || (reinterpret_cast<uintptr_t>(p) & (Cs == 4 ? 7 : 15)); }

// the checks every launch shares; returns the grid's x (image, row block) count
static unsigned up_check(const UpArgs& a, int kind, const std::string& w) {
  up_check_geometry(a, kind, w);
  const UpGeo G = up_geo(a, kind);
  if (a.R <= 0 || a.R > G.rh) throw std::invalid_argument(w + ": rows per block must be in [1, rows]");
  if (kind != UP_WGRAD && (a.kc <= 0 || a.kc > up_ks(G)))
    throw std::invalid_argument(w + ": the weight chunk must be in [1, k-steps]");
  if (up_lds_bytes(a, kind, a.R, a.kc) > UP_LDS_BUDGET)
    throw std::invalid_argument(w + ": the block's LDS stage exceeds " + std::to_string(UP_LDS_BUDGET) + " bytes");
  if (!a.w || (reinterpret_cast<uintptr_t>(a.w) & 3)) throw std::invalid_argument(w + ": weight pointer (null or misaligned)");
  const long long blocks = (long long)a.B * up_cdiv(G.rh, a.R);
  if (blocks > 0x7fffffffLL) throw std::invalid_argument(w + ": too many blocks for one launch");
  return (unsigned)blocks;
}

template <class Kn>
static void up_launch(Kn k, dim3 grid, size_t lds, hipStream_t s, const UpArgs& a) {
  if (lds > 65536) (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(k, grid, dim3(UP_THREADS), lds, s, a);
}

template <bool CS4, int KIND>
static void up_conv_launch(const UpArgs& a, dim3 grid, size_t lds, hipStream_t s) {
  if (a.ntw == 1) up_launch(up_conv_kernel<CS4, 1, KIND>, grid, lds, s, a);
  else if (a.ntw == 2) up_launch(up_conv_kernel<CS4, 2, KIND>, grid, lds, s, a);
  else if constexpr (KIND != UP_DGRAD) up_launch(up_conv_kernel<CS4, 4, KIND>, grid, lds, s, a);      // (up_check: no 4 n-tile dgrad)
}

void launch_upconv_fwd(const UpArgs& a, hipStream_t s) {
  const std::string w("upconv_fwd");
  const unsigned blocks = up_check(a, UP_FWD, w);
  if (up_bad_ptr(a.x, a.Cs_in)) throw std::invalid_argument(w + ": input pointer (null or misaligned)");
  if (up_bad_ptr(a.out, a.Cs_out)) throw std::invalid_argument(w + ": output pointer (null or misaligned)");
  if (a.bias && (reinterpret_cast<uintptr_t>(a.bias) & 3)) throw std::invalid_argument(w + ": bias pointer (misaligned)");
  if (!blocks) return;
  const dim3 grid(blocks, up_cdiv(up_cdiv(a.Cout, 16), a.ntw));
  const size_t lds = up_lds_bytes(a, UP_FWD, a.R, a.kc);
  if (a.Cs_in == 4) up_conv_launch<true, UP_FWD>(a, grid, lds, s);
  else up_conv_launch<false, UP_FWD>(a, grid, lds, s);
}

void launch_upconv_dgrad(const UpArgs& a, hipStream_t s) {
  const std::string w("upconv_dgrad");
  const unsigned blocks = up_check(a, UP_DGRAD, w);
  if (up_bad_ptr(a.dt, a.Cs_out)) throw std::invalid_argument(w + ": gradient pointer (null or misaligned)");
  const BwdThrough& t = a.bt;
  if (t.pH != a.H || t.pW != a.W || t.pC != a.Cin || t.pCs != a.Cs_in)
    throw std::invalid_argument(w + ": the feeding stage's BwdThrough geometry differs from the input grid");
  if (up_bad_ptr(t.dy, a.Cs_in)) throw std::invalid_argument(w + ": BwdThrough dy (null or misaligned)");
  if (t.prev_relu && up_bad_ptr(t.prev_out, a.Cs_in)) throw std::invalid_argument(w + ": BwdThrough prev_out (null or misaligned)");
  if (t.wt && (long long)a.B * a.H * a.W * a.Cs_in * 2 >= (1LL << 31))
    throw std::invalid_argument(w + ": write-through stores need a gradient buffer below 2 GB");
  if (t.drop_thr && !(t.drop_scale >= 1.f)) throw std::invalid_argument(w + ": BwdThrough dropout scale");
  if (!blocks) return;
  const dim3 grid(blocks, up_cdiv(up_cdiv(a.Cin, 16), a.ntw));
  up_conv_launch<false, UP_DGRAD>(a, grid, up_lds_bytes(a, UP_DGRAD, a.R, a.kc), s);
}

void launch_upconv_wgrad(const UpArgs& a, hipStream_t s) {
  const std::string w("upconv_wgrad");
  const unsigned blocks = up_check(a, UP_WGRAD, w);
  if (up_bad_ptr(a.x, a.Cs_in)) throw std::invalid_argument(w + ": input pointer (null or misaligned)");
  if (up_bad_ptr(a.dt, a.Cs_out)) throw std::invalid_argument(w + ": gradient pointer (null or misaligned)");
  if (!a.slab || (reinterpret_cast<uintptr_t>(a.slab) & 3)) throw std::invalid_argument(w + ": slab pointer (null or misaligned)");
  if (a.slab_ld < (a.has_bias ? up_bias_off(a) + a.Cout : a.KH * a.KW * a.Cin * a.Cout))
    throw std::invalid_argument(w + ": slab row stride");
  if (!blocks) {
    if (a.S) throw std::invalid_argument(w + ": slabs of an empty batch");
    return;
  }
  if (a.S <= 0 || a.pairs_per_slab <= 0 || (long long)a.S * a.pairs_per_slab > 0xffffffffLL || (long long)a.S * a.pairs_per_slab < blocks ||
      (long long)(a.S - 1) * a.pairs_per_slab >= blocks)
    throw std::invalid_argument(w + ": S slabs of pairs_per_slab (image, row block) pairs must cover the pairs, none empty");
  const dim3 grid(a.S, up_cdiv(up_cdiv(a.KH * a.KW * a.Cs_in, 16), 4 * UP_MTW), up_cdiv(up_cdiv(a.Cout, 16), a.ntw));
  const size_t lds = up_lds_bytes(a, UP_WGRAD, a.R, 0);
  const bool cs4 = a.Cs_in == 4;
  if (a.ntw == 1) cs4 ? up_launch(up_wgrad_kernel<true, 1>, grid, lds, s, a) : up_launch(up_wgrad_kernel<false, 1>, grid, lds, s, a);
  else if (a.ntw == 2) cs4 ? up_launch(up_wgrad_kernel<true, 2>, grid, lds, s, a) : up_launch(up_wgrad_kernel<false, 2>, grid, lds, s, a);
  else cs4 ? up_launch(up_wgrad_kernel<true, 4>, grid, lds, s, a) : up_launch(up_wgrad_kernel<false, 4>, grid, lds, s, a);
}

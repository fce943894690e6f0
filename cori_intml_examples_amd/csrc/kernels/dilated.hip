// Dilated convolution (Keras Conv2D, dilation_rate d >= 2, strides 1): forward, the gradient to its
// input, the weight and bias gradient (DilArgs, args.h).  ke = (k - 1) * d + 1 is the effective extent.
//
//   dil_fwd    out[b, y, x, n] = bf16(A(bias[n] + sum_{ky, kx, c} w[ky, kx, c, n] * x[b, y + ky*d - pad_t, x + kx*d - pad_l, c]))
//   dil_dgrad  dx[b, y, x, c]  = sum_{ky, kx, n} w[ky, kx, c, n] * dt[b, y + pad_t - ky*d, x + pad_l - kx*d, n]
//              handed to the feeding stage's BwdThrough (its dropout mask, relu mask and bf16 rounding)
//   dil_wgrad  dW[ky, kx, c, n] = sum_{b, y, x} x[b, y + ky*d - pad_t, x + kx*d - pad_l, c] * dt[b, y, x, n]
//              db[n]            = sum_{b, y, x} dt[b, y, x, n]
//
// All three are implicit GEMMs on v_mfma_f32_16x16x32_bf16.  w is the fp32 master, rounded to bf16 as
// it is staged into LDS (no weight pack); accumulation is fp32 in one fixed order, without atomics: two
// launches are bit-identical.
//
// dil_fwd / dil_dgrad (one body, dil_conv_kernel): M = pixels, N = result channels, K = (tap, c) padded
// to a multiple of 32.  A workgroup takes one image, a block of R result rows (grid x) and a slice of
// ntw n-tiles (grid y).  LDS map: [k-group offset table][weight chunk][halo].
//   halo    (R - 1 + ke_h) rows x (Wr + ke_w - 1) pixels x xpix elements (xpix >= Ck: the conflict-free
//           pixel stride), staged ONCE; positions outside the source grid are zeros, so the tap loop has
//           no bounds branches and dilation costs nothing there: tap (ky, kx) of pixel (r, x) is halo
//           pixel (r + ky*d, x + kx*d).  dil_dgrad stages dt with the padding ke - 1 - pad and walks the
//           taps flipped with c / n exchanged (done while the weights are staged): the same body.
//   table   one halo offset per 8 consecutive k (one tap, 8 channels: a lane's fragment is ONE 16-byte
//           read; Ck == 4: per 4 k, a fragment is two taps, two 8-byte reads).  The k padding points at
//           offset 0 -- in range, and its weights are zeros.
//   weights kc k-steps x ntw n-tiles in fragment order [(ks, nt)][lane][8]; K is walked in chunks of kc
//           k-steps when the slice does not fit (one chunk: staged once for all passes).
// The MFMA runs TRANSPOSED (weights as the A operand, pixels as B): a lane then holds 4 consecutive
// channels of ONE pixel, one exchange with lane ^ 16 makes 8, and the even 16-lane groups store 16
// bytes.  A wave keeps DIL_MTW m-tiles (16 consecutive pixels of the block, wrapping across rows) x ntw
// n-tiles; blocks of more than 4 * DIL_MTW m-tiles take further passes.  (dil_dgrad has no 4 n-tile
// instance: its epilogue, the BwdThrough of every chunk, would run out of scalar registers.)
//
// dil_wgrad: M = (tap, c), N = Cout, K = pixels.  Workgroup (g, my, nz) takes the (image, row block)
// pairs [g * pairs_per_slab, ...), stages the x halo and the block's dt rows ([pixel][channel], zero
// rows up to a multiple of 32 pixels) of each pair, and keeps its accumulators -- wave w: m-tiles
// my * 4 * DIL_MTW + w + 4u, u < DIL_MTW, x ntw n-tiles -- in registers across the pairs.  Both
// operands need k = pixel runs per lane out of [pixel][channel] tiles: transposed LDS reads
// (ds_read_b64_tr_b16), each lane addressing ITS pixel's tap-shifted halo position.  The bias
// gradient is one more MFMA per n-tile with an all-ones A fragment (wave 3 of my == 0).  It writes ONE
// slab row: [KH][KW][Cin][Cout] (Keras order, unpadded), then on the next 16-byte boundary [Cout]; the
// slab reduction takes both as identity descriptors.
#include <cstdint>
#include <stdexcept>
#include <string>
#include <tuple>

#include "args.h"
#include "bwd_through.h"

template <int VEC> struct DilVec;
template <> struct DilVec<8> {
  typedef bf16x8 T;
  __device__ __forceinline__ static T load_if(bool ok, const bf16* p, const bf16* safe) { return load_bf16x8_if(ok, p, safe); }
};
template <> struct DilVec<4> {
  typedef bf16x4 T;
  __device__ __forceinline__ static T load_if(bool ok, const bf16* p, const bf16* safe) { return load_bf16x4_if(ok, p, safe); }
};

__host__ __device__ __forceinline__ int dil_a16(int v) { return (v + 15) & ~15; }
__host__ __device__ __forceinline__ int dil_cdiv(int a, int b) { return (a + b - 1) / b; }

// What a launch kind contracts over and produces: the source grid [sh, sw, scs] (x or dt), the result
// grid [rh, rw], the result channels n (their stride ns), and where result pixel (0, 0)'s first tap lies
// in the source grid (-oy, -ox).
struct DilGeo {
  int sh, sw, scs, ck, rh, rw, n, ns, oy, ox, ke_h, ke_w;
};
__host__ __device__ __forceinline__ DilGeo dil_geo(const DilArgs& a, int kind) {
  DilGeo g;
  g.ke_h = (a.KH - 1) * a.dil + 1, g.ke_w = (a.KW - 1) * a.dil + 1;
  if (kind == DIL_DGRAD) {
    g.sh = a.Ho, g.sw = a.Wo, g.scs = g.ck = a.Cs_out, g.rh = a.H, g.rw = a.W, g.n = a.Cin, g.ns = a.Cs_in;
    g.oy = g.ke_h - 1 - a.pad_t, g.ox = g.ke_w - 1 - a.pad_l;
  } else {
    g.sh = a.H, g.sw = a.W, g.scs = g.ck = a.Cs_in, g.rh = a.Ho, g.rw = a.Wo, g.n = a.Cout, g.ns = a.Cs_out;
    g.oy = a.pad_t, g.ox = a.pad_l;
  }
  return g;
}
__host__ __device__ __forceinline__ int dil_ks(const DilArgs& a, int ck) { return dil_cdiv(a.KH * a.KW * ck, 32); }
// dil_wgrad's staged dt rows: all n-tiles' columns defined (zeros behind Cs_out), 16 bytes of padding
__host__ __device__ __forceinline__ int dil_dpix(const DilArgs& a) { return dil_a16(a.Cs_out) + 8; }
// elements of a staged halo, to a 16-byte boundary
__host__ __device__ __forceinline__ size_t dil_halo_elems(int hr, int hc, int xpix) { return ((size_t)hr * hc * xpix + 7) & ~(size_t)7; }
__host__ __device__ __forceinline__ int dil_bias_off(const DilArgs& a) { return (a.KH * a.KW * a.Cin * a.Cout + 3) & ~3; }

// Stage ``npx`` = hr * hc pixels: pixel (r, c) is source pixel (r + oy, c + ox) of [sh, sw, scs], its first
// ``ncg`` VEC-channel groups (groups >= src_ncg and pixels outside the grid: zeros), at dst + pixel * dpix.
template <int VEC>
__device__ __forceinline__ void dil_stage(bf16* dst, int dpix, const bf16* src, int scs, int hr, int hc, int ncg,
                                          int src_ncg, int oy, int ox, int sh, int sw) {
  typedef typename DilVec<VEC>::T V;
  staged_copy<4, V>(
      hr * hc * ncg, (int)threadIdx.x, DIL_THREADS,
      [&](int i) {
        const int t = i / ncg, cg = i - t * ncg;
        const int r = t / hc, c = t - r * hc;
        const int y = r + oy, x = c + ox;
        const bool ok = y >= 0 && x >= 0 && y < sh && x < sw && cg < src_ncg;
        return DilVec<VEC>::load_if(ok, src + ((size_t)y * sw + x) * scs + cg * VEC, src);
      },
      [&](int i, const V& v) {
        const int t = i / ncg, cg = i - t * ncg;
        *reinterpret_cast<V*>(dst + (size_t)t * dpix + cg * VEC) = v;
      });
}

template <bool CS4, int NTW, int KIND>
__global__ __launch_bounds__(DIL_THREADS) void dil_conv_kernel(const DilArgs a) {
  constexpr int VEC = CS4 ? 4 : 8;
  extern __shared__ __attribute__((aligned(16))) unsigned char dil_smem[];
  const DilGeo G = dil_geo(a, KIND);
  const int ntaps = a.KH * a.KW, ck = G.ck, KS = dil_ks(a, ck), nq = KS * (32 / VEC);
  int* toff = reinterpret_cast<int*>(dil_smem);
  bf16* wl = reinterpret_cast<bf16*>(dil_smem + dil_a16(nq * 4));
  bf16* hx = wl + (size_t)a.kc * NTW * 512;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 15, g = lane >> 4;
  const int nrb = dil_cdiv(G.rh, a.R);
  const int b = blockIdx.x / nrb, r0 = (blockIdx.x - b * nrb) * a.R;
  const int Rv = min(a.R, G.rh - r0);
  const int hr = Rv - 1 + G.ke_h, hc = G.rw + G.ke_w - 1;
  const int nbase = blockIdx.y * NTW * 16;
  // the halo offset of every VEC consecutive k: (tap, channel group); the padding: offset 0
  for (int q = tid; q < nq; q += DIL_THREADS) {
    const int k0 = q * VEC, tap = k0 / ck, ky = tap / a.KW, kx = tap - ky * a.KW;
    toff[q] = tap < ntaps ? ((ky * a.dil) * hc + kx * a.dil) * a.xpix + (k0 - tap * ck) : 0;
  }
  const bf16* src = KIND == DIL_FWD ? a.x : a.dt;
  dil_stage<VEC>(hx, a.xpix, src + (size_t)b * G.sh * G.sw * G.scs, G.scs, hr, hc, ck / VEC, ck / VEC, r0 - G.oy, -G.ox,
                 G.sh, G.sw);
  const uint32_t step = a.st ? (uint32_t)a.st->t : 0u;
  const int npix = Rv * G.rw, nmt = dil_cdiv(npix, 16), nchunks = dil_cdiv(KS, a.kc);
  for (int mt0 = 0; mt0 < nmt; mt0 += 4 * DIL_MTW) {
    f32x4 acc[DIL_MTW][NTW];
    int pixoff[DIL_MTW];
#pragma unroll
    for (int u = 0; u < DIL_MTW; ++u) {
#pragma unroll
      for (int nt = 0; nt < NTW; ++nt) acc[u][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
      int p = (mt0 + wave + 4 * u) * 16 + i;
      if (p >= npix) p = 0;      // (a tail lane: any pixel of the block; its results are not stored)
      const int r = p / G.rw;
      pixoff[u] = (r * hc + (p - r * G.rw)) * a.xpix;
    }
    for (int ch = 0; ch < nchunks; ++ch) {
      const int ks0 = ch * a.kc, kcn = min(a.kc, KS - ks0);
      if (nchunks > 1 || mt0 == 0) {
        __syncthreads();      // (the previous chunk's readers are done)
        // the weight chunk in fragment order, rounded to bf16: element j of lane (i, g) of (ks, nt) is
        // W[k = 32 ks + 8 g + j][n = nbase + 16 nt + i]; zeros in the k and n padding.  Thread order follows
        // the master's contiguous axis: n for the forward, the contraction channel for the dgrad.
        for (int e = tid; e < kcn * NTW * 512; e += DIL_THREADS) {
          const int t = e >> 9;
          int ei, ej, eg;
          if (KIND == DIL_FWD) ei = e & 15, ej = (e >> 4) & 7, eg = (e >> 7) & 3;
          else ej = e & 7, eg = (e >> 3) & 3, ei = (e >> 5) & 15;
          const int ksl = t / NTW, nt = t - ksl * NTW;
          const int k = (ks0 + ksl) * 32 + 8 * eg + ej, n = nbase + nt * 16 + ei;
          const int tap = k / ck, c = k - tap * ck;
          float v = 0.f;
          if (tap < ntaps && n < G.n) {
            if (KIND == DIL_FWD) {
              if (c < a.Cin) v = a.w[((size_t)tap * a.Cin + c) * a.Cout + n];
            } else {
              if (c < a.Cout) v = a.w[((size_t)(ntaps - 1 - tap) * a.Cin + n) * a.Cout + c];
            }
          }
          wl[((size_t)t * 64 + eg * 16 + ei) * 8 + ej] = f2bf(v);
        }
        __syncthreads();      // (first chunk: the table and the halo too)
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
        for (int u = 0; u < DIL_MTW; ++u) {
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
    // half of the 8-channel chunk, and the even groups store it.  (nt outermost: what depends on the
    // channel alone -- the bias, the padding channels' mask -- is live for one n-tile at a time.)
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt) {
      const int n0 = nbase + nt * 16 + 4 * g;
      float bv[4];
      uint32_t keep[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool in = n0 + j < G.n;
        bv[j] = (KIND == DIL_FWD && a.bias) ? a.bias[in ? n0 + j : 0] : 0.f;
        keep[j] = in ? 0xffffffffu : 0u;
      }
#pragma unroll
      for (int u = 0; u < DIL_MTW; ++u) {
        const int p = (mt0 + wave + 4 * u) * 16 + i;      // (an m-tile past the block: every p >= npix)
        const size_t qi = ((size_t)b * G.rh + r0) * G.rw + p;      // (a block's pixels are consecutive in the image)
        float v[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float f = acc[u][nt][j];
          if (KIND == DIL_FWD) {
            f += bv[j];
            if (a.relu) f = fmaxf(f, 0.f);
          }
          v[j] = __uint_as_float(__float_as_uint(f) & keep[j]);      // (padding channels: zeros)
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) v[4 + j] = __shfl_xor(v[j], 16);
        if ((g & 1) || p >= npix || n0 >= G.ns) continue;
        if (KIND == DIL_FWD) {
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

__device__ __forceinline__ bf16x4 dil_tr_read(const bf16* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4bf16(LDS_PTR(bf16x4, p));
}

template <bool CS4, int NTW>
__global__ __launch_bounds__(DIL_THREADS) void dil_wgrad_kernel(const DilArgs a) {
  constexpr int VEC = CS4 ? 4 : 8;
  extern __shared__ __attribute__((aligned(16))) unsigned char dil_smem[];
  const DilGeo G = dil_geo(a, DIL_WGRAD);
  const int ntaps = a.KH * a.KW, cs = a.Cs_in, mtot = ntaps * cs;
  const int hc = a.Wo + G.ke_w - 1, dpix = dil_dpix(a);
  bf16* hx = reinterpret_cast<bf16*>(dil_smem);                      // [hr][hc][xpix]
  bf16* hd = hx + dil_halo_elems(a.R - 1 + G.ke_h, hc, a.xpix);      // [32-multiple of pixels][dpix]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 15, g = lane >> 4;
  const int nbase = blockIdx.z * NTW * 16, mtb = blockIdx.y * 4 * DIL_MTW + wave;
  const int ncols = dil_a16(a.Cs_out);      // the staged dt columns
  f32x4 acc[DIL_MTW][NTW], bacc[NTW];
  int aoff[DIL_MTW];
#pragma unroll
  for (int u = 0; u < DIL_MTW; ++u) {
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt) acc[u][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    // the lane's 4 rows m of the tile, one tap's channels c .. c + 3: its tap shift in the halo (a padding
    // row: offset 0 -- in range, the row is not stored)
    const int m = (mtb + 4 * u) * 16 + 4 * (i & 3);
    const int tap = m / cs, ky = tap / a.KW, kx = tap - ky * a.KW;
    aoff[u] = m < mtot ? ((ky * a.dil) * hc + kx * a.dil) * a.xpix + (m - tap * cs) : 0;
  }
#pragma unroll
  for (int nt = 0; nt < NTW; ++nt) bacc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bool do_bias = a.has_bias && blockIdx.y == 0 && wave == 3;
  bf16x8 ones;
#pragma unroll
  for (int j = 0; j < 8; ++j) ones[j] = f2bf(1.f);
  const int nrb = dil_cdiv(a.Ho, a.R);
  const long long npairs = (long long)a.B * nrb;
  const long long p_lo = (long long)blockIdx.x * a.pairs_per_slab;
  const long long p_hi = min(p_lo + a.pairs_per_slab, npairs);
  for (long long pr = p_lo; pr < p_hi; ++pr) {
    const int b = (int)(pr / nrb), r0 = (int)(pr - (long long)b * nrb) * a.R;
    const int Rv = min(a.R, a.Ho - r0);
    const int npix = Rv * a.Wo, npix32 = (npix + 31) & ~31;
    __syncthreads();      // (the previous pair's readers are done)
    dil_stage<VEC>(hx, a.xpix, a.x + (size_t)b * a.H * a.W * cs, cs, Rv - 1 + G.ke_h, hc, cs / VEC, cs / VEC, r0 - a.pad_t,
                   -a.pad_l, a.H, a.W);
    dil_stage<8>(hd, dpix, a.dt + ((size_t)b * a.Ho + r0) * a.Wo * a.Cs_out, a.Cs_out, 1, npix32, ncols / 8, a.Cs_out / 8,
                 0, 0, 1, npix);
    __syncthreads();
    for (int p0 = 0; p0 < npix32; p0 += 32) {
      // the lane's two pixels of the 32 (rows of the transposed reads); past the block: dt rows of zeros
      // against any pixel of the block
      const int pl = p0 + 8 * g + (i >> 2), ph = pl + 4;
      const int al = pl < npix ? pl : 0, ah = ph < npix ? ph : 0;
      const int xl = ((al / a.Wo) * hc + al % a.Wo) * a.xpix, xh = ((ah / a.Wo) * hc + ah % a.Wo) * a.xpix;
      bf16x8 bfr[NTW];
#pragma unroll
      for (int nt = 0; nt < NTW; ++nt) {
        // (an n-tile past the staged columns: a defined address, the tile is not stored)
        const int col = nbase + nt * 16 < ncols ? nbase + nt * 16 + 4 * (i & 3) : 0;
        const bf16x4 lo = dil_tr_read(hd + (size_t)pl * dpix + col);
        const bf16x4 hi = dil_tr_read(hd + (size_t)ph * dpix + col);
        bfr[nt] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
      }
#pragma unroll
      for (int u = 0; u < DIL_MTW; ++u) {
        const bf16x4 lo = dil_tr_read(hx + xl + aoff[u]);
        const bf16x4 hi = dil_tr_read(hx + xh + aoff[u]);
        const bf16x8 afr = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) acc[u][nt] = mfma16(afr, bfr[nt], acc[u][nt]);
      }
      if (do_bias) {
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) bacc[nt] = mfma16(ones, bfr[nt], bacc[nt]);
      }
    }
  }
  // lane (i, g) holds rows m = 16 mt + 4 g + j of column n = nbase + 16 nt + i
  float* row = a.slab + (size_t)blockIdx.x * a.slab_ld;
#pragma unroll
  for (int nt = 0; nt < NTW; ++nt) {
    const int n = nbase + nt * 16 + i;
    if (n >= a.Cout) continue;
#pragma unroll
    for (int u = 0; u < DIL_MTW; ++u) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int m = (mtb + 4 * u) * 16 + 4 * g + j;
        const int tap = m / cs, c = m - tap * cs;
        if (m < mtot && c < a.Cin) row[((size_t)tap * a.Cin + c) * a.Cout + n] = acc[u][nt][j];
      }
    }
    if (do_bias && g == 0) row[dil_bias_off(a) + n] = bacc[nt][0];
  }
}

// ---------------------------------------------------------------------------------------------------
// n-tiles per workgroup for n result channels (dil_dgrad: at most 2)
int dil_ntw(int n, int kind) { return n <= 16 ? 1 : (n <= 32 || kind == DIL_DGRAD) ? 2 : 4; }

// LDS bytes of a launch with R rows per block (fwd / dgrad: and kc k-steps of weights)
size_t dil_lds_bytes(const DilArgs& a, int kind, int R, int kc) {
  const DilGeo G = dil_geo(a, kind);
  if (kind == DIL_WGRAD)
    return dil_halo_elems(R - 1 + G.ke_h, a.Wo + G.ke_w - 1, a.xpix) * 2 + (size_t)((R * a.Wo + 31) & ~31) * dil_dpix(a) * 2;
  const int nq = dil_ks(a, G.ck) * (G.ck == 4 ? 8 : 4);
  return (size_t)dil_a16(nq * 4) + (size_t)kc * a.ntw * 1024 + dil_halo_elems(R - 1 + G.ke_h, G.rw + G.ke_w - 1, a.xpix) * 2;
}

static void dil_check_geometry(const DilArgs& a, int kind, const std::string& w) {
  if (kind != DIL_FWD && kind != DIL_DGRAD && kind != DIL_WGRAD) throw std::invalid_argument(w + ": kind");
  if (a.dil < 2) throw std::invalid_argument(w + ": dilation_rate must be at least 2 (1 is the ordinary conv kernels')");
  if (a.stride != 1) throw std::invalid_argument(w + ": a dilated convolution has strides 1");
  if (a.Cs_in != 4 && (a.Cs_in <= 0 || a.Cs_in % 8 || a.Cs_in > 2048))
    throw std::invalid_argument(w + ": the input's channel stride must be 4 or a multiple of 8 (at most 2048)");
  if (a.Cs_out <= 0 || a.Cs_out % 8 || a.Cs_out > 2048)
    throw std::invalid_argument(w + ": the output's channel stride must be a multiple of 8 (at most 2048)");
  if (a.Cin <= 0 || a.Cin > a.Cs_in || a.Cout <= 0 || a.Cout > a.Cs_out)
    throw std::invalid_argument(w + ": channels must be in [1, channel stride]");
  if (a.B < 0 || a.H <= 0 || a.W <= 0 || a.Ho <= 0 || a.Wo <= 0) throw std::invalid_argument(w + ": batch / grid sizes");
  if (a.KH <= 0 || a.KW <= 0 || a.KH * a.KW > 1024 || a.dil > 1024) throw std::invalid_argument(w + ": kernel size / dilation");
  const DilGeo G = dil_geo(a, kind);
  if (a.pad_t < 0 || a.pad_l < 0 || a.pad_t >= G.ke_h || a.pad_l >= G.ke_w)
    throw std::invalid_argument(w + ": the top / left padding must be smaller than the effective kernel");
  if ((long long)a.H * a.W * a.Cs_in > 0x7fffffffLL || (long long)a.Ho * a.Wo * a.Cs_out > 0x7fffffffLL)
    throw std::invalid_argument(w + ": one image must stay below 2^31 elements");
  if ((long long)a.KH * a.KW * a.Cin * a.Cout > 0x7ffffff0LL) throw std::invalid_argument(w + ": kernel elements");
  if (a.ntw != 1 && a.ntw != 2 && a.ntw != 4) throw std::invalid_argument(w + ": n-tiles per workgroup must be 1, 2 or 4");
  const int vec = G.ck == 4 ? 4 : 8;
  if (kind == DIL_DGRAD && a.ntw == 4) throw std::invalid_argument(w + ": dil_dgrad takes 1 or 2 n-tiles per workgroup");
  if (kind == DIL_DGRAD && a.Cs_in == 4) throw std::invalid_argument(w + ": no input gradient for a 4-lane model input");
  if (a.xpix < G.ck || a.xpix % vec || a.xpix > G.ck + 64)
    throw std::invalid_argument(w + ": the halo pixel stride must be a multiple of the vector width in [Ck, Ck + 64]");
}

// (R, kc): rows per block -- the fewest row blocks per image (balanced) whose LDS stage fits
// DIL_LDS_BUDGET (fwd / dgrad: with at least two k-steps of weights, or all of them) and that leave at
// least ``want`` workgroups; 1 where nothing gives that many; 0 where not even one row fits -- and the
// k-steps of weights that then fit (wgrad: 0).
std::tuple<int, int> dil_cfg(const DilArgs& a, int kind, int want) {
  dil_check_geometry(a, kind, "dil_cfg");
  const DilGeo G = dil_geo(a, kind);
  const int KS = dil_ks(a, G.ck), kmin = kind == DIL_WGRAD ? 0 : (KS < 2 ? KS : 2);
  long long per = kind == DIL_WGRAD ? (long long)dil_cdiv(dil_cdiv(a.KH * a.KW * a.Cs_in, 16), 4 * DIL_MTW) : 1;
  per *= dil_cdiv(dil_cdiv(G.n, 16), a.ntw);
  int R = 0;
  if (dil_lds_bytes(a, kind, 1, kmin) <= DIL_LDS_BUDGET) {
    R = 1;
    for (int c = 1; c <= G.rh; ++c) {
      const int r = dil_cdiv(G.rh, c);
      if (dil_lds_bytes(a, kind, r, kmin) > DIL_LDS_BUDGET) continue;
      if ((long long)a.B * dil_cdiv(G.rh, r) * per < want) continue;
      R = r;
      break;
    }
  }
  int kc = 0;
  if (R > 0 && kind != DIL_WGRAD) {
    const size_t left = DIL_LDS_BUDGET - dil_lds_bytes(a, kind, R, 0);
    kc = (int)(left / ((size_t)a.ntw * 1024));
    if (kc > KS) kc = KS;
  }
  return std::make_tuple(R, kc);
}

static bool dil_bad_ptr(const void* p, int Cs) { return !p || (reinterpret_cast<uintptr_t>(p) & (Cs == 4 ? 7 : 15)); }

// the checks every launch shares; returns the grid's x (image, row block) count
static unsigned dil_check(const DilArgs& a, int kind, const std::string& w) {
  dil_check_geometry(a, kind, w);
  const DilGeo G = dil_geo(a, kind);
  if (a.R <= 0 || a.R > G.rh) throw std::invalid_argument(w + ": rows per block must be in [1, rows]");
  if (kind != DIL_WGRAD && (a.kc <= 0 || a.kc > dil_ks(a, G.ck)))
    throw std::invalid_argument(w + ": the weight chunk must be in [1, k-steps]");
  if (dil_lds_bytes(a, kind, a.R, a.kc) > DIL_LDS_BUDGET)
    throw std::invalid_argument(w + ": the block's LDS stage exceeds " + std::to_string(DIL_LDS_BUDGET) + " bytes");
  if (!a.w || (reinterpret_cast<uintptr_t>(a.w) & 3)) throw std::invalid_argument(w + ": weight pointer (null or misaligned)");
  const long long blocks = (long long)a.B * dil_cdiv(G.rh, a.R);
  if (blocks > 0x7fffffffLL) throw std::invalid_argument(w + ": too many blocks for one launch");
  return (unsigned)blocks;
}

template <class Kn>
static void dil_launch(Kn k, dim3 grid, size_t lds, hipStream_t s, const DilArgs& a) {
  if (lds > 65536) (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(k, grid, dim3(DIL_THREADS), lds, s, a);
}

template <bool CS4, int KIND>
static void dil_conv_launch(const DilArgs& a, dim3 grid, size_t lds, hipStream_t s) {
  if (a.ntw == 1) dil_launch(dil_conv_kernel<CS4, 1, KIND>, grid, lds, s, a);
  else if (a.ntw == 2) dil_launch(dil_conv_kernel<CS4, 2, KIND>, grid, lds, s, a);
  else if constexpr (KIND != DIL_DGRAD) dil_launch(dil_conv_kernel<CS4, 4, KIND>, grid, lds, s, a);      // (dil_check: no 4 n-tile dgrad)
}

void launch_dil_fwd(const DilArgs& a, hipStream_t s) {
  const std::string w("dil_fwd");
  const unsigned blocks = dil_check(a, DIL_FWD, w);
  if (dil_bad_ptr(a.x, a.Cs_in)) throw std::invalid_argument(w + ": input pointer (null or misaligned)");
  if (dil_bad_ptr(a.out, a.Cs_out)) throw std::invalid_argument(w + ": output pointer (null or misaligned)");
  if (a.bias && (reinterpret_cast<uintptr_t>(a.bias) & 3)) throw std::invalid_argument(w + ": bias pointer (misaligned)");
  if (!blocks) return;
  const dim3 grid(blocks, dil_cdiv(dil_cdiv(a.Cout, 16), a.ntw));
  const size_t lds = dil_lds_bytes(a, DIL_FWD, a.R, a.kc);
  if (a.Cs_in == 4) dil_conv_launch<true, DIL_FWD>(a, grid, lds, s);
  else dil_conv_launch<false, DIL_FWD>(a, grid, lds, s);
}

void launch_dil_dgrad(const DilArgs& a, hipStream_t s) {
  const std::string w("dil_dgrad");
  const unsigned blocks = dil_check(a, DIL_DGRAD, w);
  if (dil_bad_ptr(a.dt, a.Cs_out)) throw std::invalid_argument(w + ": gradient pointer (null or misaligned)");
  const BwdThrough& t = a.bt;
  if (t.pH != a.H || t.pW != a.W || t.pC != a.Cin || t.pCs != a.Cs_in)
    throw std::invalid_argument(w + ": the feeding stage's BwdThrough geometry differs from the input grid");
  if (dil_bad_ptr(t.dy, a.Cs_in)) throw std::invalid_argument(w + ": BwdThrough dy (null or misaligned)");
  if (t.prev_relu && dil_bad_ptr(t.prev_out, a.Cs_in)) throw std::invalid_argument(w + ": BwdThrough prev_out (null or misaligned)");
  if (t.wt && (long long)a.B * a.H * a.W * a.Cs_in * 2 >= (1LL << 31))
    throw std::invalid_argument(w + ": write-through stores need a gradient buffer below 2 GB");
  if (t.drop_thr && !(t.drop_scale >= 1.f)) throw std::invalid_argument(w + ": BwdThrough dropout scale");
  if (!blocks) return;
  const dim3 grid(blocks, dil_cdiv(dil_cdiv(a.Cin, 16), a.ntw));
  dil_conv_launch<false, DIL_DGRAD>(a, grid, dil_lds_bytes(a, DIL_DGRAD, a.R, a.kc), s);
}

void launch_dil_wgrad(const DilArgs& a, hipStream_t s) {
  const std::string w("dil_wgrad");
  const unsigned blocks = dil_check(a, DIL_WGRAD, w);
  if (dil_bad_ptr(a.x, a.Cs_in)) throw std::invalid_argument(w + ": input pointer (null or misaligned)");
  if (dil_bad_ptr(a.dt, a.Cs_out)) throw std::invalid_argument(w + ": gradient pointer (null or misaligned)");
  if (!a.slab || (reinterpret_cast<uintptr_t>(a.slab) & 3)) throw std::invalid_argument(w + ": slab pointer (null or misaligned)");
  if (a.slab_ld < (a.has_bias ? dil_bias_off(a) + a.Cout : a.KH * a.KW * a.Cin * a.Cout))
    throw std::invalid_argument(w + ": slab row stride");
  if (!blocks) {
    if (a.S) throw std::invalid_argument(w + ": slabs of an empty batch");
    return;
  }
  if (a.S <= 0 || a.pairs_per_slab <= 0 || (long long)a.S * a.pairs_per_slab < blocks ||
      (long long)(a.S - 1) * a.pairs_per_slab >= blocks)
    throw std::invalid_argument(w + ": S slabs of pairs_per_slab (image, row block) pairs must cover the pairs, none empty");
  const dim3 grid(a.S, dil_cdiv(dil_cdiv(a.KH * a.KW * a.Cs_in, 16), 4 * DIL_MTW), dil_cdiv(dil_cdiv(a.Cout, 16), a.ntw));
  const size_t lds = dil_lds_bytes(a, DIL_WGRAD, a.R, 0);
  const bool cs4 = a.Cs_in == 4;
  if (a.ntw == 1) cs4 ? dil_launch(dil_wgrad_kernel<true, 1>, grid, lds, s, a) : dil_launch(dil_wgrad_kernel<false, 1>, grid, lds, s, a);
  else if (a.ntw == 2) cs4 ? dil_launch(dil_wgrad_kernel<true, 2>, grid, lds, s, a) : dil_launch(dil_wgrad_kernel<false, 2>, grid, lds, s, a);
  else cs4 ? dil_launch(dil_wgrad_kernel<true, 4>, grid, lds, s, a) : dil_launch(dil_wgrad_kernel<false, 4>, grid, lds, s, a);
}

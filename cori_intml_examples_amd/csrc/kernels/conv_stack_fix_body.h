// conv_stack_kernel's specialised path (conv_stack_body.h) with the WHOLE geometry of the stack a
// compile-time signature (stack_sig.h): the layer sequence is unrolled, each layer body runs
// through StackGeoFix, the band's rows are selects between two constants (sp = blockIdx & 1), and
// the prologue, the border zeroing and the store-out divide by constants.  The structure is
// conv_stack_kernel's, statement for statement: the one-batch prologue, the untracked LDS-DMA
// weight prefetch with its explicit vmcnt(0), the two code planes, the barriers; the k order, MFMA
// order, rounding points, argmax rule and dropout counters are the layer body's own.  The k16 tail
// and the write-through stores are compiled in.  Run-time: the pointers, B, seed, each layer's
// dropout threshold / scale / stream id, from_data, training, step_inc.  No fallback in here: the
// host launches this kernel only for args that equal the signature (conv_stack_fixed).
#pragma once
#include "conv_stack_body.h"
#include "stack_sig.h"

template <class SIG, int l> struct StackFixL;
template <class SIG> struct StackFixL<SIG, 0> { using T = typename SIG::L0; };
template <class SIG> struct StackFixL<SIG, 1> { using T = typename SIG::L1; };
template <class SIG> struct StackFixL<SIG, 2> { using T = typename SIG::L2; };

// what conv_stack_kernel's layer loop derives from the rows of layer l (and l + 1) for band sp
struct StackFixBand {
  int c0, c1, own0, own1, p0, roff, nr, obase, OH, ol, OW, ORS, OPS, wr0, wr1;
};
template <class SIG, int l>
constexpr StackFixBand stack_fix_band(int sp) {
  using S = typename StackFixL<SIG, l>::T;
  StackFixBand g{};
  g.c0 = S::row(sp, 0), g.c1 = S::row(sp, 1), g.own0 = S::row(sp, 2), g.own1 = S::row(sp, 3);
  g.p0 = g.c0 >> 1;
  g.roff = g.c0 - S::pad_t - S::row(sp, 4);
  g.nr = (g.c1 - g.c0) >> 1;
  if constexpr (l + 1 == SIG::n) {   // a compact image of the local stage rows
    g.obase = g.p0, g.OH = g.nr, g.ol = 0, g.OW = S::Wp, g.ORS = S::Wp, g.OPS = S::Cs_out;
  } else {                           // the next layer's halo image
    using N = typename StackFixL<SIG, l + 1>::T;
    g.obase = N::row(sp, 4), g.OH = N::row(sp, 5), g.ol = N::pad_l, g.OW = N::Wo + N::KW - 1;
    g.ORS = N::xrow, g.OPS = N::xpix;
  }
  g.wr0 = g.p0 - g.obase > 0 ? g.p0 - g.obase : 0;
  g.wr1 = g.p0 - g.obase + g.nr < g.OH ? g.p0 - g.obase + g.nr : g.OH;
  return g;
}
// band sp's value of field f (a constant where the two bands agree)
#define STACK_FIX_SEL(f) (sp ? G1.f : G0.f)

template <class SIG, int l>
__device__ __forceinline__ lbf16* stack_fix_out(LDS char* smem) {
  return (lbf16*)(smem + ((l & 1) ? SIG::off_buf0 : SIG::off_buf1));
}

// layer l: zero what the epilogue does not write of the output image, then the tiles
template <class SIG, int l>
__device__ __forceinline__ void stack_fix_tiles(const ConvStackArgs& A, LDS char* smem, int b, int sp, uint32_t step) {
  using S = typename StackFixL<SIG, l>::T;
  constexpr int NTH = SIG::nth;
  constexpr StackFixBand G0 = stack_fix_band<SIG, l>(0), G1 = stack_fix_band<SIG, l>(1);
  static_assert(S::Cs_out == S::Cout && S::Cout == S::NT * 16 && S::pool && S::KH == 3 && S::KW == 3 &&
                    (S::Wp & 3) == 0 && S::Cs_out % 16 == 0,
                "row-aligned FULL layers with 16-byte code vectors");
  static_assert(G0.wr0 < G0.wr1 && G1.wr0 < G1.wr1, "both bands write rows of the output image");
  static_assert(G0.OPS == G1.OPS && G0.ORS == G1.ORS && G0.OW == G1.OW && G0.ol == G1.ol, "one output layout");
  const int tid = threadIdx.x;
  const lbf16* in = (const lbf16*)(smem + ((l & 1) ? SIG::off_buf1 : SIG::off_buf0));
  lbf16* out = stack_fix_out<SIG, l>(smem);
  const int OH = STACK_FIX_SEL(OH), wr0 = STACK_FIX_SEL(wr0), wr1 = STACK_FIX_SEL(wr1);
  {
    LDS bf16x8* z = (LDS bf16x8*)out;
    const bf16x8 zero8 = zero_bf16x8();
    constexpr int vpp = G0.OPS >> 3, nrow = G0.ORS * vpp, nside = (G0.OW - S::Wp) * vpp, lcols = G0.ol * vpp;
    const int ntop = wr0 * nrow, nbot = (OH - wr1) * nrow;
    for (int i = tid; i < ntop + nbot; i += NTH) z[i < ntop ? i : wr1 * nrow + (i - ntop)] = zero8;
    if constexpr (nside > 0) {
      for (int i = tid; i < (wr1 - wr0) * nside; i += NTH) {
        const int rr = i / nside, c = i - rr * nside;
        z[(wr0 + rr) * nrow + (c < lcols ? c : c + S::Wp * vpp)] = zero8;
      }
    }
  }
  LDS uint8_t* codes = (LDS uint8_t*)(smem + ((l & 1) ? SIG::off_codes2 : SIG::off_codes));
  const lbf16* wl = (const lbf16*)(smem + SIG::off_w) + S::w_lds;
  const LDS float* lbias = (const LDS float*)(smem + SIG::off_bias);
  stack_layer_rows<S::NT, S::TM, S::Cs_in == 4, S::KS, true, 1, false, NTH / 64, StackGeoFix<S>>(
      A, A.L[l], b, STACK_FIX_SEL(c0), STACK_FIX_SEL(c1), STACK_FIX_SEL(roff), in, out, STACK_FIX_SEL(obase), OH,
      G0.ol, G0.ORS, G0.OPS, codes, wl, step, lbias + l * 64, false);
}

// layer l's owned stage rows (+ argmax codes) -> global, 16-byte write-through stores
template <class SIG, int l>
__device__ __forceinline__ void stack_fix_store(const ConvStackArgs& A, LDS char* smem, int b, int sp) {
  using S = typename StackFixL<SIG, l>::T;
  constexpr int NTH = SIG::nth;
  constexpr StackFixBand G0 = stack_fix_band<SIG, l>(0), G1 = stack_fix_band<SIG, l>(1);
  static_assert(G0.own1 - G0.own0 == G1.own1 - G1.own0, "an even partition of the stage rows");
  const StackLayer& L = A.L[l];
  const int tid = threadIdx.x;
  const lbf16* out = stack_fix_out<SIG, l>(smem);
  const int own0 = STACK_FIX_SEL(own0), p0 = STACK_FIX_SEL(p0), obase = STACK_FIX_SEL(obase);
  constexpr int cch = S::Cs_out >> 3, n = (G0.own1 - G0.own0) * S::Wp * cch;
  const size_t g0 = ((size_t)b * S::Hp + own0) * S::Wp * S::Cs_out;
  bf16* gout = L.out + g0;
  for (int i = tid; i < n; i += NTH) {
    const int pix = i / cch, c = (i - pix * cch) * 8;
    const int pyo = pix / S::Wp, px = pix - pyo * S::Wp;
    const u32x4 v =
        *reinterpret_cast<const LDS u32x4*>(out + ((own0 + pyo - obase) * G0.ORS + px + G0.ol) * G0.OPS + c);
    st_wt16(gout, (unsigned)(pix * S::Cs_out + c) * 2u, v);
  }
  if (L.code) {
    constexpr int nbytes = (G0.own1 - G0.own0) * S::Wp * S::Cs_out;
    uint8_t* gcb = L.code + g0;
    const LDS uint8_t* lcb =
        (const LDS uint8_t*)(smem + ((l & 1) ? SIG::off_codes2 : SIG::off_codes)) + (own0 - p0) * S::Wp * S::Cs_out;
    for (int i = tid; i < (nbytes >> 4); i += NTH)
      st_wt16(gcb, (unsigned)i * 16u, *reinterpret_cast<const LDS u32x4*>(lcb + i * 16));
  }
}

template <class SIG>
__global__ __launch_bounds__(SIG::nth) void conv_stack_fix_kernel(const ConvStackArgs A) {
  using S0 = typename SIG::L0;
  using S1 = typename SIG::L1;
  using S2 = typename SIG::L2;
  constexpr int NTH = SIG::nth, NL = SIG::n;
  static_assert(NL == 3 && SIG::splits == 2 && SIG::k16 == 1 && SIG::wt == 1, "three layers, two bands");
  extern __shared__ __attribute__((aligned(16))) char smem_[];
  LDS char* smem = (LDS char*)smem_;
  const int tid = threadIdx.x;
  const int b = blockIdx.x / SIG::splits, sp = blockIdx.x % SIG::splits;
  lbf16* wlds = (lbf16*)(smem + SIG::off_w);
  const uint32_t step = A.st ? (uint32_t)A.st->t + (uint32_t)A.step_inc : 0u;
  if (tid < 8) ((LDS uint32_t*)smem)[tid] = 0u;           // the 32 zero bytes of the layout
  constexpr int PF = (4096 + NTH - 1) / NTH;
  constexpr int nv0 = S0::KS * S0::NT * 64, nv1 = S1::KS * S1::NT * 64, nv2 = S2::KS * S2::NT * 64;
  constexpr int Wi0 = S0::Wo + S0::KW - 1, hiwi0 = S0::row(0, 5) * Wi0;
  // conv_stack_kernel's conditions for the one-batch prologue and the prefetch, proved here
  static_assert(S0::Cs_in == 4 && S0::KS == 2 && nv0 <= NTH && NL * 64 <= NTH && hiwi0 <= 4 * NTH &&
                    S0::row(1, 5) == S0::row(0, 5) && nv1 + nv2 <= PF * NTH,
                "one-batch prologue, register-free prefetch");
  static_assert(S2::w_lds == S1::w_lds + nv1 * 8 && S1::w_lds == S0::w_lds + nv0 * 8, "contiguous weight packs");
  LDS float* lbias = (LDS float*)(smem + SIG::off_bias);
  {
    // every global round trip of the staging in ONE batch: biases, layer 0's pack, the image
    const int bl = min(tid, NL * 64 - 1), bc = bl & 63, blay = bl >> 6;
    const float* bptr = blay == 0 ? A.L[0].bias : blay == 1 ? A.L[1].bias : A.L[2].bias;
    const int bcout = blay == 0 ? S0::Cout : blay == 1 ? S1::Cout : S2::Cout;
    const bool bok = tid < NL * 64 && bptr != nullptr && bc < bcout;
    const float braw = *(bok ? bptr + bc : reinterpret_cast<const float*>(A.L[0].wpk));
    const bf16x8 wv = load_bf16x8(A.L[0].wpk + (size_t)min(tid, nv0 - 1) * 8);
    lbf16* img = (lbf16*)(smem + SIG::off_buf0);
    const int y0 = sp ? S0::row(1, 4) : S0::row(0, 4);
    const bf16* x = A.x + (size_t)b * S0::H * S0::W * 4;
    if (A.from_data) {
      const int src = step_src_row(A.st, A.training, b);
      x = reinterpret_cast<const bf16*>(A.st->data_x) + (size_t)src * A.st->data_R;
      if (sp == 0 && tid == 0 && A.srcidx) A.srcidx[b] = src;
    }
    bf16x4 iv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = min(tid + u * NTH, hiwi0 - 1);
      const int hy = i / Wi0, hx = i - hy * Wi0;
      const int iy = y0 + hy, ix = hx - S0::pad_l;
      const bool ok = iy >= 0 && ix >= 0 && iy < S0::H && ix < S0::W;
      iv[u] = load_bf16x4_if(ok, x + (iy * S0::W + ix) * 4, x);
    }
    if (tid < NL * 64) lbias[tid] = bok ? braw : 0.f;
    if (tid < nv0) *reinterpret_cast<LDS bf16x8*>(wlds + S0::w_lds + tid * 8) = wv;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = tid + u * NTH;
      if (i < hiwi0) {
        const int hy = i / Wi0;
        *reinterpret_cast<LDS bf16x4*>(img + (hy * S0::xrow + (i - hy * Wi0)) * S0::xpix) = iv[u];
      }
    }
  }
  __syncthreads();                  // image, layer-0 weights and biases staged

  // the later layers' packs -> their LDS slots by LDS-DMA during layer 0's tiles (see
  // conv_stack_kernel: untracked, published by the vmcnt(0) before layer 0's closing barrier)
  const bf16* dma_src[PF];
  {
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    constexpr int ntot = nv1 + nv2;
    LDS char* wdst = (LDS char*)(wlds + S1::w_lds);
#pragma unroll
    for (int j = 0; j < PF; ++j) {
      const int vb = wave * 64 + j * NTH;
      if (vb >= ntot) break;
      const int v = vb + lane;
      const bf16* src = v < nv1 ? A.L[1].wpk + (size_t)v * 8 : A.L[2].wpk + (size_t)(v - nv1) * 8;
      dma_src[j] = src;
      dma16_untracked(src, wdst + (size_t)vb * 16);
    }
  }
  stack_fix_tiles<SIG, 0>(A, smem, b, sp, step);
#pragma unroll
  for (int j = 0; j < PF; ++j) asm volatile("" ::"v"(dma_src[j]));
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the untracked DMA
  __syncthreads();
  stack_fix_store<SIG, 0>(A, smem, b, sp);
  stack_fix_tiles<SIG, 1>(A, smem, b, sp, step);
  __syncthreads();
  stack_fix_store<SIG, 1>(A, smem, b, sp);
  stack_fix_tiles<SIG, 2>(A, smem, b, sp, step);
  __syncthreads();
  stack_fix_store<SIG, 2>(A, smem, b, sp);
}

// The dual (wgrad + dgrad) backward launch with BOTH halves' geometry fixed at compile time:
// the wgrad half exactly as dual_halo_sig_kernel<DSIG::Wg, 1, TM> (dual_halo_sig_body.h), the
// dgrad half through CvGeoFix<DSIG> (conv_halo_body.h) -- the dgrad signature DSIG of the same
// layer (wgrad_sig.h).  Same workgroup layout, same DualExtra by value and same extras as that
// kernel (its prologue is repeated here: the shipped kernel stays as it is); same LDS layout,
// k order, MFMA order and epilogue arithmetic, so every output is bit-identical.  The host
// launches it only when the dgrad args match DSIG field by field (dual_halo.hip); nothing in
// here falls back.  One instance per translation unit (dual_fix_*.hip).
#pragma once
#include "dual_halo_sig_body.h"

template <class DSIG, int TM>
__global__ __launch_bounds__(256) void dual_halo_fix_kernel(const ConvMMArgs ca, const WgradArgs wa, const int n_w,
                                                            const int wgx, const int wgy, const int cgx,
                                                            const DualExtra x) {
  using SIG = typename DSIG::Wg;
  static_assert(TM == DSIG::TM, "the signature's TM is dual_pick_tm's choice for its R");
  static_assert(CvGeoFix<DSIG>::onebatch() && DSIG::kpipe && DSIG::Cs_in % 32 == 0 && DSIG::Ho % DSIG::R == 0,
                "a fixed dgrad takes the one-batch prologue and the kfast loop over whole blocks");
  // (conv_halo_body's `whole` at NTC 1: every workgroup's n-tile lies inside the channel stride)
  static_assert(DSIG::NT * 16 <= DSIG::pCs && DSIG::pC == DSIG::pCs,
                "a fixed dgrad stores whole n-tiles of real channels: no run-time channel count in its epilogue");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int id = blockIdx.x;
  if (x.n_r) {   // early-bucket reduction + optimizer workgroups (placement as in dual_halo_kernel)
    const bool inter = x.rfirst == 2 && (int)gridDim.x >= 2 * x.n_r;
    const bool first = x.rfirst == 1 || (x.rfirst == 2 && !inter);
    int r;
    if (inter) {
      const int q = (int)gridDim.x / x.n_r, e = id / q;
      r = (id - e * q == 0 && e < x.n_r) ? e : -1;
      if (r < 0) id -= min(x.n_r, e + 1);
    } else {
      r = first ? id : id - (int)gridDim.x + x.n_r;
    }
    if (r >= 0 && r < x.n_r) {
      reduce_optim_block_rt(x.grad, x.rt, x.ro, r, reinterpret_cast<float*>(smem));
      return;
    }
    if (first) id -= x.n_r;
  }
  if (id < n_w) {
    const int bx = id % wgx;
    id /= wgx;
    wgrad_halo_body<SIG::MTW, SIG::NTT, false, true, false, WgGeoFix<SIG, false>>(wa, SIG::MT, bx, id % wgy, id / wgy,
                                                                                 smem);
  } else {
    id -= n_w;
    conv_halo_body<1, TM, 8, false, 1, false, CvGeoFix<DSIG>>(ca, id % cgx, id / cgx, smem);
  }
}

#define DUAL_FIX_DEFINE(NAME, DSIG, TM)                                                                         \
  DUAL_SIG_DECL(NAME) {                                                                                         \
    auto k = dual_halo_fix_kernel<DSIG, TM>;                                                                    \
    if (lds > 65536) hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
    const int n_w = wg.x * wg.y * wg.z;                                                                         \
    hipLaunchKernelGGL(k, dim3(n_w + cgx * cgy + x.n_r), dim3(256), lds, s, ca, wa, n_w, (int)wg.x, (int)wg.y,  \
                       cgx, x);                                                                                 \
  }

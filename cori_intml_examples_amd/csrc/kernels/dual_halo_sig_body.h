// The dual (wgrad + dgrad) backward launch with the wgrad half's geometry fixed at compile time
// to a layer signature (wgrad_sig.h).  Same workgroup layout, same extras and same dgrad body
// as dual_halo_kernel<1, MTW, NTT, TM, false> (dual_halo_body.h); the producer-push (XP) form
// stays in the generic kernel.  One instance per translation unit (dual_sig_*.hip).
#pragma once
#include "conv_halo_body.h"
#include "wgrad_halo_body.h"
#include "reduce_body.h"
#include "wgrad_sig.h"

template <class SIG, int NTC, int TM>
__global__ __launch_bounds__(256) void dual_halo_sig_kernel(const ConvMMArgs ca, const WgradArgs wa, const int n_w,
                                                            const int wgx, const int wgy, const int cgx,
                                                            const DualExtra x) {
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
    conv_halo_body<NTC, TM, 8, false, 1, false>(ca, id % cgx, id / cgx, smem);
  }
}

#define DUAL_SIG_DEFINE(NAME, SIG, TM)                                                                          \
  DUAL_SIG_DECL(NAME) {                                                                                         \
    auto k = dual_halo_sig_kernel<SIG, 1, TM>;                                                                  \
    if (lds > 65536) hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
    const int n_w = wg.x * wg.y * wg.z;                                                                         \
    hipLaunchKernelGGL(k, dim3(n_w + cgx * cgy + x.n_r), dim3(256), lds, s, ca, wa, n_w, (int)wg.x, (int)wg.y,  \
                       cgx, x);                                                                                 \
  }

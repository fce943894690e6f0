// The standalone halo weight-gradient kernel with its geometry fixed at compile time to a layer
// signature (wgrad_sig.h): wgrad_halo_kernel<MTW, NTT, true, PIPE, false> of a 4-channel first
// layer without the run-time geometry reads.  XIDX: the images are dataset rows read through
// a.xidx.  Instantiated in wgrad_sig.hip (and alone in scripts/probes/wgrad_sig_probe.hip).
#pragma once
#include "wgrad_halo_body.h"
#include "wgrad_sig.h"

template <class SIG, bool PIPE, bool XIDX>
__global__ __launch_bounds__(256) void wgrad_halo_sig_kernel(const WgradArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  static_assert(SIG::Cs_in == 4, "standalone signature instances are the 4-channel first layers");
  wgrad_halo_body<SIG::MTW, SIG::NTT, true, PIPE, false, WgGeoFix<SIG, XIDX>>(a, SIG::MT, blockIdx.x, blockIdx.y,
                                                                             blockIdx.z, smem);
}

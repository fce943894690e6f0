// Compile-only probe of EVERY deep wgrad instance the extension ships (wgrad_deep.hip: the
// standalone first-layer kernel at its depth, in both input forms), each beside the depth-one
// non-pipelined form it replaces, for tests/test_wgrad_depth_resources.py.  The test checks that
// the WGRAD_DEEP_PROBE lines below are wgrad_deep.hip's instances.  Never linked into the extension.
#include "wgrad_halo_sig_body.h"

// (wgrad_deep.hip's kernel: a translation unit with host launchers cannot be included)
template <class SIG, bool XIDX, int DEPTH>
__global__ __launch_bounds__(256) void wgrad_halo_deep_kernel(const WgradArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  wgrad_halo_body<SIG::MTW, SIG::NTT, true, true, false, WgGeoFix<SIG, XIDX>, DEPTH>(a, SIG::MT, blockIdx.x,
                                                                                    blockIdx.y, blockIdx.z, smem);
}

#define WGRAD_DEEP_PROBE(SIG, DEPTH)                                                       \
  template __global__ void wgrad_halo_deep_kernel<SIG, false, DEPTH>(const WgradArgs);     \
  template __global__ void wgrad_halo_deep_kernel<SIG, true, DEPTH>(const WgradArgs);      \
  template __global__ void wgrad_halo_sig_kernel<SIG, false, false>(const WgradArgs);      \
  template __global__ void wgrad_halo_sig_kernel<SIG, false, true>(const WgradArgs)
WGRAD_DEEP_PROBE(WgSigRpv1, 2);

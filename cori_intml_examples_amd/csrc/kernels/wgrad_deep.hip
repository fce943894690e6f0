// The standalone first-layer halo weight-gradient kernel with every block of a split in flight:
// wgrad_halo_sig_kernel<SIG, false, XIDX> (the non-pipelined form a grid of >= 512 workgroups
// takes, two dependent round trips per block -- X halo, then dY) as the body's DEPTH-deep
// pipeline (wgrad_halo_body.h), where a block's X and dY chunks leave in one batch and the
// first DEPTH blocks' batches before the first commit.  Same LDS images (the pooled dY chunk
// expanded into its window's pixel rows holds what the per-pixel unpool stages), same MFMA and
// slab-store order: the slabs are bit-identical.  launch_wgrad_halo (wgrad_halo.hip) picks it.
#include "wgrad_halo_sig_body.h"

template <class SIG, bool XIDX, int DEPTH>
__global__ __launch_bounds__(256) void wgrad_halo_deep_kernel(const WgradArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  static_assert(SIG::Cs_in == 4 && DEPTH > 1, "standalone signature instances are the 4-channel first layers");
  wgrad_halo_body<SIG::MTW, SIG::NTT, true, true, false, WgGeoFix<SIG, XIDX>, DEPTH>(a, SIG::MT, blockIdx.x,
                                                                                    blockIdx.y, blockIdx.z, smem);
}

template <class SIG, int DEPTH>
static void wgrad_deep_launch(const WgradArgs& a, dim3 grid, size_t lds, hipStream_t s) {
  void (*k)(const WgradArgs) = a.xidx ? wgrad_halo_deep_kernel<SIG, true, DEPTH> : wgrad_halo_deep_kernel<SIG, false, DEPTH>;
  if (lds > 65536) (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(k, grid, dim3(256), lds, s, a);
}

void wgrad_deep_rpv1(const WgradArgs& a, dim3 grid, size_t lds, hipStream_t s) {
  wgrad_deep_launch<WgSigRpv1, 2>(a, grid, lds, s);
}

// Compile-only probe of EVERY layer-signature wgrad instance the extension ships (wgrad_sig.h:
// the standalone forms of wgrad_sig.hip, the duals of dual_sig_*.hip), for
// tests/test_wgrad_sig_resources.py.  Never linked into the extension.
#include "dual_halo_sig_body.h"
#include "wgrad_halo_sig_body.h"

template __global__ void wgrad_halo_sig_kernel<WgSigRpv1, false, true>(const WgradArgs);
template __global__ void wgrad_halo_sig_kernel<WgSigRpv1, false, false>(const WgradArgs);
template __global__ void wgrad_halo_sig_kernel<WgSigRpv1, true, true>(const WgradArgs);
template __global__ void wgrad_halo_sig_kernel<WgSigRpv1, true, false>(const WgradArgs);
template __global__ void wgrad_halo_sig_kernel<WgSigMnist1, false, true>(const WgradArgs);
template __global__ void wgrad_halo_sig_kernel<WgSigMnist1, false, false>(const WgradArgs);
template __global__ void wgrad_halo_sig_kernel<WgSigMnist1, true, true>(const WgradArgs);
template __global__ void wgrad_halo_sig_kernel<WgSigMnist1, true, false>(const WgradArgs);

#define DUAL_SIG_PROBE(SIG, TM)                                                                          \
  template __global__ void dual_halo_sig_kernel<SIG, 1, TM>(const ConvMMArgs, const WgradArgs, const int, \
                                                            const int, const int, const int, const DualExtra)
DUAL_SIG_PROBE(WgSigRpv2, 4);
DUAL_SIG_PROBE(WgSigRpv2, 1);
DUAL_SIG_PROBE(WgSigRpv3, 4);
DUAL_SIG_PROBE(WgSigRpv3, 1);
DUAL_SIG_PROBE(WgSigMnist2, 2);
DUAL_SIG_PROBE(WgSigMnist2, 1);

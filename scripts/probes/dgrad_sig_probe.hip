// Compile-only probe of EVERY dual instance the extension ships with the dgrad half's geometry
// fixed too (dual_halo_fix_body.h: the DUAL_FIX_DEFINE of dual_fix_*.hip), beside the
// dual_halo_sig_kernel instance each one replaces, for tests/test_dgrad_sig_resources.py.
// The fixed instances are exactly the shipped ones (the test checks that); the three
// counterparts are here besides them on purpose, so that the test's bound on the instruction
// count and the occupancy is the counterpart's figure from the SAME compile, not a recorded one.
// Never linked into the extension.
#include "dual_halo_fix_body.h"

#define DUAL_FIX_PROBE(DSIG, TM)                                                                           \
  template __global__ void dual_halo_fix_kernel<DSIG, TM>(const ConvMMArgs, const WgradArgs, const int,    \
                                                          const int, const int, const int, const DualExtra); \
  template __global__ void dual_halo_sig_kernel<DSIG::Wg, 1, TM>(const ConvMMArgs, const WgradArgs, const int, \
                                                                 const int, const int, const int, const DualExtra)
DUAL_FIX_PROBE(DgSigRpv2, 4);
DUAL_FIX_PROBE(DgSigRpv3, 4);
DUAL_FIX_PROBE(DgSigMnist2, 2);

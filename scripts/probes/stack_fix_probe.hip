// Compile-only probe of EVERY conv-stack instance the extension ships with the whole geometry
// fixed at compile time (conv_stack_fix_body.h: the STACK_FIX_DEFINE of conv_stack_fix.hip), beside
// the kStackSigs instance each one replaces, for tests/test_stack_fix_resources.py.  The
// counterpart is in the same compile on purpose: the test's bound on the instruction count and
// the occupancy is the counterpart's figure from THIS compile, not a recorded one.
// Never linked into the extension.
#include "conv_stack_fix_body.h"

#define STACK_FIX_PROBE(SIG, C0, C1, C2)                                                      \
  template __global__ void conv_stack_fix_kernel<SIG>(const ConvStackArgs);                   \
  template __global__ void conv_stack_kernel<true, false, C0, C1, C2, 0u, SIG::nth>(const ConvStackArgs)
// the RPV stack's all-TM-1 16-wave signature (conv_stack.hip: SIG16(RPV_L0, RPV_L1(1), RPV_L2(1), 0u))
STACK_FIX_PROBE(StackSigRpv2, stack_lc(1, true, 2, 1, 4, true), stack_lc(1, false, 5, 2, 1, true),
                stack_lc(1, false, 9, 4, 1, true));

// The shipped conv-stack instance with the whole geometry fixed at compile time
// (conv_stack_fix_body.h, stack_sig.h) and the host's field-by-field match behind it.
#include "conv_stack_fix_body.h"

int conv_stack_variant(const ConvStackArgs& a);

// STACK_FIX_DEFINE(SIG): one shipped instance (tests/test_stack_fix_resources.py reads these lines)
#define STACK_FIX_DEFINE(SIG) \
  static const StackSigVals kFixVals = stack_sig_vals<SIG>(); \
  static void (*const kFixKernel)(const ConvStackArgs) = conv_stack_fix_kernel<SIG>
STACK_FIX_DEFINE(StackSigRpv2);

static bool stack_fix_matches(const ConvStackArgs& a, const StackSigVals& v) {
#define F(n) if (a.n != v.n) return false;
  STACK_ARG_INTS(F)
#undef F
  if (a.off_buf[0] != v.off_buf0 || a.off_buf[1] != v.off_buf1 || a.B < 1 || !a.x) return false;
  for (int l = 0; l < v.n; ++l) {
    const StackLayer& L = a.L[l];
    const StackSigLayerVals& s = v.L[l];
#define F(n) if (L.n != s.n) return false;
    STACK_GEO_INTS(F)
#undef F
    if (!L.wpk || !L.out) return false;
    for (int sp = 0; sp < v.splits; ++sp)
      for (int i = 0; i < 6; ++i)
        if (a.rows[l][sp][i] != s.rows[sp][i]) return false;
  }
  return true;
}

// The fixed instance replaces the 16-wave kStackSigs launch (variant 1) and nothing else: any
// other variant, the generic kernel, a diagnostics or stamp launch keep what they had.
bool conv_stack_fixed(const ConvStackArgs& a) {
  return a.fix && conv_stack_variant(a) == 1 && stack_fix_matches(a, kFixVals);
}

void launch_conv_stack_fix(const ConvStackArgs& a, hipStream_t s) {
  if (a.lds_bytes > 65536)
    (void)hipFuncSetAttribute((const void*)kFixKernel, hipFuncAttributeMaxDynamicSharedMemorySize, a.lds_bytes);
  hipLaunchKernelGGL(kFixKernel, dim3(a.B * a.splits), dim3(kFixVals.nth), a.lds_bytes, s, a);
}

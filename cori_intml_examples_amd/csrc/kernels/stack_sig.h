// Signatures of the layer-fused conv-stack forward (conv_stack_body.h): the WHOLE geometry of one
// network's stack at one band count as compile-time constants -- every layer's extents and
// strides, the LDS layout of its input halo image, the LDS offsets and the row-band table.  A
// kernel instantiated for a signature (conv_stack_fix_kernel, conv_stack_fix.hip) reads only
// pointers, B, the dropout hyperparameters and the step switches from ConvStackArgs; the host
// compares a launch's args field by field to the signature (stack_fix_matches) and launches what
// it launched before when anything differs.  A signature also fixes each layer's TM (m-tiles per
// wave and pass).
#pragma once
#include "args.h"

// the StackLayer fields that are geometry (the pointers and the dropout triple are not)
#define STACK_GEO_INTS(F)                                                                                     \
  F(H) F(W) F(Cs_in) F(Ho) F(Wo) F(Cout) F(Cs_out) F(KH) F(KW) F(pad_t) F(pad_l) F(KS) F(NT) F(pool) F(relu) \
  F(Hp) F(Wp) F(w_lds) F(xpix) F(xrow)
// the ConvStackArgs fields that are geometry or a compiled-in switch
#define STACK_ARG_INTS(F) F(n) F(splits) F(off_w) F(off_codes) F(off_codes2) F(off_bias) F(lds_bytes) F(k16) F(wt)

// A 3x3 'same' conv + ReLU + 2x2 pool on a square S_ x S_ grid, every channel real (Cs_out == Cout
// == NT * 16), with its two bands' rows: (c0, c1, own0, own1, ib, ih) as hip_geometry._stack_rows
// gives them -- conv rows computed, stage rows stored, first row and row count of the input image.
#define STACK_SIG_LAYER(NAME, S_, CSIN_, COUT_, KS_, NT_, WLDS_, XPIX_, XROW_, TM_, A0, A1, A2, A3, A4, A5, B0, \
                        B1, B2, B3, B4, B5)                                                                         \
  struct NAME {                                                                                                     \
    static constexpr int H = S_, W = S_, Cs_in = CSIN_, Ho = S_, Wo = S_, Cout = COUT_, Cs_out = COUT_, KH = 3,     \
                         KW = 3, pad_t = 1, pad_l = 1, KS = KS_, NT = NT_, pool = 1, relu = 1, Hp = S_ / 2,         \
                         Wp = S_ / 2, w_lds = WLDS_, xpix = XPIX_, xrow = XROW_, TM = TM_;                          \
    static constexpr int row(int sp, int i) {                                                                       \
      return sp == 0 ? (i == 0 ? A0 : i == 1 ? A1 : i == 2 ? A2 : i == 3 ? A3 : i == 4 ? A4 : A5)                   \
                     : (i == 0 ? B0 : i == 1 ? B1 : i == 2 ? B2 : i == 3 ? B3 : i == 4 ? B4 : B5);                  \
    }                                                                                                               \
  }

// DistTrain_rpv at two row bands per image (64 < B < 256; scripts/plan_dump.py at B = 128, default
// tunes): 64x64x{1,3} (channel stride 4) -> conv 16 / 32 / 64, 152 / 36 / 8 m-tiles per workgroup.
//               name           S  Csin Cout KS NT w_lds xpix xrow TM  band 0                    band 1
STACK_SIG_LAYER(StackRpv2L0, 64, 4, 16, 2, 1, 0, 4, 74, 4, 0, 38, 0, 16, -1, 40, 26, 64, 16, 32, 25, 40);
STACK_SIG_LAYER(StackRpv2L1, 32, 16, 32, 5, 2, 1024, 16, 36, 1, 0, 18, 0, 8, -1, 20, 14, 32, 8, 16, 13, 20);
STACK_SIG_LAYER(StackRpv2L2, 16, 32, 64, 9, 4, 6144, 48, 20, 1, 0, 8, 0, 4, -1, 10, 8, 16, 4, 8, 7, 10);
struct StackSigRpv2 {
  static constexpr int n = 3, splits = 2, nth = 1024, k16 = 1, wt = 1;
  static constexpr int off_bias = 1312, off_w = 2336, off_buf0 = 51488, off_buf1 = 75168, off_codes = 98208,
                       off_codes2 = 107936, lds_bytes = 117664;
  using L0 = StackRpv2L0;
  using L1 = StackRpv2L1;
  using L2 = StackRpv2L2;
};

// ------------------------------------------------------------------------------ host side
struct StackSigLayerVals {
#define F(n) int n;
  STACK_GEO_INTS(F)
#undef F
  int rows[2][6];
};
struct StackSigVals {
#define F(n) int n;
  STACK_ARG_INTS(F)
#undef F
  int off_buf0, off_buf1, nth;
  StackSigLayerVals L[3];
};

template <class S>
constexpr StackSigLayerVals stack_sig_layer_vals() {
  return StackSigLayerVals{
#define F(n) S::n,
      STACK_GEO_INTS(F)
#undef F
      {{S::row(0, 0), S::row(0, 1), S::row(0, 2), S::row(0, 3), S::row(0, 4), S::row(0, 5)},
       {S::row(1, 0), S::row(1, 1), S::row(1, 2), S::row(1, 3), S::row(1, 4), S::row(1, 5)}}};
}
template <class S>
constexpr StackSigVals stack_sig_vals() {
  return StackSigVals{
#define F(n) S::n,
      STACK_ARG_INTS(F)
#undef F
      S::off_buf0, S::off_buf1, S::nth,
      {stack_sig_layer_vals<typename S::L0>(), stack_sig_layer_vals<typename S::L1>(),
       stack_sig_layer_vals<typename S::L2>()}};
}

// the args are, field by field, the shipped signature's (and a.fix is set, a specialised 16-wave
// launch is what they would otherwise get, no diagnostics): launch_conv_stack_fwd's own decision
bool conv_stack_fixed(const ConvStackArgs& a);
void launch_conv_stack_fix(const ConvStackArgs& a, hipStream_t s);

// Layer signatures of the halo weight-gradient body (wgrad_halo_body.h): the geometry of one
// conv layer's wgrad launch as compile-time constants.  A kernel instantiated for a signature
// (wgrad_halo_sig_kernel, dual_halo_sig_kernel) reads no geometry from WgradArgs -- only the
// pointers, the batch size B and blocks_per_split stay run-time -- so the staging index math,
// the FastDiv divisors and the path choices (row-aligned k-steps, pooled expansion, bias tile,
// write-through slabs) fold to constants.  The host compares a launch's args field by field
// to the signatures (wgrad_sig.hip) and takes the generic kernel when none matches.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "args.h"

// the fixed values: the geometry fields (WG_GEO_INTS, args.h) and the launch's tile counts
#define WG_SIG_INTS(F) WG_GEO_INTS(F) F(MT) F(NTT)

#define WG_SIG(NAME, H_, W_, CS_, HO_, WO_, PAD_, KT_, NT_, CSDY_, DHP_, DWP_, POOLED_, R_, XPIX_, XROW_, DYLD_, MT_, \
               NTT_)                                                                                                 \
  struct NAME {                                                                                                      \
    static constexpr int H = H_, W = W_, Cs_in = CS_, Ho = HO_, Wo = WO_, KH = 3, KW = 3, stride = 1, pad_t = PAD_,  \
                         pad_l = PAD_, Ktiles = KT_, NT = NT_, Cs_dy = CSDY_, dHp = DHP_, dWp = DWP_, R = R_,        \
                         xpix = XPIX_, xrow = XROW_, dyld = DYLD_, kperm = 1, wt = 1, MT = MT_, NTT = NTT_;          \
    static constexpr bool pooled = POOLED_, bias = true;                                                             \
    /* m-tiles per wave, as launch_wgrad_halo's instance table buckets them */                                       \
    static constexpr int MTW = (MT_ + 1 + 3) / 4 <= 1 ? 1 : ((MT_ + 1 + 3) / 4 <= 2 ? 2 : 4);                        \
  }

// DistTrain_rpv: 64x64x{1,3} (channel stride 4) -> conv 16 / 32 / 64 'same', each + 2x2 pool
//      name       H   W   Cs  Ho  Wo  pad Kt NT Csdy dHp dWp pooled R  xpix xrow dyld MT NTT
WG_SIG(WgSigRpv1, 64, 64, 4, 64, 64, 1, 3, 1, 16, 32, 32, true, 8, 4, 74, 16, 3, 1);
WG_SIG(WgSigRpv2, 32, 32, 16, 32, 32, 1, 9, 2, 32, 16, 16, true, 8, 16, 34, 48, 9, 2);
WG_SIG(WgSigRpv3, 16, 16, 32, 16, 16, 1, 18, 4, 64, 8, 8, true, 8, 48, 18, 80, 9, 4);
// DistTrain_mnist: 28x28x1 -> conv 32 'valid' (unpooled), conv 64 'valid' + 2x2 pool
WG_SIG(WgSigMnist1, 28, 28, 4, 26, 26, 0, 3, 2, 32, 0, 0, false, 8, 4, 42, 48, 3, 2);
WG_SIG(WgSigMnist2, 26, 26, 32, 24, 24, 0, 18, 4, 64, 12, 12, true, 5, 48, 26, 80, 9, 4);

// Dgrad signatures: the co-scheduled dgrad (conv_halo_body.h in mode 1) of the SAME layer as a
// wgrad signature, as executor_hip._dgrad_args and hip_geometry._halo_cfg produce it at default
// tunes for every batch >= 128 (scripts/plan_dump.py at B = 128 and 256): the conv over the pooled
// dY with the flipped taps, written through the previous stage's ReLU.  R (rows per block) and TM
// (m-tiles per wave per pass, dual_pick_tm's choice for R) are part of the signature.  epi_pre
// is no geometry but a choice made per instance from its measurement: the epilogue's ReLU-mask
// operands are fetched ahead of the MFMAs (conv_halo_body.h); false keeps the in-place loads.
#define DG_SIG(NAME, WG_, H_, W_, CS_, HO_, WO_, PAD_, KS_, NT_, R_, PH_, PW_, XPIX_, PC_, TM_, EPI_)               \
  struct NAME {                                                                                                    \
    using Wg = WG_;                                                                                                \
    static constexpr int H = H_, W = W_, Cs_in = CS_, Ho = HO_, Wo = WO_, KH = 3, KW = 3, stride = 1, pad_t = PAD_, \
                         pad_l = PAD_, in_dil = 1, KS = KS_, NT = NT_, pool = 0, Hp = 0, Wp = 0, Cs_out = 0, R = R_, \
                         in_pH = PH_, in_pW = PW_, xpix = XPIX_, kpipe = 1, pCs = PC_, pC = PC_, prev_relu = 1,     \
                         wt = 1, TM = TM_;                                                                         \
    static constexpr bool pooled = true, epi_pre = EPI_;                                                           \
  }
// (docs/ARCHITECTURE.md §16: conv2's dual gains 1.5 us with it; conv3's, whose wgrad half binds, and
// the MNIST one stayed under three noises of their launches and keep the in-place loads)
//      name         wgrad sig    H   W   Cs  Ho  Wo  pad KS  NT R   pH  pW  xpix pC  TM epi_pre
DG_SIG(DgSigRpv2, WgSigRpv2, 32, 32, 32, 32, 32, 1, 9, 1, 16, 16, 16, 48, 16, 4, true);
DG_SIG(DgSigRpv3, WgSigRpv3, 16, 16, 64, 16, 16, 1, 18, 2, 16, 8, 8, 80, 32, 4, false);
DG_SIG(DgSigMnist2, WgSigMnist2, 24, 24, 64, 26, 26, 2, 18, 2, 13, 12, 12, 0, 32, 2, false);

// ------------------------------------------------------------------------------ host side
struct DgSigVals {
#define F(n) int n;
  CV_GEO_INTS(F)
  CV_BT_INTS(F)
#undef F
  int pooled, TM;            // TM 0: the wgrad signature has no fixed dgrad
};

template <class S>
constexpr DgSigVals dg_sig_vals() {
  return DgSigVals{
#define F(n) S::n,
      CV_GEO_INTS(F) CV_BT_INTS(F)
#undef F
          S::pooled ? 1 : 0,
      S::TM};
}

struct WgSigVals {
#define F(n) int n;
  WG_SIG_INTS(F)
#undef F
  int pooled, bias;
};

template <class S>
constexpr WgSigVals wg_sig_vals() {
  return WgSigVals{
#define F(n) S::n,
      WG_SIG_INTS(F)
#undef F
          S::pooled ? 1 : 0,
      S::bias ? 1 : 0};
}

// launchers of the instantiated kernels (one translation unit per dual instance, so the build
// stays parallel): standalone wgrad (pipe / xidx forms chosen inside), dual at one dgrad TM
typedef void (*WgSigLaunch)(const WgradArgs& a, dim3 grid, size_t lds, bool pipe, hipStream_t s);
typedef void (*DualSigLaunch)(const ConvMMArgs& ca, const WgradArgs& wa, dim3 wg, int cgx, int cgy, size_t lds,
                              const DualExtra& x, hipStream_t s);
#define DUAL_SIG_DECL(NAME)                                                                                  \
  void NAME(const ConvMMArgs& ca, const WgradArgs& wa, dim3 wg, int cgx, int cgy, size_t lds, const DualExtra& x, \
            hipStream_t s)
DUAL_SIG_DECL(dual_sig_rpv2_tm1);
DUAL_SIG_DECL(dual_sig_rpv2_tm4);
DUAL_SIG_DECL(dual_sig_rpv3_tm1);
DUAL_SIG_DECL(dual_sig_rpv3_tm4);
DUAL_SIG_DECL(dual_sig_mnist2_tm1);
DUAL_SIG_DECL(dual_sig_mnist2_tm2);
// ... and with the dgrad half's geometry fixed too (dual_halo_fix_body.h, dual_fix_*.hip)
DUAL_SIG_DECL(dual_fix_rpv2_tm4);
DUAL_SIG_DECL(dual_fix_rpv3_tm4);
DUAL_SIG_DECL(dual_fix_mnist2_tm2);

struct WgradSig {
  WgSigVals v;
  WgSigLaunch alone;          // standalone wgrad launch (null: none instantiated)
  DualSigLaunch dual[3];      // dual launch (NTC 1) at dgrad TM 1 / 2 / 4 (null: none)
  DgSigVals dg;               // the layer's dgrad signature (dg.TM 0: none) ...
  DualSigLaunch fix;          // ... and the dual launch with both halves fixed (NTC 1, TM dg.TM)
};

// ... and the standalone first-layer wgrad that keeps several blocks of a split in flight
// (wgrad_halo_body.h DEPTH; wgrad_deep.hip, both input forms chosen inside)
typedef void (*WgDeepLaunch)(const WgradArgs& a, dim3 grid, size_t lds, hipStream_t s);
void wgrad_deep_rpv1(const WgradArgs& a, dim3 grid, size_t lds, hipStream_t s);

// The deep instance of a signature (a row per row of the signature table): it replaces the
// non-pipelined form of WgradSig::alone.  depth 1, alone null: the signature has none.
struct WgradDeep {
  int depth;
  WgDeepLaunch alone;
};
const WgradDeep& wgrad_deep_at(int v);

// 1 + index of the signature these args match (0: none), and the table entry
int wgrad_sig_find(const WgradArgs& a, int MT, int NTT);
const WgradSig& wgrad_sig_at(int v);
// the dgrad args (NTC ntc, TM tm) are, field by field, signature v's dgrad and it has an instance
bool dgrad_sig_matches(const ConvMMArgs& a, int ntc, int tm, int v);

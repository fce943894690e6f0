// Layer signatures of the halo weight-gradient body (wgrad_halo_body.h): the geometry of one
// conv layer's wgrad launch as compile-time constants.  A kernel instantiated for a signature
// (wgrad_halo_sig_kernel, dual_halo_sig_kernel) reads no geometry from WgradArgs -- only the
// pointers, the batch size B and blocks_per_split stay run-time -- so the staging index math,
// the FastDiv divisors and the path choices (row-aligned k-steps, pooled expansion, bias tile,
// write-through slabs) fold to constants.  The host compares a launch's args field by field
// to the signatures (wgrad_sig.hip) and takes the generic kernel when none matches.
#pragma once
#include <hip/hip_runtime.h>

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

// ------------------------------------------------------------------------------ host side
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

struct WgradSig {
  WgSigVals v;
  WgSigLaunch alone;          // standalone wgrad launch (null: none instantiated)
  DualSigLaunch dual[3];      // dual launch (NTC 1) at dgrad TM 1 / 2 / 4 (null: none)
};

// 1 + index of the signature these args match (0: none), and the table entry
int wgrad_sig_find(const WgradArgs& a, int MT, int NTT);
const WgradSig& wgrad_sig_at(int v);

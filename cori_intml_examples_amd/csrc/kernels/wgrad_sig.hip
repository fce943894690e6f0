// Layer-signature instances of the standalone halo weight-gradient kernel, and the signature
// table the launchers (wgrad_halo.hip, dual_halo.hip) match a launch's args against.
//
// wgrad_halo_sig_kernel<SIG, PIPE, XIDX> is wgrad_halo_kernel<MTW, NTT, true, PIPE, false> with
// the geometry of SIG as compile-time constants (wgrad_sig.h): same workgroup layout, same
// staging, same MFMA and slab-store order, so the slabs are bit-identical.  Both PIPE forms
// (the launcher's grid-size rule picks one, as for the generic kernel) and both input forms
// (activation buffer / dataset rows through xidx) are instantiated -- the first-layer kernels
// are small (~1k instructions each).
#include "wgrad_halo_sig_body.h"

template <class SIG>
static void wgrad_sig_launch(const WgradArgs& a, dim3 grid, size_t lds, bool pipe, hipStream_t s) {
  void (*k)(const WgradArgs) =
      a.xidx ? (pipe ? wgrad_halo_sig_kernel<SIG, true, true> : wgrad_halo_sig_kernel<SIG, false, true>)
             : (pipe ? wgrad_halo_sig_kernel<SIG, true, false> : wgrad_halo_sig_kernel<SIG, false, false>);
  if (lds > 65536) (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(k, grid, dim3(256), lds, s, a);
}

static const WgradSig kWgradSigs[] = {
    {wg_sig_vals<WgSigRpv1>(), wgrad_sig_launch<WgSigRpv1>, {nullptr, nullptr, nullptr}, {}, nullptr},
    {wg_sig_vals<WgSigRpv2>(), nullptr, {dual_sig_rpv2_tm1, nullptr, dual_sig_rpv2_tm4},
     dg_sig_vals<DgSigRpv2>(), dual_fix_rpv2_tm4},
    {wg_sig_vals<WgSigRpv3>(), nullptr, {dual_sig_rpv3_tm1, nullptr, dual_sig_rpv3_tm4},
     dg_sig_vals<DgSigRpv3>(), dual_fix_rpv3_tm4},
    {wg_sig_vals<WgSigMnist1>(), wgrad_sig_launch<WgSigMnist1>, {nullptr, nullptr, nullptr}, {}, nullptr},
    {wg_sig_vals<WgSigMnist2>(), nullptr, {dual_sig_mnist2_tm1, dual_sig_mnist2_tm2, nullptr},
     dg_sig_vals<DgSigMnist2>(), dual_fix_mnist2_tm2},
};
static_assert(std::is_same<DgSigRpv2::Wg, WgSigRpv2>::value && std::is_same<DgSigRpv3::Wg, WgSigRpv3>::value &&
                  std::is_same<DgSigMnist2::Wg, WgSigMnist2>::value,
              "a table row pairs a wgrad signature with its own layer's dgrad");

// the deep instances, row for row of kWgradSigs
// (the RPV duals' wgrad halves at depths 2 and 3 gained less than their launches' noise bar --
// the dgrad half is as long -- and the MNIST first layer's unpooled dY has no pooled-chunk
// stage: docs/ARCHITECTURE.md section 15)
static const WgradDeep kWgradDeep[] = {
    {2, wgrad_deep_rpv1}, {1, nullptr}, {1, nullptr}, {1, nullptr}, {1, nullptr},
};
static_assert(sizeof(kWgradDeep) / sizeof(kWgradDeep[0]) == sizeof(kWgradSigs) / sizeof(kWgradSigs[0]),
              "a deep row per signature");

const WgradDeep& wgrad_deep_at(int v) { return kWgradDeep[v - 1]; }

// field by field over WG_GEO_INTS (an unpooled dY never reads dHp / dWp: not compared then)
static bool wg_sig_matches(const WgradArgs& a, int MT, int NTT, const WgSigVals& v) {
  if ((a.dy_code != nullptr) != (v.pooled != 0) || (a.bslab != nullptr) != (v.bias != 0)) return false;
  if (MT != v.MT || NTT != v.NTT) return false;
  WgSigVals w = v;
#define F(n) w.n = a.n;
  WG_GEO_INTS(F)
#undef F
  if (!v.pooled) w.dHp = v.dHp, w.dWp = v.dWp;
#define F(n) \
  if (w.n != v.n) return false;
  WG_GEO_INTS(F)
#undef F
  return true;
}

int wgrad_sig_find(const WgradArgs& a, int MT, int NTT) {
  const int nsig = (int)(sizeof(kWgradSigs) / sizeof(kWgradSigs[0]));
  for (int i = 0; i < nsig; ++i)
    if (wg_sig_matches(a, MT, NTT, kWgradSigs[i].v)) return i + 1;
  return 0;
}

const WgradSig& wgrad_sig_at(int v) { return kWgradSigs[v - 1]; }

// field by field over CV_GEO_INTS (ConvMMArgs) and CV_BT_INTS (its BwdThrough); the fixed dual
// is built for one n-tile per workgroup, the backward-through epilogue and a pooled dY
bool dgrad_sig_matches(const ConvMMArgs& a, int ntc, int tm, int v) {
  const DgSigVals& d = kWgradSigs[v - 1].dg;
  if (!kWgradSigs[v - 1].fix || !d.TM || tm != d.TM || ntc != 1 || a.mode != 1) return false;
  if ((a.in_code != nullptr) != (d.pooled != 0)) return false;
#define F(n) \
  if (a.n != d.n) return false;
  CV_GEO_INTS(F)
#undef F
#define F(n) \
  if (a.bt.n != d.n) return false;
  CV_BT_INTS(F)
#undef F
  return true;
}

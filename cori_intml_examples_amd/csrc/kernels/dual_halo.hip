// Horizontal fusion of one conv layer's two independent backward GEMMs:
//   wgrad: dW = im2col(X)^T dY   (wgrad_halo body, few long workgroups: 170-350 at batch 128)
//   dgrad: dX = dY * W^T         (conv_halo body in mode 1, 512 short workgroups)
// Both read the same dY (rebuilt from dP + argmax codes on load) and nothing either writes
// is read by the other, so they run as ONE launch: workgroups [0, n_w) execute the wgrad
// body, the rest the dgrad body.  At batch 128 neither kernel alone fills 256 CUs for long;
// co-scheduled, the dgrad workgroups fill the CUs the wgrad ones leave idle and the step pays
// one kernel boundary (launch ramp + drain + L2 writeback, ~5 us here) instead of two.
// Wgrad workgroups come first: they are the long pole, so they are dispatched first.
// The LDS request is the max of the two bodies' needs.  Optionally the launch also carries an
// early bucket's reduction + optimizer (DualExtra) in extra workgroups.
#include <algorithm>

#include "dual_halo_body.h"
#include "wgrad_sig.h"

size_t conv_halo_lds_bytes(const ConvMMArgs& a, int ntc);
size_t wgrad_halo_lds_bytes(const WgradArgs& a, int MT, int NTT);

// args the dual kernels are not built for: 4-channel / tiny-K variants, ablation / diagnostics
// code, a dgrad epilogue other than backward-through
static bool dual_declines(const ConvMMArgs& ca, const WgradArgs& wa) {
  if (ca.Cs_in == 4 || wa.Cs_in == 4 || ca.KS <= 2) return true;
  return ca.mode != 1 || ca.dbg || wa.dbg || ca.ts || wa.ts || wa.ts2;
}

// dgrad m-tiles per wave per pass: the TM in {4, 2} that minimises the busiest wave's
// tile count over the block (ties -> larger TM: more fragment reuse); TM = 1 only when
// the block has <= 4 tiles (measured: TM 1 loses its fragment reuse on longer blocks)
static int dual_pick_tm(const ConvMMArgs& ca, int ntc) {
  const int rows = std::min(ca.R, ca.Ho);
  const int ntiles = ca.pool ? ((rows / 2) * ca.Wp + 3) / 4 : (rows * ca.Wo + 15) / 16;
  int tm = ntc >= 8 ? 2 : 4, best = 1 << 30;
  for (int t : {4, 2, 1}) {
    if (ntc >= 8 && t == 4) continue;
    if (ntc > 2 && t != (ntc >= 8 ? 2 : 4)) continue;
    if (t == 1 && ntiles > 4) continue;
    const int load = t * ((ntiles + 4 * t - 1) / (4 * t));   // tiles of the busiest wave
    if (load < best) { best = load; tm = t; }
  }
  if (ca.tm == 1 || ca.tm == 2 || (ca.tm == 4 && ntc < 8)) tm = ca.tm;   // host override (geometry table)
  return tm;
}

// LDS-size declines of the dual launch: over the 160 KB budget, or too small for what the
// extras stage (the reduce body <= 2 KB; an exchange mode's wait word on top)
static bool dual_lds_declines(size_t lds, bool extras, bool xp_on, int xp_mode) {
  if (lds > 160 * 1024 || (extras && lds < 2048)) return true;
  return extras && xp_on && xp_mode >= 2 && lds < 4096;
}

// 1 + index of the layer signature (wgrad_sig.hip) whose dual instance -- NTC 1 at dgrad TM
// tm, early-reduction extras included -- serves a launch that passed the declines, or 0: the
// generic kernel.  xp: the launch carries producer-push extras (generic kernel only).
static int dual_sig_variant(int ntc, const WgradArgs& wa, int MT, int NTT, int tm, bool xp) {
  if (!wa.spec || xp || ntc != 1) return 0;
  const int v = wgrad_sig_find(wa, MT, NTT);
  return v && wgrad_sig_at(v).dual[tm == 4 ? 2 : tm - 1] ? v : 0;
}

// The host's query of that choice (0 also for every launch launch_dual_halo declines).
// extras: the launch carries an early bucket's reduction; xp: as producer-push extras.
int dual_halo_variant(const ConvMMArgs& ca, int ntc, const WgradArgs& wa, int MT, int NTT, bool xp, bool extras) {
  if (dual_declines(ca, wa)) return 0;
  const size_t lds = std::max(conv_halo_lds_bytes(ca, ntc), wgrad_halo_lds_bytes(wa, MT, NTT));
  if (dual_lds_declines(lds, extras || xp, false, 1)) return 0;   // (xp launches: 0 below anyway)
  return dual_sig_variant(ntc, wa, MT, NTT, dual_pick_tm(ca, ntc), xp);
}

// A launch that takes signature instance v (dual_sig_variant) runs the instance whose dgrad
// geometry is fixed too (dual_halo_fix_body.h): ca.spec is set and the dgrad args are, field
// by field, that signature's dgrad at its TM.
static bool dual_fix_variant(const ConvMMArgs& ca, int ntc, int v, int tm) {
  return v && ca.spec && dgrad_sig_matches(ca, ntc, tm, v);
}

// The host's query of that choice (false also for every launch launch_dual_halo declines or
// serves with another kernel); the arguments of dual_halo_variant.
bool dual_halo_dgrad_fixed(const ConvMMArgs& ca, int ntc, const WgradArgs& wa, int MT, int NTT, bool xp,
                           bool extras) {
  return dual_fix_variant(ca, ntc, dual_halo_variant(ca, ntc, wa, MT, NTT, xp, extras), dual_pick_tm(ca, ntc));
}

// Returns false (nothing launched) when the pair is not a supported combination; the caller
// then launches the two kernels separately.
bool launch_dual_halo(const ConvMMArgs& ca, int ntc, const WgradArgs& wa, int MT, int NTT, int splits,
                      const DualExtra& x, hipStream_t s) {
  // the dual kernel is built without ablation / diagnostics code and with the dgrad's
  // backward-through epilogue only: anything else runs as two standalone launches
  if (dual_declines(ca, wa)) return false;
  const int cgy = (ca.NT + ntc - 1) / ntc;
  const int cgx = ca.B * ((ca.Ho + ca.R - 1) / ca.R);
  const dim3 wg(splits, (wa.NT + NTT - 1) / NTT, (wa.Ktiles + MT - 1) / MT);
  const int mtw = (MT + (wa.bslab ? 1 : 0) + 3) / 4;
  const size_t lds = std::max(conv_halo_lds_bytes(ca, ntc), wgrad_halo_lds_bytes(wa, MT, NTT));
  if (dual_lds_declines(lds, x.n_r != 0, x.xp.on != 0, x.xp.mode)) return false;
  // extras run the exchange's modes 1 (reduce + push) and 4 (owner half) only; a mode-2 table
  // (the unsplit exchange, xchg_split=0) goes to the caller's separate launches
  if (x.n_r && x.xp.on && x.xp.mode != 1 && x.xp.mode != 4) return false;
  const int tm = dual_pick_tm(ca, ntc);
  // a layer-signature instance (wgrad geometry fixed at compile time) where one matches
  if (const int v = dual_sig_variant(ntc, wa, MT, NTT, tm, x.n_r && x.xp.on)) {
    const WgradSig& sg = wgrad_sig_at(v);
    (dual_fix_variant(ca, ntc, v, tm) ? sg.fix : sg.dual[tm == 4 ? 2 : tm - 1])(ca, wa, wg, cgx, cgy, lds, x, s);
    return true;
  }
  switch (ntc) {
    case 1: return dual_launch_n1(ca, wa, MT, NTT, mtw, tm, wg, cgx, cgy, lds, x, s);
    case 2: return dual_launch_n2(ca, wa, MT, NTT, mtw, tm, wg, cgx, cgy, lds, x, s);
    case 4: return dual_launch_n4(ca, wa, MT, NTT, mtw, tm, wg, cgx, cgy, lds, x, s);
    case 8: return dual_launch_n8(ca, wa, MT, NTT, mtw, tm, wg, cgx, cgy, lds, x, s);
  }
  return false;
}

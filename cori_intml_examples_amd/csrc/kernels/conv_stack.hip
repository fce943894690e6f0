// Layer-fused forward of a whole conv stack (gfx950 MFMA 16x16x32 bf16): a workgroup runs
// every Conv2D(+bias +ReLU +2x2 max-pool +dropout) stage of the network for one row band of
// one image, with the activations resident in LDS.
//
// Why: at the reference batch (128) a per-layer conv launch is pure latency -- ~1 GFLOP of
// MFMA work spread over 512 workgroups finishes in < 1 us of math but costs 13-15 us of
// launch ramp, global staging and drain, three times per forward.  The per-image working
// set of the small CNNs this framework targets (RPV: 64x64x3 -> 32x32x16 -> 16x16x32 ->
// 8x8x64; MNIST: 28x28x1 -> 26x26x32 -> 12x12x64) fits the 160 KB LDS of a CDNA4 CU, so
// the stack runs as a single launch: the image band is staged once (zero halo included),
// each layer's output tile is written by the MFMA epilogue straight into the NEXT layer's
// zero-padded halo image in LDS, and only the stage outputs the backward pass and the
// dense layer need (pooled activations + argmax codes) are streamed to global memory with
// 16-byte stores.
//
// Grid = B x splits: workgroup (b, sp) OWNS stage-output rows [own0, own1) of every layer
// (a partition over the splits) and computes conv rows [c0, c1): its owned rows plus the
// halo rows the next layer's range needs (host-computed, ConvStackArgs::rows).  With two
// bands per image the batch-128 launch fills all 256 CUs for ~35% recomputed conv1 rows.
//
// Per layer (12 waves): m-tiles are 16 output pixels (or 4 pooling windows x 4 positions,
// so the 2x2 max-pool is register-local: an MFMA accumulator row group is one window),
// TM m-tiles x NT n-tiles per wave; A fragments are one ds_read_b128 per k-step from the
// halo image (two ds_read_b64 for the 4-channel input), B fragments come from the layer's
// fragment-major weight pack staged in LDS at kernel start.  All LDS traffic goes through
// address-space-3 pointers with 32-bit offsets (generic pointers would turn every access
// into FLAT instructions with 64-bit address math: the epilogue was VALU-bound on that).
// Numerics (bf16 rounding points, dropout counters, argmax codes) are identical to the
// per-layer kernels.
#include "conv_stack_body.h"
#include "stack_sig.h"

int conv_stack_threads() { return STACK_THREADS; }
int conv_stack_tabn() { return STACK_TABN; }

// ----------------------------------------------------------------------- host-side dispatch
// Layer l's code as the generic kernel would pick its body (stack_rows_ok, the TM rule per
// band for nw waves, FULL); 0 if the bands disagree on TM (no specialised instance serves them).
static unsigned host_layer_code(const ConvStackArgs& a, int l, int nw) {
  const StackLayer& L = a.L[l];
  const bool rows_ok = !(a.dbg & 19) && L.pool && (L.Wp & 3) == 0 && L.KH == 3 && L.KW == 3;
  const bool full = L.Cs_out == L.Cout && L.Cout == L.NT * 16;
  int tm = 0;
  for (int sp = 0; sp < a.splits; ++sp) {
    const int ntl = ((a.rows[l][sp][1] - a.rows[l][sp][0]) >> 1) * (L.Wp >> 2);
    const bool tm1 = ntl <= nw || cdiv(ntl, nw) < 2 * cdiv(ntl, 2 * nw);
    const int t = tm1 ? 1 : 2;
    if (tm && t != tm) return 0;
    tm = t;
  }
  const bool c4 = L.Cs_in == 4;
  if (rows_ok && c4 && L.KS == 2 && L.NT == 1) return stack_lc(1, true, 2, 1, 4, full);
  if (rows_ok && c4 && L.KS == 2 && L.NT == 2) return stack_lc(1, true, 2, 2, 2, full);
  if (rows_ok && !c4 && L.KS == 5 && L.NT == 2) return stack_lc(1, false, 5, 2, tm, full);
  if (rows_ok && !c4 && L.KS == 9 && L.NT == 4) return stack_lc(1, false, 9, 4, tm, full);
  if (rows_ok && !c4 && L.KS == 9 && L.NT == 2) return stack_lc(1, false, 9, 2, 2, full);
  const int nt = L.NT < 1 ? 1 : (L.NT > 4 ? 4 : L.NT);
  return stack_lc(2, c4, 0, nt, nt >= 2 ? 2 : 4, false);
}

// the specialised instances: the DistTrain_rpv stack (64x64x{1,3} -> conv 16 / 32 / 64, each
// + ReLU + 2x2 pool; the TM of layers 1 and 2 depends on the row bands) and the
// DistTrain_mnist stack (28x28x1 -> conv 32 'valid' unpooled, conv 64 + pool).  The RPV
// stack's all-TM-1 signature also has a 16-wave instance (its 12-wave build needs 120 VGPRs:
// at 16 waves the 128-VGPR cap holds without spills) -- chosen with spec = 2.
#define RPV_L0 stack_lc(1, true, 2, 1, 4, true)
#define RPV_L1(tm) stack_lc(1, false, 5, 2, tm, true)
#define RPV_L2(tm) stack_lc(1, false, 9, 4, tm, true)
#define MN_L0 stack_lc(2, true, 0, 2, 2, false)
#define MN_L1(tm) stack_lc(1, false, 9, 4, tm, true)
typedef void (*StackKernel)(const ConvStackArgs);
struct StackSig { int nth; unsigned c[MAX_STACK]; StackKernel k[2]; };   // k[TS] (k[1] null: no stamp build)
#define SIG(c0, c1, c2, c3) \
  {STACK_THREADS, {c0, c1, c2, c3}, \
   {conv_stack_kernel<true, false, c0, c1, c2, c3>, conv_stack_kernel<true, true, c0, c1, c2, c3>}}
#define SIG16(c0, c1, c2, c3) {1024, {c0, c1, c2, c3}, {conv_stack_kernel<true, false, c0, c1, c2, c3, 1024>, nullptr}}
static const StackSig kStackSigs[] = {
    // (first: conv_stack_fixed takes variant 1 as "the 16-wave RPV launch" the fixed instance replaces)
    SIG16(RPV_L0, RPV_L1(1), RPV_L2(1), 0u),
    SIG(RPV_L0, RPV_L1(2), RPV_L2(1), 0u), SIG(RPV_L0, RPV_L1(2), RPV_L2(2), 0u),
    SIG(RPV_L0, RPV_L1(1), RPV_L2(1), 0u), SIG(RPV_L0, RPV_L1(1), RPV_L2(2), 0u),
    SIG(MN_L0, MN_L1(1), 0u, 0u), SIG(MN_L0, MN_L1(2), 0u, 0u),
};
#undef SIG
#undef SIG16

// does signature i serve these args (its layer codes for its wave count, and the
// specialised prologue's geometry conditions -- the generic kernel tests those per launch)
static bool stack_sig_matches(const ConvStackArgs& a, const StackSig& g) {
  const int nth = g.nth, nw = nth / 64;
  for (int l = 0; l < MAX_STACK; ++l) {
    const unsigned c = l < a.n ? host_layer_code(a, l, nw) : 0u;
    if (c == 0u && l < a.n) return false;
    if (c != g.c[l]) return false;
  }
  const int PF = (4096 + nth - 1) / nth;
  int nv_later = 0;
  for (int l = 1; l < a.n; ++l) nv_later += a.L[l].KS * a.L[l].NT * 64;
  const StackLayer& L0 = a.L[0];
  if (L0.Cs_in != 4 || L0.KS * L0.NT * 64 > nth || a.n * 64 > nth || nv_later > PF * nth) return false;
  for (int sp = 0; sp < a.splits; ++sp)
    if (a.rows[0][sp][5] * (L0.Wo + L0.KW - 1) > 4 * nth) return false;
  return true;
}

// 1 + index of the specialised instance serving these args, or 0 (generic kernel).  spec = 1:
// the 12-wave instances; spec = 2: a 16-wave instance first where one matches; a stamp
// request (ts) takes the 12-wave stamp builds.
int conv_stack_variant(const ConvStackArgs& a) {
  if (!a.spec || a.dbg || a.n < 2 || a.n > MAX_STACK) return 0;
  const int nsig = (int)(sizeof(kStackSigs) / sizeof(kStackSigs[0]));
  for (int pass = (a.spec >= 2 && !a.ts) ? 0 : 1; pass < 2; ++pass)
    for (int i = 0; i < nsig; ++i) {
      const bool wide = kStackSigs[i].nth != STACK_THREADS;
      if (wide != (pass == 0)) continue;
      if (stack_sig_matches(a, kStackSigs[i])) return i + 1;
    }
  return 0;
}

void launch_conv_stack_fwd(const ConvStackArgs& a, hipStream_t s) {
  // the whole geometry a compile-time signature (conv_stack_fix.hip): only args that equal it
  if (conv_stack_fixed(a)) return launch_conv_stack_fix(a, s);
  const int v = conv_stack_variant(a);
  StackKernel k = v ? kStackSigs[v - 1].k[a.ts ? 1 : 0] : conv_stack_kernel<false, true, 0u, 0u, 0u, 0u>;
  const int nth = v ? kStackSigs[v - 1].nth : STACK_THREADS;
  if (a.lds_bytes > 65536)
    (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, a.lds_bytes);
  hipLaunchKernelGGL(k, dim3(a.B * a.splits), dim3(nth), a.lds_bytes, s, a);
}

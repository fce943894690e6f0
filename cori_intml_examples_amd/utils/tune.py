"""The ``INTML_TUNE`` knobs: ONE declared table of every kernel-path switch and launch-geometry
constant of the HIP backend, and ``tune(key)``, which reads one.

``INTML_TUNE="key=value,key=value"`` overrides registered knobs for measurement sweeps and A/B
tests.  A key that is not in ``KNOBS`` is an error, in the environment string (ValueError, with
the closest registered keys) as at a call site (KeyError): a mistyped or stale key can no
longer measure the default against itself.  ``python -m cori_intml_examples_amd.utils.tune``
prints the table as Markdown (docs/TUNES.md).  GPU-free.
"""
from __future__ import annotations

import difflib
import os
from typing import Dict, NamedTuple, Optional, Tuple

# what a knob does to results
EXACT = "exact"          # A/B switch: bit-identical results (a test or the kernel source says so)
PATH = "path"            # another kernel path / geometry / summation order: the usual tolerance
ABLATION = "ablation"    # timing only: wrong results
KINDS = (EXACT, PATH, ABLATION)

# per-layer knobs: tune(key, layer=i) reads ``key<i>``, then ``key`` (LAYER) or nothing (LAYER_ONLY)
LAYER, LAYER_ONLY = "layer", "layer_only"


class Knob(NamedTuple):
    key: str
    default: object          # its type decides how a value is parsed: bool, int, float, else str
    kind: str
    doc: str
    per_layer: str = ""      # "" | LAYER | LAYER_ONLY
    auto: bool = False       # 0 = auto: the call site computes the value (per-layer: 0 falls
    #                          through to the next level, as the `or` chains it replaces did)
    layer_defaults: Optional[Dict[int, object]] = None   # defaults of single layers

    def parse(self, v: str):
        d = self.default
        if isinstance(d, bool):
            return v.lower() not in ("0", "false", "no", "off", "")
        if isinstance(d, int):
            return int(v)
        if isinstance(d, float):
            return float(v)
        return v


_NO_EVIDENCE = " (no bit-identity test: classed path)"

KNOBS: Tuple[Knob, ...] = (
    # ---------------------------------------------------------------- conv forward
    Knob("conv_stack", True, EXACT, "layer-fused forward conv stack (one workgroup per image row band, "
         "activations in LDS); 0: one launch per layer (tests/test_hip_model.py "
         "test_conv_stack_forward_matches_per_layer)"),
    Knob("stack_splits", 0, PATH, "row bands per image of the conv stack; 0 = auto: enough workgroups "
         "for 256 CUs, cdiv(256, batch)" + _NO_EVIDENCE, auto=True),
    Knob("stack_dbg", 0, ABLATION, "ConvStackArgs::dbg bit mask of timing ablations; only 128 (the "
         "generic prologue) is exact (test_stack_fast_prologue_bit_identical)"),
    Knob("stack_k16", True, EXACT, "the 4-channel first layer's tap-8 k-step as a 16x16x16 MFMA "
         "(test_stack_k16_tail_bit_identical)"),
    Knob("stack_spec", 2, EXACT, "layer-signature-specialised conv stack instance (conv_stack.hip "
         "kStackSigs): 0 generic, 1 12-wave instances, 2 a 16-wave instance first where one exists "
         "(+0.4 %, profiles/r5e_ab.txt)"),
    Knob("stack_fix", 1, EXACT, "the conv stack instance with the whole geometry fixed at compile time "
         "(stack_sig.h: the RPV stack at two row bands) where the plan's args equal its signature; 0: what "
         "stack_spec selects (profiles/stack_fix_ab.txt; tests/test_stack_fix.py)"),
    Knob("wt", 7, EXACT, "write-through (16-byte sc1) stores, bit mask: 1 stage outputs / argmax codes, "
         "2 backward gradients dP / dH, 4 wgrad slabs (profiles/r4b_ab_rpv.txt; "
         "test_write_through_stores_bit_identical)"),
    Knob("lds_layout", True, PATH, "bank-conflict-model LDS strides (models/lds_layout.py) for the "
         "stack's halo images, the halo conv and the halo wgrad; 0: dense strides" + _NO_EVIDENCE),
    Knob("conv_glds", True, PATH, "wide convs and the tiled wgrad stage through LDS-DMA loads (padded "
         "rows read a zero buffer)"),
    Knob("conv_big", True, PATH, "wide convs in 256-row / 8-wave blocks when the grid keeps "
         "conv_big_min blocks: half the L2 traffic per MFMA"),
    Knob("conv_big_min", 512, PATH, "fewest blocks of a conv_big grid"),
    Knob("conv_hs", True, PATH, "halo-staged wide conv (each input pixel DMA'd once per 32-channel chunk, "
         "not once per tap) for stride-1 layers and strided dgrads' parity classes"),
    Knob("conv_hs_ntc", 8, PATH, "n-tiles per block of the halo-staged conv (8: 116 VGPRs and 80 KB of "
         "LDS, two blocks per CU); 0: off"),
    Knob("conv_hs_dil", True, PATH, "halo-staged conv for input-dilated (strided dgrad) layers too"),
    Knob("conv_hs_wv", 8, PATH, "16: 16-wave / 512-row halo-staged blocks where the shape tiles into them"),
    Knob("conv_hs_order", 1, PATH, "1: the n-blocks of a row block adjacent on one XCD (legacy conv3 "
         "forward 103.0 -> 101.6 us, profiles/r6_conv_hs_order_ab.txt)"),
    Knob("conv_gl_nbuf", 3, PATH, "LDS ring slots of the per-tap LDS-DMA conv (conv_tile)"),
    Knob("halo_tm", 2, PATH, "m-tiles per wave per pass of the standalone halo conv (2: half the epilogue "
         "staging LDS, four workgroups per CU; legacy first conv 37.7 -> 26.8 us, "
         "profiles/r6_halo_tm_ab.txt); 4: the four-tile pass"),
    Knob("halo_min_wgs", 512, PATH, "fewest workgroups of a standalone halo conv launch (bounds its "
         "rows per block)"),
    Knob("conv_kpipe", True, PATH, "software-pipelined k loop with scalar tap offsets in the halo conv "
         "(ConvMMArgs::kpipe; Cs % 32 == 0)" + _NO_EVIDENCE),
    # ---------------------------------------------------------------- conv backward / wgrad
    Knob("dual_halo", True, PATH, "one launch for a conv layer's wgrad and dgrad; bit-identical to "
         "standalone launches only with early_reduce=0 (test_dual_launch_matches_standalone)"),
    Knob("dgrad_min_wgs", 256, PATH, "fewest workgroups of a dgrad co-scheduled with its wgrad"),
    Knob("dgrad_ntc", 1, PATH, "n-tiles per workgroup of a co-scheduled dgrad (1: each workgroup stages "
         "half the weights, the launch fits the CUs in one wave)"),
    Knob("dgrad_tm", 0, PATH, "co-scheduled dgrad m-tiles per wave per pass of conv layer <i>; 0 = the "
         "kernel's choice", per_layer=LAYER_ONLY, auto=True),
    Knob("dgrad_dbg", 0, EXACT, "ConvMMArgs::dbg A/B switches of the dgrad (exact ones only; 32: no "
         "one-batch prologue, test_dgrad_onebatch_prologue_bit_identical)"),
    Knob("wgrad_tile_ntc", 0, PATH, "cap on the n-tiles per block of the tiled (wide conv) wgrad; "
         "0 = auto: 8 / 4 / 2 by the layer's n-tiles", auto=True),
    Knob("wgrad_tile_fill", 1, PATH, "tiled wgrad split count: this many rounds of resident workgroups "
         "(two per CU), never one workgroup more (legacy conv3 wgrad 113 us at 486 workgroups, 185 us "
         "at 522; profiles/r6_wgrad_splits_ab.txt)"),
    Knob("wgrad_tile_wgs", 0, PATH, "tiled wgrad workgroups wanted; 0 = auto: wgrad_tile_fill rounds",
         auto=True),
    Knob("wgrad_tile_slab_mb", 64, PATH, "byte budget (MiB) of the tiled wgrad's partial slabs"),
    Knob("wgrad_block_px", 256, PATH, "pixels per block of the halo wgrad (first layer, a standalone "
         "launch: 512 = 8 RPV rows, +0.2-0.5 %, profiles/r4m_ab_rpv.txt, r4n_ab_rpv.txt)",
         per_layer=LAYER, layer_defaults={0: 512}),
    Knob("wgrad_max_rows", 8, PATH, "most rows per block of the halo wgrad", per_layer=LAYER),
    Knob("wgrad_fit", True, PATH, "conv layer <i>: prefer the largest block whose staging fits the halo "
         "wgrad's register pipeline (wgrad_halo_body.h WH_PX / WH_PY)", per_layer=LAYER_ONLY),
    Knob("wgrad_perm", True, PATH, "WgradArgs::kperm bit 0: the halo wgrad's k index <-> pixel permutation "
         "within a 32-pixel k-step" + _NO_EVIDENCE),
    Knob("wgrad_fast", True, PATH, "0 sets WgradArgs::kperm bit 1: the halo wgrad without its "
         "row-aligned fast path" + _NO_EVIDENCE),
    Knob("wgrad_slab_mb", 8, PATH, "byte budget (MiB) of a halo wgrad's partial slabs"),
    Knob("wgrad_splits", 0, PATH, "halo wgrad workgroups across its splits; 0 = auto: one round of "
         "resident workgroups (the generic instance's occupancy x CUs); changes the summation order "
         "(profiles/r2_v12_wgrad_split_sweep.txt)", per_layer=LAYER, auto=True),
    Knob("wgrad_spec", 1, EXACT, "layer-signature halo wgrad instances (csrc/kernels/wgrad_sig.h) where "
         "one matches; 0: always the generic kernels (tests/test_wgrad_sig.py)"),
    Knob("dgrad_spec", 1, EXACT, "dual launches whose co-scheduled dgrad geometry is fixed at compile time "
         "too (csrc/kernels/dual_halo_fix_body.h) where the dgrad signature matches; 0: the dual launch "
         "as without it (tests/test_dgrad_sig.py)"),
    Knob("wgrad_depth", 0, EXACT, "blocks of a halo wgrad split whose staging loads are in flight at once, in "
         "the launches that have a deep instance (csrc/kernels/wgrad_deep.hip: the RPV first layer): 0 the "
         "instance's own depth, 1 the depth-one kernels, d that depth where it is built "
         "(profiles/wgrad_depth_ab.txt; tests/test_wgrad_depth.py)"),
    # ---------------------------------------------------------------- dense
    Knob("dense_big_wgs", 256, PATH, "workgroups wanted for a large dense layer's forward (one per CU)"),
    Knob("dense_big_minks", 8, PATH, "fewest k-steps per split of a large dense layer's forward"),
    Knob("dense_waves", 2048, PATH, "16x16-tile waves wanted for a small dense layer's split-K forward"),
    Knob("dense_bwd2", True, PATH, "dense_bwd.hip kernels (per-wave pipelined wgrad, vectorised dX "
         "epilogue) where their 8-element alignment holds; 0: generic wgrad / split-K"),
    Knob("dual_dense", True, PATH, "one launch for a dense layer's wgrad and dX" + _NO_EVIDENCE),
    Knob("dw_ntt", 4, PATH, "most n-tiles per workgroup of dense_wgrad (4: twice the workgroups of 8 -- "
         "RPV +0.6 %, MNIST +1.2 %, profiles/r4s_ab_rpv.txt, r4s_ab_mnist.txt)"),
    Knob("dw_slab_mb", 8, PATH, "byte budget (MiB) of dense_wgrad's partial slabs"),
    Knob("dw_min_wgs", 256, PATH, "workgroups wanted for dense_wgrad (sets its batch splits)"),
    Knob("dw_order", 1, PATH, "dense_wgrad grid order; 1: the n groups of one feature group consecutive "
         "(legacy -5 us, profiles/r6_dense_wgrad_ab.txt)" + _NO_EVIDENCE),
    Knob("dw_late", True, PATH, "dense_wgrad at 4 waves / SIMD (legacy 1.070 -> 1.059 ms)" + _NO_EVIDENCE),
    Knob("dx_ntc", 0, PATH, "n-tiles per wave of dense_dx (1, 2, 4; test_dense_dx_tiles_agree); 0 = auto: "
         "the most that leaves dx_min_wgs workgroups", auto=True),
    Knob("dx_min_wgs", 256, PATH, "fewest workgroups of dense_dx (256: the RPV dense dX at 2 n-tiles per "
         "wave, 3 us faster than 512 one-tile workgroups, profiles/r4p_ab_rpv.txt)"),
    Knob("dense_opt", "auto", PATH, "the optimizer update inside the one-split dense wgrad: auto = only "
         "layers whose gradient is written in place (> 16 MB; legacy 1.269 -> 1.238 ms/step, "
         "profiles/r4c_ab_legacy.txt), truthy = every one-split layer, falsy = off "
         "(tests/test_dense_bwd.py)"),
    Knob("opt_nograd", True, PATH, "a dense wgrad with the fused update does not store the gradient it "
         "consumed (profiles/r6_dense_wgrad_ab.txt); 0 keeps it readable through the store"
         + _NO_EVIDENCE),
    # ---------------------------------------------------------------- head
    Knob("fuse_head", True, PATH, "the head launch runs the last dense layer's split-K epilogue; same "
         "activations, the loss metric differs in fp32 rounding (tests/test_head_edges.py)"),
    Knob("head_generic", False, EXACT, "1: the head kernel without its fast paths "
         "(test_head_fast_paths_bit_identical)"),
    # ---------------------------------------------------------------- reduction / optimizer
    Knob("red_lanes", 16, PATH, "slab partials per reduction split-lane (set_red_lanes); changes the "
         "summation order"),
    Knob("red_desc_max", 16, PATH, "most descriptors of the ONE end-of-step reduction table (RedTable "
         "capacity, MAX_RED); more: 1 MiB buckets and a separate optimizer launch"),
    Knob("fuse_optim", True, PATH, "the Keras update fused into the reduction launch (and, with "
         "dense_opt, the dense wgrad); 0: a separate optimizer launch"),
    Knob("early_reduce", True, PATH, "the first dual conv launch reduces + updates the head / dense "
         "groups in extra workgroups; fp32 last-bit differences (test_dual_launch_early_reduce_close)"),
    Knob("early_rfirst", 0, PATH, "where a dual launch's early-reduction workgroups sit in its grid: "
         "0 last, 1 first, 2 interleaved" + _NO_EVIDENCE),
    Knob("opt_packs", True, EXACT, "pack routes: the optimizer writes the updated weights' bf16 packs "
         "itself; 0: the next prologue re-packs (bit-identical together with pro_free, "
         "test_prologue_free_step_matches_prologue)"),
    Knob("opt_tiles", True, EXACT, "optim_kernel updates aligned dense routes in 2-D tile blocks writing "
         "whole 16-byte pack vectors (legacy Dense(512): ~190 us per update less; "
         "test_optimizer_pack_routes_match_repack)"),
    # ---------------------------------------------------------------- step structure
    Knob("pro_free", True, EXACT, "prologue-free step: the conv stack reads its images from the dataset "
         "through the cursor, the first dense launch runs the bookkeeping "
         "(test_prologue_free_step_matches_prologue)"),
    Knob("pro_dbg", 0, ABLATION, "prologue timing ablation: 1 no re-pack, 2 no gather"),
    Knob("skip", "", ABLATION, "launch names ('name/name') dropped from the eager launch sequence "
         "(scripts/gpu_skip_ablation.sh)"),
    # ---------------------------------------------------------------- data-parallel / xGMI
    Knob("comm_capture", True, PATH, "the all-reduces captured with the step into one HIP graph; 0: "
         "issued between graph segments (tests/comm_worker_gpu.py)"),
    Knob("comm_fork", "", PATH, "captured all-reduces on a forked comm stream: '' = only with more than "
         "one RCCL bucket to overlap, 0 = never (a linear graph), else always"),
    Knob("dp_optim_on_comm", True, PATH, "each bucket's update follows its all-reduce on the comm stream"),
    Knob("dp_early", True, PATH, "one-bucket data-parallel step: the head / dense groups reduced inside "
         "the backward (grad_only)"),
    Knob("dp_overlap", False, PATH, "gradients <= 16 MB at size > 1: 1 MiB buckets forked onto the comm "
         "stream (135.7 vs 103.0 us/step at N = 1, profiles/r5f_ab.txt)"),
    Knob("xgmi_push", True, PATH, "producer push: an early range goes to its owners' inboxes from the "
         "launch that reduces it"),
    Knob("xgmi_xchg", True, PATH, "exchange: early range and end-of-backward table all-reduced + updated "
         "in table launches, not the fused xGMI kernel"),
    Knob("xchg_at", "dual", PATH, "end: the early range's exchange as a launch of its own after the "
         "backward, not extra workgroups of the next dual launch"),
    Knob("xchg_split", True, PATH, "split exchange: owner half in the next dual launch, finish half in "
         "the end-of-backward launch; 0: both in the dual launch"),
    Knob("xchg_p1", False, PATH, "keep the exchange structure at one rank, to measure its fixed cost "
         "(profiles/r6_xchg_ab.txt)"),
    Knob("xchg_rfirst", 1, PATH, "where a dual launch's exchange workgroups sit in its grid (1 first: "
         "their waits overlap the convs)"),
    Knob("xchg_nx", 0, PATH, "looping exchange workgroups on separate GPUs; 0: one per table block"),
    Knob("xgmi_xchg_wg", 4, PATH, "looping exchange workgroups when ranks share a GPU; 0: one per block"),
    Knob("xgmi_shared_wg", 8, PATH, "most workgroups of the fused xGMI all-reduce when ranks share a GPU"),
    Knob("xgmi_mem", "uncached", PATH, "xGMI buffer allocation: uncached | finegrained "
         "(profiles/r2_v12_xgmi_mem_n1.txt)"),
    Knob("xgmi_fence", 1, PATH, "flag fences: 1 system-scope release + acquire, 2 agent-scope acquire, "
         "3 none but sc1 payload loads (opt-in until a multi-GPU run shows parity), 0 none"),
    Knob("xgmi_selftest_stress", 64, PATH, "back-to-back skewed launches of the xGMI admission self-test "
         "(results unaffected)"),
    # ---------------------------------------------------------------- reference oracle
    Knob("ref_bf16", False, PATH, "the CPU reference rounds to bf16 where the HIP kernels do (the "
         "bf16-faithful oracle)"),
)

_BY_KEY = {k.key: k for k in KNOBS}
_PARSED = None     # (the INTML_TUNE string, {item key: parsed value})


def _knob_of_item(item_key: str) -> Optional[Knob]:
    """The knob an INTML_TUNE item key names: a registered key (unless it exists only with a
    layer suffix), or a per-layer knob's key with a layer number."""
    k = _BY_KEY.get(item_key)
    if k is not None:
        return None if k.per_layer == LAYER_ONLY else k
    base = item_key.rstrip("0123456789")
    k = _BY_KEY.get(base) if base != item_key else None
    return k if k is not None and k.per_layer else None


def _parse(raw: str) -> dict:
    d = {}
    for item in raw.split(","):
        if not item.strip():
            continue
        key, eq, v = item.partition("=")
        key = key.strip()
        knob = _knob_of_item(key) if eq else None
        if knob is None:
            names = [k.key + ("<i>" if k.per_layer == LAYER_ONLY else "") for k in KNOBS]
            close = difflib.get_close_matches(key, names, n=3, cutoff=0.5)
            raise ValueError("INTML_TUNE: %s (closest registered keys: %s; the table: docs/TUNES.md)"
                             % ("unknown key %r" % key if eq else "item %r is not key=value" % item.strip(),
                                ", ".join(close) or "none"))
        try:
            d[key] = knob.parse(v.strip())
        except ValueError:
            raise ValueError("INTML_TUNE: %s=%s is not %s %s" % (key, v.strip(), "an" if isinstance(knob.default, int)
                                                                 else "a", type(knob.default).__name__)) from None
    return d


def tune(key: str, layer: Optional[int] = None):
    """The value of knob ``key``: its registered default unless ``INTML_TUNE`` overrides it,
    parsed as the default's type.  ``layer=i`` (per-layer knobs): ``key<i>``, then ``key``,
    then the default of that layer.  The string is validated when first parsed and re-parsed
    whenever the environment value changes."""
    global _PARSED
    raw = os.environ.get("INTML_TUNE", "")
    if _PARSED is None or _PARSED[0] != raw:
        _PARSED = (raw, _parse(raw))
    knob = _BY_KEY[key]
    vals = _PARSED[1]
    if not knob.per_layer:
        if layer is not None:
            raise KeyError("%s is not a per-layer knob" % key)
        return vals.get(key, knob.default)
    if layer is None:
        raise KeyError("%s is a per-layer knob: tune(%r, layer=i)" % (key, key))
    for k in ("%s%d" % (key, layer), key):
        v = vals.get(k)
        if v is not None and not (knob.auto and v == 0):
            return v
    return (knob.layer_defaults or {}).get(layer, knob.default)


def markdown() -> str:
    """The table as Markdown (docs/TUNES.md)."""
    out = ["# `INTML_TUNE` knobs", "",
           "Generated by `python -m cori_intml_examples_amd.utils.tune` from `utils/tune.py` (`KNOBS`); "
           "`tests/test_tune.py` keeps this file and the call sites in step with the table.", "",
           "`INTML_TUNE=\"key=value,key=value\"` overrides a knob; an unregistered key is an error.  Kinds: "
           "`exact` = A/B switch with bit-identical results, `path` = another kernel path, geometry or "
           "summation order (results within the usual tolerance), `ablation` = timing only, wrong results.  "
           "`key<i>`: per-layer knob, `key<i>=v` overrides conv layer `i` alone.", "",
           "| key | default | kind | doc |", "| --- | --- | --- | --- |"]
    for k in KNOBS:
        name = {"": k.key, LAYER: "%s, %s<i>" % (k.key, k.key), LAYER_ONLY: k.key + "<i>"}[k.per_layer]
        default = "0 = auto" if k.auto else repr(k.default) if isinstance(k.default, str) else str(k.default)
        for i, v in sorted((k.layer_defaults or {}).items()):
            default += " (layer %d: %s)" % (i, v)
        out.append("| `%s` | %s | %s | %s |" % (name, default, k.kind, k.doc.replace("|", "\\|")))
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    print(markdown(), end="")

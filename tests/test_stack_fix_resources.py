"""Compiler resource report of EVERY conv-stack instance the extension ships with the whole
geometry fixed at compile time (csrc/kernels/conv_stack_fix_body.h, conv_stack_fix.hip), compiled
alone from scripts/probes/stack_fix_probe.hip beside the kStackSigs instance it replaces (CPU:
hipcc cross-compiles gfx950, a few seconds).  What the change is for is fewer instructions in the
launch: the fixed instance must come out with fewer than its counterpart in the same compile --
an instance that did not would not ship -- with no scratch, no SGPR spills, VGPRs within the cap
of its 16 waves (128) and an occupancy not below the counterpart's
(profiles/stack_fix_kernel_resources.txt)."""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
PROBE = os.path.join(ROOT, "scripts", "probes", "stack_fix_probe.hip")
KDIR = os.path.join(ROOT, "cori_intml_examples_amd", "csrc", "kernels")

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                                reason="no hipcc")

_F = "_Z21conv_stack_fix_kernelI%sEv13ConvStackArgs"                                     # <SIG>
_C = "_Z17conv_stack_kernelILb1ELb0ELj%dELj%dELj%dELj0ELi%d%sEv13ConvStackArgs"           # <true, false, C0.., NTH>
# signature -> (its counterpart's layer codes, threads per workgroup, VGPR cap of that wave count)
PINS = {
    "12StackSigRpv2": ((24853, 18985, 19529), 1024, 128),
}


def test_stack_fix_kernel_resources():
    import kernel_resources as KR
    rows = {r["name"]: r for r in KR.report(PROBE, insts=True)}
    fixed = sorted(n for n in rows if "conv_stack_fix_kernel" in n)
    assert fixed == sorted(_F % s for s in PINS), fixed
    for sig, (codes, nth, cap) in PINS.items():
        r = rows[_F % sig]
        c = rows[_C % (codes + (nth, "E"))]
        print(sig, "fixed", r, "counterpart", c)
        assert r.get("scratch", 0) == 0 and c.get("scratch", 0) == 0, (r, c)
        assert r.get("sgpr_spill", 0) == 0 and r.get("vgpr_spill", 0) == 0, r
        assert r["vgpr"] <= cap and c["vgpr"] <= cap, (r, c)
        assert r.get("occ", 0) >= c.get("occ", 0) >= nth // 256, (r, c)      # all the workgroup's waves resident
        assert 0 < r["insts"] < c["insts"], (r, c)


def test_probe_covers_every_shipped_instance():
    """The probe instantiates what the extension's translation unit does: every
    STACK_FIX_DEFINE(SIG) of conv_stack_fix.hip."""
    probe = open(PROBE).read()
    shipped = re.findall(r"^STACK_FIX_DEFINE\((\w+)\);", open(os.path.join(KDIR, "conv_stack_fix.hip")).read(), re.M)
    assert len(shipped) == len(PINS) == 1, shipped
    probed = re.findall(r"^STACK_FIX_PROBE\((\w+),", probe, re.M)
    assert sorted(probed) == sorted(shipped), (probed, shipped)
    for sig in shipped:
        assert any(p.endswith(sig) for p in PINS), sig

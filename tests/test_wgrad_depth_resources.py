"""Compiler resource report of EVERY deep wgrad instance the extension ships (csrc/kernels/
wgrad_deep.hip: the RPV first layer's standalone kernel at DEPTH 2, in both input forms), compiled
alone from scripts/probes/wgrad_depth_probe.hip beside the non-pipelined depth-one form each
replaces (CPU: hipcc cross-compiles gfx950, ~10 s).  A deep instance holds DEPTH blocks' chunks in
registers, so it may use more VGPRs than the form it replaces -- but no scratch, no SGPR / VGPR
spills, and it stays inside that form's pin of tests/test_wgrad_sig_resources.py's generic
counterpart, VGPRs <= 168 and occupancy >= 3: the host sizes the split count to ONE round of
workgroups resident at that occupancy (wgrad_halo_resident), and the deep kernel must still run
it in one round (profiles/wgrad_depth_kernel_resources.txt):

    instance                          VGPRs / SGPR spills / occupancy / instructions
    deep, activation buffer           103 / 0 / 4 / 2,060        replaces  77 / 0 / 6 / 888
    deep, dataset rows (xidx)          96 / 0 / 5 / 1,202        replaces  77 / 0 / 6 / 891
"""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
PROBE = os.path.join(ROOT, "scripts", "probes", "wgrad_depth_probe.hip")
KDIR = os.path.join(ROOT, "cori_intml_examples_amd", "csrc", "kernels")

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                                reason="no hipcc")

_DEEP = "_Z22wgrad_halo_deep_kernelI%sLb%dELi%dEEv9WgradArgs"      # <SIG, XIDX, DEPTH>
_FLAT = "_Z21wgrad_halo_sig_kernelI%sLb0ELb%dEEv9WgradArgs"        # <SIG, false, XIDX>
# (signature, DEPTH) of the shipped instances; the bounds are the replaced form's generic pin
SHIPPED = [("9WgSigRpv1", 2)]
MAX_VGPR, MIN_OCC = 168, 3


def test_wgrad_depth_kernel_resources():
    import kernel_resources as KR
    rows = {r["name"]: r for r in KR.report(PROBE, insts=True)}
    deep = sorted(n for n in rows if "wgrad_halo_deep_kernel" in n)
    assert deep == sorted(_DEEP % (sig, x, d) for sig, d in SHIPPED for x in (0, 1)), deep
    for sig, d in SHIPPED:
        for xidx in (0, 1):
            r, c = rows[_DEEP % (sig, xidx, d)], rows[_FLAT % (sig, xidx)]
            print(sig, d, xidx, "deep", r, "replaces", c)
            assert r.get("scratch", 0) == 0 and c.get("scratch", 0) == 0, (r, c)
            assert r.get("sgpr_spill", 0) == 0 and r.get("vgpr_spill", 0) == 0, r
            assert 0 < r["vgpr"] <= MAX_VGPR, r
            assert r.get("occ", 0) >= MIN_OCC, r
            assert r["insts"] > 0 and c["insts"] > 0


def test_probe_covers_every_shipped_instance():
    """The probe instantiates what wgrad_deep.hip does -- every wgrad_deep_launch<SIG, DEPTH>, in both
    input forms -- and each launcher is in the signature table's deep rows."""
    probe = open(PROBE).read()
    unit = open(os.path.join(KDIR, "wgrad_deep.hip")).read()
    table = open(os.path.join(KDIR, "wgrad_sig.hip")).read()
    shipped = re.findall(r"^void (\w+)\(const WgradArgs& a, dim3 grid, size_t lds, hipStream_t s\) \{\n"
                         r"  wgrad_deep_launch<(\w+), (\d)>\(a, grid, lds, s\);", unit, re.M)
    assert len(shipped) == len(SHIPPED) == len(re.findall(r"wgrad_deep_launch<\w+, \d>", unit)), shipped
    assert len(re.findall(r"^WGRAD_DEEP_PROBE\(", probe, re.M)) == len(shipped)
    for (name, sig, depth), (msig, mdepth) in zip(shipped, SHIPPED):
        assert msig.endswith(sig) and int(depth) == mdepth
        assert "WGRAD_DEEP_PROBE(%s, %s);" % (sig, depth) in probe, (sig, depth)
        assert "{%s, %s}" % (depth, name) in table, name

"""Compiler resource report of EVERY layer-signature wgrad instance the extension ships
(csrc/kernels/wgrad_sig.h: 8 standalone forms -- 2 first-layer signatures x PIPE x XIDX -- and
6 duals), compiled alone from scripts/probes/wgrad_sig_probe.hip (CPU: hipcc cross-compiles
gfx950, ~35 s).  With the wgrad geometry fixed at compile time no instance needs scratch (the
duals take the 1.7 KB DualExtra by value: the trap tests/test_kernel_resources.py describes),
each has fewer VGPRs than its generic counterpart and a higher occupancy, and the SGPR spills
are pinned at what the report shows (profiles/wgrad_sig_kernel_resources.txt):
  * 0 for the eight standalone forms and the RPV duals at dgrad TM 4 (the B=128 step's);
  * 7 for the three duals at dgrad TM 1 (one-row dgrad blocks of small batches; their generic
    forms: 161 and a 20-byte private segment);
  * 11 for the MNIST dual at TM 2 -- with 24-wide rows in 5-row blocks neither the row-aligned
    k-step path nor the pooled expansion applies, so the body's general paths are what is
    compiled (generic form: 171)."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                                reason="no hipcc")

_W = "_Z21wgrad_halo_sig_kernelI%sLb%dELb%dEEv9WgradArgs"                           # <SIG, PIPE, XIDX>
_D = "_Z20dual_halo_sig_kernelI%sLi1ELi%dEEv10ConvMMArgs9WgradArgsiiii9DualExtra"   # <SIG, 1, TM>
R1, R2, R3, M1, M2 = "9WgSigRpv1", "9WgSigRpv2", "9WgSigRpv3", "11WgSigMnist1", "11WgSigMnist2"

# full mangled name -> (generic counterpart's VGPRs, pinned VGPRs, pinned SGPR spills, min occupancy)
PINS = {}
for xidx in (1, 0):
    PINS[_W % (R1, 0, xidx)] = (138, 77, 0, 3)     # wgrad_halo_kernel<1, 1, true, false, false>
    PINS[_W % (R1, 1, xidx)] = (142, 82, 0, 3)     # wgrad_halo_kernel<1, 1, true, true, false>
    PINS[_W % (M1, 0, xidx)] = (142, 54, 0, 3)     # wgrad_halo_kernel<1, 2, true, false, false>
    PINS[_W % (M1, 1, xidx)] = (147, 88, 0, 3)     # wgrad_halo_kernel<1, 2, true, true, false>
PINS[_D % (R2, 4)] = (204, 136, 0, 2)              # dual_halo_kernel<1, 4, 2, 4, false>
PINS[_D % (R2, 1)] = (204, 137, 7, 2)              # dual_halo_kernel<1, 4, 2, 1, false>
PINS[_D % (R3, 4)] = (236, 148, 0, 2)              # dual_halo_kernel<1, 4, 4, 4, false>
PINS[_D % (R3, 1)] = (236, 149, 7, 2)              # dual_halo_kernel<1, 4, 4, 1, false>
PINS[_D % (M2, 2)] = (236, 161, 11, 2)             # dual_halo_kernel<1, 4, 4, 2, false>
PINS[_D % (M2, 1)] = (236, 161, 7, 2)              # dual_halo_kernel<1, 4, 4, 1, false>


def test_wgrad_sig_kernel_resources():
    import kernel_resources as KR
    rows = {r["name"]: r for r in KR.report(os.path.join(ROOT, "scripts", "probes", "wgrad_sig_probe.hip"))
            if "_sig_kernel" in r["name"]}
    assert len(PINS) == 14 and sorted(rows) == sorted(PINS), sorted(rows)
    for name, (generic, vgpr, spill, occ) in PINS.items():
        r = rows[name]
        assert r.get("scratch", 0) == 0, r
        assert r.get("sgpr_spill", 0) <= spill, r
        assert r["vgpr"] <= vgpr < generic, r
        assert r.get("occ", 0) >= occ, r


def test_probe_covers_every_shipped_instance():
    """The probe instantiates what the extension's translation units do: every
    DUAL_SIG_DEFINE(name, SIG, TM) of dual_sig_*.hip, and PIPE x XIDX of every signature with a
    standalone launcher in wgrad_sig.hip's table."""
    import glob
    import re
    kdir = os.path.join(ROOT, "cori_intml_examples_amd", "csrc", "kernels")
    probe = open(os.path.join(ROOT, "scripts", "probes", "wgrad_sig_probe.hip")).read()
    duals = []
    for f in glob.glob(os.path.join(kdir, "dual_sig_*.hip")):
        duals += re.findall(r"^DUAL_SIG_DEFINE\(\w+, (\w+), (\d)\)", open(f).read(), re.M)
    assert len(duals) == 6
    for sig, tm in duals:
        assert "DUAL_SIG_PROBE(%s, %s);" % (sig, tm) in probe, (sig, tm)
    alone = re.findall(r"wgrad_sig_launch<(\w+)>", open(os.path.join(kdir, "wgrad_sig.hip")).read())
    assert len(alone) == 2
    for sig in alone:
        for pipe in ("false", "true"):
            for xidx in ("false", "true"):
                assert "wgrad_halo_sig_kernel<%s, %s, %s>" % (sig, pipe, xidx) in probe, (sig, pipe, xidx)

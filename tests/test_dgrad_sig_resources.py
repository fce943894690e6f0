"""Compiler resource report of EVERY dual instance the extension ships with the dgrad half's
geometry fixed at compile time too (csrc/kernels/dual_halo_fix_body.h, dual_fix_*.hip), compiled
alone from scripts/probes/dgrad_sig_probe.hip beside the dual_halo_sig_kernel instance each one
replaces (CPU: hipcc cross-compiles gfx950, ~25 s).  What the change is for is less code in the
launch: each fixed instance must come out with fewer instructions than its counterpart -- an
instance that did not would not ship -- with no scratch and SGPR spills, VGPRs and occupancy no
worse (profiles/dgrad_sig_kernel_resources.txt):

    instance        fixed: spills / VGPRs / occupancy / instructions    counterpart
    RPV conv2 TM 4         0 / 136 / 3 / 15,042                         0 / 136 / 3 / 24,962
    RPV conv3 TM 4         0 / 148 / 3 / 14,741                         0 / 148 / 3 / 25,121
    MNIST conv2 TM 2       0 / 160 / 3 / 15,052                         11 / 161 / 3 / 24,473

The pins are the counterpart's recorded spills / VGPRs and the occupancy the report shows (3; never
below the counterpart's in the same compile); the instruction bound is the counterpart's count in
the same compile."""
import glob
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
PROBE = os.path.join(ROOT, "scripts", "probes", "dgrad_sig_probe.hip")
KDIR = os.path.join(ROOT, "cori_intml_examples_amd", "csrc", "kernels")

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                                reason="no hipcc")

_F = "_Z20dual_halo_fix_kernelI%sLi%dEEv10ConvMMArgs9WgradArgsiiii9DualExtra"       # <DSIG, TM>
_D = "_Z20dual_halo_sig_kernelI%sLi1ELi%dEEv10ConvMMArgs9WgradArgsiiii9DualExtra"   # <SIG, 1, TM>
# (dgrad signature, wgrad signature, TM) -> the counterpart's (SGPR spills, VGPRs, min occupancy)
PINS = {
    ("9DgSigRpv2", "9WgSigRpv2", 4): (0, 136, 3),
    ("9DgSigRpv3", "9WgSigRpv3", 4): (0, 148, 3),
    ("11DgSigMnist2", "11WgSigMnist2", 2): (11, 161, 3),
}


def test_dgrad_sig_kernel_resources():
    import kernel_resources as KR
    rows = {r["name"]: r for r in KR.report(PROBE, insts=True)}
    fixed = sorted(n for n in rows if "dual_halo_fix_kernel" in n)
    assert fixed == sorted(_F % (d, tm) for d, _, tm in PINS), fixed
    for (dsig, wsig, tm), (spill, vgpr, occ) in PINS.items():
        r, c = rows[_F % (dsig, tm)], rows[_D % (wsig, tm)]
        print(dsig, tm, "fixed", r, "counterpart", c)
        assert r.get("scratch", 0) == 0, r
        assert r.get("sgpr_spill", 0) <= spill and c.get("sgpr_spill", 0) <= spill, (r, c)
        assert r["vgpr"] <= vgpr and c["vgpr"] <= vgpr, (r, c)
        assert r.get("occ", 0) >= max(occ, c.get("occ", 0)), (r, c)
        assert 0 < r["insts"] < c["insts"], (r, c)


def test_probe_covers_every_shipped_instance():
    """The probe instantiates what the extension's translation units do: every
    DUAL_FIX_DEFINE(name, DSIG, TM) of dual_fix_*.hip -- and each is in the signature table."""
    probe = open(PROBE).read()
    table = open(os.path.join(KDIR, "wgrad_sig.hip")).read()
    shipped = []
    for f in glob.glob(os.path.join(KDIR, "dual_fix_*.hip")):
        shipped += re.findall(r"^DUAL_FIX_DEFINE\((\w+), (\w+), (\d)\)", open(f).read(), re.M)
    assert len(shipped) == len(PINS) == 3, shipped
    assert len(re.findall(r"^DUAL_FIX_PROBE\(", probe, re.M)) == len(shipped)
    for name, dsig, tm in shipped:
        assert "DUAL_FIX_PROBE(%s, %s);" % (dsig, tm) in probe, (dsig, tm)
        assert "dg_sig_vals<%s>(), %s}" % (dsig, name) in table, name

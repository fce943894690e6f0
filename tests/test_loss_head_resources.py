"""Compiler resource report of the second head kernel (CPU: hipcc cross-compiles gfx950).
loss_head.hip has exactly four instances, {N = 1, N <= 16} x {unweighted, weighted}; none uses
scratch or spills a register.  head_kernel, which absorbs a dense epilogue and therefore keeps
far more state alive, spills 16..26 SGPRs per instance; this kernel spills none, and that is
pinned.  head.hip takes its shared code from the same header and must keep compiling to what it
compiled to before the header existed: its eight instances' figures are pinned too."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                                reason="no hipcc")


def test_loss_head_has_four_instances_without_scratch_or_spills():
    import kernel_resources as KR
    rs = KR.report(os.path.join(KR.KDIR, "loss_head.hip"))
    names = KR.demangle([r["name"] for r in rs])
    for nm, r in zip(names, rs):
        print(nm, r)
    want = {"loss_head_kernel<1, false>", "loss_head_kernel<1, true>", "loss_head_kernel<16, false>", "loss_head_kernel<16, true>"}
    assert len(rs) == 4 and {w for w in want for nm in names if w in nm} == want, names
    for nm, r in zip(names, rs):
        assert r.get("scratch", 0) == 0 and r.get("vgpr_spill", 0) == 0, (nm, r)
        assert r.get("sgpr_spill", 0) == 0, (nm, r)          # (what the compiler gives; head_kernel: up to 26)
        assert 0 < r["vgpr"] <= 64 and r.get("lds", 0) <= 9216, (nm, r)


def test_head_kernel_keeps_its_instances_with_the_shared_header():
    """head.hip includes the same head_common.h: still 8 head_kernel instances, no scratch, no
    VGPR spills, and per instance the VGPRs and SGPR spills it had when all of its code was its own
    (the compiler's figures of the commit before loss_head.hip; <RB, NM, WT> -> (VGPRs, SGPR spills))."""
    import kernel_resources as KR
    rs = [r for r in KR.report(os.path.join(KR.KDIR, "head.hip")) if "head_kernel" in r["name"]]
    names = KR.demangle([r["name"] for r in rs])
    want = {"<1, 1, true>": (46, 22), "<4, 1, true>": (45, 20), "<1, 16, true>": (53, 21), "<4, 16, true>": (58, 26),
            "<1, 1, false>": (45, 22), "<4, 1, false>": (45, 16), "<1, 16, false>": (51, 18), "<4, 16, false>": (57, 22)}
    assert len(rs) == 8
    got = {}
    for nm, r in zip(names, rs):
        print(nm, r)
        assert r.get("scratch", 0) == 0 and r.get("vgpr_spill", 0) == 0, r
        got[nm[nm.index("<"):nm.index(">") + 1]] = (r["vgpr"], r.get("sgpr_spill", 0))
    assert got == want

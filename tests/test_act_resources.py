"""Compiler resource report of the activation kernels (CPU: hipcc cross-compiles gfx950).
act_fwd_kernel / act_bwd_kernel are plain streaming kernels, one instance per activation: no
scratch, no VGPR / SGPR spills and no LDS in any of them."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                                reason="no hipcc")


def test_activation_kernels_use_no_scratch_and_spill_nothing():
    import kernel_resources as KR
    rs = KR.report(os.path.join(KR.KDIR, "act.hip"))
    names = KR.demangle([r["name"] for r in rs])
    for kernel in ("act_fwd_kernel", "act_bwd_kernel"):
        rows = [(nm, r) for r, nm in zip(rs, names) if kernel in nm]
        assert len(rows) == 8, names                     # one instance per row of ACT_TABLE
        for nm, r in rows:
            print(nm, r)
            assert r.get("scratch", 0) == 0 and r.get("vgpr_spill", 0) == 0 and r.get("sgpr_spill", 0) == 0, (nm, r)
            assert r["vgpr"] > 0 and r.get("lds", 0) == 0, (nm, r)

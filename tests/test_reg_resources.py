"""Compiler resource report of the weight-regularizer kernel (CPU: hipcc cross-compiles gfx950).
weight_reg_kernel indexes its by-value range table at run time; that must stay a read of the
kernel arguments, not a private copy: 0 bytes of scratch, no VGPR / SGPR spills."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                                reason="no hipcc")


def test_weight_reg_kernel_uses_no_scratch():
    import kernel_resources as KR
    rs = KR.report(os.path.join(KR.KDIR, "reg.hip"))
    names = KR.demangle([r["name"] for r in rs])
    rows = [r for r, nm in zip(rs, names) if "weight_reg_kernel" in nm]
    assert len(rows) == 1, names
    r = rows[0]
    print("weight_reg_kernel:", r)
    assert r.get("scratch", 0) == 0 and r.get("vgpr_spill", 0) == 0 and r.get("sgpr_spill", 0) == 0, r
    assert r["vgpr"] > 0 and r.get("lds", 0) == 32, r          # (the report is this kernel's: 8 floats of LDS)

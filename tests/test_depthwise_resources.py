"""Compiler resource report of the depthwise.hip kernels (CPU: hipcc cross-compiles gfx950): no
scratch, no VGPR / SGPR spills."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                                reason="no hipcc")


def test_depthwise_kernels_use_no_scratch_and_spill_nothing():
    import kernel_resources as KR
    rs = KR.report(os.path.join(KR.KDIR, "depthwise.hip"))
    rows = dict(zip(KR.demangle([r["name"] for r in rs]), rs))
    want = ["void dw_conv_kernel<%d, %d>(DwArgs)" % (v, k) for v in (4, 8) for k in (0, 1)]
    want += ["void dw_wgrad_kernel<%d>(DwArgs)" % v for v in (4, 8)]
    assert sorted(rows) == sorted(want), sorted(rows)
    for nm, r in sorted(rows.items()):
        print("%s: VGPR %d, SGPR %d, scratch %d, occupancy %d" % (nm, r["vgpr"], r["sgpr"], r.get("scratch", 0), r.get("occ", 0)))
        assert r.get("scratch", 0) == 0 and r.get("vgpr_spill", 0) == 0 and r.get("sgpr_spill", 0) == 0, (nm, r)

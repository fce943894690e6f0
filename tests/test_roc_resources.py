"""Compiler resource report of the ROC metric kernels (CPU: hipcc cross-compiles gfx950).  roc.hip holds
the unweighted and the weighted instance of roc_accum_kernel, which use registers and cross-lane
operations only (no LDS), and roc_finish_kernel, whose scan and fixed-order sum go through LDS; none
uses scratch or spills a register."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                                reason="no hipcc")


def test_roc_kernels_use_no_scratch_and_spill_nothing():
    import kernel_resources as KR
    rs = KR.report(os.path.join(KR.KDIR, "roc.hip"))
    names = KR.demangle([r["name"] for r in rs])
    want = {"roc_accum_kernel": 2, "roc_finish_kernel": 1}
    for kernel, count in want.items():
        rows = [(nm, r) for r, nm in zip(rs, names) if kernel in nm]
        assert len(rows) == count, names
        for nm, r in rows:
            print(nm, r)
            assert r.get("scratch", 0) == 0 and r.get("vgpr_spill", 0) == 0 and r.get("sgpr_spill", 0) == 0, (nm, r)
            assert r["vgpr"] > 0
            assert (r.get("lds", 0) == 0) == (kernel == "roc_accum_kernel"), (nm, r)
    assert sorted(nm for nm in names if "roc_accum_kernel" in nm)[0] != sorted(nm for nm in names if "roc_accum_kernel" in nm)[1]
    assert len(rs) == sum(want.values()), names

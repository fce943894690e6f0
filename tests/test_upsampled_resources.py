"""Compiler resource report of the upsampled.hip kernels (hipcc cross-compiles gfx950): exactly the expected
instances, no scratch, no VGPR / SGPR spills, static LDS within the budget (the stage itself is dynamic)."""
import os
import shutil
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")


def test_upsampled_kernels_use_no_scratch_and_spill_nothing():
    import kernel_resources as KR
    rs = KR.report(os.path.join(KR.KDIR, "upsampled.hip"))
    rows = dict(zip(KR.demangle([r["name"] for r in rs]), rs))
    want = ["void up_conv_kernel<%s, %d, %d>(UpArgs)" % (c, n, k)      # (CS4, NTW, KIND): no 4-lane or 4 n-tile dgrad
            for c, k in (("true", 0), ("false", 0), ("false", 1)) for n in (1, 2, 4) if (n, k) != (4, 1)]
    want += ["void up_wgrad_kernel<%s, %d>(UpArgs)" % (c, n) for c in ("true", "false") for n in (1, 2, 4)]
    assert sorted(rows) == sorted(want), sorted(rows)
    for nm, r in sorted(rows.items()):
        print("%s: VGPR %d, SGPR %d, LDS %d, occupancy %d" % (nm, r["vgpr"], r["sgpr"], r.get("lds", 0), r.get("occ", 0)))
        assert r.get("scratch", 0) == 0 and r.get("vgpr_spill", 0) == 0 and r.get("sgpr_spill", 0) == 0, (nm, r)
        assert r.get("lds", 0) <= 160 * 1024, (nm, r)

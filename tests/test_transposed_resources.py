"""Compiler resource report of the transposed.hip kernels (CPU: hipcc cross-compiles gfx950): exactly the
expected instances, no scratch, no VGPR / SGPR spills."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                                reason="no hipcc")


def test_transposed_kernels_use_no_scratch_and_spill_nothing():
    import kernel_resources as KR
    rs = KR.report(os.path.join(KR.KDIR, "transposed.hip"))
    rows = dict(zip(KR.demangle([r["name"] for r in rs]), rs))
    # (CS4, NTW, KIND): the forward for 4-lane and 8-lane inputs, the dgrad for 8-lane gradients and 1 or 2 n-tiles
    want = ["void tconv_conv_kernel<%s, %d, %d>(TconvArgs)" % (c, n, k)
            for c, k in (("true", 0), ("false", 0), ("false", 1)) for n in (1, 2, 4) if (n, k) != (4, 1)]
    # (a 4-lane input has at most 4 input channels: one n-tile)
    want += ["void tconv_wgrad_kernel<%s, %d>(TconvArgs)" % (c, n) for c, n in (("true", 1), ("false", 1), ("false", 2), ("false", 4))]
    assert sorted(rows) == sorted(want), sorted(rows)
    for nm, r in sorted(rows.items()):
        print("%s: VGPR %d, SGPR %d, scratch %d, occupancy %d" % (nm, r["vgpr"], r["sgpr"], r.get("scratch", 0), r.get("occ", 0)))
        assert r.get("scratch", 0) == 0 and r.get("vgpr_spill", 0) == 0 and r.get("sgpr_spill", 0) == 0, (nm, r)

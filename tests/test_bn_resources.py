"""Compiler resource report of the BatchNormalization kernels (CPU: hipcc cross-compiles gfx950).
The four bn.hip kernels stream 16-byte groups and reduce through LDS trees: no scratch and no
VGPR / SGPR spills in any of them."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                                reason="no hipcc")


def test_batchnorm_kernels_use_no_scratch_and_spill_nothing():
    import kernel_resources as KR
    rs = KR.report(os.path.join(KR.KDIR, "bn.hip"))
    names = KR.demangle([r["name"] for r in rs])
    for kernel in ("bn_stats_kernel", "bn_apply_fwd_kernel", "bn_bwd_reduce_kernel", "bn_bwd_apply_kernel"):
        rows = [(nm, r) for r, nm in zip(rs, names) if kernel in nm]
        assert len(rows) == 1, names
        for nm, r in rows:
            print(nm, r)
            assert r.get("scratch", 0) == 0 and r.get("vgpr_spill", 0) == 0 and r.get("sgpr_spill", 0) == 0, (nm, r)
            assert r["vgpr"] > 0 and 0 < r.get("lds", 0) <= 17 * 256 * 4, (nm, r)
    assert len(rs) == 4, names

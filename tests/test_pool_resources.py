"""Compiler resource report of the pooling kernels (CPU: hipcc cross-compiles gfx950).  The
pool.hip kernels are plain streaming kernels: no scratch, no VGPR / SGPR spills and no LDS in any
of them."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                                reason="no hipcc")


def test_pooling_kernels_use_no_scratch_and_spill_nothing():
    import kernel_resources as KR
    rs = KR.report(os.path.join(KR.KDIR, "pool.hip"))
    names = KR.demangle([r["name"] for r in rs])
    # one instance of each 2x2 kernel, a GAVG and a GMAX instance of each global kernel
    want = {"pool_avg2_fwd_kernel": 1, "pool_avg2_bwd_kernel": 1, "pool_global_fwd_kernel": 2, "pool_global_bwd_kernel": 2}
    for kernel, count in want.items():
        rows = [(nm, r) for r, nm in zip(rs, names) if kernel in nm]
        assert len(rows) == count, names
        for nm, r in rows:
            print(nm, r)
            assert r.get("scratch", 0) == 0 and r.get("vgpr_spill", 0) == 0 and r.get("sgpr_spill", 0) == 0, (nm, r)
            assert r["vgpr"] > 0 and r.get("lds", 0) == 0, (nm, r)
    assert len(rs) == sum(want.values()), names

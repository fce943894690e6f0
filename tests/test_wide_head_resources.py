"""Compiler resource report of the wide head kernel (CPU: hipcc cross-compiles gfx950): exactly two
instances, unweighted and weighted, neither with scratch or a spilled register; the static LDS is
the row metrics and weights only (the tiles are dynamic LDS, sized by the launcher)."""
import os
import shutil
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_wide_head_has_two_instances_without_scratch_or_spills():
    import kernel_resources as KR
    rs = KR.report(os.path.join(KR.KDIR, "wide_head.hip"))
    names = KR.demangle([r["name"] for r in rs])
    assert len(rs) == 2 and all(any(w in nm for nm in names) for w in ("wide_head_kernel<false>", "wide_head_kernel<true>")), names
    for nm, r in zip(names, rs):
        print(nm, r)
        assert r.get("scratch", 0) == 0 and r.get("vgpr_spill", 0) == 0 and r.get("sgpr_spill", 0) == 0, (nm, r)
        assert 0 < r["vgpr"] <= 128 and r.get("lds", 0) <= 512, (nm, r)

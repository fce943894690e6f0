"""Compiler resource report of the gradient-clipping kernels (CPU: hipcc cross-compiles gfx950).
The new kernels and the clipped optimizer instances use no scratch, and the unclipped optimizer
instances -- optim_kernel<KIND>, the CLIP = false form of the shared body -- report what they
reported before the clip existed."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                                reason="no hipcc")

# optim_kernel<KIND> on the commit before gradient clipping, from a build of that commit with
# scripts/kernel_resources.py (KIND: VGPRs; every instance: 46 SGPRs (the compiler's TotalSGPRs),
# 0 AGPRs, no SGPR / VGPR spills, no scratch, 2560 bytes of LDS, occupancy 8).  The comparison
# below is against these recorded values, not against anything measured on the new build.
PARENT_VGPR = {0: 34, 1: 49, 2: 40, 3: 46, 4: 57, 5: 50, 6: 49, 7: 58}
PARENT_REST = {"sgpr": 46, "agpr": 0, "sgpr_spill": 0, "vgpr_spill": 0, "scratch": 0, "lds": 2560, "occ": 8}


@pytest.fixture(scope="module")
def rows():
    import kernel_resources as KR
    out = {}
    for f in ("misc.hip", "clip.hip"):
        rs = KR.report(os.path.join(KR.KDIR, f))
        for r, nm in zip(rs, KR.demangle([r["name"] for r in rs])):
            out[nm] = r
    return out


def _family(rows, prefix):
    """{KIND: row} of the instances whose demangled name starts with ``void <prefix><KIND>>``."""
    got = {}
    for nm, r in rows.items():
        if nm.startswith("void " + prefix):
            got[int(nm.split(prefix)[1].split(">")[0])] = r
    return got


def test_clip_kernels_use_no_scratch(rows):
    for k in ("grad_sqnorm_kernel", "grad_clip_apply_kernel"):
        r = [r for nm, r in rows.items() if k in nm]
        assert len(r) == 1, (k, sorted(rows))
        print(k, r[0])
        assert r[0].get("scratch", 0) == 0 and r[0].get("vgpr_spill", 0) == 0 and r[0].get("sgpr_spill", 0) == 0, r
    clipped = _family(rows, "optim_clip_kernel<")
    assert sorted(clipped) == list(range(8)), sorted(clipped)
    for kind, r in sorted(clipped.items()):
        print("optim_clip_kernel<%d>: VGPR %d, scratch %d, LDS %d, occupancy %d" % (
            kind, r["vgpr"], r.get("scratch", 0), r.get("lds", 0), r.get("occ", 0)))
        assert r.get("scratch", 0) == 0 and r.get("vgpr_spill", 0) == 0, (kind, r)


def test_unclipped_instances_are_what_they_were(rows):
    plain = _family(rows, "optim_kernel<")
    assert sorted(plain) == list(range(8)), sorted(plain)
    for kind, r in sorted(plain.items()):
        assert r["vgpr"] == PARENT_VGPR[kind], (kind, r)
        assert "sgpr" in r, (kind, r)                 # (the report carries the SGPR count at all)
        for key, want in PARENT_REST.items():
            assert r.get(key, 0) == want, (kind, key, r)

"""The data plane of a wide-head model (CPU): RCCL only, gated the way clipping is."""
import pytest

from cori_intml_examples_amd import optim
from cori_intml_examples_amd.parallel.dist import plane_for_optimizer


@pytest.mark.parametrize("plane", ["xgmi", "hybrid"])
def test_wide_head_models_stay_on_the_rccl_plane(plane):
    opt = optim.Adam()
    assert plane_for_optimizer(plane, opt, forced=False) == plane                       # a narrow head: untouched
    assert plane_for_optimizer(plane, opt, forced=False, wide_head=("dense_2",)) == "rccl"   # auto falls back
    assert plane_for_optimizer("rccl", opt, forced=True, wide_head=("dense_2",)) == "rccl"
    with pytest.raises(ValueError, match="output layer dense_2 is wider than 16 units.*%r data plane" % plane):
        plane_for_optimizer(plane, opt, forced=True, wide_head=("dense_2",))

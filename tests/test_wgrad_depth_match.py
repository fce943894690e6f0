"""The host's choice of the halo wgrad instance that keeps every block of a split in flight
(K.wgrad_depth_variant, the query launch_wgrad_halo's own decision goes through): the deep
standalone kernel exactly where the launch takes a signature's non-pipelined form, the signature
has a deep instance and WgradArgs::depth is 0 or that instance's depth; depth 1 everywhere else.
No GPU: the query is host arithmetic on argument structs; the device pointers are stand-in
non-null addresses that nothing reads.

The args are written out from scripts/plan_dump.py's dump of the RPV and MNIST bench models' B = 128
training plans, not read from the signature table under test; the expected depths are the
instances wgrad_deep.hip ships."""
import pytest

from cori_intml_examples_amd.ops.hip import kernels

K = kernels()          # the project's loader: a missing or broken extension is an error, not a skip

PTR = 1 << 20
CONV = dict(KH=3, KW=3, stride=1)
# WgradArgs ints of the conv layers that run in dual launches (no deep instance), MT, NTT
OTHERS = {
    "rpv_conv2": (dict(H=32, W=32, Cs_in=16, Ho=32, Wo=32, pad_t=1, pad_l=1, Ktiles=9, NT=2, Cs_dy=32, dHp=16, dWp=16,
                       R=8, xpix=16, xrow=34, dyld=48), 9, 2),
    "rpv_conv3": (dict(H=16, W=16, Cs_in=32, Ho=16, Wo=16, pad_t=1, pad_l=1, Ktiles=18, NT=4, Cs_dy=64, dHp=8, dWp=8,
                       R=8, xpix=48, xrow=18, dyld=80), 9, 4),
}
# name -> (WgradArgs ints, pooled dY, MT, NTT, depth of the shipped deep standalone kernel or 1)
FIRST = {
    "rpv_conv1": (dict(H=64, W=64, Cs_in=4, Ho=64, Wo=64, pad_t=1, pad_l=1, Ktiles=3, NT=1, Cs_dy=16, dHp=32, dWp=32,
                       R=8, xpix=4, xrow=74, dyld=16), True, 3, 1, 2),
    "mnist_conv1": (dict(H=28, W=28, Cs_in=4, Ho=26, Wo=26, pad_t=0, pad_l=0, Ktiles=3, NT=2, Cs_dy=32, dHp=0, dWp=0,
                         R=8, xpix=4, xrow=42, dyld=48), False, 3, 2, 1),
}


def _wa(ints, bs, pooled=True, bps=2):
    wa = K.WgradArgs()
    for k, v in dict(ints, B=bs, kperm=1, wt=1, blocks_per_split=bps, **CONV).items():
        setattr(wa, k, v)
    wa.x = wa.dy = wa.slab = wa.bslab = PTR
    wa.dy_code = PTR if pooled else 0
    return wa


@pytest.mark.parametrize("name", sorted(OTHERS))
def test_layers_without_a_standalone_instance(name):
    w, MT, NTT = OTHERS[name]
    for bs, splits, bps in ((128, 86, 3), (5, 10, 1)):
        wa = _wa(w, bs, True, bps)
        assert K.wgrad_halo_variant(wa, MT, NTT) == 0
        assert K.wgrad_depth_variant(wa, MT, NTT, splits) == 1
        wa.depth = 2
        assert K.wgrad_depth_variant(wa, MT, NTT, splits) == 1


@pytest.mark.parametrize("name", sorted(FIRST))
def test_first_layer_depth(name):
    w, pooled, MT, NTT, depth = FIRST[name]
    for bs, splits, bps in ((128, 512, 2), (3, 24, 1), (5, 40, 1), (256, 683, 3), (64, 512, 1)):
        wa = _wa(w, bs, pooled, bps)
        assert wa.depth == 0 and wa.spec == 1                    # the struct's defaults
        assert K.wgrad_halo_variant(wa, MT, NTT) > 0
        assert K.wgrad_depth_variant(wa, MT, NTT, splits) == depth, (bs, splits)   # the non-pipelined form's place
        wa.xidx = wa.xst = PTR                                   # dataset rows: the same choice
        assert K.wgrad_depth_variant(wa, MT, NTT, splits) == depth
        wa.depth = 1
        assert K.wgrad_depth_variant(wa, MT, NTT, splits) == 1
        for d in (3, 4, 18, -1):                                 # not built
            wa.depth = d
            assert K.wgrad_depth_variant(wa, MT, NTT, splits) == 1, d
        wa.depth = 2                                             # asked for by its number
        assert K.wgrad_depth_variant(wa, MT, NTT, splits) == depth
    # fewer than 512 workgroups streaming several blocks each: the launch takes the depth-one PIPELINED form
    wa = _wa(w, 5, pooled, 3)
    assert K.wgrad_depth_variant(wa, MT, NTT, 14) == 1
    assert K.wgrad_depth_variant(_wa(w, 5, pooled, 1), MT, NTT, 40) == depth       # (one block per split: not pipelined)
    for field, value in (("spec", 0), ("xpix", 0), ("R", 4), ("Cs_dy", 8), ("dbg", 16), ("ts2", PTR)):
        wa = _wa(w, 128, pooled)
        setattr(wa, field, value)
        assert K.wgrad_depth_variant(wa, MT, NTT, 512) == 1, field

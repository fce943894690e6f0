"""The host's choice of the dual instance with the dgrad geometry fixed at compile time
(K.dual_halo_dgrad_fixed, the query launch_dual_halo's own decision goes through): true for the
three shipped dgrad signatures at any batch, false as soon as one field of the dgrad args, the
picked TM, either spec switch or a decline rule differs.  No GPU: the query is host arithmetic
on argument structs; the device pointers are stand-in non-null addresses that nothing reads.

The args are written out from scripts/plan_dump.py's dump of the bench models' B = 128 training
plans (the ca / wa of wgrad_dgrad_conv1 and wgrad_dgrad_conv2), not read from the signature
table under test."""
import pytest

from cori_intml_examples_amd.ops.hip import kernels

K = kernels()          # the project's loader: a missing or broken extension is an error, not a skip

PTR = 1 << 20
CONV = dict(KH=3, KW=3, stride=1)
# name -> (ConvMMArgs ints, BwdThrough ints, WgradArgs ints, MT, NTT)
LAYERS = {
    "rpv_conv2": (dict(H=32, W=32, Cs_in=32, Ho=32, Wo=32, pad_t=1, pad_l=1, KS=9, NT=1, R=16, in_pH=16, in_pW=16,
                       xpix=48),
                  dict(pH=32, pW=32, cH=64, cW=64, pC=16, pCs=16, prev_pool=1),
                  dict(H=32, W=32, Cs_in=16, Ho=32, Wo=32, pad_t=1, pad_l=1, Ktiles=9, NT=2, Cs_dy=32, dHp=16, dWp=16,
                       R=8, xpix=16, xrow=34, dyld=48), 9, 2),
    "rpv_conv3": (dict(H=16, W=16, Cs_in=64, Ho=16, Wo=16, pad_t=1, pad_l=1, KS=18, NT=2, R=16, in_pH=8, in_pW=8,
                       xpix=80),
                  dict(pH=16, pW=16, cH=32, cW=32, pC=32, pCs=32, prev_pool=1),
                  dict(H=16, W=16, Cs_in=32, Ho=16, Wo=16, pad_t=1, pad_l=1, Ktiles=18, NT=4, Cs_dy=64, dHp=8, dWp=8,
                       R=8, xpix=48, xrow=18, dyld=80), 9, 4),
    "mnist_conv2": (dict(H=24, W=24, Cs_in=64, Ho=26, Wo=26, pad_t=2, pad_l=2, KS=18, NT=2, R=13, in_pH=12, in_pW=12,
                         xpix=0),
                    dict(pH=26, pW=26, cH=26, cW=26, pC=32, pCs=32, prev_pool=0),
                    dict(H=26, W=26, Cs_in=32, Ho=24, Wo=24, pad_t=0, pad_l=0, Ktiles=18, NT=4, Cs_dy=64, dHp=12,
                         dWp=12, R=5, xpix=48, xrow=26, dyld=80), 9, 4),
}


def _args(name, bs=128):
    c, t, w, MT, NTT = LAYERS[name]
    ca, wa = K.ConvMMArgs(), K.WgradArgs()
    for k, v in dict(c, B=bs, in_dil=1, mode=1, kpipe=1, **CONV).items():
        setattr(ca, k, v)
    bt = ca.bt
    for k, v in dict(t, prev_relu=1, wt=1).items():
        setattr(bt, k, v)
    bt.dy = bt.prev_out = PTR
    ca.bt = bt
    ca.x = ca.in_code = ca.wpk = ca.st = PTR
    for k, v in dict(w, B=bs, kperm=1, wt=1, blocks_per_split=1, **CONV).items():
        setattr(wa, k, v)
    wa.x = wa.dy = wa.dy_code = wa.slab = wa.bslab = PTR
    return ca, wa, MT, NTT


def _fixed(ca, wa, MT, NTT):
    return K.dual_halo_dgrad_fixed(ca, 1, wa, MT, NTT)


@pytest.mark.parametrize("name", sorted(LAYERS))
@pytest.mark.parametrize("bs", [128, 256, 1024])
def test_signature_args_take_the_fixed_kernel(name, bs):
    ca, wa, MT, NTT = _args(name, bs)
    assert ca.spec == 1 and wa.spec == 1                       # the structs' defaults
    assert K.dual_halo_variant(ca, 1, wa, MT, NTT) > 0
    assert _fixed(ca, wa, MT, NTT)
    assert K.dual_halo_dgrad_fixed(ca, 1, wa, MT, NTT, extras=True)


@pytest.mark.parametrize("name", sorted(LAYERS))
def test_any_difference_declines(name):
    def differs(on, field, value):
        ca, wa, MT, NTT = _args(name)
        tgt = {"ca": ca, "wa": wa, "bt": ca.bt}[on]
        assert getattr(tgt, field) != value, (on, field)
        setattr(tgt, field, value)
        if on == "bt":
            ca.bt = tgt
        return _fixed(ca, wa, MT, NTT)

    c, t = LAYERS[name][0], LAYERS[name][1]
    assert not differs("ca", "spec", 0)                        # dgrad_spec=0
    assert not differs("wa", "spec", 0)                        # wgrad_spec=0: no signature launch at all
    assert not differs("ca", "R", c["R"] // 2 or 1)            # a smaller batch's blocks (and another TM)
    assert not differs("ca", "xpix", c["xpix"] + 8)            # another LDS layout
    assert not differs("ca", "kpipe", 0)
    assert not differs("ca", "tm", 2 if name != "mnist_conv2" else 1)   # a host TM override
    assert not differs("ca", "in_dil", 2)
    assert not differs("ca", "in_code", 0)                     # an unpooled dY
    assert not differs("ca", "KS", c["KS"] + 1)
    assert not differs("ca", "pad_t", c["pad_t"] + 1)
    assert not differs("bt", "pC", t["pC"] - 1)                # a previous stage with padded channels
    assert not differs("bt", "prev_relu", 0)
    assert not differs("bt", "wt", 0)                          # wt without bit 2
    assert not differs("ca", "dbg", 32)                        # a diagnostics launch: no dual at all
    assert not differs("wa", "R", 4)                           # the wgrad half matches no signature
    ca, wa, MT, NTT = _args(name)
    assert not K.dual_halo_dgrad_fixed(ca, 2, wa, MT, NTT)     # two n-tiles per workgroup
    assert not K.dual_halo_dgrad_fixed(ca, 1, wa, MT, NTT, xp=True)   # producer-push extras: generic kernel

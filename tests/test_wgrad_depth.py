"""The halo weight-gradient instance that keeps every block of a split in flight
(csrc/kernels/wgrad_halo_body.h DEPTH > 1: wgrad_deep.hip, the RPV first layer's standalone
kernel) against the depth-one kernel it replaces (wgrad_depth=1): whole training steps
bit-identical -- every gradient buffer the dgrads write (the plan's conv_dy), every partial slab,
the master weights, the metrics -- and the launcher picks the deep instance exactly where it has
one: the RPV bench model's first-layer wgrad, at any batch, on both input routes (dataset rows
through xidx, the uploaded batch).

The splits a deep pipeline can get wrong are the ones whose block count is not DEPTH: a tail split
shorter than the ring (its loads clamp to the split's last block) and a split longer than it (the
stages wrap).  The cases are chosen so that a full split, a one-block tail and a wrap each occur,
and the test reads blocks_per_split and the block count from the plan's args and checks that they
do, so a geometry change cannot silently drop one.  The first layer has 8 * B blocks in splits of
two for every B in 128..160 (its tail split is always full there), and a launch of fewer than 512
workgroups with several blocks each takes the depth-one PIPELINED form, not this kernel; so the
one-block tail of a multi-block split is B = 200's (1600 blocks in 534 splits of three).

Which kernel the launch takes is the launcher's host-side query K.wgrad_depth_variant (it shares
the launch's decline rules and signature lookup) asked on the plan's args, not a record of the
launch; that the B=128 step really runs the deep kernel is in the kernel trace
profiles/wgrad_depth_rpv_sequence_deep.txt.

The dual launches (conv2, conv3) have no deep instance: their candidates were measured and dropped
(docs/ARCHITECTURE.md section 15), so they run what they ran -- the test checks that at B >= 128 they
still take the kernels with the fixed dgrad.  The rule of the first-layer launch is the standalone
signature's own: it does not depend on the batch or on dgrad_spec, so of the declines below only
the ones that change ITS args (conv sizes, lds_layout, wgrad_spec) take its deep instance away."""
import numpy as np
import pytest
import torch

from cori_intml_examples_amd.apps import zoo
from cori_intml_examples_amd.utils import set_random_seed

pytestmark = pytest.mark.gpu


def _build(kind, opt, drop, cin):
    if kind == "rpv_bench":       # DistTrain_rpv: 64x64x{1,3}, conv[16,32,64] fc[128]
        return zoo.rpv_cnn((64, 64, cin), conv_sizes=[16, 32, 64], fc_sizes=[128], dropout=drop,
                           optimizer=opt, lr=1e-3, device="cuda")
    if kind == "rpv_small":       # same stack, conv sizes no signature is instantiated for
        return zoo.rpv_cnn((64, 64, cin), conv_sizes=[8, 16, 32], fc_sizes=[128], dropout=drop,
                           optimizer=opt, lr=1e-3, device="cuda")
    assert kind == "mnist_bench"  # DistTrain_mnist: 28x28x1, conv 32-64, fc 128
    return zoo.mnist_cnn(32, 64, 128, dropout=drop, optimizer=opt, lr=1e-3, input_shape=(28, 28, 1), device="cuda")


def _data(model, n, seed):
    rs = np.random.RandomState(seed)
    x = torch.tensor(rs.rand(n, *model.input_shape[1:]).astype(np.float32)).to(torch.bfloat16).float().numpy()
    nout = model.output_shape[-1]
    y = (rs.rand(n) > 0.5).astype(np.float32) if nout == 1 else np.eye(nout, dtype=np.float32)[rs.randint(0, nout, n)]
    return x, y


def _run(kind, opt, drop, cin, bs, tunes, monkeypatch):
    """Two training steps at batch bs; returns (conv_dy buffers, slabs, master, metrics,
    {conv layer: (depth the launch runs, blocks_per_split, blocks, xidx route, a dual: its dgrad is the fixed one)})."""
    monkeypatch.setenv("INTML_TUNE", tunes)
    set_random_seed(61)
    m = _build(kind, opt, drop, cin)
    x, y = _data(m, 2 * bs, seed=23)
    ex = m._executor
    d = ex.upload(x, y)
    perm = torch.randperm(d.n, generator=torch.Generator().manual_seed(29)).to(ex.device)
    ex.reset_metrics()
    ex.train_steps(d, perm, 0, bs, 2)
    torch.cuda.synchronize()
    plan = ex._plans[(bs, "train")]
    K = ex.K
    info, fixed = {}, {}
    for it in plan.launches:
        if it[0].startswith("wgrad_conv"):
            wa, cfg, layer = it.args["wa"], it.args["cfg"], int(it[0][len("wgrad_conv"):])
            depth = K.wgrad_depth_variant(wa, *cfg)
        elif it[0].startswith("wgrad_dgrad_conv"):   # a dual launch: no deep instance, depth one
            ca, ntc, wa, cfg = (it.args[r] for r in ("ca", "ntc", "wa", "cfg"))
            layer, depth = int(it[0][len("wgrad_dgrad_conv"):]), 1
            fixed[layer] = K.dual_halo_dgrad_fixed(ca, ntc, wa, cfg[0], cfg[1])
        else:
            continue
        blocks = wa.B * ((wa.Ho + wa.R - 1) // wa.R)
        assert cfg[2] == (blocks + wa.blocks_per_split - 1) // wa.blocks_per_split
        info[layer] = (depth, wa.blocks_per_split, blocks, bool(wa.xidx), fixed.get(layer))
    dys = [t.clone() for t in plan.conv_dy if t is not None]
    slabs = [t.clone() for pair in plan.wgrad_slabs for t in pair if t is not None]
    return dys, slabs, m.store.master[:m.store.numel].clone(), ex.read_metrics(), info


def _pair(kind, opt, drop, cin, bs, extra, monkeypatch):
    """The default and the wgrad_depth=1 arms of one case, after checking they computed the same."""
    res = [_run(kind, opt, drop, cin, bs, ",".join(t for t in (extra, dp) if t), monkeypatch)
           for dp in ("", "wgrad_depth=1")]
    nconv = 3 if kind.startswith("rpv") else 2
    assert len(res[0][0]) == len(res[1][0]) == nconv          # a gradient buffer per conv stage
    assert len(res[0][1]) == len(res[1][1]) >= 2 * nconv
    for a, b in zip(res[0][0] + res[0][1], res[1][0] + res[1][1]):
        assert a.shape == b.shape and torch.equal(a, b)
    assert float(res[0][0][0].float().abs().sum()) > 0        # the first stage's gradient: a dgrad wrote it
    assert torch.equal(res[0][2], res[1][2])
    assert res[0][3] == res[1][3]
    assert sorted(res[0][4]) == sorted(res[1][4]) == list(range(nconv))
    assert {k: v[1:] for k, v in res[0][4].items()} == {k: v[1:] for k, v in res[1][4].items()}   # the same splits
    assert all(v[0] == 1 for v in res[1][4].values()), res[1][4]   # wgrad_depth=1: never a deep kernel
    return res[0][4]


DEPTH = 2          # wgrad_deep.hip: the first layer's instance


def _shape(info, layer=0):
    """(blocks per full split, blocks of the tail split) of a conv layer's wgrad."""
    _, bps, blocks = info[layer][:3]
    return bps, blocks - (blocks - 1) // bps * bps


# (optimizer, dropout, channels, batch, extra tune, the first layer's (blocks per split, tail blocks))
DEEP = [
    ("Adam", 0.2, 3, 128, "", (2, 2)),                      # the bench step: full splits of DEPTH blocks
    ("SGD", 0.0, 1, 128, "", (2, 2)),
    ("Adam", 0.2, 3, 256, "", (3, 2)),                      # more blocks per split than DEPTH: the ring wraps
    ("Adam", 0.2, 3, 130, "", (2, 2)),                      # 1040 blocks in 520 workgroups
    ("Adam", 0.2, 3, 200, "", (3, 1)),                      # 1600 blocks in 534 splits: a wrap and a one-block tail (the clamp)
    ("Adam", 0.2, 3, 5, "", (1, 1)),                        # one block per split: both stages hold it
    ("Adam", 0.2, 3, 3, "", (1, 1)),
    ("Adam", 0.2, 3, 3, "pro_free=0", (1, 1)),              # the uploaded-batch route
    ("Adam", 0.2, 3, 5, "pro_free=0", (1, 1)),
    ("Adam", 0.2, 3, 128, "pro_free=0", (2, 2)),
    ("Adam", 0.2, 3, 200, "pro_free=0", (3, 1)),
]


@pytest.mark.parametrize("opt,drop,cin,bs,extra,shape", DEEP)
def test_wgrad_depth_bit_identical(opt, drop, cin, bs, extra, shape, monkeypatch):
    info = _pair("rpv_bench", opt, drop, cin, bs, extra, monkeypatch)
    print(bs, extra, info)
    assert {k: v[0] for k, v in info.items()} == {0: DEPTH, 1: 1, 2: 1}, info
    assert info[0][3] == ("pro_free=0" not in extra), info         # dataset rows through xidx / the uploaded batch
    assert _shape(info) == shape, info
    if bs >= 128:
        assert info[1][4] and info[2][4], info                     # the duals: still the fixed-dgrad kernels


def test_cases_cover_full_tail_and_wrap():
    shapes = {c[5] for c in DEEP}
    assert (DEPTH, DEPTH) in shapes                                 # a full split of exactly the ring
    assert any(bps > DEPTH for bps, _ in shapes)                    # a wrap
    assert any(bps > 1 and tail == 1 for bps, tail in shapes)       # a one-block tail of a multi-block split
    assert (1, 1) in shapes                                         # a split shorter than the ring everywhere


# (kind, batch, extra tune, the first-layer launch stays deep)
DECLINES = [
    ("rpv_bench", 64, "", True),                    # the signature does not depend on the batch
    ("rpv_small", 128, "", False),                  # conv sizes [8, 16, 32]: no signature at all
    ("rpv_bench", 128, "lds_layout=0", False),      # other LDS strides: no signature matches
    ("rpv_bench", 128, "wgrad_spec=0", False),      # the generic kernels
    ("rpv_bench", 128, "dgrad_spec=0", True),       # concerns the duals' dgrad only
    ("rpv_bench", 128, "wgrad_depth=3", False),     # a depth that is not built: the depth-one kernel
    ("rpv_bench", 5, "wgrad_splits0=16", False),    # 14 workgroups of 3 blocks: the depth-one PIPELINED form
    ("mnist_bench", 128, "", False),                # no MNIST instance ships (its first layer's dY is unpooled)
]


@pytest.mark.parametrize("kind,bs,extra,first_deep", DECLINES)
def test_wgrad_depth_declines(kind, bs, extra, first_deep, monkeypatch):
    info = _pair(kind, "Adam", 0.2, 3 if kind != "mnist_bench" else 1, bs, extra, monkeypatch)
    want = {k: 1 for k in info}
    if first_deep:
        want[0] = DEPTH
    assert {k: v[0] for k, v in info.items()} == want, info

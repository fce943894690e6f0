"""Layer-signature instances of the halo weight-gradient kernels (csrc/kernels/wgrad_sig.h:
the wgrad geometry as compile-time constants) against the generic kernels (wgrad_spec=0):
whole training steps bit-identical -- every partial slab, the master weights, the metrics --
and the launcher really picks a signature instance where one exists, the generic kernel
where none does.  The split count is sized by the generic instance in both arms, so the slab
layout and the fp32 reduction order are the same.

The variant numbers are the launchers' host-side queries (K.wgrad_halo_variant,
K.dual_halo_variant, which share the launch's decline rules and signature lookup) asked on the
plan's args, not a record of what each launch took; that the B=128 steps really run the
signature kernels is in the kernel traces profiles/wgrad_sig_{rpv,mnist}_sequence_spec.txt."""
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
    """Two training steps at batch bs; returns (slabs, master, metrics, per-conv-layer launch info)."""
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
    info = {}
    for it in plan.launches:
        if it[0].startswith("wgrad_conv"):
            wa, cfg = it.args["wa"], it.args["cfg"]
            info[it[0][len("wgrad_conv"):]] = (K.wgrad_halo_variant(wa, cfg[0], cfg[1]), wa.blocks_per_split, cfg[2])
        elif it[0].startswith("wgrad_dgrad_conv"):
            ca, ntc, wa, cfg = (it.args[r] for r in ("ca", "ntc", "wa", "cfg"))
            info[it[0][len("wgrad_dgrad_conv"):]] = (K.dual_halo_variant(ca, ntc, wa, cfg[0], cfg[1]),
                                                     wa.blocks_per_split, cfg[2])
    slabs = [t.clone() for pair in plan.wgrad_slabs for t in pair if t is not None]
    return slabs, m.store.master[:m.store.numel].clone(), ex.read_metrics(), info


# (kind, optimizer, dropout, channels, batch, extra tune, {conv layer: (blocks_per_split, splits)} to check)
CASES = [
    ("rpv_bench", "Adam", 0.2, 3, 128, "", {}),                  # production split geometry
    # blocks_per_split >= 2 with a short last split: conv1 has 5 x 8 = 40 blocks -> 3 per split, 14 splits
    ("rpv_bench", "SGD", 0.0, 1, 5, "wgrad_splits=16", {"0": (3, 14)}),
    ("rpv_bench", "Adam", 0.0, 3, 2, "", {"0": (1, 16)}),        # one block per split
    ("mnist_bench", "Adam", 0.3, 1, 128, "", {}),
    ("mnist_bench", "SGD", 0.0, 1, 3, "", {}),
]


@pytest.mark.parametrize("kind,opt,drop,cin,bs,extra,splits", CASES)
def test_wgrad_sig_bit_identical(kind, opt, drop, cin, bs, extra, splits, monkeypatch):
    res = [_run(kind, opt, drop, cin, bs, ",".join(t for t in (extra, "wgrad_spec=%d" % sp) if t), monkeypatch)
           for sp in (1, 0)]
    nconv = 3 if kind == "rpv_bench" else 2
    assert sorted(res[0][3]) == [str(i) for i in range(nconv)], res[0][3]
    assert all(v[0] > 0 for v in res[0][3].values()), res[0][3]      # a signature instance per conv layer
    assert all(v[0] == 0 for v in res[1][3].values()), res[1][3]     # wgrad_spec=0: generic kernels
    for layer, want in splits.items():
        assert res[0][3][layer][1:] == want and res[1][3][layer][1:] == want, (res[0][3], res[1][3])
    # same split geometry in both arms
    assert {k: v[1:] for k, v in res[0][3].items()} == {k: v[1:] for k, v in res[1][3].items()}
    # every slab and bias slab of the plan (the conv layers' and the dense layers')
    assert len(res[0][0]) == len(res[1][0]) >= 2 * nconv
    for a, b in zip(res[0][0], res[1][0]):
        assert a.shape == b.shape and torch.equal(a, b)
    assert torch.equal(res[0][1], res[1][1])
    assert res[0][2] == res[1][2]


def test_wgrad_sig_no_match_takes_generic(monkeypatch):
    """Conv sizes [8, 16, 32]: no signature matches, so both settings run the generic kernels."""
    res = [_run("rpv_small", "Adam", 0.0, 3, 4, "wgrad_spec=%d" % sp, monkeypatch) for sp in (1, 0)]
    assert len(res[0][3]) == 3 and all(v[0] == 0 for r in res for v in r[3].values()), (res[0][3], res[1][3])
    for a, b in zip(res[0][0], res[1][0]):
        assert torch.equal(a, b)
    assert torch.equal(res[0][1], res[1][1]) and res[0][2] == res[1][2]

"""The dual launches whose co-scheduled dgrad geometry is fixed at compile time too
(csrc/kernels/dual_halo_fix_body.h, dgrad signatures in wgrad_sig.h) against the same launches
without it (dgrad_spec=0: dual_halo_sig_kernel, whose dgrad half reads its geometry at run
time): whole training steps bit-identical -- every gradient buffer the dgrads write (the plan's
conv_dy), every partial slab, the master weights, the metrics -- and the launcher picks the fixed
kernel exactly where the dgrad args match a signature: the bench models at B >= 128 and default
tunes, and nowhere else.

Which kernel a dual launch takes is the launcher's host-side query K.dual_halo_dgrad_fixed (it
shares the launch's decline rules and field-by-field match) asked on the plan's args, not a
record of the launch; that the B=128 steps really run the fixed kernels is in the kernel traces
profiles/dgrad_sig_{rpv,mnist}_sequence_fix.txt."""
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
    {dual launch name: the launcher takes the fixed kernel})."""
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
    fixed = {}
    for it in plan.launches:
        if it[0].startswith("wgrad_dgrad_conv"):
            ca, ntc, wa, cfg = (it.args[r] for r in ("ca", "ntc", "wa", "cfg"))
            fixed[it[0]] = ex.K.dual_halo_dgrad_fixed(ca, ntc, wa, cfg[0], cfg[1])
    dys = [t.clone() for t in plan.conv_dy if t is not None]
    slabs = [t.clone() for pair in plan.wgrad_slabs for t in pair if t is not None]
    return dys, slabs, m.store.master[:m.store.numel].clone(), ex.read_metrics(), fixed


def _pair(kind, opt, drop, cin, bs, extra, monkeypatch):
    """The dgrad_spec=1 and dgrad_spec=0 arms of one case, after checking they computed the same."""
    res = [_run(kind, opt, drop, cin, bs, ",".join(t for t in (extra, "dgrad_spec=%d" % sp) if t), monkeypatch)
           for sp in (1, 0)]
    nconv = 3 if kind.startswith("rpv") else 2
    assert len(res[0][0]) == len(res[1][0]) == nconv          # a gradient buffer per conv stage
    assert len(res[0][1]) == len(res[1][1]) >= 2 * nconv
    for a, b in zip(res[0][0] + res[0][1], res[1][0] + res[1][1]):
        assert a.shape == b.shape and torch.equal(a, b)
    assert float(res[0][0][0].float().abs().sum()) > 0        # the first stage's gradient: a dgrad wrote it
    assert torch.equal(res[0][2], res[1][2])
    assert res[0][3] == res[1][3]
    assert sorted(res[0][4]) == sorted(res[1][4]) == ["wgrad_dgrad_conv%d" % i for i in range(1, nconv)]
    assert not any(res[1][4].values()), res[1][4]             # dgrad_spec=0: never the fixed kernel
    return res[0][4]


# (kind, optimizer, dropout, channels, batch)
FIXED = [
    ("rpv_bench", "Adam", 0.2, 3, 128),
    ("rpv_bench", "SGD", 0.0, 1, 128),
    ("mnist_bench", "Adam", 0.3, 1, 128),
    ("rpv_bench", "Adam", 0.2, 3, 256),      # the same R: the same instances at another grid
]


@pytest.mark.parametrize("kind,opt,drop,cin,bs", FIXED)
def test_dgrad_sig_bit_identical(kind, opt, drop, cin, bs, monkeypatch):
    fixed = _pair(kind, opt, drop, cin, bs, "", monkeypatch)
    assert all(fixed.values()), fixed                         # every dual of the step


# (kind, batch, extra tune): the dgrad args match no dgrad signature
DECLINES = [
    ("rpv_bench", 64, ""),                   # R 8: other blocks, other TM
    ("rpv_bench", 5, ""),                    # R 1, TM 1
    ("rpv_small", 128, ""),                  # conv sizes [8, 16, 32]: no signature at all
    ("rpv_bench", 128, "lds_layout=0"),      # the dgrad's halo pixel stride differs
]


@pytest.mark.parametrize("kind,bs,extra", DECLINES)
def test_dgrad_sig_declines(kind, bs, extra, monkeypatch):
    fixed = _pair(kind, "Adam", 0.2, 3, bs, extra, monkeypatch)
    assert not any(fixed.values()), fixed

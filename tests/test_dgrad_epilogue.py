"""The fixed dual launches' dgrad epilogue with the backward-through ReLU-mask operands fetched
ahead of the MFMAs (csrc/kernels/conv_halo_body.h epi_pre, bwd_through_fetch8 / finish8 in
bwd_through.h) against the same steps at dgrad_spec=0, whose dgrad half (dual_halo_sig_kernel,
run-time geometry) keeps the in-place load of bwd_through_store8: the change moves a load, so
two whole training steps must come out bit-identical -- every gradient buffer the dgrads write
(the plan's conv_dy), every partial slab, the master weights and the metrics.

Batches: 128 is the smallest the fixed instances take (B <= 64 gives R 8, which stays on
dual_halo_sig_kernel) and 256 the same instances at another grid; every case asserts through
K.dual_halo_dgrad_fixed that the default arm took the fixed kernels.  The cases pick the paths of
the new epilogue: dropout on / off (finish8 tests the threshold once per chunk: two code paths),
RPV conv2 (two passes of two chunks per lane) and conv3 (one pass), 1 input channel, and the MNIST
bench model, whose dgrad has three passes of one chunk per lane with a ragged last one (the
prefetch of a chunk past the block is clamped to the block's last pixel and its store skipped).
Which instances prefetch is the signatures' epi_pre switch (wgrad_sig.h; docs/ARCHITECTURE.md
§16: conv2's dual as shipped -- all three passed these cases with the switch on); the cases do
not depend on it.  One case kills whole 8-channel chunks of two stage outputs (zero kernel
columns, negative bias: the stage output is exactly zero whatever the data) and checks that the
dgrads store exact zeros (all sixteen bits) there and nowhere only zeros."""
import numpy as np
import pytest
import torch

from cori_intml_examples_amd.apps import zoo
from cori_intml_examples_amd.utils import set_random_seed

pytestmark = pytest.mark.gpu


def _build(kind, opt, drop, cin):
    if kind == "rpv":             # DistTrain_rpv: 64x64x{1,3}, conv[16,32,64] fc[128]
        return zoo.rpv_cnn((64, 64, cin), conv_sizes=[16, 32, 64], fc_sizes=[128], dropout=drop,
                           optimizer=opt, lr=1e-3, device="cuda")
    assert kind == "mnist"        # DistTrain_mnist: 28x28x1, conv 32-64, fc 128
    return zoo.mnist_cnn(32, 64, 128, dropout=drop, optimizer=opt, lr=1e-3, input_shape=(28, 28, 1), device="cuda")


def _data(model, n, seed):
    rs = np.random.RandomState(seed)
    x = torch.tensor(rs.rand(n, *model.input_shape[1:]).astype(np.float32)).to(torch.bfloat16).float().numpy()
    nout = model.output_shape[-1]
    y = (rs.rand(n) > 0.5).astype(np.float32) if nout == 1 else np.eye(nout, dtype=np.float32)[rs.randint(0, nout, n)]
    return x, y


def _kill(model, dead):
    """Zero the kernel columns and set the bias to -1 for the channels dead[i] of conv layer i:
    relu(conv + bias) is exactly zero there for every input, and stays so (no gradient)."""
    w = model.get_weights()
    for i, chans in dead.items():
        k, b = w[2 * i], w[2 * i + 1]
        assert k.ndim == 4 and b.ndim == 1 and k.shape[-1] == b.shape[0] > max(chans)
        k[..., chans] = 0.0
        b[chans] = -1.0
    model.set_weights(w)


def _run(kind, opt, drop, cin, bs, spec, monkeypatch, dead=None):
    """Two training steps at batch bs; returns (conv_dy buffers, slabs, master, metrics,
    {dual launch name: the launcher takes the fixed kernel})."""
    monkeypatch.setenv("INTML_TUNE", "dgrad_spec=%d" % spec)
    set_random_seed(67)
    m = _build(kind, opt, drop, cin)
    if dead:
        _kill(m, dead)
    x, y = _data(m, 2 * bs, seed=31)
    ex = m._executor
    d = ex.upload(x, y)
    perm = torch.randperm(d.n, generator=torch.Generator().manual_seed(37)).to(ex.device)
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


def _pair(kind, opt, drop, cin, bs, monkeypatch, dead=None):
    new, old = (_run(kind, opt, drop, cin, bs, sp, monkeypatch, dead) for sp in (1, 0))
    nconv = 3 if kind == "rpv" else 2
    duals = ["wgrad_dgrad_conv%d" % i for i in range(1, nconv)]
    assert sorted(new[4]) == sorted(old[4]) == duals
    assert all(new[4].values()), new[4]                       # default: every dual is a fixed instance
    assert not any(old[4].values()), old[4]                   # dgrad_spec=0: none is
    assert len(new[0]) == len(old[0]) == nconv
    assert len(new[1]) == len(old[1]) >= 2 * nconv
    for a, b in zip(new[0] + new[1], old[0] + old[1]):
        assert a.shape == b.shape and torch.equal(a, b)
    for t in new[0][:nconv - 1]:                              # the buffers the fixed dgrads wrote
        assert float(t.float().abs().sum()) > 0
    assert torch.equal(new[2], old[2])
    assert new[3] == old[3]
    return new[0]


# (model, optimizer, dropout, input channels, batch)
CASES = [
    ("rpv", "Adam", 0.2, 3, 128),
    ("rpv", "SGD", 0.0, 3, 128),         # finish8's no-dropout path
    ("rpv", "Adam", 0.2, 1, 128),
    ("mnist", "Adam", 0.3, 1, 128),      # three passes, the last one ragged: the clamped prefetch
    ("mnist", "SGD", 0.0, 1, 128),
    ("rpv", "SGD", 0.2, 3, 256),
    ("mnist", "Adam", 0.3, 1, 256),
]


@pytest.mark.parametrize("kind,opt,drop,cin,bs", CASES)
def test_dgrad_epilogue_bit_identical(kind, opt, drop, cin, bs, monkeypatch):
    _pair(kind, opt, drop, cin, bs, monkeypatch)


@pytest.mark.parametrize("drop", [0.0, 0.2])
def test_dgrad_epilogue_dead_chunks_store_exact_zeros(drop, monkeypatch):
    # conv1 (16 channels, two chunks): chunk 0 dead; conv2 (32 channels): chunk 1 dead.  The dual of
    # conv2 writes conv_dy[0] through conv1's mask, the dual of conv3 conv_dy[1] through conv2's.
    dead = {0: list(range(0, 8)), 1: list(range(8, 16))}
    dys = _pair("rpv", "Adam", drop, 3, 128, monkeypatch, dead)
    for i, chans in dead.items():
        t = dys[i]
        bits = t.view(torch.int16)
        assert not bool((bits[..., chans] != 0).any())         # +0.0 in every element, not -0.0
        live = [c for c in range(t.shape[-1]) if c not in chans]
        assert float(t[..., live].float().abs().sum()) > 0

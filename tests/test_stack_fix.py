"""The conv-stack forward with its whole geometry fixed at compile time (csrc/kernels/
conv_stack_fix_body.h, signature StackSigRpv2 in stack_sig.h: the RPV stack at two row bands)
against the launches it replaces: stack_fix=0 (the 16-wave kStackSigs instance, geometry read at
run time) and stack_spec=0 (the generic kernel).  Two training steps and one evaluation pass are
bit-identical in everything the stack writes -- every stage output (plan.conv_out), every
argmax-code buffer (plan.conv_code), srcidx -- and in what follows from it: the master weights and
the metrics.  The launcher takes the fixed kernel exactly where the plan's args equal the
signature: the RPV bench stack at two bands with default tunes, at any batch size, dropout rate,
channel count and optimizer -- and nowhere else.

The geometry is the signature's, so only the batch shrinks: B = 3 (odd; 6 workgroups, both bands;
stack_splits=2 because the automatic band count at B = 3 is four) and B = 128, the bench's.

Which kernel a launch takes is the launcher's own host-side decision, K.conv_stack_fixed, asked on
the plan's args; that the B = 128 step really runs conv_stack_fix_kernel is in the kernel trace
profiles/stack_fix_rpv_sequence_fix.txt."""
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
    if kind == "rpv_small":       # same grids, conv sizes the signature does not have
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


def _stack_bufs(plan):
    out = [t.clone() for t in plan.conv_out if t is not None]
    code = [t.clone() for t in plan.conv_code if t is not None]
    # (the dataset rows the band-0 workgroups record: every prologue-free plan has them)
    src = plan.srcidx.clone() if plan.srcidx is not None else torch.zeros(0, dtype=torch.int32)
    assert plan.srcidx is not None or not plan.pro_free
    return out, code, src


def _run(kind, opt, drop, cin, bs, tunes, monkeypatch):
    """Two training steps and one evaluation pass at batch bs.  Returns (tensors, scalars, fixed):
    everything the stack wrote in either pass plus the master weights; both passes' metrics; the
    launcher's decision for the training and the evaluation launch."""
    monkeypatch.setenv("INTML_TUNE", tunes)
    set_random_seed(71)
    m = _build(kind, opt, drop, cin)
    x, y = _data(m, 2 * bs, seed=31)
    ex = m._executor
    d = ex.upload(x, y)
    perm = torch.randperm(d.n, generator=torch.Generator().manual_seed(37)).to(ex.device)
    tensors, scalars, fixed = [], [], []
    for mode in ("train", "eval"):
        ex.reset_metrics()
        if mode == "train":
            ex.train_steps(d, perm, 0, bs, 2)
        else:
            ex.eval_step(d, 0, bs)
        torch.cuda.synchronize()
        plan = next(p for k, p in ex._plans.items() if k[0] == bs and k[1] == mode)
        stack = [it.args["stack"] for it in plan.launches if it[0] == "conv_stack_fwd"]
        assert len(stack) == 1
        fixed.append(bool(ex.K.conv_stack_fixed(stack[0])))
        out, code, src = _stack_bufs(plan)
        assert len(out) == len(code) + (kind == "mnist_bench") == len(ex.convs)   # MNIST's first conv is unpooled
        assert float(out[-1].float().abs().sum()) > 0
        tensors += out + code + [src]
        scalars.append(ex.read_metrics())
    tensors.append(m.store.master[:m.store.numel].clone())
    return tensors, scalars, fixed


def _same(a, b):
    assert len(a[0]) == len(b[0])
    for s, t in zip(a[0], b[0]):
        assert s.shape == t.shape and s.dtype == t.dtype and torch.equal(s, t)
    assert a[1] == b[1]


# (batch, extra tune, dropout, channels, optimizer): both batches see both values of each variation
FIXED = [
    (3, "stack_splits=2", 0.2, 3, "Adam"),
    (3, "stack_splits=2", 0.0, 1, "SGD"),
    (3, "stack_splits=2", 0.2, 1, "SGD"),
    (128, "", 0.2, 3, "Adam"),
    (128, "", 0.0, 1, "SGD"),
    (128, "", 0.0, 3, "Adam"),
]


@pytest.mark.parametrize("bs,extra,drop,cin,opt", FIXED)
def test_stack_fix_bit_identical(bs, extra, drop, cin, opt, monkeypatch):
    arms = [_run("rpv_bench", opt, drop, cin, bs, ",".join(t for t in (extra, arm) if t), monkeypatch)
            for arm in ("stack_fix=1", "stack_fix=0", "stack_spec=0")]
    assert arms[0][2] == [True, True], arms[0][2]              # training and evaluation launches
    assert arms[1][2] == [False, False] and arms[2][2] == [False, False], (arms[1][2], arms[2][2])
    _same(arms[0], arms[1])
    _same(arms[0], arms[2])


# (kind, batch, extra tune): the args differ from the signature somewhere
DECLINES = [
    ("rpv_bench", 64, ""),                   # four bands
    ("rpv_bench", 256, ""),                  # one band
    ("rpv_small", 128, ""),                  # conv sizes [8, 16, 32]
    ("rpv_bench", 128, "lds_layout=0"),      # dense halo images: other xpix / xrow and offsets
    ("rpv_bench", 128, "stack_k16=0"),       # the k16 tail is compiled in
    ("rpv_bench", 128, "wt=0"),              # so are the write-through stores
    ("rpv_bench", 128, "stack_dbg=128"),     # a diagnostics launch: the generic kernel
    ("mnist_bench", 128, ""),
]


@pytest.mark.parametrize("kind,bs,extra", DECLINES)
def test_stack_fix_declines(kind, bs, extra, monkeypatch):
    arms = [_run(kind, "Adam", 0.2, 3 if kind != "mnist_bench" else 1, bs,
                 ",".join(t for t in (extra, arm) if t), monkeypatch) for arm in ("stack_fix=1", "stack_fix=0")]
    assert arms[0][2] == [False, False] and arms[1][2] == [False, False], (arms[0][2], arms[1][2])
    _same(arms[0], arms[1])

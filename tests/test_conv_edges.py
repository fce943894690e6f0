"""The conv and dense kernels of a captured step against the float64 oracle
(tests/helpers/conv_oracle.py), ELEMENT BY ELEMENT, at the tail batches fit() runs on plans of
their own: every stage output, max-pool argmax code, routed gradient (conv dgrad, dense dX into a
dense or a pooled conv source), weight and bias gradient and padding channel, each from the
saved bf16 / fp32 inputs of the kernel that wrote it, within bounds DERIVED in the oracle's
docstring (never measured).  tests/test_conv_oracle.py proves the checker on the CPU first.

The rig uploads 3 bs + 5 samples and runs ONE training step with a random permutation at
pos = 5, so a kernel that ignored the gather index or the device cursor reads the wrong images;
SGD and opt_nograd=0 keep every gradient stored.  Cases (helpers/conv_oracle.py TRAIN, FORCED,
EVAL): five model kinds at bs = 1, 3, 17, 33, 65 on 8x8 images (last stages 2x2 -> 1x1 pooled; the
tile-bound wide kinds at 16x16), RPV at 16x16 with bs 1 / 127, the benchmarked RPV geometry
(64x64x3: the compile-time signature instances) at bs 1 / 5, the kernel forms small shapes never
pick (per-layer forward convs, standalone dgrad / wgrad, the big wide-conv blocks, 1 and 4 conv
stack row bands), and the eval / predict plans (no dropout, another head fusion, the head's
probabilities) at a non-zero position.

Each case prints the worst error / bound per quantity.  No shape of the matrix is rejected at plan
build, and none gave a wrong element.

Largest error / bound over the whole matrix on an MI355X (U = 2**-23), with the CPU stand-in of
tests/test_conv_oracle.py (fp32 reference, bf16 storage) in brackets.  For the bf16-stored
quantities the second figure is what the error needs of the ACCUMULATION bound alone once the
2**-8 |ref| rounding term is taken off -- the figure a later tightening of U to 2**-24 would be
judged by; bf16 round-to-nearest itself reaches 2**-8 relative just above a power of two, so the
first figure sits near 1 by construction.

    conv stage outputs        0.993, 2.4e-4   [0.993, 1.5e-4]
    dense stage outputs       0.970, 0        [0.987, 0]
    conv dgrad -> conv dP     0.992, 6.8e-5   [0.989, 4.8e-4]
    dense dX -> conv dP       0.991, 0        [0.991, 0]
    dense dX -> dense dH      0.968, 0        [0.987, 0]
    conv weight gradient      0.056           [0.070]
    conv bias gradient        1.3e-4          [8.9e-5]
    dense weight gradient     0.082           [0.080]
    dense bias gradient       0               [0]      (sums of bf16 values fp32 holds exactly)
    probabilities (predict)   0.016           [0.0071]
    argmax codes              no mismatch off the near ties, every all-zero window 0; near-tie
                              share at most 0.39 % [0.78 %] against the 2 % cap
    padding channels          all zero
"""
import numpy as np
import pytest
import torch

from cori_intml_examples_amd.utils import set_random_seed

from helpers import conv_oracle as O
from test_hip_kernels import _step
from test_hip_model import _build

pytestmark = pytest.mark.gpu

POS = 5


def _f(t):
    return None if t is None else t.detach().float().cpu()


def _record(m, ex, bp, w_before, training, probs=None):
    """What the plan's last step read and wrote (O.StepRecord)."""
    slabs = {d.dst_off: d.S for grp in bp.red_groups for d in grp.descs}
    x = _f(bp.step_inputs()[0]).view(bp.bs, ex.in_H, ex.in_W, ex.in_Cs)[..., :ex.in_C]
    return O.StepRecord(
        x=x, step=int(ex._st_i32[0].item()), probs=probs,
        conv_out=[_f(t) for t in bp.conv_out], conv_code=[None if t is None else t.cpu() for t in bp.conv_code],
        conv_dy=[_f(t) for t in bp.conv_dy], dense_out=[_f(t) for t in bp.dense_out],
        dense_dh=[_f(t) for t in bp.dense_dh], dense_splits=[s for s, _ in bp.dense_splits],
        w=O.weight_reader(m, w_before),
        g=lambda layer, short: m.store.view(layer, short, grad=True).detach().cpu(),
        slabs=lambda layer, short: slabs.get(m.store.spec(layer, short).offset, 1))


def _train_case(kind, hw, bs, monkeypatch, tune_s="", present=(), absent=()):
    monkeypatch.setenv("INTML_TUNE", ",".join(s for s in ("opt_nograd=0", tune_s) if s))
    cin, drop = O.KINDS[kind]
    perm = np.random.RandomState(1000 + bs).permutation(3 * bs + 5)
    m, ex, bp, wb = _step(kind, drop, cin, hw, bs, perm=perm, pos=POS, data=lambda mm, n: O.inputs(mm, n, seed=4))
    names = [it.name for it in bp.launches]
    tag = "%s hw=%d bs=%d %s" % (kind, hw, bs, tune_s)
    print(tag, "launches:", " ".join(names))
    assert set(present) <= set(names) and not set(absent) & set(names), names
    # the rows actually trained are perm[5:5 + bs]
    rows = torch.as_tensor(perm[POS:POS + bs]).long().to(ex.device)
    data = ex._bound_ref
    xs, ys = bp.step_inputs()
    assert torch.equal(xs, data.x[rows]) and torch.equal(ys, data.y[rows]), "the step gathered other rows"
    if bp.srcidx is not None:
        assert torch.equal(bp.srcidx.long(), rows)
    d = O.describe(m)
    rec = _record(m, ex, bp, wb, True)
    res, shares = O.check_forward(d, rec, True)
    res += O.check_backward(d, rec)
    fails = O.report(tag, res, shares)
    assert not fails, fails
    # nothing above was vacuous: every stage stored something, every layer got a gradient
    assert all(float(t.abs().max()) > 0 for t in rec.conv_out + rec.conv_dy + rec.dense_out + rec.dense_dh)
    for layer in [cs.conv for cs in d.plan.convs] + [ds.dense for ds in d.plan.denses]:
        assert float(rec.g(layer, "kernel").abs().max()) > 0 and float(rec.g(layer, "bias").abs().max()) > 0
    return bp


@pytest.mark.parametrize("kind,hw,bs", O.TRAIN)
def test_train_step_tails(kind, hw, bs, monkeypatch):
    _train_case(kind, hw, bs, monkeypatch)


@pytest.mark.parametrize("kind,hw,bs,tune_s,present,absent", O.FORCED,
                         ids=["%s-%d-%d-%s" % c[:4] for c in O.FORCED])
def test_forced_kernel_forms(kind, hw, bs, tune_s, present, absent, monkeypatch):
    bp = _train_case(kind, hw, bs, monkeypatch, tune_s, present, absent)
    key, _, val = tune_s.partition("=")
    if key == "stack_splits":
        assert bp.stack_splits == int(val)
    if key == "conv_big_min":
        ca = dict((it.name, it) for it in bp.launches)["conv_fwd2"].args["ca"]
        assert bp.ex.K.conv_tile_big_blocks(ca, 8) >= 1


@pytest.mark.parametrize("kind,hw,bs", O.EVAL)
def test_eval_and_predict_plans(kind, hw, bs, monkeypatch):
    """Stage outputs and codes without dropout, dense_out, and the head's probabilities, at
    rows [7, 7 + bs) of a larger data set."""
    monkeypatch.setenv("INTML_TUNE", "")
    cin, drop = O.KINDS[kind]
    set_random_seed(99)
    m = _build(kind, "cuda", opt="SGD", drop=drop, cin=cin, hw=hw)
    ex = m._executor
    pos = 7
    x, y = O.inputs(m, 2 * bs + pos, seed=6)
    data = ex.upload(x, y)
    wb = m.store.master.clone()
    d = O.describe(m)
    ex.reset_metrics()
    ex.eval_step(data, pos, bs)
    torch.cuda.synchronize()
    fails = []
    for mode in ("eval", "predict"):
        probs = None
        if mode == "predict":
            probs = ex.predict_step(data, pos, bs).float().cpu()
            torch.cuda.synchronize()
        bp = ex._plans[(bs, mode)]
        assert torch.equal(bp.step_inputs()[0], data.x[pos:pos + bs]), "the step read other rows"
        res, shares = O.check_forward(d, _record(m, ex, bp, wb, False, probs), False)
        assert ("probs" in {r.name for r in res}) == (mode == "predict")
        fails += O.report("%s hw=%d bs=%d %s" % (kind, hw, bs, mode), res, shares)
    assert torch.equal(m.store.master, wb)
    assert not fails, fails

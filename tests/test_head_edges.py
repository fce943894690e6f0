"""The output head kernel (csrc/kernels/head.hip) against the float64 oracle
(tests/helpers/head_oracle.py) on CRAFTED logits: saturated and in-range rows, smoothed
targets, ties, overflow, every class count path (N = 1, 2, 3, 10, 16; 17 is rejected), head
weights in LDS and in global memory, the fused (one row per workgroup) and unfused (four rows,
ragged last workgroup) instances, the Keras-to-padded index map, the gradient routed into a
dense layer or a pooled conv, the eval and predict plans, one weighted instance -- and the
three fused split-K epilogue forms at their split-count borders.

How the logits are steered (no conv-free model needed): the model trains with SGD at learning
rate 0, so no weight moves.  One step gives the head's input ``a`` (read back from the plan);
``W = lstsq(a, Z* - b)`` in float64 puts the logit table Z* into the head weights; the step
is run again and ``a`` must be bit-identical.  The oracle is evaluated on the logits the kernel
actually saw, ``a.double() @ W.double() + b.double()``, never on Z* itself.

Bounds.  For dz (seen through gb), gw, gb, probs and the softmax / mse loss, each case
computes what the project's own float32 CPU reference (ops/reference.py in float32, logits by
a float32 matmul) differs from the oracle by ON THE SAME INPUTS; the kernel gets 8x that,
floored at 8 * 2**-24 * the quantity's largest magnitude (reduction order: K split over 64
lanes plus a shuffle tree against sequential; device expf / logf at up to 2 ulp against libm's
1).  The sigmoid loss, which float32 cannot reproduce tightly near saturation, gets the oracle's
derived per-row bound plus 8x the float32 reference's logit error (|dL/dz| <= 1).  The routed
gradient is stored in bf16: one bf16 ulp (2**-8 relative) plus the dz bound through |W|.
Every case prints kernel error / float32-reference error / bound per quantity.
"""
import numpy as np
import pytest
import torch

from cori_intml_examples_amd import Conv2D, Dense, Flatten, Input, MaxPooling2D, Model
from cori_intml_examples_amd.ops import reference as R
from cori_intml_examples_amd.optim import SGD
from cori_intml_examples_amd.utils import set_random_seed

from helpers import head_oracle as O
from test_sample_weight_gpu import make_weights

pytestmark = pytest.mark.gpu

LOSS = {"sigmoid": "binary_crossentropy", "softmax": "categorical_crossentropy", None: "mse"}
ORACLE = {"sigmoid": O.sigmoid_bce, "softmax": O.softmax_cce, None: O.mse}
U = 2.0 ** -24


def _cdiv(a, b):
    return -(-a // b)


def _build(arch, n_out, act, H=32, conv=8, hw=8):
    """fused / dense: conv -> pool -> flatten -> Dense(H, relu) -> head; flat: conv -> pool ->
    flatten -> head; split: conv (unpooled) -> flatten -> Dense(32, relu) -> head."""
    inp = Input(shape=(hw, hw, 1))
    h = Conv2D(conv, (3, 3), activation="relu", padding="same")(inp)
    if arch != "split":
        h = MaxPooling2D((2, 2))(h)
    h = Flatten()(h)
    if arch != "flat":
        h = Dense(H, activation="relu")(h)
    out = Dense(n_out, activation=act)(h)
    m = Model(inp, out, device="cuda")
    m.compile(optimizer=SGD(lr=0.0), loss=LOSS[act], metrics=["accuracy"])
    return m


def _inputs(m, n, seed=0):
    x = np.random.RandomState(seed).randn(n, *m.input_shape[1:]).astype(np.float32)
    return torch.tensor(x).to(torch.bfloat16).float().numpy()


class Rig:
    """One model + one input batch; runs the train / eval / predict plans and reads back what
    the head kernel read and wrote."""

    def __init__(self, m, x):
        self.m, self.ex, self.x, self.M = m, m._executor, x, x.shape[0]
        self.hd = self.ex.plan.head
        self.w0 = [w.copy() for w in m.get_weights()]

    def set_head(self, W, b):
        w = [v.copy() for v in self.w0]
        w[-2], w[-1] = np.asarray(W, np.float32).reshape(w[-2].shape), np.asarray(b, np.float32).reshape(w[-1].shape)
        self.m.set_weights(w)
        self.W, self.b = w[-2], w[-1]

    def _prev(self, bp):
        """The previous stage's saved output (padded, bf16) and the head's input in Keras order."""
        ex, src = self.ex, self.ex.head_src
        if src.kind == "conv":
            t = bp.conv_out[src.idx]
            a = t.float().cpu()[..., :ex.convs[src.idx].Cout].reshape(bp.bs, -1)
        else:
            t = bp.dense_out[src.idx]
            a = t.float().cpu()[:, :ex.denses[src.idx].N]
        return t.clone(), a.double().numpy()

    def _flag(self):
        o = self.ex.K.STEP_STATE_METRICS_OFFSET // 8
        return int(self.ex._st_i64[o:o + 4 * self.ex.K.STEP_STATE_METRIC_SLOTS].view(-1, 4)[:, 3].sum().item())

    def train(self, y, w=None):
        ex, m = self.ex, self.m
        d = ex.upload(self.x, y, w)
        ex.reset_metrics()
        ex.train_step(d, torch.arange(d.n, device=ex.device), 0, d.n)
        torch.cuda.synchronize()
        bp = ex._plans[(self.M, "train", "w") if w is not None else (self.M, "train")]
        prev, a = self._prev(bp)
        src = ex.head_src
        if src.kind == "conv":
            dp = bp.conv_dy[src.idx].float().cpu()
            C = ex.convs[src.idx].Cout
        else:
            dp = bp.dense_dh[src.idx].float().cpu()
            C = ex.denses[src.idx].N
        loss, acc, n = ex.read_metrics()
        for v0, v1 in zip(self.m.get_weights()[-2:], (self.W, self.b)):
            np.testing.assert_array_equal(v0, v1)        # learning rate 0: nothing moved
        return dict(bp=bp, prev=prev, a=a, loss=loss, acc=acc, n=n, flag=self._flag(),
                    gw=m.store.view(self.hd.dense, "kernel", grad=True).cpu().double().numpy(),
                    gb=m.store.view(self.hd.dense, "bias", grad=True).cpu().double().numpy(),
                    dprev=dp[..., :C].reshape(self.M, -1).double().numpy(),
                    dpad=float(dp[..., C:].abs().max()) if dp.shape[-1] > C else 0.0)

    def evaluate(self, y):
        ex = self.ex
        d = ex.upload(self.x, y)
        ex.reset_metrics()
        ex.eval_step(d, 0, d.n)
        torch.cuda.synchronize()
        bp = ex._plans[(self.M, "eval")]
        loss, acc, n = ex.read_metrics()
        return dict(bp=bp, a=self._prev(bp)[1], loss=loss, acc=acc, n=n, flag=self._flag())

    def predict(self):
        ex = self.ex
        d = ex.upload(self.x, None)
        p = ex.predict_step(d, 0, d.n).double().cpu().numpy()
        return dict(bp=ex._plans[(self.M, "predict")], a=self._prev(ex._plans[(self.M, "predict")])[1], probs=p)


def _oracle(a, W, b, y, act, wts=None):
    M = a.shape[0]
    z = a @ np.asarray(W, np.float64) + np.asarray(b, np.float64)
    loss, dz, cor, p = ORACLE[act](z, y)
    if wts is not None:
        f = O.weight_factor(wts)
        loss, dz = loss * f, dz * f[:, None]
    return dict(z=z, loss=loss.mean(), acc=cor.mean(), dz=dz, gw=a.T @ dz / M, gb=dz.sum(0) / M,
                dh=(dz / M) @ np.asarray(W, np.float64).T, probs=p, rows=loss)


def _ref32(a, W, b, y, act, wts=None):
    """The project's float32 CPU reference on the same inputs (logits by a float32 matmul)."""
    M = a.shape[0]
    a32, W32, y32 = torch.tensor(a, dtype=torch.float32), torch.tensor(np.asarray(W, np.float32)), torch.tensor(y)
    z = a32 @ W32 + torch.tensor(np.asarray(b, np.float32))
    if act == "sigmoid":
        loss, dz, _ = R.sigmoid_bce(z.reshape(-1), y32.reshape(-1))
        dz, p = dz.reshape(-1, 1), torch.sigmoid(z)
    elif act == "softmax":
        loss, dz, _ = R.softmax_cce(z, y32)
        p = torch.softmax(z, -1)
    else:
        loss, dz, _ = R.mse(z, y32)
        p = z
    if wts is not None:
        loss, dz = R.apply_weights(loss, dz, torch.tensor(wts))
    dz = dz / M
    d = lambda t: t.double().numpy()
    return dict(z=d(z), loss=float(loss.double().mean()), dz=d(dz) * M, gw=d(a32.t() @ dz), gb=d(dz.sum(0)), probs=d(p))


def _bound(ref, orc):
    return max(8.0 * float(np.abs(ref - orc).max()), 8.0 * U * float(np.abs(orc).max()))


def _report(tag, name, got, ref, orc, bound=None):
    ek, er = float(np.abs(got - orc).max()), float(np.abs(ref - orc).max())
    bound = _bound(ref, orc) if bound is None else bound
    print("%-34s %-5s kernel err %.3g  fp32-ref err %.3g  bound %.3g" % (tag, name, ek, er, bound))
    return ek <= bound, "%s %s: kernel err %.3g > bound %.3g (fp32 ref err %.3g)" % (tag, name, ek, bound, er)


def _loss_bound(o, r, z_or_y, act, wts):
    if act != "sigmoid":
        return None
    # the oracle's per-row bound (p rounded in float32, pushed through log(pc / (1 - pc))), plus
    # the logit error itself: |dL/dz| <= 1, so a logit error moves a row's loss by at most itself
    z, y = z_or_y
    f = O.weight_factor(wts) if wts is not None else 1.0
    rows = O.sigmoid_loss_bound(z, y) * f
    return float(rows.mean() + 8.0 * (np.abs(r["z"] - o["z"]).reshape(-1) * f).mean())


def _check_metrics(tag, got, o, r, y, act, M, wts=None):
    assert got["n"] == M and got["flag"] == 0 and np.isfinite(got["loss"])
    assert abs(got["acc"] - o["acc"]) < 1e-9, (tag, got["acc"], o["acc"])
    ok, msg = _report(tag, "loss", np.float64(got["loss"]), np.float64(r["loss"]), np.float64(o["loss"]),
                      _loss_bound(o, r, (o["z"], y), act, wts))
    assert ok, msg


def _check_train(tag, rig, t, y, act, wts=None, expect_zero=False):
    M = rig.M
    o, r = _oracle(t["a"], rig.W, rig.b, y, act, wts), _ref32(t["a"], rig.W, rig.b, y, act, wts)
    if act is not None:
        O.regime_of(o["z"], act)                   # fails if a row lies within 2 of the clip threshold
    _check_metrics(tag, t, o, r, y, act, M, wts)
    fails = []
    for name in ("gw", "gb"):
        ok, msg = _report(tag, name, t[name].reshape(o[name].shape), r[name], o[name])
        if not ok:
            fails.append(msg)
    # gradient routed into the previous stage: (dz / M) W^T through its ReLU mask (and, for a
    # pooled conv, at pooled resolution), stored in bf16
    dzb = _bound(r["dz"], o["dz"])
    mask = t["a"] > 0
    ref = o["dh"] * mask
    tol = 2.0 ** -8 * np.abs(ref) + (np.abs(np.asarray(rig.W, np.float64)).sum(1) * dzb / M)[None, :] * mask
    err = np.abs(t["dprev"] - ref)
    print("%-34s dprev kernel err %.3g  (max |ref| %.3g, dz bound %.3g)" % (tag, err.max(), np.abs(ref).max(), dzb))
    if not (err <= tol).all():
        fails.append("%s dprev: %d elements off, worst %.3g" % (tag, int((err > tol).sum()), float((err - tol).max())))
    assert t["dpad"] == 0.0
    assert not fails, fails
    if expect_zero:
        assert (o["dz"] == 0).all()
        assert (t["gw"] == 0).all() and (t["gb"] == 0).all() and (t["dprev"] == 0).all()
    return o


def _tables(regime, M, N, act):
    return O.sigmoid_table(regime, M) if act == "sigmoid" else O.softmax_table(regime, M, N)


def _ties(M, N, act):
    """W = 0 with equal biases: every logit of a row is the same.  Softmax predicts class 0
    (first maximum); targets: class 0, another class, two equal maxima (first one counts).
    Sigmoid: p = 0.5 exactly rounds to 0, correct only for y = 0."""
    if act == "sigmoid":
        return np.zeros(1), (np.arange(M) % 2).astype(np.float32).reshape(M, 1), M - M // 2
    y = np.zeros((M, N), np.float32)
    want = 0
    for r in range(M):
        k = (0, 0, 1, 2, 3)[r % 5]       # (uneven on purpose: a last-maximum argmax scores differently)
        if k == 0:
            y[r, 0] = 1
        elif k == 1:
            y[r, N - 1] = 1
        elif k == 2:
            y[r, 0] = y[r, 1] = 0.5
        else:
            y[r, N - 2] = y[r, N - 1] = 0.5
        want += int(np.argmax(y[r]) == 0)
    return np.full(N, 0.3), y, want


def _run_head_case(tag, m, M, act, fused, conv_src=False):
    N = m.output_shape[-1]
    rig = Rig(m, _inputs(m, M))
    rs = np.random.RandomState(11)
    b = (0.5 * rs.randn(N)).astype(np.float32)
    # first run: the head's input, with the initial head weights
    rig.set_head(rig.w0[-2], b)
    y0 = _tables("mixed", M, N, act)[1] if act else rs.rand(M, N).astype(np.float32)
    t0 = rig.train(y0)
    bp = t0["bp"]
    names = [it[0] for it in bp.launches]
    last = len(rig.ex.denses) - 1
    if fused:
        assert "dense_epi%d" % last not in names and bp.head_blocks == M
    else:
        assert bp.head_blocks == _cdiv(M, 4) and (conv_src or "dense_epi%d" % last in names)
    a = t0["a"]
    assert np.linalg.matrix_rank(a) == min(a.shape), "head input is rank deficient"

    def craft(Zs):
        return np.linalg.lstsq(a, Zs - b.astype(np.float64), rcond=None)[0].astype(np.float32)

    def train(y, wts=None):
        t = rig.train(y, wts)
        assert torch.equal(t["prev"], t0["prev"]), "head input changed between runs"
        return t

    if act is None:
        Zs, y = 3.0 * rs.randn(M, N), rs.rand(M, N).astype(np.float32)
        rig.set_head(craft(Zs), b)
        o = _check_train(tag + " mse", rig, train(y), y, act)
        assert np.abs(o["z"] - Zs).max() < 1e-2
        e = rig.evaluate(y)
        _check_metrics(tag + " mse eval", e, _oracle(e["a"], rig.W, rig.b, y, act), _ref32(e["a"], rig.W, rig.b, y, act), y, act, M)
        p = rig.predict()
        op, rp = _oracle(p["a"], rig.W, rig.b, y, act), _ref32(p["a"], rig.W, rig.b, y, act)
        ok, msg = _report(tag + " mse predict", "probs", p["probs"], rp["probs"], op["probs"])
        assert ok, msg
        return
    for regime in ("clip", "in", "mixed"):
        Zs, y = _tables(regime, M, N, act)
        rig.set_head(craft(Zs), b)
        if regime == "in":
            Z_in, y_in = Zs, y
        t = train(y)
        o = _check_train("%s %s" % (tag, regime), rig, t, y, act, expect_zero=regime == "clip")
        assert np.abs(o["z"] - Zs).max() < 1e-2, "crafted logits missed their table"
        e = rig.evaluate(y)
        oe, re_ = _oracle(e["a"], rig.W, rig.b, y, act), _ref32(e["a"], rig.W, rig.b, y, act)
        _check_metrics("%s %s eval" % (tag, regime), e, oe, re_, y, act, M)
        p = rig.predict()
        op, rp = _oracle(p["a"], rig.W, rig.b, y, act), _ref32(p["a"], rig.W, rig.b, y, act)
        ok, msg = _report("%s %s predict" % (tag, regime), "probs", p["probs"], rp["probs"], op["probs"])
        assert ok and p["probs"].shape == (M, N), msg
        if regime == "mixed":
            # the weighted instance on the same batch (weights with zeros)
            wts = make_weights(M, seed=M)
            tw = train(y, wts)
            assert (M, "train", "w") in rig.ex._plans and tw["bp"].weighted
            _check_train("%s mixed weighted" % tag, rig, tw, y, act, wts=wts)
    # ties: exactly equal logits
    bt, yt, want = _ties(M, N, act)
    rig.set_head(np.zeros_like(rig.w0[-2]), bt)
    t = train(yt)
    assert t["acc"] * M == want, (t["acc"] * M, want)
    _check_train(tag + " ties", rig, t, yt, act)
    e = rig.evaluate(yt)
    assert e["acc"] * M == want and e["n"] == M
    # overflow: the in-range table scaled until |z| reaches 1e4 -- everything saturates, nothing
    # may turn into inf / NaN
    rig.set_head(craft(Z_in * (1e4 / np.abs(Z_in).max())), b)
    t = train(y_in)
    o = _check_train(tag + " overflow", rig, t, y_in, act, expect_zero=True)
    assert np.abs(o["z"]).max() > 5e3 and np.isfinite(t["gw"]).all()
    e = rig.evaluate(y_in)
    assert e["flag"] == 0 and np.isfinite(e["loss"]) and abs(e["acc"] - o["acc"]) < 1e-9
    p = rig.predict()
    assert np.isfinite(p["probs"]).all()
    assert np.abs(p["probs"] - _oracle(p["a"], rig.W, rig.b, y_in, act)["probs"]).max() <= 8 * U


FUSED = [(32, 1, "sigmoid", ""), (32, 1, "sigmoid", "head_generic=1"), (32, 2, "softmax", ""),
         (32, 10, "softmax", ""), (128, 16, "softmax", ""), (136, 16, "softmax", ""), (256, 10, "softmax", ""),
         (32, 3, None, ""), (32, 16, None, "")]


@pytest.mark.parametrize("H,N,act,tune_s", FUSED)
def test_fused_head(H, N, act, tune_s, monkeypatch):
    """Head after a hidden dense layer: one row per workgroup, the dense epilogue inside the
    head launch.  K*N = 2048 is the last size whose weights are staged in LDS; 2176 and 2560
    read them from global memory."""
    monkeypatch.setenv("INTML_TUNE", tune_s)
    set_random_seed(61)
    m = _build("fused", N, act, H=H)
    assert bool(m._executor.K.head_epi_max() >= H)
    _run_head_case("fused H=%d N=%d %s %s" % (H, N, act, tune_s), m, 26, act, fused=True)


def test_head_wider_than_16_is_rejected():
    set_random_seed(61)
    with pytest.raises(NotImplementedError):
        _build("fused", 17, "softmax")._executor


@pytest.mark.parametrize("M", [26, 1])
def test_unfused_head_after_wide_dense(M):
    """Hidden width 1032 > HEAD_EPI_MAX: dense_epi is launched, the head runs four rows per
    workgroup reading its input and its 2064 weights from global memory.  M = 26: six full
    workgroups and one of two rows."""
    set_random_seed(62)
    m = _build("dense", 2, "softmax", H=1032)
    _run_head_case("dense H=1032 N=2 M=%d" % M, m, M, "softmax", fused=False)


FLAT = [(8, 8, 1, "sigmoid"), (8, 8, 3, "softmax"), (8, 8, 16, "softmax"), (8, 8, 3, None), (5, 8, 3, "softmax"),
        (8, 16, 16, "softmax")]


@pytest.mark.parametrize("M", [1, 5, 26])
@pytest.mark.parametrize("conv,hw,N,act", FLAT)
def test_unfused_head_on_flattened_conv(conv, hw, N, act, M):
    """Head straight on a pooled conv: four rows per workgroup, no weights (a ragged last
    workgroup at M = 1, 5, 26), the gradient routed into the conv's pooled dP.  Conv2D(5) pads
    its channels to 8 (the Keras-to-padded index map, K = 80); the 16x16 input gives K*N = 8192
    (global weights)."""
    set_random_seed(63)
    m = _build("flat", N, act, conv=conv, hw=hw)
    src = m._executor.head_src
    assert src.kind == "conv" and (src.C, src.Cs) == (conv, 8)
    _run_head_case("flat C=%d hw=%d N=%d %s M=%d" % (conv, hw, N, act, M), m, M, act, fused=False, conv_src=True)


# ----------------------------------------------------------------------------- split-K epilogue forms
def _split_run(monkeypatch, extra, conv, hw, N, want, M=8):
    monkeypatch.setenv("INTML_TUNE", "")
    set_random_seed(64)
    m = _build("split", N, "sigmoid" if N == 1 else "softmax", conv=conv, hw=hw)
    ex = m._executor
    g = ex.denses[-1]
    assert not ex.K.dense_big(g.NT, g.KS)
    # (the plan reads the tuning values when it is built, at the first step)
    monkeypatch.setenv("INTML_TUNE", "dense_waves=%d,%s" % (want * ex.K.dense_groups(M, g.NT, g.KS), extra))
    x = _inputs(m, M, seed=3)
    y = (np.arange(M) % 2).astype(np.float32) if N == 1 else np.eye(N, dtype=np.float32)[np.arange(M) % N]
    d = ex.upload(x, y)
    ex.reset_metrics()
    ex.train_step(d, torch.arange(M, device=ex.device), 0, M)
    torch.cuda.synchronize()
    bp = ex._plans[(M, "train")]
    assert bp.dense_splits[-1][0] == want, bp.dense_splits
    return m, bp, [it[0] for it in bp.launches], ex.read_metrics()


def _bf16_ulp(v):
    return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -126))) - 7)


# (conv channels, input, splits, head_generic): 16x16x16 flattens to KS = 128 k-steps, whose
# possible split counts are ceil(128 / k): 26 and 32 (first form; second with head_generic=1),
# 43 and 64 (second), 128 (third).  No odd count above 64 exists for KS = 128, so a 10x10x24
# source (KS = 75) adds 25, 38 and 75.
SPLITS = [(16, 16, 26, 0), (16, 16, 26, 1), (16, 16, 32, 0), (16, 16, 43, 0), (16, 16, 64, 0), (16, 16, 128, 0),
          (24, 10, 25, 0), (24, 10, 25, 1), (24, 10, 38, 0), (24, 10, 75, 0)]


@pytest.mark.parametrize("N", [1, 10])
@pytest.mark.parametrize("conv,hw,want,generic", SPLITS)
def test_fused_epilogue_forms_bit_identical(conv, hw, want, generic, N, monkeypatch):
    """The head's three fused split-K epilogue forms (<= 32 splits: one batch of loads; <= 64:
    the four split groups in parallel, also what head_generic=1 takes for <= 32; > 64:
    dense_epi_value) give dense_epilogue_kernel's activations bit for bit, at split counts that
    are and are not multiples of 4 / 8, and both are the float64 sum of the partials + bias
    through ReLU to one bf16 ulp.  Random-init head weights."""
    m1, bp1, n1, met1 = _split_run(monkeypatch, "head_generic=%d" % generic, conv, hw, N, want)
    assert "dense_epi0" not in n1 and bp1.head_blocks == 8
    m0, bp0, n0, met0 = _split_run(monkeypatch, "head_generic=%d,fuse_head=0" % generic, conv, hw, N, want)
    assert "dense_epi0" in n0 and bp0.head_blocks == 2
    assert torch.equal(bp1.dense_part[-1], bp0.dense_part[-1])
    assert torch.equal(bp1.dense_out[-1], bp0.dense_out[-1]), "fused epilogue differs from dense_epilogue_kernel"
    # same activations -> same rows; the unfused head adds four rows' losses in float32 before
    # the fixed-point accumulation (one rounding per addition), the fused one adds rows exactly
    assert met1[1:] == met0[1:] and abs(met1[0] - met0[0]) <= 4 * U * max(1.0, met0[0])
    n_hid = m1._executor.denses[-1].N
    part = bp1.dense_part[-1].double().cpu().numpy()
    ref = np.maximum(part.sum(0)[:, :n_hid] + m1.get_weights()[-3].astype(np.float64), 0.0)
    got = bp1.dense_out[-1].float().cpu().double().numpy()
    assert (np.abs(got[:, :n_hid] - ref) <= _bf16_ulp(ref)).all()
    assert (got[:, n_hid:] == 0).all() and (ref > 0).any()

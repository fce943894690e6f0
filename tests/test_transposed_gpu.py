"""Conv2DTranspose on the GPU: the three transposed.hip kernels alone against a float64 NumPy oracle written
as the plain loops of their formulas (exact on small-integer inputs; NaN-filled buffers with guard regions; a
second launch bit-identical), the launchers' checks, and whole models against the CPU executor with the
project's existing bounds."""
import numpy as np
import pytest
import torch

from cori_intml_examples_amd import (Conv2D, Conv2DTranspose, Dense, Dropout, Flatten, Input, MaxPooling2D, Model, optim,
                                     regularizers)
from cori_intml_examples_amd.apps import zoo
from cori_intml_examples_amd.models.layers import tconv_out_size
from cori_intml_examples_amd.models.lds_layout import conv_layout, tconv_wgrad_layout
from cori_intml_examples_amd.ops.reference import tconv_pads
from cori_intml_examples_amd.utils import set_random_seed

from test_hip_model import _data, _rel
from test_separable_gpu import Buf, _K, _bf16, _names, _pad, _stream, _twice, _ulp

pytestmark = pytest.mark.gpu

# (Cin, Cout, H, W, KH, KW, s, padding, B, want, kc): ``want`` workgroups asked of tconv_cfg (2 * B: two row
# blocks on the 5-row grid, 3 + 2 rows); kc: 0, or the k-steps of weights per chunk.  Borders: Cs 4 input, partial /
# one / 1.5 n-tiles, k not a multiple of s (unequal classes), k < s (bias-only outputs), k == s, 1x3, valid and same
# with k > s (border rows of the last block), s = 1, a short last row block, weight chunks, an 18x15 map (larger than
# the other maps because a second pass of m-tiles needs more than 256 pixels in a block: 270 input / 304 base pixels),
# 1x1 at s = 2 over 8 channels (single-tap and bias-only classes at the smallest K, half an m-tile of (tap, n) rows).
CASES = [(3, 5, 5, 4, 3, 3, 2, "same", 1, 1, 0), (8, 16, 5, 4, 3, 3, 2, "valid", 3, 6, 0),
         (40, 24, 5, 4, 4, 4, 2, "same", 1, 1, 0), (8, 5, 4, 5, 2, 2, 3, "valid", 3, 1, 0),
         (3, 24, 4, 5, 1, 3, 2, "valid", 1, 1, 0), (40, 16, 5, 4, 3, 3, 3, "same", 1, 1, 0),
         (8, 24, 4, 5, 2, 2, 2, "valid", 3, 1, 0), (40, 24, 5, 4, 3, 3, 2, "same", 1, 2, 2),
         (8, 16, 11, 9, 3, 3, 1, "same", 1, 1, 0), (8, 5, 18, 15, 3, 3, 2, "valid", 1, 1, 0),
         (24, 40, 5, 4, 5, 5, 3, "valid", 2, 1, 0), (8, 5, 4, 5, 1, 1, 2, "valid", 2, 1, 0)]


def _geo(case):
    Cin, Cout, H, W, KH, KW, s, padding = case[:8]
    pt, _, pl, _ = tconv_pads(KH, KW, s, padding)
    return (4 if Cin <= 4 else -(-Cin // 8) * 8, -(-Cout // 8) * 8, tconv_out_size(H, KH, s, padding),
            tconv_out_size(W, KW, s, padding), pt, pl)


def _args(K, kind, case):
    Cin, Cout, H, W, KH, KW, s, padding, B, want, kc = case
    a = K.TconvArgs()
    a.Cs_in, a.Cs_out, a.Ho, a.Wo, a.pad_t, a.pad_l = _geo(case)
    a.B, a.H, a.W, a.Cin, a.Cout, a.KH, a.KW, a.stride = B, H, W, Cin, Cout, KH, KW, s
    a.ntw = K.tconv_ntw(Cout if kind == K.TC_FWD else Cin, kind)
    if kind == K.TC_FWD:
        ty, tw, qw = -(-KH // s), -(-KW // s), -(-(a.Wo + a.pad_l) // s)
        a.xpix = conv_layout(a.Cs_in, qw + tw - 1, qw, False, ty, tw)
    elif kind == K.TC_DGRAD:
        a.xpix = conv_layout(a.Cs_out, (W - 1) * s + KW, W, False, KH, KW)
    else:
        a.xpix = tconv_wgrad_layout(a.Cs_out, (W - 1) * s + max(KW, s), W, KH, KW, s)
    a.R, a.kc = K.tconv_cfg(a, kind, want)
    assert a.R >= 1 and (kind != K.TC_FWD or want <= B or a.R < H)
    if kc and kind != K.TC_WGRAD:
        assert kc < a.kc
        a.kc = kc
    return a


def _oracle(x, w, b, dt, case):
    """(z, dx, dW, db) and the sums of |terms| of z, dx, dW by the formulas, in float64."""
    Cin, Cout, H, W, KH, KW, s, padding, B = case[:9]
    _, _, Ho, Wo, pt, pl = _geo(case)
    z, zm = np.zeros((B, Ho, Wo, Cout)) + b, np.zeros((B, Ho, Wo, Cout)) + np.abs(b)
    dx, dxm = np.zeros((B, H, W, Cin)), np.zeros((B, H, W, Cin))
    dw, dwm = np.zeros((KH, KW, Cout, Cin)), np.zeros((KH, KW, Cout, Cin))
    for i in range(H):
        for j in range(W):
            for ky in range(KH):
                for kx in range(KW):
                    Y, X = i * s + ky - pt, j * s + kx - pl
                    if 0 <= Y < Ho and 0 <= X < Wo:
                        z[:, Y, X] += x[:, i, j] @ w[ky, kx].T
                        zm[:, Y, X] += np.abs(x[:, i, j]) @ np.abs(w[ky, kx]).T
                        dx[:, i, j] += dt[:, Y, X] @ w[ky, kx]
                        dxm[:, i, j] += np.abs(dt[:, Y, X]) @ np.abs(w[ky, kx])
                        dw[ky, kx] += dt[:, Y, X].T @ x[:, i, j]
                        dwm[ky, kx] += np.abs(dt[:, Y, X]).T @ np.abs(x[:, i, j])
    return z, dx, dw, dt.sum((0, 1, 2)), zm, dxm, dwm


def _inputs(case, ints, seed=0):
    """x, w, b, dt, the feeding stage's saved output: small integers (sparse weights and gradients, so that
    every oracle value stays an exactly representable integer), or bf16-rounded normal draws."""
    Cin, Cout, H, W, KH, KW, s, padding, B = case[:9]
    _, _, Ho, Wo, _, _ = _geo(case)
    rs = np.random.RandomState(seed)
    if ints:
        draw = lambda shape, p: rs.randint(-2, 3, shape) * (rs.rand(*shape) < p)
        return (draw((B, H, W, Cin), 1.0), draw((KH, KW, Cout, Cin), 0.3), draw((Cout,), 1.0), draw((B, Ho, Wo, Cout), 0.3),
                draw((B, H, W, Cin), 1.0))
    return tuple(_bf16(rs.randn(*s)) for s in ((B, H, W, Cin), (KH, KW, Cout, Cin), (Cout,), (B, Ho, Wo, Cout))) + (
        rs.randint(-2, 3, (B, H, W, Cin)),)


def _run(case, ints, relu=False, prev="identity", seed=0):
    """Launch tconv_fwd, tconv_wgrad and (Cin > 4) tconv_dgrad of ``case``: {name: (got, want, sum of |terms|, terms)}."""
    K = _K()
    Cin, Cout, H, W, KH, KW, s, padding, B = case[:9]
    x, w, b, dt, prev_out = _inputs(case, ints, seed)
    z, dx, dw, db, zm, dxm, dwm = _oracle(x, w, b, dt, case)
    if ints:
        assert max(np.abs(z).max(), np.abs(dx).max()) <= 256 and max(np.abs(dw).max(), np.abs(db).max()) < 2 ** 24
    f = _args(K, K.TC_FWD, case)
    xb, wb, bb = Buf((B, H, W, f.Cs_in), torch.bfloat16, _pad(x, f.Cs_in)), Buf(w.shape, torch.float32, w), Buf((Cout,), torch.float32, b)
    ob, db_ = Buf((B, f.Ho, f.Wo, f.Cs_out), torch.bfloat16), Buf((B, f.Ho, f.Wo, f.Cs_out), torch.bfloat16, _pad(dt, f.Cs_out))
    f.x, f.w, f.bias, f.out, f.relu = xb.ptr, wb.ptr, bb.ptr, ob.ptr, int(relu)
    res, launches, outs = {}, [lambda: K.tconv_fwd(f, _stream())], [ob]
    g = _args(K, K.TC_WGRAD, case)
    npairs = B * -(-H // g.R)
    g.pairs_per_slab = 2 if npairs > 2 else 1
    g.S = -(-npairs // g.pairs_per_slab)
    boff = (w.size + 3) // 4 * 4
    g.slab_ld, g.has_bias = boff + Cout + 3, 1
    sb = Buf((g.S, g.slab_ld), torch.float32)
    g.x, g.dt, g.w, g.slab = xb.ptr, db_.ptr, wb.ptr, sb.ptr
    launches.append(lambda: K.tconv_wgrad(g, _stream()))
    outs.append(sb)
    if Cin > 4:
        a = _args(K, K.TC_DGRAD, case)
        pb, gb = Buf((B, H, W, a.Cs_in), torch.bfloat16, _pad(prev_out, a.Cs_in)), Buf((B, H, W, a.Cs_in), torch.bfloat16)
        codes = torch.zeros(B * H * W * a.Cs_in, dtype=torch.uint8, device="cuda")      # (no kernel here reads them)
        bt = K.BwdThrough()
        bt.prev_out, bt.dy, bt.prev_relu = pb.ptr, gb.ptr, int(prev != "identity")
        bt.pH, bt.pW, bt.pC, bt.pCs, bt.cH, bt.cW = H, W, Cin, a.Cs_in, H, W
        if prev == "pool":      # a max-pooled feeding stage: the gradient at pooled resolution, its relu mask from the pooled output
            bt.prev_pool, bt.prev_code, bt.cH, bt.cW = 1, codes.data_ptr(), 2 * H, 2 * W
        a.dt, a.w, a.bt = db_.ptr, wb.ptr, bt
        launches.append(lambda: K.tconv_dgrad(a, _stream()))
        outs.append(gb)
    for fn in launches:
        fn()
    torch.cuda.synchronize()
    got = [o.get() for o in outs]
    for fn in launches:
        _twice(fn, outs)
    assert np.all(got[0][..., Cout:] == 0.0), "padding channels"
    res["out"] = (got[0][..., :Cout], np.maximum(z, 0.0) if relu else z, zm, -(-KH // s) * -(-KW // s) * Cin + 1)
    used = np.zeros(g.slab_ld, bool)
    used[:w.size] = used[boff:boff + Cout] = True
    assert np.isnan(got[1][:, ~used]).all() and not np.isnan(got[1][:, used]).any()
    slab = np.where(used, got[1], 0.0).sum(0)
    res["dW"] = (slab[:w.size].reshape(w.shape), dw, dwm, B * H * W + g.S)      # the kernel's chain, then this sum over the slabs
    res["db"] = (slab[boff:boff + Cout], db, np.abs(dt).sum((0, 1, 2)), B * f.Ho * f.Wo + g.S)
    if Cin > 4:
        assert np.all(got[2][..., Cin:] == 0.0), "padding channels"
        res["dx"] = (got[2][..., :Cin], dx * (prev_out > 0) if prev != "identity" else dx, dxm, KH * KW * Cout)
    return res


@pytest.mark.parametrize("i", range(len(CASES)))
def test_kernels_are_exact_on_integers(i):
    """tconv_fwd, tconv_wgrad (dW, db) and tconv_dgrad (through an identity BwdThrough, a relu mask or a
    max-pooled feeding stage, by case) equal the oracle exactly."""
    res = _run(CASES[i], True, relu=bool(i % 2), prev=("identity", "relu", "pool")[i % 3])
    assert ("dx" in res) == (CASES[i][0] > 4)
    for name, (got, want, _, _) in res.items():
        np.testing.assert_array_equal(got, want, err_msg=name)


@pytest.mark.parametrize("i", [2, 5])
def test_normal_inputs_within_the_derived_bound(i):
    """Per element: one bf16 rounding of the exact value (where the result is stored as bf16) plus the fp32
    chain term n_terms * 2^-24 * sum |x * w|, on the bf16-rounded operands."""
    for name, (got, want, mag, n) in _run(CASES[i], False, seed=1 + i).items():
        bound = (_ulp(want) if name in ("out", "dx") else 0.0) + n * 2.0 ** -24 * mag
        print("case %d %s: max err / bound %.3g" % (i, name, float((np.abs(got - want) / (bound + 1e-300)).max())))
        assert np.all(np.abs(got - want) <= bound), name


def test_launchers_refuse_what_they_cannot_run():
    K = _K()
    buf = torch.zeros(1 << 18, dtype=torch.bfloat16, device="cuda")

    def filled(kind=None):
        a = _args(K, K.TC_FWD if kind is None else kind, CASES[1])
        a.x = a.out = a.dt = a.w = a.slab = buf.data_ptr()
        a.slab_ld, a.S, a.pairs_per_slab = 4096, 6, 1
        return a
    for field, value, match in (("Cs_in", 12, "channel stride"), ("Cs_out", 12, "channel stride"), ("stride", 5, "strides"),
                                ("stride", 0, "strides"), ("x", 0, "input pointer"), ("x", buf.data_ptr() + 2, "input pointer"),
                                ("out", 0, "output pointer"), ("w", 0, "weight pointer"), ("R", 0, "rows per block"),
                                ("kc", 0, "weight chunk"), ("ntw", 3, "n-tiles"), ("pad_t", 5, "padding"), ("Ho", 9, "output grid")):
        a = filled()
        setattr(a, field, value)
        with pytest.raises(ValueError, match=match):
            K.tconv_fwd(a, _stream())
    a = filled(K.TC_WGRAD)
    a.S = 5
    with pytest.raises(ValueError, match="pairs"):
        K.tconv_wgrad(a, _stream())
    with pytest.raises(ValueError, match="BwdThrough"):
        K.tconv_dgrad(filled(K.TC_DGRAD), _stream())
    a = filled()
    a.W, a.Wo = 8192, 8192 * 2 + 1        # one row block of this image is over 500 KB
    assert K.tconv_cfg(a, K.TC_FWD, 1)[0] == 0
    a.R = 1
    with pytest.raises(ValueError, match="LDS"):
        K.tconv_fwd(a, _stream())


# ------------------------------------------------------------------------------------------- models
def _hourglass(opt, device, reg=None, act="relu"):
    return zoo.rpv_hourglass_cnn((16, 16, 3), dropout=0.2, optimizer=opt, lr=None, device=device, activation=act,
                                 l2=1e-3 if reg else 0.0)


def _odd(opt, device, reg=None, act="relu"):
    """Odd sizes, valid padding: a transposed first stage (Cs 4, k == s, no dgrad), then a relu / tanh
    Conv2DTranspose(s = 2, k = 3) feeding an ordinary pooled conv."""
    kw = {"kernel_regularizer": regularizers.l2(1e-3)} if reg else {}
    h = inp = Input(shape=(5, 4, 2))
    h = Conv2DTranspose(5, (2, 2), strides=2, activation="relu", **kw)(h)
    h = Conv2DTranspose(12, (3, 3), strides=(2, 2), activation=act, **kw)(h)
    h = Dropout(0.2)(MaxPooling2D((2, 2))(Conv2D(9, (3, 3), activation="relu", padding="same", **kw)(h)))
    h = Dropout(0.2)(Dense(9, activation="relu")(Flatten()(h)))
    m = Model(inp, Dense(3, activation="softmax")(h), device=device)
    m.compile(optimizer=opt, loss="categorical_crossentropy", metrics=["accuracy"])
    return m


MODELS = {"hourglass": _hourglass, "odd": _odd}
OPTS = {"Adam": optim.Adam, "SGDm": lambda: optim.SGD(lr=0.01, momentum=0.9), "clip": lambda: optim.Adam(clipnorm=0.5)}


def _pair(kind, opt, **kw):
    out = []
    for dev in ("cuda", "cpu"):
        set_random_seed(1234)
        out.append(MODELS[kind](opt(), dev, **kw))
    for a, b in zip(out[0].get_weights(), out[1].get_weights()):
        np.testing.assert_array_equal(a, b)
    return out


@pytest.mark.parametrize("kind,opt,act", [("hourglass", "Adam", "relu"), ("odd", "SGDm", "relu"), ("hourglass", "clip", "relu"),
                                          ("odd", "Adam", "tanh")])
def test_three_steps_track_the_cpu_reference(kind, opt, act):
    """Relative L2 error of all weights <= 1e-2 after three steps over batches of 6, 6 and a ragged 4, dropout
    0.2 on the dense stage, fp32 CPU executor ("clip": clipnorm and l2; "tanh": act_fwd / act_bwd)."""
    g, c = _pair(kind, OPTS[opt], reg=opt == "clip", act=act)
    x, y = _data(g, 16, seed=3)
    n = g.store.numel
    w0 = g.store.master[:n].cpu().numpy()
    for m in (g, c):
        ex = m._executor
        d = ex.upload(x, y)
        perm = torch.arange(d.n, device=ex.device)
        for pos, bs in ((0, 6), (6, 6), (12, 4)):
            ex.train_step(d, perm, pos, bs)
    torch.cuda.synchronize()
    wg, wc = g.store.master[:n].cpu().numpy(), c.store.master[:n].numpy()
    print("%s %s %s: rel err %.3g, moved %.3g" % (kind, opt, act, _rel(wg, wc), _rel(wg, w0)))
    assert _rel(wg, wc) <= 1e-2 and _rel(wg, w0) > 1e-4
    names = _names(g, 6)
    want = {"hourglass": ["tconv_fwd3", "tconv_wgrad3", "tconv_dgrad3"],
            "odd": ["tconv_fwd0", "tconv_fwd1", "tconv_wgrad1", "tconv_dgrad1", "tconv_wgrad0"]}[kind]
    assert [nm for nm in names if nm.startswith("tconv_")] == want and names[0] == "prologue" and "conv_stack_fwd" not in names
    assert [nm for nm in names if nm.startswith("act_") and "_c" in nm] == (["act_fwd_c1", "act_bwd_c1"] if act == "tanh" else [])


@pytest.mark.parametrize("kind", sorted(MODELS))
def test_grads_match_the_bf16_reference(kind, monkeypatch):
    """Per tensor: relative error <= 5e-2 and cosine > 0.995 against the CPU executor under ref_bf16=1."""
    monkeypatch.setenv("INTML_TUNE", "ref_bf16=1")
    g, c = _pair(kind, lambda: optim.SGD(lr=0.0))
    assert c._executor.emulate_bf16
    x, y = _data(g, 48)
    for m in (g, c):
        ex = m._executor
        d = ex.upload(x, y)
        ex.train_step(d, torch.arange(d.n, device=ex.device), 0, d.n)
    torch.cuda.synchronize()
    gg, cg = g.store.grad[:g.store.numel].cpu().numpy(), c.store.grad[:c.store.numel].numpy()
    for s in g.store.specs:
        a, b = gg[s.offset:s.offset + s.numel], cg[s.offset:s.offset + s.numel]
        err, cos = _rel(a, b), float(np.dot(a, b) / max(np.linalg.norm(a) * np.linalg.norm(b), 1e-30))
        print("%s %s: grad rel err %.3g cos %.6f" % (kind, s.name, err, cos))
        assert err <= 5e-2 and cos > 0.995, s.name


def test_predict_and_evaluate_match():
    g, c = _pair("odd", optim.Adam)
    x, y = _data(g, 21, seed=5)
    g.fit(x, y, batch_size=8, epochs=1, verbose=0, shuffle=False)
    c.set_weights(g.get_weights())
    pg, pc = g.predict(x, batch_size=8), c.predict(x, batch_size=8)
    assert pg.shape == pc.shape and np.abs(pg - pc).max() < 2e-2
    eg, ec = g.evaluate(x, y, batch_size=8, verbose=0), c.evaluate(x, y, batch_size=8, verbose=0)
    assert abs(eg[0] - ec[0]) < 2e-2 * max(1, ec[0])


def test_plans_without_transposed_are_unchanged(monkeypatch):
    """The default RPV and MNIST models' training launch lists at batch 128, as the commit before this feature
    records them (tests/test_pooling_gpu.py RPV_TRAIN / MNIST_TRAIN pin the same lists)."""
    monkeypatch.delenv("INTML_TUNE", raising=False)
    want = {"rpv": ["conv_stack_fwd", "dense_fwd0", "head", "dense_bwd0", "wgrad_dgrad_conv2", "wgrad_dgrad_conv1",
                    "wgrad_conv0", "reduce_b0"],
            "mnist": ["conv_stack_fwd", "dense_fwd0", "head", "dense_bwd0", "wgrad_dgrad_conv1", "wgrad_conv0", "reduce_b0"]}
    set_random_seed(1)
    models = {"rpv": zoo.rpv_cnn((64, 64, 3), conv_sizes=[16, 32, 64], fc_sizes=[128], dropout=0.2, optimizer="Adam",
                                 lr=1e-3, device="cuda"),
              "mnist": zoo.mnist_cnn(32, 64, 128, dropout=0.4, optimizer="Adam", lr=1e-3, device="cuda")}
    for k, m in models.items():
        x, y = _data(m, 128)
        m.train_on_batch(x, y)
        assert _names(m, 128) == want[k], (k, _names(m, 128))

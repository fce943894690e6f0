"""UpSampling2D folded into a Conv2D on the GPU: the upsampled.hip kernels against the float64 loop oracle of
tests/test_upsampled.py, the launchers' checks, and whole models against the CPU executor with the existing bounds."""
import numpy as np
import pytest
import torch

from cori_intml_examples_amd import Conv2D, Dense, Dropout, Flatten, Input, MaxPooling2D, Model, UpSampling2D, optim, regularizers
from cori_intml_examples_amd.apps import zoo
from cori_intml_examples_amd.models.lds_layout import up_layout
from cori_intml_examples_amd.ops.reference import conv_pads
from cori_intml_examples_amd.utils import set_random_seed

from test_hip_model import _data, _rel
from test_pooling_gpu import RPV_TRAIN, _rpv
from test_separable_gpu import Buf, _K, _bf16, _names, _pad, _stream, _twice, _ulp
from test_upsampled import upconv_oracle

pytestmark = pytest.mark.gpu

# (Cin, Cout, H, W, KH, KW, s, padding, B, want, kc): ``want`` workgroups asked of up_cfg; kc: 0, or the k-steps of
# weights per chunk.  Borders: Cs 4 input, partial / one / 1.5 / 2.5 n-tiles, s = 2, 3, 4, same and valid 3x3, 2x2 same
# (pads 0 / 1), 1x1 (one source pixel per output), 1x3, 5x5 at s = 2 (a tap span of three source pixels), 10 output rows
# at s = 3 in blocks of 4 + 4 + 2 (case 1) and at s = 2 in blocks of 5 + 5 (case 7, which ALSO carries the forced weight
# chunk; case 9 splits 8 rows 4 + 4), a 9x8 source at s = 2 (288 output pixels in one block: a second pass of m-tiles).
CASES = [(3, 5, 4, 5, 3, 3, 2, "same", 1, 1, 0), (8, 16, 4, 5, 3, 3, 3, "valid", 2, 6, 0),
         (40, 24, 5, 4, 2, 2, 2, "same", 1, 1, 0), (8, 5, 4, 5, 1, 1, 3, "valid", 3, 1, 0),
         (3, 24, 4, 5, 1, 3, 2, "valid", 1, 1, 0), (40, 40, 5, 4, 5, 5, 2, "same", 1, 1, 0),
         (8, 16, 4, 5, 3, 3, 4, "same", 2, 1, 0), (40, 24, 5, 4, 3, 3, 2, "same", 1, 2, 2),
         (8, 5, 9, 8, 3, 3, 2, "same", 1, 1, 0), (8, 16, 5, 4, 3, 3, 2, "valid", 3, 6, 0)]


def _args(K, kind, case):
    Cin, Cout, H, W, KH, KW, s, padding, B, want, kc = case
    pt, pb, pl, pr = conv_pads(H * s, W * s, KH, KW, 1, padding)
    a, dg = K.UpArgs(), kind == K.UP_DGRAD
    a.B, a.H, a.W, a.Cin, a.Cout, a.KH, a.KW, a.up, a.pad_t, a.pad_l = B, H, W, Cin, Cout, KH, KW, s, pt, pl
    a.Cs_in, a.Cs_out, a.Ho, a.Wo = 4 if Cin <= 4 else -(-Cin // 8) * 8, -(-Cout // 8) * 8, H * s + pt + pb - KH + 1, W * s + pl + pr - KW + 1
    a.ntw = K.up_ntw(Cin if dg else Cout, kind)
    a.xpix = up_layout(a.Cs_out if dg else a.Cs_in, s, ("fwd", "dgrad", "wgrad")[kind])
    a.R, a.kc = K.up_cfg(a, kind, want)
    assert a.R >= 1 and (not kc or kc < a.kc or kind == K.UP_WGRAD)
    a.kc = kc if kc and kind != K.UP_WGRAD else a.kc
    return a


def _run(case, ints, relu=False, prev="identity", seed=0):
    """Launch upconv_fwd, upconv_wgrad and (Cin > 4) upconv_dgrad: {name: (got, want, sum of |terms|, terms)}.  Inputs: small
    integers (sparse weights and gradients: every oracle value an exactly representable integer), or bf16-rounded normal draws."""
    K, rs = _K(), np.random.RandomState(seed)
    Cin, Cout, H, W, KH, KW, s, padding, B = case[:9]
    f, g = _args(K, K.UP_FWD, case), _args(K, K.UP_WGRAD, case)
    draw = lambda shape, p: rs.randint(-2, 3, shape) * (rs.rand(*shape) < p) if ints else _bf16(rs.randn(*shape))
    x, w, b, dt = draw((B, H, W, Cin), 1.0), draw((KH, KW, Cin, Cout), 0.3), draw((Cout,), 1.0), draw((B, f.Ho, f.Wo, Cout), 0.3)
    prev_out = rs.randint(-2, 3, (B, H, W, Cin))      # the feeding stage's saved output
    z, dx, dw, db, zm, dxm, dwm = upconv_oracle(x, w, b, dt, s, f.pad_t, f.pad_l)
    if ints:
        assert max(np.abs(z).max(), np.abs(dx).max()) <= 256 and max(np.abs(dw).max(), np.abs(db).max()) < 2 ** 24
    xb, wb, bb = Buf((B, H, W, f.Cs_in), torch.bfloat16, _pad(x, f.Cs_in)), Buf(w.shape, torch.float32, w), Buf((Cout,), torch.float32, b)
    ob, db_ = Buf((B, f.Ho, f.Wo, f.Cs_out), torch.bfloat16), Buf((B, f.Ho, f.Wo, f.Cs_out), torch.bfloat16, _pad(dt, f.Cs_out))
    f.x, f.w, f.bias, f.out, f.relu = xb.ptr, wb.ptr, bb.ptr, ob.ptr, int(relu)
    npairs, boff = B * -(-f.Ho // g.R), (w.size + 3) // 4 * 4
    g.pairs_per_slab = 1 + (npairs > 2)
    g.S, g.slab_ld, g.has_bias = -(-npairs // g.pairs_per_slab), boff + Cout + 3, 1
    sb = Buf((g.S, g.slab_ld), torch.float32)
    g.x, g.dt, g.w, g.slab = xb.ptr, db_.ptr, wb.ptr, sb.ptr
    launches, outs = [lambda: K.upconv_fwd(f, _stream()), lambda: K.upconv_wgrad(g, _stream())], [ob, sb]
    if Cin > 4:
        a, bt = _args(K, K.UP_DGRAD, case), K.BwdThrough()
        pb, gb = Buf((B, H, W, a.Cs_in), torch.bfloat16, _pad(prev_out, a.Cs_in)), Buf((B, H, W, a.Cs_in), torch.bfloat16)
        codes = torch.zeros(B * H * W * a.Cs_in, dtype=torch.uint8, device="cuda")      # (no kernel here reads them)
        bt.prev_out, bt.dy, bt.prev_relu = pb.ptr, gb.ptr, int(prev != "identity")
        bt.pH, bt.pW, bt.pC, bt.pCs, bt.cH, bt.cW = H, W, Cin, a.Cs_in, H, W
        if prev == "pool":      # the gradient at a max-pooled feeder's resolution, its relu mask from the pooled output
            bt.prev_pool, bt.prev_code, bt.cH, bt.cW = 1, codes.data_ptr(), 2 * H, 2 * W
        a.dt, a.w, a.bt = db_.ptr, wb.ptr, bt
        launches, outs = launches + [lambda: K.upconv_dgrad(a, _stream())], outs + [gb]
    for fn in launches:
        fn()
    torch.cuda.synchronize()
    got = [o.get() for o in outs]
    for fn in launches:
        _twice(fn, outs)
    used = (np.arange(g.slab_ld) < w.size) | ((np.arange(g.slab_ld) >= boff) & (np.arange(g.slab_ld) < boff + Cout))
    assert all(np.all(v[..., n:] == 0.0) for v, n in zip(got[::2], (Cout, Cin))) and np.isnan(got[1][:, ~used]).all() and not np.isnan(got[1][:, used]).any()
    slab, nt = np.where(used, got[1], 0.0).sum(0), B * f.Ho * f.Wo + g.S      # the kernel's chain, then this sum over the slabs
    res = {"out": (got[0][..., :Cout], np.maximum(z, 0.0) if relu else z, zm, KH * KW * Cin + 1),
           "dW": (slab[:w.size].reshape(w.shape), dw, dwm, nt), "db": (slab[boff:boff + Cout], db, np.abs(dt).sum((0, 1, 2)), nt)}
    if Cin > 4:
        res["dx"] = (got[2][..., :Cin], dx * (prev_out > 0) if prev != "identity" else dx, dxm, s * s * KH * KW * Cout)
    return res


@pytest.mark.parametrize("i", range(len(CASES)))
def test_kernels_are_exact_on_integers(i):
    """z, dW, db and dx (through an identity BwdThrough, a relu mask, or one at a max-pooled feeder's resolution) equal the oracle."""
    res = _run(CASES[i], True, relu=bool(i % 2), prev=("identity", "relu", "pool")[i % 3])
    assert ("dx" in res) == (CASES[i][0] > 4)
    for name, (got, want, _, _) in res.items():
        np.testing.assert_array_equal(got, want, err_msg=name)


@pytest.mark.parametrize("i", [1, 5, 7])
def test_normal_inputs_within_the_derived_bound(i):
    """Per element: one bf16 rounding of the exact value (where stored as bf16) plus n_terms * 2^-24 * sum |x * w|."""
    for name, (got, want, mag, n) in _run(CASES[i], False, seed=1 + i).items():
        bound = (_ulp(want) if name in ("out", "dx") else 0.0) + n * 2.0 ** -24 * mag
        print("case %d %s: max err / bound %.3g" % (i, name, float((np.abs(got - want) / (bound + 1e-300)).max())))
        assert np.all(np.abs(got - want) <= bound), name


@pytest.mark.parametrize("kind,fields,match", [
    (0, {"Cs_in": 12}, "channel stride"), (0, {"Cs_out": 12}, "channel stride"), (0, {"Cs_out": 32}, "channel stride"),
    (0, {"up": 5}, "size"), (0, {"up": 0}, "size"), (0, {"x": 0}, "input pointer"), (0, {"x": 2}, "input pointer"),
    (0, {"out": 0}, "output pointer"), (0, {"w": 0}, "weight pointer"), (0, {"R": 0}, "rows per block"), (0, {"kc": 0}, "weight chunk"),
    (0, {"ntw": 3}, "n-tiles"), (0, {"pad_t": 1}, "output grid"), (0, {"Ho": 9}, "output grid"), (0, {"W": 8192}, "output grid"),
    (0, {"W": 8192, "Wo": 16382, "R": 1}, "LDS"), (2, {"S": 5}, "pairs"), (1, {}, "BwdThrough")])
def test_launchers_refuse_what_they_cannot_run(kind, fields, match):
    """kind: UP_FWD / UP_DGRAD / UP_WGRAD (its BwdThrough left empty).  Nothing is launched: the buffer stays zero."""
    K, buf = _K(), torch.zeros(1 << 18, dtype=torch.bfloat16, device="cuda")
    a = _args(K, kind, CASES[9])
    a.x = a.out = a.dt = a.w = a.slab = buf.data_ptr()
    a.slab_ld, a.S, a.pairs_per_slab = 4096, 6, 1
    for k, v in fields.items():
        setattr(a, k, buf.data_ptr() + v if k in ("x", "out", "w") and v else v)
    with pytest.raises(ValueError, match=match):
        (K.upconv_fwd, K.upconv_dgrad, K.upconv_wgrad)[kind](a, _stream())
    assert not buf.any()


# ------------------------------------------------------------------------------------------- models
def _odd(opt, device, reg=None, act="relu", sizes=(3, 2), shape=(5, 4, 2)):
    """Odd sizes, valid: an up-sampled stage 0 (Cs 4, s = 3), a relu / tanh one (s = 2), a pooled conv; sizes None: no UpSampling2D."""
    kw = {"kernel_regularizer": regularizers.l2(1e-3)} if reg else {}
    up = lambda i, t: UpSampling2D(sizes[i])(t) if sizes else t
    h = inp = Input(shape=shape)
    h = Conv2D(12, (3, 3), activation=act, **kw)(up(1, Conv2D(5, (2, 2), activation="relu", **kw)(up(0, h))))
    h = Dropout(0.2)(MaxPooling2D((2, 2))(Conv2D(9, (3, 3), activation="relu", padding="same", **kw)(h)))
    m = Model(inp, Dense(3, activation="softmax")(Dropout(0.2)(Dense(9, activation="relu")(Flatten()(h)))), device=device)
    m.compile(optimizer=opt, loss="categorical_crossentropy", metrics=["accuracy"])
    return m


MODELS = {"odd": _odd, "hourglass": lambda opt, device, reg=None, act="relu": zoo.rpv_hourglass_cnn(
    (16, 16, 3), dropout=0.2, optimizer=opt, lr=None, device=device, up_mode="upsample")}
OPTS = {"Adam": optim.Adam, "SGDm": lambda: optim.SGD(lr=0.01, momentum=0.9), "clip": lambda: optim.Adam(clipnorm=0.5)}


def _trained_pair(kind, opt, x_of, batches, **kw):
    """[GPU model, CPU model, initial weights], from one seed, each after train steps over ``batches`` of one data set."""
    out = []
    for dev in ("cuda", "cpu"):
        set_random_seed(1234)
        out.append(MODELS[kind](opt(), dev, **kw))
    (x, y), w0 = x_of(out[0]), out[0].store.master[:out[0].store.numel].cpu().numpy()
    for m in out:
        ex = m._executor
        d = ex.upload(x, y)
        for pos, bs in batches:
            ex.train_step(d, torch.arange(d.n, device=ex.device), pos, bs)
    torch.cuda.synchronize()
    return out + [w0]


@pytest.mark.parametrize("kind,opt,act", [("hourglass", "Adam", "relu"), ("odd", "SGDm", "relu"), ("odd", "clip", "tanh"),
                                          ("hourglass", "grads", "relu"), ("odd", "grads", "relu")])
def test_models_track_the_cpu_reference(kind, opt, act, monkeypatch):
    """Relative L2 of all weights <= 1e-2 after steps over batches of 6, 6 and a ragged 4 against the fp32 CPU executor ("clip":
    clipnorm and l2; "tanh": act_fwd / act_bwd).  "grads": one step under ref_bf16=1, per tensor relative error <= 5e-2, cosine > 0.995."""
    if opt == "grads":
        monkeypatch.setenv("INTML_TUNE", "ref_bf16=1")
        g, c, _ = _trained_pair(kind, lambda: optim.SGD(lr=0.0), lambda m: _data(m, 48), ((0, 48),))
        assert c._executor.emulate_bf16
        gg, cg = g.store.grad[:g.store.numel].cpu().numpy(), c.store.grad[:c.store.numel].numpy()
        for s in g.store.specs:
            a, b = gg[s.offset:s.offset + s.numel], cg[s.offset:s.offset + s.numel]
            err, cos = _rel(a, b), float(np.dot(a, b) / max(np.linalg.norm(a) * np.linalg.norm(b), 1e-30))
            print("%s %s: grad rel err %.3g cos %.6f" % (kind, s.name, err, cos))
            assert err <= 5e-2 and cos > 0.995, s.name
        return
    g, c, w0 = _trained_pair(kind, OPTS[opt], lambda m: _data(m, 16, seed=3), ((0, 6), (6, 6), (12, 4)), reg=opt == "clip", act=act)
    n = g.store.numel
    wg, wc = g.store.master[:n].cpu().numpy(), c.store.master[:n].numpy()
    print("%s %s %s: rel err %.3g, moved %.3g" % (kind, opt, act, _rel(wg, wc), _rel(wg, w0)))
    assert _rel(wg, wc) <= 1e-2 and _rel(wg, w0) > 1e-4
    names = _names(g, 6)
    want = {"hourglass": ["upconv_fwd3", "upconv_wgrad3", "upconv_dgrad3"],
            "odd": ["upconv_fwd0", "upconv_fwd1", "upconv_wgrad1", "upconv_dgrad1", "upconv_wgrad0"]}[kind]
    assert [nm for nm in names if nm.startswith("upconv_")] == want and names[0] == "prologue" and "conv_stack_fwd" not in names
    assert [nm for nm in names if nm.startswith("act_") and "_c" in nm] == (["act_fwd_c1", "act_bwd_c1"] if act == "tanh" else [])


def test_plans_without_the_layer_are_unchanged(monkeypatch):
    """UpSampling2D(1) records the list of the model without the layer; the default RPV model the list test_pooling_gpu.py pins."""
    monkeypatch.delenv("INTML_TUNE", raising=False)
    one, none, rpv = [_odd(optim.Adam(), "cuda", sizes=sz, shape=(9, 8, 2)) for sz in ((1, 1), None)] + [_rpv()]
    for m, bs in ((one, 6), (none, 6), (rpv, 128)):
        m.train_on_batch(*_data(m, bs))
    assert _names(one, 6) == _names(none, 6) and not any(nm.startswith("upconv_") for nm in _names(one, 6))
    assert _names(rpv, 128) == RPV_TRAIN


def test_a_stage_over_the_lds_budget_is_refused_when_the_plan_is_built():
    h = inp = Input(shape=(2, 4096, 64))      # one staged row block of this map is about a megabyte
    h = Flatten()(Conv2D(8, (3, 3), padding="same", name="cv")(UpSampling2D(2, name="ups")(h)))
    m = Model(inp, Dense(1, activation="sigmoid")(h), device="cuda")
    m.compile(optimizer="Adam", loss="binary_crossentropy")
    with pytest.raises(NotImplementedError, match=r"layer cv \(upconv_fwd0, up-sampled by ups\): .* \d+ bytes, exceeds .* 163840 bytes of LDS"):
        m.train_on_batch(*_data(m, 2))

"""DepthwiseConv2D / SeparableConv2D on the GPU: the three depthwise.hip kernels alone against a
float64 NumPy oracle written from their formulas (exact on small-integer inputs; NaN-filled buffers
with guard regions; repeated launches bit-identical), the launchers' checks, and whole models
against the CPU executor with the project's existing bounds."""
import numpy as np
import pytest
import torch

from cori_intml_examples_amd import Conv2D, Dense, Dropout, Flatten, Input, MaxPooling2D, Model, optim
from cori_intml_examples_amd.models import DepthwiseConv2D, SeparableConv2D
from cori_intml_examples_amd.models.step_program import dropout_pair
from cori_intml_examples_amd.ops.reference import conv_out_size, conv_pads
from cori_intml_examples_amd.ops.rng import dropout_keep
from cori_intml_examples_amd.utils import set_random_seed

from test_hip_model import _data, _rel

pytestmark = pytest.mark.gpu
NAN = float("nan")
GUARD = 64

# (C, H, W, KH, KW, stride, padding, B, want): ``want`` workgroups asked of dw_rows -- 2 * B on the 11-row
# grid gives two row blocks per image, 6 + 5 rows.  Every C, grid, tap set and B appears (with every kernel).
CASES = [(3, 7, 5, 3, 3, 1, "same", 1, 1), (8, 9, 9, 3, 3, 2, "same", 5, 1), (20, 11, 6, 5, 5, 1, "valid", 1, 2),
         (20, 7, 5, 1, 3, 2, "valid", 5, 1), (8, 11, 6, 3, 3, 1, "same", 5, 10), (3, 9, 9, 5, 5, 1, "valid", 1, 1),
         (20, 9, 9, 3, 3, 2, "same", 1, 1), (8, 7, 5, 1, 3, 2, "valid", 1, 1)]


def _K():
    from cori_intml_examples_amd.ops.hip import kernels
    return kernels()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Buf:
    """A tensor of ``dtype`` holding ``vals`` (or NaN) between two NaN guard regions."""

    def __init__(self, shape, dtype, vals=None):
        n = int(np.prod(shape))
        full = np.full(n + 2 * GUARD, NAN, np.float64)
        if vals is not None:
            full[GUARD:GUARD + n] = np.asarray(vals, np.float64).reshape(-1)
        self.shape, self.n = tuple(shape), n
        self.t = torch.tensor(full).to(dtype).cuda()
        self.ptr = self.t.data_ptr() + GUARD * self.t.element_size()

    def get(self):
        v = self.t.double().cpu().numpy()
        assert np.isnan(v[:GUARD]).all() and np.isnan(v[GUARD + self.n:]).all(), "guard region written"
        return v[GUARD:GUARD + self.n].reshape(self.shape)


def _geo(C, H, W, KH, KW, s, padding):
    Cs = 4 if C <= 4 else -(-C // 8) * 8
    pt, _, pl, _ = conv_pads(H, W, KH, KW, s, padding)
    return Cs, conv_out_size(H, KH, s, padding), conv_out_size(W, KW, s, padding), pt, pl


def _args(K, kind, case, want=None):
    C, H, W, KH, KW, s, padding, B, w = case
    Cs, Ho, Wo, pt, pl = _geo(C, H, W, KH, KW, s, padding)
    a = K.DwArgs()
    a.B, a.H, a.W, a.C, a.Cs, a.Ho, a.Wo = B, H, W, C, Cs, Ho, Wo
    a.KH, a.KW, a.stride, a.pad_t, a.pad_l = KH, KW, s, pt, pl
    a.R = K.dw_rows(a, kind, w if want is None else want)
    assert a.R >= 1
    return a


def _pad(v, Cs, fill=0.0):
    """[.., C] -> [.., Cs] with ``fill`` in the padding lanes."""
    out = np.full(v.shape[:-1] + (Cs,), fill, np.float64)
    out[..., :v.shape[-1]] = v
    return out


def _oracle_fwd(x, w, b, case):
    C, H, W, KH, KW, s, padding, B, _ = case
    _, Ho, Wo, pt, pl = _geo(C, H, W, KH, KW, s, padding)
    y, mag = np.zeros((B, Ho, Wo, C)), np.zeros((B, Ho, Wo, C))
    for oy in range(Ho):
        for ox in range(Wo):
            for ky in range(KH):
                for kx in range(KW):
                    iy, ix = oy * s + ky - pt, ox * s + kx - pl
                    if 0 <= iy < H and 0 <= ix < W:
                        y[:, oy, ox] += x[:, iy, ix] * w[ky, kx]
                        mag[:, oy, ox] += np.abs(x[:, iy, ix] * w[ky, kx])
    return y + b, mag + np.abs(b)


def _oracle_dx(dt, w, case):
    C, H, W, KH, KW, s, padding, B, _ = case
    _, Ho, Wo, pt, pl = _geo(C, H, W, KH, KW, s, padding)
    dx, mag = np.zeros((B, H, W, C)), np.zeros((B, H, W, C))
    for y in range(H):
        for x in range(W):
            for ky in range(KH):
                for kx in range(KW):
                    ny, nx = y + pt - ky, x + pl - kx
                    if ny % s == 0 and nx % s == 0 and 0 <= ny // s < Ho and 0 <= nx // s < Wo:
                        dx[:, y, x] += w[ky, kx] * dt[:, ny // s, nx // s]
                        mag[:, y, x] += np.abs(w[ky, kx] * dt[:, ny // s, nx // s])
    return dx, mag


def _oracle_dw(x, dt, case):
    C, H, W, KH, KW, s, padding, B, _ = case
    _, Ho, Wo, pt, pl = _geo(C, H, W, KH, KW, s, padding)
    dw, mag = np.zeros((KH, KW, C)), np.zeros((KH, KW, C))
    for ky in range(KH):
        for kx in range(KW):
            for oy in range(Ho):
                for ox in range(Wo):
                    iy, ix = oy * s + ky - pt, ox * s + kx - pl
                    if 0 <= iy < H and 0 <= ix < W:
                        dw[ky, kx] += (x[:, iy, ix] * dt[:, oy, ox]).sum(0)
                        mag[ky, kx] += np.abs(x[:, iy, ix] * dt[:, oy, ox]).sum(0)
    return dw, dt.sum((0, 1, 2)), mag, np.abs(dt).sum((0, 1, 2))


def _bf16(v):
    return torch.tensor(np.asarray(v, np.float64)).to(torch.bfloat16).double().numpy()


def _draw(rs, shape, ints):
    return rs.randint(-4, 5, shape).astype(np.float64) if ints else _bf16(rs.randn(*shape))


def _ulp(v):
    return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -126))) - 7)


def _twice(launch, bufs):
    """A second launch into the same buffers leaves them bit-identical."""
    first = [b.t.clone() for b in bufs]
    launch()
    torch.cuda.synchronize()
    for a, b in zip(first, bufs):
        assert torch.equal(a.view(torch.int16 if a.element_size() == 2 else torch.int32),
                           b.t.view(torch.int16 if a.element_size() == 2 else torch.int32))


def _run_fwd(case, ints, relu, seed=0, cs_out=0):
    K, rs = _K(), np.random.RandomState(seed)
    C, H, W, KH, KW, s, padding, B, _ = case
    a = _args(K, K.DW_FWD, case)
    a.Cs_out, cso = cs_out, cs_out or a.Cs
    x, w = _draw(rs, (B, H, W, C), ints), _draw(rs, (KH, KW, C), ints)
    b = _draw(rs, (C,), ints)
    xb, ob = Buf((B, H, W, a.Cs), torch.bfloat16, _pad(x, a.Cs)), Buf((B, a.Ho, a.Wo, cso), torch.bfloat16)
    wb, bb = Buf((KH, KW, C), torch.float32, w), Buf((C,), torch.float32, b)
    a.x, a.w, a.bias, a.out, a.relu = xb.ptr, wb.ptr, bb.ptr, ob.ptr, int(relu)
    launch = lambda: K.dw_fwd(a, _stream())
    launch()
    torch.cuda.synchronize()
    got = ob.get()
    _twice(launch, [ob])
    want, mag = _oracle_fwd(x, w, b, case)
    if relu:
        want = np.maximum(want, 0.0)
    assert np.all(got[..., C:] == 0.0), "padding lanes"
    return got[..., :C], want, mag, KH * KW + 1, a


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("relu", [False, True])
def test_forward_is_exact_on_integers(case, relu):
    got, want, _, _, a = _run_fwd(case, True, relu)
    assert a.R < a.Ho or case[8] <= case[7]           # (the two-block cases really have two blocks)
    np.testing.assert_array_equal(got, want)


def test_forward_normal_inputs_within_the_derived_bound():
    got, want, mag, n, _ = _run_fwd(CASES[2], False, False, seed=1)
    bound = _ulp(want) + n * 2.0 ** -24 * mag
    print("dw_fwd: max err / bound %.3g" % float((np.abs(got - want) / bound).max()))
    assert np.all(np.abs(got - want) <= bound)


def _run_dgrad(case, ints, prev, rate=0.0, seed=0, cs_out=0):
    """prev: 'identity' | 'relu' | 'pool' (a max-pooled feeding stage: its relu mask from the pooled output)."""
    K, rs = _K(), np.random.RandomState(seed)
    C, H, W, KH, KW, s, padding, B, _ = case
    a = _args(K, K.DW_DGRAD, case)
    a.Cs_out, cso = cs_out, cs_out or a.Cs
    dt, w = _draw(rs, (B, a.Ho, a.Wo, C), ints), _draw(rs, (KH, KW, C), ints)
    prev_out = _draw(rs, (B, H, W, C), True)
    db, wb = Buf((B, a.Ho, a.Wo, cso), torch.bfloat16, _pad(dt, cso)), Buf((KH, KW, C), torch.float32, w)
    pb, gb = Buf((B, H, W, a.Cs), torch.bfloat16, _pad(prev_out, a.Cs)), Buf((B, H, W, a.Cs), torch.bfloat16)
    codes = torch.zeros(B * H * W * a.Cs, dtype=torch.uint8, device="cuda")      # (no kernel here reads them)
    st = torch.zeros(K.STEP_STATE_BYTES, dtype=torch.uint8, device="cuda")
    st.view(torch.int32)[0] = 7
    a.dt, a.w, a.st = db.ptr, wb.ptr, st.data_ptr()
    bt = K.BwdThrough()
    bt.prev_out, bt.dy, bt.prev_relu = pb.ptr, gb.ptr, int(prev != "identity")
    bt.pH, bt.pW, bt.pC, bt.pCs, bt.cH, bt.cW = H, W, C, a.Cs, H, W
    if prev == "pool":
        bt.prev_pool, bt.prev_code, bt.cH, bt.cW = 1, codes.data_ptr(), 2 * H, 2 * W
    if rate:
        bt.drop_thr, bt.drop_scale = dropout_pair(rate)
        bt.seed, bt.stream_id = 4321, 2
    a.bt = bt
    launch = lambda: K.dw_dgrad(a, _stream())
    launch()
    torch.cuda.synchronize()
    got = gb.get()
    _twice(launch, [gb])
    want, mag = _oracle_dx(dt, w, case)
    if rate:
        keep = dropout_keep(B * H * W * C, rate, 4321, 2, 7).double().numpy().reshape(B, H, W, C)
        want = want * keep * np.float64(np.float32(1.0 / (1.0 - rate)))
    if prev != "identity":
        want = want * (prev_out > 0)
    assert np.all(got[..., C:] == 0.0), "padding lanes"
    return got[..., :C], want, mag, KH * KW


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("prev", ["identity", "relu", "pool"])
def test_routed_gradient_is_exact_on_integers(case, prev):
    got, want, _, _ = _run_dgrad(case, True, prev)
    np.testing.assert_array_equal(got, want)


def test_routed_gradient_with_dropout_within_one_ulp():
    got, want, mag, n = _run_dgrad(CASES[4], False, "relu", rate=0.2, seed=2)
    bound = _ulp(want)                      # one bf16 ulp of the oracle value (0 where the mask drops)
    print("dw_dgrad: max err / bound %.3g" % float((np.abs(got - want) / bound).max()))
    assert np.all(np.abs(got - want) <= bound) and np.any(want == 0) and np.any(want != 0)


def _run_wgrad(case, ints, bias, seed=0, slabs=None, cs_out=0):
    K, rs = _K(), np.random.RandomState(seed)
    C, H, W, KH, KW, s, padding, B, _ = case
    a = _args(K, K.DW_WGRAD, case)
    a.Cs_out, cso = cs_out, cs_out or a.Cs
    x, dt = _draw(rs, (B, H, W, C), ints), _draw(rs, (B, a.Ho, a.Wo, C), ints)
    xb, db = Buf((B, H, W, a.Cs), torch.bfloat16, _pad(x, a.Cs)), Buf((B, a.Ho, a.Wo, cso), torch.bfloat16, _pad(dt, cso))
    npairs = B * -(-a.Ho // a.R)
    a.pairs_per_slab = -(-npairs // (slabs or npairs))
    a.S = -(-npairs // a.pairs_per_slab)
    boff = (KH * KW * C + 3) // 4 * 4
    a.slab_ld, a.has_bias = boff + C + 3, int(bias)
    sb = Buf((a.S, a.slab_ld), torch.float32)
    wb = Buf((KH, KW, C), torch.float32, np.zeros((KH, KW, C)))
    a.x, a.dt, a.w, a.slab = xb.ptr, db.ptr, wb.ptr, sb.ptr
    launch = lambda: K.dw_wgrad(a, _stream())
    launch()
    torch.cuda.synchronize()
    slab = sb.get()
    _twice(launch, [sb])
    used = np.zeros(a.slab_ld, bool)
    used[:KH * KW * C] = True
    used[boff:boff + C] = bool(bias)
    assert np.isnan(slab[:, ~used]).all() and not np.isnan(slab[:, used]).any()
    got = np.where(used, slab, 0.0).sum(0)
    dw, dbias, mag, bmag = _oracle_dw(x, dt, case)
    return got[:KH * KW * C].reshape(KH, KW, C), got[boff:boff + C], dw, dbias, mag, bmag, a


@pytest.mark.parametrize("case", CASES)
def test_weight_gradient_is_exact_on_integers(case):
    gw, gb, dw, db, _, _, a = _run_wgrad(case, True, True)
    np.testing.assert_array_equal(gw, dw)
    np.testing.assert_array_equal(gb, db)
    assert np.abs(dw).max() < 2 ** 24


def test_weight_gradient_more_pairs_than_slabs_and_no_bias():
    gw, gb, dw, _, _, _, a = _run_wgrad(CASES[4], True, False, slabs=3)
    assert a.S == 3 and a.pairs_per_slab == 4 and a.B * -(-a.Ho // a.R) == 10
    np.testing.assert_array_equal(gw, dw)
    assert np.all(gb == 0)


def test_weight_gradient_normal_inputs_within_the_derived_bound():
    gw, gb, dw, db, mag, bmag, a = _run_wgrad(CASES[1], False, True, seed=3)
    n = a.B * a.Ho * a.Wo + a.S           # the kernel's chain, then this test's sum over the slabs
    assert np.all(np.abs(gw - dw) <= n * 2.0 ** -24 * mag) and np.all(np.abs(gb - db) <= n * 2.0 ** -24 * bmag)
    print("dw_wgrad: max err / bound %.3g" % float((np.abs(gw - dw) / (n * 2.0 ** -24 * mag + 1e-300)).max()))


@pytest.mark.parametrize("kind", ["fwd", "dgrad", "wgrad"])
def test_four_lane_input_with_eight_lane_output(kind):
    """A depthwise stage behind a model input of <= 4 channels: x has Cs 4, out / dt have Cs_out 8."""
    if kind == "fwd":
        got, want = _run_fwd(CASES[0], True, True, cs_out=8)[:2]
    elif kind == "dgrad":
        got, want = _run_dgrad(CASES[5], True, "relu", cs_out=8)[:2]
    else:
        gw, gb, dw, db = _run_wgrad(CASES[0], True, True, cs_out=8)[:4]
        got, want = np.concatenate([gw.ravel(), gb]), np.concatenate([dw.ravel(), db])
    np.testing.assert_array_equal(got, want)


def test_launchers_refuse_what_they_cannot_run():
    K = _K()
    ok = lambda: _args(K, K.DW_FWD, CASES[1])
    buf = torch.zeros(1 << 16, dtype=torch.bfloat16, device="cuda")

    def filled():
        a = ok()
        a.x = a.out = a.dt = a.w = a.slab = buf.data_ptr()
        a.slab_ld, a.S, a.pairs_per_slab = 1024, 5, 1
        return a
    for field, value, match in (("Cs", 12, "channel stride"), ("depth_multiplier", 2, "depth_multiplier"),
                                ("C", 9, "channels"), ("R", 0, "rows per block"), ("pad_t", 3, "padding"),
                                ("x", 0, "input pointer"), ("Cs_out", 16, "channel stride")):
        a = filled()
        setattr(a, field, value)
        with pytest.raises(ValueError, match=match):
            K.dw_fwd(a, _stream())
    a = filled()
    a.S = 4
    with pytest.raises(ValueError, match="pairs"):
        K.dw_wgrad(a, _stream())
    a = filled()
    with pytest.raises(ValueError, match="BwdThrough"):
        K.dw_dgrad(a, _stream())
    a = filled()
    a.W = a.Wo = 4096                     # one row of this halo is 196 KB
    a.KW, a.stride, a.pad_l = 1, 1, 0
    assert K.dw_rows(a, K.DW_FWD, 1) == 0
    a.R = 1
    with pytest.raises(ValueError, match="LDS"):
        K.dw_fwd(a, _stream())


# ------------------------------------------------------------------------------------------- models
def _sep_rpv(opt, device, drop=0.2, reg=None):
    kw = {} if reg is None else {"depthwise_regularizer": reg, "pointwise_regularizer": reg}
    h = inp = Input(shape=(16, 16, 3))
    h = MaxPooling2D((2, 2))(Conv2D(8, (3, 3), activation="relu", padding="same")(h))
    for c in (16, 24):
        h = MaxPooling2D((2, 2))(SeparableConv2D(c, (3, 3), activation="relu", padding="same", **kw)(h))
    h = Dropout(drop)(h)
    h = Dropout(drop)(Dense(16, activation="relu")(Flatten()(h)))
    m = Model(inp, Dense(1, activation="sigmoid")(h), device=device)
    m.compile(optimizer=opt, loss="binary_crossentropy", metrics=["accuracy"])
    return m


def _sep_odd(opt, device, drop=0.2, reg=None):
    h = inp = Input(shape=(13, 11, 2))
    h = Conv2D(5, (3, 3), activation="relu")(h)
    h = Dropout(drop)(SeparableConv2D(12, (3, 3), strides=2, padding="same", activation="relu")(h))
    h = DepthwiseConv2D((3, 3), activation="relu")(h)
    h = Dropout(drop)(Dense(9, activation="relu")(Flatten()(h)))
    m = Model(inp, Dense(3, activation="softmax")(h), device=device)
    m.compile(optimizer=opt, loss="categorical_crossentropy", metrics=["accuracy"])
    return m


def _sep_first(opt, device, drop=0.2, reg=None):
    h = inp = Input(shape=(12, 12, 3))
    h = MaxPooling2D((2, 2))(SeparableConv2D(8, (5, 5), padding="same", activation="relu")(h))
    h = Dropout(drop)(Conv2D(8, (3, 3), activation="relu")(h))
    m = Model(inp, Dense(1, activation="sigmoid")(Flatten()(h)), device=device)
    m.compile(optimizer=opt, loss="binary_crossentropy", metrics=["accuracy"])
    return m


def _dw_tanh(opt, device, drop=0.2, reg=None):
    """A DepthwiseConv2D with a table activation (act_fwd / act_bwd behind dw_fwd), as the layer's own
    activation and as an Activation layer."""
    from cori_intml_examples_amd.models import Activation
    h = inp = Input(shape=(10, 9, 2))
    h = Dropout(drop)(Conv2D(6, (3, 3), activation="relu", padding="same")(h))
    h = DepthwiseConv2D((3, 3), padding="same", activation="tanh")(h)
    h = Activation("elu")(DepthwiseConv2D((3, 3), strides=2)(h))
    m = Model(inp, Dense(1, activation="sigmoid")(Flatten()(h)), device=device)
    m.compile(optimizer=opt, loss="binary_crossentropy", metrics=["accuracy"])
    return m


MODELS = {"rpv": _sep_rpv, "odd": _sep_odd, "first": _sep_first, "dw_tanh": _dw_tanh}
OPTS = {"Adam": optim.Adam, "AMSGrad": lambda: optim.Adam(amsgrad=True), "SGDm": lambda: optim.SGD(lr=0.01, momentum=0.9),
        "clip": lambda: optim.Adam(clipnorm=0.5)}


def _pair(kind, opt, **kw):
    out = []
    for dev in ("cuda", "cpu"):
        set_random_seed(1234)
        out.append(MODELS[kind](opt(), dev, **kw))
    for a, b in zip(out[0].get_weights(), out[1].get_weights()):
        np.testing.assert_array_equal(a, b)
    return out


def _names(m, bs, mode="train"):
    return [l.name for l in m._executor._plans[(bs, mode)].launches]


@pytest.mark.parametrize("kind,opt", [("rpv", "Adam"), ("odd", "Adam"), ("first", "Adam"), ("dw_tanh", "Adam"), ("odd", "SGDm"),
                                      ("first", "AMSGrad"), ("rpv", "clip")])
def test_three_steps_track_the_cpu_reference(kind, opt):
    """Relative L2 error of all weights <= 1e-2 after three steps over batches of 6, 6 and a ragged 4,
    dropout 0.2, fp32 CPU executor ("clip": clipnorm, and l2 on the depthwise and pointwise kernels)."""
    from cori_intml_examples_amd import regularizers
    g, c = _pair(kind, OPTS[opt], **({"reg": regularizers.l2(1e-3)} if opt == "clip" else {}))
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
    print("%s %s: rel err %.3g, moved %.3g" % (kind, opt, _rel(wg, wc), _rel(wg, w0)))
    assert _rel(wg, wc) <= 1e-2 and _rel(wg, w0) > 1e-4
    names = _names(g, 6)
    ndw = len([s for s in g._executor.plan.convs if s.depthwise])
    assert ndw and len([nm for nm in names if nm.startswith("dw_fwd")]) == ndw
    assert len([nm for nm in names if nm.startswith("dw_wgrad")]) == ndw and "conv_stack_fwd" not in names
    assert ("dw_dgrad0" in names) is False
    nact = len([s for s in g._executor.plan.convs if s.depthwise and s.act])
    assert len([nm for nm in names if nm.startswith("act_fwd_c")]) == len([nm for nm in names if nm.startswith("act_bwd_c")]) == nact
    assert nact == (2 if kind == "dw_tanh" else 0)


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
    pg, pc = g.predict(x, batch_size=8), c.predict(x, batch_size=8)
    assert pg.shape == pc.shape and np.abs(pg - pc).max() < 2e-2
    eg, ec = g.evaluate(x, y, batch_size=8, verbose=0), c.evaluate(x, y, batch_size=8, verbose=0)
    assert abs(eg[0] - ec[0]) < 2e-2 * max(1, ec[0])
    for p in g._executor._plans.values():
        assert not [l.name for l in p.launches if "dw_wgrad" in l.name or "dw_dgrad" in l.name]


def test_graph_of_8_steps_equals_8_single_steps():
    res = []
    for chunks in ([1] * 8, [8]):
        set_random_seed(21)
        m = _sep_rpv(optim.Adam(decay=0.01), "cuda")
        x, y = _data(m, 64, seed=4)
        ex = m._executor
        d = ex.upload(x, y)
        perm = torch.randperm(d.n, generator=torch.Generator().manual_seed(3)).to(ex.device)
        pos = 0
        for k in chunks:
            ex.train_steps(d, perm, pos, 8, k)
            pos += 8 * k
        torch.cuda.synchronize()
        n = m.store.numel
        res.append([m.store.master[:n].clone(), m.store.grad[:n].clone()] + [s.clone() for s in ex.optimizer_state()])
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_gpu_checkpoint_loads_on_cpu(tmp_path):
    from cori_intml_examples_amd.io.keras_h5 import load_model
    set_random_seed(5)
    g = _sep_odd(optim.Adam(), "cuda")
    x, y = _data(g, 12, seed=6)
    g.train_on_batch(x, y)
    path = str(tmp_path / "sep.h5")
    g.save(path)
    c = load_model(path)
    assert [type(l).__name__ for l in c.layers] == [type(l).__name__ for l in g.layers]
    for a, b in zip(g.get_weights(), c.get_weights()):
        np.testing.assert_array_equal(a, b)
    assert np.abs(g.predict(x, batch_size=12) - c.predict(x, batch_size=12)).max() < 2e-2


def test_data_parallel_step_at_one_rank(tmp_path):
    """tests/sep_dp_worker_gpu.py: the data-parallel step of a separable model at one rank trains bit for bit
    as the single-GPU step, captured and segmented, on the RCCL plane."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "dp.json"
    env = dict(os.environ, PYTHONPATH=root)
    for k in ("WORLD_SIZE", "RANK", "INTML_DP_BACKEND", "INTML_COMM", "INTML_XGMI", "INTML_TUNE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "sep_dp_worker_gpu.py"), str(out)],
                       env=env, capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rep = json.load(open(out))
    print(json.dumps(rep, indent=1))
    assert rep["native"] and rep["moved"] > 1e-4, rep
    dws = [n for n in rep["base_launches"] if n.startswith("dw_")]
    assert dws == ["dw_fwd1", "dw_fwd3", "dw_wgrad3", "dw_dgrad3", "dw_wgrad1", "dw_dgrad1"]
    assert "xgmi" in rep["forced_xgmi_error"] and "separable_conv2d" in rep["forced_xgmi_error"]
    for mode in ("captured", "segmented"):
        c = rep[mode]
        assert c["reducer"] == "NativeGradReducer" and c["plane"] == "rccl", c
        assert c["comm_in_graph"] == (mode == "captured") and [n for n in c["launches"] if n.startswith("dw_")] == dws
        assert c["iterations"] == 4 and all(c["identical"]), (mode, c)


def test_default_models_record_the_launches_they_recorded(monkeypatch):
    """The default RPV and MNIST models' training launch lists at batch 128, as the commit before this
    feature records them (tests/test_pooling_gpu.py RPV_TRAIN / MNIST_TRAIN pin the same lists)."""
    from cori_intml_examples_amd.apps import zoo
    monkeypatch.delenv("INTML_TUNE", raising=False)
    want = {"rpv": ["conv_stack_fwd", "dense_fwd0", "head", "dense_bwd0", "wgrad_dgrad_conv2", "wgrad_dgrad_conv1",
                    "wgrad_conv0", "reduce_b0"],
            "mnist": ["conv_stack_fwd", "dense_fwd0", "head", "dense_bwd0", "wgrad_dgrad_conv1", "wgrad_conv0",
                      "reduce_b0"]}
    set_random_seed(1)
    models = {"rpv": zoo.rpv_cnn((64, 64, 3), conv_sizes=[16, 32, 64], fc_sizes=[128], dropout=0.2, optimizer="Adam",
                                 lr=1e-3, device="cuda"),
              "mnist": zoo.mnist_cnn(32, 64, 128, dropout=0.4, optimizer="Adam", lr=1e-3, device="cuda")}
    for k, m in models.items():
        x, y = _data(m, 128)
        m.train_on_batch(x, y)
        assert _names(m, 128) == want[k], (k, _names(m, 128))

"""Dilated Conv2D on the GPU: the three dilated.hip kernels alone against a float64 NumPy oracle written
as the plain loops of their formulas (exact on small-integer inputs; NaN-filled buffers with guard
regions; a second launch bit-identical), the launchers' checks, and whole models against the CPU
executor with the project's existing bounds."""
import numpy as np
import pytest
import torch

from cori_intml_examples_amd import Conv2D, Dense, Dropout, Flatten, Input, MaxPooling2D, Model, optim, regularizers
from cori_intml_examples_amd.apps import zoo
from cori_intml_examples_amd.models.lds_layout import conv_layout
from cori_intml_examples_amd.ops.reference import conv_out_size, conv_pads
from cori_intml_examples_amd.utils import set_random_seed

from test_hip_model import _data, _rel
from test_separable_gpu import Buf, _K, _bf16, _names, _pad, _stream, _twice, _ulp

pytestmark = pytest.mark.gpu

# (Cin, Cout, H, W, KH, KW, d, padding, B, want, kc): ``want`` workgroups asked of dil_cfg (2 * B: two row blocks
# on the 11-row grid, 6 + 5 rows); kc: 0, or the k-steps of weights per chunk (2 of 12: six chunks).  Borders: Cs 4
# input, partial / one / 1.5 n-tiles, 2x2 asymmetric same, 1x3, an effective kernel larger than the image, m-tiles
# wrapping across rows, a short last row block, 320 pixels (a second pass of m-tiles), 23 (tap, c) m-tiles (two
# wgrad m groups), an LDS stage of more than 64 KB (the last case: d = 8).
CASES = [(3, 5, 11, 9, 3, 3, 2, "same", 1, 1, 0), (8, 16, 11, 9, 3, 3, 2, "valid", 3, 6, 0),
         (40, 24, 11, 9, 3, 3, 2, "same", 1, 1, 0), (8, 5, 11, 9, 2, 2, 3, "same", 3, 1, 0),
         (3, 16, 4, 5, 3, 3, 3, "same", 1, 1, 0), (40, 16, 11, 9, 1, 3, 2, "valid", 1, 1, 0),
         (8, 24, 4, 5, 2, 2, 2, "valid", 3, 1, 0), (40, 24, 11, 9, 3, 3, 2, "same", 1, 2, 2),
         (8, 16, 11, 9, 3, 3, 3, "same", 1, 1, 0), (8, 5, 20, 16, 3, 3, 2, "same", 1, 1, 0),
         (64, 8, 6, 40, 3, 3, 8, "same", 1, 1, 0)]


def _geo(case):
    Cin, Cout, H, W, KH, KW, d, padding = case[:8]
    pt, _, pl, _ = conv_pads(H, W, KH, KW, 1, padding, d)
    return (4 if Cin <= 4 else -(-Cin // 8) * 8, -(-Cout // 8) * 8, conv_out_size(H, KH, 1, padding, d),
            conv_out_size(W, KW, 1, padding, d), pt, pl)


def _args(K, kind, case):
    Cin, Cout, H, W, KH, KW, d, padding, B, want, kc = case
    a = K.DilArgs()
    a.Cs_in, a.Cs_out, a.Ho, a.Wo, a.pad_t, a.pad_l = _geo(case)
    a.B, a.H, a.W, a.Cin, a.Cout, a.KH, a.KW, a.dil = B, H, W, Cin, Cout, KH, KW, d
    ck, wr = (a.Cs_out, W) if kind == K.DIL_DGRAD else (a.Cs_in, a.Wo)
    a.ntw = K.dil_ntw(Cin if kind == K.DIL_DGRAD else Cout, kind)
    a.xpix = conv_layout(ck, wr + (KW - 1) * d, wr, False, KH, KW)
    a.R, a.kc = K.dil_cfg(a, kind, want)
    assert a.R >= 1 and (kind != K.DIL_FWD or want <= B or a.R < a.Ho)
    assert kind == K.DIL_DGRAD or (K.dil_lds_bytes(a, kind, a.R, a.kc) > 65536) == (d == 8)
    if kc and kind != K.DIL_WGRAD:
        assert kc < a.kc
        a.kc = kc
    return a


def _oracle(x, w, b, dt, case):
    """(z, dx, dW, db) and the sums of |terms| of z, dx, dW by the formulas, in float64."""
    Cin, Cout, H, W, KH, KW, d, padding, B = case[:9]
    _, _, Ho, Wo, pt, pl = _geo(case)
    z, zm = np.zeros((B, Ho, Wo, Cout)) + b, np.zeros((B, Ho, Wo, Cout)) + np.abs(b)
    dx, dxm = np.zeros((B, H, W, Cin)), np.zeros((B, H, W, Cin))
    dw, dwm = np.zeros((KH, KW, Cin, Cout)), np.zeros((KH, KW, Cin, Cout))
    for oy in range(Ho):
        for ox in range(Wo):
            for ky in range(KH):
                for kx in range(KW):
                    iy, ix = oy + ky * d - pt, ox + kx * d - pl
                    if 0 <= iy < H and 0 <= ix < W:
                        z[:, oy, ox] += x[:, iy, ix] @ w[ky, kx]
                        zm[:, oy, ox] += np.abs(x[:, iy, ix]) @ np.abs(w[ky, kx])
                        dx[:, iy, ix] += dt[:, oy, ox] @ w[ky, kx].T
                        dxm[:, iy, ix] += np.abs(dt[:, oy, ox]) @ np.abs(w[ky, kx]).T
                        dw[ky, kx] += x[:, iy, ix].T @ dt[:, oy, ox]
                        dwm[ky, kx] += np.abs(x[:, iy, ix]).T @ np.abs(dt[:, oy, ox])
    return z, dx, dw, dt.sum((0, 1, 2)), zm, dxm, dwm


def _inputs(case, ints, seed=0):
    """x, w, b, dt, the feeding stage's saved output: small integers (sparse weights and gradients, so that
    every oracle value stays an exactly representable integer), or bf16-rounded normal draws."""
    Cin, Cout, H, W, KH, KW, d, padding, B = case[:9]
    _, _, Ho, Wo, _, _ = _geo(case)
    rs = np.random.RandomState(seed)
    if ints:
        draw = lambda shape, p: rs.randint(-2, 3, shape) * (rs.rand(*shape) < p)
        return (draw((B, H, W, Cin), 1.0), draw((KH, KW, Cin, Cout), 0.3), draw((Cout,), 1.0), draw((B, Ho, Wo, Cout), 0.3),
                draw((B, H, W, Cin), 1.0))
    return tuple(_bf16(rs.randn(*s)) for s in ((B, H, W, Cin), (KH, KW, Cin, Cout), (Cout,), (B, Ho, Wo, Cout))) + (
        rs.randint(-2, 3, (B, H, W, Cin)),)


def _run(case, ints, relu=False, prev="identity", seed=0):
    """Launch dil_fwd, dil_wgrad and (Cin > 4) dil_dgrad of ``case``: {name: (got, want, sum of |terms|, terms)}."""
    K = _K()
    Cin, Cout, H, W, KH, KW, d, padding, B = case[:9]
    x, w, b, dt, prev_out = _inputs(case, ints, seed)
    z, dx, dw, db, zm, dxm, dwm = _oracle(x, w, b, dt, case)
    if ints:
        assert max(np.abs(z).max(), np.abs(dx).max()) <= 256 and max(np.abs(dw).max(), np.abs(db).max()) < 2 ** 24
    f = _args(K, K.DIL_FWD, case)
    xb, wb, bb = Buf((B, H, W, f.Cs_in), torch.bfloat16, _pad(x, f.Cs_in)), Buf(w.shape, torch.float32, w), Buf((Cout,), torch.float32, b)
    ob, db_ = Buf((B, f.Ho, f.Wo, f.Cs_out), torch.bfloat16), Buf((B, f.Ho, f.Wo, f.Cs_out), torch.bfloat16, _pad(dt, f.Cs_out))
    f.x, f.w, f.bias, f.out, f.relu = xb.ptr, wb.ptr, bb.ptr, ob.ptr, int(relu)
    res, launches, outs = {}, [lambda: K.dil_fwd(f, _stream())], [ob]
    g = _args(K, K.DIL_WGRAD, case)
    npairs = B * -(-g.Ho // g.R)
    g.pairs_per_slab = 2 if npairs > 2 else 1
    g.S = -(-npairs // g.pairs_per_slab)
    boff = (w.size + 3) // 4 * 4
    g.slab_ld, g.has_bias = boff + Cout + 3, 1
    sb = Buf((g.S, g.slab_ld), torch.float32)
    g.x, g.dt, g.w, g.slab = xb.ptr, db_.ptr, wb.ptr, sb.ptr
    launches.append(lambda: K.dil_wgrad(g, _stream()))
    outs.append(sb)
    if Cin > 4:
        a = _args(K, K.DIL_DGRAD, case)
        pb, gb = Buf((B, H, W, a.Cs_in), torch.bfloat16, _pad(prev_out, a.Cs_in)), Buf((B, H, W, a.Cs_in), torch.bfloat16)
        codes = torch.zeros(B * H * W * a.Cs_in, dtype=torch.uint8, device="cuda")      # (no kernel here reads them)
        bt = K.BwdThrough()
        bt.prev_out, bt.dy, bt.prev_relu = pb.ptr, gb.ptr, int(prev != "identity")
        bt.pH, bt.pW, bt.pC, bt.pCs, bt.cH, bt.cW = H, W, Cin, a.Cs_in, H, W
        if prev == "pool":      # a max-pooled feeding stage: the gradient at pooled resolution, its relu mask from the pooled output
            bt.prev_pool, bt.prev_code, bt.cH, bt.cW = 1, codes.data_ptr(), 2 * H, 2 * W
        a.dt, a.w, a.bt = db_.ptr, wb.ptr, bt
        launches.append(lambda: K.dil_dgrad(a, _stream()))
        outs.append(gb)
    for fn in launches:
        fn()
    torch.cuda.synchronize()
    got = [o.get() for o in outs]
    for fn in launches:
        _twice(fn, outs)
    n = KH * KW * Cin
    assert np.all(got[0][..., Cout:] == 0.0), "padding channels"
    res["out"] = (got[0][..., :Cout], np.maximum(z, 0.0) if relu else z, zm, n + 1)
    used = np.zeros(g.slab_ld, bool)
    used[:w.size] = used[boff:boff + Cout] = True
    assert np.isnan(got[1][:, ~used]).all() and not np.isnan(got[1][:, used]).any()
    slab = np.where(used, got[1], 0.0).sum(0)
    npx = B * g.Ho * g.Wo + g.S           # the kernel's chain, then this sum over the slabs
    res["dW"] = (slab[:w.size].reshape(w.shape), dw, dwm, npx)
    res["db"] = (slab[boff:boff + Cout], db, np.abs(dt).sum((0, 1, 2)), npx)
    if Cin > 4:
        assert np.all(got[2][..., Cin:] == 0.0), "padding channels"
        res["dx"] = (got[2][..., :Cin], dx * (prev_out > 0) if prev != "identity" else dx, dxm, KH * KW * Cout)
    return res


@pytest.mark.parametrize("i", range(len(CASES)))
def test_kernels_are_exact_on_integers(i):
    """dil_fwd, dil_wgrad (dW, db) and dil_dgrad (through an identity BwdThrough, a relu mask or a max-pooled
    feeding stage, by case) equal the oracle exactly."""
    res = _run(CASES[i], True, relu=bool(i % 2), prev=("identity", "relu", "pool")[i % 3])
    assert ("dx" in res) == (CASES[i][0] > 4)
    for name, (got, want, _, _) in res.items():
        np.testing.assert_array_equal(got, want, err_msg=name)


@pytest.mark.parametrize("i", [2, 3])
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
        a = _args(K, K.DIL_FWD if kind is None else kind, CASES[1])
        a.x = a.out = a.dt = a.w = a.slab = buf.data_ptr()
        a.slab_ld, a.S, a.pairs_per_slab = 4096, 6, 1
        return a
    for field, value, match in (("Cs_in", 12, "channel stride"), ("Cs_out", 12, "channel stride"), ("dil", 1, "dilation_rate"),
                                ("stride", 2, "strides"), ("x", 0, "input pointer"), ("x", buf.data_ptr() + 2, "input pointer"),
                                ("out", 0, "output pointer"), ("w", 0, "weight pointer"), ("R", 0, "rows per block"),
                                ("kc", 0, "weight chunk"), ("ntw", 3, "n-tiles"), ("pad_t", 5, "padding")):
        a = filled()
        setattr(a, field, value)
        with pytest.raises(ValueError, match=match):
            K.dil_fwd(a, _stream())
    a = filled(K.DIL_WGRAD)
    a.S = 5
    with pytest.raises(ValueError, match="pairs"):
        K.dil_wgrad(a, _stream())
    with pytest.raises(ValueError, match="BwdThrough"):
        K.dil_dgrad(filled(K.DIL_DGRAD), _stream())
    a = filled()
    a.W = a.Wo = 8192                     # one row of this halo is 640 KB
    assert K.dil_cfg(a, K.DIL_FWD, 1)[0] == 0
    a.R = 1
    with pytest.raises(ValueError, match="LDS"):
        K.dil_fwd(a, _stream())


# ------------------------------------------------------------------------------------------- models
def _context(opt, device, reg=None, act="relu"):
    return zoo.rpv_context_cnn((16, 16, 3), dropout=0.2, optimizer=opt, lr=None, device=device, activation=act,
                               l2=1e-3 if reg else 0.0)


def _odd(opt, device, reg=None, act="relu"):
    """Odd sizes, valid padding: a dilated first layer (Cs 4), a relu / tanh dilated conv feeding an ordinary
    pooled conv."""
    kw = {"kernel_regularizer": regularizers.l2(1e-3)} if reg else {}
    h = inp = Input(shape=(19, 17, 2))
    h = Conv2D(5, (3, 3), dilation_rate=2, activation="relu", **kw)(h)
    h = Conv2D(12, (2, 2), dilation_rate=(3, 3), activation=act, **kw)(h)
    h = Dropout(0.2)(MaxPooling2D((2, 2))(Conv2D(9, (3, 3), activation="relu", padding="same", **kw)(h)))
    h = Dropout(0.2)(Dense(9, activation="relu")(Flatten()(h)))
    m = Model(inp, Dense(3, activation="softmax")(h), device=device)
    m.compile(optimizer=opt, loss="categorical_crossentropy", metrics=["accuracy"])
    return m


MODELS = {"context": _context, "odd": _odd}
OPTS = {"Adam": optim.Adam, "SGDm": lambda: optim.SGD(lr=0.01, momentum=0.9), "clip": lambda: optim.Adam(clipnorm=0.5)}


def _pair(kind, opt, **kw):
    out = []
    for dev in ("cuda", "cpu"):
        set_random_seed(1234)
        out.append(MODELS[kind](opt(), dev, **kw))
    for a, b in zip(out[0].get_weights(), out[1].get_weights()):
        np.testing.assert_array_equal(a, b)
    return out


@pytest.mark.parametrize("kind,opt,act", [("context", "Adam", "relu"), ("odd", "Adam", "relu"), ("odd", "SGDm", "relu"),
                                          ("context", "clip", "relu"), ("odd", "Adam", "tanh")])
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
    want = {"context": ["dil_fwd1", "dil_fwd2", "dil_wgrad2", "dil_dgrad2", "dil_wgrad1", "dil_dgrad1"],
            "odd": ["dil_fwd0", "dil_fwd1", "dil_wgrad1", "dil_dgrad1", "dil_wgrad0"]}[kind]
    assert [nm for nm in names if nm.startswith("dil_")] == want and names[0] == "prologue" and "conv_stack_fwd" not in names
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
    pg, pc = g.predict(x, batch_size=8), c.predict(x, batch_size=8)
    assert pg.shape == pc.shape and np.abs(pg - pc).max() < 2e-2
    eg, ec = g.evaluate(x, y, batch_size=8, verbose=0), c.evaluate(x, y, batch_size=8, verbose=0)
    assert abs(eg[0] - ec[0]) < 2e-2 * max(1, ec[0])


def test_graph_of_8_steps_equals_8_single_steps():
    res = []
    for chunks in ([1] * 8, [8]):
        set_random_seed(21)
        m = _context(optim.Adam(decay=0.01), "cuda")
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


def test_forced_xgmi_plane_is_refused():
    from cori_intml_examples_amd.parallel import dist
    m = _context(optim.Adam(), "cpu")
    names = dist.dil_layer_names(m._plan)
    assert len(names) == 2
    for plane in ("xgmi", "hybrid"):
        with pytest.raises(ValueError, match=r"dilated Conv2D layers \(%s\).*%s" % (", ".join(names), plane)):
            dist.plane_for_optimizer(plane, m.optimizer, forced=True, dil_layers=names)
    assert dist.plane_for_optimizer("xgmi", m.optimizer, forced=False, dil_layers=names) == "rccl"

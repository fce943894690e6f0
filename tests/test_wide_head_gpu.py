"""The wide output head (csrc/kernels/wide_head.hip, 17..1024 columns) on the GPU: the kernel alone on
guarded buffers against a float64 oracle written out below (h, w in {-2..2} / 2 are bf16 values; the bias
(perm(n) + 1/2) / (4 Np2) keeps every logit apart from zero and from its row's other logits by more
than the logit bound, which the test asserts: exact counts), then whole models against the CPU executor
at the project's standing bounds.  u = 2^-24; the bounds are derived where they are used."""
import numpy as np
import pytest
import torch

from cori_intml_examples_amd import optim
from cori_intml_examples_amd.utils import set_random_seed

from helpers import loss_models as LM
from test_hip_model import _rel

pytestmark = pytest.mark.gpu
U, G = 2.0 ** -24, 64          # G: guard elements on both sides of every written buffer


@pytest.fixture(autouse=True)
def _opt_in(monkeypatch):
    monkeypatch.setenv("INTML_TUNE", "wide_head=1")        # the wide head is opt-in


def _K():
    from cori_intml_examples_amd.ops import hip
    return hip.kernels()


# (M, N, K, activation code, weighted, flattened conv source of C = 3 in a stride of 8)
CASES = [(1, 17, 5, 2, 0, 0), (15, 32, 32, 1, 1, 0), (16, 33, 33, 0, 0, 0), (17, 65, 32, 2, 1, 0), (33, 100, 33, 1, 0, 0),
         (33, 1024, 5, 2, 0, 0), (17, 1024, 32, 1, 1, 0), (33, 17, 130, 2, 1, 0), (15, 32, 130, 0, 1, 0),
         (17, 33, 33, 2, 0, 1), (257, 17, 5, 1, 1, 0), (257, 33, 32, 2, 0, 0), (1, 100, 130, 0, 0, 0), (16, 17, 1030, 0, 0, 0)]


def _launch(M, N, Kd, act, weighted, flat, seed=5):
    """One training launch (probs requested too) -> the inputs, the outputs and the guard check."""
    K = _K()
    rs = np.random.RandomState(seed)
    C, Cs = (3, 8) if flat else (Kd, -(-Kd // 8) * 8)
    HW, Ks = Kd // C, Kd // C * Cs
    kp = (np.arange(Kd) // C) * Cs + np.arange(Kd) % C
    hp = np.zeros((M, Ks), np.float32)
    hp[:, kp] = rs.randint(-2, 3, (M, Kd)) / 2.0
    w = (rs.randint(-2, 3, (Kd, N)) / 2.0).astype(np.float32)
    np2 = 1 << (N - 1).bit_length()
    b = ((rs.permutation(N) + 0.5) / (4.0 * np2)).astype(np.float32)
    y = {2: np.eye(N)[rs.randint(0, N, M)], 1: rs.rand(M, N) < 0.5, 0: rs.randn(M, N)}[act].astype(np.float32)
    sw = (10.0 ** rs.uniform(-1, 1, M)).astype(np.float32)
    sw[M // 2] = 0.0
    slabs = K.wide_head_slabs(M)
    dev = lambda a, dt=torch.float32: torch.tensor(a, dtype=dt, device="cuda")
    t = dict(h=dev(hp, torch.bfloat16), w=dev(w), b=dev(b), y=dev(y), sw=dev(sw),
             st=torch.zeros(K.STEP_STATE_BYTES, dtype=torch.uint8, device="cuda"))
    full = {k: torch.full((n + 2 * G,), 7.0, dtype=dt, device="cuda") for k, n, dt in (("wslab", slabs * Kd * N, torch.float32), ("bslab", slabs * N, torch.float32),
                                                      ("probs", M * N, torch.float32), ("dy", M * Ks, torch.bfloat16))}
    bufs = {k: (v, v[G:len(v) - G]) for k, v in full.items()}          # (guarded buffer, the view the kernel gets)
    a = K.HeadArgs()
    a.h, a.w, a.bias, a.y, a.st = (t[k].data_ptr() for k in ("h", "w", "b", "y", "st"))
    a.M, a.K, a.Ks, a.N, a.flat_C, a.flat_Cs = M, Kd, Ks, N, C, Cs
    a.act, a.loss, a.training, a.inv_bs = act, {2: K.LOSS_CCE, 1: K.LOSS_BCE, 0: K.LOSS_MSE}[act], 1, 1.0 / M
    a.wslab, a.bslab, a.probs = (bufs[k][1].data_ptr() for k in ("wslab", "bslab", "probs"))
    if weighted:
        a.wb = t["sw"].data_ptr()
    bt = K.BwdThrough()
    bt.dy, bt.pH, bt.pW, bt.pC, bt.pCs = bufs["dy"][1].data_ptr(), HW, 1, C, Cs
    a.bt = bt
    K.wide_head(a, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for k, (full, _) in bufs.items():
        assert (full[:G] == 7.0).all() and (full[-G:] == 7.0).all(), (k, "guard region written")
    o = K.STEP_STATE_METRICS_OFFSET // 8
    met = t["st"].view(torch.int64)[o:o + 64].view(-1, 4).sum(0).tolist()
    out = {k: v[1].clone() for k, v in bufs.items()}
    return dict(h=hp[:, kp].astype(np.float64), w=w.astype(np.float64), b=b.astype(np.float64), y=y.astype(np.float64),
                sw=sw.astype(np.float64) if weighted else None, kp=kp, Ks=Ks, slabs=slabs, args=(a, t, bufs)), out, met


@pytest.mark.parametrize("case", CASES, ids=lambda c: "M%d-N%d-K%d-act%d-w%d-flat%d" % c)
def test_wide_head_kernel_against_the_fp64_oracle(case):
    M, N, Kd, act, weighted, flat = case
    i, out, met = _launch(*case)
    h, w, y = i["h"], i["w"], i["y"]
    z = h @ w + i["b"]
    bz = 4 * Kd * U * (np.abs(h) @ np.abs(w))                         # the logit bound
    f = np.ones(M) if i["sw"] is None else i["sw"] * M / max(np.count_nonzero(i["sw"]), 1)
    if act == 2:
        e = np.exp(z - z.max(1, keepdims=True))
        p = e / e.sum(1, keepdims=True)
        # Keras' clip of the target's probability to [eps, 1 - eps]: outside it the row has no gradient
        eps, pt = float(np.float32(1e-7)), (p * y).sum(1)
        inr = (pt >= eps) & (pt <= 1 - eps)
        loss, g = -np.log(np.clip(pt, eps, 1 - eps)), (p - y) * inr[:, None]
        bp = p * (bz + (p * bz).sum(1, keepdims=True))
        bg = bp
        top = np.sort(z, 1)[:, -2:]
        assert ((top[:, 1] - top[:, 0]) > 2 * bz.max(1)).all() and (np.abs(pt / eps - 1) > 1e-2).all() and pt.max() < 1 - 1e-6
        correct = (z.argmax(1) == y.argmax(1)).sum()
    elif act == 1:
        p = 1 / (1 + np.exp(-z))
        loss, g = (np.maximum(z, 0) - z * y + np.log1p(np.exp(-np.abs(z)))).mean(1), (p - y) / N
        bp = p * (1 - p) * bz
        bg = bp / N
        assert (np.abs(z) > bz).all() and np.abs(z).max() < 15          # no element at the rounding point or the clip
        correct = (np.rint(p) == y).sum()
    else:
        p, loss, g = z, ((z - y) ** 2).mean(1), 2 * (z - y) / N
        bp, bg, correct = bz, 2 * bz / N, 0
    dz, bdz = g * f[:, None] / M, bg * f[:, None] / M
    ep = np.abs(out["probs"].cpu().numpy().reshape(M, N) - p)
    assert (ep <= bp + 8 * U * np.abs(p)).all(), ("probs", float((ep / (bp + 8 * U * np.abs(p))).max()))
    # the loss: the logit bound to first order, 8 u relative, and the metric's fixed point (one rounding
    # to 2^-32 per tile commit)
    lb = float((f * (np.abs(g) * bz).sum(1)).sum() + 8 * U * (f * loss).sum() + -(-M // 16) * 2.0 ** -33)
    el = abs(met[0] / 2.0 ** 32 - (f * loss).sum())
    assert met[3] == 0 and met[2] == M and met[1] == correct and el <= lb, (met, correct, el, lb)
    gw = out["wslab"].cpu().numpy().astype(np.float64).reshape(i["slabs"], Kd, N).sum(0)
    gb = out["bslab"].cpu().numpy().astype(np.float64).reshape(i["slabs"], N).sum(0)
    dh = out["dy"].float().cpu().numpy().astype(np.float64).reshape(M, i["Ks"])
    # dW, db, dh: 2^-8 sum|a_i||dz_i| (one rounding of dz to bf16: 8 significant bits, unit roundoff 2^-8)
    # + the fp32 chain n u sum|.| (n = M rows, N columns).  Two terms more, each from a real rounding:
    # dz carries the logit error (bdz, first order, tiny next to 2^-8), and dh is STORED as bf16, one
    # more unit roundoff 2^-8 of the result (its bound is therefore about twice the issue's)
    rel, worst = 2.0 ** -8 + M * U, {}
    for nm, got, ref, tol in (("dW", gw, h.T @ dz, rel * (np.abs(h).T @ np.abs(dz)) + np.abs(h).T @ bdz),
                              ("db", gb, dz.sum(0), rel * np.abs(dz).sum(0) + bdz.sum(0)),
                              ("dh", dh[:, i["kp"]], dz @ w.T, (2.0 ** -8 + N * U) * (np.abs(dz) @ np.abs(w).T)
                               + bdz @ np.abs(w).T + 2.0 ** -8 * np.abs(dz @ w.T))):
        err = np.abs(got - ref)
        worst[nm] = float((err / (tol + 1e-300)).max())
        assert (err <= tol + 1e-300).all(), (nm, worst[nm])
    print(case, "fractions of the bounds: loss %.3g probs %.3g" % (el / lb, (ep / (bp + 8 * U * np.abs(p))).max()), worst)
    pad = np.ones(i["Ks"], bool)
    pad[i["kp"]] = False
    assert (dh[:, pad] == 0).all()                                        # padded channels: exact zeros
    a, t, bufs = i["args"]                                                # a second launch: bit for bit
    _K().wide_head(a, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for k in out:
        assert torch.equal(out[k], bufs[k][1]), (k, "not bit-identical")


def test_launcher_checks_and_refused_models(monkeypatch):
    K = _K()
    buf, epi = torch.zeros(4096, device="cuda"), K.DenseEpiArgs()
    epi.part = buf.data_ptr()
    for kw, msg in ((dict(N=16), "N must be in 17..1024"), (dict(N=1025), "N must be in 17..1024"), (dict(act=3), "unknown activation"),
                    (dict(loss=K.LOSS_MSE), "no instance for"), (dict(act=1), "no instance for"),
                    (dict(act=0, loss=K.LOSS_HINGE), "no instance for"), (dict(M=0), "must be positive"),
                    (dict(w=0), "null input or weight pointer"), (dict(epi=epi), "never absorbs a dense epilogue"),
                    (dict(training=1, wslab=0), "needs targets and slabs")):
        h = K.HeadArgs()
        h.h = h.w = h.y = h.wslab = buf.data_ptr()
        h.M, h.K, h.Ks, h.N, h.act, h.loss = 4, 8, 8, 20, 2, K.LOSS_CCE
        for k, v in kw.items():
            setattr(h, k, v)
        with pytest.raises(ValueError, match=msg):
            K.wide_head(h, torch.cuda.current_stream().cuda_stream)
    assert K.wide_head_slabs(16) == 1 and K.wide_head_slabs(17) == 2 and K.wide_head_slabs(4096) == 16
    with pytest.raises(NotImplementedError, match="loss hinge on a linear output layer of 40 units"):
        LM.build("tiny", None, "hinge", 40, optim.Adam(), "cuda")
    with pytest.raises(NotImplementedError, match="output layers wider than 1024 units"):
        LM.build("tiny", "softmax", "categorical_crossentropy", 1025, optim.Adam(), "cuda")
    monkeypatch.delenv("INTML_TUNE")
    with pytest.raises(NotImplementedError, match="need INTML_TUNE=wide_head=1"):
        LM.build("tiny", "softmax", "categorical_crossentropy", 40, optim.Adam(), "cuda")


# ------------------------------------------------------------------------------------ 2. whole models
MODELS = [("tiny", "softmax", "categorical_crossentropy", 40), ("tiny", "sigmoid", "binary_crossentropy", 33)]
IDS = ["softmax40", "sigmoid33"]


def _pair_after(spec, mk, n, batches, seed):
    """The GPU and the CPU model of ``spec`` after train steps over ``batches`` of the same data."""
    ms = []
    for dev in ("cuda", "cpu"):
        set_random_seed(1234)
        m = LM.build(*spec, mk(), dev, drop=0.2)
        x, y = LM.data(m, n, spec[2], seed=seed)
        d = m._executor.upload(x, y)
        w0 = m.store.master[:m.store.numel].cpu().numpy()
        for pos, bs in batches:
            m._executor.train_step(d, torch.arange(d.n, device=m._executor.device), pos, bs)
        ms.append(m)
    torch.cuda.synchronize()
    assert ms[0]._executor.wide_head
    return ms[0], ms[1], x, y, w0


@pytest.mark.parametrize("spec", MODELS, ids=IDS)
def test_three_steps_evaluate_and_predict_track_the_cpu_reference(spec):
    g, c, x, y, w0 = _pair_after(spec, optim.Adam, 16, ((0, 6), (6, 6), (12, 4)), 3)
    n = g.store.numel
    wg, wc = g.store.master[:n].cpu().numpy(), c.store.master[:n].numpy()
    assert _rel(wg, wc) <= 1e-2 and _rel(wg, w0) > 1e-4
    names = [l.name for l in g._executor._plans[(6, "train")].launches]
    assert "wide_head" in names and "dense_epi0" in names and "head" not in names and "loss_head" not in names
    eg, ec = g.evaluate(x, y, batch_size=6, verbose=0), c.evaluate(x, y, batch_size=6, verbose=0)
    assert abs(eg[0] - ec[0]) < 2e-2 * max(1.0, abs(ec[0])) and abs(eg[1] - ec[1]) <= 2.0 / 16, (eg, ec)
    assert np.abs(g.predict(x, batch_size=6) - c.predict(x, batch_size=6)).max() < 2e-2


@pytest.mark.parametrize("spec", MODELS, ids=IDS)
def test_grads_match_the_bf16_reference(spec, monkeypatch):
    monkeypatch.setenv("INTML_TUNE", "ref_bf16=1,wide_head=1")
    g, c, _, _, _ = _pair_after(spec, lambda: optim.SGD(lr=0.0), 48, ((0, 48),), 0)
    gg, cg = g.store.grad[:g.store.numel].cpu().numpy(), c.store.grad[:c.store.numel].numpy()
    for s in g.store.specs:
        a, b = gg[s.offset:s.offset + s.numel], cg[s.offset:s.offset + s.numel]
        cos = float(np.dot(a, b) / max(np.linalg.norm(a) * np.linalg.norm(b), 1e-30))
        assert _rel(a, b) <= 5e-2 and cos > 0.995, (s.name, _rel(a, b), cos)


def test_graph_replay_equals_single_steps_and_the_narrow_twin_keeps_its_head():
    res = []
    for chunks in ([1] * 8, [8]):
        set_random_seed(21)
        m = LM.build("tiny", "softmax", "categorical_crossentropy", 40, optim.Adam(), "cuda", drop=0.2)
        x, y = LM.data(m, 64, "categorical_crossentropy", seed=4)
        ex = m._executor
        d = ex.upload(x, y)
        perm, pos = torch.arange(d.n, device=ex.device), 0
        for k in chunks:
            ex.train_steps(d, perm, pos, 8, k)
            pos += 8 * k
        torch.cuda.synchronize()
        res.append((m.store.master[:m.store.numel].clone(), ex._metrics()))
    assert torch.equal(res[0][0], res[1][0]) and res[0][1] == res[1][1] and res[0][1][2] == 64
    wide = [l.name for l in ex._plans[(8, "train")].launches]
    assert "wide_head" in wide and "dense_epi0" in wide and "head" not in wide, wide
    # the softmax(10) twin records the list it recorded before this kernel existed, knob or not
    set_random_seed(21)
    t = LM.build("tiny", "softmax", "categorical_crossentropy", 10, optim.Adam(), "cuda", drop=0.2)
    t.train_on_batch(*LM.data(t, 8, "categorical_crossentropy", seed=4))
    assert [l.name for l in t._executor._plans[(8, "train")].launches] == [
        "conv_stack_fwd", "dense_fwd0", "head", "dense_bwd0", "wgrad_dgrad_conv2", "wgrad_dgrad_conv1", "wgrad_conv0", "reduce_b0"]

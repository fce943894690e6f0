"""Sample-weighted loss in the fused HIP head kernel (gfx950) against the bf16-faithful CPU
oracle (``ref_bf16=1``) and against its own variants: every head launch shape (fused
one-row-per-workgroup binary / softmax-lanes, unfused four-rows-per-workgroup sigmoid /
softmax / mse), the prologue-free and the gathered weight path, multi-step graph replay,
evaluate / validation, and switching between weighted and unweighted data sets.

Test weights: 0.25 + 3.75 * rand with every fifth entry exactly 0 (zeros in every batch)."""
import numpy as np
import pytest
import torch

from cori_intml_examples_amd import Conv2D, Dense, Dropout, Flatten, Input, MaxPooling2D, Model, Sequential
from cori_intml_examples_amd.utils import set_random_seed

pytestmark = pytest.mark.gpu


def make_weights(n, seed=0):
    w = (0.25 + 3.75 * np.random.RandomState(seed).rand(n)).astype(np.float32)
    w[::5] = 0.0
    return w


def _build(kind, device, opt="Adam", drop=0.0, cin=1, hw=16):
    # "mnist" / "rpv" / "odd": the geometries of tests/test_hip_model.py::_build
    if kind == "mnist":
        m = Sequential(device=device)
        m.add(Conv2D(8, (3, 3), activation="relu", input_shape=(hw, hw, cin)))
        m.add(Conv2D(16, (3, 3), activation="relu"))
        m.add(MaxPooling2D((2, 2)))
        m.add(Dropout(drop))
        m.add(Flatten())
        m.add(Dense(32, activation="relu"))
        m.add(Dropout(drop))
        m.add(Dense(10, activation="softmax"))
        m.compile(optimizer=opt, loss="categorical_crossentropy", metrics=["accuracy"])
        return m
    if kind == "rpv":
        inp = Input(shape=(hw, hw, cin))
        h = inp
        for c in (16, 32, 64):
            h = Conv2D(c, (3, 3), activation="relu", padding="same")(h)
            h = MaxPooling2D((2, 2))(h)
        h = Dropout(drop)(h)
        h = Flatten()(h)
        h = Dense(128, activation="relu")(h)
        h = Dropout(drop)(h)
        out = Dense(1, activation="sigmoid")(h)
        m = Model(inp, out, name="RPVClassifier", device=device)
        m.compile(optimizer=opt, loss="binary_crossentropy", metrics=["accuracy"])
        return m
    if kind == "odd":     # odd channel counts, odd pooled grid, two hidden denses
        inp = Input(shape=(hw + 3, hw + 1, cin))
        h = Conv2D(5, (3, 3), activation="relu", padding="same")(inp)
        h = MaxPooling2D((2, 2))(h)
        h = Conv2D(12, (3, 3), activation="relu")(h)
        h = MaxPooling2D((2, 2))(h)
        h = Flatten()(h)
        h = Dense(20, activation="relu")(h)
        h = Dropout(drop)(h)
        h = Dense(9, activation="relu")(h)
        out = Dense(3, activation="softmax")(h)
        m = Model(inp, out, device=device)
        m.compile(optimizer=opt, loss="categorical_crossentropy", metrics=["accuracy"])
        return m
    if kind.startswith("flat_"):
        # the head directly on the flattened conv: no hidden dense, so the head does not fuse a
        # dense epilogue and runs four rows per workgroup
        units, act, loss = {"flat_sigmoid": (1, "sigmoid", "binary_crossentropy"),
                            "flat_softmax": (3, "softmax", "categorical_crossentropy"),
                            "flat_mse": (3, None, "mse")}[kind]
        inp = Input(shape=(8, 8, 1))
        h = Conv2D(8, (3, 3), activation="relu", padding="same")(inp)
        h = MaxPooling2D((2, 2))(h)
        h = Flatten()(h)
        out = Dense(units, activation=act)(h)
        m = Model(inp, out, device=device)
        m.compile(optimizer=opt, loss=loss, metrics=["accuracy"])
        return m
    raise ValueError(kind)


def _pair(kind, **kw):
    set_random_seed(1234)
    g = _build(kind, "cuda", **kw)
    set_random_seed(1234)
    c = _build(kind, "cpu", **kw)
    assert g._seed == c._seed
    for a, b in zip(g.get_weights(), c.get_weights()):
        np.testing.assert_array_equal(a, b)
    return g, c


def _data(model, n, seed=0, regress=False):
    rs = np.random.RandomState(seed)
    x = rs.rand(n, *model.input_shape[1:]).astype(np.float32)
    x = torch.tensor(x).to(torch.bfloat16).float().numpy()    # both backends see identical inputs
    nout = model.output_shape[-1]
    if regress:
        y = rs.rand(n, nout).astype(np.float32)
    elif nout == 1:
        y = (rs.rand(n) > 0.5).astype(np.float32)
    else:
        y = np.eye(nout, dtype=np.float32)[rs.randint(0, nout, n)]
    return x, y


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-12)


def _check_step(g, c, x, y, w):
    """One weighted training step on both backends at the bounds of
    test_hip_model.py::test_grads_match_bf16_reference."""
    for m in (g, c):
        ex = m._executor
        d = ex.upload(x, y, w)
        ex.reset_metrics()
        ex.train_step(d, torch.arange(d.n, device=ex.device), 0, d.n)
    torch.cuda.synchronize()
    gg = g.store.grad[:g.store.numel].cpu().numpy()
    cg = c.store.grad[:c.store.numel].numpy()
    for s in g.store.specs:
        a, b = gg[s.offset:s.offset + s.numel], cg[s.offset:s.offset + s.numel]
        err = _rel(a, b)
        cos = float(np.dot(a, b) / max(np.linalg.norm(a) * np.linalg.norm(b), 1e-30))
        print("%s: grad rel err %.3g cos %.6f" % (s.name, err, cos))
        assert err < 5e-2 and cos > 0.995, "%s: grad rel err %.3g cos %.6f" % (s.name, err, cos)
    lg, ag, _ = g._executor.read_metrics()
    lc, ac, _ = c._executor.read_metrics()
    print("loss hip %.7g ref %.7g acc %g %g" % (lg, lc, ag, ac))
    assert abs(lg - lc) < 1e-3 * max(1.0, abs(lc)) and ag == ac, (lg, lc, ag, ac)
    return lg


@pytest.mark.parametrize("kind,drop,cin,hw,n", [("rpv", 0.3, 3, 16, 48), ("mnist", 0.4, 1, 16, 48),
                                                ("odd", 0.25, 2, 16, 48)])
def test_weighted_step_matches_bf16_reference(kind, drop, cin, hw, n, monkeypatch):
    """The fused head (binary fast path; softmax lanes) with weights: gradients, loss, acc."""
    monkeypatch.setenv("INTML_TUNE", "ref_bf16=1")
    g, c = _pair(kind, drop=drop, cin=cin, hw=hw)
    assert c._executor.emulate_bf16
    x, y = _data(g, n)
    w = make_weights(n)
    lw = _check_step(g, c, x, y, w)
    assert (n, "train", "w") in g._executor._plans and (n, "train") not in g._executor._plans
    # the weights reached the kernel: the unweighted loss of the same batch differs
    set_random_seed(1234)
    ex = _build(kind, "cuda", drop=drop, cin=cin, hw=hw)._executor
    d = ex.upload(x, y)
    ex.reset_metrics()
    ex.train_step(d, torch.arange(d.n, device=ex.device), 0, d.n)
    assert abs(ex.read_metrics()[0] - lw) > 1e-3 * max(1.0, abs(lw))


@pytest.mark.parametrize("kind", ["flat_sigmoid", "flat_softmax", "flat_mse"])
def test_weighted_unfused_head_matches_bf16_reference(kind, monkeypatch):
    """Four rows per workgroup, batch 6: one full and one 2-row workgroup; the serial sigmoid,
    the softmax lanes and the mse branch; weights gathered by the prologue."""
    monkeypatch.setenv("INTML_TUNE", "ref_bf16=1")
    g, c = _pair(kind)
    x, y = _data(g, 6, seed=2, regress=kind == "flat_mse")
    w = make_weights(6, seed=2)
    assert w[0] == 0 and w[5] == 0 and (w[1:5] > 0).all()
    _check_step(g, c, x, y, w)
    bp = g._executor._plans[(6, "train", "w")]
    assert bp.head_blocks == 2 and "prologue" in [it[0] for it in bp.launches]
    np.testing.assert_array_equal(bp.wb.cpu().numpy(), w)      # the gathered weights


def _run_steps(kind, drop, cin, hw, opt, w, n=48, bs=16, steps=3, seed=46):
    set_random_seed(seed)
    m = _build(kind, "cuda", opt=opt, drop=drop, cin=cin, hw=hw)
    x, y = _data(m, n, seed=10)
    ex = m._executor
    d = ex.upload(x, y, w)
    perm = torch.randperm(d.n, generator=torch.Generator().manual_seed(6)).to(ex.device)
    ex.reset_metrics()
    ex.train_steps(d, perm, 0, bs, steps)
    torch.cuda.synchronize()
    key = (bs, "train", "w") if w is not None else (bs, "train")
    names = [it[0] for it in ex._plans[key].launches]
    return m.store.master[:m.store.numel].clone(), ex.read_metrics(), int(m.optimizer.iterations), names


@pytest.mark.parametrize("kind,drop,cin,hw,opt", [("rpv", 0.2, 3, 16, "Adam"), ("mnist", 0.4, 1, 16, "Nadam")])
@pytest.mark.parametrize("variant", ["head_generic=1", "pro_free=0"])
def test_weighted_variants_bit_identical(kind, drop, cin, hw, opt, variant, monkeypatch):
    """The generic serial head path, and the step with a prologue launch (weights gathered
    with the targets), train bit-identically to the default with weights."""
    w = make_weights(48, seed=3)
    res = []
    for tv in ("", variant):
        monkeypatch.setenv("INTML_TUNE", tv)
        res.append(_run_steps(kind, drop, cin, hw, opt, w))
    (w1, m1, i1, n1), (w0, m0, i0, n0) = res
    if variant == "pro_free=0":
        assert "prologue" in n0
    assert torch.equal(w1, w0)
    assert m1 == m0 and i1 == i0 == 3


@pytest.mark.parametrize("kind,drop,cin,hw,opt", [("rpv", 0.2, 3, 16, "Adam"), ("mnist", 0.4, 1, 16, "Nadam")])
def test_all_ones_weights_bit_identical_to_unweighted(kind, drop, cin, hw, opt):
    a = _run_steps(kind, drop, cin, hw, opt, np.ones(48, np.float32))
    b = _run_steps(kind, drop, cin, hw, opt, None)
    assert torch.equal(a[0], b[0])
    assert a[1] == b[1] and a[2] == b[2] == 3


def test_weighted_multi_step_graph_matches_single_steps():
    """Eight steps in one graph replay == eight single steps, then the partial tail alone."""
    n, bs = 16 * 8 + 5, 16
    w = make_weights(n, seed=4)
    res = []
    for chunks in ([8], [1] * 8):
        set_random_seed(21)
        m = _build("rpv", "cuda", opt="Adam", drop=0.2, cin=3)
        x, y = _data(m, n, seed=4)
        ex = m._executor
        d = ex.upload(x, y, w)
        perm = torch.randperm(d.n, generator=torch.Generator().manual_seed(3)).to(ex.device)
        ex.reset_metrics()
        pos = 0
        for k in chunks:
            ex.train_steps(d, perm, pos, bs, k)
            pos += bs * k
        ex.train_step(d, perm, pos, n - pos)
        torch.cuda.synchronize()
        res.append((m.store.master[:m.store.numel].clone(), ex.read_metrics(), int(m.optimizer.iterations)))
    assert torch.equal(res[0][0], res[1][0])
    assert res[0][1] == res[1][1] and res[0][2] == res[1][2] == 9
    assert res[0][1][2] == n


def test_weighted_evaluate_validation_and_dataset_switch(monkeypatch):
    monkeypatch.setenv("INTML_TUNE", "ref_bf16=1")
    g, c = _pair("rpv", opt="SGD", drop=0.2, cin=3)
    x, y = _data(g, 48, seed=5)
    w, w2 = make_weights(48, seed=5), make_weights(48, seed=6)

    def close(a, b):
        print("hip", a, "ref", b)
        assert abs(a[0] - b[0]) < 1e-3 * max(1.0, abs(b[0])) and a[1] == b[1], (a, b)

    # weighted -> unweighted -> other weights -> unweighted, on the same model and batch size:
    # each data set gets its own loss (no stale weight pointer, no stale plan)
    seq = [w, None, w2, None, w]
    got = [g.evaluate(x, y, batch_size=16, verbose=0, sample_weight=s) for s in seq]
    want = [c.evaluate(x, y, batch_size=16, verbose=0, sample_weight=s) for s in seq]
    for a, b in zip(got, want):
        close(a, b)
    assert got[0] == got[4] and got[1] == got[3]
    assert len({round(v[0], 6) for v in got[:3]}) == 3
    # the same through train_on_batch / test_on_batch switches
    close(g.test_on_batch(x, y, sample_weight=w), c.test_on_batch(x, y, sample_weight=w))
    close(g.test_on_batch(x, y), c.test_on_batch(x, y))
    # fit with weighted training and validation data
    hg = g.fit(x, y, batch_size=16, epochs=1, verbose=0, shuffle=False, sample_weight=w, validation_data=(x, y, w2))
    hc = c.fit(x, y, batch_size=16, epochs=1, verbose=0, shuffle=False, sample_weight=w, validation_data=(x, y, w2))
    close((hg.history["loss"][0], hg.history["acc"][0]), (hc.history["loss"][0], hc.history["acc"][0]))
    close((hg.history["val_loss"][0], hg.history["val_acc"][0]), (hc.history["val_loss"][0], hc.history["val_acc"][0]))
    close(g.evaluate(x, y, batch_size=16, verbose=0), c.evaluate(x, y, batch_size=16, verbose=0))

"""Adagrad, Adamax and Adam(amsgrad=True) on the CPU: the reference updates against the float64
oracle of tests/helpers/optim_oracle.py, the closed-form first step, the name / config surface,
the Keras-HDF5 optimizer state, and the compiler's resource report of the optimizer kernels."""
import os
import shutil
import sys

import numpy as np
import pytest
import torch

from cori_intml_examples_amd import compat, optim
from cori_intml_examples_amd.apps import rpv, zoo
from cori_intml_examples_amd.io.datasets import synthetic_rpv
from cori_intml_examples_amd.io.h5 import H5File
from cori_intml_examples_amd.models import load_model
from cori_intml_examples_amd.ops import reference as R
from cori_intml_examples_amd.utils import set_random_seed

from helpers import optim_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, STEPS = 257, 25


def make_opt(name, **kw):
    """"Adagrad" / "Adamax" / "AMSGrad" (= Adam(amsgrad=True)) / "Adam"."""
    if name == "AMSGrad":
        return optim.Adam(amsgrad=True, **kw)
    return getattr(optim, name)(**kw)


def _grads(seed=0):
    """[STEPS][N] float64: random signs that flip from step to step, exact zeros, one element
    near 1e-20 and one near 1e4."""
    rs = np.random.RandomState(seed)
    g = rs.randn(STEPS, N) * 10.0 ** rs.uniform(-4, 0, size=(STEPS, N))
    g[:, 3] = 0.0                              # always zero: state stays zero, 0 / (0 + eps)
    g[1::2, 5] = 0.0                           # zero every other step
    g[:, 7] = np.abs(g[:, 7]) * (-1.0) ** np.arange(STEPS)   # strict sign flips
    g[:, 11] = 1e-20 * (1.0 + rs.rand(STEPS))
    g[:, 13] = 1e4 * (1.0 + rs.rand(STEPS)) * rs.choice([-1.0, 1.0], STEPS)
    return g


def _ref_step(kind, p, g, slots, t, lr):
    """ops/reference, in place on float64 tensors."""
    if kind == "adagrad":
        R.adagrad_update(p, g, slots[0], lr)
    elif kind == "adamax":
        R.adamax_update(p, g, slots[0], slots[1], t, lr)
    elif kind == "amsgrad":
        R.amsgrad_update(p, g, slots[0], slots[1], slots[2], t, lr)
    else:
        R.adam_update(p, g, slots[0], slots[1], t, lr)


@pytest.mark.parametrize("name,nslots", [("Adagrad", 1), ("Adamax", 2), ("AMSGrad", 3)])
def test_reference_matches_oracle(name, nslots):
    opt = make_opt(name, lr=0.01)
    g = _grads()
    p0 = np.random.RandomState(1).randn(N)
    p, slots = p0.copy(), [np.zeros(N) for _ in range(nslots)]
    tp = torch.tensor(p0.copy(), dtype=torch.float64)
    ts = [torch.zeros(N, dtype=torch.float64) for _ in range(nslots)]
    for t in range(1, STEPS + 1):
        p, slots = O.step(opt.kind, p, g[t - 1], slots, t, opt)
        _ref_step(opt.kind, tp, torch.tensor(g[t - 1]), ts, t, 0.01)
        np.testing.assert_allclose(tp.numpy(), p, rtol=1e-12, atol=0)
        for a, b in zip(ts, slots):
            np.testing.assert_allclose(a.numpy(), b, rtol=1e-12, atol=0)
    assert np.all(slots[0][3] == 0) and p[3] == p0[3]          # the always-zero gradient moved nothing


def test_amsgrad_keeps_its_maximum_and_differs_from_adam():
    """g = 1, 0.01, 0.01, ...: v decays after the first step, vhat must not."""
    ams, adam = make_opt("AMSGrad", lr=0.01), make_opt("Adam", lr=0.01)
    pa = torch.zeros(4, dtype=torch.float64)
    pd = torch.zeros(4, dtype=torch.float64)
    sa = [torch.zeros(4, dtype=torch.float64) for _ in range(3)]
    sd = [torch.zeros(4, dtype=torch.float64) for _ in range(2)]
    op, osl = np.zeros(4), [np.zeros(4) for _ in range(3)]
    for t in range(1, 11):
        g = np.full(4, 1.0 if t == 1 else 0.01)
        _ref_step("amsgrad", pa, torch.tensor(g), sa, t, 0.01)
        _ref_step("adam", pd, torch.tensor(g), sd, t, 0.01)
        op, osl = O.step("amsgrad", op, g, osl, t, ams)
        np.testing.assert_allclose(pa.numpy(), op, rtol=1e-12, atol=0)
        if t == 1:
            vmax = sa[2].clone()
            assert torch.equal(pa, pd)
        else:
            assert torch.equal(sa[2], vmax)                    # vhat stays at the first step's v
            assert bool((sa[1] < vmax).all())                  # ... while v itself has decayed
    # Adam divides by the decayed sqrt(v) (0.999^((t-1)/2) of AMSGrad's divisor: up to 0.45 % less
    # over 9 steps of ~4e-3 each), so it has moved strictly further -- by ~1e-4, far above float64
    assert bool((pd.abs() > pa.abs()).all()) and float((pa - pd).abs().min()) > 1e-5
    del adam


@pytest.mark.parametrize("name", ["Adagrad", "Adamax"])
def test_first_step_closed_form(name):
    """From zero state: dp = -lr * g / (|g| + eps) for both (Adamax: lr_t m = lr g, u = |g|)."""
    lr, g = 0.01, _grads(3)[0]
    opt = make_opt(name, lr=lr)
    p = torch.zeros(N, dtype=torch.float64)
    slots = [torch.zeros(N, dtype=torch.float64) for _ in range(opt.n_slots)]
    _ref_step(opt.kind, p, torch.tensor(g), slots, 1, lr)
    np.testing.assert_allclose(p.numpy(), -lr * g / (np.abs(g) + 1e-7), rtol=1e-12, atol=0)


def _tiny(opt, device="cpu"):
    return zoo.rpv_cnn((16, 16, 1), conv_sizes=[4, 8, 8], fc_sizes=[16], optimizer=opt, lr=None, dropout=0.0,
                       device=device)


def test_amsgrad_first_step_equals_adam_bitwise_in_cpu_executor():
    x, y, _ = synthetic_rpv(16, size=16, seed=1)
    w = []
    for o in (optim.Adam(lr=0.01), optim.Adam(lr=0.01, amsgrad=True)):
        set_random_seed(3)
        m = _tiny(o)
        m.train_on_batch(x, y)
        w.append(np.concatenate([a.reshape(-1) for a in m.get_weights()]))
        assert m.optimizer.iterations == 1
    np.testing.assert_array_equal(w[0], w[1])
    assert m._executor.optimizer.kind == "amsgrad" and len(m._executor.optimizer_state()) == 3
    # vhat == v after the first step
    st = m._executor.optimizer_state()
    assert torch.equal(st[1], st[2]) and float(st[2].abs().sum()) > 0


def test_names_configs_and_compat():
    a, x, s = optim.get("adagrad"), optim.get("Adamax"), optim.Adam(amsgrad=True)
    assert (type(a).__name__, a.kind, a.n_slots, a.lr.get()) == ("Adagrad", "adagrad", 1, 0.01)
    assert (type(x).__name__, x.kind, x.n_slots, x.lr.get()) == ("Adamax", "adamax", 2, 0.002)
    assert (type(s).__name__, s.kind, s.n_slots, s.amsgrad) == ("Adam", "amsgrad", 3, True)
    plain = optim.Adam()
    assert (plain.kind, plain.n_slots, plain.get_config()["amsgrad"]) == ("adam", 2, False)
    assert set(a.get_config()) == {"lr", "epsilon", "decay"}
    assert set(x.get_config()) == {"lr", "beta_1", "beta_2", "epsilon", "decay"}
    assert s.get_config()["amsgrad"] is True
    for o in (optim.Adagrad(lr=0.5, epsilon=1e-6, decay=0.01), optim.Adamax(lr=0.3, beta_1=0.8, beta_2=0.99),
              optim.Adam(lr=0.2, amsgrad=True)):
        cfg = optim.serialize(o)
        back = optim.deserialize(cfg)
        assert type(back) is type(o) and back.kind == o.kind and back.n_slots == o.n_slots
        assert back.get_config() == o.get_config() == cfg["config"]
    mods = compat._keras_modules()
    ko = mods["keras.optimizers"]
    assert ko.Adagrad is optim.Adagrad and ko.Adamax is optim.Adamax
    assert getattr(ko, "Adamax")(lr=0.1).lr.get() == 0.1       # the search spaces' getattr(optimizers, name)(lr=lr)
    assert mods["keras"].optimizers.get("Adagrad").kind == "adagrad"


def test_rpv_build_model_by_name_fits():
    x, y, _ = synthetic_rpv(64, size=16, seed=2)
    set_random_seed(4)
    m = rpv.build_model((16, 16, 1), conv_sizes=[4, 8, 8], fc_sizes=[16], optimizer="Adamax", lr=0.002,
                        device="cpu")
    assert type(m.optimizer).__name__ == "Adamax"
    w0 = [w.copy() for w in m.get_weights()]
    h = m.fit(x, y, batch_size=16, epochs=1, verbose=0)
    assert np.isfinite(h.history["loss"][0]) and m.optimizer.iterations == 4
    assert any(np.abs(a - b).max() > 0 for a, b in zip(w0, m.get_weights()))


@pytest.mark.parametrize("name", ["Adagrad", "Adamax", "AMSGrad"])
def test_checkpoint_roundtrip_and_resume(tmp_path, name):
    x, y, _ = synthetic_rpv(64, size=16, seed=1)
    m = _tiny(make_opt(name))
    m.fit(x, y, batch_size=16, epochs=1, verbose=0, shuffle=False)
    p = str(tmp_path / "m.h5")
    m.save(p)
    n = len(m.store.specs)
    with H5File(p) as f:
        wn = f.attrs("optimizer_weights")["weight_names"]
        cls = type(m.optimizer).__name__
        assert len(wn) == {"Adagrad": n, "Adamax": 1 + 2 * n, "AMSGrad": 1 + 3 * n}[name]
        assert (wn[0] == "%s/iterations:0" % cls) == (name != "Adagrad")
        slot_names = [w for w in wn if "iterations" not in w]
        assert slot_names[0] == "training/%s/Variable:0" % cls and slot_names[1] == "training/%s/Variable_1:0" % cls
        if name == "AMSGrad":
            for w, s in zip(wn[1 + 2 * n:], m.store.specs):
                assert f.shape("optimizer_weights/" + w) == tuple(s.shape)
    m2 = load_model(p)
    assert type(m2.optimizer) is type(m.optimizer) and m2.optimizer.kind == m.optimizer.kind
    assert m2.optimizer.get_config() == m.optimizer.get_config()
    assert m2.optimizer.iterations == m.optimizer.iterations == 4
    for a, b in zip(m.get_weights(), m2.get_weights()):
        np.testing.assert_array_equal(a, b)
    sa, sb = m._executor.optimizer_state(), m2._executor.optimizer_state()
    assert len(sa) == len(sb) == m.optimizer.n_slots
    for a, b in zip(sa, sb):
        assert float(a.abs().sum()) > 0
        np.testing.assert_array_equal(a.numpy(), b.numpy())
    m2._executor.seed = m._executor.seed
    m.train_on_batch(x[:16], y[:16])
    m2.train_on_batch(x[:16], y[:16])
    for a, b in zip(m.get_weights(), m2.get_weights()):
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-6)


def test_plain_adam_checkpoint_keeps_placeholder_vhats(tmp_path):
    m = _tiny(optim.Adam())
    p = str(tmp_path / "a.h5")
    m.save(p)
    n = len(m.store.specs)
    with H5File(p) as f:
        wn = f.attrs("optimizer_weights")["weight_names"]
        assert len(wn) == 1 + 3 * n
        assert all(f.shape("optimizer_weights/" + w) == (1,) for w in wn[1 + 2 * n:])


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_optimizer_kernels_no_scratch():
    """Every optim_kernel / reduce_optim_kernel instance -- the five earlier kinds and Adagrad (5),
    Adamax (6), AMSGrad (7) -- keeps its by-value arguments and state out of scratch."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_resources as KR
    rows = KR.report(os.path.join(KR.KDIR, "misc.hip"))
    names = KR.demangle([r["name"] for r in rows])
    for fam in ("optim_kernel<", "reduce_optim_kernel<"):
        got = {}
        for r, nm in zip(rows, names):
            if ("void " + fam) in nm:
                got[int(nm.split(fam)[1].split(">")[0])] = r
        assert sorted(got) == list(range(8)), (fam, sorted(got))
        for kind, r in sorted(got.items()):
            if kind >= 5:
                print("%s%d>: VGPR %d, SGPR spills %d, VGPR spills %d, scratch %d, LDS %d, occupancy %d" % (
                    fam, kind, r["vgpr"], r.get("sgpr_spill", 0), r.get("vgpr_spill", 0), r.get("scratch", 0),
                    r.get("lds", 0), r.get("occ", 0)))
            assert r.get("scratch", 0) == 0, (fam, kind, r)

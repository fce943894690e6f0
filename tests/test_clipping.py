"""Keras gradient clipping (clipnorm / clipvalue) on the CPU: the float64 oracle of
tests/helpers/clip_oracle.py against hand-computed vectors, ops.reference.clip_gradients against
it, the config surface (get_config, serialize, get, checkpoints, DistributedOptimizer), the CPU
executor's clipped steps against the oracle, and the data-parallel order (clip each rank's local
gradient, then average) at 2 gloo ranks."""
import json
import os

import numpy as np
import pytest
import torch

from cori_intml_examples_amd import optim
from cori_intml_examples_amd.apps import zoo
from cori_intml_examples_amd.io.datasets import synthetic_rpv
from cori_intml_examples_amd.io.h5 import H5File
from cori_intml_examples_amd.models import executor_ref as ER
from cori_intml_examples_amd.models import load_model
from cori_intml_examples_amd.ops import reference as R
from cori_intml_examples_amd.parallel.dist import _DistributedOptimizer
from cori_intml_examples_amd.utils import set_random_seed

from helpers import clip_oracle as C
from test_dp import _torchrun

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = {"SGD": lambda **kw: optim.SGD(lr=0.01, momentum=0.9, **kw), "Adam": optim.Adam, "Nadam": optim.Nadam,
         "Adadelta": optim.Adadelta, "Adamax": optim.Adamax, "RMSprop": optim.RMSprop, "Adagrad": optim.Adagrad,
         "AMSGrad": lambda **kw: optim.Adam(amsgrad=True, **kw)}


# ------------------------------------------------------------------------------------ 1. oracle
def test_oracle_hand_computed_vectors():
    g = np.array([3.0, -4.0])                        # norm 5
    out, info = C.clip(g, clipnorm=10.0)             # below c: unchanged
    assert info == {"norm": 5.0, "fired": False, "clamped": 0} and np.array_equal(out, g)
    out, info = C.clip(g, clipnorm=5.0)              # equal to c: n >= c fires, factor exactly 1
    assert info["fired"] and np.array_equal(out, g)
    out, info = C.clip(g, clipnorm=2.5)              # above c: scaled by 0.5
    assert info["fired"] and np.array_equal(out, [1.5, -2.0])
    out, info = C.clip(np.zeros(3), clipnorm=1.0)    # zero gradient: nothing divided, no NaN
    assert info["norm"] == 0.0 and not info["fired"] and np.array_equal(out, np.zeros(3))
    out, info = C.clip(np.array([np.nan, 1.0]), clipnorm=1.0)     # a NaN norm fails the comparison
    assert not info["fired"] and np.isnan(out[0]) and out[1] == 1.0
    # both, the order visible: norm clip first (g -> [1.5, -2.0]), then the clamp to 1.6 changes one
    # element; value-then-norm would give [1.6, -1.6] * 2.5 / sqrt(5.12) = [1.7678, -1.7678]
    out, info = C.clip(g, clipnorm=2.5, clipvalue=1.6)
    assert np.array_equal(out, [1.5, -1.6]) and info["clamped"] == 1
    wrong = np.clip(g, -1.6, 1.6)
    wrong = wrong * (2.5 / np.sqrt(np.sum(wrong * wrong)))
    assert np.abs(wrong - out).max() > 0.1
    out, info = C.clip(g, clipvalue=3.5)             # clipvalue alone
    assert np.array_equal(out, [3.0, -3.5]) and info == {"norm": None, "fired": False, "clamped": 1}
    for off in (None, 0, 0.0, -1.0):                 # off
        out, info = C.clip(g, clipnorm=off, clipvalue=off)
        assert np.array_equal(out, g) and not info["fired"] and info["clamped"] == 0


# ------------------------------------------------------------------------------------ 2. reference
@pytest.mark.parametrize("cn,cv", [(0.5, None), (None, 0.01), (0.5, 0.004), (1e30, 1e30), (None, None), (0.0, -1.0)])
def test_reference_clip_matches_oracle(cn, cv):
    rs = np.random.RandomState(2)
    g = (rs.randn(1001) * 10.0 ** rs.uniform(-4, 0, 1001)).astype(np.float32)
    want, info = C.clip(g, cn, cv)
    t = torch.tensor(g.copy())
    norm = R.clip_gradients(t, cn, cv)
    # fp32: the norm (a 1001-term sum), the quotient and the product round once each
    np.testing.assert_allclose(t.numpy(), want, rtol=1e-5, atol=0)
    if cn:
        assert abs(float(norm) - info["norm"]) <= 1e-5 * info["norm"]
    else:
        assert norm is None
    if (cn, cv) in ((1e30, 1e30), (None, None), (0.0, -1.0)):
        assert np.array_equal(t.numpy(), g)          # off / never reached: the bits are untouched
    else:
        assert info["fired"] or info["clamped"]


def test_reference_clip_zero_and_nan():
    z = torch.zeros(7)
    assert float(R.clip_gradients(z, 1.0, None)) == 0.0 and torch.equal(z, torch.zeros(7))
    t = torch.tensor([float("nan"), 2.0, -3.0])
    R.clip_gradients(t, 1.0, None)                   # NaN norm: comparison fails, g unchanged
    assert bool(torch.isnan(t[0])) and t[1] == 2.0 and t[2] == -3.0


# ------------------------------------------------------------------------------------ 3. config
def _tiny(opt, device="cpu", channels=1, dp=False):
    return zoo.rpv_cnn((16, 16, channels), conv_sizes=[4, 8, 8], fc_sizes=[16], optimizer=opt, lr=None, dropout=0.0,
                       use_horovod=dp, device=device)


def test_default_config_has_no_clip_keys():
    for name, mk in KINDS.items():
        o = mk()
        assert "clipnorm" not in o.get_config() and "clipvalue" not in o.get_config(), name
        assert not o.clips
    assert optim.Adam().get_config() == {"lr": 0.001, "decay": 0.0, "beta_1": 0.9, "beta_2": 0.999,
                                         "epsilon": 1e-07, "amsgrad": False}


@pytest.mark.parametrize("name", sorted(KINDS))
def test_config_round_trips(name):
    o = KINDS[name](clipnorm=1.0, clipvalue=0.5)
    cfg = o.get_config()
    assert cfg["clipnorm"] == 1.0 and cfg["clipvalue"] == 0.5 and o.clips
    ser = optim.serialize(o)
    for back in (optim.deserialize(ser), optim.get(ser), type(o).from_config(cfg)):
        assert type(back) is type(o) and back.kind == o.kind
        assert back.get_config() == cfg and back.clipnorm == 1.0 and back.clipvalue == 0.5 and back.clips
    only = KINDS[name](clipnorm=2.0)                 # only the given argument is kept
    assert only.get_config()["clipnorm"] == 2.0 and "clipvalue" not in only.get_config()
    for off in (0.0, -1.0, None):                    # <= 0 / None: kept in the config, but off
        o = KINDS[name](clipnorm=off)
        assert not o.clips and o.get_config()["clipnorm"] == off


def test_distributed_optimizer_exposes_the_values():
    # (the wrapper class itself: hvd.DistributedOptimizer would start a process group here; the
    # 2-rank worker below checks the real one)
    d = _DistributedOptimizer(optim.Adam(clipnorm=1.0, clipvalue=0.5))
    assert d.clipnorm == 1.0 and d.clipvalue == 0.5 and d.clips
    assert d.get_config()["clipnorm"] == 1.0 and d.get_config()["clipvalue"] == 0.5
    assert optim.serialize(d)["config"]["clipnorm"] == 1.0
    plain = _DistributedOptimizer(optim.Adam())
    assert not plain.clips and "clipnorm" not in plain.get_config()


def test_checkpoint_keeps_clipping_and_resumes_identically(tmp_path):
    x, y, _ = synthetic_rpv(96, size=16, seed=1)
    set_random_seed(3)
    m = _tiny(optim.Adam(lr=0.01, clipnorm=0.05, clipvalue=0.004))
    m.fit(x[:64], y[:64], batch_size=16, epochs=1, verbose=0, shuffle=False)
    p = str(tmp_path / "c.h5")
    m.save(p)
    with H5File(p) as f:
        tc = json.loads(f.attrs("/")["training_config"])
    oc = tc["optimizer_config"]
    assert oc["class_name"] == "Adam" and oc["config"]["clipnorm"] == 0.05 and oc["config"]["clipvalue"] == 0.004
    m2 = load_model(p)
    assert m2.optimizer.get_config() == m.optimizer.get_config()
    assert m2.optimizer.clipnorm == 0.05 and m2.optimizer.clipvalue == 0.004 and m2.optimizer.clips
    m2._executor.seed = m._executor.seed
    for i in range(2):                               # the loaded model continues like the unsaved one
        m.train_on_batch(x[64 + 16 * i:80 + 16 * i], y[64 + 16 * i:80 + 16 * i])
        m2.train_on_batch(x[64 + 16 * i:80 + 16 * i], y[64 + 16 * i:80 + 16 * i])
    for a, b in zip(m.get_weights(), m2.get_weights()):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(m._executor.optimizer_state(), m2._executor.optimizer_state()):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------ 4.-6. CPU executor
@pytest.fixture
def unclipped(monkeypatch):
    """The gradients the CPU executor hands to clip_gradients, before it clips them in place."""
    rec = []
    orig = R.clip_gradients

    def spy(g, cn, cv):
        rec.append(g.detach().clone().double().numpy())
        return orig(g, cn, cv)
    monkeypatch.setattr(ER.R, "clip_gradients", spy)
    return rec


@pytest.mark.parametrize("name", ["SGD", "Adam", "Nadam"])
def test_cpu_executor_matches_oracle(name, unclipped):
    """3 train_on_batch steps of the tiny RPV model (16x16x3, conv [4, 8, 8], fc [16]) with
    clipnorm = 0.05, below every step's gradient norm (0.16 .. 0.2 here), so every step clips;
    master and slots against the oracle fed with the executor's own (unclipped) gradients.
    Bound: the project's 2e-5 * max(1, 100 lr)."""
    c = 0.05
    set_random_seed(5)
    opt = KINDS[name](clipnorm=c)
    m = _tiny(opt, channels=3)
    x, y, _ = synthetic_rpv(96, size=16, channels=3, seed=3)
    n = m.store.numel
    p = m.store.master[:n].double().numpy().copy()
    slots = [np.zeros(n) for _ in range(opt.n_slots)]
    bound = 2e-5 * max(1.0, 100 * float(opt.lr))
    for t in range(1, 4):
        m.train_on_batch(x[32 * (t - 1):32 * t], y[32 * (t - 1):32 * t])
        assert len(unclipped) == t
        p, slots, info = C.step(opt.kind, p, unclipped[-1], slots, t, opt, clipnorm=c)
        assert info["fired"] and info["norm"] > 2 * c, (t, info)          # every step clips
        # what the update consumed (store.grad: the CPU executor clips in place) has norm c
        assert abs(C.global_norm(m.store.grad[:n].double().numpy()) - c) < 1e-6 * c
        errs = [float(np.abs(m.store.master[:n].double().numpy() - p).max())]
        errs += [float(np.abs(s.double().numpy() - r).max()) for s, r in zip(m._executor.optimizer_state(), slots)]
        print("%s step %d: norm %.4f, max |err| %s (bound %.3g)" % (name, t, info["norm"], errs, bound))
        assert max(errs) < bound, (name, t, errs)


@pytest.mark.parametrize("name", ["SGD", "Adam", "Adadelta"])
def test_huge_clipnorm_is_bit_identical_to_no_clipping(name):
    x, y, _ = synthetic_rpv(64, size=16, channels=3, seed=3)
    res = []
    for kw in ({}, {"clipnorm": 1e30}, {"clipnorm": 1e30, "clipvalue": 1e30}):
        set_random_seed(5)
        m = _tiny(KINDS[name](**kw), channels=3)
        for t in range(4):
            m.train_on_batch(x[16 * t:16 * t + 16], y[16 * t:16 * t + 16])
        res.append([m.store.master[:m.store.numel].clone()] + [s.clone() for s in m._executor.optimizer_state()])
    for other in res[1:]:
        for a, b in zip(res[0], other):
            assert torch.equal(a, b)


@pytest.mark.parametrize("name", sorted(KINDS))
def test_all_zero_sample_weights(name):
    """An all-zero sample_weight batch: a zero gradient, norm 0 -- nothing divided, no NaN."""
    x, y, _ = synthetic_rpv(16, size=16, channels=3, seed=3)
    set_random_seed(5)
    opt = KINDS[name](clipnorm=1.0) if name != "SGD" else optim.SGD(lr=0.01, clipnorm=1.0)
    m = _tiny(opt, channels=3)
    w0 = [w.copy() for w in m.get_weights()]
    m.train_on_batch(x, y, sample_weight=np.zeros(16, dtype=np.float32))
    assert all(np.all(np.isfinite(w)) for w in m.get_weights())
    assert all(bool(torch.isfinite(s).all()) for s in m._executor.optimizer_state())
    if name == "SGD":
        for a, b in zip(w0, m.get_weights()):
            np.testing.assert_array_equal(a, b)


# ------------------------------------------------------------------------------------ 7. data parallel
def test_two_ranks_clip_locally_then_average(tmp_path):
    """Exactly one rank's local norm exceeds clipnorm; the step must equal "clip each local
    gradient, then average" within the DP-vs-single bound of tests/test_dp.py (1e-5) and differ
    from "average, then clip" by more than it."""
    r = _torchrun(2, [os.path.join(ROOT, "tests", "clip_dp_worker.py"), str(tmp_path)])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    reps = [json.load(open(tmp_path / ("rank%d.json" % i))) for i in range(2)]
    print(json.dumps(reps, indent=1))
    r0 = reps[0]
    norms, c = r0["norms"], r0["clipnorm"]
    assert sum(n >= c for n in norms) == 1 and sorted(r0["fired"]) == [False, True], r0
    assert all(rep["w0_equal"] and rep["dist_clipnorm"] == c for rep in reps)
    assert reps[1]["w1_digest"] == r0["w1_digest"]
    assert r0["err_clip_then_average"] < 1e-5, r0
    assert r0["err_average_then_clip"] > 1e-5, r0

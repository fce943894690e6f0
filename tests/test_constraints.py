"""Keras weight constraints on the CPU: the module, the layers' configs, the CPU executor against float64."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cori_intml_examples_amd import constraints, optim
from cori_intml_examples_amd.models import Conv2D, Dense, load_model
from cori_intml_examples_amd.utils import set_random_seed

from helpers import con_models as M

OPTS = {"SGD": lambda: optim.SGD(lr=0.05), "Adam": lambda: optim.Adam(lr=0.001)}      # (Adam: Keras' default lr)


@pytest.mark.parametrize("make,name,cfg", [
    (lambda: constraints.MaxNorm(), "MaxNorm", {"max_value": 2.0, "axis": 0}),
    (lambda: constraints.maxnorm(0.1, axis=[0, 1, 2]), "MaxNorm", {"max_value": float(np.float32(0.1)), "axis": [0, 1, 2]}),
    (lambda: constraints.nonneg(), "NonNeg", {}),
    (lambda: constraints.unit_norm(axis=(0, 1)), "UnitNorm", {"axis": [0, 1]}),
    (lambda: constraints.min_max_norm(rate=0.5), "MinMaxNorm", {"min_value": 0.0, "max_value": 1.0, "rate": 0.5, "axis": 0}),
])
def test_configs_aliases_and_round_trips(make, name, cfg):
    c = make()
    ser = constraints.serialize(c)
    assert isinstance(c, constraints.Constraint) and ser == {"class_name": name, "config": cfg}
    assert json.loads(json.dumps(ser)) == ser
    for back in (constraints.get(ser), constraints.deserialize(ser), type(c).from_config(cfg)):
        assert back == c and back.get_config() == cfg
    assert constraints.get(c) is c and type(constraints.get(name)) is type(c) and constraints.get(None) is None


@pytest.mark.parametrize("cls,args,axis", [(Dense, (5,), 0), (Conv2D, (5, (3, 3)), [0, 1, 2]), (Conv2D, (5, (3, 3)), [-4, 1])])
def test_layer_config_round_trips_constraints(cls, args, axis):
    layer = cls(*args, name="x", kernel_constraint=constraints.MaxNorm(0.5, axis=axis), bias_constraint="non_neg")
    cfg = layer.get_config()
    assert cfg["kernel_constraint"] == {"class_name": "MaxNorm", "config": {"max_value": 0.5, "axis": axis}}
    assert cfg["bias_constraint"] == {"class_name": "NonNeg", "config": {}}
    back = cls.from_config(json.loads(json.dumps(cfg)))
    assert back.get_config() == cfg and set(back.weight_constraints()) == {"kernel", "bias"}
    assert set(cls(*args, use_bias=False, bias_constraint="non_neg").weight_constraints()) == set()


@pytest.mark.parametrize("make", [
    lambda: Conv2D(4, (3, 3), name="refused", kernel_constraint=constraints.max_norm(1, axis=3)),
    lambda: Conv2D(4, (3, 3), name="refused", kernel_constraint=constraints.unit_norm(axis=[0, 2])),
    lambda: Dense(4, name="refused", kernel_constraint=constraints.min_max_norm(axis=-1)),
    lambda: Dense(4, name="refused", bias_constraint=constraints.max_norm(1, axis=[0, 1])),
])
def test_refused_axes_name_the_layer(make):
    with pytest.raises(NotImplementedError, match="refused.*axis"):
        make()


def test_hdf5_round_trip_keeps_the_constraints(tmp_path):
    m = M.small(optim.SGD(lr=0.05))
    m.save(str(tmp_path / "con.h5"))
    back = load_model(str(tmp_path / "con.h5"))
    assert [l.get_config() for l in back.layers] == [l.get_config() for l in m.layers]
    assert back.store.constrained_tensors() == m.store.constrained_tensors() and len(m.store.constrained_tensors()) == 4


def _constrain64(w, kind, axes=1, max_value=0.5):
    if kind == "non_neg":
        return w * (w >= 0).to(w.dtype)
    n = torch.sqrt((w * w).sum(dim=tuple(range(axes)), keepdim=True))
    return w / (1e-7 + n) if kind == "unit_norm" else w * (torch.clamp(n, 0, max_value) / (1e-7 + n))


@pytest.mark.parametrize("name", sorted(OPTS))
def test_cpu_executor_matches_float64_model(name):
    """Three steps against float64 autograd + Keras update + constraint formulas; the project's CPU weight bound."""
    set_random_seed(4)
    opt = OPTS[name]()
    m = M.small(opt)
    lr, start = float(opt.lr), m.get_weights()[2].astype(np.float64)
    p = [torch.tensor(w, dtype=torch.float64, requires_grad=True) for w in m.get_weights()]
    ms, vs = [torch.zeros_like(w) for w in p], [torch.zeros_like(w) for w in p]
    for t, (x, y) in enumerate(M.batches(3), 1):
        m.train_on_batch(x, y)
        h = torch.tensor(x, dtype=torch.float64).permute(0, 3, 1, 2)
        h = F.max_pool2d(F.relu(F.conv2d(h, p[0].permute(3, 2, 0, 1), p[1], padding=1)), 2)
        h = F.relu(F.conv2d(h, p[2].permute(3, 2, 0, 1), p[3], padding=1))
        h = F.relu(h.permute(0, 2, 3, 1).reshape(len(x), -1) @ p[4] + p[5])
        loss = F.binary_cross_entropy_with_logits((h @ p[6] + p[7])[:, 0], torch.tensor(y, dtype=torch.float64))
        grads = torch.autograd.grad(loss, p)
        with torch.no_grad():
            for w, g, mm, vv in zip(p, grads, ms, vs):
                if name == "SGD":
                    w -= lr * g
                else:
                    mm.mul_(0.9).add_(0.1 * g)
                    vv.mul_(0.999).add_(0.001 * g * g)
                    w -= lr * (1 - 0.999 ** t) ** 0.5 / (1 - 0.9 ** t) * mm / (vv.sqrt() + 1e-7)
            p[0].copy_(_constrain64(p[0], "max_norm", 1))
            p[2].copy_(_constrain64(p[2], "max_norm", 3))
            p[4].copy_(_constrain64(p[4], "unit_norm", 1))
            p[5].copy_(_constrain64(p[5], "non_neg"))
        errs = [float(np.abs(a.astype(np.float64) - b.detach().numpy()).max()) for a, b in zip(m.get_weights(), p)]
        print("%s step %d: max |err| per tensor %s" % (name, t, ["%.2e" % e for e in errs]))
        assert max(errs) < 2e-5 * max(1.0, 100 * lr), (name, t, errs)
    assert np.sqrt((start ** 2).sum(axis=(0, 1, 2))).min() > 0.6      # glorot starts every filter above MaxNorm's 0.5
    M.check_constrained(m.get_weights())

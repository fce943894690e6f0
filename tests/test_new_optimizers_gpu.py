"""Adagrad, Adamax and Adam(amsgrad=True) on the GPU: the fused HIP update against the float64
oracle (tests/helpers/optim_oracle.py), optim_kernel's pack routes and tile blocks, graph replay
consistency (the Adamax scalar of the device bookkeeping), plan gating (no early reduction, no
fused dense update), the data-parallel step at one rank and a GPU -> CPU checkpoint."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cori_intml_examples_amd import optim
from cori_intml_examples_amd.apps import zoo
from cori_intml_examples_amd.io.datasets import synthetic_rpv
from cori_intml_examples_amd.io.keras_h5 import load_model
from cori_intml_examples_amd.utils import set_random_seed

from helpers import optim_oracle as O
from helpers import param_oracle as P
from test_hip_model import _build, _data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ["Adagrad", "Adamax", "AMSGrad"]
NSLOTS = {"Adagrad": 1, "Adamax": 2, "AMSGrad": 3}

pytestmark = pytest.mark.gpu


def make_opt(name, **kw):
    return optim.Adam(amsgrad=True, **kw) if name == "AMSGrad" else getattr(optim, name)(**kw)


def _tiny(opt, device="cuda", drop=0.0):
    """16x16x3, conv [4, 8, 8], fc [16]."""
    return zoo.rpv_cnn((16, 16, 3), conv_sizes=[4, 8, 8], fc_sizes=[16], dropout=drop, optimizer=opt, lr=None,
                       device=device)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("model", ["tiny", "odd"])
@pytest.mark.parametrize("name", KINDS)
def test_kernel_matches_keras_math(name, model, fused, monkeypatch):
    """3 steps at batch 32; after each, the master and every state slot against the float64
    oracle applied to the gradients read back from the device.  Bound: the project's
    2e-5 * max(1, 100 lr) (test_hip_model.py::test_optimizer_kernel_matches_keras_math).
    fused: reduce_optim_kernel<KIND> (default); else slab_reduce + optim_kernel<KIND>."""
    monkeypatch.setenv("INTML_TUNE", "" if fused else "fuse_optim=0")
    set_random_seed(5)
    opt = make_opt(name)
    m = _tiny(opt) if model == "tiny" else _build("odd", "cuda", opt=opt, cin=2, hw=16)
    ex = m._executor
    o = ex.opt
    n = m.store.numel
    x, y = _data(m, 96, seed=3)
    d = ex.upload(x, y)
    p = m.store.master[:n].cpu().double().numpy()
    slots = [np.zeros(n) for _ in range(NSLOTS[name])]
    assert len(ex.slots) == NSLOTS[name]
    bound = 2e-5 * max(1.0, 100 * float(o.lr))
    for t in range(1, 4):
        prev = [m.store.master[:n].cpu().numpy()] + [s.cpu().numpy() for s in ex.optimizer_state()]
        ex.train_step(d, torch.arange(d.n, device=ex.device), 32 * (t - 1), 32)
        torch.cuda.synchronize()
        gr = m.store.grad[:n].cpu().double().numpy()
        assert np.abs(gr).max() > 0
        p, slots = O.step(o.kind, p, gr, slots, t, o)
        got = m.store.master[:n].cpu().double().numpy()
        # per element, from the device's own state before the step: the derived bounds of
        # helpers/param_oracle.py
        ratio, _ = P.keras_step_ratio(o, t, prev[0], gr, prev[1:], got, [s.cpu().numpy() for s in ex.optimizer_state()])
        print("%s %s fused=%d step %d: worst per-element error / bound %.3f" % (name, model, fused, t, ratio))
        assert ratio <= 1.0, (name, model, fused, t, ratio)
        errs = [float(np.abs(got - p).max())] + [float(np.abs(s.cpu().double().numpy() - r).max())
                                                 for s, r in zip(ex.optimizer_state(), slots)]
        print("%s %s fused=%d step %d: max |err| master %.3g, slots %s (bound %.3g)" % (
            name, model, fused, t, errs[0], ["%.3g" % e for e in errs[1:]], bound))
        assert max(errs) < bound, (name, model, fused, t, errs)
    plan = ex._plans[(32, "train")]
    assert bool(plan.optim_fused) == fused
    # the packs mirror the master after the update
    arena = ex.arena.clone()
    ex.params_changed()
    torch.cuda.synchronize()
    assert torch.equal(arena, ex.arena)


def _route_run(name, kind, cin, use_tiles):
    """Two rounds of optim_kernel<KIND> launches over the whole parameter range; after each, the
    packs it wrote must equal a full re-pack.  Returns the master and the slots."""
    set_random_seed(45)
    m = _build(kind, "cuda", opt=make_opt(name), drop=0.0, cin=cin, hw=16)
    ex = m._executor
    assert ex.routes is not None
    n = ex.store.numel
    # this step's scalar (lr for Adagrad, the bias-corrected rates for the others), as the
    # bookkeeping would leave it
    ex._st_f32[ex.K.STEP_STATE_S_OFFSET // 4] = 1e-3
    gen = torch.Generator().manual_seed(7)
    g1 = torch.randn(ex.store.capacity, generator=gen) * 1e-2
    # round 2: a hundredth of the first gradient (AMSGrad keeps vhat, Adamax keeps beta_2 u) or
    # three times it (both take the new value), element by element
    small = torch.rand(ex.store.capacity, generator=gen) < 0.5
    g2 = g1 * torch.where(small, torch.tensor(0.01), torch.tensor(3.0))
    ranges = ((0, n),) if use_tiles else ((0, n // 3), (n // 3, n))
    for g in (g1, g2):
        ex.store.grad.copy_(g.to(ex.device))
        a = ex._optim_args(False, defer_pack=True)
        for lo, hi in ranges:
            a.lo, a.n = lo, hi - lo
            if use_tiles:
                ex.tile_routes(a)
                assert a.ntile == 1
            ex.K.optim(a, ex.pack_table, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        written = ex.arena.clone()
        ex.params_changed()
        torch.cuda.synchronize()
        assert torch.equal(written, ex.arena)
    slots = [s[:n].clone() for s in ex.slots]
    sm, g2n = small[:n].to(ex.device), g2[:n].to(ex.device)
    if name == "AMSGrad":      # the maximum decided both ways
        v, vhat = slots[1], slots[2]
        assert bool((vhat[sm] > v[sm]).all()) and bool((vhat[~sm] == v[~sm]).all())
    if name == "Adamax":
        u = slots[1]
        assert bool((u[sm] > g2n[sm].abs()).all()) and bool((u[~sm] == g2n[~sm].abs()).all())
    assert all(float(s.abs().sum()) > 0 for s in slots)
    return m.store.master[:n].clone(), slots


@pytest.mark.parametrize("kind,cin,tiled", [("odd", 2, False), ("rpv", 3, True)])
@pytest.mark.parametrize("name", KINDS)
def test_optim_kernel_pack_routes_and_tiles(name, kind, cin, tiled):
    flat = _route_run(name, kind, cin, False)
    if tiled:
        til = _route_run(name, kind, cin, True)
        assert torch.equal(flat[0], til[0])
        assert len(flat[1]) == len(til[1]) == NSLOTS[name]
        for a, b in zip(flat[1], til[1]):
            assert torch.equal(a, b)


@pytest.mark.parametrize("name", KINDS)
def test_graph_of_8_steps_equals_8_single_steps(name):
    res = []
    for chunks in ([1] * 8, [8]):
        set_random_seed(21)
        m = _tiny(make_opt(name, decay=0.01), drop=0.2)
        x, y = _data(m, 256, seed=4)
        ex = m._executor
        d = ex.upload(x, y)
        perm = torch.randperm(d.n, generator=torch.Generator().manual_seed(3)).to(ex.device)
        pos = 0
        for k in chunks:
            ex.train_steps(d, perm, pos, 32, k)
            pos += 32 * k
        torch.cuda.synchronize()
        n = m.store.numel
        res.append(([m.store.master[:n].clone()] + [s.clone() for s in ex.optimizer_state()],
                    int(ex._st_i32[0]), int(m.optimizer.iterations)))
    assert len(res[0][0]) == 1 + NSLOTS[name]
    for a, b in zip(res[0][0], res[1][0]):
        assert torch.equal(a, b)
    assert res[0][1] == res[1][1] == res[0][2] == res[1][2] == 8


def _plan_of(opt, tv, monkeypatch):
    monkeypatch.setenv("INTML_TUNE", tv)
    set_random_seed(57)
    m = _build("rpv_bench", "cuda", opt=opt, drop=0.2, cin=3, hw=64)
    x, y = _data(m, 128, seed=21)
    ex = m._executor
    d = ex.upload(x, y)
    ex.train_steps(d, torch.arange(d.n, device=ex.device), 0, 128, 1)
    torch.cuda.synchronize()
    assert np.isfinite(m.store.master[:m.store.numel].sum().item())
    return ex._plans[(128, "train")]


@pytest.mark.parametrize("name", KINDS)
def test_plan_has_no_early_reduction_and_no_fused_dense_update(name, monkeypatch):
    for tv in ("", "dense_opt=1"):
        plan = _plan_of(make_opt(name), tv, monkeypatch)
        assert plan.early_red == {} and plan.dense_fused_opt == [] and not plan.dense_opt_ok
        assert plan.optim_fused          # one reduce_optim_kernel<KIND> launch at the end of the step


def test_plan_of_adam_keeps_its_early_reduction(monkeypatch):
    plan = _plan_of("Adam", "", monkeypatch)
    assert plan.early_red and plan.optim_fused


def test_data_parallel_step_at_one_rank(tmp_path):
    out = tmp_path / "dp.json"
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("WORLD_SIZE", "RANK", "INTML_DP_BACKEND", "INTML_COMM", "INTML_XGMI", "INTML_TUNE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "optim_dp_worker_gpu.py"), str(out)],
                       env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rep = json.load(open(out))
    print(json.dumps(rep, indent=1))
    assert rep["native"], rep
    for name in KINDS:
        k = rep[name]
        assert k["n_state"] == NSLOTS[name] and k["moved"] > 1e-4 and k["base_fused"], k
        for mode in ("captured", "segmented"):
            c = k[mode]
            assert c["reducer"] == "NativeGradReducer" and c["plane"] == "rccl" and not c["xgmi"], c
            assert c["comm_in_graph"] == (mode == "captured") and c["early_red"] == 0, c
            assert not [nm for nm in c["launches"] if "xgmi" in nm or "xchg" in nm], c
            assert c["iterations"] == 4 and all(c["identical"]), (name, mode, c)
        assert "optim_b0" in k["captured"]["launches"], k
        for plane in ("xgmi", "hybrid"):
            msg = k["forced_" + plane]
            assert ("Adam(amsgrad=True)" if name == "AMSGrad" else name) in msg and repr(plane) in msg, k
    assert rep["history_data_plane"].startswith("NativeGradReducer:rccl"), rep["history_data_plane"]


@pytest.mark.parametrize("name", KINDS)
def test_gpu_checkpoint_loads_on_cpu(tmp_path, name):
    x, y, _ = synthetic_rpv(64, channels=3, size=16, seed=1)
    set_random_seed(8)
    m = _tiny(make_opt(name))
    m.fit(x, y, batch_size=16, epochs=1, verbose=0, shuffle=False)
    p = str(tmp_path / "g.h5")
    m.save(p)
    c = load_model(p, device="cpu")
    assert c.store.master.device.type == "cpu" and c.optimizer.kind == m.optimizer.kind
    assert c.optimizer.iterations == m.optimizer.iterations == 4
    for a, b in zip(m.get_weights(), c.get_weights()):
        np.testing.assert_array_equal(a, b)
    sg, sc = m._executor.optimizer_state(), c._executor.optimizer_state()
    assert len(sg) == len(sc) == NSLOTS[name]
    for a, b in zip(sg, sc):
        assert float(b.abs().sum()) > 0
        np.testing.assert_array_equal(a.cpu().numpy(), b.numpy())

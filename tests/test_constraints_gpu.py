"""Keras weight constraints on the GPU: constraint.hip alone against float64, the small model, the launch lists."""
import numpy as np
import pytest
import torch

from cori_intml_examples_amd import optim
from cori_intml_examples_amd.io.keras_h5 import load_model
from cori_intml_examples_amd.utils import set_random_seed

from helpers import con_models as M

pytestmark = pytest.mark.gpu

MAXN, NONNEG, UNIT, MINMAX = 0, 1, 2, 3
PARAMS = {MAXN: (0.0, 5.0, 1.0), NONNEG: (0.0, 0.0, 0.0), UNIT: (0.0, 0.0, 0.0), MINMAX: (2.0, 5.0, 0.5)}
# (offset, R, M, float4 columns): conv axis 0 at an offset that is no multiple of 4, and the same aligned with
# M % 4 == 0 (float4, one chunk: summed inside the apply launch); 27 x 5; 1000 rows = 8 row chunks of
# CON_MIN_CHUNK_ROWS = 128 (the two-launch path), aligned (float4) and not (scalar although M % 4 == 0); a bias
SHAPES = {"3x105": (5, 3, 105, 0), "3x104": (8, 3, 104, 1), "27x5": (8, 27, 5, 0), "1000x24": (16, 1000, 24, 1),
          "1000x24u": (5, 1000, 24, 0), "10x1": (4, 10, 1, 0)}
# 4 fp32 ulp per element, derived: the sum of squares of small integers is exact, then the sqrt, the epsilon
# add, the divide and the multiply round once each
ULPS = 4


def _expected(w, kind):
    w = w.astype(np.float64)
    lo, hi, rate = PARAMS[kind]
    n = np.sqrt((w * w).sum(axis=0, keepdims=True))
    eps = float(np.float32(1e-7))
    out = {MAXN: lambda: w * (np.clip(n, 0, hi) / (eps + n)), NONNEG: lambda: w * (w >= 0),
           UNIT: lambda: w / (eps + n), MINMAX: lambda: w * ((rate * np.clip(n, lo, hi) + (1 - rate) * n) / (eps + n))}
    return out[kind]().astype(np.float32)


def _run(tensors, total, seed):
    from cori_intml_examples_amd.ops.hip import kernels
    K = kernels()
    rs = np.random.RandomState(seed)
    src = rs.randint(-4, 5, total).astype(np.float32)
    want = src.copy()
    for off, R, Mc, kind in tensors:
        w = src[off:off + R * Mc].reshape(R, Mc)
        if Mc >= 3:
            w[:, 0] = 0.0                                 # an all-zero column
            w[:, 1] = 0.0
            w[:2, 1] = (3.0, -4.0)                        # a column whose norm is max_value = 5 exactly
        want[off:off + R * Mc] = _expected(w, kind).reshape(-1)
    buf = torch.from_numpy(src.copy()).cuda()
    a = K.ConArgs()
    a.p, a.n = buf.data_ptr(), total
    a.set_tensors([(off, R, Mc, kind) + PARAMS[kind] for off, R, Mc, kind in tensors])
    plan = a.plan()
    part = torch.zeros(max(plan[0], 1), dtype=torch.float32, device="cuda")
    a.partials, a.npartials = part.data_ptr(), part.numel()
    s = torch.cuda.current_stream().cuda_stream
    K.constraint_norms(a, s)
    K.constraint_apply(a, s)
    torch.cuda.synchronize()
    return src, buf.cpu().numpy(), want, plan


def _check(tensors, total, seed):
    src, got, want, plan = _run(tensors, total, seed)
    inside = np.zeros(total, dtype=bool)
    for off, R, Mc, kind in tensors:
        inside[off:off + R * Mc] = True
        ulps = np.abs(got[off:off + R * Mc].astype(np.float64) - want[off:off + R * Mc]) / np.spacing(
            np.abs(want[off:off + R * Mc]))
        print("%dx%d kind %d: max %.2f ulp" % (R, Mc, kind, ulps.max()))
        assert ulps.max() <= ULPS, (R, Mc, kind, ulps.max())
    assert np.array_equal(got[~inside].view(np.uint32), src[~inside].view(np.uint32))      # outside: bit-unchanged
    assert np.array_equal(_run(tensors, total, seed)[1].view(np.uint32), got.view(np.uint32))  # a second run: same bits
    return got, plan


@pytest.mark.parametrize("kind", [MAXN, NONNEG, UNIT, MINMAX])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_kernel_against_float64(shape, kind):
    off, R, Mc, want_vec = SHAPES[shape]
    got, plan = _check([(off, R, Mc, kind)], off + R * Mc + 7, seed=R + kind)
    vec, _, rchunk, nchunk, _ = plan[3][0]
    assert vec == want_vec and nchunk == (8 if R == 1000 else 1) and rchunk == 128
    assert plan[1] == (8 if R == 1000 and kind != NONNEG else 0)       # the norms launch: split reductions only
    w = got[off:off + R * Mc].reshape(R, Mc)
    assert Mc < 3 or not w[:, 0].any()                    # norm 0 stays 0: no NaN
    assert Mc < 3 or kind != NONNEG or (w[0, 1] == 3.0 and w[1, 1] == 0.0 and w.min() >= 0.0)


def test_two_tensors_and_a_bias_in_one_table():
    tensors = [(5, 3, 105, MAXN), (320, 1000, 24, UNIT), (320 + 24000 + 3, 10, 1, NONNEG)]
    _check(tensors, 24400, seed=11)


@pytest.mark.parametrize("name,knobs", [("SGD", ""), ("Adam", ""), ("SGD", "opt_packs=0")])
def test_small_model_matches_the_cpu_executor(name, knobs, tmp_path, monkeypatch):
    """Three steps on both executors: masters within the project's model-level bound (relative L2 1e-2; Adam at
    Keras' default lr, which that bound was set for: README; its GPU steps are ONE graph of three bodies), the
    packs hold the constrained values (opt_packs=0: no routes, the packs are marked stale), the norms hold."""
    monkeypatch.setenv("INTML_TUNE", knobs)
    mk = {"SGD": lambda: optim.SGD(lr=0.05), "Adam": lambda: optim.Adam(lr=0.001)}[name]
    models = {}
    for dev in ("cpu", "cuda"):
        set_random_seed(4)
        m = models[dev] = M.small(mk(), device=dev)
        if dev == "cuda" and name == "Adam":
            d = m._executor.upload(*(np.concatenate(v) for v in zip(*M.batches(3))))
            m._executor.train_steps(d, torch.arange(d.n, device="cuda"), 0, 8, 3)
            continue
        for x, y in M.batches(3):
            m.train_on_batch(x, y)
    g, c = models["cuda"], models["cpu"]
    plan = next(p for (_, mode, *_), p in g._executor._plans.items() if mode == "train")
    assert [l.name for l in plan.end_launches] == ["constraint_norms", "constraint_apply"]    # (240 x 12 dense: 2 chunks)
    assert [t[0] for t in plan.end_launches[-1].args["con"].plan()[3]] == [0, 1, 1, 0]         # float4: conv 2, dense
    assert (g._executor.routes is None) == bool(knobs)
    wg, wc = np.concatenate([w.ravel() for w in g.get_weights()]), np.concatenate([w.ravel() for w in c.get_weights()])
    rel = float(np.linalg.norm(wg.astype(np.float64) - wc) / np.linalg.norm(wc))
    x = M.batches(1, rows=16, seed=9)[0][0]
    pred = g.predict(x)
    g.save(str(tmp_path / "con.h5"))
    fresh = load_model(str(tmp_path / "con.h5"), device="cuda").predict(x)
    rel_pred = float(np.linalg.norm(pred.astype(np.float64) - fresh) / np.linalg.norm(fresh))
    print("%s: masters rel L2 %.3e, predict vs reloaded copy rel L2 %.3e" % (name, rel, rel_pred))
    assert rel <= 1e-2 and rel_pred <= 1e-2
    arena = g._executor.arena.clone()                     # the packs mirror the constrained master
    g._executor.params_changed()
    assert torch.equal(arena, g._executor.arena)
    M.check_constrained(g.get_weights())


def test_no_constraints_no_change():
    names = []
    for con in (False, None):
        set_random_seed(4)
        m = M.small(optim.Adam(lr=0.001), device="cuda", con=con)
        m.train_on_batch(*M.batches(1)[0])
        ex = m._executor
        plan = next(p for (_, mode, *_), p in ex._plans.items() if mode == "train")
        assert plan.end_launches == [] and ex.cons == [] and ex.con_partials is None
        names.append([l.name for l in plan.launches])
    assert names[0] == names[1]

"""Keras gradient clipping on the GPU: the ticketed global-norm kernel against float64 (ragged
lengths, the comparison's flip, determinism and the ticket reset), the clipped optimizer launch
against the float64 oracle (tests/helpers/clip_oracle.py), its tile blocks and pack routes, the
bit-identity of a never-reached clip with the unclipped fuse_optim=0 step, graph replay, plan
gating, the data-parallel step at one rank, zero gradients and a GPU -> CPU checkpoint."""
import json
import math
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

from helpers import clip_oracle as C
from test_hip_model import _build, _data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

KINDS = {"SGD": lambda **kw: optim.SGD(lr=0.01, momentum=0.9, **kw), "Adam": optim.Adam, "Nadam": optim.Nadam,
         "Adadelta": optim.Adadelta, "Adamax": optim.Adamax, "AMSGrad": lambda **kw: optim.Adam(amsgrad=True, **kw)}
# From a dry run of the CPU executor on these models and batches: the global gradient norm of the
# three steps is 0.16 .. 0.19 ("tiny") and 0.45 .. 1.5 ("odd"), the largest element 0.06 .. 0.27;
# after the norm clip to 0.05 the largest element is 0.007 .. 0.02.  So clipnorm 0.05 fires on
# every step, clipvalue 0.01 alone clamps elements, and so does 0.004 behind the norm clip
# (each test asserts both from the oracle).
CLIPS = {"norm": {"clipnorm": 0.05}, "value": {"clipvalue": 0.01}, "both": {"clipnorm": 0.05, "clipvalue": 0.004}}


def _K():
    from cori_intml_examples_amd.ops.hip import kernels
    return kernels()


def _tiny(opt, device="cuda", drop=0.0):
    """16x16x3, conv [4, 8, 8], fc [16] (tests/test_new_optimizers_gpu.py::_tiny)."""
    return zoo.rpv_cnn((16, 16, 3), conv_sizes=[4, 8, 8], fc_sizes=[16], dropout=drop, optimizer=opt, lr=None,
                       device=device)


# ------------------------------------------------------------------------------------ 8. the norm kernel
def _sqnorm(K, buf, off, n, c, state, partials):
    a = K.ClipArgs()
    a.g = buf.data_ptr() + 4 * off
    a.n, a.clipnorm = n, c
    a.partials, a.npartials = partials.data_ptr(), partials.numel()
    a.state = state.data_ptr()
    K.grad_sqnorm(a, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    s = state.cpu()
    assert int(s.view(torch.int32)[K.CLIP_TICKET]) == 0          # the last workgroup reset the ticket
    return np.float32(s[K.CLIP_NORM].item()), np.float32(s[K.CLIP_FACTOR].item()), K.clip_blocks(a)


def _chain(K, nparts):
    """The longest chain of additions of grad_sqnorm_kernel: per thread CLIP_VEC_PER_THREAD groups
    of ((x2 + y2) + (z2 + w2)) added to the accumulator (3 each), the workgroup tree (6 butterfly
    levels + 3 adds of the 4 wave sums), then the finish: ceil(partials / 256) adds per thread and
    the same tree."""
    tree = 6 + 3
    return 3 * K.CLIP_VEC_PER_THREAD + tree + math.ceil(nparts / K.CLIP_THREADS) + tree


def _lengths(K):
    ch = K.CLIP_CHUNK
    return [1, 3, 4, 1023, 1024, 1025, ch - 1, ch, ch + 1, 3 * ch + 5, 200003]


@pytest.mark.parametrize("off", [0, 1, 3])
def test_grad_sqnorm_against_float64(off):
    """Random fp32 vectors inside a NaN-padded buffer (a read outside [0, n) poisons the norm), at
    16-byte-aligned and 4-byte-aligned bases.  All terms are non-negative, so the sum's relative
    error is at most (L + 2) * 2^-24 (L: _chain); 2 ulp more for the square root and the quotient."""
    K = _K()
    dev = torch.device("cuda")
    state = torch.zeros(K.CLIP_STATE_WORDS, dtype=torch.float32, device=dev)
    gen = torch.Generator().manual_seed(11)
    for n in _lengths(K):
        partials = torch.full((n // K.CLIP_CHUNK + 3,), float("nan"), dtype=torch.float32, device=dev)
        host = torch.full((n + 64,), float("nan"), dtype=torch.float32)
        g = torch.randn(n, generator=gen) * 10.0 ** torch.empty(n).uniform_(-3, 1, generator=gen)
        host[8 + off:8 + off + n] = g
        buf = host.to(dev)
        ref = float(np.sqrt(np.sum(g.double().numpy() ** 2)))
        c = 0.25 * ref                                # the clip fires: factor = c / norm
        norm, factor, blocks = _sqnorm(K, buf, 8 + off, n, c, state, partials)
        assert blocks == max(1, math.ceil((off + n) / K.CLIP_CHUNK))
        tol = (_chain(K, blocks) + 2) * 2.0 ** -24 + 2 * 2.0 ** -23
        print("n %d off %d: %d partials, norm %.8g (float64 %.8g, rel err %.3g, bound %.3g), factor %.8g" % (
            n, off, blocks, norm, ref, abs(float(norm) - ref) / ref, tol, factor))
        assert abs(float(norm) - ref) <= tol * ref, (n, off, norm, ref)
        assert abs(float(factor) - c / ref) <= tol * (c / ref), (n, off, factor, c / ref)
        # the comparison flips between c just below / at and c just above the fp32 norm
        for cc, fires in ((np.nextafter(norm, np.float32(0)), True), (norm, True),
                          (np.nextafter(norm, np.float32(np.inf)), False)):
            n2, f2, _ = _sqnorm(K, buf, 8 + off, n, float(cc), state, partials)
            assert n2 == norm                         # bit-identical norm
            want = np.float32(cc) / norm if fires else np.float32(1.0)
            assert abs(float(f2) - float(want)) <= 2.0 ** -23 and f2 <= 1.0, (n, cc, f2)
            assert (f2 < 1.0) == (cc < norm), (n, cc, f2)      # strictly below 1 only when c < norm
        assert bool(torch.isnan(buf[:8 + off]).all()) and bool(torch.isnan(buf[8 + off + n:]).all())


def test_grad_sqnorm_zero_vector_and_nan():
    K = _K()
    dev = torch.device("cuda")
    state = torch.full((K.CLIP_STATE_WORDS,), 7.0, dtype=torch.float32, device=dev)
    state.view(torch.int32)[K.CLIP_TICKET] = 0
    partials = torch.zeros(8, dtype=torch.float32, device=dev)
    z = torch.zeros(3 * K.CLIP_CHUNK + 5, dtype=torch.float32, device=dev)
    norm, factor, _ = _sqnorm(K, z, 0, z.numel(), 1.0, state, partials)
    assert norm == 0.0 and factor == 1.0              # no division, no NaN
    z[777] = float("nan")
    norm, factor, _ = _sqnorm(K, z, 0, z.numel(), 1.0, state, partials)
    assert np.isnan(norm) and factor == 1.0           # a NaN norm fails the comparison


# ------------------------------------------------------------------------------------ 9. determinism
def test_grad_sqnorm_is_deterministic_and_resets_its_ticket():
    K = _K()
    dev = torch.device("cuda")
    state = torch.zeros(K.CLIP_STATE_WORDS, dtype=torch.float32, device=dev)
    partials = torch.zeros(64, dtype=torch.float32, device=dev)
    gen = torch.Generator().manual_seed(3)
    g1 = torch.randn(200003, generator=gen).to(dev)
    g2 = (torch.randn(200003, generator=gen) * 3).to(dev)
    first = _sqnorm(K, g1, 0, g1.numel(), 1.0, state, partials)
    for _ in range(19):                               # 20 consecutive launches: the same bits
        assert _sqnorm(K, g1, 0, g1.numel(), 1.0, state, partials)[:2] == first[:2]
    other = _sqnorm(K, g2, 0, g2.numel(), 1.0, state, partials)
    ref2 = float(np.sqrt(np.sum(g2.double().cpu().numpy() ** 2)))
    assert other[0] != first[0] and abs(float(other[0]) - ref2) < 1e-5 * ref2     # its own value, not a stale one
    # back to back without a host sync in between (stream order alone), then the first input again
    a = K.ClipArgs()
    a.g, a.n, a.clipnorm = g1.data_ptr(), g1.numel(), 1.0
    a.partials, a.npartials, a.state = partials.data_ptr(), partials.numel(), state.data_ptr()
    b = K.ClipArgs()
    b.g, b.n, b.clipnorm = g2.data_ptr(), g2.numel(), 1.0
    b.partials, b.npartials, b.state = partials.data_ptr(), partials.numel(), state.data_ptr()
    s = torch.cuda.current_stream().cuda_stream
    for args in (b, a, b, a):
        K.grad_sqnorm(args, s)
    torch.cuda.synchronize()
    assert np.float32(state[K.CLIP_NORM].item()) == first[0]
    assert int(state.view(torch.int32)[K.CLIP_TICKET].item()) == 0


def test_grad_clip_apply_matches_oracle():
    """The in-place clip of the data-parallel step: ragged length, 4-byte-aligned base, NaN padding."""
    K = _K()
    dev = torch.device("cuda")
    n, off = 3 * K.CLIP_CHUNK + 5, 9
    gen = torch.Generator().manual_seed(5)
    g = torch.randn(n, generator=gen) * 0.1
    for cn, cv in ((2.0, 0.0), (0.0, 0.05), (2.0, 0.01)):
        host = torch.full((n + 64,), float("nan"), dtype=torch.float32)
        host[off:off + n] = g
        buf = host.to(dev)
        state = torch.zeros(K.CLIP_STATE_WORDS, dtype=torch.float32, device=dev)
        partials = torch.zeros(8, dtype=torch.float32, device=dev)
        a = K.ClipArgs()
        a.g, a.n, a.clipnorm, a.clipvalue, a.use_norm = buf.data_ptr() + 4 * off, n, cn, cv, int(cn > 0)
        a.partials, a.npartials, a.state = partials.data_ptr(), partials.numel(), state.data_ptr()
        s = torch.cuda.current_stream().cuda_stream
        if cn:
            K.grad_sqnorm(a, s)
        K.grad_clip_apply(a, s)
        torch.cuda.synchronize()
        want, info = C.clip(g.double().numpy(), cn or None, cv or None)
        assert (info["fired"] or not cn) and (info["clamped"] or not cv)
        got = buf[off:off + n].cpu().double().numpy()
        np.testing.assert_allclose(got, want, rtol=2e-6, atol=0)
        assert bool(torch.isnan(buf[:off]).all()) and bool(torch.isnan(buf[off + n:]).all())


# ------------------------------------------------------------------------------------ 10. the clipped update
@pytest.mark.parametrize("clip", sorted(CLIPS))
@pytest.mark.parametrize("model", ["tiny", "odd"])
@pytest.mark.parametrize("name", sorted(KINDS))
def test_clipped_update_matches_keras_math(name, model, clip):
    """3 steps at batch 32; after each, the master and every slot against the float64 oracle fed
    with the (unclipped) reduced gradient read back from the device.  Bound: the project's
    2e-5 * max(1, 100 lr)."""
    kw = CLIPS[clip]
    set_random_seed(5)
    opt = KINDS[name](**kw)
    m = _tiny(opt) if model == "tiny" else _build("odd", "cuda", opt=opt, cin=2, hw=16)
    ex = m._executor
    o = ex.opt
    n = m.store.numel
    assert n % 4 != 0                                 # (1537 and 3046 parameters: ragged float4 tails)
    x, y = _data(m, 96, seed=3)
    d = ex.upload(x, y)
    p = m.store.master[:n].cpu().double().numpy()
    slots = [np.zeros(n) for _ in range(o.n_slots)]
    assert len(ex.slots) == o.n_slots
    bound = 2e-5 * max(1.0, 100 * float(o.lr))
    fired = clamped = 0
    for t in range(1, 4):
        ex.train_step(d, torch.arange(d.n, device=ex.device), 32 * (t - 1), 32)
        torch.cuda.synchronize()
        gr = m.store.grad[:n].cpu().double().numpy()              # single GPU: the unclipped gradient
        p, slots, info = C.step(o.kind, p, gr, slots, t, o, **kw)
        fired += info["fired"]
        clamped += info["clamped"]
        if "clipnorm" in kw:
            dn = float(ex.clip_state[ex.K.CLIP_NORM].item())
            assert abs(dn - info["norm"]) < 1e-5 * info["norm"], (dn, info)
        got = m.store.master[:n].cpu().double().numpy()
        errs = [float(np.abs(got - p).max())] + [float(np.abs(s.cpu().double().numpy() - r).max())
                                                 for s, r in zip(ex.optimizer_state(), slots)]
        print("%s %s %s step %d: norm %s, clamped %d, max |err| master %.3g, slots %s (bound %.3g)" % (
            name, model, clip, t, info["norm"], info["clamped"], errs[0], ["%.3g" % e for e in errs[1:]], bound))
        assert max(errs) < bound, (name, model, clip, t, errs)
    assert fired >= 1 or "clipnorm" not in kw
    assert clamped >= 1 or "clipvalue" not in kw
    plan = ex._plans[(32, "train")]
    assert not plan.optim_fused and plan.early_red == {} and plan.dense_fused_opt == []
    arena = ex.arena.clone()                                       # the packs mirror the master
    ex.params_changed()
    torch.cuda.synchronize()
    assert torch.equal(arena, ex.arena)


# ------------------------------------------------------------------------------------ 11. tile blocks
def _clipped_route_run(use_tiles, clipped=True):
    set_random_seed(45)
    opt = optim.Adam(clipnorm=0.5, clipvalue=0.004) if clipped else optim.Adam()
    m = _build("rpv", "cuda", opt=opt, drop=0.0, cin=3, hw=16)
    ex = m._executor
    assert ex.routes is not None
    n = ex.store.numel
    ex._st_f32[ex.K.STEP_STATE_S_OFFSET // 4] = 1e-3
    gen = torch.Generator().manual_seed(7)
    g1 = torch.randn(ex.store.capacity, generator=gen) * 1e-2
    s = torch.cuda.current_stream().cuda_stream
    for g in (g1, 3 * g1):
        ex.store.grad.copy_(g.to(ex.device))
        if clipped:
            ex.K.grad_sqnorm(ex._clip_args(), s)
        a = ex._optim_args(False, defer_pack=True, clip=clipped)
        assert bool(a.clip) == clipped and (a.clipvalue > 0) == clipped
        if use_tiles:
            ex.tile_routes(a)
            assert a.ntile == 1
        ex.K.optim(a, ex.pack_table, s)
        torch.cuda.synchronize()
        if clipped:
            norm, factor = ex.clip_state[:2].tolist()
            assert norm > 0.5 and factor < 1.0          # (norm ~ 1e-2 sqrt(n) > 0.5: the clip fired)
        written = ex.arena.clone()
        ex.params_changed()
        torch.cuda.synchronize()
        assert torch.equal(written, ex.arena)           # the packs it wrote equal a full re-pack
    return m.store.master[:n].clone(), [s_[:n].clone() for s_ in ex.slots]


def test_clipped_tile_blocks_equal_the_flat_launch():
    flat = _clipped_route_run(False)
    til = _clipped_route_run(True)
    assert torch.equal(flat[0], til[0])
    for a, b in zip(flat[1], til[1]):
        assert torch.equal(a, b) and float(a.abs().sum()) > 0
    plain = _clipped_route_run(True, clipped=False)
    assert not torch.equal(plain[1][0], til[1][0])      # ... and the clip changed what Adam's m saw
    # the value clip bounds what m saw: |m| <= (1 - beta_1) v + beta_1 (1 - beta_1) v after two steps
    assert float(til[1][0].abs().max()) <= 0.19 * 0.004 * (1 + 1e-5)


# ------------------------------------------------------------------------------------ 12. a clip never reached
def _train4(opt, tv, monkeypatch, drop=0.2):
    monkeypatch.setenv("INTML_TUNE", tv)
    set_random_seed(9)
    m = _tiny(opt, drop=drop)
    x, y = _data(m, 128, seed=6)
    ex = m._executor
    d = ex.upload(x, y)
    for t in range(4):
        ex.train_step(d, torch.arange(d.n, device=ex.device), 32 * t, 32)
    torch.cuda.synchronize()
    n = m.store.numel
    plan = ex._plans[(32, "train")]
    return [m.store.master[:n].clone()] + [s.clone() for s in ex.optimizer_state()], plan, ex


@pytest.mark.parametrize("name", ["Adam", "Adadelta"])
def test_unreached_clip_is_bit_identical_to_the_unfused_step(name, monkeypatch):
    """clipnorm = clipvalue = 1e30 against the same optimizer under fuse_optim=0,early_reduce=0 (the
    same structure without the clip): master and every slot, 4 steps."""
    got, plan, ex = _train4(KINDS[name](clipnorm=1e30, clipvalue=1e30), "", monkeypatch)
    assert [l.name for l in plan.launches].count("grad_sqnorm") == 1 and not plan.optim_fused
    assert float(ex.clip_state[ex.K.CLIP_FACTOR].item()) == 1.0 and float(ex.clip_state[ex.K.CLIP_NORM].item()) > 0
    ref, rplan, rex = _train4(KINDS[name](), "fuse_optim=0,early_reduce=0", monkeypatch)
    assert not rplan.optim_fused and rex.clip_state is None
    assert [l.name for l in plan.launches if l.name != "grad_sqnorm"] == [l.name for l in rplan.launches]
    assert len(got) == len(ref) == 3
    for a, b in zip(got, ref):
        assert torch.equal(a, b) and float(a.abs().sum()) > 0


# ------------------------------------------------------------------------------------ 13. graph replay
@pytest.mark.parametrize("name", ["Adam", "Adamax", "SGD"])
def test_graph_of_8_steps_equals_8_single_steps(name):
    """The ticket and the factor must be right across the steps inside one graph."""
    res = []
    for chunks in ([1] * 8, [8]):
        set_random_seed(21)
        m = _tiny(KINDS[name](decay=0.01, clipnorm=0.05), drop=0.2)
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
                    int(ex._st_i32[0]), int(m.optimizer.iterations), ex.clip_state.clone()))
        assert float(ex.clip_state[ex.K.CLIP_FACTOR].item()) < 1.0
    for a, b in zip(res[0][0], res[1][0]):
        assert torch.equal(a, b)
    assert torch.equal(res[0][3], res[1][3])
    assert res[0][1] == res[1][1] == res[0][2] == res[1][2] == 8


# ------------------------------------------------------------------------------------ 14. plan gating
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
    return ex._plans[(128, "train")], ex


@pytest.mark.parametrize("name", ["Adam", "Nadam", "Adamax"])
def test_clipping_plan_is_gated_like_the_standalone_kinds(name, monkeypatch):
    for kw, nnorm in (({"clipnorm": 1.0}, 1), ({"clipvalue": 0.5}, 0), ({"clipnorm": 1.0, "clipvalue": 0.5}, 1)):
        for tv in ("", "dense_opt=1"):
            plan, ex = _plan_of(KINDS[name](**kw), tv, monkeypatch)
            assert plan.early_red == {} and plan.dense_fused_opt == [] and not plan.dense_opt_ok
            assert not plan.optim_fused
            names = [l.name for l in plan.launches]
            assert names.count("grad_sqnorm") == nnorm and names[-1] == ("grad_sqnorm" if nnorm else names[-1])
            assert not [nm for nm in names if "clip_apply" in nm]      # one GPU: clipped on the fly
            a = ex._optim_args(False, defer_pack=True, clip=True)
            assert bool(a.clip) == bool(nnorm) and a.clipvalue == kw.get("clipvalue", 0.0)


def test_plan_without_clipping_is_unchanged(monkeypatch):
    plan, ex = _plan_of("Adam", "", monkeypatch)
    assert plan.early_red and plan.optim_fused
    names = [l.name for l in plan.launches]
    assert not [nm for nm in names if "sqnorm" in nm or "clip" in nm], names
    assert not ex.clips and ex.clip_state is None and ex.clip_partials is None
    for a in (ex._optim_args(False, defer_pack=True), ex._optim_args(False, defer_pack=True, clip=True)):
        assert a.clip == 0 and a.clipvalue == 0.0      # the unclipped kernel instance is launched
    assert names.count("reduce_b0") == 1                # ONE fused reduction + update launch


# ------------------------------------------------------------------------------------ 15. data parallel
def test_data_parallel_step_at_one_rank(tmp_path):
    out = tmp_path / "dp.json"
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("WORLD_SIZE", "RANK", "INTML_DP_BACKEND", "INTML_COMM", "INTML_XGMI", "INTML_TUNE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "clip_dp_worker_gpu.py"), str(out)],
                       env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rep = json.load(open(out))
    print(json.dumps(rep, indent=1))
    assert rep["native"], rep
    for name in ("Adam", "Adamax"):
        k = rep[name]
        assert k["moved"] > 1e-4 and not k["base_fused"] and k["base_sqnorm"] == 1, k
        for mode in ("captured", "segmented"):
            c = k[mode]
            assert c["reducer"] == "NativeGradReducer" and c["plane"] == "rccl" and not c["xgmi"], c
            assert c["comm_in_graph"] == (mode == "captured") and c["early_red"] == 0 and c["buckets"] == 1, c
            assert not [nm for nm in c["launches"] if "xgmi" in nm or "xchg" in nm], c
            # the order: local reduction, norm, in-place clip, all-reduce, unclipped update
            want = ["reduce_b0", "grad_sqnorm_b0", "grad_clip_apply_b0"]
            if mode == "captured":
                want += ["allreduce_b0", "optim_b0"]
            assert c["launches"] == want, c
            assert c["iterations"] == 4 and c["factor"] < 1.0, c
            print(name, mode, "bit-identical to the single-GPU clipped run:", c["identical"])
            assert max(c["max_abs_diff"]) < k["bound"], (name, mode, c)
            # store.grad after a data-parallel step: the (averaged) clipped gradient, norm = clipnorm
            assert abs(c["grad_norm"] - k["clipnorm"]) < 1e-5 * k["clipnorm"], c
        for plane in ("xgmi", "hybrid"):
            msg = k["forced_" + plane]
            assert name in msg and repr(plane) in msg and "clipnorm" in msg, k
    assert rep["history_data_plane"].startswith("NativeGradReducer:rccl"), rep["history_data_plane"]


# ------------------------------------------------------------------------------------ 16. zero gradient
@pytest.mark.parametrize("name", sorted(KINDS))
def test_all_zero_sample_weights(name):
    x, y, _ = synthetic_rpv(32, size=16, channels=3, seed=3)
    set_random_seed(5)
    opt = KINDS[name](clipnorm=1.0) if name != "SGD" else optim.SGD(lr=0.01, clipnorm=1.0)
    m = _tiny(opt)
    w0 = [w.copy() for w in m.get_weights()]
    m.train_on_batch(x, y, sample_weight=np.zeros(32, dtype=np.float32))
    torch.cuda.synchronize()
    ex = m._executor
    assert ex.clip_state[:2].tolist() == [0.0, 1.0]                # norm 0: factor 1, nothing divided
    assert all(np.all(np.isfinite(w)) for w in m.get_weights())
    assert all(bool(torch.isfinite(s).all()) for s in ex.optimizer_state())
    if name == "SGD":
        for a, b in zip(w0, m.get_weights()):
            np.testing.assert_array_equal(a, b)


# ------------------------------------------------------------------------------------ 17. checkpoint
def test_gpu_checkpoint_loads_on_cpu(tmp_path):
    x, y, _ = synthetic_rpv(64, channels=3, size=16, seed=1)
    set_random_seed(8)
    m = _tiny(optim.Adam(clipnorm=0.05, clipvalue=0.004))
    m.fit(x, y, batch_size=16, epochs=1, verbose=0, shuffle=False)
    p = str(tmp_path / "g.h5")
    m.save(p)
    c = load_model(p, device="cpu")
    assert c.store.master.device.type == "cpu" and c.optimizer.kind == "adam"
    cfg = c.optimizer.get_config()
    assert cfg["clipnorm"] == 0.05 and cfg["clipvalue"] == 0.004 and cfg == m.optimizer.get_config()
    assert c.optimizer.iterations == m.optimizer.iterations == 4
    for a, b in zip(m.get_weights(), c.get_weights()):
        np.testing.assert_array_equal(a, b)
    sg, sc = m._executor.optimizer_state(), c._executor.optimizer_state()
    assert len(sg) == len(sc) == 2
    for a, b in zip(sg, sc):
        assert float(b.abs().sum()) > 0
        np.testing.assert_array_equal(a.cpu().numpy(), b.numpy())

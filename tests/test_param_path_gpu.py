"""The kernels between a step's gradients and the next step's weights, each driven directly and held
per element to the float64 / exact-integer oracle of tests/helpers/param_oracle.py: the deterministic
slab reduction (slab_reduce_kernel, both paths of reduce_body.h), the eight Keras updates in their
three launch forms (optim_kernel flat and tile blocks, reduce_optim_kernel), the bf16 fragment packs
(pack_kernel, the pack routes of the updates) and the step bookkeeping scalars (step_book.h).

Every output buffer starts from a known bit pattern and every element a case should not write must
keep it; slab positions no map reads are NaN.  The inputs are those of tests/helpers/param_cases.py;
tests/test_param_oracle.py proves on the CPU that they discriminate.  Every case passes
``check_case_fits`` on the host before its first launch.

Worst observed error / bound per kernel form and kind (MI355X; the bounds are the oracle's derivation
and were not changed after the run).  A weight's ratio sits just below 1 by construction: its bound is
dominated by the half ulp of the final ``p - update`` rounding, which some element always reaches.

  slab_reduce        scalar path 0.996    float4 path 0.993    descriptors alone 0.629
                     (integer slabs exact; float4 == scalar and launch == launch bit for bit)
  form               kind          p      s0     s1     s2
  optim flat         sgd           0.938
  optim flat         sgd_momentum  0.961  0.444
  optim flat         sgd_nesterov  0.988  0.455
  optim flat         rmsprop       0.978  0.552
  optim flat         adadelta      0.920  0.435  0.385
  optim flat         adam          0.979  0.527  0.552
  optim flat         nadam         0.951  0.527  0.435
  optim flat         adagrad       0.982  0.648
  optim flat         adamax        0.969  0.563  0.973
  optim flat         amsgrad       0.979  0.583  0.552  0.552
  optim routes       sgd           0.982
  optim routes       adam          0.990  0.463  0.550
  optim routes       amsgrad       0.980  0.596  0.550  0.550
  optim tile         sgd_nesterov  0.988  0.455
  optim tile         rmsprop       0.978  0.552
  optim tile         adam          0.979  0.495  0.552
  optim tile         amsgrad       0.979  0.583  0.552  0.552
  optim tile, clip   adam          0.981  0.491  0.501                  (flat launch of the pair: the same)
  reduce_optim       sgd           0.948
  reduce_optim       sgd_momentum  0.969  0.547
  reduce_optim       sgd_nesterov  0.922  0.547
  reduce_optim       rmsprop       0.953  0.670
  reduce_optim       adadelta      0.992  0.670  0.390
  reduce_optim       adam          0.965  0.682  0.663
  reduce_optim       nadam         0.950  0.682  0.663
  reduce_optim       adagrad       0.972  0.790
  reduce_optim       adamax        0.982  0.682  0.975
  reduce_optim       amsgrad       0.965  0.682  0.663  0.663
  reduce_optim tile  adam          0.972  0.708  0.673
  reduce_optim tile  amsgrad       0.972  0.708  0.673  0.673
  step scalars       sgd 0.053  rmsprop 0.204  adagrad 0.053  adadelta 0.315  adam 0.438  adamax 0.346
                     nadam 0.424  amsgrad 0.438          (m_schedule equal to the float64 product)
  packs              exact (uint16 equality), subnormals and ties included
``pytest -s`` prints the current figures.
"""
import numpy as np
import pytest
import torch

from cori_intml_examples_amd import optim
from cori_intml_examples_amd.apps import zoo
from cori_intml_examples_amd.utils import set_random_seed

from helpers import clip_oracle as C
from helpers import param_cases as PC
from helpers import param_oracle as P

pytestmark = pytest.mark.gpu

DEV = "cuda"
F_SENTINEL = 0x7FA5A5A5            # int32 view of an untouched float element (a NaN)
A_SENTINEL = 0x7FA5                # int16 view of an untouched arena element
RED_LANES = 16                     # the split-lane target these tests set themselves
_worst = {}


def _K():
    from cori_intml_examples_amd.ops.hip import kernels
    return kernels()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _fbuf(n):
    return torch.full((n,), F_SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)


def _abuf(n):
    return torch.full((n,), A_SENTINEL, dtype=torch.int16, device=DEV).view(torch.bfloat16)


def _np(t):
    return t.detach().cpu().numpy()


def _u16(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _note(key, got, ref, bound):
    """Record and return the worst error / bound ratio (0 / 0 counts as 0)."""
    w = P._ratio(got, ref, bound)
    _worst[key] = max(_worst.get(key, 0.0), w)
    print("%-40s worst error / bound %.3f" % (key, _worst[key]))
    return w


class _Lanes:
    """K.set_red_lanes for the duration of a block; the tuned value is put back afterwards."""

    def __init__(self, K, n):
        self.K, self.n = K, n

    def __enter__(self):
        self.K.set_red_lanes(self.n)

    def __exit__(self, *exc):
        from cori_intml_examples_amd.utils.tune import tune
        self.K.set_red_lanes(int(tune("red_lanes")))


# =============================================================================== slab reduction
def _table(K, descs, slab_t):
    tab = K.RedTable()
    for d in descs:
        tab.add(slab_t.data_ptr() + 4 * d.slab_off, d.stride_s, d.S, d.ld, d.dst_off, d.numel, d.type, d.KH, d.KW,
                d.Cin, d.Cout, d.Cs, tpe=d.tpe)
    return tab


def _reduce(K, descs, slab, slab_numel, grad_numel):
    P.check_case_fits({"red": {"descs": descs, "slab_numel": slab_numel, "grad_numel": grad_numel}})
    slab_t = _dev(slab)
    tab = _table(K, descs, slab_t)
    out = []
    for _ in range(2):
        grad = _fbuf(grad_numel)
        K.slab_reduce(grad.data_ptr(), 0, grad_numel, tab, _stream())
        torch.cuda.synchronize()
        out.append(grad)
    assert _same_bits(out[0], out[1]), "two launches differ"
    return out[0], tab


def _check_reduce(key, grad, descs, slab, mode):
    g = _np(grad)
    untouched = np.ones(g.size, dtype=bool)
    for d in descs:
        got = g[d.dst_off:d.dst_off + d.numel]
        untouched[d.dst_off:d.dst_off + d.numel] = False
        if mode == "int":
            ref = P.slab_sum_exact(slab, d)
            assert np.array_equal(got.astype(np.float64), ref.astype(np.float64)), (key, d.name, d.S, d.tpe)
        else:
            ref, A = P.slab_sum(slab, d)
            w = _note("slab_reduce %s" % key, got, ref, P.slab_bound(d.S, A))
            assert w <= 1.0, (key, d.name, d.S, d.tpe, w)
    assert np.all(g.view(np.int32)[untouched] == F_SENTINEL), (key, "stray write")


@pytest.mark.parametrize("tpe", PC.TPES)
def test_slab_reduce_scalar_path(tpe):
    """Explicit tpe (scalar path) over the boundaries of the 8-deep slab loop and its tail, the six
    descriptors in one table: exact on integer slabs, inside gamma(S-1) A on spread normals."""
    K = _K()
    for S in PC.s_list(tpe):
        descs, numel = PC.red_descs(S, tpe)
        for mode in ("int", "normal"):
            slab = PC.red_slab(descs, numel, mode, seed=S)
            grad, tab = _reduce(K, descs, slab, numel, PC.GRAD_NUMEL)
            assert all(tab.flags(i)[:2] == (tpe, 0) for i in range(len(descs)))
            _check_reduce("scalar", grad, descs, slab, mode)


@pytest.mark.parametrize("name", PC.DESC_NAMES)
def test_slab_reduce_descriptor_alone(name):
    """Each descriptor as the only one of its table, at its own dst_off (3, 8, ...), tpe 4 and auto."""
    K = _K()
    with _Lanes(K, RED_LANES):
        for tpe in (4, -1):
            for S in PC.s_list(4):
                descs, numel = PC.red_descs(S, tpe, names=[name], alone=True)
                for mode in ("int", "normal"):
                    slab = PC.red_slab(descs, numel, mode, seed=S)
                    grad, _ = _reduce(K, descs, slab, numel, 2176)
                    _check_reduce("alone", grad, descs, slab, mode)


@pytest.mark.parametrize("tpe", [1, 2, 4, 8, 64])
def test_slab_reduce_float4_path_and_its_agreement_with_the_scalar_path(tpe):
    """The identity descriptors without a tpe (float4 path, split-lanes chosen through
    set_red_lanes) and, in the same table over the same slabs, the scalar path at the same tpe:
    reduce_body.h says the two agree bit for bit."""
    K = _K()
    for S in PC.s_list(tpe):
        lanes = PC.lanes_for(S, tpe) or 1
        want = PC.auto_tpe(S, lanes)
        with _Lanes(K, lanes):
            v4, numel = PC.red_descs(S, -1, names=PC.VEC4_NAMES)
            sc, _ = PC.red_descs(S, want, names=PC.VEC4_NAMES)
            for d in sc:
                d.dst_off += PC.GRAD_NUMEL
            for mode in ("int", "normal"):
                slab = PC.red_slab(v4, numel, mode, seed=S)
                grad, tab = _reduce(K, v4 + sc, slab, numel, 2 * PC.GRAD_NUMEL)
                for i in range(3):
                    assert tab.flags(i)[:2] == (want, 1) and tab.flags(i + 3)[:2] == (want, 0), (S, tab.flags(i))
                _check_reduce("float4", grad, v4 + sc, slab, mode)
                assert _same_bits(grad[:PC.GRAD_NUMEL], grad[PC.GRAD_NUMEL:]), (S, want, "float4 != scalar")


# =============================================================================== optimizer
def _state(K, scalars):
    st = torch.zeros(K.STEP_STATE_BYTES, dtype=torch.uint8, device=DEV)
    o = K.STEP_STATE_S_OFFSET // 4
    st.view(torch.float32)[o:o + 6] = torch.tensor(scalars, dtype=torch.float32)
    return st


def _optim_args(K, form, bufs, st, lo, n, clipvalue=0.0):
    hp = PC.hyper_of(form)
    a = K.OptimArgs()
    a.p, a.g = bufs["p"].data_ptr(), bufs["g"].data_ptr()
    for i in range(PC.slots_of(form)):
        setattr(a, "s%d" % i, bufs["s%d" % i].data_ptr())
    a.n, a.lo, a.st = n, lo, st.data_ptr()
    a.kind = P.KIND_ID[PC.form_kind(form)]
    a.beta1, a.beta2, a.eps, a.rho, a.momentum = hp.beta1, hp.beta2, hp.eps, hp.rho, hp.momentum
    a.nesterov, a.grad_scale = int(hp.nesterov), hp.grad_scale
    a.defer_pack = 1
    a.clipvalue = clipvalue
    return a


def _buffers(form, numel, seed=0, g=None):
    """The five device buffers: p, g and the form's slots from the shared inputs; the slots the
    form does not use hold ordinary random values nothing may change."""
    p, g0, slots = PC.optim_inputs(form, numel, seed)
    rs = np.random.RandomState(77)
    host = {"p": p, "g": g0 if g is None else g}
    for i in range(3):
        host["s%d" % i] = slots[i] if i < len(slots) else rs.randn(numel).astype(np.float32)
    return host, {k: _dev(v) for k, v in host.items()}


def _routes_dev(K, routes):
    return _dev(P.route_array(routes, K.PACK_ROUTE_BYTES // 4))


def _check_update(key, form, host, bufs, idx, g_used, g_unchanged=True):
    """Master and slots at the elements ``idx`` (bool mask) against the oracle of the values before
    the launch; everything else bit-identical; the gradient untouched."""
    kind, ns = PC.form_kind(form), PC.slots_of(form)
    after = {k: _np(v) for k, v in bufs.items()}
    r = P.update(kind, host["p"][idx], g_used[idx], [host["s%d" % i][idx] for i in range(ns)], PC.hyper_of(form),
                 PC.scalars_of(form))
    bp, bs = P.update_bounds(r)
    assert np.all(np.isfinite(r.p))
    w = [_note("%s %s p" % (key, form), after["p"][idx], r.p, bp)]
    for i in range(ns):
        w.append(_note("%s %s s%d" % (key, form, i), after["s%d" % i][idx], r.slots[i], bs[i]))
    assert max(w) <= 1.0, (key, form, w)
    for k in after:
        if k == "g" and not g_unchanged:
            continue
        used = k == "p" or (k[0] == "s" and int(k[1]) < ns)
        keep = ~idx if used else np.ones(idx.size, dtype=bool)
        assert np.array_equal(after[k].view(np.int32)[keep], host[k].view(np.int32)[keep]), (key, form, k, "stray write")
    # a zero gradient over zero state leaves the weight exactly where it was
    z = idx & (g_used == 0)
    for i in range(ns):
        z &= host["s%d" % i] == 0
    assert np.array_equal(after["p"][z], host["p"][z]), (key, form)
    return after


@pytest.mark.parametrize("form", PC.forms())
def test_optim_flat_blocks_ranges(form):
    """optim_kernel's flat blocks over every (lo, n): aligned, unaligned at both ends, tiny, and across
    a 1024-element block edge; non-default hyper-parameters, pre-filled state, hand-written scalars."""
    K = _K()
    st = _state(K, PC.scalars_of(form))
    for lo, n in PC.RANGES:
        P.check_case_fits({"optim": {"lo": lo, "n": n, "numel": PC.NUMEL}})
        host, bufs = _buffers(form, PC.NUMEL)
        K.optim(_optim_args(K, form, bufs, st, lo, n), K.PackTable(), _stream())
        torch.cuda.synchronize()
        idx = np.zeros(PC.NUMEL, dtype=bool)
        idx[lo:lo + n] = True
        _check_update("optim flat", form, host, bufs, idx, host["g"])


# routes of the flat-block test: (lo, hi, kind, KHW, Cin, Cout, Cs, Csb, NT, NTb, fwd, bwd)
ROUTES = [
    (2, 137, 1, 9, 3, 5, 4, 8, 1, 1, 64, 1152),            # conv, padded input, lo % 4 == 2: per-element stores
    (140, 716, 1, 9, 8, 8, 8, 8, 1, 1, 2752, 4352),        # conv, identity: float4 forward, 8-byte backward store
    (716, 1076, 2, 6, 5, 12, 8, 0, 1, 3, 5952, 7040),      # dense, padded input
]
ROUTE_ARENA = 8640
ROUTE_RANGES = [(0, PC.NUMEL), (2, 135), (0, 900), (140, 576), (137, 943)]


@pytest.mark.parametrize("form", ["adam", "sgd", "amsgrad"])
def test_optim_flat_blocks_write_their_pack_routes(form):
    """With routes, the arena equals the oracle's pack of the device's own updated master at every
    position an updated route element maps to (bit equality) and keeps its sentinel elsewhere --
    also for a launch range that ends in the middle of a route."""
    K = _K()
    st = _state(K, PC.scalars_of(form))
    rdev = _routes_dev(K, ROUTES)
    for lo, n in ROUTE_RANGES:
        P.check_case_fits({"optim": {"lo": lo, "n": n, "numel": PC.NUMEL},
                           "routes": {"routes": ROUTES, "arena_numel": ROUTE_ARENA, "max_routes": K.MAX_ROUTES,
                                      "master_numel": PC.NUMEL}})
        host, bufs = _buffers(form, PC.NUMEL, seed=1)
        arena = _abuf(ROUTE_ARENA)
        a = _optim_args(K, form, bufs, st, lo, n)
        a.arena, a.routes, a.nroutes = arena.data_ptr(), rdev.data_ptr(), len(ROUTES)
        K.optim(a, K.PackTable(), _stream())
        torch.cuda.synchronize()
        idx = np.zeros(PC.NUMEL, dtype=bool)
        idx[lo:lo + n] = True
        after = _check_update("optim routes", form, host, bufs, idx, host["g"])
        exp = P.route_expect(ROUTES, after["p"], np.full(ROUTE_ARENA, A_SENTINEL, dtype=np.uint16), lo, lo + n)
        assert (exp != A_SENTINEL).sum() > 0
        assert np.array_equal(_u16(arena), exp), (form, lo, n)


def _tile_routes():
    routes, lo, off = [], 0, 64
    for N, Kk in ((32, 8), (32, 24), (160, 8), (160, 24)):
        NT, NTb, KS, KSb = N // 16, P.cdiv(Kk, 16), P.cdiv(Kk, 32), N // 32
        fwd, bwd = off, off + KS * NT * 512 + 64
        off = bwd + KSb * NTb * 512 + 64
        routes.append((lo, lo + N * Kk, 2, Kk // 8, 8, N, 8, 0, NT, NTb, fwd, bwd))
        lo += N * Kk
    return routes, lo, off


def _set_tiles(a, routes):
    """The tile blocks of a launch over [a.lo, a.lo + a.n), as the executor lays them out."""
    span = a.lo + a.n - (a.lo & ~3)
    b0 = 0
    for i, rt in enumerate(routes):
        a.set_tile(i, i, b0)
        b0 += ((rt[1] - rt[0]) // rt[5] // 8) * P.cdiv(rt[5], 128)
    a.set_tile(len(routes), 0, b0)
    a.ntile, a.flat_blocks = len(routes), P.cdiv(P.cdiv(span, 4), 256)


@pytest.mark.parametrize("form,clipvalue", [("adam", 0.0), ("amsgrad", 0.0), ("sgd_nesterov", 0.0), ("rmsprop", 0.0),
                                            ("adam", 0.05)])
def test_optim_tile_blocks_equal_the_flat_blocks(form, clipvalue):
    """Dense routes N in {32, 160} x K in {8, 24} updated by tile blocks (N = 160: a second column
    block of which one wave has work): master, state and arena bit-identical to the flat launch and
    inside the oracle's bounds; clipvalue: the same through optim_clip_kernel."""
    K = _K()
    routes, used, arena_numel = _tile_routes()
    numel = P.cdiv(used + 1, 64) * 64
    P.check_case_fits({"optim": {"lo": 0, "n": used, "numel": numel},
                       "routes": {"routes": routes, "arena_numel": arena_numel, "max_routes": K.MAX_ROUTES,
                                  "master_numel": numel, "tiled": range(4)}})
    st = _state(K, PC.scalars_of(form))
    rdev = _routes_dev(K, routes)
    res = []
    for tiled in (False, True):
        host, bufs = _buffers(form, numel, seed=2)
        arena = _abuf(arena_numel)
        a = _optim_args(K, form, bufs, st, 0, used, clipvalue)
        a.arena, a.routes, a.nroutes = arena.data_ptr(), rdev.data_ptr(), len(routes)
        if tiled:
            _set_tiles(a, routes)
        K.optim(a, K.PackTable(), _stream())
        torch.cuda.synchronize()
        idx = np.arange(numel) < used
        g_used = C.clip(host["g"], None, clipvalue)[0].astype(np.float32) if clipvalue else host["g"]
        if clipvalue:
            assert (np.abs(host["g"][idx]) > clipvalue).sum() > 100
        after = _check_update("optim %s%s" % ("tile" if tiled else "flat", " clip" if clipvalue else ""), form, host,
                              bufs, idx, g_used)
        exp = P.route_expect(routes, after["p"], np.full(arena_numel, A_SENTINEL, dtype=np.uint16))
        assert np.array_equal(_u16(arena), exp), (form, tiled)
        res.append((bufs, arena))
    for k in res[0][0]:
        assert _same_bits(res[0][0][k], res[1][0][k]), (form, k, "tile != flat")
    assert torch.equal(res[0][1].view(torch.int16), res[1][1].view(torch.int16))


# =============================================================================== reduction + update
def _reduce_optim_case(K, form, S, names=None, grad_only=False):
    descs, numel = PC.red_descs(S, -1, names=names)
    slab = PC.red_slab(descs, numel, "int", seed=S)
    P.check_case_fits({"red": {"descs": descs, "slab_numel": numel, "grad_numel": PC.GRAD_NUMEL,
                               "state_numel": PC.GRAD_NUMEL},
                       "optim": {"lo": 0, "n": PC.GRAD_NUMEL, "numel": PC.GRAD_NUMEL}})
    slab_t = _dev(slab)
    tab = _table(K, descs, slab_t)
    host, bufs = _buffers(form, PC.GRAD_NUMEL, seed=3, g=np.full(PC.GRAD_NUMEL, F_SENTINEL, dtype=np.int32).view(np.float32))
    st = _state(K, PC.scalars_of(form))
    a = _optim_args(K, form, bufs, st, 0, PC.GRAD_NUMEL)
    a.grad_only = int(grad_only)
    return descs, slab, slab_t, tab, host, bufs, st, a


def _exact_grad(descs, slab):
    g = np.full(PC.GRAD_NUMEL, F_SENTINEL, dtype=np.int32).view(np.float32).copy()
    idx = np.zeros(PC.GRAD_NUMEL, dtype=bool)
    for d in descs:
        g[d.dst_off:d.dst_off + d.numel] = P.slab_sum_exact(slab, d).astype(np.float32)
        idx[d.dst_off:d.dst_off + d.numel] = True
    return g, idx


@pytest.mark.parametrize("form", PC.forms())
def test_reduce_optim_fused(form):
    """reduce_optim_kernel over the float4 and scalar descriptors at S in {1, 9, 17}, integer slabs:
    the gradient written is exact, master and state inside the oracle's bounds, nothing else touched;
    Adagrad, Adamax and AMSGrad bit-identical to slab_reduce followed by optim_kernel."""
    K = _K()
    with _Lanes(K, RED_LANES):
        for S in (1, 9, 17):
            descs, slab, slab_t, tab, host, bufs, st, a = _reduce_optim_case(K, form, S)
            assert [tab.flags(i)[1] for i in range(6)] == [0, 1, 0, 1, 0, 1]
            K.reduce_optim(bufs["g"].data_ptr(), tab, a, _stream())
            torch.cuda.synchronize()
            g, idx = _exact_grad(descs, slab)
            assert np.array_equal(_np(bufs["g"]).view(np.int32), g.view(np.int32)), (form, S, "gradient")
            _check_update("reduce_optim", form, host, bufs, idx, np.where(idx, g, 0).astype(np.float32), g_unchanged=False)
            if PC.form_kind(form) in ("adagrad", "adamax", "amsgrad"):
                host2, bufs2 = _buffers(form, PC.GRAD_NUMEL, seed=3, g=host["g"])
                K.slab_reduce(bufs2["g"].data_ptr(), 0, PC.GRAD_NUMEL, tab, _stream())
                for d in descs:
                    K.optim(_optim_args(K, form, bufs2, st, d.dst_off, d.numel), K.PackTable(), _stream())
                torch.cuda.synchronize()
                for k in bufs:
                    assert _same_bits(bufs[k], bufs2[k]), (form, S, k, "fused != reduce + optim")


def test_reduce_optim_grad_only_leaves_master_and_state():
    K = _K()
    with _Lanes(K, RED_LANES):
        for form in ("adam", "amsgrad"):
            descs, slab, slab_t, tab, host, bufs, st, a = _reduce_optim_case(K, form, 9, grad_only=True)
            K.reduce_optim(bufs["g"].data_ptr(), tab, a, _stream())
            torch.cuda.synchronize()
            g, _ = _exact_grad(descs, slab)
            assert np.array_equal(_np(bufs["g"]).view(np.int32), g.view(np.int32))
            for k in ("p", "s0", "s1", "s2"):
                assert np.array_equal(_np(bufs[k]).view(np.int32), host[k].view(np.int32)), (form, k)


@pytest.mark.parametrize("N,numel", [(n, e) for n in (16, 32, 128) for e in (1024, 2048)])
def test_reduce_optim_tiled_dense_blocks(N, numel):
    """An identity RED_FLATW descriptor whose blocks are whole 8-row groups (tile) with a dense route:
    update_vec4 stages the block's bf16 weights and writes whole pack vectors, forward and backward."""
    K = _K()
    Kk, lo = numel // N, 64
    NT, NTb, KS, KSb = P.cdiv(N, 16), P.cdiv(Kk, 16), P.cdiv(Kk, 32), P.cdiv(N, 32)
    fwd = 64
    bwd = fwd + KS * NT * 512 + 64
    arena_numel = bwd + KSb * NTb * 512 + 64
    rt = (lo, lo + numel, 2, Kk // 8, 8, N, 8, 0, NT, NTb, fwd, bwd)
    total = lo + numel + 64
    with _Lanes(K, RED_LANES):
        for form in ("adam", "amsgrad"):
            for S in (1, 9):
                d = P.red_desc(P.RED_FLATW, S, numel + 8, ld=N, dst_off=lo, KH=Kk // 8, KW=1, Cin=8, Cout=N, Cs=8)
                d.name = "tiled"
                slab_numel = S * d.stride_s + 8
                P.check_case_fits({"red": {"descs": [d], "slab_numel": slab_numel, "grad_numel": total, "state_numel": total},
                                   "optim": {"lo": lo, "n": numel, "numel": total},
                                   "routes": {"routes": [rt], "arena_numel": arena_numel, "max_routes": K.MAX_ROUTES,
                                              "master_numel": total}})
                slab = PC.red_slab([d], slab_numel, "int", seed=S)
                slab_t = _dev(slab)
                tab = _table(K, [d], slab_t)
                assert tab.flags(0)[:3] == (1, 1, 1), tab.flags(0)
                host, bufs = _buffers(form, total, seed=4, g=np.full(total, F_SENTINEL, dtype=np.int32).view(np.float32))
                arena, rdev = _abuf(arena_numel), _routes_dev(K, [rt])
                a = _optim_args(K, form, bufs, _state(K, PC.scalars_of(form)), lo, numel)
                a.arena, a.routes, a.nroutes = arena.data_ptr(), rdev.data_ptr(), 1
                K.reduce_optim(bufs["g"].data_ptr(), tab, a, _stream())
                torch.cuda.synchronize()
                g = host["g"].copy()
                g[lo:lo + numel] = P.slab_sum_exact(slab, d).astype(np.float32)
                idx = (np.arange(total) >= lo) & (np.arange(total) < lo + numel)
                assert np.array_equal(_np(bufs["g"]).view(np.int32), g.view(np.int32))
                after = _check_update("reduce_optim tile", form, host, bufs, idx, np.where(idx, g, 0).astype(np.float32),
                                      g_unchanged=False)
                exp = P.route_expect([rt], after["p"], np.full(arena_numel, A_SENTINEL, dtype=np.uint16))
                assert np.array_equal(_u16(arena), exp), (form, N, numel, S)


# =============================================================================== pack_kernel
def _run_pack(K, adds, master, arena_numel):
    tab = K.PackTable()
    for ad in adds:
        tab.add(*ad)
    m, arena = _dev(master), _abuf(arena_numel)
    K.pack(m.data_ptr(), arena.data_ptr(), tab, _stream())
    torch.cuda.synchronize()
    assert np.array_equal(_np(m).view(np.int32), master.view(np.int32))
    return _u16(arena)


def test_pack_kernel_conv_descriptors():
    """Forward and dgrad packs of the four conv shapes in one table: the arena as uint16 equals the
    oracle (layout, zero padding, tap flip, the Cs == 4 vector across two taps, nearest-even
    rounding of ties, large values and fp32 subnormals); sentinels beyond each pack are untouched."""
    K = _K()
    adds, conv, exp_parts, src, dst = [], [], [], 3, 64
    for KH, KW, Cin, Cs, Cout, Cso in PC.PACK_CONVS:
        n = KH * KW * Cin * Cout
        for type, cs, NT in ((P.PACK_CONV_FWD, Cs, P.cdiv(Cout, 16)), (P.PACK_CONV_DGRAD, Cso, P.cdiv(Cs, 16))):
            adds.append((src, n, type, KH, KW, Cin, Cout, cs, NT, dst))
            conv.append((src, type, KH * KW, Cin, Cout, cs, NT, dst))
            exp_parts.append((src, n, type, (KH * KW, Cin, Cout), cs, NT, dst))
            dst += P.cdiv(KH * KW * cs, 32) * NT * 512 + 64
        src += n + 5
    master = PC.pack_master(src + 8)
    P.check_case_fits({"packs": {"conv": conv, "master_numel": master.size, "arena_numel": dst}})
    exp = np.full(dst, A_SENTINEL, dtype=np.uint16)
    for s0, n, type, shape, cs, NT, d0 in exp_parts:
        w = master[s0:s0 + n].reshape(shape)
        pack, idx = (P.conv_fwd_pack if type == P.PACK_CONV_FWD else P.conv_dgrad_pack)(w, cs, NT)
        exp[d0:d0 + pack.size] = pack
        assert idx.size < pack.size                                 # (every pack has padding to check)
    got = _run_pack(K, adds, master, dst)
    assert np.array_equal(got, exp), np.flatnonzero(got != exp)[:8]


@pytest.mark.parametrize("with_bwd", [True, False])
def test_pack_kernel_dense_pairs(with_bwd):
    K = _K()
    adds, dense, exp_parts, src, dst = [], [], [], 2, 64
    for pixels, Cin, Cs, N in PC.PACK_DENSES:
        n = pixels * Cin * N
        NT, NTb = P.cdiv(N, 16), P.cdiv(pixels * Cs, 16)
        fwd = dst
        dst += P.cdiv(pixels * Cs, 32) * NT * 512 + 64
        adds.append((src, n, P.PACK_DENSE_FWD, pixels, 1, Cin, N, Cs, NT, fwd))
        bwd = -1
        if with_bwd:
            bwd = dst
            dst += P.cdiv(N, 32) * NTb * 512 + 64
            adds.append((src, n, P.PACK_DENSE_BWD, pixels, 1, Cin, N, Cs, NTb, bwd))
        dense.append((src, pixels, Cin, Cs, N, NT, fwd, NTb, bwd))
        exp_parts.append((src, n, pixels, Cin, Cs, N, NT, fwd, NTb, bwd))
        src += n + 3
    master = PC.pack_master(src + 8, seed=1)
    P.check_case_fits({"packs": {"dense": dense, "master_numel": master.size, "arena_numel": dst}})
    exp = np.full(dst, A_SENTINEL, dtype=np.uint16)
    for s0, n, pixels, Cin, Cs, N, NT, fwd, NTb, bwd in exp_parts:
        w = master[s0:s0 + n].reshape(pixels * Cin, N)
        pack, _ = P.dense_fwd_pack(w, Cin, Cs, NT)
        exp[fwd:fwd + pack.size] = pack
        if bwd >= 0:
            pack, _ = P.dense_bwd_pack(w, Cin, Cs, NTb)
            exp[bwd:bwd + pack.size] = pack
    got = _run_pack(K, adds, master, dst)
    assert np.array_equal(got, exp), np.flatnonzero(got != exp)[:8]


# =============================================================================== step scalars
def _opt(kind):
    kw = {} if kind == "nadam" else {"decay": 0.01}
    if kind in ("adam", "adamax", "nadam", "amsgrad"):
        kw["beta_1"] = 0.8
    if kind == "nadam":
        kw["schedule_decay"] = 0.01
    if kind == "amsgrad":
        return optim.Adam(amsgrad=True, **kw)
    return {"sgd": optim.SGD, "rmsprop": optim.RMSprop, "adagrad": optim.Adagrad, "adadelta": optim.Adadelta,
            "adam": optim.Adam, "adamax": optim.Adamax, "nadam": optim.Nadam}[kind](**kw)


@pytest.mark.parametrize("kind", ["sgd", "rmsprop", "adagrad", "adadelta", "adam", "adamax", "nadam", "amsgrad"])
def test_step_scalars(kind):
    """One training step of the smallest model at iterations = t - 1 for t in {1, 2, 1000, 50000}:
    lr_eff, s[0..5] and m_schedule read back from the device state against the float64 oracle
    (Keras decay, Adam / AMSGrad / Adamax bias correction, Nadam's momentum schedule)."""
    set_random_seed(11)
    o = _opt(kind)
    m = zoo.rpv_cnn((16, 16, 3), conv_sizes=[4, 8, 8], fc_sizes=[16], dropout=0.0, optimizer=o, lr=None, device="cuda")
    ex = m._executor
    K = ex.K
    rs = np.random.RandomState(0)
    d = ex.upload(rs.rand(8, 16, 16, 3).astype(np.float32), (rs.rand(8) > 0.5).astype(np.float32))
    perm = torch.arange(d.n, device=ex.device)
    lr = float(ex.opt.lr)
    for t in (1, 2, 1000, 50000):
        ex.set_optimizer_state(t - 1, [])
        ms0 = P.nadam_m_schedule(t - 1, 0.8, 0.01) if kind == "nadam" else 1.0
        ex._st_f64[K.STEP_STATE_MSCHED_OFFSET // 8] = ms0
        ex.train_step(d, perm, 0, 8)
        torch.cuda.synchronize()
        o4 = K.STEP_STATE_LR_OFFSET // 4
        f = np.zeros(K.STEP_STATE_BYTES // 4)
        f[o4:o4 + 8] = ex._st_f32[o4:o4 + 8].cpu().numpy()          # lr, lr_eff, s[0..5]
        assert int(ex._st_i32[0]) == t
        lr_eff, s, ms1 = P.step_scalars(kind, t, lr, getattr(o, "initial_decay", 0.0), getattr(o, "beta_1", 0.9),
                                        getattr(o, "beta_2", 0.999), getattr(o, "schedule_decay", 0.004), ms0)
        got = [f[K.STEP_STATE_LR_OFFSET // 4 + 1]] + list(f[K.STEP_STATE_S_OFFSET // 4:K.STEP_STATE_S_OFFSET // 4 + 6])
        for name, a, b in zip(["lr_eff"] + ["s%d" % i for i in range(6)], got, [lr_eff] + s):
            if b is None:
                continue
            w = _note("step scalars %s" % kind, np.array([a]), np.array([b]), np.array([P.scalar_bound(b)]))
            assert w <= 1.0, (kind, t, name, a, b)
        if kind == "nadam":
            got_ms = float(ex._st_f64[K.STEP_STATE_MSCHED_OFFSET // 8])
            assert abs(got_ms - ms1) <= 1e-12 * abs(ms1), (t, got_ms, ms1)
            assert ms1 != ms0 or t > 2          # (the product underflows long before step 50000)
        if t > 1 and kind != "nadam":
            assert lr_eff < lr

"""CPU proof that the checker of tests/test_param_path_gpu.py can fail and that its bounds are
attainable: an fp32 NumPy evaluation of every formula (each operation rounded to float32, once
with separate multiply and add, once with the products fused) stays inside the oracle's bounds at
every input the GPU tests use, and every listed mutation of a formula or an index map is flagged
at those inputs.  Also: frag_index is a bijection, and the oracle agrees with the project's CPU
reference (ops/reference.py) -- that last one checks the reference, not the oracle."""
import numpy as np
import pytest
import torch

from helpers import clip_oracle as C
from helpers import param_cases as PC
from helpers import param_oracle as P

F = np.float32


# ------------------------------------------------------------------------------- fp32 emulation
def _mad(a, b, c, fused):
    """a * b + c in fp32: two roundings, or one (the product exact in float64)."""
    if fused:
        return (a.astype(np.float64) * np.float64(b) + c.astype(np.float64)).astype(F)
    return (F(b) * a + c).astype(F)


def emu_update(kind, p, g, slots, hp, s, fused=False, mut=None):
    """optim_math.h's opt_update in float32 NumPy, operation by operation; ``mut``: one of the
    mutations below.  Returns (p, [slots])."""
    p, g = p.astype(F), g.astype(F)
    sl = [x.astype(F) for x in slots]
    s = [F(x) for x in s]
    b1, b2, eps, rho, mom = F(hp.beta1), F(hp.beta2), F(hp.eps), F(hp.rho), F(hp.momentum)
    one = F(1.0)
    gs = g if mut == "grad_scale_ignored" else g * F(hp.grad_scale)

    def first(m0):                     # m = b1 m0 + (1 - b1) g
        bb = b2 if mut == "beta2_for_m" else b1
        t2 = gs if mut == "factor_dropped" else (one - bb) * gs
        return _mad(m0, bb, t2, fused)

    def second(v0, r):                 # v = r v0 + (1 - r) g g
        t2 = gs * gs if mut == "factor_dropped" else ((one - r) * gs) * gs
        return _mad(v0, r, t2, fused)

    def den(v):
        return np.sqrt(v + eps) if mut == "eps_in_sqrt" else np.sqrt(v) + eps

    if kind == "sgd":
        lr = s[0]
        if hp.momentum:
            v = _mad(sl[0], mom, -(lr * gs), fused)
            if hp.nesterov and mut != "nesterov_ignored":
                return p + _mad(v, mom, -(lr * gs), fused), [v]
            return p + v, [v]
        return _mad(-gs, lr, p, fused), sl
    if kind == "rmsprop":
        a = second(sl[0], rho)
        return p - s[0] * gs / den(a), [a]
    if kind == "adagrad":
        a = _mad(gs, gs, sl[0], fused)
        return p - s[0] * gs / den(a), [a]
    if kind == "adadelta":
        a = second(sl[0], rho)
        upd = gs * np.sqrt(sl[1] + eps) / np.sqrt((sl[0] if mut == "adadelta_old_acc" else a) + eps)
        d = _mad(sl[1], rho, ((one - rho) * upd) * upd, fused)
        return _mad(-upd, s[0], p, fused), [a, d]
    if kind == "adam":
        m, v = first(sl[0]), second(sl[1], b2)
        return p - s[0] * m / den(v), [m, v]
    if kind == "amsgrad":
        m, v = first(sl[0]), second(sl[1], b2)
        vh = np.maximum(sl[2], v)
        return p - s[0] * m / den(v if mut == "amsgrad_v" else vh), [m, v, vh]
    if kind == "adamax":
        m = first(sl[0])
        u = np.maximum(sl[1] if mut == "adamax_no_beta2" else b2 * sl[1], np.abs(gs))
        return p - s[0] * m / (u + eps), [m, u]
    if kind == "nadam":
        gp = gs * s[2]
        m, v = first(sl[0]), second(sl[1], b2)
        mp, vp = m * s[3], v * s[4]
        mbar = _mad(gp, one - s[0], (s[0] if mut == "nadam_mc_t_both" else s[1]) * mp, fused)
        return p - s[5] * mbar / den(vp), [m, v]
    raise ValueError(kind)


def _outside(got, ref, bound):
    """Elements outside the bound (a NaN counts as outside)."""
    return ~(np.abs(np.asarray(got, dtype=np.float64) - ref) <= bound)


def _check_update(form, got_p, got_s, p, g, slots, hp, s):
    """True when some element of p or of a slot is outside the oracle's bound."""
    r = P.update(PC.form_kind(form), p, g, slots, hp, s)
    bp, bs = P.update_bounds(r)
    bad = bool(_outside(got_p, r.p, bp).any())
    for a, b, c in zip(got_s, r.slots, bs):
        bad = bad or bool(_outside(a, b, c).any())
    return bad


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("form", PC.forms())
def test_fp32_updates_stay_inside_the_bounds(form, fused):
    hp, s = PC.hyper_of(form), PC.scalars_of(form)
    for seed in range(3):
        p, g, slots = PC.optim_inputs(form, seed=seed)
        gp, gsl = emu_update(PC.form_kind(form), p, g, slots, hp, s, fused)
        r = P.update(PC.form_kind(form), p, g, slots, hp, s)
        bp, bs = P.update_bounds(r)
        assert np.all(np.isfinite(r.p)) and np.all(np.isfinite(gp))
        assert not _outside(gp, r.p, bp).any(), (form, float((np.abs(gp - r.p) / bp).max()))
        for k, (a, b, c) in enumerate(zip(gsl, r.slots, bs)):
            ok = ~_outside(a, b, c)
            assert ok.all(), (form, k, int((~ok).sum()))


UPDATE_MUTATIONS = {
    "eps_in_sqrt": ["rmsprop", "adagrad", "adam", "nadam", "amsgrad"],
    "beta2_for_m": ["adam", "nadam", "adamax", "amsgrad"],
    "factor_dropped": ["rmsprop", "adadelta", "adam", "nadam", "adamax", "amsgrad"],
    "nesterov_ignored": ["sgd_nesterov"],
    "grad_scale_ignored": PC.forms(),
    "adamax_no_beta2": ["adamax"],
    "amsgrad_v": ["amsgrad"],
    "adadelta_old_acc": ["adadelta"],
    "nadam_mc_t_both": ["nadam"],
}


@pytest.mark.parametrize("mut,form", [(m, f) for m, fs in UPDATE_MUTATIONS.items() for f in fs])
def test_update_mutations_are_flagged(mut, form):
    hp, s = PC.hyper_of(form), PC.scalars_of(form)
    p, g, slots = PC.optim_inputs(form)
    for fused in (False, True):
        gp, gsl = emu_update(PC.form_kind(form), p, g, slots, hp, s, fused, mut)
        assert _check_update(form, gp, gsl, p, g, slots, hp, s), (mut, form, fused)
    # ... and at the smallest ranges the GPU test launches: the mutation shows inside (0, 64) alone
    gp, gsl = emu_update(PC.form_kind(form), p[:64], g[:64], [x[:64] for x in slots], hp, s, False, mut)
    assert _check_update(form, gp, gsl, p[:64], g[:64], [x[:64] for x in slots], hp, s), (mut, form)


def test_zero_gradient_over_zero_state_is_finite_and_exact():
    for form in PC.forms():
        hp, s = PC.hyper_of(form), PC.scalars_of(form)
        p, g, slots = PC.optim_inputs(form)
        z = np.arange(p.size) % 16 == 3
        assert not g[z].any() and not any(x[z].any() for x in slots)
        r = P.update(PC.form_kind(form), p, g, slots, hp, s)
        assert np.array_equal(r.p[z], p[z].astype(np.float64)), form
        nz = np.arange(p.size) % 16 == 7          # zero gradient over non-zero state
        assert not g[nz].any() and all(x[nz].any() for x in slots)


def test_inputs_decide_the_maxima_both_ways():
    hp = PC.hyper_of("amsgrad")
    p, g, sl = PC.optim_inputs("amsgrad")
    r = P.update("amsgrad", p, g, sl, hp, PC.scalars_of("amsgrad"))
    live = sl[2] > 0
    assert (r.slots[2][live] > r.slots[1][live]).sum() > 100 and (r.slots[2][live] == r.slots[1][live]).sum() > 100
    p, g, sl = PC.optim_inputs("adamax")
    gs = np.abs(g.astype(np.float64) * hp.grad_scale)
    bu = hp.beta2 * sl[1].astype(np.float64)
    live = (g != 0) & (sl[1] > 0)
    assert (bu[live] > gs[live]).sum() > 100 and (bu[live] < gs[live]).sum() > 100


# ------------------------------------------------------------------------------- step scalars
STEPS = [1, 2, 1000, 50000]
SCALAR_KINDS = ["sgd", "rmsprop", "adagrad", "adadelta", "adam", "adamax", "nadam", "amsgrad"]


def _scalar_case(kind, t, mut=None):
    decay = 0.0 if kind == "nadam" or mut == "decay_ignored" else 0.01
    tt = t - 1 if mut == "bias_t_minus_1" else t
    ms = P.nadam_m_schedule(t - 1, 0.8, 0.01)
    lr_eff, s, ms1 = P.step_scalars(kind, tt, 1e-3, decay, 0.8, 0.999, 0.01, ms)
    if mut == "bias_t_minus_1":       # the decay of step t, the bias correction of step t - 1
        lr_t = P.step_scalars(kind, t, 1e-3, decay)[0]
        s = [None if x is None else x * lr_t / lr_eff for x in s] if kind != "nadam" else s
        lr_eff = lr_t
    return lr_eff, s, ms1


def _scalars_differ(a, b):
    va = [a[0]] + [x for x in a[1] if x is not None]
    vb = [b[0]] + [x for x in b[1] if x is not None]
    return any(abs(float(F(x)) - y) > P.scalar_bound(y) for x, y in zip(va, vb))


def test_float_stored_scalars_are_inside_their_bound():
    for kind in SCALAR_KINDS:
        for t in STEPS:
            ref = _scalar_case(kind, t)
            assert not _scalars_differ(ref, ref), (kind, t)       # rounding to float alone passes


def test_scalar_mutations_are_flagged():
    for kind in ["adam", "adamax", "amsgrad"]:
        assert any(_scalars_differ(_scalar_case(kind, t, "bias_t_minus_1"), _scalar_case(kind, t)) for t in STEPS[1:]), kind
    for kind in [k for k in SCALAR_KINDS if k != "nadam"]:
        for t in STEPS[1:]:
            assert _scalars_differ(_scalar_case(kind, t, "decay_ignored"), _scalar_case(kind, t)), (kind, t)
    # Nadam: the schedule of step t - 1
    for t in STEPS[1:3]:
        assert _scalars_differ(_scalar_case("nadam", t, "bias_t_minus_1"), _scalar_case("nadam", t)), t


def test_nadam_from_scalars_is_keras_nadam():
    """The scalar form the kernel uses against the closed Keras form of helpers/clip_oracle.py."""
    p, g, sl = PC.optim_inputs("nadam")
    for t in (1, 2, 7):
        ms = P.nadam_m_schedule(t - 1, 0.8, 0.01)
        _, s, _ = P.step_scalars("nadam", t, 2e-3, 0.0, 0.8, 0.95, 0.01, ms)
        a = P.nadam_from_scalars(p, g, sl[0], sl[1], s, P.f32(0.8), P.f32(0.95), 1e-3)
        b = C.nadam(p, g, sl[0], sl[1], t, P.f32(2e-3), P.f32(0.8), P.f32(0.95), 1e-3, P.f32(0.01))
        for x, y in zip(a, b):
            assert np.allclose(x, y, rtol=1e-11, atol=0)


# ------------------------------------------------------------------------------- slab reduction
def emu_reduce(x, tpe):
    """reduce_body.h's summation order in float32: x [S, n] -> [n]."""
    S, n = x.shape
    part = []
    for lane in range(tpe):
        a = np.zeros((8, n), dtype=F)
        s = lane
        while s + 7 * tpe < S:
            for u in range(8):
                a[u] += x[s + u * tpe]
            s += 8 * tpe
        for u in range(7):
            if s + u * tpe < S:
                a[u] += x[s + u * tpe]
        part.append(((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7])))
    off = tpe >> 1
    while off > 0:
        for lane in range(off):
            part[lane] = part[lane] + part[lane + off]
        off >>= 1
    return part[0]


@pytest.mark.parametrize("tpe", PC.TPES)
def test_fp32_reduction_stays_inside_the_bound_and_is_exact_on_integers(tpe):
    for S in PC.s_list(tpe):
        descs, numel = PC.red_descs(S, tpe)
        for mode in ("int", "normal"):
            slab = PC.red_slab(descs, numel, mode, seed=S)
            for d in descs:
                x = P.slab_gather(slab, d)
                assert np.isfinite(x).all()
                got = emu_reduce(x, tpe)
                seq = np.zeros(d.numel, dtype=F)
                for s in range(S):
                    seq = seq + x[s]
                if mode == "int":
                    ref = P.slab_sum_exact(slab, d)
                    assert np.abs(x).sum(0).max() < 2 ** 24
                    assert np.array_equal(got.astype(np.int64), ref) and np.array_equal(seq.astype(np.int64), ref)
                else:
                    ref, A = P.slab_sum(slab, d)
                    b = P.slab_bound(S, A)
                    assert not _outside(got, ref, b).any() and not _outside(seq, ref, b).any(), (d.name, S)


def _mut_src(d, mut):
    kw = dict(vars(d))
    if mut == "cin_for_cs":
        kw["Cs"] = d.Cin
    m = P.red_desc(**{k: kw[k] for k in ("type", "S", "stride_s", "ld", "dst_off", "numel", "KH", "KW", "Cin", "Cout",
                                         "Cs", "tpe", "slab_off")})
    if mut == "ci_co_swapped":
        tap, ci, co = np.meshgrid(np.arange(d.KH * d.KW), np.arange(d.Cin), np.arange(d.Cout), indexing="ij")
        return ((tap * d.Cs + co) * d.ld + ci).reshape(-1)
    return P.red_src(m)


@pytest.mark.parametrize("tpe", [1, 4, 64])
def test_reduction_mutations_are_flagged(tpe):
    for S in PC.s_list(tpe):
        descs, numel = PC.red_descs(S, tpe)
        for mode in ("int", "normal"):
            slab = PC.red_slab(descs, numel, mode, seed=S)
            for d in descs:
                x = P.slab_gather(slab, d)
                ref, A = P.slab_sum(slab, d)
                bound = P.slab_bound(S, A) if mode == "normal" else np.zeros_like(A)
                muts = {"twice": np.concatenate([x, x[:1]])}
                if S > 1:
                    muts["last_dropped"] = x[:-1]
                if S > 8 * tpe:
                    muts["slab_8tpe_dropped"] = np.delete(x, 8 * tpe, axis=0)
                for name, xm in muts.items():
                    assert _outside(emu_reduce(xm, tpe), ref, bound).any(), (name, d.name, S, mode)
                for name in ("cin_for_cs", "ci_co_swapped"):
                    if d.type == P.RED_BIAS or (name == "cin_for_cs" and d.Cin == d.Cs):
                        continue
                    if name == "ci_co_swapped" and d.type != P.RED_CONVW:
                        continue
                    idx = d.slab_off + _mut_src(d, name)
                    xm = np.stack([slab[idx + s * d.stride_s] for s in range(S)])
                    assert _outside(emu_reduce(xm, tpe), ref, bound).any(), (name, d.name, S, mode)


def test_unread_slab_positions_are_nan():
    descs, numel = PC.red_descs(9)
    slab = PC.red_slab(descs, numel, "normal")
    mask = P.slab_read_mask(numel, descs)
    assert np.isnan(slab[~mask]).all() and np.isfinite(slab[mask]).all() and (~mask).sum() > 1000
    d = {x.name: x for x in descs}["conv_padded"]
    src = set(P.red_src(d).tolist())
    assert (3 * 16 + 0) not in src and 5 not in src and d.stride_s - 1 not in src    # padded row, column >= Cout, gap


# ------------------------------------------------------------------------------- packs
@pytest.mark.parametrize("KS,NT", [(1, 1), (2, 1), (3, 2), (1, 9), (5, 3)])
def test_frag_index_is_a_bijection(KS, NT):
    k, n = np.meshgrid(np.arange(32 * KS), np.arange(16 * NT), indexing="ij")
    idx = P.frag_index(k, n, NT).reshape(-1)
    assert np.array_equal(np.sort(idx), np.arange(KS * NT * 512))
    # the documented layout, read the other way round
    for ks, nt, lane, j in [(0, 0, 0, 0), (KS - 1, NT - 1, 63, 7), (0, NT - 1, 17, 3), (KS - 1, 0, 46, 5)]:
        assert P.frag_index(32 * ks + 8 * (lane >> 4) + j, 16 * nt + (lane & 15), NT) == ((ks * NT + nt) * 64 + lane) * 8 + j


def test_bf16_rounding_is_nearest_even():
    one = F(1.0)
    assert P.bf16_rne(one + F(2.0 ** -8)) == 0x3F80                      # tie -> even (1)
    assert P.bf16_rne(one + F(3 * 2.0 ** -8)) == 0x3F82                  # tie -> even (1 + 2^-6)
    assert P.bf16_rne(-(one + F(3 * 2.0 ** -8))) == 0xBF82
    v = PC.pack_master(4096)
    t = torch.from_numpy(v).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(P.bf16_rne(v), t)
    assert np.isfinite(torch.from_numpy(v).to(torch.bfloat16).float().numpy()).all()
    sp = PC.special_values()
    assert (np.abs(sp[np.isfinite(sp)]) < 1.2e-38).sum() >= 5 and (np.abs(sp) > 3e38).sum() >= 4


def _conv_packs(shape, w, mut=None):
    KH, KW, Cin, Cs, Cout, Cso = shape
    NT, NTd = P.cdiv(Cout, 16), P.cdiv(Cs, 16)
    fwd, _ = P.conv_fwd_pack(w, Cs, NT)
    dg, _ = P.conv_dgrad_pack(w[::-1] if mut == "tap_not_flipped" else w, Cso, NTd)
    return fwd, dg


def _mutate_pack(build, w, mut):
    """A pack built with one of the pack mutations."""
    saved = P.bf16_rne, P.frag_index
    try:
        if mut == "truncation":
            P.bf16_rne = lambda x: (np.ascontiguousarray(np.asarray(x, dtype=F)).view(np.uint32) >> 16).astype(np.uint16)
        if mut == "lane_fields_swapped":
            def swapped(k, n, NT):
                k, n = np.asarray(k, dtype=np.int64), np.asarray(n, dtype=np.int64)
                lane = 4 * (n % 16) + (k % 32) // 8
                return ((k // 32 * NT + n // 16) * 64 + lane) * 8 + k % 8
            P.frag_index = swapped
        out = build(w)
    finally:
        P.bf16_rne, P.frag_index = saved
    return out


def test_pack_mutations_are_flagged():
    for shape in PC.PACK_CONVS:
        KH, KW, Cin, Cs, Cout, Cso = shape
        w = PC.pack_master(KH * KW * Cin * Cout).reshape(KH * KW, Cin, Cout)
        fwd, dg = _conv_packs(shape, w)
        for mut in ("truncation", "lane_fields_swapped"):
            f2, d2 = _mutate_pack(lambda x: _conv_packs(shape, x), w, mut)
            assert not np.array_equal(f2, fwd) and not np.array_equal(d2, dg), (mut, shape)
        if KH * KW > 1:
            assert not np.array_equal(_conv_packs(shape, w, "tap_not_flipped")[1], dg), shape
        # padding left non-zero: a pack that keeps a sentinel where nothing is written
        _, idx = P.conv_fwd_pack(w, Cs, P.cdiv(Cout, 16))
        dirty = np.full(fwd.size, 0x7FA5, dtype=np.uint16)
        dirty[idx] = fwd[idx]
        assert idx.size < fwd.size and not np.array_equal(dirty, fwd), shape
    for pixels, Cin, Cs, N in PC.PACK_DENSES:
        w = PC.pack_master(pixels * Cin * N).reshape(pixels * Cin, N)
        build = lambda x: (P.dense_fwd_pack(x, Cin, Cs, P.cdiv(N, 16))[0],
                           P.dense_bwd_pack(x, Cin, Cs, P.cdiv(pixels * Cs, 16))[0])
        fwd, bwd = build(w)
        for mut in ("truncation", "lane_fields_swapped"):
            f2, b2 = _mutate_pack(build, w, mut)
            assert not np.array_equal(f2, fwd) and not np.array_equal(b2, bwd), (mut, pixels, N)
        assert (fwd == 0).sum() >= fwd.size - w.size      # padding is zero


def test_route_expect_is_the_pack_of_the_range():
    rt = (2, 137, 1, 9, 3, 5, 4, 8, 1, 1, 64, 64 + 1024 + 64)
    w = PC.pack_master(192)
    arena0 = np.full(4096, 0x7FA5, dtype=np.uint16)
    full = P.route_expect([rt], w, arena0)
    part = P.route_expect([rt], w, arena0, 0, 60)
    fwd, idx = P.conv_fwd_pack(w[2:137].reshape(9, 3, 5), 4, 1)
    assert np.array_equal(full[64 + idx], fwd[idx]) and (full != 0x7FA5).sum() == 2 * 135
    assert (part != 0x7FA5).sum() == 2 * 58 and np.array_equal(part[part != 0x7FA5], full[part != 0x7FA5])
    P.check_case_fits({"routes": {"routes": [rt], "arena_numel": 4096, "max_routes": 8, "master_numel": 192}})
    with pytest.raises(AssertionError):
        P.check_case_fits({"routes": {"routes": [rt], "arena_numel": 2048, "max_routes": 8, "master_numel": 192}})


def test_check_case_fits_refuses_a_case_that_leaves_its_tensors():
    descs, numel = PC.red_descs(9)
    ok = {"red": {"descs": descs, "slab_numel": numel, "grad_numel": PC.GRAD_NUMEL, "state_numel": PC.GRAD_NUMEL}}
    P.check_case_fits(ok)
    for key, val in (("slab_numel", numel - 16), ("grad_numel", 4900)):
        bad = {"red": dict(ok["red"], **{key: val})}
        with pytest.raises(AssertionError):
            P.check_case_fits(bad)
    for lo, n in PC.RANGES:
        P.check_case_fits({"optim": {"lo": lo, "n": n, "numel": PC.NUMEL}})
    with pytest.raises(AssertionError):
        P.check_case_fits({"optim": {"lo": 2170, "n": 7, "numel": PC.NUMEL + 1}})
    with pytest.raises(AssertionError):
        P.check_case_fits({"optim": {"lo": 2170, "n": 7, "numel": 2172 // 64 * 64}})


# ------------------------------------------------------------------------------- the host's tile flag
def test_a_narrow_identity_dense_descriptor_is_not_tiled():
    """update_vec4's backward half splits a row into Cout / 8 vectors: RedTable.add must not mark a
    Cout = 4 identity RED_FLATW descriptor ``tile`` (host only: nothing is launched)."""
    from cori_intml_examples_amd.ops.hip import kernels
    K = kernels()
    for Cout, tile in ((4, 0), (8, 1), (16, 1), (128, 1), (256, 0)):
        tab = K.RedTable()
        K.set_red_lanes(16)
        try:
            tab.add(0, 1024 + 8, 1, Cout, 0, 1024, P.RED_FLATW, 1024 // Cout // 4, 1, 4, Cout, 4)
        finally:
            from cori_intml_examples_amd.utils.tune import tune
            K.set_red_lanes(int(tune("red_lanes")))
        tpe, vec4, got, blk0 = tab.flags(0)
        assert (tpe, vec4, blk0) == (1, 1, 0) and got == tile, (Cout, tab.flags(0))
    with pytest.raises(IndexError):
        tab.flags(1)


# ------------------------------------------------------------------------------- the CPU reference
def test_oracle_agrees_with_the_cpu_reference_at_default_hyper_parameters():
    from cori_intml_examples_amd.ops import reference as R
    t, lr = 3, P.f32(1e-3)
    b1, b2, sd = P.f32(0.9), P.f32(0.999), P.f32(0.004)

    def close(a, b, scale):
        return bool(np.all(np.abs(np.asarray(a) - b) <= 1e-12 * np.maximum(np.abs(b), scale)))

    for form in PC.forms():
        kind = PC.form_kind(form)
        mom, nest = ("momentum" in form or "nesterov" in form), "nesterov" in form
        rho = 0.9 if kind == "rmsprop" else 0.95
        hp = P.hyper(beta1=0.9, beta2=0.999, eps=1e-7, rho=rho, momentum=0.9 if mom else 0.0, nesterov=nest)
        p, g, slots = PC.optim_inputs(form)
        ms0 = P.nadam_m_schedule(t - 1, 0.9, 0.004)
        _, s, _ = P.step_scalars(kind, t, lr, 0.0, 0.9, 0.999, 0.004, ms0)
        s = [0.0 if x is None else x for x in s]
        r = P.update(kind, p, g, slots, hp, s)
        tp, tg = torch.from_numpy(p).double(), torch.from_numpy(g).double()
        ts = [torch.from_numpy(x).double() for x in slots]
        if kind == "sgd":
            R.sgd_update(tp, tg, ts[0] if ts else None, lr, hp.momentum, nest)
        elif kind == "rmsprop":
            R.rmsprop_update(tp, tg, ts[0], lr, hp.rho, hp.eps)
        elif kind == "adagrad":
            R.adagrad_update(tp, tg, ts[0], lr, hp.eps)
        elif kind == "adadelta":
            R.adadelta_update(tp, tg, ts[0], ts[1], lr, hp.rho, hp.eps)
        elif kind == "adam":
            R.adam_update(tp, tg, ts[0], ts[1], t, lr, b1, b2, hp.eps)
        elif kind == "amsgrad":
            R.amsgrad_update(tp, tg, ts[0], ts[1], ts[2], t, lr, b1, b2, hp.eps)
        elif kind == "adamax":
            R.adamax_update(tp, tg, ts[0], ts[1], t, lr, b1, b2, hp.eps)
        else:
            R.nadam_update(tp, tg, ts[0], ts[1], t, lr, ms0, b1, b2, hp.eps, sd)
        assert close(tp.numpy(), r.p, r.D), form
        for a, b, m in zip(ts, r.slots, r.M):
            assert close(a.numpy(), b, m), form

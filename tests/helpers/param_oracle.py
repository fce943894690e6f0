"""Float64 / exact-integer oracle of the kernels that turn gradients into the next step's weights:
the deterministic slab reduction, the eight Keras 2.2.4 optimizer updates, the step bookkeeping
scalars and the bf16 fragment-major weight packs -- with DERIVED per-element bounds.

Written from the Keras formulas (keras/optimizers.py) and from the layout comments of
csrc/kernels/args.h, common.h and optim_math.h, not from ops/reference.py or the executor, which
tests/test_param_oracle.py checks against it.  NumPy only.

Notation: ``U = 2**-24`` is the fp32 unit roundoff, ``gamma(c) = c U / (1 - c U)`` bounds the
relative error of a value that went through c roundings (Higham, Accuracy and Stability, lemma
3.1).  A fused multiply-add removes a rounding and never adds one, so every count below holds
whatever the compiler contracts.  sqrt of a value with relative error gamma(c) has relative error
<= gamma(ceil(c / 2)) before its own rounding.  Hyper-parameters are float kernel arguments: every
formula is evaluated at their float32 values (``f32``); ``1 - beta`` and ``1 - rho`` are exact in
fp32 for beta, rho in [0.5, 1] (Sterbenz).

Slab sum.  S partials summed in ANY order: every partial goes through at most S - 1 additions,
    |got - ref| <= gamma(S - 1) A,   A = sum_s |x_s|.

Updates.  g' = g * grad_scale (1 rounding).  Every scalar s[i] is an input, evaluated as given (the
tests pass the float32 values the kernel reads); the counts still carry ONE rounding per scalar
factor, so a caller may pass the float64 scalar of ``step_scalars`` instead.  A state value is
bounded by ``gamma(c_state) M`` with M the magnitude sum of its formula, a weight by
``U |p_new| + gamma(c_p) D`` with D the magnitude of the update, in which every cancelling sum is
replaced by its magnitude sum (so an m that cancelled to nothing still carries the error of its
terms).  Counts, longest path (``x(c)``: x carries c roundings):

  m   = b1 m0 (1) + (1-b1) g' (1+1)                      add 1            c_m   = 3
  v   = b2 v0 (1) + ((1-b2) g' (2)) g' (2+1+1 = 4)       add 1            c_v   = 5   (acc of RMSprop,
                                                                                       Adadelta alike)
  den = sqrt(v) (ceil(5/2) + 1 = 4) + eps                add 1            c_den = 5
  Adam     D = s0 (1) * M_m (3), mul 1 (5) / den (5), div 1               c_p   = 11
  AMSGrad  vhat = max(vhat0, v): 1-Lipschitz                              c_vhat = 5, c_p = 11
  Adamax   u = max(b2 u0 (1), |g'| (1))                                   c_u   = 1
           D = s0 M_m (5) / (u + eps) (1 + 1), div 1                      c_p   = 8
  Adagrad  a = a0 + g' g' (1+1+1 = 3), add 1                              c_a   = 4
           D = s0 g' (1+1+1 = 3) / (sqrt(a) (2+1) + eps (1) = 4), div 1   c_p   = 8
  RMSprop  D = s0 g' (3) / den (5), div 1                                 c_p   = 9
  Adadelta upd = g' sqrt(d0 + eps) (1 + (1+1) + 1 = 4) / sqrt(a + eps) (ceil(6/2) + 1 = 4), div 1 = 9
           D = s0 upd (1 + 9 + 1)                                         c_p   = 11
           d = rho d0 (1) + ((1-rho) upd (10)) upd (10+9+1 = 20), add 1   c_d   = 21
  SGD      D = lr g' (1+1+1)                                              c_p   = 3
  momentum vel = mom v0 (1) - lr g' (3), sub 1                            c_vel = 4;  D = M_vel, c_p = 4
  Nesterov D = mom vel (4+1 = 5) - lr g' (3), sub 1                       c_p   = 6
  Nadam    gp = g' s2 (1+1+1 = 3);  mp = m s3 (3+1+1 = 5);  vp = v s4 (5+1+1 = 7)
           mbar = (1 - mc_t) (1 + q) gp (3), mul 1 (5 + q)  +  mc_t1 (1) mp (5), mul 1 (7), add 1 = 8 + q
                  with q = ceil(mc_t / (1 - mc_t)): a relative error U of mc_t is q U of 1 - mc_t
           D = s5 (1) mbar (8 + q), mul 1 / (sqrt(vp) (ceil(7/2) + 1 = 5) + eps (1) = 6), div 1
                                                                          c_p   = 17 + q

Step scalars: computed in double on the device and stored as float: ``|got - ref| <= 2 U |ref|``.

Packs: exact.  ``frag_index`` is the documented layout
``pack[((ks*NT + nt)*64 + lane)*8 + j] = B[k = 32 ks + 8 (lane >> 4) + j][n = 16 nt + (lane & 15)]``;
bf16 is round-to-nearest-even by integer arithmetic on the uint32 view; padding is zero.
"""
import math
from types import SimpleNamespace

import numpy as np

from . import clip_oracle as C
from . import optim_oracle as O

U = 2.0 ** -24
RED_CONVW, RED_BIAS, RED_FLATW = 0, 1, 2
PACK_CONV_FWD, PACK_CONV_DGRAD, PACK_DENSE_FWD, PACK_DENSE_BWD = 0, 1, 2, 3
KIND_ID = {"sgd": 0, "rmsprop": 1, "adadelta": 2, "adam": 3, "nadam": 4, "adagrad": 5, "adamax": 6, "amsgrad": 7}
N_SLOTS = {"sgd": 1, "rmsprop": 1, "adadelta": 2, "adam": 2, "nadam": 2, "adagrad": 1, "adamax": 2, "amsgrad": 3}
# the optimizer forms the tests run: (name, kind, momentum on, nesterov)
FORMS = [("sgd", "sgd", False, False), ("sgd_momentum", "sgd", True, False), ("sgd_nesterov", "sgd", True, True),
         ("rmsprop", "rmsprop", False, False), ("adadelta", "adadelta", False, False), ("adam", "adam", False, False),
         ("nadam", "nadam", False, False), ("adagrad", "adagrad", False, False), ("adamax", "adamax", False, False),
         ("amsgrad", "amsgrad", False, False)]


def gamma(c):
    return c * U / (1.0 - c * U)


def f32(x):
    """The float32 value of a float kernel argument, as a Python float."""
    return float(np.float32(x))


def f64(x):
    return np.asarray(x, dtype=np.float64)


# --------------------------------------------------------------------------- slab reduction
def red_desc(type, S, stride_s, ld=0, dst_off=0, numel=0, KH=1, KW=1, Cin=1, Cout=1, Cs=1, tpe=-1, slab_off=0):
    """One reduction descriptor (RedDesc of args.h; slab_off: where its slab starts in the case's
    slab tensor).  numel 0: the whole tensor of a RED_CONVW / RED_FLATW (KH*KW*Cin*Cout)."""
    if not numel:
        numel = KH * KW * Cin * Cout
    return SimpleNamespace(type=type, S=S, stride_s=stride_s, ld=ld, dst_off=dst_off, numel=numel, KH=KH, KW=KW,
                           Cin=Cin, Cout=Cout, Cs=Cs, tpe=tpe, slab_off=slab_off)


def red_src(d):
    """Slab offset (within one split) of every Keras-order element of descriptor d."""
    if d.type == RED_CONVW:      # keras (tap, ci, co) -> slab[(tap*Cs + ci)*ld + co]
        tap, ci, co = np.meshgrid(np.arange(d.KH * d.KW), np.arange(d.Cin), np.arange(d.Cout), indexing="ij")
        src = (tap * d.Cs + ci) * d.ld + co
    elif d.type == RED_FLATW:    # keras (k, n) -> slab[((k // Cin)*Cs + k % Cin)*ld + n]
        k, n = np.meshgrid(np.arange(d.KH * d.KW * d.Cin), np.arange(d.Cout), indexing="ij")
        src = ((k // d.Cin) * d.Cs + k % d.Cin) * d.ld + n
    else:                        # RED_BIAS: plain
        src = np.arange(d.numel)
    src = src.reshape(-1).astype(np.int64)
    assert src.size == d.numel, (src.size, d.numel)
    return src


def slab_gather(slab, d):
    """[S, numel]: the partials of every element, in the slab's own dtype."""
    idx = d.slab_off + red_src(d)
    return np.stack([np.asarray(slab)[idx + s * d.stride_s] for s in range(d.S)])


def slab_sum(slab, d):
    """(float64 sum over the S slabs, A = sum |x_s|) per Keras-order element."""
    x = slab_gather(slab, d).astype(np.float64)
    return x.sum(0), np.abs(x).sum(0)


def slab_sum_exact(slab, d):
    """int64 sum of integer-valued slabs."""
    x = slab_gather(slab, d)
    xi = x.astype(np.int64)
    assert np.array_equal(xi.astype(x.dtype), x), "slab values are not integers"
    return xi.sum(0)


def slab_bound(S, A):
    return gamma(S - 1) * f64(A) if S > 1 else np.zeros_like(f64(A))


def slab_read_mask(numel, descs):
    """True at every position of the slab tensor that some descriptor's map reads."""
    m = np.zeros(numel, dtype=bool)
    for d in descs:
        idx = d.slab_off + red_src(d)
        for s in range(d.S):
            m[idx + s * d.stride_s] = True
    return m


# --------------------------------------------------------------------------- updates
def hyper(beta1=0.9, beta2=0.999, eps=1e-7, rho=0.95, momentum=0.0, nesterov=False, grad_scale=1.0):
    """Hyper-parameters at their float32 kernel-argument values."""
    return SimpleNamespace(beta1=f32(beta1), beta2=f32(beta2), eps=f32(eps), rho=f32(rho), momentum=f32(momentum),
                           nesterov=bool(nesterov), grad_scale=f32(grad_scale))


def rmsprop(p, g, a, lr, rho=0.9, eps=O.EPS):
    """Keras RMSprop: a = rho a + (1 - rho) g^2;  p = p - lr g / (sqrt(a) + eps)."""
    p, g, a = O._f64(p, g, a)
    a = rho * a + (1.0 - rho) * g * g
    return p - lr * g / (np.sqrt(a) + eps), a


def nadam_from_scalars(p, g, m, v, s, beta_1, beta_2, eps):
    """Keras Nadam with the step's scalars given: s = [mc_t, mc_t1, 1 / (1 - m_sched_new),
    1 / (1 - m_sched_next), 1 / (1 - beta_2^t), lr]."""
    p, g, m, v = O._f64(p, g, m, v)
    gp = g * s[2]
    m = beta_1 * m + (1.0 - beta_1) * g
    v = beta_2 * v + (1.0 - beta_2) * g * g
    mbar = (1.0 - s[0]) * gp + s[1] * (m * s[3])
    return p - s[5] * mbar / (np.sqrt(v * s[4]) + eps), m, v


def update(kind, p, g, slots, hp, s):
    """One update of ``kind`` from (p, g, slots) with hyper-parameters ``hp`` (hyper()) and the
    step's scalars s[0..5].  Returns a namespace: p, slots (new values), D (the update's magnitude),
    M (the magnitude sum of each new slot), c_p, c_s (the rounding counts of the module docstring)."""
    p, g = f64(p), f64(g)
    slots = [f64(x) for x in slots]
    s = [float(x) for x in s]
    gs = g * hp.grad_scale                                     # grad_scale first, as the kernel
    ag = np.abs(gs)
    b1, b2, eps, rho = hp.beta1, hp.beta2, hp.eps, hp.rho
    inf = float("inf")    # t = inf: the imported functions' own bias correction is the identity
    if kind == "sgd":
        lr = s[0]
        if hp.momentum:
            pn, new = C.sgd(p, gs, slots[0], lr, hp.momentum, hp.nesterov)
            Mv = np.abs(hp.momentum * slots[0]) + lr * ag
            if hp.nesterov:
                D, c_p = hp.momentum * Mv + lr * ag, 6
            else:
                D, c_p = Mv, 4
            M, c_s = [Mv], [4]
        else:
            pn, new = C.sgd(p, gs, None, lr)
            D, c_p, M, c_s = lr * ag, 3, [], []
    elif kind == "rmsprop":
        pn, a = rmsprop(p, gs, slots[0], s[0], rho, eps)
        new, M, c_s = [a], [np.abs(rho * slots[0]) + (1.0 - rho) * gs * gs], [5]
        D, c_p = s[0] * ag / (np.sqrt(a) + eps), 9
    elif kind == "adagrad":
        pn, a = O.adagrad(p, gs, slots[0], s[0], eps)
        new, M, c_s = [a], [np.abs(slots[0]) + gs * gs], [4]
        D, c_p = s[0] * ag / (np.sqrt(a) + eps), 8
    elif kind == "adadelta":
        pn, a, d = C.adadelta(p, gs, slots[0], slots[1], s[0], rho, eps)
        upd = gs * np.sqrt(slots[1] + eps) / np.sqrt(a + eps)
        new = [a, d]
        M = [np.abs(rho * slots[0]) + (1.0 - rho) * gs * gs, np.abs(rho * slots[1]) + (1.0 - rho) * upd * upd]
        c_s = [5, 21]
        D, c_p = s[0] * np.abs(upd), 11
    elif kind in ("adam", "amsgrad", "adamax", "nadam"):
        Mm = np.abs(b1 * slots[0]) + (1.0 - b1) * ag
        Mv = np.abs(b2 * slots[1]) + (1.0 - b2) * gs * gs
        if kind == "adam":
            pn, m, v = O.adam(p, gs, slots[0], slots[1], inf, s[0], b1, b2, eps)
            new, M, c_s = [m, v], [Mm, Mv], [3, 5]
            D, c_p = s[0] * Mm / (np.sqrt(v) + eps), 11
        elif kind == "amsgrad":
            pn, m, v, vh = O.amsgrad(p, gs, slots[0], slots[1], slots[2], inf, s[0], b1, b2, eps)
            new, M, c_s = [m, v, vh], [Mm, Mv, np.maximum(np.abs(slots[2]), Mv)], [3, 5, 5]
            D, c_p = s[0] * Mm / (np.sqrt(vh) + eps), 11
        elif kind == "adamax":
            pn, m, u = O.adamax(p, gs, slots[0], slots[1], inf, s[0], b1, b2, eps)
            new, M, c_s = [m, u], [Mm, np.abs(u)], [3, 1]
            D, c_p = s[0] * Mm / (u + eps), 8
        else:
            pn, m, v = nadam_from_scalars(p, gs, slots[0], slots[1], s, b1, b2, eps)
            new, M, c_s = [m, v], [Mm, Mv], [3, 5]
            q = int(math.ceil(s[0] / (1.0 - s[0])))
            Mbar = np.abs((1.0 - s[0]) * s[2]) * ag + np.abs(s[1] * s[3]) * Mm
            D, c_p = s[5] * Mbar / (np.sqrt(v * s[4]) + eps), 17 + q
    else:
        raise ValueError(kind)
    return SimpleNamespace(p=pn, slots=list(new), D=f64(D), M=[f64(x) for x in M], c_p=c_p, c_s=list(c_s))


def update_bounds(r):
    """(bound of p, [bound of each slot]) of an ``update`` result."""
    return U * np.abs(r.p) + gamma(r.c_p) * r.D, [gamma(c) * m for c, m in zip(r.c_s, r.M)]


def _ratio(got, ref, bound):
    """Worst |got - ref| / bound over the elements (0 where the error is 0, inf for a NaN)."""
    err = np.abs(f64(got) - ref)
    out = np.zeros(err.shape)
    nz = ~(err == 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        out[nz] = np.where(np.isfinite(err[nz]), err[nz] / np.broadcast_to(bound, err.shape)[nz], np.inf)
    return float(out.max()) if out.size else 0.0


def keras_step_ratio(opt, t, prev_p, g, prev_slots, new_p, new_slots, m_schedule=1.0, grad_scale=1.0):
    """One whole-model step t of optimizer object ``opt`` held to the per-element bounds: the
    device's own master and slots BEFORE the step, the gradient it used, and what it left.  The
    scalars are ``step_scalars`` in float64 (the counts carry their float rounding).  Returns
    (worst error / bound over master and slots, m_schedule after the step)."""
    kind = opt.kind
    _, s, ms = step_scalars(kind, t, float(opt.lr), getattr(opt, "initial_decay", 0.0), getattr(opt, "beta_1", 0.9),
                            getattr(opt, "beta_2", 0.999), getattr(opt, "schedule_decay", 0.004), m_schedule)
    hp = hyper(getattr(opt, "beta_1", 0.9), getattr(opt, "beta_2", 0.999), getattr(opt, "epsilon", 1e-7),
               getattr(opt, "rho", 0.95), getattr(opt, "momentum", 0.0), getattr(opt, "nesterov", False), grad_scale)
    r = update(kind, prev_p, g, list(prev_slots), hp, [0.0 if x is None else x for x in s])
    bp, bs = update_bounds(r)
    w = [_ratio(new_p, r.p, bp)] + [_ratio(a, b, c) for a, b, c in zip(new_slots, r.slots, bs)]
    return max(w), ms


# --------------------------------------------------------------------------- step scalars
def nadam_mc(t, beta1, schedule_decay):
    return beta1 * (1.0 - 0.5 * 0.96 ** (t * schedule_decay))


def nadam_m_schedule(t, beta1, schedule_decay):
    """Keras' running product m_schedule after step t (1 before the first step)."""
    b1, sd = f32(beta1), f32(schedule_decay)
    ms = 1.0
    for i in range(1, t + 1):
        ms *= nadam_mc(float(i), b1, sd)
    return ms


def step_scalars(kind, t, lr, decay=0.0, beta1=0.9, beta2=0.999, schedule_decay=0.004, m_schedule=1.0):
    """(lr_eff, s[0..5], m_schedule after the step) of 1-based step t in float64; entries of s the
    kind does not define are None.  lr: the float base rate; m_schedule: the product before the step."""
    lr, decay, b1, b2, sd = f32(lr), f32(decay), f32(beta1), f32(beta2), f32(schedule_decay)
    t = float(t)
    lr_eff = lr / (1.0 + decay * (t - 1.0))                      # Keras `decay`
    s = [None] * 6
    if kind in ("adam", "amsgrad"):
        s[0] = lr_eff * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
    elif kind == "adamax":
        s[0] = lr_eff / (1.0 - b1 ** t)
    elif kind == "nadam":
        mc_t, mc_t1 = nadam_mc(t, b1, sd), nadam_mc(t + 1.0, b1, sd)
        m_schedule = m_schedule * mc_t
        s = [mc_t, mc_t1, 1.0 / (1.0 - m_schedule), 1.0 / (1.0 - m_schedule * mc_t1), 1.0 / (1.0 - b2 ** t), lr_eff]
    else:
        s[0] = lr_eff
    return lr_eff, s, m_schedule


def scalar_bound(ref):
    return 2.0 * U * abs(ref)


# --------------------------------------------------------------------------- packs
def frag_index(k, n, NT):
    """Element index of B[k][n] in a fragment-major pack with NT n-tiles."""
    k, n = np.asarray(k, dtype=np.int64), np.asarray(n, dtype=np.int64)
    ks, nt = k // 32, n // 16
    lane = 16 * ((k % 32) // 8) + n % 16
    j = k % 8
    return ((ks * NT + nt) * 64 + lane) * 8 + j


def bf16_rne(x):
    """float32 -> bf16 bits (uint16), round to nearest even, by integer arithmetic (finite x)."""
    b = np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def cdiv(a, b):
    return -(-a // b)


def _scatter(kk, nn, w, krows, NT):
    """(pack uint16 [KS*NT*512] with zero padding, the indices written)."""
    KS = cdiv(krows, 32)
    out = np.zeros(KS * NT * 512, dtype=np.uint16)
    idx = frag_index(kk.reshape(-1), nn.reshape(-1), NT)
    assert idx.size == np.unique(idx).size and idx.max() < out.size
    out[idx] = bf16_rne(np.asarray(w, dtype=np.float32).reshape(-1))
    return out, idx


def conv_fwd_pack(w, Cs, NT):
    """w [KHW, Cin, Cout] (Keras order): k = tap*Cs + ci, n = co."""
    KHW, Cin, Cout = w.shape
    tap, ci, co = np.meshgrid(np.arange(KHW), np.arange(Cin), np.arange(Cout), indexing="ij")
    return _scatter(tap * Cs + ci, co, w, KHW * Cs, NT)


def conv_dgrad_pack(w, Cs_out, NT):
    """k = (KHW-1-tap)*Cs_out + co, n = ci."""
    KHW, Cin, Cout = w.shape
    tap, ci, co = np.meshgrid(np.arange(KHW), np.arange(Cin), np.arange(Cout), indexing="ij")
    return _scatter((KHW - 1 - tap) * Cs_out + co, ci, w, KHW * Cs_out, NT)


def _padded(k, Cin, Cs):
    return (k // Cin) * Cs + k % Cin


def dense_fwd_pack(w, Cin, Cs, NT):
    """w [K = pixels*Cin, N] (Keras order): k = padded flat k, n = n."""
    K, N = w.shape
    k, n = np.meshgrid(np.arange(K), np.arange(N), indexing="ij")
    return _scatter(_padded(k, Cin, Cs), n, w, (K // Cin) * Cs, NT)


def dense_bwd_pack(w, Cin, Cs, NTb):
    """k = n_dense, n = padded flat k."""
    K, N = w.shape
    k, n = np.meshgrid(np.arange(K), np.arange(N), indexing="ij")
    return _scatter(n, _padded(k, Cin, Cs), w, N, NTb)


# routes (PackRoute, args.h), as the tuple the executor builds:
# (lo, hi, kind, KHW, Cin, Cout, Cs, Csb, NT, NTb, fwd, bwd)
def route_array(routes, words):
    """The device array of routes: 10 int32 + 2 int64 each (``words`` int32 words per route)."""
    arr = np.zeros(len(routes) * words, dtype=np.int32)
    a64 = arr.view(np.int64)
    for r, rt in enumerate(routes):
        arr[r * words:r * words + 10] = rt[:10]
        a64[r * words // 2 + 5] = rt[10]
        a64[r * words // 2 + 6] = rt[11]
    return arr


def route_packs(rt, w_flat):
    """{arena offset: (pack, indices written)} of route rt from the flat master w_flat."""
    lo, hi, kind, KHW, Cin, Cout, Cs, Csb, NT, NTb, fwd, bwd = rt
    w = np.asarray(w_flat, dtype=np.float32)[lo:hi]
    out = {}
    if kind == 1:
        w = w.reshape(KHW, Cin, Cout)
        if fwd >= 0:
            out[fwd] = conv_fwd_pack(w, Cs, NT)
        if bwd >= 0:
            out[bwd] = conv_dgrad_pack(w, Csb, NTb)
    else:
        w = w.reshape(KHW * Cin, Cout)
        if fwd >= 0:
            out[fwd] = dense_fwd_pack(w, Cin, Cs, NT)
        if bwd >= 0:
            out[bwd] = dense_bwd_pack(w, Cin, Cs, NTb)
    return out


def route_expect(routes, w_flat, arena0, lo=None, hi=None):
    """The arena (uint16) after an update of master elements [lo, hi) wrote its routes: arena0 with
    the pack element of every updated route element replaced by the bf16 of w_flat."""
    exp = np.array(arena0, dtype=np.uint16)
    for rt in routes:
        for off, (pack, idx) in route_packs(rt, w_flat).items():
            e = rt[0] + np.arange(rt[1] - rt[0])     # _scatter keeps Keras order: idx[i] <-> element rt.lo + i
            keep = np.ones(e.size, dtype=bool)
            if lo is not None:
                keep = (e >= lo) & (e < hi)
            exp[off + idx[keep]] = pack[idx[keep]]
    return exp


# --------------------------------------------------------------------------- host-side fit check
def _pow2(x):
    return x > 0 and (x & (x - 1)) == 0


def check_case_fits(case):
    """Assert on the host that a synthetic case stays inside its tensors and inside the kernels'
    stated contracts.  ``case``: a dict with any of
      red:    {"descs": [...], "slab_numel", "grad_numel", "state_numel" (0: no update)}
      optim:  {"lo", "n", "numel" (of master / gradient / state buffers)}
      routes: {"routes": [...], "arena_numel", "max_routes", "tiled": [route indices]}
      packs:  {"conv": [(src_off, type, KHW, Cin, Cout, Cs, NT, dst)], "dense": [(src_off, pixels, Cin, Cs, N, NT,
               dst_fwd, NTb, dst_bwd)], "master_numel", "arena_numel"}"""
    red = case.get("red")
    if red:
        for d in red["descs"]:
            assert d.S >= 1 and d.numel >= 1 and d.dst_off >= 0
            assert d.tpe <= 0 or (_pow2(d.tpe) and d.tpe <= 256), "tpe: a power of two <= 256"
            if d.type != RED_BIAS:
                assert d.Cs == 4 or d.Cs % 8 == 0, "Cs in {4} + 8N"
                assert d.Cin <= d.Cs and d.Cout <= d.ld
            src = red_src(d)
            ident = d.type == RED_BIAS or (d.Cin == d.Cs and d.ld == d.Cout)
            vec4 = ident and d.numel % 4 == 0 and d.dst_off % 4 == 0 and d.stride_s % 4 == 0 and d.tpe <= 0
            last = d.slab_off + (d.S - 1) * d.stride_s + int(src.max()) + (3 if vec4 else 0)
            assert last < red["slab_numel"], ("slab read past the end", last, red["slab_numel"])
            assert int(src.max()) < d.stride_s or d.S == 1, "splits overlap"
            if vec4:
                assert d.slab_off % 4 == 0, "float4 loads need a 16-byte aligned slab"
            assert d.dst_off + d.numel <= red["grad_numel"]
            if red.get("state_numel"):
                assert d.dst_off + d.numel <= red["state_numel"]
    opt = case.get("optim")
    if opt:
        lo, n, numel = opt["lo"], opt["n"], opt["numel"]
        assert numel % 64 == 0, "state buffers are padded to a multiple of 64 floats"
        assert lo >= 0 and n >= 1
        base, end = lo & ~3, lo + n
        groups = cdiv(end - base, 4)
        assert base + 4 * groups <= numel, "the last aligned float4 group lies past the buffers"
    ro = case.get("routes")
    if ro:
        assert len(ro["routes"]) <= ro["max_routes"]
        for i, rt in enumerate(ro["routes"]):
            lo, hi, kind, KHW, Cin, Cout, Cs, Csb, NT, NTb, fwd, bwd = rt
            assert kind in (1, 2) and hi - lo == KHW * Cin * Cout
            assert Cs == 4 or Cs % 8 == 0
            assert Cin <= Cs and Cout <= NT * 16
            if kind == 1 and bwd >= 0:
                assert Csb % 4 == 0 and Cout <= Csb and Cin <= NTb * 16, "a conv route has bwd only when Cs_out % 4 == 0"
            if kind == 2 and bwd >= 0:
                assert KHW * Cs <= NTb * 16
            if i in ro.get("tiled", ()):
                K = (hi - lo) // Cout
                assert kind == 2 and Cin == Cs and Cout % 32 == 0 and K % 8 == 0 and lo % 4 == 0 and fwd >= 0
            w = np.zeros(ro.get("master_numel", hi), dtype=np.float32)
            for off, (pack, _idx) in route_packs(rt, w).items():
                assert off % 8 == 0 and off + pack.size <= ro["arena_numel"], "pack past the arena"
            if opt:
                assert hi <= opt["numel"]
    pk = case.get("packs")
    if pk:
        for src_off, type, KHW, Cin, Cout, Cs, NT, dst in pk.get("conv", ()):
            assert Cs == 4 or Cs % 8 == 0
            assert src_off + KHW * Cin * Cout <= pk["master_numel"]
            assert (Cout if type == PACK_CONV_FWD else Cin) <= NT * 16
            assert (Cin if type == PACK_CONV_FWD else Cout) <= Cs
            assert dst % 8 == 0 and dst + cdiv(KHW * Cs, 32) * NT * 512 <= pk["arena_numel"]
        for src_off, pixels, Cin, Cs, N, NT, dst_fwd, NTb, dst_bwd in pk.get("dense", ()):
            assert Cs % 8 == 0 and Cin <= Cs and N <= NT * 16
            assert src_off + pixels * Cin * N <= pk["master_numel"]
            assert dst_fwd % 8 == 0 and dst_fwd + cdiv(pixels * Cs, 32) * NT * 512 <= pk["arena_numel"]
            if dst_bwd >= 0:
                assert pixels * Cs <= NTb * 16
                assert dst_bwd % 8 == 0 and dst_bwd + cdiv(N, 32) * NTb * 512 <= pk["arena_numel"]

"""The synthetic inputs of tests/test_param_path_gpu.py, shared with tests/test_param_oracle.py, which
proves on the CPU that these inputs discriminate (every listed mutation is flagged at them) and that
an fp32 evaluation of the formulas stays inside the oracle's bounds at them.  NumPy only."""
import numpy as np

from . import param_oracle as P

# ------------------------------------------------------------------------------- optimizer
NUMEL = 2176                       # 34 * 64 floats
RANGES = [(0, 64), (1, 1), (3, 1), (2, 3), (5, 4), (1, 62), (4, 7), (1022, 1030)]
SETTINGS = dict(beta1=0.8, beta2=0.95, eps=1e-3, rho=0.9, grad_scale=1.0 / 3.0)
MOMENTUM = 0.7
# hand-written step scalars (float32 values): one rate for most kinds, Nadam's six
SCALARS = {"nadam": [0.41, 0.43, 1.7, 1.3, 20.5, 2e-3]}
RATE = 1.25e-3


def forms():
    return [f[0] for f in P.FORMS]


def form_kind(form):
    return {f[0]: f[1] for f in P.FORMS}[form]


def hyper_of(form):
    _, _, mom, nest = {f[0]: f for f in P.FORMS}[form]
    return P.hyper(momentum=MOMENTUM if mom else 0.0, nesterov=nest, **SETTINGS)


def slots_of(form):
    """State buffers the launch of this form gets (plain SGD: none)."""
    return 0 if form == "sgd" else P.N_SLOTS[form_kind(form)]


def scalars_of(form):
    s = SCALARS.get(form_kind(form), [RATE, 0.0, 0.0, 0.0, 0.0, 0.0])
    return [P.f32(x) for x in s]


def optim_inputs(form, numel=NUMEL, seed=0):
    """(p, g, [slots]) float32.  |g| from 1e-8 to 1e2, both signs; element i % 16 == 3: g = 0 over
    zero state, i % 16 == 7: g = 0 over non-zero state, i % 16 == 11: zero state under a non-zero g.
    Second moments are g^2 times 1e-2 .. 1e2; AMSGrad's vhat is half or four times v (below / above
    the new v); Adamax' u is 0.1 or 3 times |g| (beta_2 u below / above |g| / 3)."""
    kind = form_kind(form)
    rs = np.random.RandomState(1000 + seed)
    i = np.arange(numel)
    p = (0.5 * rs.randn(numel)).astype(np.float32)
    mag = 10.0 ** rs.uniform(-8, 2, numel)
    g = (mag * np.where(rs.rand(numel) < 0.5, -1.0, 1.0)).astype(np.float32)
    first = (2.0 * rs.uniform(-1, 1, numel) * g).astype(np.float32)                  # m / velocity
    second = (g.astype(np.float64) ** 2 * 10.0 ** rs.uniform(-2, 2, numel)).astype(np.float32)
    coin = rs.rand(numel) < 0.5
    delta = (10.0 ** rs.uniform(-6, -2, numel)).astype(np.float32)
    g[(i % 16 == 3) | (i % 16 == 7)] = 0.0
    if kind == "sgd":
        slots = [first]
    elif kind in ("rmsprop", "adagrad"):
        slots = [second]
    elif kind == "adadelta":
        slots = [second, delta]
    elif kind in ("adam", "nadam"):
        slots = [first, second]
    elif kind == "adamax":
        slots = [first, (np.abs(mag) * np.where(coin, 0.1, 3.0)).astype(np.float32)]
    else:
        slots = [first, second, (second * np.where(coin, 0.5, 4.0).astype(np.float32)).astype(np.float32)]
    zero = (i % 16 == 3) | (i % 16 == 11)
    for s in slots:
        s[zero] = 0.0
    return p, g, slots[:slots_of(form)]


# ------------------------------------------------------------------------------- slab reduction
TPES = [1, 2, 4, 8, 64, 256]
S_CAP = 1100


def s_list(tpe):
    out = []
    for s in (1, tpe, tpe + 1, 7 * tpe, 8 * tpe - 1, 8 * tpe, 8 * tpe + 1, 16 * tpe + 3):
        s = min(s, S_CAP)
        if s not in out:
            out.append(s)
    return out


def auto_tpe(S, lanes):
    """RedTable.add's split-lane choice for a descriptor without an explicit tpe."""
    t = 1
    while t < 64 and t * lanes < S:
        t *= 2
    return t


def lanes_for(S, tpe):
    """A red_lanes value that makes auto_tpe(S, .) the wanted tpe (None: not reachable)."""
    n = max(1, P.cdiv(S, tpe))
    return n if auto_tpe(S, n) == tpe else None


# (name, type, dst_off when run alone, dst_off in the table, desc fields, gap to stride_s)
_DESCS = [
    ("bias37", P.RED_BIAS, 3, 3, dict(numel=37), 3),
    ("bias2052", P.RED_BIAS, 8, 64 + 8, dict(numel=2052), 4),
    ("conv_padded", P.RED_CONVW, 5, 2181, dict(KH=3, KW=3, Cin=3, Cs=4, Cout=5, ld=16), 16),
    ("conv_ident", P.RED_CONVW, 4, 2368, dict(KH=3, KW=3, Cin=8, Cs=8, Cout=16, ld=16), 8),
    ("flat_padded", P.RED_FLATW, 2, 3522, dict(KH=6, KW=1, Cin=5, Cs=8, Cout=12, ld=16), 4),
    ("flat_ident", P.RED_FLATW, 0, 3904, dict(KH=8, KW=1, Cin=8, Cs=8, Cout=16, ld=16), 8),
]
DESC_NAMES = [d[0] for d in _DESCS]
VEC4_NAMES = ["bias2052", "conv_ident", "flat_ident"]       # identity layouts: float4 without a tpe
GRAD_NUMEL = 4992                                            # 78 * 64: the table's flat range


def _rows(kw):
    return kw["KH"] * kw["KW"] * kw["Cs"] * kw["ld"] if "ld" in kw else kw["numel"]


def red_descs(S, tpe=-1, names=None, alone=False):
    """(descriptors, slab_numel): every descriptor's slab in one tensor, each with a gap up to its
    stride_s and 8 spare floats behind its last split."""
    descs, off = [], 0
    for name, type, dst_alone, dst_tab, kw, gap in _DESCS:
        if names is not None and name not in names:
            continue
        stride = _rows(kw) + gap
        d = P.red_desc(type, S, stride, dst_off=dst_alone if alone else dst_tab, tpe=tpe, slab_off=off, **kw)
        d.name = name
        descs.append(d)
        off += S * stride + 8
    return descs, off


def red_slab(descs, slab_numel, mode, seed=0):
    """float32 slab tensor: NaN wherever no descriptor's map reads; ``mode`` "int": integers in
    [-64, 64], "normal": normal values spread over six decades."""
    rs = np.random.RandomState(2000 + seed)
    mask = P.slab_read_mask(slab_numel, descs)
    slab = np.full(slab_numel, np.nan, dtype=np.float32)
    n = int(mask.sum())
    if mode == "int":
        slab[mask] = rs.randint(-64, 65, n).astype(np.float32)
    else:
        slab[mask] = (rs.randn(n) * 10.0 ** rs.uniform(-3, 3, n)).astype(np.float32)
    return slab


# ------------------------------------------------------------------------------- packs
# (KH, KW, Cin, Cs, Cout, Cs_out)
PACK_CONVS = [(3, 3, 1, 4, 5, 8), (3, 3, 3, 4, 16, 16), (1, 1, 5, 8, 20, 24), (5, 5, 8, 8, 8, 8)]
# (pixels, Cin, Cs, N)
PACK_DENSES = [(6, 5, 8, 10), (4, 8, 8, 130), (1, 40, 40, 32)]


def _bits(*words):
    return np.array(words, dtype=np.uint32).view(np.float32)


def special_values():
    """bf16 ties both ways, their negatives, values near the largest finite bf16, fp32 subnormals."""
    one = np.float32(1.0)
    ties = np.array([one + np.float32(2.0 ** -8), one + np.float32(3 * 2.0 ** -8)], dtype=np.float32)
    big = np.concatenate([np.array([3.0e38, -3.38e38], dtype=np.float32), _bits(0x7F7F7FFF, 0xFF7F7FFF, 0x7F7F0001)])
    sub = np.concatenate([np.array([1e-40, -1e-40], dtype=np.float32), _bits(0x00000001, 0x00008000, 0x00018000,
                                                                              0x00018001, 0x807FFFFF)])
    return np.concatenate([ties, -ties, big, sub])


def pack_master(numel, seed=0):
    """float32 master: normal values with the special values scattered at every 7th element."""
    rs = np.random.RandomState(3000 + seed)
    w = rs.randn(numel).astype(np.float32)
    sp = special_values()
    pos = np.arange(0, numel, 7)
    w[pos] = sp[np.arange(pos.size) % sp.size]
    return w

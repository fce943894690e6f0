"""Float64 NumPy oracle of the loss table (README, "Losses") behind a linear, sigmoid or softmax
output, the multi-label sigmoid binary_crossentropy included, and DERIVED bounds for a float32
evaluation of it.  Clip bounds are the FLOAT32 values TF computes with (``head_oracle.LO`` /
``HI``), as in ``head_oracle.py``.

``evaluate(act, loss, z, y)`` returns an ``Eval`` with, per row, ``loss [M]``, ``dz [M, N]``
(dl/dlogits, not / M), ``correct [M]`` (Keras' compile rule: the row's COUNT of correct elements
under binary_accuracy -- N == 1 or binary_crossentropy --, 0 / 1 under categorical_accuracy) and
``probs [M, N]``, plus what the bounds need (below).

Subgradient conventions: a maximum's tie gives the first argument the gradient (hinge margin
exactly 0 -> -y / N; msle p == eps -> passes), clips pass it on the closed interval, sign(0) = 0,
the FIRST row maximum takes categorical_hinge's whole gradient.

Bounds (``bounds(ev, dzl)``), first-order error propagation of the formulas, nothing measured:

* ``dzl [M, N]`` is the caller's bound on the logit error (``logit_error_bound``: the standard
  (K + 2) u sum |a| |w| of a length-K float32 dot product, u = 2**-24).
* The output p = A(z) then errs by ``dp``: linear dzl; sigmoid p (1 - p) dzl + 8 u p; softmax
  p_n (dzl_n + sum_m p_m dzl_m) + 16 u p_n (|dp/dz| times the logit error, plus the roundings
  of exp / sum / divide at p's magnitude).
* Every loss lists the magnitudes ``Lmag`` / ``Gmag`` at which its element loss l_n and its
  g_n = dl/dp_n round (for example msle: the two logarithms each err by u (1 + 2 |log|), so their
  difference D errs at magnitude Dmag = 1 + |a| + |b|; l = D^2 / N at 2 |D| Dmag + D^2, g at
  2 Dmag / (p + 1)).  At most 8 operations of at most 2 ulp each: 16 u per magnitude.
* loss: sum_n |g_n| dp_n + 16 u Lmag_n   (binary_crossentropy: |dz_n| dzl_n + head_oracle's
  derived sigmoid bound / N).
* dz: |d dz / d p| dp + 16 u (the chain's own magnitudes), with the analytic g' = dg/dp of every
  loss: linear |g'| dp; sigmoid |g' p (1 - p) + g (1 - 2 p)| dp; softmax, with S = sum p g,
  |g_n - S + p_n g'_n| dp_n + p_n sum_m |g_m + p_m g'_m| dp_m.
* Both are doubled for the second-order terms first-order propagation drops.

Kinks.  ``near_kink [M, N]`` marks the elements whose float64 margin to a kink of the gradient
(mae p = y, hinge margin 0, a clip edge, categorical_hinge's v = 0 or tied maxima) is within
``dp`` (scaled into the margin's units): float32 may take the other branch there.  ``jump`` is
the size of g's discontinuity at that kink, pushed through the chain into ``dz_jump``; a
comparison adds it to the tolerance of exactly those elements (for a softmax output the row's
other elements feel it through S, which the chain formula carries).  ``acc_ambiguous [M]``
counts the elements (rows) whose accuracy decision float32 may take the other way.
"""
from types import SimpleNamespace

import numpy as np

from . import head_oracle as H

U = 2.0 ** -24
EPS = H.LO                         # float32(1e-7)
LOSSES = ("mse", "mae", "msle", "logcosh", "hinge", "squared_hinge", "categorical_hinge", "kld", "poisson")
ACTS = (None, "sigmoid", "softmax")
NATURAL = {"mse": "sigmoid", "mae": None, "msle": None, "logcosh": None, "hinge": None, "squared_hinge": None,
           "categorical_hinge": None, "kld": "softmax", "poisson": "sigmoid", "binary_crossentropy": "sigmoid"}
PAIRS = [(a, l) for l in LOSSES for a in ACTS] + [("sigmoid", "binary_crossentropy")]
# the pairs of the second head kernel (linear + mse is the first kernel's; mse's "natural" output here is sigmoid)
KERNEL_PAIRS = [p for p in PAIRS if p != (None, "mse")]


def probs(act, z):
    z = np.asarray(z, np.float64)
    if act == "sigmoid":
        with np.errstate(over="ignore"):
            return 1.0 / (1.0 + np.exp(-z))
    if act == "softmax":
        e = np.exp(z - z.max(axis=1, keepdims=True))
        return e / e.sum(axis=1, keepdims=True)
    return z.copy()


def first_argmax(v):
    return np.argmax(v, axis=1)            # numpy: the first maximum


def _elementwise(loss, p, y, N):
    """(l_n, g, g', Lmag, Gmag, margin-to-kink in units of p, jump of g at that kink)."""
    inf = np.full_like(p, np.inf)
    zero = np.zeros_like(p)
    d = p - y
    if loss == "mse":
        return d * d / N, 2 * d / N, 2 / N + zero, d * d / N, 2 * np.abs(d) / N, inf, zero
    if loss == "mae":
        return np.abs(d) / N, np.sign(d) / N, zero, np.abs(d) / N, 1 / N + zero, np.abs(d), 2 / N + zero
    if loss == "msle":
        pm, ym = np.maximum(p, EPS), np.maximum(y, EPS)
        a, b = np.log(pm + 1), np.log(ym + 1)
        D, Dmag = a - b, 1 + np.abs(a) + np.abs(b)
        on = p >= EPS
        g = np.where(on, 2 * D / (pm + 1) / N, 0.0)
        gp = np.where(on, 2 * (1 - D) / (pm + 1) ** 2 / N, 0.0)
        return (D * D / N, g, gp, (2 * np.abs(D) * Dmag + D * D) / N, on * 2 * Dmag / (pm + 1) / N,
                np.abs(p - EPS), np.abs(2 * D / (pm + 1) / N))
    if loss == "logcosh":
        ad = np.abs(d)
        l = (ad + np.log1p(np.exp(-2 * ad)) - np.log(2.0)) / N
        return l, np.tanh(d) / N, (1 - np.tanh(d) ** 2) / N, (ad + 2 * np.log(2.0)) / N, np.minimum(1, ad) / N, inf, zero
    if loss == "hinge":
        m = 1 - y * p
        on = m >= 0
        ay = np.maximum(np.abs(y), 1e-300)
        return (np.maximum(m, 0) / N, np.where(on, -y / N, 0.0), zero, (1 + np.abs(y * p)) / N, on * np.abs(y) / N,
                np.abs(m) / ay, np.abs(y) / N)
    if loss == "squared_hinge":
        m = 1 - y * p
        h = np.maximum(m, 0)
        mag = 1 + np.abs(y * p)
        # (g is continuous at the kink: no jump; g' = 2 y^2 / N on the active side bounds both)
        return h * h / N, -2 * y * h / N, 2 * y * y / N, (2 * h * mag + h * h) / N, 2 * np.abs(y) * mag / N * (m > -1e-3), inf, zero
    if loss == "kld":
        yc, pc = np.clip(y, EPS, 1.0), np.clip(p, EPS, 1.0)
        on = (p >= EPS) & (p <= 1.0)
        lg = np.log(yc / pc)
        return (yc * lg, np.where(on, -yc / pc, 0.0), np.where(on, yc / pc ** 2, 0.0), yc * (1 + np.abs(lg)),
                on * yc / pc, np.minimum(np.abs(p - EPS), np.abs(p - 1.0)), yc / pc)
    if loss == "poisson":
        q = p + EPS
        with np.errstate(invalid="ignore", divide="ignore"):
            lq = np.log(q)
            return ((p - y * lq) / N, (1 - y / q) / N, y / q ** 2 / N, (np.abs(p) + np.abs(y) * (1 + np.abs(lq))) / N,
                    (1 + 2 * np.abs(y / q)) / N, inf, zero)
    raise KeyError(loss)


def evaluate(act, loss, z, y):
    z, y = np.asarray(z, np.float64), np.asarray(y, np.float64)
    z, y = z.reshape(z.shape[0], -1), y.reshape(y.shape[0], -1)
    M, N = z.shape
    p = probs(act, z)
    ev = SimpleNamespace(act=act, loss_name=loss, z=z, y=y, probs=p, M=M, N=N, direct=False)
    exact_p = act == "softmax" and N == 1            # p == 1 exactly in every precision
    if loss == "binary_crossentropy":
        assert act == "sigmoid"
        l, dz, cor, _ = H.sigmoid_bce(z.reshape(-1), y.reshape(-1))
        pc = np.clip(p, H.LO, H.HI)
        on = (p >= H.LO) & (p <= H.HI)
        ev.l_el, ev.g = l.reshape(M, N) / N, dz.reshape(M, N) / N
        ev.gp, ev.Gmag = on / N, (pc + np.abs(y)) / N
        ev.Lmag = H.sigmoid_loss_bound(z.reshape(-1), y.reshape(-1)).reshape(M, N) / N / (16 * U)
        ev.margin, ev.jump = np.minimum(np.abs(p - H.LO), np.abs(p - H.HI)), np.abs(pc - y) / N
        ev.direct = True
    elif loss == "categorical_hinge":
        pos = (y * p).sum(1)
        negs = (1 - y) * p
        m = first_argmax(negs)
        neg = negs[np.arange(M), m]
        v = neg - pos + 1
        first = np.eye(N)[m]
        ev.l_el = np.zeros_like(p)
        ev.l_el[:, 0] = np.maximum(v, 0)
        ev.g = np.where((v > 0)[:, None], -y + first * (1 - y), 0.0)
        ev.gp = np.zeros_like(p)
        ev.Lmag = np.zeros_like(p)
        ev.Lmag[:, 0] = np.abs(y * p).sum(1) + np.abs(neg) + 1
        ev.Gmag = (1 + np.abs(y)) * (v > 0)[:, None]
        # row-level kinks, in units of p: v = 0 (v moves by at most sum |y| dp + dp) and the two
        # largest (1 - y) p tied; a row near either is marked whole
        srt = np.sort(negs, axis=1)
        gap = srt[:, -1] - srt[:, -2] if N > 1 else np.full(M, np.inf)
        scale = np.abs(y).sum(1) + np.abs(1 - y).max(1)
        ev.margin = np.minimum(np.abs(v) / np.maximum(scale, 1e-300), gap / np.maximum(2 * np.abs(1 - y).max(1), 1e-300))[:, None] + 0 * p
        ev.jump = 1 + 2 * np.abs(y) + 0 * p
    else:
        ev.l_el, ev.g, ev.gp, ev.Lmag, ev.Gmag, ev.margin, ev.jump = _elementwise(loss, p, y, N)
    ev.loss = ev.l_el.sum(1)
    ev.dz = _chain(ev, ev.g)
    if N == 1 or loss == "binary_crossentropy":
        ev.binary = True
        ev.correct = (np.rint(p) == y).sum(1).astype(np.float64)
        ev.acc_margin = np.abs(p - np.floor(p) - 0.5)          # distance to the nearest half-integer
    else:
        ev.binary = False
        ev.correct = (first_argmax(p) == first_argmax(y)).astype(np.float64)
        srt = np.sort(p, axis=1)
        ev.acc_margin = ((srt[:, -1] - srt[:, -2]) / 2)[:, None] + 0 * p
    ev.exact_p = exact_p
    return ev


def _chain(ev, g):
    p = ev.probs
    if ev.direct or ev.act is None:
        return g.copy()
    if ev.act == "sigmoid":
        return g * p * (1 - p)
    return p * (g - (p * g).sum(1, keepdims=True))


def logit_error_bound(a, W, b):
    """Bound on |float32 logits - float64 logits| of z = a W + b, a [M, K]: (K + 2) u sum |a| |w|."""
    a, W, b = np.asarray(a, np.float64), np.asarray(W, np.float64), np.asarray(b, np.float64).reshape(-1)
    return (a.shape[1] + 2) * U * (np.abs(a) @ np.abs(W) + np.abs(b)[None, :])


def bounds(ev, dzl):
    """SimpleNamespace(dp, loss [M], dz [M, N], near_kink [M, N], dz_jump [M, N], acc_ambiguous [M])."""
    p, g, gp = ev.probs, ev.g, ev.gp
    dzl = np.broadcast_to(np.asarray(dzl, np.float64), p.shape)
    if ev.exact_p:
        dp = np.zeros_like(p)
    elif ev.act is None:
        dp = dzl + 0.0
    elif ev.act == "sigmoid":
        dp = p * (1 - p) * dzl + 8 * U * p
    else:
        dp = p * (dzl + (p * dzl).sum(1, keepdims=True)) + 16 * U * p
    c = 16 * U
    with np.errstate(invalid="ignore"):
        if ev.direct:
            loss_b = (np.abs(ev.g) * dzl + c * ev.Lmag).sum(1)
            dz_b = np.abs(gp) * dp + c * ev.Gmag
        else:
            loss_b = (np.abs(g) * dp + c * ev.Lmag).sum(1)
            if ev.act is None:
                dz_b = np.abs(gp) * dp + c * ev.Gmag
            elif ev.act == "sigmoid":
                dz_b = (np.abs(gp * p * (1 - p) + g * (1 - 2 * p)) * dp + c * (ev.Gmag + np.abs(g)) * p * (1 - p)
                        + 2 * U * np.abs(g) * p)
            else:
                S = (p * g).sum(1, keepdims=True)
                dz_b = (np.abs(g - S + p * gp) * dp + p * (np.abs(g + p * gp) * dp).sum(1, keepdims=True)
                        + c * p * (ev.Gmag + np.abs(g) + (p * (ev.Gmag + np.abs(g))).sum(1, keepdims=True)))
    near = ev.margin <= dp + 2 * U * np.maximum(1.0, np.abs(p))
    if ev.exact_p:
        near = np.zeros_like(near)
    jump = np.where(near, ev.jump, 0.0)
    if ev.direct or ev.act is None:
        dz_jump = jump
    elif ev.act == "sigmoid":
        dz_jump = jump * p * (1 - p)
    else:
        dz_jump = p * (jump + (p * jump).sum(1, keepdims=True))
    amb = ev.acc_margin <= dp + 2 * U * np.maximum(1.0, np.abs(p))
    amb = amb.sum(1) if ev.binary else amb.any(1).astype(np.int64)
    return SimpleNamespace(dp=dp, loss=2 * loss_b, dz=2 * dz_b, near_kink=near, dz_jump=dz_jump, acc_ambiguous=amb)


# ----------------------------------------------------------------------------- inputs
def draw(loss, act, M, N, seed=0):
    """(Z* [M, N] float64 logits to place, y [M, N] float32 targets), drawn CONTINUOUS (no value
    sits on a kink by construction) from each loss's natural range; a linear output straddles the
    clip edges of msle / kld, and stays positive for poisson (whose log needs p + eps > 0)."""
    rs = np.random.RandomState(1000 + seed + 17 * M + 131 * N + 7 * LOSSES.index(loss) if loss in LOSSES else seed + M + N)
    Z = 1.5 * rs.randn(M, N)
    if loss in ("hinge", "squared_hinge"):
        y = np.where(rs.rand(M, N) < 0.5, -1.0, 1.0)
    elif loss == "categorical_hinge":
        y = np.eye(N)[rs.randint(0, N, M)]
    elif loss == "binary_crossentropy":
        y = (rs.rand(M, N) < 0.5).astype(np.float64)
        Z = 3.0 * rs.randn(M, N)
    elif loss == "msle":
        y = 3.0 * rs.rand(M, N)
        if act is None:
            Z = rs.uniform(-0.5, 3.0, (M, N))
    elif loss == "kld":
        e = np.exp(rs.randn(M, N))
        y = e / e.sum(1, keepdims=True)
        if act is None:
            Z = rs.uniform(-0.2, 1.2, (M, N))
    elif loss == "poisson":
        y = rs.poisson(2.0, (M, N)).astype(np.float64)
        if act is None:
            Z = rs.uniform(0.2, 4.0, (M, N))
    elif act is None:
        y = rs.uniform(-1.0, 1.0, (M, N))
    else:
        y = rs.rand(M, N)
    return Z, y.astype(np.float32)


# ----------------------------------------------------------------------------- the kernel test's cases
MS, NS, KS = (1, 3, 4, 5, 26), (1, 2, 3, 15, 16), (5, 64, 65, 130)


def kernel_cases():
    """[(act, loss, M, N, K, arch)] of tests/test_loss_head_gpu.py's kernel test, which the CPU proof
    (tests/test_loss_head.py) runs through the float32 reference too.  Every loss on its natural
    activation at every N (the multi-label binary_crossentropy at every N > 1), every other
    (activation, loss) pair once, M / N / K cycling through the borders of four rows per
    workgroup, the class counts and K * N on both sides of HEAD_W_LDS = 2048 (130 x 15 = 1950,
    130 x 16 = 2080).  arch 'dense': the head behind a hidden Dense(K); 'conv': on a flattened
    pooled conv of 3 channels padded to 8 (K = 4 * 4 * 3 = 48)."""
    out, i = [], 0
    for loss in LOSSES + ("binary_crossentropy",):
        for N in NS:
            if loss == "binary_crossentropy" and N == 1:
                continue                    # (the one-column pair is the first head kernel's)
            arch = "conv" if i % 4 == 2 else "dense"
            out.append((NATURAL[loss], loss, MS[i % 5], N, 48 if arch == "conv" else KS[(i + N) % 4], arch))
            i += 1
    for loss in LOSSES:
        for act in ACTS:
            if act != NATURAL[loss] and (act, loss) in KERNEL_PAIRS:
                arch = "conv" if i % 4 == 2 else "dense"
                # (poisson on a linear output needs every placed logit positive: rows <= K, exact placement)
                M = 4 if (act, loss) == (None, "poisson") else MS[i % 5]
                out.append((act, loss, M, NS[i % 5], 48 if arch == "conv" else KS[i % 4] if M <= 5 else KS[1 + i % 3], arch))
                i += 1
    out += [(None, "mae", 26, 15, 130, "dense"), (None, "mae", 26, 16, 130, "dense"),
            ("sigmoid", "binary_crossentropy", 5, 15, 130, "dense"), ("sigmoid", "binary_crossentropy", 5, 16, 130, "dense")]
    return out


def synthetic_input(M, K, seed=0):
    """A head input like a ReLU stage's stored output: non-negative, bf16-representable, full rank."""
    a = np.maximum(np.random.RandomState(77 + seed + M + 3 * K).randn(M, K), 0.0) + 0.01
    return (a.astype(np.float32).view(np.uint32) & 0xFFFF0000).view(np.float32).astype(np.float64)


def place(a, Zs, b):
    """float32 head weights W with a W + b ~= Zs (least squares; exact where rank(a) >= rows)."""
    return np.linalg.lstsq(a, Zs - np.asarray(b, np.float64), rcond=None)[0].astype(np.float32)


def tie_cases():
    """[(name, loss, z [1, N], y [1, N], want dz [1, N])] on a LINEAR output whose logits are exact
    (zero weights, the bias is the logit): one per subgradient convention."""
    e = float(np.float32(1e-7))
    c = []
    c.append(("hinge margin exactly 0 takes -y/N", "hinge", [[1.0, -1.0, 0.5]], [[1.0, -1.0, 1.0]], [[-1 / 3, 1 / 3, -1 / 3]]))
    c.append(("mae p == y has sign 0", "mae", [[0.25, 0.5, -1.0]], [[0.25, 0.0, -1.0]], [[0.0, 1 / 3, 0.0]]))
    c.append(("categorical_hinge tied maxima: the first", "categorical_hinge", [[0.5, 0.5, 0.5, 0.5]], [[0.0, 1.0, 0.0, 0.0]],
              [[1.0, -1.0, 0.0, 0.0]]))
    c.append(("kld p == eps and p == 1 pass", "kld", [[e, 1.0, 0.5]], [[0.5, 0.25, 0.25]], [[-0.5 / e, -0.25, -0.5]]))
    pm = e + 1.0
    c.append(("msle p == eps passes", "msle", [[e, 1.0]], [[1.0, 1.0]],
              [[2 * (np.log(pm) - np.log(2.0)) / pm / 2, 0.0]]))
    return c

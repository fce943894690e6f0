"""Float64 NumPy oracle of the output head: sigmoid + binary_crossentropy, softmax +
categorical_crossentropy and linear + mse, per row, with the Keras / TF clipping semantics of
``ops/reference.py`` and two differences that matter to a float32 kernel:

* the probability clip uses the FLOAT32 bounds TF computes with, ``float32(1e-7)`` and
  ``float32(1) - float32(1e-7)`` = 1 - 2**-23 (0.99999988...), not the float64 1 - 1e-7: a
  saturated sigmoid row's loss is log(2**23 - 1) = 15.94, not 16.118;
* ``correct`` is spelled out: first-maximum argmax of logits AND targets (softmax),
  round-half-even of p (sigmoid: p = 0.5 exactly rounds to 0).

Every function takes float64-convertible arrays and returns per-row
``(loss [M], dz [M, N], correct [M], probs [M, N])``; dz is dL/dlogits of the row (not / M).
"""
import numpy as np

LO = float(np.float32(1e-7))
HI = float(np.float32(1) - np.float32(1e-7))
LOGIT_CLIP = float(np.log(1e7))          # |logit of a probability| where the clip starts


def _f64(a, ndim):
    a = np.asarray(a, np.float64)
    return a.reshape(a.shape[0], -1) if ndim == 2 else a.reshape(-1)


def sigmoid_bce(z, y):
    z, y = _f64(z, 1), _f64(y, 1)
    with np.errstate(over="ignore"):
        p = 1.0 / (1.0 + np.exp(-z))
    inr = (p >= LO) & (p <= HI)
    pc = np.clip(p, LO, HI)
    lg = np.log(pc / (1.0 - pc))
    loss = np.maximum(lg, 0.0) - lg * y + np.log1p(np.exp(-np.abs(lg)))
    dz = np.where(inr, pc - y, 0.0)
    correct = (np.rint(p) == y).astype(np.float64)      # np.rint: round-half-even
    return loss, dz.reshape(-1, 1), correct, p.reshape(-1, 1)


def sigmoid_loss_bound(z, y):
    """Per-row bound on |float32 loss - oracle loss| of ``sigmoid_bce``.

    Keras goes back from p to a logit, log(pc / (1 - pc)): a float32 rounding of p (relative
    2**-24) moves that logit by 2**-24 / (1 - pc) near 1 and by 2**-24 near 0, i.e. by at most
    2**-24 / (pc * (1 - pc)).  Two such roundings (p itself and 1 - p), doubled, give the first
    term; the second covers the float32 evaluation of the log / log1p / exp chain at the loss's
    magnitude.  In a clipped row pc is exactly LO or HI in both precisions, so the first term
    is zero there."""
    loss, _, _, p = sigmoid_bce(z, y)
    p = p.reshape(-1)
    inr = (p >= LO) & (p <= HI)
    pc = np.clip(p, LO, HI)
    u = 4.0 * 2.0 ** -24
    return np.where(inr, u / (pc * (1.0 - pc)), 0.0) + u * np.maximum(1.0, loss)


def softmax_cce(z, y):
    z, y = _f64(z, 2), _f64(y, 2)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    s = p.sum(axis=1, keepdims=True)
    q = p / s
    inr = (q >= LO) & (q <= HI)
    qc = np.clip(q, LO, HI)
    loss = -(y * np.log(qc)).sum(axis=1)
    g = np.where(inr, -y / qc, 0.0)                                  # dL/dq
    gp = (g - (g * q).sum(axis=1, keepdims=True)) / s                # through the renormalisation
    dz = p * (gp - (p * gp).sum(axis=1, keepdims=True))              # softmax jacobian
    correct = (np.argmax(z, axis=1) == np.argmax(y, axis=1)).astype(np.float64)   # first maximum
    return loss, dz, correct, p


def mse(z, y):
    z, y = _f64(z, 2), _f64(y, 2)
    d = z - y
    return (d * d).mean(axis=1), 2.0 * d / z.shape[1], np.zeros(z.shape[0]), z


def prob_logits(z, act):
    """The logit log(q / (1 - q)) of every output probability: the clip acts where its
    magnitude passes LOGIT_CLIP.  Sigmoid: z itself; softmax: z_n - logsumexp(z_others)."""
    z = _f64(z, 2)
    if act == "sigmoid":
        return z
    out = np.empty_like(z)
    for n in range(z.shape[1]):
        o = np.delete(z, n, axis=1)
        mx = o.max(axis=1)
        out[:, n] = z[:, n] - (mx + np.log(np.exp(o - mx[:, None]).sum(axis=1)))
    return out


def weight_factor(w):
    """Row factors of the sample-weighted loss: w_i * M / nnz (``ops/reference.py``)."""
    w = np.asarray(w, np.float64).reshape(-1)
    return w * (w.shape[0] / max(int((w != 0).sum()), 1))


# ----------------------------------------------------------------------------- crafted logits
IN_GAPS = (0.5, 3.0, 8.0, 12.0, 13.0)      # >= 2 below LOGIT_CLIP = 16.118
CLIP_GAPS = (20.0, 25.0, 40.0)             # >= 2 above it


def _gaps(regime):
    if regime == "in":
        return list(IN_GAPS)
    if regime == "clip":
        return list(CLIP_GAPS)
    return [g for pair in zip(IN_GAPS, (CLIP_GAPS * 2)[:len(IN_GAPS)]) for g in pair]     # mixed: alternate


def _pick(regime, r, variants):
    """Row r's (gap, variant): the gaps cycle fastest and each gap walks through the variants,
    so 4 * len(gaps) rows see every combination and fewer rows still see every gap."""
    gaps = _gaps(regime)
    return gaps[r % len(gaps)], variants[(r // len(gaps) + r % len(gaps)) % len(variants)]


def sigmoid_table(regime, m):
    """(Z* [m, 1], y [m, 1]): z = +-gap for y in {0, 1}."""
    Z, Y = np.zeros((m, 1)), np.zeros((m, 1), np.float32)
    for r in range(m):
        g, (s, yv) = _pick(regime, r, [(1.0, 0.0), (-1.0, 1.0), (1.0, 1.0), (-1.0, 0.0)])
        Z[r, 0], Y[r, 0] = s * g, yv
    return Z, Y


def softmax_table(regime, m, n):
    """(Z* [m, n], y [m, n]).  Row families, true class t cycling over the classes:

    * t ABOVE / BELOW the rest by a gap: one rival class at logit 0, t at +-gap from the
      logsumexp of the rest (so the logit of q_t is +-gap exactly), the other classes a deep
      tail at -25 - 3j whose probabilities are clipped in every regime;
    * the same rows with smoothed targets 0.9 y + 0.1 / n;
    * (regimes "in" and "mixed": the last rows) every class in range: a permutation of
      linspace(-2, 2, n), true class the maximum or another one.

    Top-2 logit margins are >= 0.25, so float32 logit error cannot flip an argmax."""
    n_dense = min({"in": 6, "mixed": 4, "clip": 0}[regime], m // 4)
    rs = np.random.RandomState(7)
    Z, Y = np.zeros((m, n)), np.zeros((m, n), np.float32)
    for r in range(m):
        t = r % n
        if r >= m - n_dense:
            Z[r] = rs.permutation(np.linspace(-2.0, 2.0, n))
            if r % 2:
                t = int(np.argmax(Z[r]))
            Y[r, t] = 1.0
            continue
        g, (up, sm) = _pick(regime, r, [(True, False), (False, False), (True, True), (False, True)])
        rest = [c for c in range(n) if c != t]
        Z[r, rest[0]] = 0.0
        for j, c in enumerate(rest[1:]):
            Z[r, c] = -25.0 - 3.0 * j
        lse = np.log(np.exp(Z[r, rest]).sum())
        Z[r, t] = lse + (g if up else -g)
        Y[r, t] = 1.0
        if sm:
            Y[r] = (0.9 * Y[r] + 0.1 / n).astype(np.float32)
    return Z, Y


def regime_of(z, act):
    """Per-row regime from the logits the kernel saw: "in" (no probability clipped), "clip"
    (every probability clipped) or "mixed" row; raises if any probability's logit lies within
    2 of the clip threshold (14 < |logit| < 18), where float32 and float64 may disagree on
    the branch."""
    a = np.abs(prob_logits(z, act))
    bad = (a > 14.0) & (a < 18.0)
    if bad.any():
        raise AssertionError("rows %s lie within 2 of the clip threshold" % sorted(set(np.nonzero(bad)[0].tolist())))
    c = a >= 18.0
    return np.where(c.all(axis=1), "clip", np.where(c.any(axis=1), "mixed", "in"))

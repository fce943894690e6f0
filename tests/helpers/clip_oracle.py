"""float64 NumPy oracle of Keras 2.2.4 gradient clipping, written from
``keras.optimizers.Optimizer.get_gradients`` / ``clip_norm`` (not from ops/reference.py, which it
checks):

    clipnorm = c > 0:   n = sqrt(sum over ALL parameters of g^2)          (one global norm)
                        g = g * (c / n)  if n >= c  else g                 (quotient first)
                        (n == 0 and a NaN n fail the comparison: g unchanged, nothing divided)
    clipvalue = v > 0:  g = min(max(g, -v), v)                             (after the norm clip)

and of the Keras updates helpers/optim_oracle.py does not have (SGD with momentum / Nesterov,
Adadelta, Nadam), so that ``step`` below covers every kind the clipping tests use: it clips the
gradient and hands it to the update -- the optimizer's state sees the clipped gradient.

Every function returns new arrays and leaves its inputs alone."""
import numpy as np

from . import optim_oracle as O


def global_norm(g):
    g = np.asarray(g, dtype=np.float64)
    return float(np.sqrt(np.sum(g * g)))


def clip(g, clipnorm=None, clipvalue=None):
    """(clipped g, info) with info = {"norm": n or None, "fired": the norm clip scaled g,
    "clamped": elements the value clip changed}."""
    g = np.array(g, dtype=np.float64)
    info = {"norm": None, "fired": False, "clamped": 0}
    if clipnorm is not None and clipnorm > 0:
        n = global_norm(g)
        info["norm"] = n
        if n >= clipnorm:
            g = g * (clipnorm / n)
            info["fired"] = True
    if clipvalue is not None and clipvalue > 0:
        info["clamped"] = int(np.sum(np.abs(g) > clipvalue))
        g = np.minimum(np.maximum(g, -clipvalue), clipvalue)
    return g, info


def sgd(p, g, mom, lr, momentum=0.0, nesterov=False):
    p, g = O._f64(p, g)
    if not momentum:
        return p - lr * g, []
    v = momentum * np.asarray(mom, dtype=np.float64) - lr * g
    return (p + momentum * v - lr * g) if nesterov else (p + v), [v]


def adadelta(p, g, a, d, lr, rho=0.95, eps=O.EPS):
    p, g, a, d = O._f64(p, g, a, d)
    a = rho * a + (1.0 - rho) * g * g
    upd = g * np.sqrt(d + eps) / np.sqrt(a + eps)
    return p - lr * upd, a, rho * d + (1.0 - rho) * upd * upd


def nadam(p, g, m, v, t, lr, beta_1=0.9, beta_2=0.999, eps=O.EPS, schedule_decay=0.004):
    p, g, m, v = O._f64(p, g, m, v)
    mc = lambda i: beta_1 * (1.0 - 0.5 * 0.96 ** (i * schedule_decay))
    m_sched_new = float(np.prod([mc(i) for i in range(1, t + 1)]))      # m_schedule starts at 1
    m_sched_next = m_sched_new * mc(t + 1)
    gp = g / (1.0 - m_sched_new)
    m = beta_1 * m + (1.0 - beta_1) * g
    mp = m / (1.0 - m_sched_next)
    v = beta_2 * v + (1.0 - beta_2) * g * g
    vp = v / (1.0 - beta_2 ** t)
    mbar = (1.0 - mc(t)) * gp + mc(t + 1) * mp
    return p - lr * mbar / (np.sqrt(vp) + eps), m, v


def update(kind, p, g, slots, t, opt):
    """One unclipped update of any kind the clipping tests use; returns (p, [slots])."""
    if kind in ("adagrad", "adamax", "amsgrad", "adam"):
        return O.step(kind, p, g, slots, t, opt)
    if kind == "nadam":       # (Keras' Nadam has no decay)
        p, m, v = nadam(p, g, slots[0], slots[1], t, float(opt.lr), opt.beta_1, opt.beta_2, opt.epsilon,
                        opt.schedule_decay)
        return p, [m, v]
    lr = O.decayed_lr(float(opt.lr), opt.initial_decay, t)
    if kind == "sgd":
        return sgd(p, g, slots[0] if slots else None, lr, opt.momentum, opt.nesterov)
    if kind == "adadelta":
        p, a, d = adadelta(p, g, slots[0], slots[1], lr, opt.rho, opt.epsilon)
        return p, [a, d]
    raise ValueError(kind)


def step(kind, p, g, slots, t, opt, clipnorm=None, clipvalue=None):
    """Clip ``g`` (the unclipped gradient), then update: (p, [slots], clip info)."""
    gc, info = clip(g, clipnorm, clipvalue)
    p, slots = update(kind, p, gc, slots, t, opt)
    return p, slots, info

"""float64 NumPy oracle of the Keras 2.2.4 Adagrad, Adamax and Adam / AMSGrad updates, written
from the formulas of keras/optimizers.py (not from ops/reference.py, which it checks):

    lr   = lr0 / (1 + decay * (t - 1))                     t: the 1-based step
    Adagrad:  a = a + g^2;               p = p - lr * g / (sqrt(a) + eps)
    Adamax:   lr_t = lr / (1 - b1^t);    m = b1 m + (1 - b1) g;   u = max(b2 u, |g|)
              p = p - lr_t * m / (u + eps)
    Adam:     lr_t = lr sqrt(1 - b2^t) / (1 - b1^t);   m as above;   v = b2 v + (1 - b2) g^2
              p = p - lr_t * m / (sqrt(v) + eps)
    AMSGrad:  Adam's lr_t, m, v;   vhat = max(vhat, v);   p = p - lr_t * m / (sqrt(vhat) + eps)

Every function returns new arrays (p, slots...) and leaves its inputs alone."""
import numpy as np

EPS = 1e-7


def _f64(*xs):
    return [np.asarray(x, dtype=np.float64) for x in xs]


def decayed_lr(lr, decay, t):
    return lr / (1.0 + decay * (t - 1))


def adagrad(p, g, a, lr, eps=EPS):
    p, g, a = _f64(p, g, a)
    a = a + g * g
    return p - lr * g / (np.sqrt(a) + eps), a


def adamax(p, g, m, u, t, lr, beta_1=0.9, beta_2=0.999, eps=EPS):
    p, g, m, u = _f64(p, g, m, u)
    lr_t = lr / (1.0 - beta_1 ** t)
    m = beta_1 * m + (1.0 - beta_1) * g
    u = np.maximum(beta_2 * u, np.abs(g))
    return p - lr_t * m / (u + eps), m, u


def adam(p, g, m, v, t, lr, beta_1=0.9, beta_2=0.999, eps=EPS):
    p, g, m, v = _f64(p, g, m, v)
    lr_t = lr * np.sqrt(1.0 - beta_2 ** t) / (1.0 - beta_1 ** t)
    m = beta_1 * m + (1.0 - beta_1) * g
    v = beta_2 * v + (1.0 - beta_2) * g * g
    return p - lr_t * m / (np.sqrt(v) + eps), m, v


def amsgrad(p, g, m, v, vhat, t, lr, beta_1=0.9, beta_2=0.999, eps=EPS):
    p, g, m, v, vhat = _f64(p, g, m, v, vhat)
    lr_t = lr * np.sqrt(1.0 - beta_2 ** t) / (1.0 - beta_1 ** t)
    m = beta_1 * m + (1.0 - beta_1) * g
    v = beta_2 * v + (1.0 - beta_2) * g * g
    vhat = np.maximum(vhat, v)
    return p - lr_t * m / (np.sqrt(vhat) + eps), m, v, vhat


def step(kind, p, g, slots, t, opt):
    """One update of optimizer kind ``kind`` ("adagrad" / "adamax" / "amsgrad" / "adam") with the
    hyper-parameters of the optimizer object ``opt``; returns (p, [slots])."""
    lr = decayed_lr(float(opt.lr), opt.initial_decay, t)
    if kind == "adagrad":
        p, a = adagrad(p, g, slots[0], lr, opt.epsilon)
        return p, [a]
    if kind == "adamax":
        p, m, u = adamax(p, g, slots[0], slots[1], t, lr, opt.beta_1, opt.beta_2, opt.epsilon)
        return p, [m, u]
    if kind == "amsgrad":
        p, m, v, vh = amsgrad(p, g, slots[0], slots[1], slots[2], t, lr, opt.beta_1, opt.beta_2, opt.epsilon)
        return p, [m, v, vh]
    if kind == "adam":
        p, m, v = adam(p, g, slots[0], slots[1], t, lr, opt.beta_1, opt.beta_2, opt.epsilon)
        return p, [m, v]
    raise ValueError(kind)

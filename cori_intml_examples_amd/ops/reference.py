"""Plain-PyTorch fp32 reference implementations of every fused op.

These serve two roles:
  * the oracle that the HIP-kernel numerics tests compare against, and
  * the CPU plumbing backend (BASELINE config "MNIST 3-layer CNN single-process
    Keras fit() on CPU").

Layouts follow Keras ``channels_last`` (``mnist.py:30``): activations NHWC,
conv kernels (KH, KW, Cin, Cout), dense kernels (in, out).  Semantics follow the
Keras 2.2 / TF 1.x ops the reference executes.
"""
from __future__ import annotations

import math
from typing import Tuple

import torch
import torch.nn.functional as F

EPS = 1e-7  # keras.backend.epsilon()


# --------------------------------------------------------------------------- conv geometry
def conv_out_size(n: int, k: int, s: int, padding: str) -> int:
    if padding == "same":
        return -(-n // s)
    return (n - k) // s + 1


def same_pad(n: int, k: int, s: int) -> Tuple[int, int]:
    """TF 'same' padding split (extra row/col goes to the bottom/right)."""
    out = -(-n // s)
    total = max((out - 1) * s + k - n, 0)
    return total // 2, total - total // 2


def conv_pads(h: int, w: int, kh: int, kw: int, s: int, padding: str):
    if padding == "same":
        pt, pb = same_pad(h, kh, s)
        pl, pr = same_pad(w, kw, s)
        return pt, pb, pl, pr
    return 0, 0, 0, 0


# --------------------------------------------------------------------------- conv
def conv2d(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor | None, stride: int = 1,
           padding: str = "valid") -> torch.Tensor:
    """x [B,H,W,C], w [KH,KW,C,Co] -> y [B,Ho,Wo,Co] (no activation)."""
    kh, kw = w.shape[0], w.shape[1]
    pt, pb, pl, pr = conv_pads(x.shape[1], x.shape[2], kh, kw, stride, padding)
    xn = x.permute(0, 3, 1, 2)
    if pt or pb or pl or pr:
        xn = F.pad(xn, (pl, pr, pt, pb))
    y = F.conv2d(xn, w.permute(3, 2, 0, 1), b, stride=stride)
    return y.permute(0, 2, 3, 1)


def conv2d_backward(x: torch.Tensor, w: torch.Tensor, dy: torch.Tensor, stride: int,
                    padding: str, need_dx: bool = True):
    """Returns (dx or None, dw [KH,KW,C,Co], db [Co])."""
    with torch.enable_grad():
        xr = x.detach().clone().requires_grad_(need_dx)
        wr = w.detach().clone().requires_grad_(True)
        y = conv2d(xr, wr, None, stride, padding)
        y.backward(dy)
    db = dy.sum(dim=(0, 1, 2))
    return (xr.grad if need_dx else None), wr.grad, db


# --------------------------------------------------------------------------- pool
def maxpool2x2(x: torch.Tensor):
    """2x2/2 valid max-pool on NHWC.  Returns (y, code) where code in {0..3} is the
    window position (dy*2+dx) of the FIRST maximum in row-major order."""
    B, H, W, C = x.shape
    Hp, Wp = H // 2, W // 2
    xw = x[:, :Hp * 2, :Wp * 2, :].reshape(B, Hp, 2, Wp, 2, C).permute(0, 1, 3, 2, 4, 5)
    xw = xw.reshape(B, Hp, Wp, 4, C)
    y, code = xw.max(dim=3)
    # torch.max returns *a* max index; enforce first-max tie-breaking explicitly
    eq = xw == y.unsqueeze(3)
    pos = torch.arange(4, device=x.device).view(1, 1, 1, 4, 1)
    code = torch.where(eq, pos, torch.full_like(pos, 4)).min(dim=3).values
    return y, code.to(torch.uint8)


def maxpool2x2_backward(dy: torch.Tensor, code: torch.Tensor, in_hw: Tuple[int, int]) -> torch.Tensor:
    B, Hp, Wp, C = dy.shape
    H, W = in_hw
    onehot = F.one_hot(code.long(), 4).permute(0, 1, 2, 4, 3).to(dy.dtype)  # B,Hp,Wp,4,C
    g = onehot * dy.unsqueeze(3)
    g = g.reshape(B, Hp, Wp, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, Hp * 2, Wp * 2, C)
    out = torch.zeros(B, H, W, C, dtype=dy.dtype, device=dy.device)
    out[:, :Hp * 2, :Wp * 2, :] = g
    return out


def avgpool2x2(x: torch.Tensor) -> torch.Tensor:
    """2x2/2 valid average pool on NHWC: 0.25 * ((a + b) + (c + d)) with a b / c d the window in
    row-major order (pool.hip's order); a leftover odd row / column contributes nothing."""
    B, H, W, C = x.shape
    Hp, Wp = H // 2, W // 2
    xw = x[:, :Hp * 2, :Wp * 2, :].reshape(B, Hp, 2, Wp, 2, C)
    return ((xw[:, :, 0, :, 0] + xw[:, :, 0, :, 1]) + (xw[:, :, 1, :, 0] + xw[:, :, 1, :, 1])) * 0.25


def avgpool2x2_backward(dy: torch.Tensor, in_hw: Tuple[int, int]) -> torch.Tensor:
    """0.25 * dy at each of a window's four pixels; zero in a leftover odd row / column."""
    B, Hp, Wp, C = dy.shape
    out = torch.zeros(B, in_hw[0], in_hw[1], C, dtype=dy.dtype, device=dy.device)
    out[:, :Hp * 2, :Wp * 2, :] = (dy * 0.25).repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    return out


def global_avgpool(x: torch.Tensor) -> torch.Tensor:
    """Mean over H and W of NHWC: the sum times fp32(1 / (H * W))."""
    B, H, W, C = x.shape
    return x.reshape(B, H * W, C).sum(1) * torch.tensor(1.0 / (H * W), dtype=x.dtype)


def global_avgpool_backward(dy: torch.Tensor, in_hw: Tuple[int, int]) -> torch.Tensor:
    H, W = in_hw
    g = dy * torch.tensor(1.0 / (H * W), dtype=dy.dtype)
    return g[:, None, None, :].expand(-1, H, W, -1).clone()


def global_maxpool(x: torch.Tensor):
    """Maximum over H and W of NHWC.  Returns (y, index) with index the flat y * W + x of the FIRST
    maximum in row-major order (int64 [B, C])."""
    B, H, W, C = x.shape
    xf = x.reshape(B, H * W, C)
    y = xf.max(dim=1).values
    pos = torch.arange(H * W, device=x.device).view(1, H * W, 1)
    idx = torch.where(xf == y.unsqueeze(1), pos, torch.full_like(pos, H * W)).min(dim=1).values
    return y, idx


def global_maxpool_backward(dy: torch.Tensor, idx: torch.Tensor, in_hw: Tuple[int, int]) -> torch.Tensor:
    """The whole gradient at the saved index, zero elsewhere."""
    H, W = in_hw
    B, C = dy.shape
    out = torch.zeros(B, H * W, C, dtype=dy.dtype, device=dy.device)
    out.scatter_(1, idx.view(B, 1, C), dy.view(B, 1, C))
    return out.reshape(B, H, W, C)


# --------------------------------------------------------------------------- activations
# The hidden activations beyond relu / linear (Keras 2.2.4 keras/activations.py and the
# LeakyReLU / ELU layers): name -> whether it takes an alpha.  Every function is non-decreasing
# and every derivative is a function of the OUTPUT, clamped to >= 0.
ACTIVATIONS = {"tanh": False, "sigmoid": False, "hard_sigmoid": False, "elu": True, "selu": False,
               "softplus": False, "softsign": False, "leaky_relu": True}
SELU_SCALE, SELU_ALPHA = 1.0507009873554805, 1.6732632423543772


def act(name: str, alpha: float, x: torch.Tensor) -> torch.Tensor:
    """A(x) of the activation table, in x's dtype (fp32 twin of act_fwd_kernel)."""
    if name == "tanh":
        return torch.tanh(x)
    if name == "sigmoid":
        return 1.0 / (1.0 + torch.exp(-x))
    if name == "hard_sigmoid":
        v = 0.2 * x + 0.5
        return torch.where(v < 0, torch.zeros_like(v), torch.where(v > 1, torch.ones_like(v), v))
    if name == "elu":
        return torch.where(x > 0, x, alpha * torch.expm1(x))
    if name == "selu":
        return SELU_SCALE * torch.where(x > 0, x, SELU_ALPHA * torch.expm1(x))
    if name == "softplus":
        return torch.where(x > 0, x, torch.where(x < 0, torch.zeros_like(x), x)) + torch.log1p(torch.exp(-x.abs()))
    if name == "softsign":
        return torch.where(torch.isinf(x), torch.sign(x), x / (1.0 + x.abs()))
    if name == "leaky_relu":
        neg = torch.zeros_like(x) if alpha == 0 else alpha * x      # (alpha = 0 is relu, also at -inf)
        return torch.where(x > 0, x, torch.where(x < 0, neg, alpha * x))
    raise NotImplementedError("activation %r" % (name,))


def act_grad_from_output(name: str, alpha: float, y: torch.Tensor) -> torch.Tensor:
    """dA/dx as a function of the output y = A(x), clamped to >= 0 (fp32 twin of act_bwd_kernel)."""
    zero = torch.zeros_like(y)
    if name == "tanh":
        return torch.maximum(zero, 1.0 - y * y)
    if name == "sigmoid":
        return torch.maximum(zero, y * (1.0 - y))
    if name == "hard_sigmoid":
        return torch.where((y > 0) & (y < 1), torch.full_like(y, 0.2), zero)
    if name == "elu":
        return torch.where(y > 0, torch.ones_like(y), torch.maximum(zero, y + alpha))
    if name == "selu":
        return torch.where(y > 0, torch.full_like(y, SELU_SCALE), torch.maximum(zero, y + SELU_SCALE * SELU_ALPHA))
    if name == "softplus":
        return torch.maximum(zero, -torch.expm1(-y))
    if name == "softsign":
        d = 1.0 - torch.minimum(y.abs(), torch.ones_like(y))
        return d * d
    if name == "leaky_relu":
        return torch.where(y > 0, torch.ones_like(y), torch.full_like(y, alpha))
    raise NotImplementedError("activation %r" % (name,))


# --------------------------------------------------------------------------- losses
def softmax_cce(logits: torch.Tensor, y: torch.Tensor):
    """Keras categorical_crossentropy on a softmax output (TF backend semantics).

    Returns (loss_per_row, dlogits_per_row (not /B), correct_per_row)."""
    p = torch.softmax(logits, dim=-1)
    s = p.sum(dim=-1, keepdim=True)
    q = p / s
    inr = (q >= EPS) & (q <= 1.0 - EPS)
    qc = q.clamp(EPS, 1.0 - EPS)
    loss = -(y * torch.log(qc)).sum(dim=-1)
    g = torch.where(inr, -y / qc, torch.zeros_like(q))          # dL/dq
    gp = (g - (g * q).sum(-1, keepdim=True)) / s                 # dL/dp through normalisation
    dz = p * (gp - (p * gp).sum(-1, keepdim=True))               # softmax jacobian
    correct = (logits.argmax(-1) == y.argmax(-1)).to(torch.float32)
    return loss, dz, correct


def sigmoid_bce(z: torch.Tensor, y: torch.Tensor):
    """Keras binary_crossentropy on a sigmoid output: clip p to [eps, 1-eps], go back
    to logits, sigmoid-CE-with-logits.  z, y: [B] (or [B,1]).  Returns per-row
    (loss, dz, correct).

    z, y of shape [B, N] with N > 1 (a multi-label head): the loss is the mean over the columns
    of the per-element formula, dz [B, N] carries the 1/N, and correct is the row's COUNT of
    correct elements (binary_accuracy is its sum over rows * N)."""
    p = torch.sigmoid(z)
    inr = (p >= EPS) & (p <= 1.0 - EPS)
    pc = p.clamp(EPS, 1.0 - EPS)
    lg = torch.log(pc / (1.0 - pc))
    loss = torch.clamp(lg, min=0) - lg * y + torch.log1p(torch.exp(-lg.abs()))
    dz = torch.where(inr, pc - y, torch.zeros_like(p))
    correct = (torch.round(p) == y).to(torch.float32)   # round-half-even like TF
    if z.dim() == 2 and z.shape[1] > 1:
        return loss.mean(-1), dz / z.shape[1], correct.sum(-1)
    return loss, dz, correct


# The loss table (README, "Losses"): per-row loss l(p, y) [B] and g = dl/dp [B, N] of an output
# p = A(z) [B, N].  Keras 2.2.4 / TF subgradients: a maximum's tie gives the first argument the
# gradient, clips pass it on the closed interval, the FIRST row maximum takes the whole gradient.
def _first_argmax(v: torch.Tensor) -> torch.Tensor:
    mx = v.max(dim=-1, keepdim=True).values
    idx = torch.arange(v.shape[-1], device=v.device).expand_as(v)
    # (a row of NaNs has no maximum: index 0)
    return torch.where(v == mx, idx, torch.full_like(idx, v.shape[-1])).min(dim=-1).values % v.shape[-1]


def loss_mse(p, y):
    d = p - y
    return (d * d).mean(-1), 2.0 * d / p.shape[-1]


def loss_mae(p, y):
    d = p - y
    return d.abs().mean(-1), torch.sign(d) / p.shape[-1]


def loss_msle(p, y):
    pm, ym = p.clamp(min=EPS), y.clamp(min=EPS)
    d = torch.log(pm + 1.0) - torch.log(ym + 1.0)
    g = torch.where(p >= EPS, 2.0 * d / (pm + 1.0), torch.zeros_like(p))
    return (d * d).mean(-1), g / p.shape[-1]


def loss_logcosh(p, y):
    d = p - y
    ad = d.abs()
    return (ad + torch.log1p(torch.exp(-2.0 * ad)) - math.log(2.0)).mean(-1), torch.tanh(d) / p.shape[-1]


def loss_hinge(p, y):
    m = 1.0 - y * p
    return m.clamp(min=0).mean(-1), torch.where(m >= 0, -y, torch.zeros_like(p)) / p.shape[-1]


def loss_squared_hinge(p, y):
    h = (1.0 - y * p).clamp(min=0)
    return (h * h).mean(-1), -2.0 * y * h / p.shape[-1]


def loss_categorical_hinge(p, y):
    pos = (y * p).sum(-1)
    negs = (1.0 - y) * p
    neg = negs.max(dim=-1).values
    v = neg - pos + 1.0
    first = torch.nn.functional.one_hot(_first_argmax(negs), p.shape[-1]).to(p.dtype)
    g = torch.where((v > 0).unsqueeze(-1), -y + first * (1.0 - y), torch.zeros_like(p))
    return v.clamp(min=0), g


def loss_kld(p, y):
    yc, pc = y.clamp(EPS, 1.0), p.clamp(EPS, 1.0)
    g = torch.where((p >= EPS) & (p <= 1.0), -yc / pc, torch.zeros_like(p))
    return (yc * torch.log(yc / pc)).sum(-1), g


def loss_poisson(p, y):
    q = p + EPS
    return (p - y * torch.log(q)).mean(-1), (1.0 - y / q) / p.shape[-1]


TABLE_LOSSES = {"mse": loss_mse, "mae": loss_mae, "msle": loss_msle, "logcosh": loss_logcosh, "hinge": loss_hinge,
                "squared_hinge": loss_squared_hinge, "categorical_hinge": loss_categorical_hinge, "kld": loss_kld,
                "poisson": loss_poisson}


def head_probs(activation, z: torch.Tensor) -> torch.Tensor:
    if activation == "softmax":
        return torch.softmax(z, dim=-1)
    if activation == "sigmoid":
        return torch.sigmoid(z)
    return z


def table_loss(activation, loss: str, z: torch.Tensor, y: torch.Tensor):
    """A loss of the table on the output A(z), z and y [B, N].  Returns per-row
    (loss [B], dlogits [B, N] (not /B), correct [B]); correct is the row's count of correct
    elements under Keras' binary_accuracy (N == 1) and 0 / 1 under categorical_accuracy (first
    argmax of the output against first argmax of the targets)."""
    p = head_probs(activation, z)
    l, g = TABLE_LOSSES[loss](p, y)
    if activation == "sigmoid":
        dz = g * p * (1.0 - p)
    elif activation == "softmax":
        dz = p * (g - (p * g).sum(-1, keepdim=True))
    else:
        dz = g
    if z.shape[-1] == 1:
        correct = (torch.round(p) == y).to(torch.float32).sum(-1)
    else:
        correct = (_first_argmax(p) == _first_argmax(y)).to(torch.float32)
    return l, dz, correct


def mse(out: torch.Tensor, y: torch.Tensor):
    d = out - y
    loss = (d * d).mean(dim=-1)
    dz = 2.0 * d / out.shape[-1]
    return loss, dz, torch.zeros(out.shape[0], device=out.device)


def weight_factor(w: torch.Tensor) -> torch.Tensor:
    """Row factors of the sample-weighted loss (Keras 2.2 ``weighted_masked_objective``) for one
    batch of weights w [M]: w_i * (M / nnz), nnz = number of non-zero weights.  Scaling the
    per-row (loss, dlogits) by it gives rows that sum to M * L_batch with
    L_batch = sum(w l) / nnz -- the batch's contribution to Keras' epoch mean -- and, after the
    step's 1/M, the gradient of L_batch.  A batch of all-zero weights (0/0 in Keras) gives
    zero factors: the divisor is clamped to 1.  All-ones weights give exactly 1.0."""
    w = w.reshape(-1).to(torch.float32)
    nnz = max(int((w != 0).sum()), 1)
    scale = torch.tensor(float(w.shape[0]), dtype=torch.float32) / torch.tensor(float(nnz), dtype=torch.float32)
    return w * scale


def apply_weights(loss: torch.Tensor, dz: torch.Tensor, w: torch.Tensor):
    """(loss, dz) per row scaled by weight_factor(w); dz [M] or [M, N]."""
    f = weight_factor(w)
    return loss * f, dz * (f if dz.dim() == 1 else f.unsqueeze(-1))


# --------------------------------------------------------------------------- regularizers (Keras 2.2)
def regularization_penalty(ranges, master: torch.Tensor) -> torch.Tensor:
    """Keras 2.2.4 ``L1L2`` penalty of the flat fp32 weights: the sum over ``ranges``
    [(lo, hi, l1, l2)] of l1 * sum(|w|) + l2 * sum(w * w), as an fp32 scalar tensor."""
    total = torch.zeros((), dtype=torch.float32)
    for lo, hi, l1, l2 in ranges:
        w = master[lo:hi].to(torch.float32)
        total = total + (torch.tensor(l1, dtype=torch.float32) * w.abs()
                         + torch.tensor(l2, dtype=torch.float32) * (w * w)).sum()
    return total


def add_regularization_grad(ranges, master: torch.Tensor, g_flat: torch.Tensor) -> None:
    """g += l1 * sgn(w) + 2 * l2 * w over ``ranges`` [(lo, hi, l1, l2)], in place, in fp32 and in
    the HIP kernel's operation order g + (l1 * sgn(w) + (2 * l2) * w); sgn(0) = 0 (TensorFlow's
    gradient of abs).  Elements outside every range are untouched."""
    for lo, hi, l1, l2 in ranges:
        w = master[lo:hi]
        c1 = torch.tensor(l1, dtype=torch.float32)
        c2 = torch.tensor(l2, dtype=torch.float32) * 2.0
        g_flat[lo:hi] = g_flat[lo:hi] + (c1 * torch.sign(w) + c2 * w)


# --------------------------------------------------------------------------- optimizers (Keras 2.2)
def clip_gradients(g_flat: torch.Tensor, clipnorm=None, clipvalue=None):
    """Keras 2.2.4 ``Optimizer.get_gradients`` clipping of the flat fp32 gradient, in place.
    clipnorm = c > 0: with n the GLOBAL norm sqrt(sum g^2) over every parameter, g *= c / n when
    n >= c (the quotient formed first); n == 0 and a NaN norm fail the comparison and leave g
    unchanged.  clipvalue = v > 0: g = min(max(g, -v), v), applied after the norm clip.
    None or <= 0 means off.  Returns the norm (None without clipnorm)."""
    norm = None
    if clipnorm is not None and clipnorm > 0:
        norm = torch.sqrt((g_flat * g_flat).sum())
        if bool(norm >= clipnorm):
            g_flat.mul_(torch.tensor(clipnorm, dtype=g_flat.dtype) / norm)
    if clipvalue is not None and clipvalue > 0:
        g_flat.clamp_(-clipvalue, clipvalue)
    return norm


def adam_update(p, g, m, v, t: int, lr: float, beta_1=0.9, beta_2=0.999, eps=EPS):
    lr_t = lr * math.sqrt(1.0 - beta_2 ** t) / (1.0 - beta_1 ** t)
    m.mul_(beta_1).add_(g, alpha=1.0 - beta_1)
    v.mul_(beta_2).addcmul_(g, g, value=1.0 - beta_2)
    p.sub_(lr_t * m / (v.sqrt() + eps))


def amsgrad_update(p, g, m, v, vhat, t: int, lr: float, beta_1=0.9, beta_2=0.999, eps=EPS):
    lr_t = lr * math.sqrt(1.0 - beta_2 ** t) / (1.0 - beta_1 ** t)
    m.mul_(beta_1).add_(g, alpha=1.0 - beta_1)
    v.mul_(beta_2).addcmul_(g, g, value=1.0 - beta_2)
    torch.maximum(vhat, v, out=vhat)
    p.sub_(lr_t * m / (vhat.sqrt() + eps))


def adamax_update(p, g, m, u, t: int, lr: float, beta_1=0.9, beta_2=0.999, eps=EPS):
    lr_t = lr / (1.0 - beta_1 ** t)
    m.mul_(beta_1).add_(g, alpha=1.0 - beta_1)
    torch.maximum(u.mul_(beta_2), g.abs(), out=u)
    p.sub_(lr_t * m / (u + eps))


def adagrad_update(p, g, a, lr: float, eps=EPS):
    a.addcmul_(g, g)
    p.sub_(lr * g / (a.sqrt() + eps))


def adadelta_update(p, g, a, d, lr: float, rho=0.95, eps=EPS):
    a.mul_(rho).addcmul_(g, g, value=1.0 - rho)
    upd = g * torch.sqrt(d + eps) / torch.sqrt(a + eps)
    p.sub_(lr * upd)
    d.mul_(rho).addcmul_(upd, upd, value=1.0 - rho)


def nadam_schedule(t: int, m_schedule: float, beta_1=0.9, schedule_decay=0.004):
    mc_t = beta_1 * (1.0 - 0.5 * (0.96 ** (t * schedule_decay)))
    mc_t1 = beta_1 * (1.0 - 0.5 * (0.96 ** ((t + 1) * schedule_decay)))
    ms_new = m_schedule * mc_t
    ms_next = ms_new * mc_t1
    return mc_t, mc_t1, ms_new, ms_next


def nadam_update(p, g, m, v, t: int, lr: float, m_schedule: float, beta_1=0.9, beta_2=0.999,
                 eps=EPS, schedule_decay=0.004) -> float:
    """Returns the new m_schedule."""
    mc_t, mc_t1, ms_new, ms_next = nadam_schedule(t, m_schedule, beta_1, schedule_decay)
    g_prime = g / (1.0 - ms_new)
    m.mul_(beta_1).add_(g, alpha=1.0 - beta_1)
    v.mul_(beta_2).addcmul_(g, g, value=1.0 - beta_2)
    m_prime = m / (1.0 - ms_next)
    v_prime = v / (1.0 - beta_2 ** t)
    m_bar = (1.0 - mc_t) * g_prime + mc_t1 * m_prime
    p.sub_(lr * m_bar / (v_prime.sqrt() + eps))
    return ms_new


def sgd_update(p, g, mom, lr: float, momentum=0.0, nesterov=False):
    if momentum == 0.0:
        p.sub_(lr * g)
        return
    mom.mul_(momentum).sub_(lr * g)
    if nesterov:
        p.add_(momentum * mom - lr * g)
    else:
        p.add_(mom)


def rmsprop_update(p, g, a, lr: float, rho=0.9, eps=EPS):
    a.mul_(rho).addcmul_(g, g, value=1.0 - rho)
    p.sub_(lr * g / (a.sqrt() + eps))

"""float64 NumPy oracle of Keras 2.2.4 BatchNormalization (axis -1) as the fused stage computes it:

    dropout( maxpool( A( BN( z ) ) ) )

written from the definitions, not from the executors: per channel over the m rows of z,

    mean = sum z / m,  var = sum (z - mean)^2 / m,  xhat = (z - mean) / sqrt(var + eps),
    u = gamma xhat + beta
    moving_mean <- moving_mean mom + mean (1 - mom)
    moving_var  <- moving_var mom + var m / (m - (1 + eps)) (1 - mom)
    dbeta = sum du,  dgamma = sum du xhat,  dz = gamma / sqrt(var + eps) (du - dbeta / m - xhat dgamma / m)

du is the pooled gradient at each 2x2 window's FIRST maximum (row-major) and zero elsewhere,
including the last row / column an odd size leaves outside every window.  Channels are the last
axis; every function takes z of shape [..., C].
"""
import numpy as np


def batch_stats(z):
    z = np.asarray(z, np.float64)
    z2 = z.reshape(-1, z.shape[-1])
    m = z2.shape[0]
    mean = z2.sum(0) / m
    var = ((z2 - mean) ** 2).sum(0) / m
    return mean, var, m


def forward_train(z, gamma, beta, eps):
    """(u, xhat, mean, var, m) with the batch statistics."""
    z = np.asarray(z, np.float64)
    mean, var, m = batch_stats(z)
    xhat = (z - mean) / np.sqrt(var + eps)
    return np.asarray(gamma, np.float64) * xhat + np.asarray(beta, np.float64), xhat, mean, var, m


def forward_eval(z, gamma, beta, moving_mean, moving_var, eps):
    z = np.asarray(z, np.float64)
    return (np.asarray(gamma, np.float64) * (z - np.asarray(moving_mean, np.float64))
            / np.sqrt(np.asarray(moving_var, np.float64) + eps) + np.asarray(beta, np.float64))


def moving_update(moving_mean, moving_var, mean, var, m, momentum, eps):
    """Keras 2.2.4's update: the sample-variance factor m / (m - (1 + eps)), no Bessel factor on top."""
    mm = np.asarray(moving_mean, np.float64) * momentum + mean * (1.0 - momentum)
    mv = np.asarray(moving_var, np.float64) * momentum + var * (m / (m - (1.0 + eps))) * (1.0 - momentum)
    return mm, mv


def maxpool2x2(u):
    """(pooled [B, H//2, W//2, C], code uint8): code = dy * 2 + dx of the first maximum."""
    B, H, W, C = u.shape
    Hp, Wp = H // 2, W // 2
    win = np.stack([u[:, dy:2 * Hp:2, dx:2 * Wp:2, :] for dy in (0, 1) for dx in (0, 1)], axis=3)   # B,Hp,Wp,4,C
    code = win.argmax(axis=3)            # numpy's argmax returns the first maximum
    return np.take_along_axis(win, code[:, :, :, None, :], axis=3)[:, :, :, 0, :], code.astype(np.uint8)


def route(dp, code, hw):
    """du [B, H, W, C] from the pooled gradient and the codes."""
    B, Hp, Wp, C = dp.shape
    H, W = hw
    du = np.zeros((B, H, W, C), np.float64)
    for j in range(4):
        dy, dx = j >> 1, j & 1
        du[:, dy:2 * Hp:2, dx:2 * Wp:2, :] = np.where(code == j, dp, 0.0)
    return du


def backward(du, xhat, gamma, var, eps):
    """(dz, dgamma, dbeta) of the training-mode BN."""
    du = np.asarray(du, np.float64)
    C = du.shape[-1]
    m = du.size // C
    dbeta = du.reshape(-1, C).sum(0)
    dgamma = (du * xhat).reshape(-1, C).sum(0)
    dz = np.asarray(gamma, np.float64) / np.sqrt(var + eps) * (du - dbeta / m - xhat * dgamma / m)
    return dz, dgamma, dbeta


def stage_forward(z, gamma, beta, eps, relu=False, pool=False):
    """The stage output before dropout: (out, code or None, xhat, mean, var, m)."""
    u, xhat, mean, var, m = forward_train(z, gamma, beta, eps)
    r = np.maximum(u, 0.0) if relu else u
    code = None
    if pool:
        _, code = maxpool2x2(u)           # the argmax on u (relu is non-decreasing)
        r = np.take_along_axis(
            np.stack([r[:, dy:2 * (r.shape[1] // 2):2, dx:2 * (r.shape[2] // 2):2, :] for dy in (0, 1) for dx in (0, 1)],
                     axis=3), code[:, :, :, None, :].astype(np.int64), axis=3)[:, :, :, 0, :]
    return r, code, xhat, mean, var, m


def bf16_round(x):
    """Round-to-nearest-even to bfloat16, returned as float64."""
    import torch
    return torch.as_tensor(np.asarray(x, np.float32)).to(torch.bfloat16).to(torch.float64).numpy()


def bf16_ulp(x):
    """The spacing of bfloat16 at |x| (8 significand bits); the smallest normal's below it."""
    ax = np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(ax)) - 7)

"""float64 NumPy oracle of AveragePooling2D 2x2 / 2 / 'valid', GlobalAveragePooling2D and
GlobalMaxPooling2D on NHWC arrays, written from the formulas:

    avg2        out[b, i, j, c] = 0.25 * ((x[2i, 2j] + x[2i, 2j+1]) + (x[2i+1, 2j] + x[2i+1, 2j+1]))
                dx[b, y, x, c]  = 0.25 * dout[b, y // 2, x // 2, c], zero in a leftover odd row / column
    gavg        out[b, c] = sum_yx x[b, y, x, c] * inv_n,  dx[b, y, x, c] = dout[b, c] * inv_n
                inv_n = fp32(1 / (H * W))
    gmax        out[b, c] = max_yx x[b, y, x, c], idx[b, c] = the FIRST maximum's y * W + x (row-major)
                dx[b, y, x, c] = dout[b, c] at idx[b, c], zero elsewhere
    through     what a consumer's gradient g wrt a stage's OUTPUT becomes when it is stored through that
                stage: g * dropout mask * scale, zero where relu's saved output is not > 0
"""
import numpy as np


def inv_n(H, W):
    return float(np.float32(1.0 / (H * W)))


def avg2_fwd(x):
    x = np.asarray(x, np.float64)
    B, H, W, C = x.shape
    Hp, Wp = H // 2, W // 2
    out = np.zeros((B, Hp, Wp, C))
    for i in range(Hp):
        for j in range(Wp):
            out[:, i, j] = 0.25 * ((x[:, 2 * i, 2 * j] + x[:, 2 * i, 2 * j + 1])
                                   + (x[:, 2 * i + 1, 2 * j] + x[:, 2 * i + 1, 2 * j + 1]))
    return out


def avg2_bwd(dout, hw, lin=None):
    """``lin``: the un-pooled activation of a relu stage (the gradient is zero where it is not > 0)."""
    dout = np.asarray(dout, np.float64)
    B, Hp, Wp, C = dout.shape
    dx = np.zeros((B, hw[0], hw[1], C))
    for y in range(2 * Hp):
        for x in range(2 * Wp):
            dx[:, y, x] = 0.25 * dout[:, y // 2, x // 2]
    if lin is not None:
        dx = dx * (np.asarray(lin, np.float64) > 0)
    return dx


def gavg_fwd(x):
    x = np.asarray(x, np.float64)
    B, H, W, C = x.shape
    return x.reshape(B, H * W, C).sum(1) * inv_n(H, W)


def gavg_bwd(dout, hw):
    dout = np.asarray(dout, np.float64)
    H, W = hw
    return np.broadcast_to((dout * inv_n(H, W))[:, None, None, :], (dout.shape[0], H, W, dout.shape[1])).copy()


def gmax_fwd(x):
    """(max, idx): idx the smallest flat position holding the maximum."""
    x = np.asarray(x, np.float64)
    B, H, W, C = x.shape
    xf = x.reshape(B, H * W, C)
    best = xf[:, 0].copy()
    idx = np.zeros((B, C), np.int64)
    for p in range(1, H * W):
        gt = xf[:, p] > best                 # strict: an equal later value does not take the index
        best = np.where(gt, xf[:, p], best)
        idx = np.where(gt, p, idx)
    return best, idx


def gmax_bwd(dout, idx, hw):
    dout = np.asarray(dout, np.float64)
    H, W = hw
    B, C = dout.shape
    dx = np.zeros((B, H * W, C))
    for b in range(B):
        for c in range(C):
            dx[b, idx[b, c], c] = dout[b, c]
    return dx.reshape(B, H, W, C)


def through(g, keep=None, scale=1.0, relu_out=None):
    """The gradient g wrt a stage's output as stored through that stage's backward: times its dropout
    mask and scale, zero where the stage is relu and its saved output is not > 0."""
    g = np.asarray(g, np.float64)
    if keep is not None:
        g = np.where(keep, g * scale, 0.0)
    if relu_out is not None:
        g = np.where(np.asarray(relu_out, np.float64) > 0, g, 0.0)
    return g

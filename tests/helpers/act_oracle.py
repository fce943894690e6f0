"""float64 NumPy oracle of the hidden activations (Keras 2.2.4 formulas) and bf16 helpers.

    name           A(x)                                A' from the output y
    tanh           tanh(x)                             max(0, 1 - y^2)
    sigmoid        1 / (1 + e^-x)                      max(0, y (1 - y))
    hard_sigmoid   clip(0.2 x + 0.5, 0, 1)             0.2 if 0 < y < 1 else 0
    elu            x > 0 ? x : alpha (e^x - 1)         y > 0 ? 1 : max(0, y + alpha)
    selu           s elu(x, a)                         y > 0 ? s : max(0, y + s a)
    softplus       max(x, 0) + log1p(e^-|x|)           max(0, -expm1(-y))
    softsign       x / (1 + |x|)                       (1 - min(|y|, 1))^2
    leaky_relu     x > 0 ? x : alpha x                 y > 0 ? 1 : alpha

At +-inf the functions take their limits (softsign +-1; leaky_relu with alpha = 0 is relu: 0 at
-inf); NaN gives NaN."""
import numpy as np
import torch

SELU_S, SELU_A = 1.0507009873554805, 1.6732632423543772
STRINGS = ("tanh", "sigmoid", "hard_sigmoid", "elu", "selu", "softplus", "softsign")
# (name, alpha) of every case the GPU tests run: the seven strings, LeakyReLU and ELU layers
CASES = [(n, 1.0 if n == "elu" else 0.0) for n in STRINGS] + [
    ("leaky_relu", 0.0), ("leaky_relu", float(np.float32(0.3))), ("leaky_relu", float(np.float32(1.7))),
    ("elu", 0.5)]


def act(name, alpha, x):
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        if name == "tanh":
            return np.tanh(x)
        if name == "sigmoid":
            return 1.0 / (1.0 + np.exp(-x))
        if name == "hard_sigmoid":
            v = 0.2 * x + 0.5
            return np.where(v < 0, 0.0, np.where(v > 1, 1.0, v))
        if name == "elu":
            return np.where(x > 0, x, alpha * np.expm1(x))
        if name == "selu":
            return SELU_S * np.where(x > 0, x, SELU_A * np.expm1(x))
        if name == "softplus":
            return np.where(x > 0, x, np.where(x < 0, 0.0, x)) + np.log1p(np.exp(-np.abs(x)))
        if name == "softsign":
            return np.where(np.isinf(x), np.sign(x), x / (1.0 + np.abs(x)))
        if name == "leaky_relu":
            return np.where(x > 0, x, np.where((x < 0) & (alpha == 0), 0.0, alpha * x))
    raise ValueError(name)


def act_grad_from_output(name, alpha, y):
    y = np.asarray(y, np.float64)
    with np.errstate(all="ignore"):
        if name == "tanh":
            return np.maximum(0.0, 1.0 - y * y)
        if name == "sigmoid":
            return np.maximum(0.0, y * (1.0 - y))
        if name == "hard_sigmoid":
            return np.where((y > 0) & (y < 1), 0.2, 0.0)
        if name == "elu":
            return np.where(y > 0, 1.0, np.maximum(0.0, y + alpha))
        if name == "selu":
            return np.where(y > 0, SELU_S, np.maximum(0.0, y + SELU_S * SELU_A))
        if name == "softplus":
            return np.maximum(0.0, -np.expm1(-y))
        if name == "softsign":
            return (1.0 - np.minimum(np.abs(y), 1.0)) ** 2
        if name == "leaky_relu":
            return np.where(y > 0, 1.0, alpha)
    raise ValueError(name)


def out_range(name, alpha):
    """[lo, hi] of the function's values (closed: bf16 rounding reaches the limits)."""
    return {"tanh": (-1.0, 1.0), "sigmoid": (0.0, 1.0), "hard_sigmoid": (0.0, 1.0), "elu": (-alpha, np.inf),
            "selu": (-SELU_S * SELU_A, np.inf), "softplus": (0.0, np.inf), "softsign": (-1.0, 1.0),
            "leaky_relu": (-np.inf if alpha > 0 else 0.0, np.inf)}[name]


# ------------------------------------------------------------------------------------ bf16
def all_bf16():
    """Every bf16 bit pattern, as (bits int32 [65536], values float32 [65536])."""
    bits = np.arange(65536, dtype=np.int64)
    vals = (bits << 16).astype(np.uint32).view(np.float32)
    return bits.astype(np.int32), vals


def bits_of(t):
    """bf16 tensor -> int32 NumPy array of its bit patterns."""
    return t.detach().cpu().contiguous().view(torch.int16).numpy().astype(np.int32) & 0xFFFF


def to_bf16_bits(v64):
    """float64 array -> bits of the nearest bf16."""
    t = torch.as_tensor(np.asarray(v64, np.float64)).to(torch.float32).to(torch.bfloat16)
    return bits_of(t)


def bf16_values(bits):
    return ((np.asarray(bits, np.int64) & 0xFFFF) << 16).astype(np.uint32).view(np.float32)


def ordinal(bits):
    """Monotone integer of a bf16 bit pattern (+0 and -0 both 0): ulp distance = |difference|."""
    b = np.asarray(bits, np.int64) & 0xFFFF
    return np.where(b & 0x8000, -(b & 0x7FFF), b)


def is_nan_bits(bits):
    b = np.asarray(bits, np.int64) & 0x7FFF
    return b > 0x7F80

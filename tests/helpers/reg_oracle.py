"""Float64 NumPy oracle of the Keras 2.2.4 L1 / L2 weight regularizers (``keras/regularizers.py``
``L1L2.__call__``: ``sum(l1 * |w|) + sum(l2 * w^2)``), written from the formulas only.

``ranges`` is what ``Model.regularized_ranges()`` returns: [(lo, hi, l1, l2)] over the flat
parameter vector.  The coefficients are taken as given (float32-rounded by the model, as Keras
casts them to floatx)."""
import numpy as np


def penalty(ranges, w):
    """P = sum over ranges of l1 * sum(|w|) + l2 * sum(w * w), in float64."""
    w = np.asarray(w, dtype=np.float64)
    return float(sum(l1 * np.abs(w[lo:hi]).sum() + l2 * np.square(w[lo:hi]).sum() for lo, hi, l1, l2 in ranges))


def grad_term(ranges, w):
    """d P / d w: l1 * sgn(w) + 2 * l2 * w inside the ranges (sgn(0) = 0, TensorFlow's gradient of
    abs), zero elsewhere; float64."""
    w = np.asarray(w, dtype=np.float64)
    out = np.zeros_like(w)
    for lo, hi, l1, l2 in ranges:
        seg = w[lo:hi]
        out[lo:hi] = l1 * ((seg > 0).astype(np.float64) - (seg < 0).astype(np.float64)) + 2.0 * l2 * seg
    return out


def add_grad(ranges, w, g):
    """The gradient the update sees: g + d P / d w (added before any clipping); float64."""
    return np.asarray(g, dtype=np.float64) + grad_term(ranges, w)


def batch_loss(data_loss, ranges, w):
    """What a train / test batch reports: L_data + P (the penalty is not sample-weighted)."""
    return float(data_loss) + penalty(ranges, w)


def epoch_loss(batches):
    """Keras' epoch loss sum_b(M_b * loss_b) / N over [(rows M_b, data loss, penalty P_b)]: a batch
    of M_b rows contributes M_b * (L_b + P_b)."""
    n = sum(m for m, _, _ in batches)
    return float(sum(m * (l + p) for m, l, p in batches) / n)


def grad_f32(ranges, w, g):
    """The HIP kernel's gradient arithmetic in NumPy float32, bit for bit: inside a range
    g + (l1 * sgn(w) + (2 * l2) * w), every operation rounded to float32 in that order; outside
    the ranges g is returned as it is."""
    w = np.asarray(w, dtype=np.float32)
    out = np.array(g, dtype=np.float32, copy=True)
    for lo, hi, l1, l2 in ranges:
        seg = w[lo:hi]
        c1, c2 = np.float32(l1), np.float32(l2) * np.float32(2.0)
        sg = (seg > 0).astype(np.float32) - (seg < 0).astype(np.float32)
        out[lo:hi] = out[lo:hi] + (c1 * sg + c2 * seg)
    return out

"""Independent float64 oracle of the ROC metrics (cori_intml_examples_amd/metrics.py, csrc/kernels/roc.hip):
the exact AUC by sorting with ties counted half (sklearn's ``roc_auc_score(sample_weight=)``), the
confusion sums at a threshold, and the per-input bound of the histogram AUC against the exact one."""
import numpy as np


def _w(n, w):
    return np.ones(n, np.float64) if w is None else np.asarray(w, np.float64).reshape(-1)


def exact_auc(labels, scores, w=None):
    """The weighted Mann-Whitney statistic: sum over (positive, negative) pairs of w_p * w_n * [s_p > s_n] +
    0.5 * [s_p == s_n], over P * N.  NaN when a class has zero weight."""
    s = np.asarray(scores, np.float64).reshape(-1)
    pos = np.asarray(labels).reshape(-1) > 0.5
    w = _w(len(s), w)
    order = np.argsort(s, kind="stable")
    s, pos, w = s[order], pos[order], w[order]
    wp, wn = np.where(pos, w, 0.0), np.where(pos, 0.0, w)
    P, N = wp.sum(), wn.sum()
    if not (P > 0 and N > 0):
        return float("nan")
    # groups of equal scores, ascending: a negative group gains the positives strictly above it
    # and half of those tied with it
    starts = np.concatenate([[0], np.nonzero(np.diff(s))[0] + 1])
    gp, gn = np.add.reduceat(wp, starts), np.add.reduceat(wn, starts)
    above = P - np.cumsum(gp)
    return float((gn * (above + 0.5 * gp)).sum() / (P * N))


def confusion(labels, scores, w=None, threshold=0.5):
    """(TP, FP, TN, FN) sums with pred = score > threshold, label positive iff > 0.5."""
    s = np.asarray(scores, np.float32).reshape(-1)
    pos = np.asarray(labels).reshape(-1) > 0.5
    w = _w(len(s), w)
    pred = s > np.float32(threshold)
    return (float(w[pos & pred].sum()), float(w[~pos & pred].sum()), float(w[~pos & ~pred].sum()),
            float(w[pos & ~pred].sum()))


def summary(labels, scores, w=None):
    """{'acc', 'purity', 'efficiency'} at threshold 0.5 (a zero denominator gives 0.0)."""
    tp, fp, tn, fn = confusion(labels, scores, w)
    r = lambda a, b: a / b if b else 0.0
    return {"acc": r(tp + tn, tp + fp + tn + fn), "purity": r(tp, tp + fp), "efficiency": r(tp, tp + fn)}


def hist_bound(labels, scores, keys, w=None):
    """B = 0.5 * (sum_b P_b N_b - sum_u P_u N_u) / (P * N) over the bins b that ``keys`` assigns and the
    distinct scores u: the histogram AUC counts every cross-class pair that shares a bin 0.5 where the
    exact one counts 0, 0.5 or 1 -- and 0.5 as well when the two scores are equal, so tied pairs cost
    nothing (a fully saturated set has B == 0)."""
    pos = np.asarray(labels).reshape(-1) > 0.5
    w = _w(len(pos), w)
    keys = np.asarray(keys).reshape(-1)

    def cross(groups):
        nb = int(groups.max()) + 1
        return (np.bincount(groups[pos], weights=w[pos], minlength=nb)
                * np.bincount(groups[~pos], weights=w[~pos], minlength=nb)).sum()

    P, N = w[pos].sum(), w[~pos].sum()
    if not (P > 0 and N > 0):
        return float("nan")
    uniq = np.unique(np.asarray(scores, np.float32).reshape(-1), return_inverse=True)[1].reshape(-1)
    return float(0.5 * max(cross(keys) - cross(uniq), 0.0) / (P * N))


def synthetic(kind, n, seed=0):
    """(labels, fp32 scores) of the synthetic score sets: 'weak' / 'strong' separation, 'rpv' (a trained
    classifier's bimodal sigmoid outputs, 30% signal) and 'saturated' (everything exactly 0 or 1)."""
    rs = np.random.RandomState(seed)
    y = (rs.rand(n) < 0.3).astype(np.float32)
    if kind == "weak":
        z = 2.0 * rs.randn(n) + 0.5 * y
    elif kind == "strong":
        z = rs.randn(n) + 3.0 * (2 * y - 1)
    elif kind == "rpv":
        z = rs.randn(n) * 2.5 + 5.0 * (2 * y - 1)
    elif kind == "saturated":
        flip = rs.rand(n) < 0.1
        return y, np.where(flip, 1 - y, y).astype(np.float32)
    else:
        raise ValueError(kind)
    return y, (1.0 / (1.0 + np.exp(-z))).astype(np.float32)

"""ROC curve, AUC, purity, efficiency and their sample-weighted twins from a score histogram.

The statistics the RPV notebooks end with (``summarize_metrics``, ``draw_roc``), computed from
64-bit integer sums so that they are order-independent and bit-identical from run to run:

* ``score_bin(s)``: the key of an fp32 score in [0, 1].  With ``H = 0x3F00``: ``bits(s) >> 16`` for
  ``s < 0.5``, ``2H - (bits(1 - s) >> 16)`` otherwise (``1 - s`` is exact in fp32 on [0.5, 1]).  The key is
  non-decreasing in ``s`` and resolves 128 bins per octave towards both 0 and 1.  NaN, negative and
  ``> 1`` scores are not binned but counted as invalid; a pass with an invalid score reads NaN.
* per (set, class): ``pos[ROC_BINS]`` / ``neg[ROC_BINS]``, the exact confusion sums at threshold 0.5
  (``pred = s > 0.5``) and, for a softmax head, ``sum(w * correct)`` / ``sum(w)``.  Set 0 holds exact
  counts, set 1 the weights as ``llrint(w * 2^k)`` with ``sum(w) * 2^k <= 2^61``.
* the AUC is the weighted Mann-Whitney statistic with ties counted half, evaluated on the bins
  (all pairs that share a bin count half).

On a GPU the sums come from the ``roc_accum`` / ``roc_finish`` HIP kernels (csrc/kernels/roc.hip); ``RocState``
here is their numpy twin, which forms the same integers.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

ROC_SHIFT = 16
ROC_H = 0x3F00
ROC_BINS = 2 * ROC_H + 1
ROC_HDR = 8
ROC_TAIL = 8
T_TP, T_FP, T_TN, T_FN, T_WC, T_WS, T_INVALID = range(7)
ROC_BLOCK = 2 * ROC_BINS + ROC_TAIL
ROC_RES_WORDS = 16
MAX_CLASSES = 16

# canonical metric names and their aliases (Model.compile)
CANONICAL = {"accuracy": "acc", "acc": "acc", "auc": "auc", "purity": "purity", "precision": "purity",
             "efficiency": "efficiency", "recall": "efficiency"}
ROC_FAMILY = ("auc", "purity", "efficiency")


def canonical_metric(name) -> str:
    """'acc' / 'auc' / 'purity' / 'efficiency' for a metric name or alias; NotImplementedError otherwise."""
    c = CANONICAL.get(name) if isinstance(name, str) else None
    if c is None:
        raise NotImplementedError("metric %r" % (name,))
    return c


def larger_is_better(name: str) -> bool:
    """True for a logged name (with or without ``val_`` / ``weighted_``) of acc or the ROC family."""
    return any(k in name for k in ("acc",) + ROC_FAMILY)


# ------------------------------------------------------------------------------ the key
def score_valid(scores) -> np.ndarray:
    s = np.asarray(scores, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return (s >= 0) & (s <= 1)


def score_bin(scores) -> np.ndarray:
    """int32 key of every fp32 score; -1 for an invalid one (NaN, negative, > 1)."""
    s = np.ascontiguousarray(scores, dtype=np.float32)
    ok = score_valid(s)
    z = np.where(ok, s, np.float32(0))
    low = (z.view(np.uint32) & np.uint32(0x7FFFFFFF)) >> np.uint32(ROC_SHIFT)
    t = (np.float32(1.0) - z).astype(np.float32)
    high = 2 * ROC_H - (t.view(np.uint32) >> np.uint32(ROC_SHIFT)).astype(np.int64)
    key = np.where(z < np.float32(0.5), low.astype(np.int64), high)
    return np.where(ok, key, -1).astype(np.int32)


def bin_lower_edge(idx) -> np.ndarray:
    """The smallest fp32 score whose key is ``idx`` (or, for a bin no fp32 score reaches, larger: the
    scores in [0.5, 1] lie on a grid of 2^-24, so towards 1 most of the upper half's bins are empty).
    Lower half: bits ``idx << 16``.  Upper half: ``1 - t`` with ``t`` the largest multiple of 2^-24 not above
    ``t_max``, whose bits are ``((2H - idx) << 16) | 0xFFFF`` (and not above 0.5); exact, key 2H being 1.0."""
    i = np.asarray(idx, dtype=np.int64)
    if np.any((i < 0) | (i >= ROC_BINS)):
        raise ValueError("bin index outside [0, %d)" % ROC_BINS)
    low = (np.minimum(i, ROC_H) << ROC_SHIFT).astype(np.uint32).view(np.float32)
    tb = ((np.clip(2 * ROC_H - i, 0, ROC_H) << ROC_SHIFT) | 0xFFFF).astype(np.uint32)
    t = np.minimum(np.floor(tb.view(np.float32).astype(np.float64) * 2.0 ** 24) / 2.0 ** 24, 0.5)
    return np.where(i < ROC_H, low, (1.0 - t).astype(np.float32)).astype(np.float32)


# ------------------------------------------------------------------------------ weights
BAD_WEIGHTS = "sample weights must be finite and non-negative for the weighted metrics"


def check_weights(w) -> None:
    """ValueError for negative or non-finite sample weights (the weighted metrics' fixed point)."""
    w = np.asarray(w)
    if w.size and (not np.all(np.isfinite(w)) or np.any(w < 0)):
        raise ValueError(BAD_WEIGHTS)


def weight_shift(total: float) -> int:
    """k with ``total * 2^k <= 2^61`` (``total`` = the data set's sum of weights, in float64)."""
    if not (total > 0) or not math.isfinite(total):
        return 0
    _, e = math.frexp(total)          # total = m * 2^e, 0.5 <= m < 1: total <= 2^e
    return max(-1000, min(61 - e, 1000))


def fixed_weights(w, k: int) -> np.ndarray:
    """llrint(float64(w) * 2^k) as int64 (round half to even, like the kernel)."""
    return np.rint(np.ldexp(np.asarray(w, dtype=np.float32).astype(np.float64), k)).astype(np.int64)


# ------------------------------------------------------------------------------ the numpy twin
def first_argmax(a: np.ndarray) -> np.ndarray:
    """The kernels' first-maximum rule (strict '>' from column 0) over the rows of ``a``: a NaN is
    never chosen, unless it sits in column 0, which then nothing beats."""
    a = np.asarray(a, dtype=np.float32)
    b = np.where(np.isnan(a), -np.inf, a)
    b[:, 0] = np.where(np.isnan(a[:, 0]), np.inf, b[:, 0])
    return b.argmax(axis=1)


class RocState:
    """The ROC state of ``n_classes`` columns as the kernels keep it: ``pos`` / ``neg`` [2][N][ROC_BINS] and
    ``tail`` [2][N][ROC_TAIL] int64, set 0 unweighted, set 1 weighted with shift ``k``."""

    def __init__(self, n_classes: int, softmax: bool, k: int = 0):
        if not 1 <= n_classes <= MAX_CLASSES:
            raise ValueError("n_classes must be 1..%d" % MAX_CLASSES)
        self.N, self.softmax, self.k = int(n_classes), bool(softmax), int(k)
        self.pos = np.zeros((2, self.N, ROC_BINS), np.int64)
        self.neg = np.zeros((2, self.N, ROC_BINS), np.int64)
        self.tail = np.zeros((2, self.N, ROC_TAIL), np.int64)

    def reset(self):
        for a in (self.pos, self.neg, self.tail):
            a.fill(0)

    def accumulate(self, probs, y, w=None):
        """One batch: probs [M][N] fp32, targets y [M][N], weights w [M] or None (set 0 only)."""
        p = np.ascontiguousarray(probs, dtype=np.float32).reshape(-1, self.N)
        y = np.asarray(y, dtype=np.float32).reshape(-1, self.N)
        M = p.shape[0]
        if self.softmax:
            ay, am = first_argmax(y), first_argmax(p)
            posm = ay[:, None] == np.arange(self.N)[None, :]
            correct = (ay == am).astype(np.int64)
        else:
            posm = y > np.float32(0.5)
        key = score_bin(p.reshape(-1)).reshape(M, self.N)
        pred = p > np.float32(0.5)
        sets = [(0, np.ones(M, np.int64))]
        if w is not None:
            sets.append((1, fixed_weights(np.asarray(w).reshape(-1), self.k)))
        for s, q in sets:
            for n in range(self.N):
                ok = key[:, n] >= 0
                ps, kk, pr = posm[:, n], key[:, n], pred[:, n]
                np.add.at(self.pos[s, n], kk[ok & ps], q[ok & ps])
                np.add.at(self.neg[s, n], kk[ok & ~ps], q[ok & ~ps])
                t = self.tail[s, n]
                t[T_TP] += q[ok & ps & pr].sum()
                t[T_FP] += q[ok & ~ps & pr].sum()
                t[T_TN] += q[ok & ~ps & ~pr].sum()
                t[T_FN] += q[ok & ps & ~pr].sum()
                t[T_INVALID] += int(np.count_nonzero(~ok & (q > 0)))
            if self.softmax:
                self.tail[s, 0, T_WC] += (q * correct).sum()
                self.tail[s, 0, T_WS] += q.sum()


def hist_auc(pos: np.ndarray, neg: np.ndarray) -> float:
    """sum_b neg[b] * (2 * pos_above[b] + pos[b]) / (2 P N) in exact integer arithmetic, one rounding at
    the division; NaN when a class is empty."""
    pos = np.asarray(pos, dtype=np.int64)
    neg = np.asarray(neg, dtype=np.int64)
    nz = np.nonzero(neg)[0]
    P, N = int(pos.sum()), int(neg.sum())
    if P <= 0 or N <= 0:
        return float("nan")
    above = (P - np.cumsum(pos))[nz]           # positives strictly above each bin
    num = sum(int(n) * (2 * int(a) + int(p)) for n, a, p in zip(neg[nz].tolist(), above.tolist(), pos[nz].tolist()))
    return num / (2 * P * N)


def _ratio(a: int, b: int) -> float:
    return a / b if b else 0.0


def scalar_metrics(softmax: bool, aucs: Sequence[float], tails: np.ndarray) -> Dict[str, float]:
    """{'acc', 'auc', 'purity', 'efficiency'} of one set from its classes' AUCs and tails [N][ROC_TAIL]
    (purity / efficiency for a sigmoid head only).  Everything is NaN when a score was invalid."""
    tails = np.asarray(tails, dtype=np.int64)
    names = ("acc", "auc") if softmax else ("acc", "auc", "purity", "efficiency")
    if int(tails[:, T_INVALID].sum()) > 0:
        return {n: float("nan") for n in names}
    if softmax:
        ok = [a for a in aucs if not math.isnan(a)]
        return {"acc": _ratio(int(tails[0, T_WC]), int(tails[0, T_WS])),
                "auc": sum(ok) / len(ok) if ok else float("nan")}
    tp, fp, tn, fn = (int(v) for v in tails[0, :4])
    return {"acc": _ratio(tp + tn, tp + fp + tn + fn), "auc": aucs[0],
            "purity": _ratio(tp, tp + fp), "efficiency": _ratio(tp, tp + fn)}


def named_metrics(softmax: bool, aucs, tails, weighted_seen: bool) -> Dict[str, float]:
    """Every metric name of a pass from the per-(set, class) AUCs [2][N] and tails [2][N][ROC_TAIL]: the
    unweighted set's under their canonical names, the weighted set's as 'weighted_' + name.  A pass
    over data without weights (``weighted_seen`` False) reads its weighted twins from set 0."""
    out = {}
    for si, prefix in ((0, ""), (1, "weighted_")):
        use = si if weighted_seen else 0
        for name, v in scalar_metrics(softmax, list(aucs[use]), tails[use]).items():
            out[prefix + name] = v
    return out


# ------------------------------------------------------------------------------ the curve
@dataclass
class RocResult:
    fpr: np.ndarray
    tpr: np.ndarray
    thresholds: np.ndarray
    auc: float
    accuracy: float
    purity: float
    efficiency: float
    confusion: Tuple[float, float, float, float]     # (TP, FP, TN, FN) sums (of weights, if given)
    n_invalid: int


def result_from_state(pos, neg, tail, k: int = 0, auc: Optional[float] = None) -> RocResult:
    """The curve of one (set, class) from its integers: one point per non-empty bin from the top,
    starting at (0, 0) with threshold inf."""
    pos = np.asarray(pos, dtype=np.int64)
    neg = np.asarray(neg, dtype=np.int64)
    tail = np.asarray(tail, dtype=np.int64)
    n_invalid = int(tail[T_INVALID])
    nan = float("nan")
    P, N = int(pos.sum()), int(neg.sum())
    idx = np.nonzero(pos + neg)[0][::-1]
    with np.errstate(invalid="ignore", divide="ignore"):
        tpr = np.concatenate([[0.0], np.cumsum(pos[idx]).astype(np.float64) / P]) if P else np.full(len(idx) + 1, nan)
        fpr = np.concatenate([[0.0], np.cumsum(neg[idx]).astype(np.float64) / N]) if N else np.full(len(idx) + 1, nan)
    thr = np.concatenate([[np.inf], bin_lower_edge(idx).astype(np.float64)])
    tp, fp, tn, fn = (int(v) for v in tail[:4])
    scale = math.ldexp(1.0, -k)
    conf = tuple(v * scale for v in (tp, fp, tn, fn))
    if n_invalid:
        return RocResult(fpr, tpr, thr, nan, nan, nan, nan, conf, n_invalid)
    if auc is None:
        auc = hist_auc(pos, neg)
    return RocResult(fpr, tpr, thr, auc, _ratio(tp + tn, tp + fp + tn + fn), _ratio(tp, tp + fp),
                     _ratio(tp, tp + fn), conf, 0)


def _gpu_kernels():
    """The HIP kernel module when a GPU is present, else None."""
    import torch
    if not torch.cuda.is_available():
        return None
    from .ops.hip import kernels
    return kernels()


def _is_cuda_tensor(a) -> bool:
    return type(a).__module__.startswith("torch") and getattr(a, "is_cuda", False)


def _binary_state_gpu(K, labels, scores, w):
    """(pos, neg, tail, k, auc) of the set the call asks for, from roc_accum / roc_finish."""
    import torch
    dev = scores.device if _is_cuda_tensor(scores) else torch.device("cuda", torch.cuda.current_device())
    f32 = lambda a: torch.as_tensor(a).to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
    with torch.cuda.device(dev):
        p, y = f32(scores), f32(labels)
        if p.numel() != y.numel():
            raise ValueError("labels and scores differ in length")
        wt, k = None, 0
        if w is not None:
            wt = f32(w)
            if wt.numel() != p.numel():
                raise ValueError("sample_weight and scores differ in length")
            if wt.numel() and (not bool(torch.isfinite(wt).all()) or bool((wt < 0).any())):
                raise ValueError(BAD_WEIGHTS)
            k = weight_shift(float(wt.double().sum()))
        state = torch.zeros(ROC_HDR + 2 * ROC_BLOCK, dtype=torch.int64, device=dev)
        state[0] = k
        state[1:2].view(torch.float64)[0] = math.ldexp(1.0, k)
        res = torch.zeros(2 * ROC_RES_WORDS, dtype=torch.int64, device=dev)
        a = K.RocArgs()
        a.probs, a.y, a.M, a.N, a.softmax = p.data_ptr(), y.data_ptr(), p.numel(), 1, 0
        a.state, a.res = state.data_ptr(), res.data_ptr()
        if wt is not None:
            a.wb, a.weighted = wt.data_ptr(), 1
        s = torch.cuda.current_stream().cuda_stream
        if p.numel():
            K.roc_accum(a, s)
        K.roc_finish(a, s)
        st = state.cpu().numpy()
        r = res.cpu().numpy()
    si = 1 if w is not None else 0
    blk = st[ROC_HDR + si * ROC_BLOCK:ROC_HDR + (si + 1) * ROC_BLOCK]
    auc = float(r[si * ROC_RES_WORDS:si * ROC_RES_WORDS + 1].view(np.float64)[0])
    return blk[:ROC_BINS], blk[ROC_BINS:2 * ROC_BINS], blk[2 * ROC_BINS:], k, auc


def roc_curve(labels, scores, sample_weight=None) -> RocResult:
    """The ROC curve and threshold-0.5 statistics of binary ``labels`` (positive iff > 0.5) against fp32
    ``scores``.  CUDA tensors, or numpy arrays when a GPU is present, run the HIP kernels; otherwise
    the numpy twin forms the same integers."""
    K = _gpu_kernels()
    if K is not None:
        pos, neg, tail, k, auc = _binary_state_gpu(K, labels, scores, sample_weight)
        return result_from_state(pos, neg, tail, k, auc)
    to_np = lambda a: a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    p = to_np(scores).astype(np.float32).reshape(-1)
    y = to_np(labels).astype(np.float32).reshape(-1)
    if p.shape != y.shape:
        raise ValueError("labels and scores differ in length")
    w, k = None, 0
    if sample_weight is not None:
        w = to_np(sample_weight).astype(np.float32).reshape(-1)
        if w.shape != p.shape:
            raise ValueError("sample_weight and scores differ in length")
        check_weights(w)
        k = weight_shift(float(w.astype(np.float64).sum()))
    st = RocState(1, False, k)
    st.accumulate(p.reshape(-1, 1), y.reshape(-1, 1), w)
    si = 1 if w is not None else 0
    return result_from_state(st.pos[si, 0], st.neg[si, 0], st.tail[si, 0], k)


def roc_auc_score(labels, scores, sample_weight=None) -> float:
    return roc_curve(labels, scores, sample_weight).auc


def per_class_curves(y, probs, sample_weight=None) -> List[RocResult]:
    """One-vs-rest curves of a softmax output: class n positive iff n is the first argmax of the target row."""
    y = np.asarray(y, dtype=np.float32)
    probs = np.asarray(probs, dtype=np.float32)
    ay = first_argmax(y)
    return [roc_curve((ay == n).astype(np.float32), probs[:, n], sample_weight) for n in range(probs.shape[1])]

"""Time of the stand-alone ROC curve (``metrics.roc_curve``) on one GPU.

    python benchmarks/roc_metrics.py [--n 1048576] [--calls 20] [--warmup 5]

``n`` fp32 scores resident on the device, once all equal to 1.0 (every row of every wave lands in ONE
histogram word and ONE confusion word per class: the case the wave-level combination in
``roc_accum_kernel`` is there to bound) and once uniform in (0, 1) (nearly every lane of a wave in a
bin of its own).  Each figure is the median of ``calls`` timed calls after ``warmup`` untimed ones.
Two times per case: ``kernels_us``, the ``roc_accum`` + ``roc_finish`` launches between two device
events, and ``call_us``, the whole ``roc_curve`` call on the host clock (state allocation, the launches,
the download of the histograms and the curve built from the integers).  Prints one JSON line."""
import argparse
import json
import math
import os
import statistics
import sys
import time


sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from cori_intml_examples_amd import metrics as MT  # noqa: E402
from cori_intml_examples_amd.ops.hip import kernels  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    K = kernels()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(0)
    labels = (torch.rand(a.n, generator=g) < 0.3).float().to(dev)
    weights = (torch.rand(a.n, generator=g) + 0.5).to(dev)
    cases = {"all_ones": torch.ones(a.n, device=dev),
             "uniform": torch.rand(a.n, generator=g).clamp_(1e-7, 1 - 1e-7).to(dev)}
    state = torch.zeros(K.ROC_HDR + 2 * K.ROC_BLOCK, dtype=torch.int64, device=dev)
    res = torch.zeros(2 * K.ROC_RES_WORDS, dtype=torch.int64, device=dev)
    k = MT.weight_shift(float(weights.double().sum()))
    state[0] = k
    state[1:2].view(torch.float64)[0] = math.ldexp(1.0, k)
    stream = torch.cuda.current_stream().cuda_stream
    out = {"n": a.n, "calls": a.calls, "warmup": a.warmup, "cases": {}}
    for name, scores in cases.items():
        rec = {}
        for label, w in (("unweighted", None), ("weighted", weights)):
            args = K.RocArgs()
            args.probs, args.y, args.M, args.N = scores.data_ptr(), labels.data_ptr(), a.n, 1
            args.state, args.res = state.data_ptr(), res.data_ptr()
            if w is not None:
                args.wb, args.weighted = w.data_ptr(), 1
            kt, ct = [], []
            for i in range(a.warmup + a.calls):
                state[K.ROC_HDR:].zero_()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                K.roc_accum(args, stream)
                K.roc_finish(args, stream)
                e1.record()
                e1.synchronize()
                if i >= a.warmup:
                    kt.append(e0.elapsed_time(e1) * 1e3)
            for i in range(a.warmup + a.calls):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = MT.roc_curve(labels, scores, w)
                t1 = time.perf_counter()
                if i >= a.warmup:
                    ct.append((t1 - t0) * 1e6)
            rec[label] = {"kernels_us": round(statistics.median(kt), 1), "kernels_us_min_max": [round(min(kt), 1), round(max(kt), 1)],
                          "call_us": round(statistics.median(ct), 1), "call_us_min_max": [round(min(ct), 1), round(max(ct), 1)],
                          "auc": r.auc, "points": int(len(r.fpr))}
        out["cases"][name] = rec
    for label in ("unweighted", "weighted"):
        out["ratio_all_ones_over_uniform_" + label] = {
            t: round(out["cases"]["all_ones"][label][t] / out["cases"]["uniform"][label][t], 3) for t in ("kernels_us", "call_us")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

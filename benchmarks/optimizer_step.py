"""Step time of the RPV CNN ([16,32,64]/[128], 64x64x3, B=128) per optimizer on one GPU.

    python benchmarks/optimizer_step.py [--opts Adam,Adagrad,Adamax,AMSGrad] [--rounds 6] [--steps 256]

Method (the README's sample-weight measurement): one model per optimizer, all alive at once;
``rounds`` interleaved rounds, in each of which every model runs ``steps`` training steps as
32-step graph replays, timed with device events after a settle run; the figure is the median of a
model's rounds.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from cori_intml_examples_amd import optim  # noqa: E402
from cori_intml_examples_amd.apps import zoo  # noqa: E402
from cori_intml_examples_amd.utils import set_random_seed  # noqa: E402

REPLAY = 32


def make_opt(name):
    return optim.Adam(amsgrad=True) if name == "AMSGrad" else getattr(optim, name)()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--opts", default="Adam,Adagrad,Adamax,AMSGrad")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--batch", type=int, default=128)
    a = ap.parse_args()
    names = a.opts.split(",")
    bs, reps = a.batch, max(1, a.steps // REPLAY)
    rs = np.random.RandomState(0)
    x = rs.rand(bs * REPLAY, 64, 64, 3).astype(np.float32)
    y = (rs.rand(bs * REPLAY) > 0.5).astype(np.float32)
    runs = {}
    for nm in names:
        set_random_seed(1)
        m = zoo.rpv_cnn((64, 64, 3), conv_sizes=[16, 32, 64], fc_sizes=[128], dropout=0.2, optimizer=make_opt(nm),
                        lr=None, device="cuda:0")
        ex = m._executor
        d = ex.upload(x, y)
        perm = torch.arange(d.n, device=ex.device)
        runs[nm] = (m, ex, d, perm)

    def timed(nm, n):
        _, ex, d, perm = runs[nm]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            ex.train_steps(d, perm, 0, bs, REPLAY)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / (n * REPLAY)      # us per step

    for nm in names:                    # graph capture + clock settle
        timed(nm, 4)
    us = {nm: [] for nm in names}
    for _ in range(a.rounds):
        for nm in names:
            timed(nm, 2)                # back under load after the other models' turn
            us[nm].append(timed(nm, reps))
    out = {"workload": "rpv_cnn 64x64x3 [16,32,64]/[128] B=%d" % bs, "steps_per_run": reps * REPLAY, "rounds": a.rounds,
           "us_per_step_median": {nm: round(statistics.median(v), 2) for nm, v in us.items()},
           "us_per_step_runs": {nm: [round(t, 2) for t in v] for nm, v in us.items()},
           "launches": {nm: [it[0] for it in runs[nm][1]._plans[(bs, "train")].launches] for nm in names},
           "finite": {nm: bool(np.isfinite(runs[nm][0].store.master[:runs[nm][0].store.numel].sum().item()))
                      for nm in names}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

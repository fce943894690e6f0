"""Worker for tests/test_regularizers.py: 2 gloo ranks on the CPU (under ``torch.distributed.run``,
as tests/clip_dp_worker.py).  Every rank adds the regularizers' term to its own local gradient,
then the gradients are averaged; weights are identical on all ranks, so the step equals the
single-process step at the global batch.  One data-parallel SGD step of the regularized tiny model
against that single-process step, and every rank's reported loss against its own data loss (from
an unregularized twin) plus the float64 oracle's penalty.  Writes one JSON report per rank."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from cori_intml_examples_amd import optim  # noqa: E402
from cori_intml_examples_amd.io.datasets import synthetic_rpv  # noqa: E402
from cori_intml_examples_amd.parallel import hvd  # noqa: E402
from cori_intml_examples_amd.utils import set_random_seed  # noqa: E402

from helpers import reg_models as M  # noqa: E402
from helpers import reg_oracle as G  # noqa: E402

LR = 0.1


def main(out_dir):
    hvd.init()
    r, n = hvd.rank(), hvd.size()
    rep = {"rank": r, "size": n}
    set_random_seed(11)
    xs, ys = zip(*[synthetic_rpv(8, size=16, seed=40 + k)[:2] for k in range(n)])   # different data per rank
    x, y = xs[r], ys[r]
    # the single-process step at the global batch (equal shards: its mean is the ranks' average)
    single = M.tiny(optim.SGD(lr=LR), channels=1)
    w0 = [w.copy() for w in single.get_weights()]
    nel = single.store.numel
    p0 = single.store.master[:nel].double().numpy().copy()
    ranges = single.regularized_ranges()
    rep["ranges"] = len(ranges)
    single.train_on_batch(np.concatenate(xs), np.concatenate(ys))
    want = single.store.master[:nel].double().numpy()
    # this rank's data loss at w0
    twin = M.tiny(optim.SGD(lr=LR), channels=1, reg=False)
    twin.set_weights(w0)
    data_loss = twin.test_on_batch(x, y)[0]
    # the data-parallel step
    m = M.tiny(optim.SGD(lr=LR), channels=1, dp=True)
    m.set_weights(w0)
    hvd.broadcast_model_state(m, 0)
    rep["w0_equal"] = bool(np.array_equal(m.store.master[:nel].double().numpy(), p0))
    loss = m.train_on_batch(x, y)[0]
    got = m.store.master[:nel].double().numpy()
    rep["buckets"] = len(m._executor.reducer.buckets)
    rep["penalty"] = G.penalty(ranges, p0)
    rep["loss"], rep["data_loss"] = float(loss), float(data_loss)
    rep["err_vs_single"] = float(np.abs(got - want).max())
    rep["moved"] = float(np.abs(got - p0).max())
    # the unregularized twin's step, to show the term changed the update
    twin.train_on_batch(np.concatenate(xs), np.concatenate(ys))
    rep["diff_vs_unregularized"] = float(np.abs(got - twin.store.master[:nel].double().numpy()).max())
    rep["w1_digest"] = [float(got.sum()), float(np.abs(got).sum())]
    with open(os.path.join(out_dir, "rank%d.json" % r), "w") as f:
        json.dump(rep, f)
    hvd.shutdown()


if __name__ == "__main__":
    main(sys.argv[1])

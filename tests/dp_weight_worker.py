"""Worker for tests/test_sample_weight.py::test_dp_two_ranks_weighted: runs under
``torch.distributed.run`` (gloo, CPU).  Sample weights under data parallelism: every rank
normalises by its own local count of non-zero weights (Horovod over Keras), so with strictly
positive weights the DP step equals the single-process step on the global batch."""
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cori_intml_examples_amd.apps import zoo  # noqa: E402
from cori_intml_examples_amd.io.datasets import synthetic_rpv  # noqa: E402
from cori_intml_examples_amd.parallel import hvd  # noqa: E402
from cori_intml_examples_amd.utils import set_random_seed  # noqa: E402


def _model(use_horovod):
    return zoo.rpv_cnn((16, 16, 1), conv_sizes=[4, 8, 8], fc_sizes=[16], dropout=0.0, optimizer="Adam",
                       lr=0.01, use_horovod=use_horovod, device="cpu")


def _flat(m):
    return np.concatenate([w.reshape(-1) for w in m.get_weights()])


def main(out_dir):
    hvd.init()
    r, n = hvd.rank(), hvd.size()
    rep = {"rank": r, "size": n}
    set_random_seed(1000 + r)
    m = _model(True)
    hvd.broadcast_model_state(m, 0)
    w0 = [w.copy() for w in m.get_weights()]

    per = 8
    x, y, _ = synthetic_rpv(per * n, size=16, seed=5)
    sw = (0.25 + 3.75 * np.random.RandomState(2).rand(per * n)).astype(np.float32)   # strictly positive
    sl = slice(r * per, (r + 1) * per)
    m.train_on_batch(x[sl], y[sl], sample_weight=sw[sl])
    w1 = _flat(m)
    rep["w1"] = hashlib.sha256(w1.tobytes()).hexdigest()
    if r == 0:
        ref = _model(False)
        ref.set_weights(w0)
        ref.train_on_batch(x, y, sample_weight=sw)
        rep["dp_vs_single_maxdiff"] = float(np.abs(_flat(ref) - w1).max())
        unw = _model(False)
        unw.set_weights(w0)
        unw.train_on_batch(x, y)
        rep["weighted_differs_from_unweighted"] = float(np.abs(_flat(unw) - w1).max())

    # a weighted fit with weighted validation: the ranks stay in lockstep
    from cori_intml_examples_amd.apps.rpv import train_model
    xt, yt, _ = synthetic_rpv(64, size=16, seed=7 + r)
    xv, yv, _ = synthetic_rpv(32, size=16, seed=99)
    wt = (0.25 + 3.75 * np.random.RandomState(10 + r).rand(64)).astype(np.float32)
    wv = (0.25 + 3.75 * np.random.RandomState(20).rand(32)).astype(np.float32)
    train_model(m, xt, yt, xv, yv, batch_size=16, n_epochs=1, use_horovod=True, verbose=0,
                train_weights=wt, valid_weights=wv)
    wf = _flat(m)
    rep["wf"] = hashlib.sha256(wf.tobytes()).hexdigest()
    with open(os.path.join(out_dir, "wrank%d.json" % r), "w") as f:
        json.dump(rep, f)
    hvd.shutdown()


if __name__ == "__main__":
    main(sys.argv[1])

"""Worker for tests/test_clipping.py: 2 gloo ranks on the CPU (under ``torch.distributed.run``,
as tests/dp_worker.py).  Horovod's DistributedOptimizer clips each rank's OWN gradient by its own
global norm and averages the clipped gradients; this worker measures both ranks' local norms,
picks a clipnorm between them (so exactly one rank clips), runs one data-parallel SGD step and
compares the weights, in float64, with "clip each local gradient, then average" and with
"average, then clip".  Writes one JSON report per rank."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from cori_intml_examples_amd import optim  # noqa: E402
from cori_intml_examples_amd.apps import zoo  # noqa: E402
from cori_intml_examples_amd.io.datasets import synthetic_rpv  # noqa: E402
from cori_intml_examples_amd.parallel import hvd  # noqa: E402
from cori_intml_examples_amd.utils import set_random_seed  # noqa: E402

from helpers import clip_oracle as C  # noqa: E402

LR = 0.1


def tiny(opt, dp):
    return zoo.rpv_cnn((16, 16, 1), conv_sizes=[4, 8, 8], fc_sizes=[16], dropout=0.0, optimizer=opt, lr=None,
                       use_horovod=dp, device="cpu")


def flat(m):
    return np.concatenate([w.reshape(-1) for w in m.get_weights()]).astype(np.float64)


def main(out_dir):
    hvd.init()
    r, n = hvd.rank(), hvd.size()
    rep = {"rank": r, "size": n}
    set_random_seed(11)
    x, y, _ = synthetic_rpv(8, size=16, seed=40 + r)              # different data per rank
    # this rank's local gradient: one step of an unclipped single-process twin (its store keeps it)
    twin = tiny(optim.SGD(lr=LR), False)
    w0 = [w.copy() for w in twin.get_weights()]
    nel = twin.store.numel
    p0 = twin.store.master[:nel].double().numpy().copy()            # flat, in the gradient's order
    twin.train_on_batch(x, y)
    g_local = twin.store.grad[:nel].double().numpy().copy()
    norms = hvd.allgather(C.global_norm(g_local))
    rep["norms"] = norms
    c = float(np.sqrt(norms[0] * norms[1]))                        # between the two local norms
    rep["clipnorm"] = c
    # the data-parallel step
    m = tiny(optim.SGD(lr=LR, clipnorm=c), True)
    m.set_weights(w0)
    hvd.broadcast_model_state(m, 0)
    rep["w0_equal"] = bool(np.array_equal(m.store.master[:nel].double().numpy(), p0))
    m.train_on_batch(x, y)
    w1 = flat(m)
    rep["w1_digest"] = [float(w1.sum()), float(np.abs(w1).sum())]
    rep["dist_clipnorm"] = m.optimizer.clipnorm
    p1 = m.store.master[:nel].double().numpy()
    grads = hvd.allgather(g_local.tolist())
    if r == 0:
        gs = [np.asarray(g, dtype=np.float64) for g in grads]
        clipped = [C.clip(g, clipnorm=c) for g in gs]
        rep["fired"] = [bool(info["fired"]) for _, info in clipped]
        a = p0 - LR * np.mean([g for g, _ in clipped], axis=0)     # clip each, then average
        b = p0 - LR * C.clip(np.mean(gs, axis=0), clipnorm=c)[0]   # average, then clip
        rep["err_clip_then_average"] = float(np.abs(p1 - a).max())
        rep["err_average_then_clip"] = float(np.abs(p1 - b).max())
    with open(os.path.join(out_dir, "rank%d.json" % r), "w") as f:
        json.dump(rep, f)
    hvd.shutdown()


if __name__ == "__main__":
    main(sys.argv[1])

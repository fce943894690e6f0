"""Worker for tests/test_batchnorm.py: 2 gloo ranks on the CPU (under ``torch.distributed.run``, as
tests/reg_dp_worker.py).  Horovod-over-Keras semantics: every rank normalises with its OWN batch
statistics and keeps its OWN moving statistics, gamma / beta gradients are averaged like every
other gradient, the broadcast carries the moving statistics, and the per-epoch weight digest
covers trainable weights only.  Writes one JSON report per rank."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from cori_intml_examples_amd import optim  # noqa: E402
from cori_intml_examples_amd.io.datasets import synthetic_rpv  # noqa: E402
from cori_intml_examples_amd.parallel import hvd  # noqa: E402
from cori_intml_examples_amd.train.loop import dp_consistency_check, weight_digest  # noqa: E402
from cori_intml_examples_amd.utils import set_random_seed  # noqa: E402

from helpers import bn_models as M  # noqa: E402
from helpers import bn_oracle as O  # noqa: E402


def moving(m):
    return [w for l in m.layers for w, (n, _, _) in zip(l.get_weights(), l.weight_specs()) if n.startswith("moving")]


def main(out_dir):
    hvd.init()
    r, n = hvd.rank(), hvd.size()
    rep = {"rank": r, "size": n}
    set_random_seed(11 + r)                                  # different initial weights per rank ...
    x, y, _ = synthetic_rpv(8, size=16, channels=3, seed=40 + r)       # ... and different data
    m = M.tiny(optim.SGD(lr=0.1), dp=True, momentum=0.5)
    # rank 0's moving statistics are made recognisable before the broadcast
    ws = m.get_weights()
    for i, s in enumerate(m.store.specs):
        if not s.trainable:
            ws[i] = ws[i] + (0.25 if r == 0 else 0.75)
    m.set_weights(ws)
    hvd.broadcast_model_state(m, 0)
    mv0 = moving(m)
    rep["moving_after_broadcast"] = [float(w.mean()) for w in mv0]
    w0 = m.get_weights()
    nel = m.store.numel
    m.train_on_batch(x, y)
    got = m.store.master[:nel].double().numpy()
    rep["trainable_digest"] = weight_digest(m)
    rep["moved"] = float(np.abs(got - np.concatenate([w.reshape(-1) for w, s in zip(w0, m.store.specs) if s.trainable])).max())
    # this rank's own local oracle for the moving statistics: its own batch through the same weights
    _, _, stats = M.torch_loss_grads(_twin(w0), x, y, step=1)
    errs = []
    k = 0
    bns = [l for l in m.layers if type(l).__name__ == "BatchNormalization"]
    for layer, (_, mean, var, rows) in zip(bns, stats):      # (the twin's layers have names of their own)
        wm, wv = O.moving_update(mv0[k], mv0[k + 1], mean, var, rows, layer.momentum, layer.epsilon)
        mm, mvv = layer.get_weights()[-2:]
        errs.append(float(max(np.abs(mm - wm).max(), np.abs(mvv - wv).max())))
        k += 2
    rep["moving_err_vs_local_oracle"] = max(errs)
    rep["moving_digest"] = [float(np.concatenate([w.reshape(-1) for w in moving(m)]).sum())]
    m.history = type("H", (), {"dp_consistency": []})()
    rep["digest_check_identical"] = bool(dp_consistency_check(m, 0)["identical"])
    with open(os.path.join(out_dir, "rank%d.json" % r), "w") as f:
        json.dump(rep, f)
    hvd.shutdown()


def _twin(w0):
    t = M.tiny(optim.SGD(lr=0.1), momentum=0.5)
    t.set_weights(w0)
    return t


if __name__ == "__main__":
    main(sys.argv[1])

"""GPU worker for tests/test_roc_metrics_gpu.py: a model compiled with the ROC and weighted metrics
through the data-parallel step on ONE MI355X (INTML_DP_FORCE=1, the native RCCL engine at size 1, as
tests/pool_dp_worker_gpu.py).  roc_accum sits directly behind the head, ahead of every slab
reduction; it has no parameters and touches no gradient, so with one rank (the all-reduce is the
identity, grad_scale is 1, Adamax's update is compiled without fp contraction) the data-parallel
step must train bit-identically to the single-GPU step, captured and segmented, and every rank's
own validation pass gives the same val_auc.  Writes a JSON report."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ["INTML_DP_FORCE"] = "1"

import torch  # noqa: E402

from cori_intml_examples_amd import optim  # noqa: E402
from cori_intml_examples_amd.models import Conv2D, Dense, Dropout, Flatten, Input, MaxPooling2D, Model  # noqa: E402
from cori_intml_examples_amd.io.datasets import synthetic_rpv  # noqa: E402
from cori_intml_examples_amd.parallel import dist, hvd  # noqa: E402
from cori_intml_examples_amd.utils import set_random_seed  # noqa: E402


def tiny(dp):
    inp = Input(shape=(16, 16, 3))
    h = MaxPooling2D((2, 2))(Conv2D(4, (3, 3), activation="relu", padding="same")(inp))
    h = Dropout(0.2)(MaxPooling2D((2, 2))(Conv2D(8, (3, 3), activation="relu", padding="same")(h)))
    h = Dropout(0.2)(Dense(16, activation="relu")(Flatten()(h)))
    m = Model(inp, Dense(1, activation="sigmoid")(h), device="cuda:0")
    opt = optim.Adamax()
    m.compile(optimizer=hvd.DistributedOptimizer(opt) if dp else opt, loss="binary_crossentropy",
              metrics=["accuracy", "auc"], weighted_metrics=["auc"])
    return m


def main(out):
    rep = {}
    st = hvd.init()
    rep["native"] = st.comm is not None
    x, y, _ = synthetic_rpv(160, size=16, channels=3, seed=5)
    w = np.random.RandomState(2).uniform(0.1, 3.0, 160).astype(np.float32)

    def train(m):
        for i in range(4):
            sl = slice(i * 32, (i + 1) * 32)
            last = m.train_on_batch(x[sl], y[sl], sample_weight=w[sl])
        val = m.evaluate(x[128:], y[128:], batch_size=16, sample_weight=w[128:], verbose=0)
        torch.cuda.synchronize()
        n = m.store.numel
        names = m.metrics_names
        return ([m.store.master[:n].cpu().numpy()] + [s.cpu().numpy() for s in m._executor.optimizer_state()],
                dict(zip(names, last)), dict(zip(names, val)))

    os.environ.pop("INTML_XGMI", None)
    os.environ["INTML_TUNE"] = ""
    set_random_seed(1)
    base = tiny(False)
    w0 = base.get_weights()
    ref, last, val = train(base)
    bplan = base._executor._plans[(32, "train", "w")]
    rep["moved"] = float(np.abs(ref[0] - np.concatenate([a.reshape(-1) for a in w0])).max())
    rep["base_launches"] = [it[0] for it in bplan.launches]
    rep["base_auc"], rep["base_val_auc"], rep["base_val_weighted_auc"] = last["auc"], val["auc"], val["weighted_auc"]
    for mode, tv in (("captured", "comm_capture=1"), ("segmented", "comm_capture=0")):
        os.environ["INTML_TUNE"] = tv
        set_random_seed(1)          # the same model seed: the same dropout masks
        m = tiny(True)
        assert m._seed == base._seed
        m.set_weights(w0)
        got, last, val = train(m)
        red = m._executor.reducer
        plan = m._executor._plans[(32, "train", "w")]
        rep[mode] = {"reducer": type(red).__name__, "plane": red.plane,
                     "comm_in_graph": bool(plan.comm_in_graph),
                     "launches": [it[0] for it in plan.launches],
                     "identical": [bool(np.array_equal(a, b)) for a, b in zip(got, ref)],
                     "max_abs_diff": [float(np.abs(a - b).max()) for a, b in zip(got, ref)],
                     "iterations": int(m.optimizer.iterations),
                     "auc": last["auc"], "val_auc": val["auc"], "val_weighted_auc": val["weighted_auc"]}
    with open(out, "w") as f:
        json.dump(rep, f, indent=1)
    dist.shutdown()


if __name__ == "__main__":
    main(sys.argv[1])

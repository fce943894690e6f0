"""GPU worker for tests/test_loss_head_gpu.py: a model whose output head runs the second head kernel
(Dense(3), linear, hinge) through the data-parallel step on ONE MI355X (INTML_DP_FORCE=1, the native
RCCL engine at size 1, as tests/pool_dp_worker_gpu.py).  The loss head writes head_kernel's slabs in
head_kernel's layouts, so the gradient route is the one of any other model; with one rank the
all-reduce is the identity and grad_scale is 1, and Adamax's update is compiled without fp
contraction, so the data-parallel step must train bit-identically to the single-GPU step -- weights
and every state slot, captured and segmented.  Writes a JSON report."""
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
    h = Dropout(0.2)(MaxPooling2D()(Conv2D(4, (3, 3), activation="relu", padding="same")(inp)))
    h = Dropout(0.2)(Dense(16, activation="relu")(Flatten()(h)))
    m = Model(inp, Dense(3)(h), device="cuda:0")
    opt = optim.Adamax()
    m.compile(optimizer=hvd.DistributedOptimizer(opt) if dp else opt, loss="hinge", metrics=["accuracy"])
    return m


def main(out):
    rep = {}
    st = hvd.init()
    rep["native"] = st.comm is not None
    x, _, _ = synthetic_rpv(128, size=16, channels=3, seed=5)
    y = np.where(np.random.RandomState(6).rand(128, 3) < 0.5, -1.0, 1.0).astype(np.float32)

    def train(m):
        for i in range(4):
            m.train_on_batch(x[i * 32:(i + 1) * 32], y[i * 32:(i + 1) * 32])
        torch.cuda.synchronize()
        n = m.store.numel
        return [m.store.master[:n].cpu().numpy()] + [s.cpu().numpy() for s in m._executor.optimizer_state()]

    os.environ.pop("INTML_XGMI", None)
    os.environ["INTML_TUNE"] = ""
    set_random_seed(1)
    base = tiny(False)
    w0 = base.get_weights()
    ref = train(base)
    bplan = next(iter(base._executor._plans.values()))
    rep["moved"] = float(np.abs(ref[0] - np.concatenate([w.reshape(-1) for w in w0])).max())
    rep["base_launches"] = [it[0] for it in bplan.launches]
    for mode, tv in (("captured", "comm_capture=1"), ("segmented", "comm_capture=0")):
        os.environ["INTML_TUNE"] = tv
        set_random_seed(1)          # the same model seed: the same dropout masks
        m = tiny(True)
        assert m._seed == base._seed
        m.set_weights(w0)
        got = train(m)
        red = m._executor.reducer
        plan = next(iter(m._executor._plans.values()))
        rep[mode] = {"reducer": type(red).__name__, "plane": red.plane,
                     "comm_in_graph": bool(plan.comm_in_graph),
                     "launches": [it[0] for it in plan.launches],
                     "identical": [bool(np.array_equal(a, b)) for a, b in zip(got, ref)],
                     "max_abs_diff": [float(np.abs(a - b).max()) for a, b in zip(got, ref)],
                     "iterations": int(m.optimizer.iterations)}
    with open(out, "w") as f:
        json.dump(rep, f, indent=1)
    dist.shutdown()


if __name__ == "__main__":
    main(sys.argv[1])

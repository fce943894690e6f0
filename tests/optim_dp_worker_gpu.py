"""GPU worker for tests/test_new_optimizers_gpu.py: Adagrad, Adamax and Adam(amsgrad=True) through
the data-parallel step on ONE MI355X (INTML_DP_FORCE=1, the native RCCL engine at size 1, as
tests/comm_worker_gpu.py).  With one rank the all-reduce is the identity and grad_scale is 1, and
the update of these kinds is compiled without fp contraction, so the data-parallel step
(optim_kernel behind the all-reduce) must train bit-identically to the single-GPU step
(reduce_optim_kernel) -- weights and every state slot, captured and segmented.  A forced xGMI
plane must be refused with a ValueError.  Writes a JSON report."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["INTML_DP_FORCE"] = "1"

import torch  # noqa: E402

from cori_intml_examples_amd import optim  # noqa: E402
from cori_intml_examples_amd.apps import zoo  # noqa: E402
from cori_intml_examples_amd.io.datasets import synthetic_rpv  # noqa: E402
from cori_intml_examples_amd.parallel import dist, hvd  # noqa: E402
from cori_intml_examples_amd.utils import set_random_seed  # noqa: E402

KINDS = ("Adagrad", "Adamax", "AMSGrad")


def make_opt(name):
    return optim.Adam(amsgrad=True) if name == "AMSGrad" else getattr(optim, name)()


def tiny(name, dp):
    return zoo.rpv_cnn((16, 16, 3), conv_sizes=[4, 8, 8], fc_sizes=[16], dropout=0.2, optimizer=make_opt(name),
                       lr=None, use_horovod=dp, device="cuda:0")


def main(out):
    rep = {}
    st = hvd.init()
    rep["native"] = st.comm is not None
    x, y, _ = synthetic_rpv(128, size=16, channels=3, seed=5)

    def train(m):
        for i in range(4):
            m.train_on_batch(x[i * 32:(i + 1) * 32], y[i * 32:(i + 1) * 32])
        torch.cuda.synchronize()
        n = m.store.numel
        return [m.store.master[:n].cpu().numpy()] + [s.cpu().numpy() for s in m._executor.optimizer_state()]

    for name in KINDS:
        os.environ.pop("INTML_XGMI", None)
        os.environ["INTML_TUNE"] = ""
        set_random_seed(1)
        base = tiny(name, False)
        w0 = base.get_weights()
        ref = train(base)
        r = {"n_state": len(ref) - 1, "moved": float(np.abs(ref[0] - np.concatenate([w.reshape(-1) for w in w0])).max()),
             "base_fused": bool(next(iter(base._executor._plans.values())).optim_fused)}
        for mode, tv in (("captured", "comm_capture=1"), ("segmented", "comm_capture=0")):
            os.environ["INTML_TUNE"] = tv
            set_random_seed(1)          # the same model seed: the same dropout masks
            m = tiny(name, True)
            assert m._seed == base._seed
            m.set_weights(w0)
            got = train(m)
            red = m._executor.reducer
            plan = next(iter(m._executor._plans.values()))
            r[mode] = {"reducer": type(red).__name__, "plane": red.plane, "xgmi": red.xgmi is not None,
                       "comm_in_graph": bool(plan.comm_in_graph), "early_red": len(plan.early_red or {}),
                       "launches": [it[0] for it in plan.launches if "optim" in it[0] or "allreduce" in it[0]
                                    or "xgmi" in it[0] or "xchg" in it[0]],
                       "identical": [bool(np.array_equal(a, b)) for a, b in zip(got, ref)],
                       "max_abs_diff": [float(np.abs(a - b).max()) for a, b in zip(got, ref)],
                       "iterations": int(m.optimizer.iterations)}
        os.environ["INTML_TUNE"] = "comm_capture=1"
        for plane in ("xgmi", "hybrid"):
            os.environ["INTML_XGMI"] = plane
            try:
                m = tiny(name, True)
                m.train_on_batch(x[:32], y[:32])
                r["forced_" + plane] = "no error"
            except ValueError as e:
                r["forced_" + plane] = str(e)
        os.environ.pop("INTML_XGMI", None)
        rep[name] = r
    # History.data_plane of a fit() with one of them
    m = tiny("Adamax", True)
    h = m.fit(x, y, batch_size=32, epochs=1, verbose=0)
    rep["history_data_plane"] = h.data_plane
    with open(out, "w") as f:
        json.dump(rep, f, indent=1)
    dist.shutdown()


if __name__ == "__main__":
    main(sys.argv[1])

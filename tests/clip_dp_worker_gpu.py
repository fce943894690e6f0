"""GPU worker for tests/test_clipping_gpu.py: gradient clipping through the data-parallel step on
ONE MI355X (INTML_DP_FORCE=1, the native RCCL engine at size 1, as tests/optim_dp_worker_gpu.py).
The step must run on the RCCL plane with ONE bucket and the launch order "local slab reduction,
grad_sqnorm, grad_clip_apply, all-reduce, unclipped optim_kernel", captured and segmented.  With
one rank the all-reduce is the identity and grad_scale is 1, so the weights and slots must match
the single-GPU clipped run (which clips on the fly inside the optimizer launch) within the
optimizer tests' bound; whether they are bit-identical is reported, not asserted (the five-way
kinds are compiled with fp contraction).  A forced xGMI / hybrid plane must be refused with a
ValueError naming the optimizer and the plane.  Writes a JSON report."""
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

KINDS = ("Adam", "Adamax")          # a five-way kind and a stand-alone kind
CLIPNORM = 0.05                     # below every step's gradient norm of this model (0.16 .. 0.2)


def tiny(name, dp):
    return zoo.rpv_cnn((16, 16, 3), conv_sizes=[4, 8, 8], fc_sizes=[16], dropout=0.2,
                       optimizer=getattr(optim, name)(clipnorm=CLIPNORM), lr=None, use_horovod=dp, device="cuda:0")


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
        bplan = next(iter(base._executor._plans.values()))
        r = {"moved": float(np.abs(ref[0] - np.concatenate([w.reshape(-1) for w in w0])).max()),
             "base_fused": bool(bplan.optim_fused),
             "base_sqnorm": [it[0] for it in bplan.launches].count("grad_sqnorm"),
             "clipnorm": CLIPNORM, "bound": 2e-5 * max(1.0, 100 * float(base.optimizer.lr))}
        for mode, tv in (("captured", "comm_capture=1"), ("segmented", "comm_capture=0")):
            os.environ["INTML_TUNE"] = tv
            set_random_seed(1)          # the same model seed: the same dropout masks
            m = tiny(name, True)
            assert m._seed == base._seed
            m.set_weights(w0)
            got = train(m)
            ex = m._executor
            red = ex.reducer
            plan = next(iter(ex._plans.values()))
            n = m.store.numel
            r[mode] = {"reducer": type(red).__name__, "plane": red.plane, "xgmi": red.xgmi is not None,
                       "comm_in_graph": bool(plan.comm_in_graph), "early_red": len(plan.early_red or {}),
                       "buckets": len(red.buckets),
                       "launches": [it[0] for it in plan.launches if "optim" in it[0] or "allreduce" in it[0]
                                    or "xgmi" in it[0] or "xchg" in it[0] or "reduce" in it[0] or "sqnorm" in it[0]
                                    or "clip" in it[0]],
                       "factor": float(ex.clip_state[ex.K.CLIP_FACTOR].item()),
                       "grad_norm": float(m.store.grad[:n].double().norm().item()),
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
    m = tiny("Adam", True)
    h = m.fit(x, y, batch_size=32, epochs=1, verbose=0)
    rep["history_data_plane"] = h.data_plane
    with open(out, "w") as f:
        json.dump(rep, f, indent=1)
    dist.shutdown()


if __name__ == "__main__":
    main(sys.argv[1])

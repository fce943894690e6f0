"""GPU worker for tests/test_regularizers_gpu.py: weight regularizers through the data-parallel
step on ONE MI355X (INTML_DP_FORCE=1, the native RCCL engine at size 1, as
tests/clip_dp_worker_gpu.py).  The step must run on the RCCL plane with ONE bucket and the launch
order "local slab reduction, weight_reg, [grad_sqnorm, grad_clip_apply,] all-reduce, optim",
captured and segmented.  With one rank the all-reduce is the identity and grad_scale is 1, so the
weights and slots must match the single-GPU regularized run within the optimizer tests' bound.  A
forced xGMI / hybrid plane must be refused with a ValueError naming the regularized layers and the
plane; auto falls back to rccl, recorded in History.data_plane.  Writes a JSON report."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ["INTML_DP_FORCE"] = "1"

import torch  # noqa: E402

from cori_intml_examples_amd import optim  # noqa: E402
from cori_intml_examples_amd.io.datasets import synthetic_rpv  # noqa: E402
from cori_intml_examples_amd.parallel import dist, hvd  # noqa: E402
from cori_intml_examples_amd.utils import set_random_seed  # noqa: E402

from helpers import reg_models as M  # noqa: E402

CASES = {"Adam": {}, "Adamax+clipnorm": {"clipnorm": 0.1}}     # (0.1: below every step's regularized norm, 0.4 .. 0.5)
SHOWN = ("optim", "allreduce", "xgmi", "xchg", "reduce", "sqnorm", "clip", "weight_reg")


def tiny(case, dp):
    name = case.split("+")[0]
    return M.tiny(getattr(optim, name)(**CASES[case]), device="cuda:0", drop=0.2, dp=dp)


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

    for case in CASES:
        os.environ.pop("INTML_XGMI", None)
        os.environ["INTML_TUNE"] = ""
        set_random_seed(1)
        base = tiny(case, False)
        w0 = base.get_weights()
        ref = train(base)
        bplan = next(iter(base._executor._plans.values()))
        r = {"moved": float(np.abs(ref[0] - np.concatenate([w.reshape(-1) for w in w0])).max()),
             "base_fused": bool(bplan.optim_fused),
             "base_launches": [it[0] for it in bplan.launches if any(k in it[0] for k in SHOWN)],
             "base_penalty": float(base._executor.reg_state[base._executor.K.REG_PENALTY].item()),
             "layers": base.store.regularized_layers(),
             "bound": 2e-5 * max(1.0, 100 * float(base.optimizer.lr))}
        for mode, tv in (("captured", "comm_capture=1"), ("segmented", "comm_capture=0")):
            os.environ["INTML_TUNE"] = tv
            set_random_seed(1)          # the same model seed: the same dropout masks
            m = tiny(case, True)
            assert m._seed == base._seed
            m.set_weights(w0)
            got = train(m)
            ex = m._executor
            red = ex.reducer
            plan = next(iter(ex._plans.values()))
            r[mode] = {"reducer": type(red).__name__, "plane": red.plane, "xgmi": red.xgmi is not None,
                       "comm_in_graph": bool(plan.comm_in_graph), "early_red": len(plan.early_red or {}),
                       "buckets": len(red.buckets),
                       "launches": [it[0] for it in plan.launches if any(k in it[0] for k in SHOWN)],
                       "penalty": float(ex.reg_state[ex.K.REG_PENALTY].item()),
                       "identical": [bool(np.array_equal(a, b)) for a, b in zip(got, ref)],
                       "max_abs_diff": [float(np.abs(a - b).max()) for a, b in zip(got, ref)],
                       "iterations": int(m.optimizer.iterations)}
        os.environ["INTML_TUNE"] = "comm_capture=1"
        for plane in ("xgmi", "hybrid"):
            os.environ["INTML_XGMI"] = plane
            try:
                m = tiny(case, True)
                m.train_on_batch(x[:32], y[:32])
                r["forced_" + plane] = "no error"
            except ValueError as e:
                r["forced_" + plane] = str(e)
        os.environ.pop("INTML_XGMI", None)
        rep[case] = r
    m = tiny("Adam", True)
    h = m.fit(x, y, batch_size=32, epochs=1, verbose=0)
    rep["history_data_plane"] = h.data_plane
    rep["history_loss_finite"] = bool(np.isfinite(h.history["loss"][0]))
    with open(out, "w") as f:
        json.dump(rep, f, indent=1)
    dist.shutdown()


if __name__ == "__main__":
    main(sys.argv[1])

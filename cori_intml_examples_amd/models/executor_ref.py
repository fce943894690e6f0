"""CPU reference backend: executes a Plan with the fp32 PyTorch ops of
``ops/reference.py``.  This is the "MNIST 3-layer CNN single-process Keras fit() on
CPU (plumbing, no GPU)" configuration of BASELINE.json and the oracle for the
whole-model HIP tests.  Forward/backward are written out explicitly (no autograd
graph) in exactly the stage order the HIP executor uses.

``INTML_TUNE=ref_bf16=1`` makes it a bf16-FAITHFUL oracle: values are rounded to bf16 at
exactly the points where the HIP step stores them in bf16 (weight packs of the convs and
hidden denses, every stage output after its dropout, the hidden denses' dH and every pooled
dP after their masks; for a stage with a hidden activation also its pre-activation, which the
GPU stores between its linear kernels and the activation launch, and its gradient on both sides of
the multiplication by A'; for a BatchNormalization stage its pre-activation z before the
statistics, the pooled gradient buffer and dz; for an average-pooled stage its un-pooled activation
before the averaging, the pooled output once, the pooled gradient and dz; the global pooling
stage's output and gradient, the GlobalMaxPooling2D index taken on the stored values the GPU
kernel reads), everything else in fp32 -- so the whole-step gradient test can use
the per-kernel tests' tight tolerances instead of the loose fp32-vs-bf16 bound.
"""
from __future__ import annotations

from typing import List

import numpy as np
import torch

from ..ops import reference as R
from ..ops.rng import dropout_keep
from ..optim.optimizers import clip_pair
from ..utils.tune import tune
from .executor_base import DeviceData, Executor, prepare_targets
from .plan import Plan, binary_accuracy_head, classic_head


class RefExecutor(Executor):
    def __init__(self, plan: Plan, store, optimizer, seed: int):
        super().__init__(plan, store, optimizer, seed)
        self.device = torch.device("cpu")
        n_slots = getattr(optimizer, "n_slots", 0)
        self.slots: List[torch.Tensor] = [torch.zeros(store.capacity) for _ in range(n_slots)]
        self.m_schedule = 1.0
        self._acc = torch.zeros(3, dtype=torch.float64)
        # binary_accuracy of a multi-column output counts correct ELEMENTS: the divisor per row
        hd = plan.head
        self._acc_div = float(hd.N) if (hd.N > 1 and binary_accuracy_head(hd.loss, hd.N)
                                        and not classic_head(hd.activation, hd.loss, hd.N)) else 1.0
        self._last = (0.0, 0.0)
        self.emulate_bf16 = bool(tune("ref_bf16"))
        # Keras weight regularizers [(lo, hi, l1, l2)], read here (at compile) like the clip values
        self.regs = store.regularized_ranges()
        self._roc = None             # metrics.RocState, the numpy twin of the HIP executor's ROC state
        self._roc_w_seen = False

    def _init_roc(self):
        from ..metrics import RocState
        hd = self.plan.head
        self._roc = RocState(hd.N, hd.activation == "softmax")

    # ------------------------------------------------------------------------------ data
    def upload(self, x, y, w=None):
        xt = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32))
        if xt.shape[1:] != tuple(self.plan.input_shape):
            raise ValueError("input shape %s != model input %s" % (tuple(xt.shape[1:]),
                                                                   self.plan.input_shape))
        yt = torch.as_tensor(prepare_targets(y, self.plan)) if y is not None else None
        wt = torch.as_tensor(np.ascontiguousarray(w, dtype=np.float32)).reshape(-1) if w is not None else None
        if wt is not None and wt.shape[0] != xt.shape[0]:
            raise ValueError("sample weights have %d entries for %d samples" % (wt.shape[0], xt.shape[0]))
        if wt is not None and self.roc_weighted:
            from ..metrics import check_weights
            check_weights(wt.numpy())
        return DeviceData(xt, yt, xt.shape[0], wt)

    # ------------------------------------------------------------------------------ core
    def _mask(self, numel, rate, stream, step):
        keep = dropout_keep(numel, rate, self.seed, stream, step)
        return keep.to(torch.float32) / (1.0 - rate)

    def _q(self, t):
        """bf16 rounding at a HIP storage point (identity unless emulating bf16)."""
        return t.to(torch.bfloat16).to(torch.float32) if self.emulate_bf16 else t

    def _act_slope(self, stage, out, dropped: bool):
        """A' of a stage with a hidden activation from its STORED output: the dropout scale is
        undone first (y = out * fp32(1 - rate), as act_bwd_kernel does; dropped elements carry a
        zero gradient already)."""
        y = out * torch.tensor(1.0 - stage.rate, dtype=torch.float32) if dropped else out
        return R.act_grad_from_output(stage.act, stage.act_alpha, y)

    def _bn_forward(self, bn, z, training: bool):
        """BatchNormalization of the (stored, so rounded) pre-activation z over all axes but the last
        (Keras 2.2.4): batch statistics and the moving update in a training step, the moving statistics
        otherwise.  Returns (u, (xhat, gamma * invstd) or None)."""
        st = self.store
        C = z.shape[-1]
        gamma = st.view(bn, "gamma") if bn.scale else torch.ones(C)
        beta = st.view(bn, "beta") if bn.center else torch.zeros(C)
        eps = torch.tensor(bn.epsilon, dtype=torch.float32)
        if not training:
            inv = 1.0 / torch.sqrt(st.view(bn, "moving_variance") + eps)
            return gamma * ((z - st.view(bn, "moving_mean")) * inv) + beta, None
        z2 = z.reshape(-1, C)
        m = z2.shape[0]
        mean = z2.sum(0) / m
        var = ((z2 - mean) ** 2).sum(0) / m           # biased, about the mean
        inv = 1.0 / torch.sqrt(var + eps)
        xhat = (z - mean) * inv
        # Keras 2.2.4's sample-variance factor m / (m - (1 + eps)); m = 1 gives var = 0 exactly
        mom = torch.tensor(bn.momentum, dtype=torch.float32)
        unb = var * torch.tensor(m / (m - (1.0 + bn.epsilon)), dtype=torch.float32)
        mm, mv = st.view(bn, "moving_mean"), st.view(bn, "moving_variance")
        mm.copy_(mm * mom + mean * (1.0 - mom))
        mv.copy_(mv * mom + unb * (1.0 - mom))
        return gamma * xhat + beta, (xhat, gamma * inv)

    def _bn_backward(self, bn, du, ctx):
        """dz of a BatchNormalization stage from du (un-pooled, dense); writes dgamma / dbeta."""
        st = self.store
        xhat, ginv = ctx
        C = du.shape[-1]
        m = du.numel() // C
        dbeta = du.reshape(-1, C).sum(0)
        dgamma = (du * xhat).reshape(-1, C).sum(0)
        if bn.scale:
            st.view(bn, "gamma", grad=True).copy_(dgamma)
        if bn.center:
            st.view(bn, "beta", grad=True).copy_(dbeta)
        return self._q(ginv * (du - dbeta / m - xhat * (dgamma / m)))

    def _forward(self, x, training: bool, step: int):
        st = self.store
        saved = []
        self._bn_ctx = {}
        a = x
        for cs in self.plan.convs:
            w = self._q(st.view(cs.conv, "kernel"))
            b = st.view(cs.conv, "bias") if cs.conv.use_bias else None
            z = R.conv2d(a, w, b, cs.stride, cs.conv.padding)
            z_code = z
            if cs.bn is not None:
                # z is stored (bf16) before the statistics; everything behind it acts on u = BN(z),
                # and the argmax is taken on the fp32 u
                z, self._bn_ctx[id(cs)] = self._bn_forward(cs.bn, self._q(z), training)
                z_code = z
            r = torch.relu(z) if cs.relu else z
            if cs.act is not None:
                # Keras' order: activate, then pool (the GPU pools the linear conv, then activates:
                # the same for a non-decreasing function)
                r = R.act(cs.act, cs.act_alpha, self._q(z))
            code = None
            p = r
            if cs.pool_kind == "avg":
                # Keras' order, dropout(avgpool(A(conv))): the un-pooled activation is stored, then averaged
                r = self._q(r)
                p = R.avgpool2x2(r)
            elif cs.pool is not None:
                p, code = R.maxpool2x2(r)
                if cs.bn is not None:
                    code = R.maxpool2x2(z_code)[1]
                elif cs.act is not None and self.emulate_bf16:
                    # the bf16 rounding of the pre-activation ties neighbours that the GPU's linear
                    # kernel, which takes the argmax on its fp32 accumulators, never sees tied: the
                    # codes from z (the values are the same: A and the rounding are non-decreasing)
                    code = R.maxpool2x2(z)[1]
            mask = None
            if training and cs.rate > 0:
                mask = self._mask(p.numel(), cs.rate, cs.stream, step).view(p.shape)
                p = p * mask
            a_in, a = a, self._q(p)
            saved.append((a_in, r, code, mask, a))
        gp = self.plan.gpool
        if gp is not None:
            # the global pooling stage reads the last conv stage's STORED output (so does its index)
            p, idx = (R.global_avgpool(a), None) if gp.mode == "avg" else R.global_maxpool(a)
            mask = None
            if training and gp.rate > 0:
                mask = self._mask(p.numel(), gp.rate, gp.stream, step).view(p.shape)
                p = p * mask
            self._gp_ctx = (tuple(a.shape[1:3]), idx, mask)
            a = self._q(p)
        a = a.reshape(a.shape[0], -1)
        for ds in self.plan.denses:
            w = self._q(st.view(ds.dense, "kernel"))
            z = a @ w
            if ds.dense.use_bias:
                z = z + st.view(ds.dense, "bias")
            if ds.bn is not None:
                z, self._bn_ctx[id(ds)] = self._bn_forward(ds.bn, self._q(z), training)
            r = torch.relu(z) if ds.relu else z
            if ds.act is not None:
                r = R.act(ds.act, ds.act_alpha, self._q(z))
            mask = None
            if training and ds.rate > 0:
                mask = self._mask(r.numel(), ds.rate, ds.stream, step).view(r.shape)
                r = r * mask
            a_in, a = a, self._q(r)
            saved.append((a_in, z, None, mask, a))
        hd = self.plan.head
        z = a @ st.view(hd.dense, "kernel")
        if hd.dense.use_bias:
            z = z + st.view(hd.dense, "bias")
        return z, a, saved

    def _head_loss(self, z, y, w=None):
        """Per-row (loss, dlogits, correct); with weights w [M], loss and dlogits carry the row
        factor w_i * M / nnz (R.weight_factor), the accuracy stays unweighted."""
        hd = self.plan.head
        if not classic_head(hd.activation, hd.loss, hd.N):
            # the loss table, or the multi-label binary_crossentropy (corr: correct ELEMENTS per row)
            if hd.loss == "binary_crossentropy":
                loss, dz, corr = R.sigmoid_bce(z, y)
            else:
                loss, dz, corr = R.table_loss(hd.activation, hd.loss, z, y)
        elif hd.activation == "softmax":
            loss, dz, corr = R.softmax_cce(z, y)
        elif hd.activation == "sigmoid":
            loss, dz, corr = R.sigmoid_bce(z.reshape(-1), y.reshape(-1))
            dz = dz.reshape(-1, 1)
        else:
            loss, dz, corr = R.mse(z, y)
        if w is not None:
            loss, dz = R.apply_weights(loss, dz, w)
        return loss, dz, corr

    def _backward(self, dz, a_head, saved):
        st = self.store
        hd = self.plan.head
        st.view(hd.dense, "kernel", grad=True).copy_(a_head.t() @ dz)
        if hd.dense.use_bias:
            st.view(hd.dense, "bias", grad=True).copy_(dz.sum(0))
        da = dz @ st.view(hd.dense, "kernel").t()
        nconv = len(self.plan.convs)
        for i in reversed(range(len(self.plan.denses))):
            ds = self.plan.denses[i]
            a_in, z, _, mask, out = saved[nconv + i]
            if mask is not None:
                da = da * mask
            if ds.relu:
                da = da * (z > 0).to(da.dtype)
            if ds.act is not None:                             # (the masked gradient is stored first)
                da = self._q(da) * self._act_slope(ds, out, mask is not None)
            da = self._q(da)                                   # the stored bf16 dH
            if ds.bn is not None:
                da = self._bn_backward(ds.bn, da, self._bn_ctx[id(ds)])
            st.view(ds.dense, "kernel", grad=True).copy_(a_in.t() @ da)
            if ds.dense.use_bias:
                st.view(ds.dense, "bias", grad=True).copy_(da.sum(0))
            da = da @ self._q(st.view(ds.dense, "kernel")).t()
        gp = self.plan.gpool
        if gp is not None:
            hw, idx, mask = self._gp_ctx
            if mask is not None:
                da = da * mask
            da = self._q(da)                                   # the stored bf16 gradient of the global stage
            da = R.global_avgpool_backward(da, hw) if gp.mode == "avg" else R.global_maxpool_backward(da, idx, hw)
        elif nconv:
            cs_last = self.plan.convs[-1]
            da = da.reshape((da.shape[0],) + tuple(cs_last.out_shape))
        for i in reversed(range(nconv)):
            cs = self.plan.convs[i]
            a_in, r, code, mask, out = saved[i]
            if mask is not None:
                da = da * mask
            if cs.pool_kind == "avg":
                # the stored pooled dP (dropout mask only) -> dz = 0.25 dP [* relu mask of the stored
                # un-pooled activation], stored -> [* A' of that activation, stored]
                da = R.avgpool2x2_backward(self._q(da), r.shape[1:3])
                if cs.relu:
                    da = da * (r > 0).to(da.dtype)
                da = self._q(da)
                if cs.act is not None:
                    da = self._q(da * self._act_slope(cs, r, False))
            elif self.emulate_bf16:
                # the HIP step stores this gradient (masked by the dropout and the ReLU of
                # the stage output, at the stage's output resolution) as bf16 before routing it
                if cs.relu:
                    pooled = R.maxpool2x2(r)[0] if cs.pool is not None else r
                    da = da * (pooled > 0).to(da.dtype)
                da = self._q(da)
            if cs.pool_kind == "avg":
                pass
            elif cs.act is not None:
                da = self._q(da * self._act_slope(cs, out, mask is not None))
            if cs.pool_kind == "max":
                da = R.maxpool2x2_backward(da, code, r.shape[1:3])
            if cs.relu and cs.pool_kind != "avg":
                da = da * (r > 0).to(da.dtype)
            if cs.bn is not None:
                da = self._bn_backward(cs.bn, da, self._bn_ctx[id(cs)])
            dx, dw, db = R.conv2d_backward(a_in, self._q(st.view(cs.conv, "kernel")), da, cs.stride,
                                           cs.conv.padding, need_dx=i > 0)
            st.view(cs.conv, "kernel", grad=True).copy_(dw)
            if cs.conv.use_bias:
                st.view(cs.conv, "bias", grad=True).copy_(db)
            da = dx

    def _apply_update(self):
        opt = self.optimizer
        base = getattr(opt, "_base_optimizer", opt)
        base.iterations += 1
        t = base.iterations
        lr = self.base_lr_for_step(t, float(base.lr))
        if base.initial_decay != 0:
            lr = lr / (1.0 + base.initial_decay * (t - 1))
        n = self.store.numel
        p, g = self.store.master[:n], self.store.grad[:n]
        k = base.kind
        if k == "adam":
            R.adam_update(p, g, self.slots[0][:n], self.slots[1][:n], t, lr, base.beta_1, base.beta_2,
                          base.epsilon)
        elif k == "amsgrad":
            R.amsgrad_update(p, g, self.slots[0][:n], self.slots[1][:n], self.slots[2][:n], t, lr, base.beta_1,
                             base.beta_2, base.epsilon)
        elif k == "adamax":
            R.adamax_update(p, g, self.slots[0][:n], self.slots[1][:n], t, lr, base.beta_1, base.beta_2,
                            base.epsilon)
        elif k == "adagrad":
            R.adagrad_update(p, g, self.slots[0][:n], lr, base.epsilon)
        elif k == "adadelta":
            R.adadelta_update(p, g, self.slots[0][:n], self.slots[1][:n], lr, base.rho, base.epsilon)
        elif k == "nadam":
            self.m_schedule = R.nadam_update(p, g, self.slots[0][:n], self.slots[1][:n], t, lr,
                                             self.m_schedule, base.beta_1, base.beta_2, base.epsilon,
                                             base.schedule_decay)
            base.m_schedule = self.m_schedule
        elif k == "sgd":
            R.sgd_update(p, g, self.slots[0][:n] if self.slots else None, lr, base.momentum,
                         base.nesterov)
        elif k == "rmsprop":
            R.rmsprop_update(p, g, self.slots[0][:n], lr, base.rho, base.epsilon)
        else:
            raise NotImplementedError(k)

    # ------------------------------------------------------------------------------ steps
    def train_step(self, data: DeviceData, perm: torch.Tensor, pos: int, bs: int) -> None:
        idx = perm[pos:pos + bs]
        x, y = data.x[idx], data.y[idx]
        w = data.w[idx] if data.w is not None else None
        base = getattr(self.optimizer, "_base_optimizer", self.optimizer)
        step = base.iterations + 1
        with torch.no_grad():
            z, a_head, saved = self._forward(x, True, step)
            loss, dz, corr = self._head_loss(z, y, w)
            self._backward(dz / bs, a_head, saved)
            # Keras weight regularizers: the penalty of the weights this forward used joins the
            # batch loss (unweighted), its gradient joins this rank's gradient before the clip
            penalty = self._penalty()
            if self.regs:
                R.add_regularization_grad(self.regs, self.store.master, self.store.grad)
            # Keras clipping of this rank's own gradient (Horovod's DistributedOptimizer clips
            # locally, then all-reduces): before the reducer, never on the average
            cn, cv = clip_pair(base)
            if cn or cv:
                R.clip_gradients(self.store.grad[:self.store.numel], cn, cv)
            if self.reducer is not None:
                if not getattr(self, "_buckets_configured", False):
                    # same bucketing as the GPU executor: per-layer flat ranges in backward
                    # order (last layer first), merged up to the reducer's bucket size
                    ranges = sorted(self.store.layer_ranges().values(), key=lambda r: -r[0])
                    self.reducer.configure(ranges)
                    self._buckets_configured = True
                self.reducer.reduce_all(self.store.grad)
            self._apply_update()
        self._accumulate(loss, corr, bs, penalty)
        self._roc_accumulate(z, y, w, data)

    def _penalty(self) -> float:
        return float(R.regularization_penalty(self.regs, self.store.master)) if self.regs else 0.0

    def _accumulate(self, loss, corr, bs, penalty=0.0):
        # (a batch of bs rows reports L_data + P: it adds bs * P to the epoch's loss sum)
        ls, cs = float(loss.sum()) + bs * penalty, float(corr.sum()) / self._acc_div
        self._acc += torch.tensor([ls, cs, bs], dtype=torch.float64)
        self._last = (ls / bs, cs / bs)

    def eval_step(self, data: DeviceData, pos: int, bs: int) -> None:
        x, y = data.x[pos:pos + bs], data.y[pos:pos + bs]
        w = data.w[pos:pos + bs] if data.w is not None else None
        with torch.no_grad():
            z, _, _ = self._forward(x, False, 0)
            loss, _, corr = self._head_loss(z, y, w)
        self._accumulate(loss, corr, bs, self._penalty())
        self._roc_accumulate(z, y, w, data)

    def _probs(self, z):
        act = self.plan.head.activation
        if act == "softmax":
            return torch.softmax(z, -1)
        if act == "sigmoid":
            return torch.sigmoid(z)
        return z

    def _roc_accumulate(self, z, y, w, data):
        """The batch's probabilities (what predict_step returns for these rows) into the ROC state."""
        if self._roc is None:
            return
        if w is not None and self.roc_weighted:
            self._roc.k = self.roc_shift(data)
            self._roc_w_seen = True
        else:
            w = None
        self._roc.accumulate(self._probs(z).numpy(), y.numpy(), None if w is None else w.numpy())

    def extra_metrics(self):
        from ..metrics import hist_auc, named_metrics
        st = self._roc
        aucs = [[hist_auc(st.pos[s, n], st.neg[s, n]) for n in range(st.N)] for s in range(2)]
        return named_metrics(st.softmax, aucs, st.tail, self._roc_w_seen)

    def predict_step(self, data: DeviceData, pos: int, bs: int) -> torch.Tensor:
        with torch.no_grad():
            z, _, _ = self._forward(data.x[pos:pos + bs], False, 0)
        return self._probs(z)

    def reset_metrics(self):
        self._acc.zero_()
        if self._roc is not None:
            self._roc.reset()
            self._roc_w_seen = False

    def read_metrics(self):
        ls, cs, n = self._acc.tolist()
        n = max(n, 1.0)
        return ls / n, cs / n, int(n)

    def last_batch_metrics(self):
        return self._last

    def m_schedule_value(self) -> float:
        return float(self.m_schedule)

    def set_m_schedule(self, v: float) -> None:
        self.m_schedule = float(v)

    def optimizer_state(self):
        return [s[:self.store.numel] for s in self.slots]

    def set_optimizer_state(self, iterations, slots):
        base = getattr(self.optimizer, "_base_optimizer", self.optimizer)
        base.iterations = int(iterations)
        for dst, src in zip(self.slots, slots):
            dst[:self.store.numel].copy_(torch.as_tensor(src).reshape(-1))

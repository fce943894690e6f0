"""HIP / gfx950 backend: executes a Plan with the hand-written CDNA4 kernels.

One training step is a fixed sequence of ~15-20 launches (SURVEY.md §2.7 "fused op
boundaries"), captured once per batch size into a HIP graph and replayed:

  prologue(gather + re-pack + bookkeeping) -> conv_mm(fwd) x C -> [dense split-K + epilogue] x D -> head
  -> [wgrad(dense) + conv_mm(dX, bwd-through)] x D -> [wgrad(conv) + conv_mm(dgrad,
  bwd-through)] x C -> slab_reduce (per DP bucket) -> [RCCL all-reduce] -> optim
  (a clipping optimizer: slab_reduce -> grad_sqnorm -> clipped optim on one GPU; data parallel
  slab_reduce -> grad_sqnorm -> grad_clip_apply -> RCCL all-reduce -> optim; a model with weight
  regularizers: slab_reduce -> weight_reg -> [grad_sqnorm ..] as above, and head -> weight_reg in
  an evaluation step; a stage with a hidden activation other than relu / linear: its linear
  forward kernels -> act_fwd, and the launch that stores its gradient -> act_bwd; a stage with a
  BatchNormalization: its linear forward kernels (un-pooled) -> bn_stats -> bn_apply_fwd [-> act_fwd],
  and the launch that stores its gradient [-> act_bwd] -> bn_bwd_reduce -> bn_bwd_apply -> its wgrad /
  dgrad in their un-pooled linear form; a conv stage with an AveragePooling2D: its conv kernel
  (un-pooled, relu in it) [-> act_fwd] -> pool_fwd, and the launch that stores its pooled gradient ->
  pool_bwd [-> act_bwd] -> its wgrad / dgrad in their un-pooled form; a global pooling layer: gpool_fwd
  behind the last conv stage, and the launch that stores its gradient -> gpool_bwd -> the last conv
  stage's own backward tail)

Activations are bf16 NHWC with channel strides padded to 8 (input: 4); weights live in
ONE fp32 master buffer (Keras layout) and are mirrored into bf16 fragment-major packs by
the optimizer kernel; gradients land in ONE flat fp32 buffer via deterministic slab
reductions.  Metrics accumulate on the device; the host syncs once per epoch.
"""
from __future__ import annotations

import gc
import os
from types import SimpleNamespace
from operator import attrgetter
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from ..ops.hip import kernels
from ..optim.optimizers import KIND_IDS, STANDALONE_KINDS, clip_pair, fill_clip_args, fill_kernel_args
from ..utils.env import env_flag
from ..utils.tune import tune
from .executor_base import DeviceData, Executor, prepare_targets
from .hip_geometry import GeometryMixin
from .plan import Plan, binary_accuracy_head, classic_head
from .step_program import (ConvGeo, DenseGeo, Exchange, GPoolGeo, Launch, RedDesc, RedGroup, Src,  # noqa: F401  (re-exported)
                           cdiv, check_bucket_cover, defer_after_readers, dropout_pair, gpool_geometry,
                           splice_bucket_launches, stage_geometry, stream_program)

# canonical loss name -> the loss-code constant of the kernels module (HeadArgs.loss, loss_head.hip)
LOSS_CODES = {"mse": "LOSS_MSE", "mae": "LOSS_MAE", "msle": "LOSS_MSLE", "logcosh": "LOSS_LOGCOSH",
              "hinge": "LOSS_HINGE", "squared_hinge": "LOSS_SQ_HINGE", "categorical_hinge": "LOSS_CAT_HINGE",
              "kld": "LOSS_KLD", "poisson": "LOSS_POISSON", "binary_crossentropy": "LOSS_BCE"}

BF16 = torch.bfloat16
# views of the optimizer-kind table (optim/optimizers.py KINDS); STANDALONE_KINDS: see
# HipExecutor.inline_update_ok
OPT_KIND = KIND_IDS
PACK_CONV_FWD, PACK_CONV_DGRAD, PACK_DENSE_FWD, PACK_DENSE_BWD = 0, 1, 2, 3
RED_CONVW, RED_BIAS, RED_FLATW = 0, 1, 2


class StageBufs(NamedTuple):
    """The buffers of one hidden stage in one BatchPlan (BatchPlan.stage_bufs)."""
    lin_out: torch.Tensor          # where the linear kernel / epilogue writes: ``out``, or a BatchNormalization's z,
    #                                or an average-pooled stage's un-pooled activation
    out: torch.Tensor              # the stage output
    code: Optional[torch.Tensor]   # the pooling argmax codes
    dout: Optional[torch.Tensor]   # the gradient wrt the stage output: what the next stage's BwdThrough
    #                                stores and act_bwd scales (training)
    dz: Optional[torch.Tensor]     # what the stage's own wgrad and dgrad read: ``dout``, or bn_bwd_apply's /
    #                                pool_bwd's un-pooled dz


class HipExecutor(Executor):
    def __init__(self, plan: Plan, store, optimizer, seed: int):
        super().__init__(plan, store, optimizer, seed)
        self.K = kernels()
        self.K.set_red_lanes(int(tune("red_lanes")))   # slab partials per reduction split-lane
        self.device = store.device
        if self.device.type != "cuda":
            raise RuntimeError("HipExecutor needs a GPU device")
        torch.cuda.set_device(self.device)
        self.use_graphs = env_flag("INTML_GRAPHS", True)
        self.state = torch.zeros(self.K.STEP_STATE_BYTES, dtype=torch.uint8, device=self.device)
        self._st_i32 = self.state.view(torch.int32)
        self._st_f32 = self.state.view(torch.float32)
        self._st_f64 = self.state.view(torch.float64)
        self._st_i64 = self.state.view(torch.int64)
        self._st_f64[self.K.STEP_STATE_MSCHED_OFFSET // 8] = 1.0
        base = getattr(optimizer, "_base_optimizer", optimizer)
        self.opt = base
        n_slots = getattr(base, "n_slots", 0)
        self.slots = [torch.zeros(store.capacity, dtype=torch.float32, device=self.device) for _ in range(n_slots)]
        # Keras gradient clipping (clipnorm over the global norm, then clipvalue), read HERE like the
        # other hyper-parameters except lr: the values go into kernel arguments of the captured
        # step, so a later change of optimizer.clipnorm / clipvalue takes a new compile().  A clipping
        # optimizer's step has the fuse_optim=0 structure whatever its kind -- every slab
        # reduction, the norm launch, then the clipped optimizer launch (whole_grad_first below).
        # The clip scalars (norm, factor, the norm kernel's ticket) live in a buffer of their own.
        self.clipnorm, self.clipvalue = clip_pair(base)
        self.clips = bool(self.clipnorm or self.clipvalue)
        self.clip_state = self.clip_partials = None
        if self.clips:
            K = self.K
            self.clip_state = torch.zeros(K.CLIP_STATE_WORDS, dtype=torch.float32, device=self.device)
            self.clip_state[K.CLIP_FACTOR] = 1.0
            self.clip_partials = torch.zeros(cdiv(store.numel + 3, K.CLIP_CHUNK) + 1, dtype=torch.float32,
                                             device=self.device)
        # Keras weight regularizers [(lo, hi, l1, l2)] over the flat store, read HERE like the clip
        # values (they go into kernel arguments of the captured step).  The term joins the whole
        # reduced gradient in ONE weight_reg launch (reg.hip) behind the last slab reduction and
        # ahead of the norm launch and the update.  reg_state[REG_PENALTY] is the last step's penalty P.
        self.regs = store.regularized_ranges()
        # The update gate, read by everything that could update before the step's end.
        # whole_grad_first: something must see the WHOLE reduced gradient before any update -- the
        # global norm of a clipping optimizer, the regularizers' term -- so the step is every slab
        # reduction, BatchPlan._whole_grad_launches, then the update: optim_fused = False, ONE
        # data-parallel bucket, RCCL plane only.
        # inline_update_ok: an update may run inside the backward -- the dual launch's early
        # reduction, the dense wgrad's fused update.  Not with whole_grad_first, and not for
        # STANDALONE_KINDS: kinds with instances of optim_kernel / reduce_optim_kernel only, while
        # the kernels that choose the optimizer at run time (those two, the xGMI exchange and
        # all-reduce kernels) stay five-way, so their data plane updates after the all-reduce.
        self.whole_grad_first = self.clips or bool(self.regs)
        self.inline_update_ok = not self.whole_grad_first and base.kind not in STANDALONE_KINDS
        self.reg_state = self.reg_partials = None
        if self.regs:
            K = self.K
            if len(self.regs) > K.MAX_REG_RANGES:
                raise ValueError("%d regularized weight tensors (layers %s): the regularizer kernel takes at most "
                                 "MAX_REG_RANGES = %d" % (len(self.regs), ", ".join(store.regularized_layers()),
                                                          K.MAX_REG_RANGES))
            self.reg_state = torch.zeros(K.REG_STATE_WORDS, dtype=torch.float32, device=self.device)
            self.reg_partials = torch.zeros(cdiv(store.numel + 3, K.REG_CHUNK) + 1, dtype=torch.float32,
                                            device=self.device)
        self._build_geometry()
        self._build_packs()
        self._plans: Dict[Tuple[int, str], "BatchPlan"] = {}
        self._lr_host = None
        self._expected_pos = None
        self._expected_eval_pos = None
        self._bound_data = None
        self._bound_ref = None
        self._bound_w = 0
        self._use_perm = None
        self._perm_obj = None
        self._perm_buf = None
        self._metrics_prev = (0.0, 0.0, 0.0)
        self.grad_scale = 1.0
        # the ROC state (args.h RocArgs; a buffer of its own, StepState's layout stays), its result
        # block and the bound data set's fixed-point shift: configure_metrics -> _init_roc
        self.roc_state = self.roc_res = None
        self._roc_k = 0
        self._roc_w_seen = False
        self.params_changed()

    # ------------------------------------------------------------------ ROC metrics
    def _init_roc(self):
        K, N = self.K, self.plan.head.N
        self.roc_state = torch.zeros(K.ROC_HDR + 2 * N * K.ROC_BLOCK, dtype=torch.int64, device=self.device)
        self.roc_state[1:2].view(torch.float64)[0] = 1.0       # 2^k, k = 0
        self.roc_res = torch.zeros(2 * N * K.ROC_RES_WORDS, dtype=torch.int64, device=self.device)
        self._plans.clear()

    def _roc_args(self):
        a = self.K.RocArgs()
        hd = self.plan.head
        a.N, a.softmax = hd.N, int(hd.activation == "softmax")
        a.state, a.res = self.roc_state.data_ptr(), self.roc_res.data_ptr()
        return a

    def _bind_roc(self, data: DeviceData):
        """The weighted set's shift k of the bound data set into the state's header: device memory,
        not a kernel argument, so captured graphs stay data-set independent (like data_w)."""
        if not (self.roc_weighted and data.w is not None):
            return
        self._roc_w_seen = True
        k = self.roc_shift(data)
        if k != self._roc_k:
            self.roc_state[0] = k
            self.roc_state[1:2].view(torch.float64)[0] = float(np.ldexp(1.0, k))
            self._roc_k = k

    def extra_metrics(self):
        from ..metrics import named_metrics
        K, N = self.K, self.plan.head.N
        K.roc_finish(self._roc_args(), torch.cuda.current_stream().cuda_stream)
        r = self.roc_res.cpu().numpy().reshape(2, N, K.ROC_RES_WORDS)
        aucs = r[:, :, 0].copy().view(np.float64)
        return named_metrics(self.plan.head.activation == "softmax", aucs.tolist(), r[:, :, 3:3 + K.ROC_TAIL],
                             self._roc_w_seen)

    def roc_histograms(self):
        """(pos, neg, tail) int64 numpy [2][N][...]: the whole ROC state (tests, curves)."""
        K, N = self.K, self.plan.head.N
        b = self.roc_state[K.ROC_HDR:].cpu().numpy().reshape(2, N, K.ROC_BLOCK)
        return b[:, :, :K.ROC_BINS], b[:, :, K.ROC_BINS:2 * K.ROC_BINS], b[:, :, 2 * K.ROC_BINS:]

    # ------------------------------------------------------------------ geometry
    def _build_geometry(self):
        inp, self.convs, self.denses, self.head_src, self.head_act = stage_geometry(self.plan)
        hd = self.plan.head
        # the second head kernel (loss_head.hip) runs every pair the first one does not; it reads
        # the last hidden stage's stored output, never a split-K epilogue
        self.loss_head = not classic_head(hd.activation, hd.loss, hd.N)
        self.acc_div = float(hd.N) if self.loss_head and hd.N > 1 and binary_accuracy_head(hd.loss, hd.N) else 1.0
        self.in_C, self.in_Cs, self.in_H, self.in_W = inp.C, inp.Cs, inp.H, inp.W
        # the global pooling stage behind the last conv stage (None: the model has none)
        self.gpool = gpool_geometry(self.plan, self.convs[-1].out_src) if self.convs else None

    def stage_of(self, src: Src):
        """The hidden stage whose output ``src`` describes (None: the model input)."""
        return {"input": [None], "conv": self.convs, "dense": self.denses, "gpool": [self.gpool]}[src.kind][src.idx]

    def _build_packs(self):
        K = self.K
        st = self.store
        self.pack_descs = []          # descriptor tuples, for per-bucket pack tables

        class _Tab:
            def __init__(self, outer):
                self.t, self.outer = K.PackTable(), outer

            def add(self, *d):
                self.t.add(*d)
                self.outer.pack_descs.append(d)

        tab = _Tab(self)
        off = 0

        def alloc(ks, nt):
            nonlocal off
            o = off
            off += ks * nt * 64 * 8
            return o

        for g, cs in zip(self.convs, self.plan.convs):
            sp = st.spec(cs.conv, "kernel")
            g.pack_fwd = alloc(g.KS, g.NT)
            tab.add(sp.offset, sp.numel, PACK_CONV_FWD, g.KH, g.KW, g.Cin, g.Cout, g.Cs_in, g.NT, g.pack_fwd)
            if g.i > 0:
                g.pack_dgrad = alloc(g.KSd, g.NTd)
                tab.add(sp.offset, sp.numel, PACK_CONV_DGRAD, g.KH, g.KW, g.Cin, g.Cout, g.Cs_out, g.NTd,
                        g.pack_dgrad)
        for g, ds in zip(self.denses, self.plan.denses):
            sp = st.spec(ds.dense, "kernel")
            g.pack_fwd = alloc(g.KS, g.NT)
            tab.add(sp.offset, sp.numel, PACK_DENSE_FWD, g.src.H, g.src.W, g.src.C, g.N, g.src.Cs, g.NT, g.pack_fwd)
            if g.KSb:
                g.pack_bwd = alloc(g.KSb, g.NTb)
                tab.add(sp.offset, sp.numel, PACK_DENSE_BWD, g.src.H, g.src.W, g.src.C, g.N, g.src.Cs, g.NTb, g.pack_bwd)
        self.pack_table = tab.t
        self.arena = torch.zeros(max(off, 8), dtype=BF16, device=self.device)
        # pack routes (PackRoute, args.h): the optimizer writes every updated weight's bf16
        # copies into these packs itself, so a training step needs no re-pack pass
        routes = []
        for g, cs in zip(self.convs, self.plan.convs):
            sp = st.spec(cs.conv, "kernel")
            bwd = g.pack_dgrad if g.i > 0 and g.Cs_out % 4 == 0 else -1
            routes.append((sp.offset, sp.offset + sp.numel, 1, g.KH * g.KW, g.Cin, g.Cout, g.Cs_in,
                           g.Cs_out if g.i > 0 else 0, g.NT, g.NTd if g.i > 0 else 0, g.pack_fwd, bwd))
        for g, ds in zip(self.denses, self.plan.denses):
            sp = st.spec(ds.dense, "kernel")
            routes.append((sp.offset, sp.offset + sp.numel, 2, g.src.H * g.src.W, g.src.C, g.N, g.src.Cs, 0,
                           g.NT, g.NTb if g.KSb else 0, g.pack_fwd, g.pack_bwd if g.KSb else -1))
        # (a dense layer whose optimizer runs inside its wgrad kernel writes its packs there
        # too -- WgradArgs.pk_fwd -- or is not fused: see BatchPlan._dense_wgrad)
        self.routes_ok = bool(routes) and len(routes) <= K.MAX_ROUTES and tune("opt_packs")
        self.routes = None
        self.route_list = routes
        if self.routes_ok:
            words = K.PACK_ROUTE_BYTES // 4
            arr = np.zeros(len(routes) * words, dtype=np.int32)
            a64 = arr.view(np.int64)
            for r, rt in enumerate(routes):
                arr[r * words:r * words + 10] = rt[:10]
                a64[r * words // 2 + 5] = rt[10]
                a64[r * words // 2 + 6] = rt[11]
            self.routes = torch.from_numpy(arr).to(self.device)

    # ------------------------------------------------------------------ params / optimizer
    def _clip_args(self):
        """ClipArgs over the whole flat gradient: the norm launch's and the in-place clip's."""
        c = self.K.ClipArgs()
        c.g = self.store.grad.data_ptr()
        c.n = self.store.numel
        c.clipnorm, c.clipvalue, c.use_norm = self.clipnorm, self.clipvalue, int(bool(self.clipnorm))
        c.partials, c.npartials = self.clip_partials.data_ptr(), self.clip_partials.numel()
        c.state = self.clip_state.data_ptr()
        return c

    def _reg_args(self, rows: int, add_grad: bool):
        """RegArgs of a step of ``rows`` rows: the gradient term (training) and the penalty."""
        r = self.K.RegArgs()
        r.p = self.store.master.data_ptr()
        r.g = self.store.grad.data_ptr()
        r.n = self.store.numel
        r.set_ranges([tuple(x) for x in self.regs])
        r.rows, r.add_grad = float(rows), int(add_grad)
        r.partials, r.npartials = self.reg_partials.data_ptr(), self.reg_partials.numel()
        r.st = self.state.data_ptr()
        r.state = self.reg_state.data_ptr()
        return r

    def _optim_args(self, pack_only: bool, defer_pack: bool = False, clip: bool = False):
        """clip: the clipped optimizer launch (single-GPU step of a clipping optimizer); every
        other user of these args -- the fused reductions, the data-parallel update behind the
        all-reduce of already clipped gradients -- leaves the clip fields off."""
        K = self.K
        a = K.OptimArgs()
        a.p = self.store.master.data_ptr()
        a.g = self.store.grad.data_ptr()
        if self.slots:
            a.s0 = self.slots[0].data_ptr()
        if len(self.slots) > 1:
            a.s1 = self.slots[1].data_ptr()
        if len(self.slots) > 2:
            a.s2 = self.slots[2].data_ptr()
        a.n = self.store.numel
        a.st = self.state.data_ptr()
        fill_kernel_args(self.opt, a)
        a.grad_scale = self.grad_scale
        a.pack_only = int(pack_only)
        a.defer_pack = int(defer_pack)
        a.arena = self.arena.data_ptr()
        if clip and self.clips:
            fill_clip_args(self.opt, a, self.clip_state.data_ptr())
        if self.routes is not None and not pack_only:
            a.routes = self.routes.data_ptr()
            a.nroutes = self.routes.numel() * 4 // K.PACK_ROUTE_BYTES
        return a

    def tile_routes(self, a):
        """optim_kernel launches: the dense routes wholly inside [a.lo, a.lo + a.n) (identity
        padding, N % 32 == 0, K % 8 == 0) are updated by 2-D tile blocks that write whole
        16-byte pack vectors (the flat blocks' scattered 2-byte pack stores cost the legacy
        model's 33.5M-weight dense layer ~190 us per update)."""
        if self.routes is None or not tune("opt_tiles"):
            return a
        span = a.lo + a.n - (a.lo & ~3)
        flat = cdiv(cdiv(span, 4), 256)
        b0 = i = 0
        for r, rt in enumerate(self.route_list):
            lo, hi, kind, _khw, cin, n, cs = rt[:7]
            k = (hi - lo) // n
            if (kind != 2 or cin != cs or n % 32 or k % 8 or lo % 4 or lo < a.lo or hi > a.lo + a.n
                    or i == 4 or rt[10] < 0):
                continue
            a.set_tile(i, r, b0)
            b0 += (k // 8) * cdiv(n, 128)
            i += 1
        if i:
            a.set_tile(i, 0, b0)
            a.ntile, a.flat_blocks = i, flat
        return a

    def params_changed(self):
        self.K.optim(self._optim_args(True), self.pack_table, torch.cuda.current_stream().cuda_stream)

    def optimizer_state(self):
        return [s[:self.store.numel] for s in self.slots]

    def set_optimizer_state(self, iterations, slots):
        self.opt.iterations = int(iterations)
        self._st_i32[0] = int(iterations)
        for dst, src in zip(self.slots, slots):
            dst[:self.store.numel].copy_(torch.as_tensor(src, device=self.device).reshape(-1))

    def m_schedule_value(self) -> float:
        return float(self._st_f64[self.K.STEP_STATE_MSCHED_OFFSET // 8])

    def set_m_schedule(self, v: float) -> None:
        self._st_f64[self.K.STEP_STATE_MSCHED_OFFSET // 8] = float(v)

    def set_lr_warmup(self, t0, steps, spe, size, epochs, base):
        super().set_lr_warmup(t0, steps, spe, size, epochs, base)
        w = self.lr_warmup or (0, 0, 1, 1, 1.0, 0.0)
        o = self.K.STEP_STATE_WARM_OFFSET
        self._st_i32[o // 4:o // 4 + 4] = torch.tensor(w[:4], dtype=torch.int32)
        # StepState order: warm_base, warm_epochs
        self._st_f32[o // 4 + 4:o // 4 + 6] = torch.tensor([w[5], w[4]], dtype=torch.float32)

    def _sync_lr(self):
        lr = float(self.opt.lr)
        if lr != self._lr_host:
            self._st_f32[self.K.STEP_STATE_LR_OFFSET // 4] = lr
            self._lr_host = lr

    # ------------------------------------------------------------------ data
    def upload(self, x, y, w=None):
        if x is None:
            return None
        x = np.asarray(x)
        if tuple(x.shape[1:]) != tuple(self.plan.input_shape):
            raise ValueError("input shape %s != model input %s" % (x.shape[1:], self.plan.input_shape))
        n = x.shape[0]
        xt = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32)).to(self.device, non_blocking=False)
        xt = xt.reshape(n, self.in_H, self.in_W, self.in_C)
        xs = torch.zeros(n, self.in_H, self.in_W, self.in_Cs, dtype=BF16, device=self.device)
        xs[..., :self.in_C] = xt.to(BF16)
        del xt
        yt = None
        if y is not None:
            yt = torch.as_tensor(prepare_targets(y, self.plan)).to(self.device)
        else:
            yt = torch.zeros(n, self.plan.head.N, dtype=torch.float32, device=self.device)
        wt = None
        if w is not None:
            wt = torch.as_tensor(np.ascontiguousarray(w, dtype=np.float32)).reshape(-1).to(self.device)
            if wt.shape[0] != n:
                raise ValueError("sample weights have %d entries for %d samples" % (wt.shape[0], n))
            if self.roc_weighted:
                from ..metrics import check_weights
                check_weights(w)
        return DeviceData(xs.reshape(n, -1), yt, n, wt)

    def _bind_data(self, data: DeviceData, perm: Optional[torch.Tensor]):
        K = self.K
        w_ptr = data.w.data_ptr() if data.w is not None else 0
        key = (id(data), data.x.data_ptr(), data.y.data_ptr(), w_ptr)
        if self._bound_data != key or self._bound_ref is not data:
            self._bound_ref = data     # keep alive: its id / memory must not be recycled while bound
            o = K.STEP_STATE_DATA_OFFSET // 8
            self._st_i64[o] = data.x.data_ptr()
            self._st_i64[o + 1] = data.y.data_ptr()
            on = K.STEP_STATE_DATAN_OFFSET // 4
            self._st_i32[on] = data.n
            self._st_i32[on + 1] = data.x.shape[1]
            self._st_i32[on + 2] = data.y.shape[1]
            # the weights' pointer is per-data-set state like x / y (0 = unweighted); which head
            # instance runs is the plan's (keyed on weighted data, _plan_for)
            if w_ptr != self._bound_w:
                self._st_i64[K.STEP_STATE_DATAW_OFFSET // 8] = w_ptr
                self._bound_w = w_ptr
            self._bound_data = key
            self._perm_obj = None
        if perm is not None and perm is not self._perm_obj:
            # (a DP rank's epoch slice of the sampler permutation is shorter than the data set)
            m = min(int(perm.numel()), data.n)
            if self._perm_buf is None or self._perm_buf.numel() < max(data.n, 1):
                self._perm_buf = torch.empty(max(data.n, 1), dtype=torch.int32, device=self.device)
            self._perm_buf[:m].copy_(perm[:m].to(device=self.device, dtype=torch.int32))
            self._st_i64[K.STEP_STATE_DATA_OFFSET // 8 + 2] = self._perm_buf.data_ptr()
            self._perm_obj = perm
        use = 1 if perm is not None else 0
        if use != self._use_perm:     # host->device writes only on change (each is a copy + sync point)
            self._st_i32[K.STEP_STATE_DATAN_OFFSET // 4 + 3] = use
            self._use_perm = use

    # ------------------------------------------------------------------ steps
    def _plan_for(self, bs: int, mode: str, weighted: bool = False) -> "BatchPlan":
        # weighted data runs a plan of its own (the weighted head instances, the weight gather):
        # a plan is never shared between weighted and unweighted data sets
        key = (bs, mode, "w") if weighted else (bs, mode)
        bp = self._plans.get(key)
        if bp is None:
            bp = BatchPlan(self, bs, mode, weighted)
            self._plans[key] = bp
        return bp

    def train_step(self, data, perm, pos, bs):
        self.train_steps(data, perm, pos, bs, 1)

    def train_steps(self, data, perm, pos, bs, k):
        """k consecutive full training steps over batches [pos, pos + k*bs) of ``perm``
        (one graph replay; the caller guarantees no host-side change between them)."""
        self._sync_lr()
        self._bind_data(data, perm)
        if self._expected_pos != pos:
            self._st_i32[1] = pos
        bp = self._plan_for(bs, "train", data.w is not None)
        if self.roc_on:
            self._bind_roc(data)
        bp.run(k)
        self._expected_pos = pos + k * bs
        self.opt.iterations += k

    def _set_eval_pos(self, pos, bs):
        if self._expected_eval_pos != pos:
            self._st_i32[3] = pos
        self._expected_eval_pos = pos + bs

    def eval_step(self, data, pos, bs):
        self._bind_data(data, None)
        self._set_eval_pos(pos, bs)
        if self.roc_on:
            self._bind_roc(data)
        self._plan_for(bs, "eval", data.w is not None).run()

    def predict_step(self, data, pos, bs):
        self._bind_data(data, None)
        self._set_eval_pos(pos, bs)
        bp = self._plan_for(bs, "predict")
        bp.run()
        out = bp.probs.clone()
        return out

    # ------------------------------------------------------------------ metrics
    def _metrics(self):
        # int64 fixed point (StepState::metric_slots [16][4]): loss in units of 2^-32, counts
        # exact; integer sums over the slots are order-independent
        o = self.K.STEP_STATE_METRICS_OFFSET // 8
        v = self.state.view(torch.int64)[o:o + 4 * self.K.STEP_STATE_METRIC_SLOTS].view(-1, 4).sum(0).tolist()
        # v[3] counts head workgroups whose loss was non-finite or out of fixed-point range:
        # the loss is then NaN (sticky until reset_metrics), never a finite garbage value
        # (v[1]: correct rows, or correct ELEMENTS of a multi-column binary_accuracy head -- the
        # loss head's integer count -- divided by the columns here so that cs / rows is the accuracy)
        return [v[0] / 4294967296.0 if v[3] == 0 else float("nan"), float(v[1]) / self.acc_div, float(v[2])]

    def reset_metrics(self):
        o = self.K.STEP_STATE_METRICS_OFFSET // 8
        self._st_f64[o:o + 4 * self.K.STEP_STATE_METRIC_SLOTS].zero_()
        self._metrics_prev = (0.0, 0.0, 0.0)
        if self.roc_on:
            self.roc_state[self.K.ROC_HDR:].zero_()
            self._roc_w_seen = False

    def read_metrics(self):
        ls, cs, n = self._metrics()
        self._metrics_prev = (ls, cs, n)
        n1 = max(n, 1.0)
        return ls / n1, cs / n1, int(n)

    def last_batch_metrics(self):
        ls, cs, n = self._metrics()
        pl, pc, pn = self._metrics_prev
        self._metrics_prev = (ls, cs, n)
        dn = max(n - pn, 1.0)
        return (ls - pl) / dn, (cs - pc) / dn   # NaN propagates once the flag is set

    def synchronize(self):
        torch.cuda.synchronize(self.device)


class BatchPlan(GeometryMixin):
    """Buffers + prepared kernel argument structs for one (batch size, mode); records the
    launch sequence and replays it from a HIP graph."""

    # the exchange plan's fields, readable on the plan under their names as well
    early_push, early_xchg, xchg_end, xchg_fin, bucket_xchg, pushed, exchanged = (
        property(attrgetter("xchg." + n)) for n in ("early_push", "early_xchg", "xchg_end", "xchg_fin",
                                                    "bucket_xchg", "pushed", "exchanged"))

    def __init__(self, ex: HipExecutor, bs: int, mode: str, weighted: bool = False):
        self.ex, self.bs, self.mode = ex, bs, mode
        self.weighted = bool(weighted) and mode != "predict"
        self.training = mode == "train"
        K = ex.K
        dev = ex.device
        self.graph = None
        self.multi_graphs: Dict[int, torch.cuda.CUDAGraph] = {}   # k -> graph of k steps
        self.dp_graphs = None
        # (a second compute stream for the weight gradients and a per-bucket early optimizer
        # stream were measured slower on one MI355X and removed: docs/ARCHITECTURE.md §6)
        self.optim_fused = False           # set by _assign_buckets
        self.early_red = {}                # dual launch name -> (RedTable, span, grad_only): _early_groups
        self.xchg = Exchange()             # the xGMI exchange plan of a data-parallel step
        self.launches: List[Launch] = []
        self.srcidx = None                 # prologue-free step: the dataset row of each image
        self.stack_args = None
        self.red_groups: List[RedGroup] = []   # per layer, in backward order
        self.pack_readers = []     # (launch name, param lo, hi): backward launches reading a layer's pack
        self.wgrad_slabs = []
        self.dense_fused_opt = []          # (WgradArgs, params) updated inside dense_wgrad
        self.bucket_tables, self.bucket_ready = [], []
        self.bucket_overflow = {}          # bucket -> further RedTables (more than MAX_RED descriptors)
        self._no_packs = K.PackTable()     # a comm-stream optimizer re-packs nothing
        self._ncu = self._zero16 = None    # hip_geometry: CU count, the DMA kernels' zero bytes
        # Native RCCL data plane: the bucket all-reduces are part of the launch sequence (on
        # their own comm stream) and captured with the rest of the step into ONE HIP graph.
        red = ex.reducer
        self.comm_in_graph = (self.training and red is not None and getattr(red, "capturable", False)
                              and red.active and tune("comm_capture"))
        # tune comm_fork=0: the captured all-reduces stay on the main stream (a linear graph:
        # no cross-queue edges, whose graph-launch cost is several us each, but no overlap)
        # (default: fork only when there is more than one bucket to overlap; set in _comm_launches)
        self.comm_fork = None
        self.comm_stream = None
        # ... and each bucket's optimizer update follows its all-reduce on the comm stream (the
        # 1/size average folded in), so the dense bucket's update overlaps the conv backward and
        # only the last bucket's (small) update is on the step's tail
        self.optim_on_comm = self.comm_in_graph and tune("dp_optim_on_comm")
        z = lambda *s, dt=BF16: torch.zeros(*s, dtype=dt, device=dev)
        self.xb = z(bs, ex.in_H * ex.in_W * ex.in_Cs)
        self.yb = z(bs, ex.plan.head.N, dt=torch.float32)
        self.wb = z(max(bs, 1), dt=torch.float32) if self.weighted else None   # gathered sample weights
        self.conv_out, self.conv_code, self.conv_dy = [], [], []
        # BatchNormalization stages: ('conv' | 'dense', index) -> z (the un-pooled pre-activation the
        # linear kernels store), dp (the gradient wrt the stage output, which the next stage's
        # BwdThrough stores), the statistics partials, the saved mean / invstd, the dbeta / dgamma
        # slabs and the BnArgs.  Such a stage's conv_dy / dense_dh is dz: un-pooled, what its wgrad
        # and dgrad read as the dY of a linear stage.  Read through stage_bufs
        self.bn: Dict[Tuple[str, int], SimpleNamespace] = {}
        # average-pooled conv stages: index -> lin (the un-pooled activation the conv kernel and
        # act_fwd store), dp (the pooled gradient the next stage's BwdThrough stores); conv_out is
        # the pooled output and conv_dy the un-pooled dz of pool_bwd.  The global pooling stage: its
        # output, its gradient and GlobalMaxPooling2D's first-maximum indices
        self.avg: Dict[int, SimpleNamespace] = {}
        self.gp = None
        for g in ex.convs:
            if g.avg:
                self.avg[g.i] = SimpleNamespace(lin=z(bs, g.Ho, g.Wo, g.Cs_out),
                                                dp=z(bs, g.Hp, g.Wp, g.Cs_out) if self.training else None)
            self.conv_out.append(z(bs, g.Hp, g.Wp, g.Cs_out))
            self.conv_code.append(z(bs, g.Hp, g.Wp, g.Cs_out, dt=torch.uint8) if g.pool else None)
            # gradient wrt the stage OUTPUT resolution (pooled dP for pooled convs; the
            # full-resolution dY is rebuilt on load from dP + codes, never stored)
            self.conv_dy.append(z(bs, g.linear.Hp, g.linear.Wp, g.Cs_out) if self.training else None)
            if g.bn is not None:
                self.bn["conv", g.i] = self._bn_buffers(z, bs * g.Ho * g.Wo, (bs, g.Ho, g.Wo, g.Cs_out),
                                                        (bs, g.Hp, g.Wp, g.Cs_out))
        if ex.gpool is not None:
            g = ex.gpool
            self.gp = SimpleNamespace(out=z(bs, g.Cs), dout=z(bs, g.Cs) if self.training else None,
                                      idx=(z(bs, g.Cs, dt=torch.int32)
                                           if self.training and g.mode == "max" else None))
        self.dense_out, self.dense_part, self.dense_dh = [], [], []
        self.dense_splits = []
        for g in ex.denses:
            self.dense_out.append(z(bs, g.Ns))
            if K.dense_big(g.NT, g.KS):
                # large weights: ~256 workgroups (one per CU) of >= 8 k-steps; each owns
                # 128 rows x 8 n-tiles, so every weight byte streams from HBM once
                splits = max(1, min(cdiv(tune("dense_big_wgs"), K.dense_groups(bs, g.NT, g.KS)),
                                    cdiv(g.KS, tune("dense_big_minks"))))
            else:
                # ~2048 16x16-tile waves: latency-bound small layers want parallelism
                splits = max(1, min(g.KS, tune("dense_waves") // max(1, K.dense_groups(bs, g.NT, g.KS))))
            kps = cdiv(g.KS, splits)
            splits = cdiv(g.KS, kps)
            self.dense_splits.append((splits, kps))
            self.dense_part.append(z(splits, bs, g.NT * 16, dt=torch.float32))
            self.dense_dh.append(z(bs, g.Ns) if self.training else None)
            if g.bn is not None:
                self.bn["dense", g.j] = self._bn_buffers(z, bs, (bs, g.Ns), (bs, g.Ns))
        # Stage.kind -> its (output, pooling code, gradient) lists, for stage_bufs
        self._stage_lists = {"conv": (self.conv_out, self.conv_code, self.conv_dy),
                             "dense": (self.dense_out, [None] * len(ex.denses), self.dense_dh)}
        hd = ex.plan.head
        self.head_blocks = cdiv(bs, K.head_rows_per_block(False))   # re-set below if the head fuses the epilogue
        head_slab_blocks = cdiv(bs, K.head_rows_per_block(True))
        # (a plan with a ROC metric: roc_accum reads the head's probabilities in train and eval mode too)
        self.roc = ex.roc_on and mode != "predict"
        self.probs = z(bs, hd.N, dt=torch.float32) if mode == "predict" or self.roc else None
        if self.training:
            self.head_wslab = z(head_slab_blocks, hd.K, hd.N, dt=torch.float32)
            self.head_bslab = z(head_slab_blocks, hd.N, dt=torch.float32)
        self._build_args()

    # ---------------------------------------------------------------- helpers
    def _bn_buffers(self, z, rows, z_shape, out_shape):
        """The buffers of one BatchNormalization stage over ``rows`` rows (bn_plan's chunking)."""
        Cs = z_shape[-1]
        chunk, nchunks, gp_log2 = self.ex.K.bn_plan(max(rows, 1), Cs)
        f32 = torch.float32
        return SimpleNamespace(z=z(*z_shape), dp=z(*out_shape) if self.training else None,
                               part=z(2, nchunks, Cs, dt=f32), saved=z(2, Cs, dt=f32),
                               slab=None,
                               plan=(chunk, nchunks, gp_log2), args=None)

    def stage_bufs(self, g) -> StageBufs:
        """Which buffer holds what for hidden stage ``g`` (a ConvGeo / DenseGeo)."""
        if g.kind == "gpool":
            return StageBufs(self.gp.out, self.gp.out, None, self.gp.dout, self.gp.dout)
        out, code, dz = (lst[g.idx] for lst in self._stage_lists[g.kind])
        if g.avg:
            av = self.avg[g.idx]
            return StageBufs(av.lin, out, None, av.dp, dz)
        b = self.bn.get((g.kind, g.idx))
        return StageBufs(out, out, code, dz, dz) if b is None else StageBufs(b.z, out, code, b.dp, dz)

    def _bn_args(self, g):
        """The BnArgs of stage g: one struct for the stage's four launches."""
        ex, K, store = self.ex, self.ex.K, self.ex.store
        b, bufs = self.bn[g.kind, g.idx], self.stage_bufs(g)
        if b.args is not None:
            return b.args
        a = K.BnArgs()
        bn = g.bn
        a.z = bufs.lin_out.data_ptr()
        (a.Ho, a.Wo), (a.Hp, a.Wp) = g.lin_grid, g.out_grid
        a.B, a.rows, a.C, a.Cs, a.pool = self.bs, self.bs * a.Ho * a.Wo, g.C, g.Cs, int(g.pool)
        a.chunk, a.nchunks, a.gp_log2 = b.plan
        a.part, a.saved = b.part.data_ptr(), b.saved.data_ptr()
        if bn.scale:
            a.gamma = store.view(bn, "gamma").data_ptr()
        if bn.center:
            a.beta = store.view(bn, "beta").data_ptr()
        a.moving_mean = store.view(bn, "moving_mean").data_ptr()
        a.moving_var = store.view(bn, "moving_variance").data_ptr()
        m = a.rows
        a.eps, a.momentum = bn.epsilon, bn.momentum
        a.unbias = m / (m - (1.0 + bn.epsilon))     # Keras 2.2.4's sample-variance factor
        a.training, a.relu = int(self.training), int(g.relu)
        a.out = bufs.out.data_ptr()
        if bufs.code is not None:
            a.code = bufs.code.data_ptr()
        if self.training and g.dropout_in == "bn":
            a.drop_thr, a.drop_scale = dropout_pair(g.rate)
        a.seed, a.stream_id, a.st = ex.seed, g.stream, ex.state.data_ptr()
        if self.training:
            # the chunk slabs: [nchunks][dgamma[C], dbeta[C]]
            b.slab = torch.zeros(b.plan[1], 2, a.C, dtype=torch.float32, device=ex.device)
            a.dp, a.slab, a.dz = bufs.dout.data_ptr(), b.slab.data_ptr(), bufs.dz.data_ptr()
        b.args = a
        return a

    def _bn_descs(self, g):
        """(RedDescs, specs) of stage g's gamma / beta: the bn_bwd_reduce slabs [chunk][dgamma, dbeta]
        as ONE bias-like reduction over gamma and beta, which are adjacent in the store (or over the
        one of them the layer has)."""
        if g.bn is None:
            return [], []
        store = self.ex.store
        b = self.bn[g.kind, g.idx]
        _, nchunks, _ = b.plan
        C = b.slab.shape[-1]
        specs = [store.spec(g.bn, short) for short in ("gamma", "beta") if store.has(g.bn, short)]
        if not specs:
            return [], []
        if len(specs) == 2 and specs[0].offset + C != specs[1].offset:
            raise AssertionError("gamma and beta of %s are not adjacent in the parameter store" % g.bn.name)
        first = b.slab[0, 0 if specs[0].short == "gamma" else 1]
        return [RedDesc(first.data_ptr(), 2 * C, nchunks, 2 * C, specs[0].offset, C * len(specs), RED_BIAS)], specs

    def step_inputs(self):
        """(x [bs, R] bf16, y [bs, C] fp32) of this plan's last step: the gathered batch
        buffers, or -- prologue-free step -- the dataset rows the conv stack recorded."""
        if self.srcidx is None:
            return self.xb, self.yb
        d = self.ex._bound_ref
        idx = self.srcidx.long()
        return d.x[idx], d.y[idx]

    def _src_buf(self, src: Src):
        g = self.ex.stage_of(src)
        return self.xb if g is None else self.stage_bufs(g).out

    def _bt_for(self, src: Src):
        """BwdThrough args routing a gradient wrt ``src``'s output back into its layer."""
        K, ex = self.ex.K, self.ex
        g = ex.stage_of(src)
        if g is None:
            return None
        bufs = self.stage_bufs(g)
        bt = K.BwdThrough()
        bt.prev_out = bufs.out.data_ptr()
        if bufs.code is not None:
            bt.prev_code = bufs.code.data_ptr()
        # (an average-pooled stage: no mask from the pooled output -- pool_bwd takes the relu mask
        # from the un-pooled activation)
        bt.prev_relu, bt.prev_pool = int(g.relu and not g.avg), int(g.pool)
        (bt.pH, bt.pW), bt.pC, bt.pCs = g.out_grid, g.C, g.Cs
        bt.cH, bt.cW = g.lin_grid
        bt.dy = bufs.dout.data_ptr()
        if g.rate > 0:
            bt.drop_thr, bt.drop_scale = dropout_pair(g.rate)
        bt.seed, bt.stream_id = ex.seed, g.stream
        # write-through gradient stores (16-byte sc1; byte offsets < 2 GB)
        bt.wt = int(bool(int(tune("wt")) & 2) and bufs.dout.numel() * 2 < (1 << 31))
        return bt

    # ---------------------------------------------------------------- step program: forward
    def _add(self, name, fn, tag="main", **args):
        self.launches.append(Launch(name, fn, tag, args))

    def _act_args(self, g, bwd):
        """ActArgs of stage g with a hidden activation: the forward launch (in place on the stage
        output, with the stage's dropout in a training step) or the backward launch (in place on
        the stage's gradient buffer, reading the saved output)."""
        ex, K, bufs = self.ex, self.ex.K, self.stage_bufs(g)
        a = K.ActArgs()
        Hp, Wp = g.out_grid
        a.rows, a.C, a.Cs = self.bs * Hp * Wp, g.C, g.Cs
        a.act, a.alpha = K.ACT_CODES[g.act], g.act_alpha
        if g.avg:
            # an average-pooled stage: A at un-pooled resolution, in place on the un-pooled activation
            # (no dropout: pool_fwd carries it) and on dz (the saved activation is not dropout-scaled)
            Ho, Wo = g.lin_grid
            a.rows = self.bs * Ho * Wo
            if bwd:
                a.x, a.y = bufs.dz.data_ptr(), bufs.lin_out.data_ptr()
            else:
                a.x = bufs.lin_out.data_ptr()
                a.seed, a.stream_id, a.st = ex.seed, g.stream, ex.state.data_ptr()
        elif bwd:
            a.x, a.y = bufs.dout.data_ptr(), bufs.out.data_ptr()
            if g.rate > 0:       # the saved output carries the dropout scale: undo it (fp32(1 - rate))
                a.y_scale = float(np.float32(1.0 - g.rate))
        else:
            a.x = bufs.out.data_ptr()
            if self.training and g.dropout_in == "act":
                a.drop_thr, a.drop_scale = dropout_pair(g.rate)
            a.seed, a.stream_id, a.st = ex.seed, g.stream, ex.state.data_ptr()
        return a

    def _add_stage_tail_fwd(self, g):
        """Behind stage g's linear kernels, as the stage has them: bn_stats (training) ->
        bn_apply_fwd -> act_fwd (A and, unless an earlier launch carried it, the stage's dropout,
        in place) -> pool_fwd (an average-pooled stage: the average and the stage's dropout)."""
        K = self.ex.K
        if g.bn is not None:
            a = self._bn_args(g)
            if self.training:
                self._add("bn_stats_" + g.tag, lambda s, a=a: K.bn_stats(a, s), bn=a)
            self._add("bn_apply_fwd_" + g.tag, lambda s, a=a: K.bn_apply_fwd(a, s), bn=a)
        if g.act is not None:
            fa = self._act_args(g, False)
            self._add("act_fwd_" + g.tag, lambda s, a=fa: K.act_fwd(a, s), act=fa)
        if g.avg:
            self.avg[g.idx].args = pa = self._pool_args(g)
            self._add("pool_fwd_" + g.tag, lambda s, a=pa: K.pool_fwd(a, s), pool=pa)

    def _pool_args(self, g):
        """The PoolArgs of average-pooled conv stage g or of the global pooling stage: one struct for
        the stage's forward and backward launch."""
        ex, K, bufs = self.ex, self.ex.K, self.stage_bufs(g)
        a = K.PoolArgs()
        a.B, a.C, a.Cs = self.bs, g.C, g.Cs
        if g.kind == "gpool":
            feed = self.stage_bufs(ex.stage_of(g.src))
            a.mode = K.POOL_GAVG if g.mode == "avg" else K.POOL_GMAX
            a.H, a.W = g.src.H, g.src.W
            a.x = feed.out.data_ptr()
            if self.gp.idx is not None:
                a.idx = self.gp.idx.data_ptr()
        else:
            a.mode = K.POOL_AVG2
            a.H, a.W = g.lin_grid
            a.x = bufs.lin_out.data_ptr()
        a.out = bufs.out.data_ptr()
        if self.training and g.rate > 0:
            a.drop_thr, a.drop_scale = dropout_pair(g.rate)
        a.seed, a.stream_id, a.st = ex.seed, g.stream, ex.state.data_ptr()
        if self.training:
            a.dp = bufs.dout.data_ptr()
            if g.kind == "gpool":
                a.bt = self._bt_for(g.src)
            else:
                a.dz, a.lin, a.relu = bufs.dz.data_ptr(), bufs.lin_out.data_ptr(), int(g.relu)
        return a

    def _build_gpool_fwd(self):
        """gpool_fwd behind the last conv stage: the global pooling stage and its dropout."""
        g, K = self.ex.gpool, self.ex.K
        if g is None:
            return
        self.gp.args = pa = self._pool_args(g)
        self._add("gpool_fwd", lambda s, a=pa: K.pool_fwd(a, s), pool=pa)

    def _add_stage_tail_bwd(self, g):
        """Behind the launch that stored the gradient wrt stage g's output (None: the model input)
        through its BwdThrough (dropout mask applied, prev_relu = 0): gpool_bwd of the global pooling
        stage, then the tail of the conv stage that feeds it; pool_bwd of an average-pooled stage (the
        un-pooled dz from the pooled gradient); act_bwd, the multiplication by
        A' of a stage with a hidden activation, before anything reads that gradient buffer; and for
        a stage with a BatchNormalization bn_bwd_reduce -> bn_bwd_apply (the dbeta / dgamma slabs,
        and the dense dz the stage's wgrad / dgrad read)."""
        if g is None:
            return
        K = self.ex.K
        if g.kind == "gpool":
            # the global stage's gradient goes through the last conv stage's BwdThrough over its
            # whole output grid; that stage's own tail follows
            pa = self.gp.args
            self._add("gpool_bwd", lambda s, a=pa: K.pool_bwd(a, s), pool=pa)
            return self._add_stage_tail_bwd(self.ex.stage_of(g.src))
        if g.avg:
            pa = self.avg[g.idx].args
            self._add("pool_bwd_" + g.tag, lambda s, a=pa: K.pool_bwd(a, s), pool=pa)
        if g.act is not None:
            a = self._act_args(g, True)
            self._add("act_bwd_" + g.tag, lambda s, a=a: K.act_bwd(a, s), act=a)
        if g.bn is not None:
            b = self._bn_args(g)
            self._add("bn_bwd_reduce_" + g.tag, lambda s, a=b: K.bn_bwd_reduce(a, s), bn=b)
            self._add("bn_bwd_apply_" + g.tag, lambda s, a=b: K.bn_bwd_apply(a, s), bn=b)

    def _build_args(self):
        """The step program, stage by stage; each stage appends its launches."""
        ex = self.ex
        stack, sb = self._build_prologue()
        self._build_conv_fwd(stack)
        self._build_gpool_fwd()
        head_epi = self._build_dense_fwd(sb)
        self._build_head(head_epi)
        if not self.training:
            if self.mode == "eval" and ex.regs:
                # an evaluation batch reports L_data + P too: the penalty only, after the head
                ra = ex._reg_args(self.bs, False)
                self._add("weight_reg", lambda s, a=ra: ex.K.weight_reg(a, s), reg=ra)
            return
        self._begin_backward()
        for g, ds in reversed(list(zip(ex.denses, ex.plan.denses))):
            self._build_dense_bwd(g, ds)
        for g, cs in reversed(list(zip(ex.convs, ex.plan.convs))):
            self._build_conv_bwd(g, cs)
        self._build_reduce()

    def _build_prologue(self):
        """The prologue launch (gather + re-pack + bookkeeping), unless the step is prologue-free.
        Returns (the conv stack's args or None, the StepBeginArgs)."""
        ex, K, bs, training = self.ex, self.ex.K, self.bs, self.training
        st_ptr = ex.state.data_ptr()
        # step begin
        sb = K.StepBeginArgs()
        sb.st = st_ptr
        sb.training = int(training)
        sb.bs = bs
        fill_kernel_args(ex.opt, sb, "opt_kind")
        ga = K.GatherArgs()
        ga.st = st_ptr
        ga.bs = bs
        ga.R = self.xb.shape[1]
        ga.xb = self.xb.data_ptr()
        ga.yb = self.yb.data_ptr()
        if self.weighted:
            ga.wb = self.wb.data_ptr()
        # one prologue launch: gather + the previous update's weight re-pack (training: always,
        # except with per-bucket optimizers that pack themselves; eval/predict: only if an
        # optimizer ran since the last pack) + the step bookkeeping
        # (a conv stage with a hidden activation other than relu / linear: the per-layer structure
        # of conv_stack=0, each such layer's linear kernel followed by its act_fwd launch)
        # (a conv stage with a BatchNormalization likewise: its linear kernel stores the un-pooled
        # pre-activation for the bn.hip launches)
        # (an average-pooled stage or a global pooling layer likewise: the pool.hip launches sit
        # between the per-layer kernels)
        stack = (self._conv_stack_args(training)
                 if tune("conv_stack") and all(g.plain for g in ex.convs) and ex.gpool is None else None)
        # Prologue-free step (conv stack + a hidden dense layer + optimizer-written packs): the
        # stack reads its images straight from the dataset through the cursor and permutation
        # (recording each image's dataset row for the first layer's wgrad and the head's
        # targets), the optimizer keeps the bf16 packs current, and the first dense launch runs
        # the step bookkeeping -- the step has no prologue launch
        self.pro_free = bool(stack is not None and ex.denses and ex.routes_ok and tune("pro_free"))
        if self.pro_free:
            self.srcidx = torch.zeros(max(bs, 1), dtype=torch.int32, device=ex.device)
            stack.from_data, stack.training, stack.step_inc = 1, int(training), int(training)
            stack.srcidx = self.srcidx.data_ptr()
        pa = K.PrologueArgs()
        pa.sb, pa.ga = sb, ga
        pa.gather_gx = 1 if ga.skip_x else K.gather_gx(ga.R)
        pa.gather_blocks = pa.gather_gx * bs
        pa.pack_mode = 1 if training else 2
        pro_dbg = tune("pro_dbg")          # timing ablation only: 1 no re-pack, 2 no gather
        if pro_dbg == 1:
            pa.pack_mode = 0
        elif pro_dbg == 2:
            pa.gather_blocks = 0
        pa.master = ex.store.master.data_ptr()
        pa.arena = ex.arena.data_ptr()
        if training and ex.routes_ok:
            pa.pack_mode = 0          # the optimizer writes the packs itself (pack routes)
        if not self.pro_free:
            self._add("prologue", lambda s, a=pa: K.prologue(a, ex.pack_table, s), pro=pa)
        return stack, sb

    def _build_conv_fwd(self, stack):
        """The forward convs: the layer-fused stack launch, or one launch per layer."""
        ex, K = self.ex, self.ex.K
        if stack is not None:
            self.stack_args = stack
            self._add("conv_stack_fwd", lambda s, a=stack: K.conv_stack_fwd(a, s), stack=stack)
            return
        x_buf = self.xb
        for g, cs in zip(ex.convs, ex.plan.convs):
            a = K.ConvMMArgs()
            a.x = x_buf.data_ptr()
            a.B, a.H, a.W, a.Cs_in = self.bs, g.H, g.W, g.Cs_in
            a.Ho, a.Wo = g.Ho, g.Wo
            a.KH, a.KW, a.stride, a.pad_t, a.pad_l, a.in_dil = g.KH, g.KW, g.stride, g.pad_t, g.pad_l, 1
            a.KS = g.KS
            a.wpk = ex.arena.data_ptr() + 2 * g.pack_fwd
            a.NT = g.NT
            a.bias = ex.store.view(cs.conv, "bias").data_ptr() if cs.conv.use_bias else 0
            a.N = g.Cout
            a.mode = 0
            # (a BatchNormalization stage in its linear, un-pooled form: z for the bn.hip launches)
            lin, bufs = g.linear, self.stage_bufs(g)
            a.relu, a.pool = int(lin.relu), int(lin.pool)
            a.out = bufs.lin_out.data_ptr()
            a.Cs_out, a.Hp, a.Wp = g.Cs_out, lin.Hp, lin.Wp
            if lin.pool:
                a.code = bufs.code.data_ptr()
            if self.training and g.dropout_in == "linear":
                a.drop_thr, a.drop_scale = dropout_pair(g.rate)
            a.seed, a.stream_id, a.st = ex.seed, g.stream, ex.state.data_ptr()
            self._add("conv_fwd%d" % g.i, self._conv_launch(a, g.NT, lin.pool), ca=a)
            self._add_stage_tail_fwd(g)
            x_buf = bufs.out

    def _build_dense_fwd(self, sb):
        """The hidden dense layers: split-K GEMM + epilogue each.  Returns the last layer's
        epilogue args when the head launch runs that epilogue itself, else None."""
        ex, K, bs = self.ex, self.ex.K, self.bs
        head_epi = None
        for g, ds in zip(ex.denses, ex.plan.denses):
            splits, kps = self.dense_splits[g.j]
            a = K.DenseFwdArgs()
            a.x = self._src_buf(g.src).data_ptr()
            a.M, a.Ks = bs, g.src.width
            a.wpk = ex.arena.data_ptr() + 2 * g.pack_fwd
            a.NT, a.KS = g.NT, g.KS
            a.splits, a.ks_per_split = splits, kps
            a.part = self.dense_part[g.j].data_ptr()
            if self.pro_free and g.j == 0 and self.training:
                a.book, a.sb = 1, sb      # this step's bookkeeping (the stack read t + 1)
            self._add("dense_fwd%d" % g.j, lambda s, a=a: K.dense_fwd(a, s), da=a)
            e = K.DenseEpiArgs()
            e.part = a.part
            e.splits, e.M, e.N, e.Ns, e.ldp = splits, bs, g.N, g.Ns, g.NT * 16
            e.bias = ex.store.view(ds.dense, "bias").data_ptr() if ds.dense.use_bias else 0
            e.relu = int(g.relu and g.bn is None)      # (a BatchNormalization stage: the linear z)
            e.out = self.stage_bufs(g).lin_out.data_ptr()
            if self.training and g.dropout_in == "linear":
                e.drop_thr, e.drop_scale = dropout_pair(g.rate)
            e.seed, e.stream_id, e.st = ex.seed, g.stream, ex.state.data_ptr()
            if (g.j == len(ex.denses) - 1 and ex.head_src.kind == "dense" and g.Ns <= K.head_epi_max()
                    and tune("fuse_head") and g.plain and not ex.loss_head):
                # the head launch (one row per workgroup, the row's split groups in parallel)
                # reduces this layer's partials itself: one kernel boundary fewer
                head_epi = e
                self.head_blocks = cdiv(bs, K.head_rows_per_block(True))
            else:
                self._add("dense_epi%d" % g.j, lambda s, e=e: K.dense_epi(e, s), epi=e)
            self._add_stage_tail_fwd(g)      # (behind the epilogue, never the head's: fuse_head=0 structure)
        return head_epi

    def _build_head(self, head_epi):
        ex, K, store, training = self.ex, self.ex.K, self.ex.store, self.training
        hd = ex.plan.head
        h = K.HeadArgs()
        src = ex.head_src
        h.h = self._src_buf(src).data_ptr()
        h.M, h.K, h.Ks, h.N = self.bs, hd.K, src.width, hd.N
        h.flat_C, h.flat_Cs = src.C, src.Cs
        h.w = store.view(hd.dense, "kernel").data_ptr()
        h.bias = store.view(hd.dense, "bias").data_ptr() if hd.dense.use_bias else 0
        h.y = self.yb.data_ptr() if self.mode != "predict" else 0
        if self.pro_free and h.y:
            h.yidx = self.srcidx.data_ptr()      # targets straight from the dataset rows
        if self.weighted and h.y:
            # the weighted head instances; the rows' weights from the gathered batch, or with
            # yidx from the bound data set's weights (StepState::data_w) like the targets
            h.wb = self.wb.data_ptr()
        h.act = ex.head_act
        if head_epi is not None:
            h.epi = head_epi
        h.training = int(training)
        h.generic = int(tune("head_generic"))
        h.inv_bs = 1.0 / self.bs
        h.st = ex.state.data_ptr()
        if self.probs is not None:
            h.probs = self.probs.data_ptr()
        if training:
            h.wslab = self.head_wslab.data_ptr()
            h.bslab = self.head_bslab.data_ptr()
            bt = self._bt_for(src)
            if bt is not None:
                h.bt = bt
        # (a fused dense layer + head launch -- 16-wave K-slice tiles, the last arriving workgroup
        # of each row group running the head -- measured 15.6 us against 13.3 us for the split-K
        # dense launch + this head launch at RPV B=128, and was removed in round 5)
        if ex.loss_head:
            h.loss = getattr(K, LOSS_CODES[hd.loss])
            self._add("loss_head", lambda s, a=h: K.loss_head(a, s), head=h)
        else:
            self._add("head", lambda s, a=h: K.head(a, s), head=h)
        if self.roc:
            # directly behind the head, on the main stream, inside the captured step
            r = ex._roc_args()
            r.probs, r.M = self.probs.data_ptr(), self.bs
            r.y, r.st = self.yb.data_ptr(), ex.state.data_ptr()
            if self.pro_free:
                r.yidx = self.srcidx.data_ptr()
            if self.weighted and ex.roc_weighted:
                r.wb, r.weighted = self.wb.data_ptr(), 1
            self._add("roc_accum", lambda s, a=r: K.roc_accum(a, s), roc=r)

    # ---------------------------------------------------------------- step program: backward
    def _add_group(self, spec, descs, bias_spec=None, more=()):
        """A layer's reduction group over its kernel (and bias, and its BatchNormalization's gamma /
        beta: ``more``) span, its partial slabs final after the launches appended so far."""
        lo, hi = spec.offset, spec.offset + spec.numel
        for sp in ([bias_spec] if bias_spec is not None else []) + list(more):
            hi = max(hi, sp.offset + sp.numel)
        self.red_groups.append(RedGroup(lo, hi, descs, len(self.launches)))
        return lo, hi

    def _begin_backward(self):
        """The head's reduction group (its slabs are final after the head launch) and the
        fused-dense-optimizer switches."""
        ex, store, hd = self.ex, self.ex.store, self.ex.plan.head
        hw = store.spec(hd.dense, "kernel")
        hb = store.spec(hd.dense, "bias") if hd.dense.use_bias else None
        descs = [RedDesc(self.head_wslab.data_ptr(), hd.K * hd.N, self.head_blocks, hd.N, hw.offset, hw.numel,
                         RED_BIAS)]
        if hb is not None:
            descs.append(RedDesc(self.head_bslab.data_ptr(), hd.N, self.head_blocks, hd.N, hb.offset, hb.numel,
                                 RED_BIAS))
        self._add_group(hw, descs, hb)
        # (the head stored the last hidden stage's gradient)
        self._add_stage_tail_bwd(ex.stage_of(ex.head_src))
        # opt-in: the dense layer's optimizer update inside its (one-split) wgrad kernel.  Measured
        # slower on RPV at batch 128: the 128 wgrad workgroups move the layer's 14 MB of optimizer
        # state at per-CU bandwidth (wgrad 6.1 -> 9.7 us) while the end-of-step reduction, which
        # spreads it over thousands of workgroups, only drops 10.8 -> 8.2 us
        # dense_opt: "auto" (default) = only layers whose gradient is written in place (> 16 MB,
        # the legacy model's 33.5M-weight Dense(512)): their update moves ~1 GB either way, and
        # fusing it saves the gradient's own write + re-read (legacy 1.269 -> 1.238 ms/step,
        # profiles/r4c_ab_legacy.txt); "1" = every one-split layer; "0" = off
        dense_opt = str(tune("dense_opt")).lower()
        self.dense_opt_ok = (ex.reducer is None and tune("fuse_optim")
                             and dense_opt not in ("0", "false", "off", "no") and ex.inline_update_ok)
        self.dense_opt_all = dense_opt in ("1", "true", "on", "yes")

    def _dense_wgrad(self, g, ds, direct):
        """A dense layer's weight gradient: (Wgrad, launch callable, whether the optimizer
        update is fused into it, whether the dense_bwd.hip kernels run it)."""
        ex, K, store = self.ex, self.ex.K, self.ex.store
        xin = self._src_buf(g.src)
        sp = store.spec(ds.dense, "kernel")
        direct_ptr = (store.grad.data_ptr() + 4 * sp.offset) if direct else None
        # dense_bwd.hip kernels (per-wave pipelined wgrad, vectorised dX epilogue) where the
        # 8-element alignment they assume holds; the generic wgrad / split-K path otherwise
        bwd2 = tune("dense_bwd2") and g.src.width % 8 == 0 and g.Ns % 8 == 0
        if not bwd2:
            w = self._wgrad_args(xin, g.src.width, self.dense_dh[g.j], g.Ns, g.N, ds.dense.use_bias, direct_ptr)
            return w, (lambda s, a=w.a, c=w.cfg: K.wgrad(a, *c, s)), False, False
        w = self._dense_wgrad_args(xin, g.src.width, self.dense_dh[g.j], g.Ns, g.N, ds.dense.use_bias, direct_ptr)
        wa, (kg, ntt) = w.a, w.tiles
        # one split + identity layout: the kernel's fixed-order sum IS the Keras
        # gradient -- write it in place and apply the optimizer there (single GPU,
        # fused-optimizer step), so the layer skips the end-of-step reduction
        # (a BatchNormalization stage's group also holds gamma / beta, which the kernel does not update)
        fused_opt = (self.dense_opt_ok and (self.dense_opt_all or direct) and g.bn is None
                     and w.splits == 1 and g.src.C == g.src.Cs and g.N % 16 == 0 and sp.offset % 4 == 0)
        # with optimizer-written packs the kernel must write this layer's packs itself
        pk_ok = (kg == 2 and g.src.width % 32 == 0 and g.N % 32 == 0
                 and (not g.KSb or ntt % 2 == 0))
        if fused_opt and ex.routes_ok and not pk_ok:
            fused_opt = False
        if fused_opt:
            grad = store.grad.data_ptr()
            wa.slab = grad + 4 * sp.offset
            wa.opt = ex._optim_args(False, defer_pack=True)
            wa.opt_w = sp.offset
            # the gradient the update consumed is not stored (134 MB of writes for the
            # legacy Dense(512): 1.107 -> 1.097 ms/step, with dw_order 1.101 -> 1.086,
            # profiles/r6_dense_wgrad_ab.txt) -- this layer's gradient is then not
            # readable through the store (store.view(..., grad=True)); opt_nograd=0 keeps it
            wa.opt_nograd = int(tune("opt_nograd"))
            if ex.routes_ok:
                wa.pk_fwd, wa.pk_NT = g.pack_fwd, g.NT
                wa.pk_bwd, wa.pk_NTb = (g.pack_bwd, g.NTb) if g.KSb else (-1, 0)
            if ds.dense.use_bias:
                wa.bslab = grad + 4 * store.spec(ds.dense, "bias").offset
                wa.opt_b = store.spec(ds.dense, "bias").offset
        # grid order 1: the n groups of one feature group consecutive (whole rows of the
        # weight / optimizer-state arrays per resident wave of workgroups; legacy -5 us)
        dw_order = int(tune("dw_order"))
        dw_late = bool(tune("dw_late"))     # 4 waves / SIMD: legacy 1.070 -> 1.059 ms
        wl = lambda s, a=wa, c=w.cfg, o=dw_order, l=dw_late: K.dense_wgrad(a, *c, s, o, l)
        return w, wl, fused_opt, True

    def _dense_dx(self, g, bwd2):
        """A dense layer's dX GEMM through its backward pack: (DenseFwdArgs, n-tiles per wave
        of dense_dx_kernel or 0 for the split-K dense kernel, launch callable)."""
        ex, K = self.ex, self.ex.K
        a = K.DenseFwdArgs()
        a.x = self.dense_dh[g.j].data_ptr()
        a.M, a.Ks = self.bs, g.Ns
        a.wpk = ex.arena.data_ptr() + 2 * g.pack_bwd
        a.NT, a.KS = g.NTb, g.KSb
        a.splits, a.ks_per_split = 1, g.KSb
        a.mode = 1
        a.st = ex.state.data_ptr()
        a.bt = self._bt_for(g.src)
        ntc = self._dense_dx_ntc(a) if (bwd2 and a.bt.pCs % 8 == 0 and a.Ks % 8 == 0
                                       and not K.dense_big(a.NT, a.KS)) else 0
        return a, ntc, ((lambda s, a=a, n=ntc: K.dense_dx(a, n, s)) if ntc else (lambda s, a=a: K.dense_fwd(a, s)))

    def _build_dense_bwd(self, g, ds):
        """One dense layer's backward: its wgrad and (unless it is the first layer) its dX, as
        one launch or two, and the layer's reduction group."""
        K, store = self.ex.K, self.ex.store
        sp = store.spec(ds.dense, "kernel")
        bsp = store.spec(ds.dense, "bias") if ds.dense.use_bias else None
        # Unpadded flatten source and N % 16 == 0: the single-split slab IS the Keras
        # (in, out) layout, so the wgrad kernel writes the gradient buffer directly and
        # the slab round trip disappears (the dense kernel is most of the model's bytes).
        direct = (g.src.C == g.src.Cs and g.N % 16 == 0 and g.src.width % 16 == 0
                  and g.src.width * g.N * 4 > (16 << 20))     # small layers keep split-K slabs
        w, wl, fused_opt, bwd2 = self._dense_wgrad(g, ds, direct)
        wa, cfg = w.a, w.cfg
        wname, dname = "wgrad_dense%d" % g.j, "dense_dx%d" % g.j
        da, ntc, dl = self._dense_dx(g, bwd2) if g.KSb else (None, 0, None)
        dx_first = da is not None and fused_opt
        dual = da is not None and not fused_opt and tune("dual_dense")
        if dx_first:
            # the wgrad's fused optimizer rewrites this layer's backward pack: its dX (that
            # pack's reader) runs first, as a launch of its own on the same stream -- never
            # in one launch with it (dense_bwd_pair: dX workgroups would read a pack the
            # wgrad workgroups are rewriting)
            self._add(dname, dl, da=da)
            self._add_stage_tail_bwd(self.ex.stage_of(g.src))
        if dual:
            # one launch for the dense wgrad and dX (independent GEMMs over dH); the layer's
            # slabs are final after it
            dname = "dense_bwd%d" % g.j
            if ntc:
                fn = lambda s, a=da, w=wa, c=cfg, n=ntc: K.dense_bwd_pair(w, *c, a, n, s)
            elif bwd2:
                fn = lambda s, a=da, w=wa, c=cfg: (K.dense_wgrad(w, *c, s), K.dense_fwd(a, s))
            else:
                fn = lambda s, a=da, w=wa, c=cfg: self._dense_dual(w, c, a, s)
            self._add(dname, fn, wa=wa, cfg=cfg, da=da)
        else:
            self._add(wname, wl, "main" if dx_first else "side", wa=wa, cfg=cfg)
        ld = g.NT * 16
        descs = [] if (direct or fused_opt) else [RedDesc(w.slab.data_ptr(), wa.Ktiles * 16 * ld, w.splits, ld,
                                                          sp.offset, sp.numel, RED_FLATW, 0, 0, g.src.C, g.N,
                                                          g.src.Cs)]
        if bsp is not None and not fused_opt:
            descs.append(RedDesc(w.bslab.data_ptr(), ld, w.splits, ld, bsp.offset, bsp.numel, RED_BIAS))
        bn_descs, bn_specs = self._bn_descs(g)
        lo, hi = self._add_group(sp, descs + bn_descs, bsp, bn_specs)
        if fused_opt:
            self.dense_fused_opt.append((wa, hi - lo))
        if da is not None and not (dx_first or dual):
            self._add(dname, dl, da=da)
        if da is not None:
            self.pack_readers.append((dname, sp.offset, sp.offset + sp.numel))
            if not dx_first:
                self._add_stage_tail_bwd(self.ex.stage_of(g.src))

    def _dgrad_args(self, g):
        """ConvMMArgs of conv layer g's dgrad (a stride-1 conv over the input-dilated dY with
        the flipped taps of its backward pack), written through the previous stage's backward."""
        ex = self.ex
        prev = ex.convs[g.i - 1]
        a = ex.K.ConvMMArgs()
        a.x = self.conv_dy[g.i].data_ptr()
        a.B, a.H, a.W, a.Cs_in = self.bs, g.Ho, g.Wo, g.Cs_out
        if g.pool:      # dY rebuilt on load from pooled dP + argmax codes
            a.in_code = self.conv_code[g.i].data_ptr()
            a.in_pH, a.in_pW = g.Hp, g.Wp
        a.Ho, a.Wo = g.H, g.W            # == prev stage output grid
        a.KH, a.KW, a.stride = g.KH, g.KW, 1
        a.pad_t, a.pad_l, a.in_dil = g.KH - 1 - g.pad_t, g.KW - 1 - g.pad_l, g.stride
        a.KS = g.KSd
        a.wpk = ex.arena.data_ptr() + 2 * g.pack_dgrad
        a.NT = g.NTd
        a.mode, a.flat_out = 1, 0
        a.st = ex.state.data_ptr()
        a.bt = self._bt_for(prev.out_src)
        a.tm = tune("dgrad_tm", layer=g.i)      # co-scheduled dgrad m-tiles per wave per pass
        a.dbg = tune("dgrad_dbg")            # A/B switches (ConvMMArgs::dbg; exact ones only)
        return a

    def _build_conv_bwd(self, g, cs):
        """One conv layer's backward: its wgrad and (unless it is the first layer) its dgrad --
        one dual launch where both take the halo kernels -- and the layer's reduction group."""
        ex, K, store = self.ex, self.ex.K, self.ex.store
        xin = self.xb if g.i == 0 else self.conv_out[g.i - 1]
        # (a BatchNormalization stage: conv_dy holds the dense un-pooled dz of bn_bwd_apply)
        g_stage, g = g, g.linear
        wide = self._wide(g.Cs_in, g.KS, g.NT)
        if wide:
            w = self._wgrad_tile_args(xin, g, cs.conv.use_bias)
            wl = lambda s, a=w.a, c=w.cfg: K.wgrad_tile(a, c[0], s)
        else:
            w = self._wgrad_halo_args(xin, g, cs.conv.use_bias)
            if g.i == 0 and self.pro_free:      # the images the stack read from the dataset
                w.a.xidx, w.a.xst = self.srcidx.data_ptr(), ex.state.data_ptr()
            wl = lambda s, a=w.a, c=w.cfg: K.wgrad_halo(a, *c, s)
        ca = self._dgrad_args(g) if g.i > 0 else None
        dual = (ca is not None and tune("dual_halo")
                and not wide and not self._wide(ca.Cs_in, ca.KS, g.NTd))
        dname = "dgrad_conv%d" % g.i
        if dual:
            # one launch for the layer's wgrad and dgrad (independent GEMMs sharing dY); the
            # layer's slabs are final after it
            ntc = self._halo_cfg(ca, g.NTd, False, dual=True)
            dname = "wgrad_dgrad_conv%d" % g.i
            fn = lambda s, a=ca, n=ntc, w=w.a, c=w.cfg, nm=dname: self._dual(a, n, w, c, s, nm)
            self._add(dname, fn, "main", ca=ca, ntc=ntc, wa=w.a, cfg=w.cfg)
        else:
            self._add("wgrad_conv%d" % g.i, wl, "side", wa=w.a, cfg=w.cfg)
        sp = store.spec(cs.conv, "kernel")
        bsp = store.spec(cs.conv, "bias") if cs.conv.use_bias else None
        ld = g.NT * 16
        descs = [RedDesc(w.slab.data_ptr(), w.a.Ktiles * 16 * ld, w.splits, ld, sp.offset, sp.numel, RED_CONVW,
                         g.KH, g.KW, g.Cin, g.Cout, g.Cs_in)]
        if bsp is not None:
            descs.append(RedDesc(w.bslab.data_ptr(), ld, w.splits, ld, bsp.offset, bsp.numel, RED_BIAS))
        bn_descs, bn_specs = self._bn_descs(g_stage)
        self._add_group(sp, descs + bn_descs, bsp, bn_specs)
        if ca is not None:
            if not dual:
                self._add(dname, self._conv_launch(ca, g.NTd, False), ca=ca)
            self.pack_readers.append((dname, sp.offset, sp.offset + sp.numel))
            self._add_stage_tail_bwd(ex.convs[g.i - 1])

    # ---------------------------------------------------------------- step program: reductions
    def _build_reduce(self):
        """Merge per-layer slab groups (backward order) into buckets -- the DP reducer's
        buckets, or the same 1 MiB bucketing without DP (dense layer first, then convs) --
        and insert one reduction launch per bucket right after its last group's wgrad, on
        the side stream, so the dense bucket's reduction overlaps the conv backward."""
        ex, reducer = self.ex, self.ex.reducer
        if reducer is None:
            bucket_groups, dp_early = self._assign_buckets(), []
        else:
            bucket_groups, dp_early = self._assign_buckets_dp(reducer)
        inserts = []                       # (launch index to insert after, bucket)
        for k, bg in enumerate(bucket_groups):
            tab = ex.K.RedTable()
            # longest reductions (most slabs) first: their workgroups dispatch first and their
            # memory round trips overlap the many short ones instead of trailing the launch
            descs = sorted((d for i in bg if i not in dp_early for d in self.red_groups[i].descs),
                           key=lambda d: -d.S)
            # (a bucket with more descriptors than a table holds -- many BatchNormalization stages:
            # further tables, launched as plain slab reductions behind the first)
            more = []
            for j, d in enumerate(descs):
                if j and j % ex.K.MAX_RED == 0:
                    more.append(ex.K.RedTable())
                (more[-1] if more else tab).add(*d)
            if more:
                self.bucket_overflow[k] = more
            lo = min(self.red_groups[i].lo for i in bg)
            hi = max(self.red_groups[i].hi for i in bg)
            self.bucket_tables.append((lo, hi, tab))
            inserts.append((max(self.red_groups[i].ready for i in bg), k))
        whole = self._whole_grad_launches(dp=reducer is not None)
        # data parallel: behind the (one) bucket's slab reduction, ahead of its all-reduce
        extra = [(name + "_b%d", lambda k, fn=fn: fn, "main") for name, fn, _ in whole] if reducer is not None else []
        if self.comm_in_graph:
            xk = getattr(reducer, "xgmi_bucket", None)
            if ex.whole_grad_first and xk is not None:
                raise AssertionError("gradient clipping / weight regularizers run on the RCCL plane only")
            self._plan_bucket_exchange(reducer, xk, bucket_groups, dp_early)
            extra += self._comm_launches(reducer, xk, len(bucket_groups))
        self.launches, self.bucket_ready = splice_bucket_launches(
            self.launches, inserts,
            [("reduce_b%d", lambda k: (lambda s: self._launch_bucket_reduce(k, s)), "side")] + extra)
        if reducer is None:
            # single GPU: after the last slab reduction, ahead of the (clipped) optimizer launch
            # (_launch_optim) -- inside the captured step
            for name, fn, args in whole:
                self._add(name, fn, **args)
        spans = [(lo, hi) for lo, hi, _ in self.bucket_tables]
        if self.comm_in_graph and self.optim_on_comm:
            # a comm-stream optimizer writes its layers' packs: never while a later
            # main-stream launch (a wide conv's separate dgrad) still reads one of them
            self.launches = defer_after_readers(self.launches, "optim_b%d", spans, self.pack_readers)
        # (data parallel: every early reduction lies inside its all-reduce bucket's span)
        if reducer is None:
            spans = spans + [e[1] for e in self.early_red.values()]
        check_bucket_cover(spans, ex.store.numel)

    def _whole_grad_launches(self, dp: bool):
        """The launches over the WHOLE reduced gradient, in their order, behind the last slab
        reduction and ahead of any update (HipExecutor.whole_grad_first):
        [(name, fn(stream), Launch.args)].
        weight_reg: the regularizers' term joins the gradient in place (data parallel: every rank
        adds it to its OWN reduced gradient -- weights are identical on all ranks, the average is
        avg(g) + reg'(w) -- and every rank's loss takes the penalty).
        grad_sqnorm: the global norm for clipnorm, which the clipped optimizer launch reads.
        grad_clip_apply, data parallel only: each rank clips its OWN reduced gradient by its own
        norm, in memory, ahead of the all-reduce (Horovod's order: clip, then average); the update
        behind the all-reduce is the ordinary unclipped one with grad_scale = 1 / size."""
        ex, out = self.ex, []
        if ex.regs:
            ra = ex._reg_args(self.bs, True)
            out.append(("weight_reg", lambda s, a=ra: ex.K.weight_reg(a, s), {"reg": ra}))
        ca = ex._clip_args() if ex.clips else None
        if ex.clipnorm:
            out.append(("grad_sqnorm", lambda s, a=ca: ex.K.grad_sqnorm(a, s), {"clip": ca}))
        if dp and ex.clips:
            out.append(("grad_clip_apply", lambda s, a=ca: ex.K.grad_clip_apply(a, s), {"clip": ca}))
        return out

    def _assign_buckets(self):
        """Single GPU: the groups of each bucket (lists of red_groups indices), less the groups
        an early reduction takes; decides optim_fused."""
        # single stream, no all-reduce to overlap: ONE reduction launch at the end of the
        # backward (each launch boundary costs ~5 us here), if the descriptors fit a table
        ndesc = sum(len(grp.descs) for grp in self.red_groups)
        one = ndesc <= tune("red_desc_max")       # (RedTable capacity, MAX_RED)
        limit = 1 << 62 if one else int(os.environ.get("INTML_BUCKET_BYTES", 1 << 20))
        # ... with the optimizer fused into it when its table covers every parameter
        covered = sum(d.numel for grp in self.red_groups for d in grp.descs)
        covered += sum(n for _, n in self.dense_fused_opt)
        self.optim_fused = (one and covered == self.ex.store.numel and tune("fuse_optim")
                            and not self.ex.whole_grad_first)
        if not self.optim_fused:
            # the step ends with a full optimizer launch after all: the dense layers keep
            # writing their gradient in place, but leave the update -- and the bf16 pack
            # writes that go with it -- to it, so they also store the gradient it reads
            for wa, _ in self.dense_fused_opt:
                wa.opt_w, wa.opt_b = -1, -1
                wa.pk_fwd, wa.pk_bwd = -1, -1
                wa.opt_nograd = 0
            self.dense_fused_opt = []
        early = self._early_groups() if self.optim_fused else []
        bucket_groups, cur, nb = [], [], 0
        for gi, grp in enumerate(self.red_groups):
            if gi in early:
                continue
            cur.append(gi)
            nb += (grp.hi - grp.lo) * 4
            if nb >= limit:
                bucket_groups.append(cur)
                cur, nb = [], 0
        if cur:
            bucket_groups.append(cur)
        return bucket_groups

    def _assign_buckets_dp(self, reducer):
        """Data parallel: the reducer's buckets, and the groups reduced early inside the
        backward (with their xGMI push / exchange planned).  Returns (bucket groups, early groups)."""
        # (whole_grad_first: the reducers' configure gives ONE bucket, from optimizer.clips / the
        # needs_local_gradient flag make_reducer passes)
        bucket_groups = reducer.configure([(grp.lo, grp.hi) for grp in self.red_groups])
        if self.ex.whole_grad_first and len(bucket_groups) != 1:
            raise AssertionError("gradient clipping / weight regularizers: the data-parallel step needs ONE bucket")
        # one bucket at the end of the backward (the adaptive plan for gradients <= 16 MB):
        # the groups final before the first dual launch (head, dense -- the single-GPU
        # step's early bucket) are REDUCED early there (grad_only: no update), so the
        # end-of-backward reduction ahead of the all-reduce only has the conv layers' slabs
        # left (the update stays behind the all-reduce)
        # one rank (the N = 1 data-parallel step): nothing to exchange -- the early groups
        # are reduced AND updated in that launch, as on a single GPU (xchg_p1: keep the
        # exchange structure, to measure its fixed cost)
        solo = reducer.size == 1 and getattr(reducer, "xgmi", None) is not None and not tune("xchg_p1")
        if not (len(bucket_groups) == 1 and self.comm_in_graph and tune("dp_early")):
            return bucket_groups, []
        dp_early = self._early_groups(grad_only=not solo)
        if solo and self.early_red:
            self.xchg.pushed = next(iter(self.early_red.values()))[1]
            self.xchg.exchanged = True
        # producer push (xGMI plane): the early groups' reduced gradient goes straight to
        # its owners' inboxes from the launch that reduces it, inside the backward, and
        # the fused all-reduce kernel skips those elements in its phase 1
        # ... and (exchange) the NEXT dual launch finishes that range's all-reduce and
        # applies its update in extra workgroups of its own, so the fused kernel after
        # the backward is left with the conv layers only
        if tune("xgmi_push") and not solo:
            # every early table would start at block-flag slot 0 (fbase) and the pushed /
            # exchanged range is ONE span: _early_groups caps them at one dual launch
            assert len(self.early_red) <= 1, "exchange: one early table per step (flag slots, pushed range)"
            for nm, (tab, span, grad_only) in self.early_red.items():
                if grad_only:
                    self._plan_early_exchange(reducer, nm, tab, *span)
        return bucket_groups, dp_early

    def _plan_early_exchange(self, reducer, nm, tab, elo, ehi):
        """How the early range [elo, ehi), reduced by dual launch ``nm`` through ``tab``, crosses
        the xGMI plane: split exchange, else unsplit exchange, else producer push only."""
        x = self.xchg
        # (xchg_at=end: the exchange as a launch of its own after the end-of-
        # backward reduction instead of extra workgroups of the next dual launch)
        at_end = tune("xchg_at") == "end"
        nxt = (("end" if at_end else self._xchg_launch(nm, elo, ehi))
               if tune("xgmi_xchg") else None)
        # split exchange (default): the owner half (wait for the senders, sum,
        # push the sums back: mode 4) in extra workgroups of the next dual launch,
        # covering only the table blocks this rank owns part of (none at one
        # rank), and the finish half (wait for the other owners, update: mode 5)
        # beside the end-of-backward table in ONE launch -- every wait is on a
        # flag raised in an EARLIER launch, and no conv-sized workgroup holds a
        # CU slot for the update (xchg_split=0: both halves in the dual launch)
        if nxt and not at_end and tune("xchg_split"):
            trip = reducer.exchange_args(elo, ehi, tab.nblocks, table=tab)
            if trip is not None:
                x.early_push[nm] = trip[0]
                if trip[1].b_hi > trip[1].b_lo:
                    x.early_xchg[nxt] = (tab, trip[1])
                x.xchg_fin = (tab, trip[2])
                x.pushed, x.exchanged = (elo, ehi), True
                return
        # unsplit exchange: the whole finish in the next dual launch (or at the end)
        pair = reducer.exchange_args(elo, ehi, tab.nblocks) if nxt else None
        if pair is not None:
            x.early_push[nm] = pair[0]
            if at_end:
                x.xchg_end = (tab, pair[1])
            else:
                x.early_xchg[nxt] = (tab, pair[1])
            x.pushed, x.exchanged = (elo, ehi), True
            return
        # push only: the fused all-reduce kernel finishes the range
        xp = reducer.push_args(elo, ehi)
        if xp is not None:
            x.early_push[nm], x.pushed = xp, (elo, ehi)

    def _plan_bucket_exchange(self, reducer, xk, bucket_groups, dp_early):
        """xGMI exchange of the end-of-backward table too (XgmiPush mode 3): its launch reduces the
        conv layers' slabs, pushes them to their owners, finishes their all-reduce and applies
        the update -- with the early range exchanged inside the backward, the whole step's
        all-reduce + optimizer then runs in table launches and the fused kernel is not launched."""
        x = self.xchg
        if xk is None or not tune("xgmi_xchg") or not (x.exchanged or not dp_early):
            return
        blo, bhi, btab = self.bucket_tables[xk]
        rlo, rhi = reducer.buckets[xk]
        early_n = (x.pushed[1] - x.pushed[0]) if x.exchanged else 0
        tab_n = sum(self.red_groups[i].hi - self.red_groups[i].lo for i in bucket_groups[xk] if i not in dp_early)
        if btab.nblocks > 0 and early_n + tab_n == rhi - rlo:
            # (the early table's flag slots [0, its nblocks) -- one early table, asserted above)
            fb = sum(t.nblocks for t in {id(t): t for t in [e[0] for e in x.early_xchg.values()]
                                         + ([x.xchg_end[0]] if x.xchg_end else [])
                                         + ([x.xchg_fin[0]] if x.xchg_fin else [])}.values())
            x3 = reducer.exchange_args(blo, bhi, btab.nblocks, fbase=fb, fused=True)
            if x3 is not None:
                x.bucket_xchg[xk] = x3

    def _comm_launches(self, reducer, xk, nbuckets):
        """The per-bucket launches behind each bucket's slab reduction when the all-reduces are
        captured with the step: [(name pattern, factory k -> fn(stream) or None, stream tag)]."""
        ex, K, x = self.ex, self.ex.K, self.xchg
        rccl_buckets = [k for k in range(nbuckets) if k != xk]
        # fork the comm stream only when an RCCL bucket has later backward work to overlap
        fork = tune("comm_fork")
        self.comm_fork = ((fork not in ("0", "false", "False")) if fork
                          else any(k < nbuckets - 1 for k in rccl_buckets))
        if self.comm_fork:
            self.comm_stream = torch.cuda.Stream(device=ex.device)
        if xk is not None:
            self.optim_on_comm = True
        grad = ex.store.grad

        def xchg_optim(pair):     # an exchange launch of its own: (RedTable, XgmiPush)
            return lambda s: K.reduce_optim(grad.data_ptr(), pair[0], ex._optim_args(False, defer_pack=True), s,
                                            pair[1])
        extra = [("allreduce_b%d", lambda k: None if k == xk else (lambda s: reducer.launch(k, grad, s)), "comm")]
        if self.optim_on_comm:
            extra.append(("optim_b%d", lambda k: None if k == xk else
                          (lambda s: self._launch_optim_comm(k, s)), "comm"))
        # the xGMI bucket: all-reduce + Keras update in one kernel on the main stream
        # (xchg_at=end: the early range's exchange + update after the end-of-backward reduction)
        extra.append(("xchg_early_b%d", lambda k: None if (k != xk or x.xchg_end is None) else
                      xchg_optim(x.xchg_end), "main"))
        # (the split exchange's finish half rides in the end-of-backward table launch; a launch
        # of its own only when that table is not exchanged)
        extra.append(("xchg_fin_b%d", lambda k: None if (k != xk or x.xchg_fin is None or k in x.bucket_xchg) else
                      xchg_optim(x.xchg_fin), "main"))
        extra.append(("xgmi_allreduce_optim_b%d", lambda k: None if (k != xk or k in x.bucket_xchg) else
                      (lambda s: reducer.launch_fused(grad, ex._optim_args(False, defer_pack=True), s,
                                                      pushed=x.pushed, exchanged=x.exchanged)),
                      "main"))
        return extra

    def _early_groups(self, grad_only: bool = False):
        """Single-GPU fused-optimizer step: slab groups whose gradients are final before a dual
        conv backward launch (the head and dense layers before the first one) are reduced and
        updated by extra workgroups OF that launch (DualExtra) instead of in the end-of-step
        reduction -- their latency-bound reduce + update overlaps the conv backward.  Only
        groups no later launch reads the weights of (pack readers), as one contiguous
        parameter span.  Sets
        self.early_red = {launch name: (RedTable, (lo, hi), grad_only)}; returns the groups
        assigned.  grad_only (data-parallel step): reduction only -- no update, no pack
        writes, so later pack readers do not matter."""
        self.early_red = {}
        # (not inline_update_ok: the head and dense groups stay in the end-of-step / per-bucket
        # reduce_optim_kernel<KIND> launch)
        if not tune("early_reduce") or not self.ex.inline_update_ok:
            return []
        names = [it[0] for it in self.launches]
        # only the FIRST dual launch carries a bucket: every dual launch carrying the previous
        # layer's bucket (conv2's in dual conv1, ...) measured 3% slower on RPV (conv2's
        # many-split slabs stretch dual conv1's tail by ~3 us, more than the reduction sheds)
        # (the step's last wgrad launch -- the first conv layer's -- carrying the other conv
        # layers' reductions as extra workgroups measured 2-3 us slower on RPV and MNIST:
        # profiles/r3_s2_early_wgrad_ab.txt)
        duals = [i for i, nm in enumerate(names) if nm.startswith("wgrad_dgrad_conv")][:1]
        # (the step's last launch -- the first conv layer's halo wgrad -- reducing + updating the
        # earlier conv layers' slabs in its own workgroups' tails measured slower too: RPV
        # 1.121M -> 1.071M img/s, legacy 103.4k -> 94.7k; profiles/r4_ab_rpv.txt)
        taken = []
        for t in duals:
            late_readers = [] if grad_only else [(rlo, rhi) for nm, rlo, rhi in self.pack_readers
                                                 if nm not in names[:t]]
            grp = [gi for gi, rg in enumerate(self.red_groups) if gi not in taken and rg.ready <= t
                   and not any(rlo < rg.hi and rhi > rg.lo for rlo, rhi in late_readers)]
            if not grp:
                continue
            lo = min(self.red_groups[gi].lo for gi in grp)
            hi = max(self.red_groups[gi].hi for gi in grp)
            descs = [d for gi in grp for d in self.red_groups[gi].descs]
            if (sum(self.red_groups[gi].hi - self.red_groups[gi].lo for gi in grp) != hi - lo
                    or not descs or len(descs) > 16):
                continue                                   # not one contiguous span / table
            tab = self.ex.K.RedTable()
            for d in sorted(descs, key=lambda d: -d.S):
                tab.add(*d)
            self.early_red[names[t]] = (tab, (lo, hi), grad_only)
            taken += grp
        return taken

    def _xchg_launch(self, name, lo, hi):
        """The dual launch after ``name`` that can run the exchange (all-reduce finish + update)
        of the early range [lo, hi): the next dual backward launch, provided no launch from it
        on reads the range's bf16 packs (the update rewrites them).  None if there is none."""
        names = [it[0] for it in self.launches]
        i = names.index(name)
        nxt = [j for j in range(i + 1, len(names)) if names[j].startswith("wgrad_dgrad_conv")]
        if not nxt:
            return None
        later = set(names[nxt[0]:])
        if any(nm in later and rlo < hi and rhi > lo for nm, rlo, rhi in self.pack_readers):
            return None
        return names[nxt[0]]

    def _launch_optim_comm(self, k, stream):
        """Keras update of bucket k's parameters on the comm stream after its all-reduce;
        it writes the bf16 packs of the weights it updates (pack routes), so the launch list
        places it behind the last backward launch reading one of them (defer_after_readers)."""
        ex = self.ex
        lo, hi, _ = self.bucket_tables[k]
        a = ex._optim_args(False, defer_pack=True)   # built at capture time: grad_scale = 1/size
        a.lo, a.n = lo, hi - lo
        ex.tile_routes(a)
        ex.K.optim(a, self._no_packs, stream.cuda_stream if hasattr(stream, "cuda_stream") else stream)

    # ---------------------------------------------------------------- execution
    def _run_seq(self, lo: int = 0, hi: Optional[int] = None):
        """Launch [lo, hi) on the streams ``stream_program`` assigns (concurrent chains that
        join main at the end)."""
        items = self.launches[lo:hi]
        skip = tune("skip")          # timing ablation only (wrong results): "name/name"
        if skip:
            drop = set(skip.split("/"))
            items = [it for it in items if it[0] not in drop]
        tags = [it.tag for it in items]
        streams = {"main": torch.cuda.current_stream(), "comm": self.comm_stream}
        for op in stream_program(tags, comm=self.comm_stream is not None):
            if op[0] == "wait":
                streams[op[1]].wait_stream(streams[op[2]])
                continue
            _, sname, i = op
            st = streams[sname]
            # comm launches take the Stream (RCCL wrappers use it as a context); others the handle
            items[i][1](st if tags[i] == "comm" else st.cuda_stream)

    def _launch_bucket_reduce(self, k, s):
        lo, hi, tab = self.bucket_tables[k]
        ex = self.ex
        xp, fin = self.xchg.bucket_xchg.get(k), self.xchg.xchg_fin
        if xp is not None and fin is not None:   # + the early range's exchange finish (mode 5)
            ex.K.reduce_optim_end(ex.store.grad.data_ptr(), tab, ex._optim_args(False, defer_pack=True), s, xp,
                                  fin[0], fin[1])
        elif xp is not None:     # reduction + all-reduce (exchange) + Keras update in one launch
            ex.K.reduce_optim(ex.store.grad.data_ptr(), tab, ex._optim_args(False, defer_pack=True), s, xp)
        elif self.optim_fused:     # gradient reduction + Keras update in one launch (re-pack deferred)
            ex.K.reduce_optim(ex.store.grad.data_ptr(), tab, ex._optim_args(False, defer_pack=True), s)
        else:
            ex.K.slab_reduce(ex.store.grad.data_ptr(), lo, hi, tab, s)
        for t in self.bucket_overflow.get(k, ()):
            if xp is not None or self.optim_fused:
                raise AssertionError("a bucket of several reduction tables is reduced by plain slab reductions only")
            ex.K.slab_reduce(ex.store.grad.data_ptr(), lo, hi, t, s)

    def _launch_optim(self):
        ex = self.ex
        # the re-pack of the updated weights is done by the next step's prologue launch
        # (a clipping optimizer: the clipped launch on one GPU -- store.grad keeps the unclipped
        # reduced gradient; behind a reducer the gradient in memory is already clipped)
        ex.K.optim(ex.tile_routes(ex._optim_args(False, defer_pack=True, clip=ex.reducer is None)), ex.pack_table,
                   torch.cuda.current_stream().cuda_stream)

    def _body(self, with_optim: bool):
        self._run_seq()
        if self.training and with_optim and not self.optim_fused and not self.optim_on_comm:
            self._launch_optim()

    def _dp_segments(self):
        """[(launch_lo, launch_hi, bucket)]: segment k ends with the slab reduction that
        completes bucket k; a trailing (lo, hi, None) segment holds any later launches."""
        segs, lo = [], 0
        for k, ready in enumerate(self.bucket_ready):
            segs.append((lo, ready, k))
            lo = ready
        if lo < len(self.launches):
            segs.append((lo, len(self.launches), None))
        return segs

    def _run_segment(self, lo, hi, k):
        self._run_seq(lo, hi)

    def run(self, k: int = 1):
        """Run ``k`` consecutive steps.  Step bookkeeping (data cursor, iteration count, LR,
        dropout counter) is device-resident, so k steps are ONE graph of k back-to-back step
        bodies: the inter-graph launch gap is paid once per k steps."""
        ex = self.ex
        dp = self.training and ex.reducer is not None and ex.reducer.active
        if dp:
            ex.grad_scale = 1.0 / ex.reducer.size
        if not dp or self.comm_in_graph:
            # single launch sequence; with the native RCCL engine it includes the bucket
            # all-reduces on the comm stream (one graph replay per DP step / k steps)
            if not ex.use_graphs:
                for _ in range(k):
                    self._body(with_optim=True)
            elif k == 1:
                if self.graph is None:
                    self.graph = self._capture(lambda: self._body(with_optim=True))
                self.graph.replay()
            else:
                g = self.multi_graphs.get(k)
                if g is None:
                    def body_k():
                        for _ in range(k):
                            self._body(with_optim=True)
                    g = self.multi_graphs[k] = self._capture(body_k)
                g.replay()
            if dp:
                ex.reducer.after_step()
            return
        for _ in range(k):
            self._run_dp_segmented()

    def _run_dp_segmented(self):
        ex = self.ex
        # Data parallel, torch.distributed data plane: each bucket's all-reduce is issued
        # between graph segments as soon as its slab reduction is done, so RCCL moves the
        # dense bucket over xGMI while the conv backward runs; the fused optimizer (with the
        # 1/size average folded in) runs after the last wait.
        segs = self._dp_segments()
        if ex.use_graphs and self.dp_graphs is None:
            self.dp_graphs = [self._capture(lambda a=lo, b=hi, k=k: self._run_segment(a, b, k))
                              for lo, hi, k in segs]
            self.dp_graphs.append(self._capture(self._launch_optim))
        for j, (lo, hi, k) in enumerate(segs):
            if ex.use_graphs:
                self.dp_graphs[j].replay()
            else:
                self._run_segment(lo, hi, k)
            if k is not None:
                ex.reducer.start(k, ex.store.grad)
        ex.reducer.finish()
        if ex.use_graphs:
            self.dp_graphs[-1].replay()
        else:
            self._launch_optim()

    def _capture(self, fn):
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream(device=self.ex.device)
        s.wait_stream(torch.cuda.current_stream())
        # no Python GC inside the capture: collecting an unreachable plan of another model
        # destroys its graphs/events, which HIP forbids while a stream is capturing (abort)
        gc_was = gc.isenabled()
        gc.collect()
        gc.disable()
        try:
            # thread-local capture mode: RCCL / watchdog threads may query events meanwhile
            with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
                fn()
        finally:
            if gc_was:
                gc.enable()
        torch.cuda.current_stream().wait_stream(s)
        return g

"""Horovod-shaped data-parallel runtime over torch.distributed (RCCL on ROCm).

API parity with the calls the reference makes:
  ``hvd.init()``                    train_rpv.py:37, DistTrain_mnist.ipynb:148
  ``hvd.rank()/local_rank()/size()``train_rpv.py:38-39,56,65
  ``hvd.DistributedOptimizer(opt)`` rpv.py:65, DistTrain_mnist.ipynb:310
  ``hvd.callbacks.*``               rpv.py:83-93, DistTrain_mnist.ipynb:494

MI355X design (not a translation of Horovod's coordinator/fusion-buffer core):
  * one process per GPU, ``torch.distributed`` backend ``nccl`` (= RCCL over xGMI);
  * the flat gradient buffer is split into size-capped buckets in *backward order*
    (head/dense grads first), so the first bucket's all-reduce is in flight on
    RCCL's stream while the conv backward kernels still run;
  * averaging (1/size) is folded into the fused optimizer kernel, no extra pass;
  * initial state broadcast happens BEFORE step 0 (the reference's Horovod
    broadcasts after batch 0);
  * epoch metrics are averaged with ONE packed all-reduce.
"""
from __future__ import annotations

import os
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.distributed as tdist

from . import state as S
from ..optim.optimizers import STANDALONE_KINDS
from ..utils.tune import tune


class DataParallelDivergence(RuntimeError):
    """The ranks of a data-parallel job hold different weights (fit()'s per-epoch digest check,
    train.loop.dp_consistency_check): raised on every rank at the same epoch end."""


# ------------------------------------------------------------------------------ bootstrap
def init(shard_data: Optional[bool] = None, backend: Optional[str] = None,
         bucket_bytes: Optional[int] = None) -> S.DPState:
    """Initialise the data-parallel group from torchrun-style env vars
    (RANK, WORLD_SIZE, LOCAL_RANK, MASTER_ADDR, MASTER_PORT).  Without them this
    is a size-1 group (no process group is created).

    On GPUs the data plane is the native RCCL engine (``parallel/comm.py``) and the
    torch.distributed group is a gloo control plane; ``INTML_COMM=torch`` (or an explicit
    ``INTML_DP_BACKEND``) uses torch.distributed (``nccl`` = RCCL) for both.
    ``INTML_DP_FORCE=1`` runs the DP machinery even at size 1 (tests on a 1-GPU box)."""
    st = S.current()
    if st is not None:
        if shard_data is not None:
            st.shard_data = shard_data
        return st
    env_shard = os.environ.get("INTML_DP_SHARD")
    if shard_data is None:
        shard_data = True if env_shard is None else env_shard not in ("0", "false", "False")
    # None: adaptive (the native reducer sizes buckets from the model's gradient bytes)
    env_bb = os.environ.get("INTML_BUCKET_BYTES")
    bucket_bytes = bucket_bytes or (int(env_bb) if env_bb else None)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))
    local_size = int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))
    force = os.environ.get("INTML_DP_FORCE", "0") not in ("0", "", "false", "False")
    use_gpu = torch.cuda.is_available() and os.environ.get("INTML_DEVICE", "cuda").startswith("cuda")
    timeout_s = float(os.environ.get("INTML_DP_TIMEOUT", 600))
    owns, comm, xgmi_only = False, None, False
    plane_note = None
    if tdist.is_available() and tdist.is_initialized():
        world, rank = tdist.get_world_size(), tdist.get_rank()
        be = tdist.get_backend()
        plane_note = "torch.distributed %s (process group created by the caller)" % be
    elif world > 1:
        from . import comm as C
        mode = C.comm_mode(use_gpu, backend, local_size, torch.cuda.device_count() if use_gpu else 0)
        be = backend or os.environ.get("INTML_DP_BACKEND") or ("nccl" if use_gpu else "gloo")
        if mode in ("native", "xgmi"):
            be = "gloo"                  # control plane only; the data plane is native
        xgmi_only = mode == "xgmi"
        if use_gpu:
            torch.cuda.set_device(local_rank % torch.cuda.device_count())
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # a dead or hung rank turns into an error on every other rank after this timeout
        # (failure detection) instead of a silent hang
        import datetime
        timeout = datetime.timedelta(seconds=timeout_s)
        tdist.init_process_group(backend=be, rank=rank, world_size=world, timeout=timeout)
        owns = True
        if mode == "native":
            # collective fallback: if the RCCL communicator fails to come up -- or fails its
            # closed-form numeric self-test, eager or graph-captured -- on ANY rank, every rank
            # runs the RCCL-free plane (the fused xGMI kernel over IPC-mapped peer memory, gloo
            # control plane) instead of one rank raising while the others wait
            # (comm.establish: phased, every phase ends in a control-plane collective)
            dev = torch.device("cuda", torch.cuda.current_device()) if use_gpu else torch.device("cpu")
            comm, bad = C.establish(rank, world, dev, timeout_s)
            if bad:
                xgmi_only = True
                plane_note = "xgmi (RCCL unavailable: %s)" % "; ".join("rank %d: %s" % b for b in bad)[:400]
            else:
                plane_note = "rccl (communicator up on %d ranks, numeric self-test passed eager + captured)" % world
        elif mode == "xgmi":
            plane_note = "xgmi (RCCL-free: %s)" % ("INTML_COMM=xgmi" if os.environ.get("INTML_COMM", "").lower()
                                                   == "xgmi" else "ranks share a GPU")
        else:
            plane_note = "torch.distributed %s" % be
    else:
        be = backend or "none"
        if force and use_gpu:
            from . import comm as C
            if C.comm_mode(use_gpu, backend) == "native":
                comm = C.NativeComm(0, 1, torch.device("cuda", torch.cuda.current_device()), timeout_s)
                be = "rccl"
                plane_note = "rccl (size 1, INTML_DP_FORCE)"
    st = S.DPState(rank=rank, size=world, local_rank=local_rank, local_size=local_size,
                   backend=be, shard_data=shard_data, bucket_bytes=bucket_bytes, owns_pg=owns,
                   comm=comm, xgmi_only=xgmi_only, plane=plane_note)
    S.set_state(st)
    if plane_note and rank == 0 and world > 1:
        import sys
        print("[dp] %d ranks, gradient data plane: %s" % (world, plane_note), file=sys.stderr, flush=True)
    return st


def shutdown() -> None:
    st = S.current()
    if st is not None and st.comm is not None:
        st.comm.close()
    if st is not None and st.owns_pg and tdist.is_initialized():
        tdist.destroy_process_group()
    S.set_state(None)


def _st() -> S.DPState:
    st = S.current()
    if st is None:
        raise ValueError("Horovod-style API used before init()")
    return st


def rank() -> int: return _st().rank
def size() -> int: return _st().size
def local_rank() -> int: return _st().local_rank
def local_size() -> int: return _st().local_size
def is_initialized() -> bool: return S.current() is not None


def _active() -> bool:
    st = S.current()
    return st is not None and st.size > 1 and tdist.is_initialized()


def _native():
    """The RCCL data-plane engine when it is in use (also at size 1 under INTML_DP_FORCE)."""
    st = S.current()
    return st.comm if st is not None else None


# ------------------------------------------------------------------------------ collectives
def allreduce(value, average: bool = True, name: Optional[str] = None):
    """All-reduce a tensor / numpy array / python scalar (returns the same kind).
    Device tensors go over RCCL; host values over the control plane."""
    comm = _native()
    is_t = isinstance(value, torch.Tensor)
    if comm is not None and is_t and value.is_cuda:
        t = value.detach().clone().contiguous()
        comm.all_reduce(t)
        return t / comm.size if average else t
    if not _active():
        return value
    dev = _comm_device()
    t = value if is_t else torch.as_tensor(np.asarray(value, dtype=np.float64))
    src = t
    t = t.to(dev, dtype=torch.float64 if not is_t else t.dtype).clone()
    tdist.all_reduce(t)
    if average:
        t = t / size()
    if is_t:
        return t.to(src.device)
    out = t.cpu().numpy()
    return out.item() if np.ndim(value) == 0 else out


def allgather(value) -> list:
    if not _active():
        return [value]
    out = [None] * size()
    tdist.all_gather_object(out, value)
    return out


def broadcast(tensor: torch.Tensor, root_rank: int = 0) -> torch.Tensor:
    comm = _native()
    if comm is not None and tensor.is_cuda and comm.size > 1:
        if tensor.is_contiguous():
            comm.broadcast(tensor, root_rank)
        else:
            tmp = tensor.contiguous()
            comm.broadcast(tmp, root_rank)
            tensor.copy_(tmp)
        return tensor
    if _active():
        dev = _comm_device()
        if tensor.device == dev:
            tdist.broadcast(tensor, src=root_rank)
        else:
            tmp = tensor.to(dev)
            tdist.broadcast(tmp, src=root_rank)
            tensor.copy_(tmp.to(tensor.device))
    return tensor


def broadcast_object(obj, root_rank: int = 0):
    if not _active():
        return obj
    box = [obj]
    tdist.broadcast_object_list(box, src=root_rank)
    return box[0]


def barrier() -> None:
    if _active():
        if _st().backend == "nccl":
            tdist.barrier(device_ids=[torch.cuda.current_device()])
        else:
            tdist.barrier()


def _comm_device() -> torch.device:
    if _st().backend == "nccl":
        return torch.device("cuda", torch.cuda.current_device())
    return torch.device("cpu")


def broadcast_model_state(model, root_rank: int = 0) -> None:
    """R2: one broadcast of the flat master buffer + each optimizer slot + step."""
    if not _active():
        return
    ex = model._executor
    broadcast(model.store.master, root_rank)
    if ex is not None:
        for slot in ex.optimizer_state():
            broadcast(slot, root_rank)
        base = getattr(model.optimizer, "_base_optimizer", model.optimizer)
        it = broadcast_object(int(base.iterations), root_rank)
        ex.set_optimizer_state(it, ex.optimizer_state())
        ex.params_changed()


# ------------------------------------------------------------------------------ optimizer wrap
class _DistributedOptimizer:
    """Wraps a Keras optimizer; the executor all-reduces gradients in buckets."""

    def __init__(self, optimizer, compression=None, bucket_bytes=None):
        from ..optim import get
        object.__setattr__(self, "_base_optimizer", get(optimizer))
        object.__setattr__(self, "distributed", True)
        object.__setattr__(self, "compression", compression)
        object.__setattr__(self, "bucket_bytes", bucket_bytes)

    def __getattr__(self, item):
        return getattr(self._base_optimizer, item)

    def __setattr__(self, key, value):
        setattr(self._base_optimizer, key, value)

    def get_config(self):
        return self._base_optimizer.get_config()

    @property
    def __class__(self):   # serialises / isinstance-checks as the wrapped class
        return type(self._base_optimizer)


def DistributedOptimizer(optimizer, name=None, device_dense="", device_sparse="", compression=None,
                         sparse_as_dense=False, bucket_bytes=None):
    if not is_initialized():
        init()
    return _DistributedOptimizer(optimizer, compression=compression, bucket_bytes=bucket_bytes)


class Compression:
    """``hvd.Compression.none`` / ``.fp16``; on MI355X the 16-bit wire format is bf16."""
    none = None
    fp16 = "bf16"
    bf16 = "bf16"


# ------------------------------------------------------------------------------ grad reducer
def merge_buckets(groups: Sequence[Tuple[int, int]], bucket_bytes: int):
    """Merge backward-ordered flat (lo, hi) groups into buckets of >= ``bucket_bytes``
    (fp32); returns (group indices per bucket, (lo, hi) per bucket)."""
    buckets, cur, cur_bytes = [], [], 0
    for gi, (lo, hi) in enumerate(groups):
        cur.append(gi)
        cur_bytes += (hi - lo) * 4
        if bucket_bytes is not None and cur_bytes >= bucket_bytes:
            buckets.append(cur)
            cur, cur_bytes = [], 0
    if cur:
        buckets.append(cur)
    spans = [(min(groups[g][0] for g in b), max(groups[g][1] for g in b)) for b in buckets]
    return buckets, spans


def one_bucket_for(optimizer, needs_local_gradient=False) -> bool:
    """True when ``optimizer`` (or the one a DistributedOptimizer wraps) clips gradients: its global
    norm needs every local reduction before the first all-reduce, so both reducers configure the
    whole gradient as ONE bucket.  ``needs_local_gradient`` (the executor's: a model with weight
    regularizers, whose term joins the rank's whole local gradient in one launch ahead of the
    all-reduce) asks for the same."""
    return bool(needs_local_gradient) or bool(getattr(getattr(optimizer, "_base_optimizer", optimizer), "clips", False))


class GradReducer:
    """Bucketed gradient all-reduce over the flat grad buffer (torch.distributed data plane).

    ``groups`` are (lo, hi) flat ranges in the order their gradients become final
    during backward.  Consecutive groups are merged until ``bucket_bytes``; each
    bucket is ONE all-reduce (async, on the backend's stream) over a contiguous view,
    issued by the executor between graph segments.
    """
    capturable = False

    def __init__(self, store, compression=None, bucket_bytes: int = 4 << 20, optimizer=None,
                 needs_local_gradient=()):
        self.store = store
        self.optimizer = optimizer      # (one_bucket_for: a clipping optimizer's single bucket)
        self.needs_local_gradient = needs_local_gradient   # (... and a regularized model's: its layer names)
        self.compression = compression
        self.bucket_bytes = bucket_bytes
        self.size = size()
        self.buckets: List[Tuple[int, int]] = [(0, store.numel)]
        self.bucket_groups: List[List[int]] = [[0]]
        self._pending = {}                  # bucket -> (work, bf16 buffer or None, view)

    @property
    def active(self) -> bool:
        return self.size > 1 and _active()

    def configure(self, groups: Sequence[Tuple[int, int]]) -> List[List[int]]:
        """Merge backward-ordered groups into buckets; returns group indices per bucket."""
        one = one_bucket_for(getattr(self, "optimizer", None), getattr(self, "needs_local_gradient", ()))
        bb = (1 << 62) if one else (self.bucket_bytes or (4 << 20))
        self.bucket_groups, self.buckets = merge_buckets(groups, bb)
        return self.bucket_groups

    def start(self, bucket: int, grad: torch.Tensor):
        """Launch the all-reduce of one bucket asynchronously (stream-ordered after the
        producing kernels on the current stream)."""
        if not _active():
            return
        lo, hi = self.buckets[bucket]
        view = grad[lo:hi]
        if self.compression == "bf16":
            buf = view.to(torch.bfloat16)
            work = tdist.all_reduce(buf, async_op=True)
            self._pending[bucket] = (work, buf, view)
        else:
            work = tdist.all_reduce(view, async_op=True)
            self._pending[bucket] = (work, None, None)

    def wait(self, bucket: int) -> None:
        """Make the current stream wait for one bucket's all-reduce (and decompress it)."""
        item = self._pending.pop(bucket, None)
        if item is None:
            return
        work, buf, view = item
        work.wait()
        if buf is not None:
            view.copy_(buf.to(torch.float32))

    def finish(self) -> None:
        """Make the current stream wait for every in-flight bucket."""
        for bucket in sorted(self._pending):
            self.wait(bucket)

    def after_step(self) -> None:
        pass

    def reduce_all(self, grad: torch.Tensor, average: bool = True) -> None:
        for i in range(len(self.buckets)):
            self.start(i, grad)
        self.finish()
        if average and _active():
            grad[: self.store.numel].div_(self.size)


def adaptive_bucket_bytes(groups: Sequence[Tuple[int, int]], size: int = 1) -> int:
    """Bucket size for the captured RCCL data plane.

    * Gradients <= 16 MB: ONE fused all-reduce at the end of the backward on the main stream
      -- a linear graph.  (INTML_TUNE=dp_overlap=1, size > 1: the first bucket closes after
      the backward-ordered groups reach 1 MiB -- for the RPV model the head + dense gradient,
      96 % of the bytes -- and every bucket's all-reduce + update is forked onto the comm
      stream, overlapping the conv backward.  Measured 135.7 vs 103.0 us/step at N = 1 on the
      round-5 kernels, so it is not the default; the xGMI plane overlaps the dense bucket's
      transfer inside the backward instead -- producer push.)
    * Larger gradients (the 34.5M-param legacy RPV model: 138 MB) get ~4 buckets of >= 16 MB,
      forked onto the comm stream so the all-reduces overlap the rest of the backward."""
    total = 4 * sum(hi - lo for lo, hi in groups)
    if total <= (16 << 20):
        # (opt-in: on the round-5 kernels the forked two-bucket step measured 135.7 us/step at
        # N = 1 against 103.0 for one bucket -- profiles/r5f_ab.txt; bench.py's probe times it
        # on the real fabric at N > 1 and keeps whichever plane is faster)
        if size > 1 and total > (1 << 20) and tune("dp_overlap"):
            return 1 << 20
        return total + 1
    return max(16 << 20, total // 4)


def data_plane(grad_bytes: Optional[int] = None) -> str:
    """The gradient data plane of the native (captured) reducer, from ``INTML_XGMI``:
    "xgmi" ("1"): the whole gradient on the xGMI plane -- the early (head / dense) range
    all-reduced and updated inside the backward (exchange), the rest by the end-of-backward
    reduction launch;  "rccl" ("0"): one RCCL all-reduce + optimizer;  "hybrid": RCCL for the
    early buckets, the fused xGMI kernel for the last;  "auto" (default): ``auto_plane()``.
    ``bench.py``'s probe times every plane on the job itself and pins the fastest
    (``probe_data_planes``)."""
    mode = os.environ.get("INTML_XGMI", "auto").lower()
    if mode in ("1", "on", "true", "xgmi"):
        return "xgmi"
    if mode == "hybrid":
        return "hybrid"
    if mode in ("0", "off", "false", "rccl"):
        return "rccl"
    return auto_plane(grad_bytes)


def device_key(device) -> str:
    """Identity of the physical GPU behind ``device``: host + PCI location (else UUID)."""
    import socket
    try:
        p = torch.cuda.get_device_properties(device)
        ident = "pci:%s:%s:%s" % (p.pci_domain_id, p.pci_bus_id, p.pci_device_id)
    except Exception:                  # noqa: BLE001 -- older runtimes: the visible-device index
        ident = "idx:%s/%s" % (os.environ.get("HIP_VISIBLE_DEVICES", ""), getattr(device, "index", device))
    return socket.gethostname() + "/" + ident


# ------------------------------------------------------------------------------ plane verdicts
# A measured data-plane choice, persisted: bench.py's probe (probe_data_planes) times every
# plane on the job itself, checks the ranks' weights bit-identical after each, and rank 0
# records the winner here, keyed by (host, world size, gradient size class).  auto_plane reads
# it: without a verdict for the job's key, "auto" means RCCL (nothing but a
# measurement on the real fabric admits the xGMI plane).
VERDICT_PLANES = ("xgmi", "hybrid", "rccl")


def verdict_path() -> str:
    return os.environ.get("INTML_PLANE_VERDICTS") or os.path.join(
        os.path.expanduser("~"), ".cache", "cori_intml_examples_amd", "plane_verdicts.json")


def verdict_key(world: int, grad_bytes: int, host: Optional[str] = None) -> str:
    """(host, world size, gradient size class): the class is the power of two at or above
    the gradient's bytes, so a verdict measured on one model applies to models of the same
    order of gradient size (the quantity the planes' relative cost depends on)."""
    import socket
    cls = 1 << max(0, int(grad_bytes) - 1).bit_length()
    return "%s/P%d/%dB" % (host or socket.gethostname(), int(world), cls)


def plane_family(plane: str) -> str:
    """A probe candidate's plane family as auto_plane uses it ("xgmi_end" -> "xgmi",
    "rccl_single" / "rccl_forked" -> "rccl")."""
    return "xgmi" if plane.startswith("xgmi") else ("hybrid" if plane == "hybrid" else "rccl")


def _read_verdicts(path: str) -> dict:
    import json
    try:
        with open(path) as f:
            d = json.load(f)
        return d if isinstance(d, dict) else {}
    except (OSError, ValueError):
        return {}


def record_verdict(world: int, grad_bytes: int, plane: str, probe: Optional[dict] = None) -> Optional[str]:
    """Persist a measured plane choice (rank 0 of the measuring job).  Atomic replace; returns
    the file written, or None if it could not be (a read-only home: auto stays on RCCL)."""
    import json
    import tempfile
    import time
    path = verdict_path()
    fam = plane_family(plane)
    try:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        d = _read_verdicts(path)
        d[verdict_key(world, grad_bytes)] = {
            "plane": fam, "probe_choice": plane, "grad_bytes": int(grad_bytes), "time": time.time(),
            "probe_ms_per_step": {k: v for k, v in (probe or {}).items() if isinstance(v, (float, int))}}
        fd, tmp = tempfile.mkstemp(dir=os.path.dirname(path), prefix=".verdicts.")
        with os.fdopen(fd, "w") as f:
            json.dump(d, f, indent=1, sort_keys=True)
        os.replace(tmp, path)
        return path
    except OSError:
        return None


def lookup_verdict(world: int, grad_bytes: int) -> Optional[str]:
    """The recorded plane family for this job's key, or None."""
    v = _read_verdicts(verdict_path()).get(verdict_key(world, grad_bytes))
    plane = v.get("plane") if isinstance(v, dict) else None
    return plane if plane in VERDICT_PLANES else None


def auto_plane(grad_bytes: Optional[int] = None) -> str:
    """The default plane.  "rccl", unless a MEASURED verdict for this job's (host, world size,
    gradient size class) says otherwise (``record_verdict``, written by bench.py's plane probe
    after it checked every plane's ranks bit-identical).  The xGMI / hybrid verdicts apply only
    where those planes can run: every rank a GPU of its own on ONE node and a gradient small
    enough for one fused bucket (<= 16 MB; the 138 MB legacy gradient keeps RCCL buckets
    forked onto the comm stream).  Even then the xGMI plane is used only after its collective
    setup and stressed self-test pass the vote on every rank, else the step keeps RCCL
    (NativeGradReducer._setup_xgmi).  The caller makes the choice collective (rank 0's)."""
    if grad_bytes is not None and grad_bytes > (16 << 20):
        return "rccl"
    if is_initialized():
        st = _st()
        if (st.size > 1 and st.local_size == st.size and torch.cuda.is_available()
                and torch.cuda.device_count() >= st.local_size and grad_bytes is not None):
            v = lookup_verdict(st.size, grad_bytes)
            if v is not None:
                return v
    return "rccl"


# Optimizer kinds without instances of the xGMI exchange / all-reduce kernels (they update
# through the optimizer launch behind an RCCL all-reduce): never on the "xgmi" / "hybrid" planes.
RCCL_ONLY_KINDS = STANDALONE_KINDS    # (optim/optimizers.py KINDS: no run-time-switch instance)


def plane_for_optimizer(plane: str, optimizer, forced: bool, needs_local_gradient=(), bn_layers=()) -> str:
    """``plane`` as the step of ``optimizer`` can run it: an xGMI-family plane becomes "rccl"
    for RCCL_ONLY_KINDS -- and for any optimizer with gradient clipping (``clips``), and for a
    model with weight regularizers (``needs_local_gradient``: the names of its regularized
    layers) -- when it was merely chosen (auto / a recorded verdict), and is a ValueError when it
    was forced (INTML_XGMI, or a job without an RCCL communicator).  A model with
    BatchNormalization layers (``bn_layers``: their names) is gated the same way: its step is
    exercised on the RCCL plane only."""
    base = getattr(optimizer, "_base_optimizer", optimizer)
    clips = bool(getattr(base, "clips", False))
    if plane not in ("xgmi", "hybrid") or not (getattr(base, "kind", None) in RCCL_ONLY_KINDS or clips
                                               or needs_local_gradient or bn_layers):
        return plane
    if forced and bn_layers:
        raise ValueError("BatchNormalization layers (%s) have no kernels for the %r data plane (their gamma / beta "
                         "gradients are all-reduced over RCCL): unset INTML_XGMI / INTML_COMM"
                         % (", ".join(bn_layers), plane))
    if forced and needs_local_gradient:
        # weight regularizers: their term joins the local gradient in memory ahead of the
        # all-reduce, which only the RCCL plane's step does
        raise ValueError("weight regularizers (layers %s) have no kernels for the %r data plane (the regularized "
                         "gradient is all-reduced over RCCL): unset INTML_XGMI / INTML_COMM"
                         % (", ".join(needs_local_gradient), plane))
    if forced and clips:
        # gradient clipping: the local gradient is clipped in memory ahead of the all-reduce,
        # which only the RCCL plane's step does (the xGMI kernels reduce and exchange in one launch)
        cfg = ", ".join("%s=%g" % (k, getattr(base, k)) for k in ("clipnorm", "clipvalue")
                        if getattr(base, k, None))
        raise ValueError("optimizer %s(%s): gradient clipping has no kernels for the %r data plane (the "
                         "clipped gradient is all-reduced over RCCL): unset INTML_XGMI / INTML_COMM"
                         % (type(base).__name__, cfg, plane))
    if forced:
        name = type(base).__name__ + ("(amsgrad=True)" if getattr(base, "amsgrad", False) else "")
        raise ValueError("optimizer %s has no kernels for the %r data plane (its update runs behind an RCCL "
                         "all-reduce): unset INTML_XGMI / INTML_COMM or pick one of SGD, RMSprop, Adadelta, "
                         "Adam, Nadam" % (name, plane))
    return "rccl"


def forced_plane() -> Optional[str]:
    """The plane INTML_XGMI pins ("xgmi" / "hybrid" / "rccl"), None for auto."""
    return None if os.environ.get("INTML_XGMI", "auto").lower() in ("auto", "") else data_plane()


class NativeGradReducer:
    """Bucketed gradient all-reduce on the native RCCL engine, CAPTURABLE: the executor
    inserts ``launch(k, ..)`` into the step's launch sequence on a comm stream forked after
    bucket k's slab reduction, so the whole DP step (backward, RCCL all-reduces over
    xGMI, optimizer) is ONE HIP graph replay.  The 1/size average is folded into the fused
    optimizer (``grad_scale``).  Hvd ``Compression.fp16`` maps to a bf16 wire format
    (fp32 -> bf16 staging copy, bf16 all-reduce, copy back), all on the comm stream."""
    capturable = True

    def __init__(self, store, comm, compression=None, bucket_bytes: int = 1 << 20,
                 rank: Optional[int] = None, size: Optional[int] = None, device=None, optimizer=None,
                 needs_local_gradient=(), bn_layers=()):
        self.store, self.comm = store, comm
        self.bn_layers = bn_layers      # (a model with BatchNormalization layers: RCCL plane only)
        self.optimizer = optimizer      # (plane_for_optimizer: kinds that stay off the xGMI planes)
        self.needs_local_gradient = needs_local_gradient   # (a regularized model's layer names: the same)
        self.compression = compression
        self.bucket_bytes = bucket_bytes
        # comm None: the RCCL-free data plane (state.xgmi_only) -- the whole gradient is ONE
        # bucket through the fused xGMI kernel, rank / size from the control plane
        self.rank = comm.rank if comm is not None else int(rank)
        self.size = comm.size if comm is not None else int(size)
        self.device = comm.device if comm is not None else device
        self.buckets: List[Tuple[int, int]] = [(0, store.numel)]
        self.bucket_groups: List[List[int]] = [[0]]
        self.stream = torch.cuda.Stream(device=self.device)   # for the segmented (uncaptured) mode
        self._stage = {}
        self._configured = False
        self.xgmi = None               # parallel.xgmi.XgmiAllreduce when the fused path is on
        self.xgmi_bucket = None        # index of the bucket it reduces
        self.plane = "rccl"
        self._xgmi_err_host = None

    @property
    def active(self) -> bool:
        return True

    def configure(self, groups: Sequence[Tuple[int, int]]) -> List[List[int]]:
        self.plane = (data_plane(4 * sum(hi - lo for lo, hi in groups)) if self.comm is not None
                      else "xgmi")
        local = getattr(self, "needs_local_gradient", ())
        self.plane = plane_for_optimizer(self.plane, getattr(self, "optimizer", None),
                                         forced=self.comm is None or forced_plane() is not None,
                                         needs_local_gradient=local, bn_layers=getattr(self, "bn_layers", ()))
        if self.comm is not None and self.size > 1 and _active():
            # one plane for the job: rank 0's (a verdict file written between two ranks' reads
            # must not split the job between planes)
            self.plane = broadcast_object(self.plane, 0)
        bb = self.bucket_bytes
        if self.plane == "xgmi" or one_bucket_for(getattr(self, "optimizer", None), local):
            # the whole gradient is ONE bucket: the fused xGMI kernel's, or a clipping
            # optimizer's (the global norm needs every local reduction before any all-reduce),
            # or a regularized model's (one weight_reg launch over the whole local gradient)
            bb = 1 << 62
        elif self.plane == "hybrid" and not bb:
            bb = 1 << 20                    # dense bucket(s) over RCCL, the conv tail over xGMI
        bg, spans = merge_buckets(groups, bb or adaptive_bucket_bytes(groups, self.size))
        if self._configured and spans == self.buckets and bg == self.bucket_groups:
            return self.bucket_groups       # same layout (another batch size): keep the staging
        self.bucket_groups, self.buckets = bg, spans   # buffers earlier graphs reference
        self._configured = True
        self._stage = {}
        self._setup_xgmi()
        if self.compression == "bf16":
            for k, (lo, hi) in enumerate(self.buckets):
                if k != self.xgmi_bucket:
                    self._stage[k] = torch.empty(hi - lo, dtype=torch.bfloat16, device=self.device)
        return self.bucket_groups

    def _setup_xgmi(self):
        """The bucket that goes over the fused xGMI all-reduce + optimizer kernel instead of
        RCCL + an optimizer launch: plane "xgmi" -> the single whole-gradient bucket; plane
        "hybrid" -> the LAST bucket (the small conv tail of the backward, latency-bound on
        RCCL) while the earlier ones stay on RCCL, forked onto the comm stream so they overlap
        the conv backward.  fp32 wire only; collective setup + self-test, same decision on
        every rank (else every bucket stays on RCCL)."""
        # (without an RCCL communicator the wire is always fp32 xGMI: Compression.fp16 is
        # a bandwidth option, the result is the fp32 all-reduce either way)
        want = self.plane in ("xgmi", "hybrid") and (self.compression is None or self.comm is None)
        k = len(self.buckets) - 1 if want else None
        n = (self.buckets[k][1] - self.buckets[k][0]) if want else 0
        if self.xgmi is not None and (not want or self.xgmi.n != n):
            self.xgmi.close()
            self.xgmi = None
        self.xgmi_bucket = None
        if want and self.xgmi is None:
            from . import xgmi as X
            # ranks sharing a GPU (the one-GPU rehearsal of the multi-GPU step): a few
            # workgroups only.  A rank's spinning all-reduce workgroups hold their CUs' register
            # files; at one workgroup per CU they would leave no CU able to host a peer's conv
            # stack workgroup (3 waves x 168 VGPRs per SIMD), and the peer never reaches its own
            # all-reduce -- a deadlock that separate GPUs cannot have
            # (the physical GPUs of every rank compared: processes pinned with set_device
            # while every GPU stays visible -- farm engines -- share a GPU without it showing
            # in the device count)
            keys = allgather(device_key(self.device))
            shared = len(set(keys)) < len(keys) or _st().local_size > max(1, torch.cuda.device_count())
            max_wg = int(tune("xgmi_shared_wg")) if shared else None
            # (shared goes into create(): the admission self-test runs the exchange geometry --
            # looping or one workgroup per block -- that training will use)
            self.xgmi = X.create(self.rank, self.size, n, self.device, allgather, max_wg=max_wg, shared=shared)
            if self.xgmi is not None:
                self._xgmi_err_host = torch.zeros(4, dtype=torch.int32).pin_memory()
        if self.xgmi is not None:
            self.xgmi_bucket = k
        elif self.comm is None:
            raise RuntimeError("data parallel without RCCL (INTML_COMM=xgmi, or ranks sharing a GPU): the "
                               "fused xGMI all-reduce failed its collective setup / self-test (see stderr)")

    def launch_fused(self, grad: torch.Tensor, opt_args, stream: int, pushed=None, exchanged=False) -> None:
        """The fused all-reduce + optimizer of the xGMI bucket (capturable); ``opt_args``
        cover the whole flat buffer and are offset to the bucket here.  ``pushed``: the flat
        (lo, hi) range the backward already pushed to its owners (push_args); ``exchanged``:
        that range was also all-reduced and updated in the backward (exchange_args)."""
        from . import xgmi as X
        lo, _ = self.buckets[self.xgmi_bucket]
        skip = (pushed[0] - lo, pushed[1] - lo) if pushed else (0, 0)
        self.xgmi.launch(grad.data_ptr() + 4 * lo, stream, opt=X.offset_optim(opt_args, lo), skip=skip,
                         exchanged=bool(pushed) and exchanged)

    def push_args(self, lo: int, hi: int):
        """XgmiPush for an early range [lo, hi) finalised inside the backward, when it lies in
        the xGMI bucket and there are peers to push to; else None."""
        blo = self._xgmi_lo(lo, hi)
        return None if blo is None else self.xgmi.push_args(blo)

    def exchange_args(self, lo: int, hi: int, nblk: int, fbase: int = 0, fused: bool = False, table=None):
        """(push, exchange) XgmiPush pair for an early range [lo, hi) whose reduction table has
        ``nblk`` blocks: the launch that reduces it pushes + flags (mode 1), a later backward
        launch finishes its all-reduce and applies its update (mode 2).  ``fused``: ONE
        XgmiPush doing both in one launch (mode 3, the end-of-backward table).  ``fbase``: the
        table's first block-flag slot.  None when the range is not in the xGMI bucket or the
        flags cannot cover the table.  ``table`` (the split exchange): returns (mode 1, mode 4,
        mode 5) -- the owner half of the exchange in the next backward launch over the table
        blocks this rank owns part of (``table.owned_blocks``; none at size 1), the finish half
        beside the end-of-backward table."""
        blo = self._xgmi_lo(lo, hi)
        if blo is None:
            return None
        if fused:
            return self.xgmi.push_args(blo, mode=3, nblk=nblk, fbase=fbase)
        x1 = self.xgmi.push_args(blo, mode=1, nblk=nblk, fbase=fbase)
        if table is not None:
            own = tuple(table.owned_blocks(blo, self.xgmi.chunk, self.rank)) if self.size > 1 else (0, 0)
            x4 = self.xgmi.push_args(blo, mode=4, nblk=nblk, fbase=fbase, blocks=own)
            x5 = self.xgmi.push_args(blo, mode=5, nblk=nblk, fbase=fbase)
            return None if x1 is None or x4 is None or x5 is None else (x1, x4, x5)
        x2 = self.xgmi.push_args(blo, mode=2, nblk=nblk, fbase=fbase)
        return None if x1 is None or x2 is None else (x1, x2)

    def _xgmi_lo(self, lo: int, hi: int):
        if self.xgmi is None or self.xgmi_bucket is None:
            return None
        blo, bhi = self.buckets[self.xgmi_bucket]
        return None if lo < blo or hi > bhi else blo

    def launch(self, bucket: int, grad: torch.Tensor, stream: torch.cuda.Stream) -> None:
        """Enqueue bucket ``bucket``'s all-reduce on ``stream`` (capturable)."""
        lo, hi = self.buckets[bucket]
        if bucket == self.xgmi_bucket:      # segmented mode: the fused kernel as a plain all-reduce
            self.xgmi.launch(grad.data_ptr() + 4 * lo, stream.cuda_stream if hasattr(stream, "cuda_stream")
                             else stream)
            return
        view = grad[lo:hi]
        buf = self._stage.get(bucket)
        if buf is None:
            self.comm.all_reduce(view, stream=stream)
            return
        with torch.cuda.stream(stream):
            buf.copy_(view)
            self.comm.all_reduce(buf, stream=stream)
            view.copy_(buf)

    # segmented (uncaptured) protocol, same as GradReducer
    def start(self, bucket: int, grad: torch.Tensor):
        self.stream.wait_stream(torch.cuda.current_stream())
        self.launch(bucket, grad, self.stream)

    def wait(self, bucket: int) -> None:
        torch.cuda.current_stream().wait_stream(self.stream)

    def finish(self) -> None:
        torch.cuda.current_stream().wait_stream(self.stream)

    def after_step(self) -> None:
        """Watchdog marker after a step (raises if a peer failed / RCCL reported an error);
        with the xGMI path, the error word of an earlier launch (async copy, no sync)."""
        if self.comm is not None:
            self.comm.mark()
        if self.xgmi is not None:
            if int(self._xgmi_err_host[0]):
                from . import xgmi as X
                raise RuntimeError(X.describe_error(*self._xgmi_err_host.tolist()))
            self._xgmi_err_host.copy_(self.xgmi.err, non_blocking=True)

    def reduce_all(self, grad: torch.Tensor, average: bool = True) -> None:
        for i in range(len(self.buckets)):
            self.start(i, grad)
        self.finish()
        if average:
            grad[: self.store.numel].div_(self.size)


def check_optimizer_plane(optimizer, on_gpu: bool, needs_local_gradient=(), bn_layers=()) -> None:
    """ValueError when the job pins a data plane ``optimizer`` -- or a model with weight
    regularizers (``needs_local_gradient``: its regularized layers' names) -- has no kernels for
    (INTML_XGMI = xgmi / hybrid, or no RCCL communicator).  The model calls it before it builds
    the executor, so nothing has been launched when it raises."""
    if not is_initialized():
        init()
    st = _st()
    if on_gpu and st.comm is not None:
        plane_for_optimizer(forced_plane() or "rccl", optimizer, forced=True, needs_local_gradient=needs_local_gradient,
                            bn_layers=bn_layers)
    elif on_gpu and st.xgmi_only and st.size > 1:
        plane_for_optimizer("xgmi", optimizer, forced=True, needs_local_gradient=needs_local_gradient,
                            bn_layers=bn_layers)


def bn_layer_names(plan) -> tuple:
    """Names of a plan's BatchNormalization layers, in stage order."""
    return tuple(s.bn.name for s in list(plan.convs) + list(plan.denses) if getattr(s, "bn", None) is not None)


def make_reducer(executor, optimizer):
    if not is_initialized():
        init()
    st = _st()
    bb = getattr(optimizer, "bucket_bytes", None) or st.bucket_bytes
    comp = getattr(optimizer, "compression", None)
    on_gpu = getattr(executor.store, "device", torch.device("cpu")).type == "cuda"
    # a model with weight regularizers needs each rank's whole local gradient ahead of the
    # all-reduce, as a clipping optimizer does: ONE bucket, RCCL plane (the layers' names, for errors)
    local = tuple(executor.store.regularized_layers()) if getattr(executor, "regs", None) else ()
    bn = bn_layer_names(executor.plan)
    check_optimizer_plane(optimizer, on_gpu, local, bn)
    if on_gpu and st.comm is not None:
        return NativeGradReducer(executor.store, st.comm, comp, bb, optimizer=optimizer, needs_local_gradient=local,
                                 bn_layers=bn)
    if on_gpu and st.xgmi_only and st.size > 1:
        return NativeGradReducer(executor.store, None, comp, bb, rank=st.rank, size=st.size,
                                 device=executor.store.device, optimizer=optimizer, needs_local_gradient=local,
                                 bn_layers=bn)
    return GradReducer(executor.store, comp, bb, optimizer=optimizer, needs_local_gradient=local)

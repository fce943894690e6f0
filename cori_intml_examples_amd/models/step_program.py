"""The step program of the HIP backend, GPU-free: what a launch, a slab-reduction descriptor
and a reduction group are, and the pure list transformations that place the per-bucket
launches into a step (executor_hip.BatchPlan builds the entries; hip_geometry sizes them)."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, List, NamedTuple, Optional, Tuple

from ..ops.rng import keep_threshold


class Launch(NamedTuple):
    """One entry of BatchPlan.launches.  ``fn(stream)`` issues it; ``tag`` is its stream
    ('main', 'side': only feeds a slab reduction, 'comm'); ``args`` maps role names to the
    kernel argument objects ``fn`` passes (wa / cfg: a wgrad's WgradArgs and its
    (tile, tile, splits) launch configuration; ca / ntc: a conv's ConvMMArgs and n-tiles per
    workgroup; da: a dense GEMM's DenseFwdArgs; stack, head, pro, epi: that launch's struct)."""
    name: str
    fn: Callable
    tag: str = "main"
    args: dict = {}


class RedDesc(NamedTuple):
    """One slab reduction: the arguments of RedTable.add, in its order."""
    slab: int
    stride_s: int
    S: int
    ld: int
    dst_off: int
    numel: int
    type: int
    KH: int = 0
    KW: int = 0
    Cin: int = 0
    Cout: int = 0
    Cs: int = 0


class RedGroup(NamedTuple):
    """A layer's reductions: its parameter span [lo, hi), its descriptors, and the launch
    count after which its partial slabs are final."""
    lo: int
    hi: int
    descs: List[RedDesc]
    ready: int


@dataclass
class Exchange:
    """How a data-parallel step's gradients cross the xGMI plane inside the step (everything
    empty on one GPU and over RCCL); XgmiPush args from the reducer, by where they are launched."""
    early_push: dict = field(default_factory=dict)    # dual launch name -> push of its early table's range
    early_xchg: dict = field(default_factory=dict)    # dual launch name -> (RedTable, XgmiPush): finishes that range
    xchg_end: Optional[tuple] = None     # (RedTable, XgmiPush): ... in a launch of its own after the backward
    xchg_fin: Optional[tuple] = None     # (RedTable, XgmiPush): the split exchange's finish half
    bucket_xchg: dict = field(default_factory=dict)   # bucket -> XgmiPush: its table launch exchanges + updates
    pushed: Optional[Tuple[int, int]] = None          # the early range pushed to its owners
    exchanged: bool = False              # ... and its all-reduce + update finished in table launches


def dropout_pair(rate):
    """(drop_thr, drop_scale) of a dropout rate, as the kernels' argument structs take them."""
    return keep_threshold(rate), 1.0 / (1.0 - rate)


def splice_bucket_launches(launches, inserts, per_bucket):
    """Insert each bucket's launches into the step's launch list.

    ``inserts``: (launch index after which bucket k's partial slabs are final, k);
    ``per_bucket``: [(name pattern, factory k -> fn(stream), stream tag)] appended, in
    order, at that point (slab reduction, then all-reduce / optimizer on the comm stream).
    Returns (new launch list, bucket_ready[k] = index just past bucket k's launches)."""
    out, ready, pos = [], [0] * len(inserts), 0
    for at, k in sorted(inserts):
        out.extend(launches[pos:at])
        pos = at
        for pat, make, tag in per_bucket:
            fn = make(k)
            if fn is not None:          # a factory returns None for buckets it does not apply to
                out.append(Launch(pat % k, fn, tag))
        ready[k] = len(out)
    out.extend(launches[pos:])
    return out, ready


def defer_after_readers(launches, pattern, spans, readers):
    """Move each bucket's comm-stream optimizer (launch name ``pattern % k``) behind the
    last launch that reads a bf16 pack of a parameter in bucket k's span ``spans[k]``.

    The optimizer writes the packs of the weights it updates (pack routes), and a
    comm-stream launch forks after everything issued on main before it: a bucket whose
    slabs are final before a later dgrad / dense-dX launch reads the same layer's pack
    (wide convs have no dual launch, so their dgrad runs after the wgrad) must not update
    that pack while the reader runs.  ``readers``: [(launch name, param lo, param hi)].
    Returns the new launch list (the all-reduce stays where it was, so it still overlaps)."""
    out = list(launches)
    for k, (lo, hi) in enumerate(spans):
        names = [it[0] for it in out]
        name = pattern % k
        if name not in names:
            continue
        at = names.index(name)
        rd = {rn for rn, rlo, rhi in readers if rlo < hi and rhi > lo}
        last = max((i for i, n in enumerate(names) if n in rd), default=-1)
        if last > at:
            item = out.pop(at)
            out.insert(last, item)          # (the pop shifted the reader to last - 1)
    return out


def stream_program(tags, comm=True):
    """The stream schedule of a launch sequence, as a list of ops:
    ("run", stream, i)  launch i on "main" / "comm";
    ("wait", dst, src)  make stream dst wait for everything issued so far on src.

    'main' launches (any tag other than 'comm': 'side' marks the launches that only feed a
    slab reduction) run in order on the current stream.  'comm' launches fork the comm
    stream after everything issued so far (the bucket's slab reduction) -- RCCL and the
    bucket's optimizer run there while main continues the backward -- and the comm stream
    is joined back into main at the end.  ``comm=False``: comm launches run in order on main
    (a linear graph)."""
    ops, used = [], False
    for i, tag in enumerate(tags):
        if tag == "comm" and comm:
            ops.append(("wait", "comm", "main"))
            ops.append(("run", "comm", i))
            used = True
        else:
            ops.append(("run", "main", i))
    if used:
        ops.append(("wait", "main", "comm"))
    return ops


def check_bucket_cover(spans, numel):
    """Bucket (lo, hi) spans must tile [0, numel) exactly: disjoint, no gap, nothing left
    out (every gradient is reduced, all-reduced and updated exactly once)."""
    sp = sorted(spans)
    if not sp or sp[0][0] != 0 or sp[-1][1] != numel or any(a[1] != b[0] for a, b in zip(sp, sp[1:])):
        raise AssertionError("gradient buckets %s do not tile [0, %d)" % (spans, numel))

"""The step program of the HIP backend, GPU-free: the geometry of a model's hidden stages (one
record per stage, the same view for a conv and a dense one), what a launch, a slab-reduction
descriptor and a reduction group are, and the pure list transformations that place the per-bucket
launches into a step (executor_hip.BatchPlan builds the entries; hip_geometry sizes them)."""
from __future__ import annotations

from dataclasses import dataclass, field, replace
from operator import attrgetter
from typing import Callable, List, NamedTuple, Optional, Tuple

from ..ops.rng import keep_threshold


def cdiv(a, b):
    return -(-a // b)


def r8(x):
    return cdiv(x, 8) * 8


@dataclass
class Src:
    """An activation buffer feeding the next stage (for flatten mapping / bwd-through)."""
    kind: str            # 'input' | 'conv' | 'dense' | 'gpool' (the global pooling stage)
    idx: int
    C: int               # logical channels (flatten mapping)
    Cs: int              # padded channel stride
    H: int = 1
    W: int = 1

    @property
    def width(self):
        return self.H * self.W * self.Cs


@dataclass(kw_only=True)
class Stage:
    """What a hidden stage is around its linear kernel (plan.ConvStage / DenseStage), and the view
    its tail launches are written against: ``kind`` 'conv' | 'dense', ``idx`` (ConvGeo.i /
    DenseGeo.j), ``C`` / ``Cs`` the logical and padded output channels, ``lin_grid`` the grid of the
    linear kernel's output and ``out_grid`` the stage output's (pooled; (1, 1) for a dense stage)."""
    relu: bool
    rate: float
    stream: int                    # RNG stream id of the dropout
    act: Optional[str] = None      # hidden activation other than relu / linear
    act_alpha: float = 0.0
    bn: Optional[object] = None    # the stage's BatchNormalization layer
    avg: bool = False              # a conv stage with an AveragePooling2D: dropout(avgpool(A(conv)))
    lin_grid = out_grid = (1, 1)

    @classmethod
    def of(cls, st, *geo):
        """The record of plan stage ``st`` with the positional geometry ``geo``."""
        return cls(*geo, relu=st.relu, rate=st.rate, stream=st.stream, act=st.act, act_alpha=st.act_alpha, bn=st.bn,
                   avg=getattr(st, "pool_kind", None) == "avg")

    @property
    def tag(self):
        """'c0', 'd1': the suffix of the stage's tail launch names."""
        return "%s%d" % (self.kind[0], self.idx)

    @property
    def out_src(self):
        return Src(self.kind, self.idx, self.C, self.Cs, *self.out_grid)

    @property
    def plain(self):
        """Neither a table activation nor a BatchNormalization nor an average pool: the linear kernels
        are the whole stage (the condition for the conv stack and for the head launch running the
        epilogue)."""
        return self.act is None and self.bn is None and not self.avg

    @property
    def dropout_in(self):
        """The launch that carries the stage's dropout in a training step (plan.py): the 'linear'
        kernel iff the stage is plain, bn_apply_fwd ('bn') iff it has a BatchNormalization and no
        table activation, else act_fwd ('act'); pool_fwd ('pool') of an average-pooled stage and of
        the global pooling stage; None at rate 0."""
        if not self.rate > 0:
            return None
        if self.avg or getattr(self, "kind", None) == "gpool":
            return "pool"
        return "linear" if self.plain else "bn" if self.act is None else "act"


def _alias(name):
    return property(attrgetter(name))


@dataclass
class ConvGeo(Stage):
    i: int
    H: int
    W: int
    Cin: int
    Cs_in: int
    Ho: int
    Wo: int
    Cout: int
    Cs_out: int
    Hp: int
    Wp: int
    KH: int
    KW: int
    stride: int
    pad_t: int
    pad_l: int
    pool: bool
    KS: int = 0
    NT: int = 0
    KSd: int = 0
    NTd: int = 0
    pack_fwd: int = 0
    pack_dgrad: int = -1
    kind = "conv"
    idx, C, Cs = _alias("i"), _alias("Cout"), _alias("Cs_out")
    lin_grid = property(lambda g: (g.Ho, g.Wo))
    out_grid = property(lambda g: (g.Hp, g.Wp))

    @property
    def linear(self):
        """The form the stage's conv kernels run in: a BatchNormalization stage's forward, wgrad and
        dgrad are those of a linear, un-pooled, dropout-free stage (the bn.hip launches do the rest);
        an average-pooled stage's are un-pooled and dropout-free with the relu left in the conv kernel
        (the pool.hip launches average, drop and route the gradient back)."""
        if self.bn is None and not self.avg:
            return self
        return replace(self, pool=False, relu=self.relu and self.bn is None, rate=0.0, Hp=self.Ho, Wp=self.Wo,
                       avg=False)


@dataclass
class DenseGeo(Stage):
    j: int
    src: Src
    K: int
    N: int
    Ns: int
    KS: int = 0
    NT: int = 0
    KSb: int = 0
    NTb: int = 0
    pack_fwd: int = 0
    pack_bwd: int = -1
    kind, pool = "dense", False
    idx, C, Cs = _alias("j"), _alias("N"), _alias("Ns")


@dataclass
class GPoolGeo(Stage):
    """The global pooling stage (plan.GlobalPoolStage): no weights, ``src`` the last conv stage's
    output -> [B, Cs]; ``mode`` 'avg' | 'max'.  rate / stream are those of the Dropout behind it."""
    src: Src
    mode: str
    kind, pool, idx = "gpool", False, 0
    C, Cs = property(lambda g: g.src.C), property(lambda g: g.src.Cs)


def gpool_geometry(plan, src):
    """The GPoolGeo of ``plan``'s global pooling stage fed by ``src`` (None: the plan has none)."""
    return GPoolGeo.of(plan.gpool, src, plan.gpool.mode) if getattr(plan, "gpool", None) is not None else None


def stage_geometry(plan):
    """(input Src, [ConvGeo], [DenseGeo], head Src, head activation code) of a models.plan.Plan."""
    shape = plan.input_shape
    H, W, Cin = shape if len(shape) == 3 else (1, 1, shape[0])
    Cs_in = 4 if Cin <= 4 else r8(Cin)
    src = inp = Src("input", 0, Cin, Cs_in, H, W)
    convs, denses = [], []
    for i, cs in enumerate(plan.convs):
        Ho, Wo, Cout = cs.conv_shape
        Hp, Wp, _ = cs.out_shape
        pt, _, pl, _ = cs.pads
        kh, kw = cs.conv.kernel_size
        g = ConvGeo.of(cs, i, H, W, Cin, Cs_in, Ho, Wo, Cout, r8(Cout), Hp, Wp, kh, kw, cs.stride, pt, pl,
                       cs.pool is not None and getattr(cs, "pool_kind", "max") == "max")
        g.KS = cdiv(kh * kw * Cs_in, 32)
        g.NT = cdiv(Cout, 16)
        if i > 0:
            g.KSd = cdiv(kh * kw * g.Cs_out, 32)
            g.NTd = cdiv(Cin, 16)
        convs.append(g)
        H, W, Cin, Cs_in = Hp, Wp, Cout, g.Cs_out
        src = g.out_src
    gp = gpool_geometry(plan, src)
    if gp is not None:
        src = gp.out_src
    for j, ds in enumerate(plan.denses):
        g = DenseGeo.of(ds, j, src, ds.K, ds.N, r8(ds.N))
        if g.K != src.H * src.W * src.C:
            raise ValueError("dense %d input width mismatch" % j)
        g.KS = cdiv(src.width, 32)
        g.NT = cdiv(ds.N, 16)
        if j > 0 or convs:
            g.KSb = cdiv(g.Ns, 32)
            g.NTb = cdiv(src.width, 16)
        denses.append(g)
        src = g.out_src
    hd = plan.head
    if hd.K != src.H * src.W * src.C:
        raise ValueError("head input width mismatch")
    if hd.N > 16:
        raise NotImplementedError("output layers wider than 16 units")
    return inp, convs, denses, src, {None: 0, "sigmoid": 1, "softmax": 2}[hd.activation]


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

"""Float64 oracle of the conv and dense stage kernels, with DERIVED per-element bounds.

Every function works in float64 torch on exactly the values a kernel read -- the saved bf16
activations, argmax codes and gradients, the bf16-rounded weights where the kernel reads a bf16
pack, the fp32 master where it reads that -- and returns the value AND the magnitude sum
``A = sum |a| |b|`` its error bound is built from.  The convolutions are written out tap by tap
on a zero canvas (TF 'same' padding: the odd row / column goes to the bottom / right), on purpose
not through ``ops/reference.py``: tests/test_conv_oracle.py pins them against hand-computed
values and against that reference.

Bounds (``U = 2**-23``, one fp32 ulp = twice the unit roundoff, so that a matrix unit whose
accumulate is not round-to-nearest still passes):

* a value stored in bf16 (stage outputs, routed gradients):
  ``|got - ref| <= 2**-8 |ref| + (K + s + 2) U A`` with K the reduction length and s the number
  of split-K partials.  ReLU and max are 1-Lipschitz: a pooled cell carries the largest of its
  window's four bounds; an element whose reference lies below ``-bound`` under a ReLU is zero in
  the kernel too and carries no error at all.  Dropout scales value and bound alike (the scale
  is the fp32 number the kernels multiply by); the dropout and ReLU masks are exact.
* a gradient stored in fp32: ``|got - ref| <= (P + S + 2) U sum |x| |dy|`` with P the number of
  pixels (rows) summed and S the plan's slab count.
* argmax codes: equal to the first-maximum code wherever the cell is no NEAR TIE -- no other
  window element within the sum of the two elements' bounds of the maximum.  A window whose four
  values are all surely zero under the ReLU is an exact tie that "first maximum" decides: code 0.
  At most ``NEAR_TIE_CAP`` of a stage's pooled cells may be near ties (asserted before the mask
  is used: an input over the cap needs another seed, not another cap).
* padding channels are exactly zero.
"""
from types import SimpleNamespace
from typing import NamedTuple

import numpy as np
import torch

from cori_intml_examples_amd.models.step_program import dropout_pair, stage_geometry
from cori_intml_examples_amd.ops.rng import dropout_keep

U = 2.0 ** -23
BF16_ULP = 2.0 ** -8
NEAR_TIE_CAP = 0.02
F64 = torch.float64


def f64(t):
    return torch.as_tensor(t).detach().to("cpu", F64)


def bf16(t):
    """The bf16 rounding of the weight packs (round to nearest even), as float64."""
    return torch.as_tensor(t).detach().cpu().float().to(torch.bfloat16).to(F64)


# --------------------------------------------------------------------------- convolution
def conv_geometry(H, W, KH, KW, stride, padding):
    """(Ho, Wo, pad_top, pad_left) of a Keras conv."""
    def one(n, k):
        if padding == "same":
            out = -(-n // stride)
            return out, max((out - 1) * stride + k - n, 0) // 2
        return (n - k) // stride + 1, 0
    (Ho, pt), (Wo, pl) = one(H, KH), one(W, KW)
    return Ho, Wo, pt, pl


def _canvas(B, H, W, C, Ho, Wo, KH, KW, s, pt, pl):
    return torch.zeros(B, max(H + pt, (Ho - 1) * s + KH), max(W + pl, (Wo - 1) * s + KW), C, dtype=F64)


def _taps(KH, KW, Ho, Wo, s):
    for ky in range(KH):
        for kx in range(KW):
            yield ky, kx, slice(ky, ky + (Ho - 1) * s + 1, s), slice(kx, kx + (Wo - 1) * s + 1, s)


def conv_forward(x, w, b, stride, padding):
    """x [B,H,W,C], w [KH,KW,C,Co], b [Co] or None -> (z [B,Ho,Wo,Co], A = sum |x||w| + |b|)."""
    x, w = f64(x), f64(w)
    B, H, W, C = x.shape
    KH, KW, _, Co = w.shape
    Ho, Wo, pt, pl = conv_geometry(H, W, KH, KW, stride, padding)
    xp = _canvas(B, H, W, C, Ho, Wo, KH, KW, stride, pt, pl)
    xp[:, pt:pt + H, pl:pl + W] = x
    z = torch.zeros(B, Ho, Wo, Co, dtype=F64)
    A = torch.zeros_like(z)
    for ky, kx, sy, sx in _taps(KH, KW, Ho, Wo, stride):
        z += xp[:, sy, sx] @ w[ky, kx]
        A += xp[:, sy, sx].abs() @ w[ky, kx].abs()
    if b is not None:
        z, A = z + f64(b), A + f64(b).abs()
    return z, A


def conv_dgrad(dy, w, in_hw, stride, padding):
    """dy [B,Ho,Wo,Co], w [KH,KW,C,Co] -> (dx [B,H,W,C], A = sum |dy||w|)."""
    dy, w = f64(dy), f64(w)
    B, Ho, Wo, Co = dy.shape
    KH, KW, C, _ = w.shape
    H, W = in_hw
    Ho2, Wo2, pt, pl = conv_geometry(H, W, KH, KW, stride, padding)
    assert (Ho2, Wo2) == (Ho, Wo), "dY grid does not belong to this input grid"
    dx = _canvas(B, H, W, C, Ho, Wo, KH, KW, stride, pt, pl)
    A = torch.zeros_like(dx)
    for ky, kx, sy, sx in _taps(KH, KW, Ho, Wo, stride):
        dx[:, sy, sx] += dy @ w[ky, kx].t()
        A[:, sy, sx] += dy.abs() @ w[ky, kx].abs().t()
    return dx[:, pt:pt + H, pl:pl + W].clone(), A[:, pt:pt + H, pl:pl + W].clone()


def conv_wgrad(x, dy, ksize, stride, padding):
    """-> (dw [KH,KW,C,Co], db [Co], Aw = sum |x||dy|, Ab = sum |dy|)."""
    x, dy = f64(x), f64(dy)
    B, H, W, C = x.shape
    _, Ho, Wo, Co = dy.shape
    KH, KW = ksize
    Ho2, Wo2, pt, pl = conv_geometry(H, W, KH, KW, stride, padding)
    assert (Ho2, Wo2) == (Ho, Wo)
    xp = _canvas(B, H, W, C, Ho, Wo, KH, KW, stride, pt, pl)
    xp[:, pt:pt + H, pl:pl + W] = x
    dw = torch.zeros(KH, KW, C, Co, dtype=F64)
    Aw = torch.zeros_like(dw)
    d2, a2 = dy.reshape(-1, Co), dy.abs().reshape(-1, Co)
    for ky, kx, sy, sx in _taps(KH, KW, Ho, Wo, stride):
        dw[ky, kx] = xp[:, sy, sx].reshape(-1, C).t() @ d2
        Aw[ky, kx] = xp[:, sy, sx].abs().reshape(-1, C).t() @ a2
    return dw, d2.sum(0), Aw, a2.sum(0)


# --------------------------------------------------------------------------- relu, pool, dropout
def _windows(t):
    """[B,H,W,C] -> [B,H//2,W//2,4,C], window position dy*2+dx; a leftover odd row / column is dropped."""
    B, H, W, C = t.shape
    Hp, Wp = H // 2, W // 2
    return t[:, :2 * Hp, :2 * Wp].reshape(B, Hp, 2, Wp, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, 4, C)


def relu_pool(z, bound, relu, pool):
    """ReLU or linear, then the 2x2 max-pool or none.  Returns a namespace: ``value``, ``bound``
    (per stored element), and for a pooled stage ``code`` (first maximum, dy*2+dx), ``near`` (the
    near-tie mask) and ``zero`` (windows that are all surely zero under the ReLU: code 0)."""
    z, bound = f64(z), f64(bound)
    if relu:
        v = z.clamp(min=0.0)
        be = torch.where(z < -bound, torch.zeros_like(bound), bound)     # surely zero: no error
    else:
        v, be = z, bound
    if not pool:
        return SimpleNamespace(value=v, bound=be, code=None, near=None, zero=None)
    vw, bw = _windows(v), _windows(be)
    pos = torch.arange(4).view(1, 1, 1, 4, 1)
    top = vw.max(dim=3, keepdim=True).values
    code = torch.where(vw == top, pos, torch.full_like(pos, 4)).min(dim=3, keepdim=True).values
    btop = bw.gather(3, code)
    near = (((top - vw) < (btop + bw)) & (pos != code)).any(dim=3)
    zero = (_windows(z) < -_windows(bound)).all(dim=3) if relu else torch.zeros_like(near)
    return SimpleNamespace(value=top.squeeze(3), bound=bw.max(dim=3).values, code=code.squeeze(3).to(torch.uint8),
                           near=near, zero=zero)


def unpool(dp, code, out_hw):
    """Full-resolution dY from the pooled dP and the argmax codes (zero in a leftover row / column)."""
    dp = f64(dp)
    B, Hp, Wp, C = dp.shape
    out = torch.zeros(B, out_hw[0], out_hw[1], C, dtype=F64)
    c = torch.as_tensor(code).cpu().long()
    for k in range(4):
        out[:, k // 2:2 * Hp:2, k % 2:2 * Wp:2] = dp * (c == k)
    return out


def dropout_scale(rate):
    """The fp32 number the kernels multiply a kept element by."""
    return float(np.float32(dropout_pair(rate)[1]))


def dropout(value, bound, rate, seed, stream, step):
    """Dropout over the LOGICAL elements of ``value`` in row-major order: (value, bound, keep)."""
    keep = dropout_keep(value.numel(), rate, seed, stream, step).view(value.shape)
    f = keep.to(F64) * dropout_scale(rate)
    return value * f, bound * f, keep


def through(dx, bound, out, relu, rate, seed, stream, step):
    """A gradient wrt a stage's output routed back through that stage's dropout mask and its ReLU
    mask ``out > 0`` (``out``: the saved stage output, logical channels).  Both masks are exact."""
    if rate > 0:
        dx, bound, _ = dropout(dx, bound, rate, seed, stream, step)
    if relu:
        m = (f64(out) > 0).to(F64)
        dx, bound = dx * m, bound * m
    return dx, bound


# --------------------------------------------------------------------------- dense
def dense_forward(a, w, b, splits=1):
    """-> (z, A = |a||w| + |b|, bound = (K + splits + 2) U A): the bound depends on the split count."""
    a, w = f64(a), f64(w)
    z, A = a @ w, a.abs() @ w.abs()
    if b is not None:
        z, A = z + f64(b), A + f64(b).abs()
    return z, A, (a.shape[1] + splits + 2) * U * A


def dense_dx(dh, w):
    """dH W^T -> (dx [M, K], A)."""
    dh, w = f64(dh), f64(w)
    return dh @ w.t(), dh.abs() @ w.abs().t()


def dense_wgrad(a, dh):
    """-> (dw [K,N], db [N], Aw, Ab)."""
    a, dh = f64(a), f64(dh)
    return a.t() @ dh, dh.sum(0), a.abs().t() @ dh.abs(), dh.abs().sum(0)


def head_probs(a, W, b, act):
    """Head forward on the fp32 master weights -> (probs, tol).  The logits carry
    (K + 3) U A; sigmoid and softmax are at most 1/2-Lipschitz in the largest logit error of the row
    (sum_j |dp_i/dz_j| = 2 p_i (1 - p_i)), taken as 1; 4 U covers expf and the division."""
    z, _, zb = dense_forward(a, W, b)
    if act == "sigmoid":
        p = torch.sigmoid(z)
    elif act == "softmax":
        p = torch.softmax(z, -1)
    else:
        p = z
    tol = zb.max(dim=1, keepdim=True).values.expand_as(p) + 4 * U * (1.0 if act else 1.0 + z.abs())
    return p, tol


# --------------------------------------------------------------------------- comparisons
class Res(NamedTuple):
    name: str
    ratio: float       # worst error / bound (inf: an error where the bound is zero)
    nfail: int
    n: int
    where: str
    excess: float = -1.0     # bf16-stored values: worst (error - 2**-8 |ref|) / accumulation bound; -1: not computed

    @property
    def ok(self):
        return self.nfail == 0

    def __str__(self):
        s = "%-22s worst err/bound %.3g over %d elements" % (self.name, self.ratio, self.n)
        if self.excess >= 0:
            s += " (beyond the bf16 rounding: %.3g of the accumulation bound)" % self.excess
        return s if self.ok else s + " -- %d FAIL, worst at %s" % (self.nfail, self.where)


_AXES = {4: ("image", "row", "col", "channel"), 2: ("row", "column"), 1: ("channel",)}


def _where(idx, shape, axes=None):
    idx = np.unravel_index(int(idx), tuple(shape)) if len(shape) else ()
    names = axes or _AXES.get(len(shape), ["axis%d" % i for i in range(len(shape))])
    return "%s (%s)" % (tuple(int(i) for i in idx), ", ".join("%s %d" % (n, i) for n, i in zip(names, idx)))


def compare(name, got, ref, tol, axes=None):
    got, ref, tol = f64(got), f64(ref), f64(tol)
    assert got.shape == ref.shape == tol.shape, (name, got.shape, ref.shape, tol.shape)
    if got.numel() == 0:
        return Res(name, 0.0, 0, 0, "")
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    ratio = torch.where(err == 0, torch.zeros_like(err),
                        torch.where(tol > 0, err / tol.clamp(min=1e-300), torch.full_like(err, float("inf"))))
    bad = err > tol
    k = int(ratio.reshape(-1).argmax())
    where = "%s: got %.6g, reference %.6g, bound %.3g" % (_where(k, got.shape, axes), float(got.reshape(-1)[k]),
                                                          float(ref.reshape(-1)[k]), float(tol.reshape(-1)[k]))
    return Res(name, float(ratio.reshape(-1)[k]), int(bad.sum()), got.numel(), where)


def compare_bf16(name, got, ref, bound):
    """The bf16 rule; also reports how much of the ACCUMULATION bound alone the error needs once
    the bf16 rounding term is taken off (what a later tightening of U would be judged by)."""
    ref, bound = f64(ref), f64(bound)
    r = compare(name, got, ref, BF16_ULP * ref.abs() + bound)
    over = ((f64(got) - ref).abs() - BF16_ULP * ref.abs()).clamp(min=0.0)
    over = torch.where(bound > 0, over / bound.clamp(min=1e-300), torch.zeros_like(over))
    return r._replace(excess=float(over.max()) if over.numel() else 0.0)


def compare_f32(name, got, ref, A, P, S, axes=None):
    return compare(name, got, ref, (P + S + 2) * U * f64(A), axes)


def exact_zero(name, got):
    """Padding channels: exactly zero."""
    got = f64(got)
    return compare(name, got, torch.zeros_like(got), torch.zeros_like(got))


def compare_codes(name, got, p):
    """[codes off the near ties, codes of the all-zero windows].  Asserts the near-tie share first."""
    got = torch.as_tensor(got).cpu().to(torch.uint8)
    share = float(p.near.double().mean()) if p.near.numel() else 0.0
    assert share <= NEAR_TIE_CAP, "%s: %.2f %% of the pooled cells are near ties (cap %.0f %%): change the input " \
        "seed" % (name, 100 * share, 100 * NEAR_TIE_CAP)
    out = []
    for tag, sel, ref in ((" code", ~p.near, p.code), (" code0", p.zero, torch.zeros_like(p.code))):
        bad = sel & (got != ref)
        where = ""
        if bool(bad.any()):
            k = int(bad.reshape(-1).double().argmax())
            where = "%s: got %d, reference %d" % (_where(k, got.shape), int(got.reshape(-1)[k]), int(ref.reshape(-1)[k]))
        out.append(Res(name + tag, float("inf") if bool(bad.any()) else 0.0, int(bad.sum()), int(sel.sum()), where))
    return out, share


# --------------------------------------------------------------------------- the case matrix
# kind (tests/test_hip_model._build) -> (input channels, dropout rate)
KINDS = {"rpv": (3, 0.3), "mnist": (1, 0.4), "odd": (2, 0.25), "strided": (3, 0.0), "wide_strided": (3, 0.0),
         "wide": (3, 0.2), "rpv_bench": (3, 0.2)}
TAILS = (1, 3, 17, 33, 65)       # one image, an odd count below a 16-row tile, one past 16 / 32 / 64 rows
# (kind, hw, bs): hw = 8 makes the last RPV stage a 2x2 grid pooled to 1x1 and `odd` 11x9 ending in a
# 1x1 pooled grid; the wide kinds are tile-bound and run at 16; rpv_bench is the real geometry of the
# compile-time signature instances at tail sizes a fit() epoch produces
TRAIN = ([(k, 16 if k == "wide_strided" else 8, bs) for k in ("rpv", "mnist", "odd", "strided", "wide_strided")
          for bs in TAILS] + [("rpv", 16, 1), ("rpv", 16, 127), ("rpv_bench", 64, 1), ("rpv_bench", 64, 5)])
# kernel forms the small shapes would never pick: (kind, hw, bs, INTML_TUNE, launch names that must be
# present, launch names that must be absent)
FORCED = ([(k, 8, bs, "conv_stack=0", ("conv_fwd0", "conv_fwd1"), ("conv_stack_fwd",))
           for k in ("rpv", "odd") for bs in (1, 17)]
          + [("rpv", 8, 3, "dual_halo=0", ("wgrad_conv1", "dgrad_conv1", "wgrad_conv2", "dgrad_conv2"), ()),
             ("wide", 16, 3, "conv_big_min=1", ("conv_fwd2", "wgrad_conv2", "dgrad_conv2"), ()),
             # (four row bands need four pooled rows in the last stage: 32x32 images)
             ("rpv", 32, 3, "stack_splits=1", ("conv_stack_fwd",), ()),
             ("rpv", 32, 3, "stack_splits=4", ("conv_stack_fwd",), ())])
EVAL = [(k, 8, bs) for k in ("rpv", "mnist", "odd") for bs in (1, 17)]
GEOMETRIES = sorted(set(TRAIN) | {c[:3] for c in FORCED} | set(EVAL))


def inputs(model, n, seed):
    """randn inputs rounded to bf16 (both signs, unlike rand) and targets for the model's head."""
    rs = np.random.RandomState(seed)
    x = rs.randn(n, *model.input_shape[1:]).astype(np.float32)
    x = torch.tensor(x).to(torch.bfloat16).float().numpy()
    nout = model.output_shape[-1]
    y = (rs.rand(n) > 0.5).astype(np.float32) if nout == 1 else np.eye(nout, dtype=np.float32)[rs.randint(0, nout, n)]
    return x, y


# --------------------------------------------------------------------------- a whole step
def describe(model):
    """The stage geometry of a compiled model (CPU or HIP executor; GPU-free)."""
    ex = model._executor
    inp, convs, denses, head_src, _ = stage_geometry(ex.plan)
    return SimpleNamespace(plan=ex.plan, inp=inp, convs=convs, denses=denses, head_src=head_src, seed=ex.seed)


def weight_reader(model, master):
    """(layer, 'kernel' | 'bias') -> that tensor out of a flat fp32 parameter (or gradient) buffer."""
    master = torch.as_tensor(master).detach().cpu()

    def read(layer, short):
        s = model.store.spec(layer, short)
        return master[s.offset:s.offset + s.numel].view(s.shape)
    return read


W_AXES = ("tap row", "tap col", "in channel", "out channel")


class StepRecord(SimpleNamespace):
    """What one step read and wrote, as CPU tensors with PADDED channel strides where the plan
    pads: x [bs,H,W,Cin] (logical channels); conv_out / conv_code / conv_dy and dense_out /
    dense_dh per stage (the gradients None outside a training step); probs (a predict step);
    w(layer, short) the fp32 weights before the step and g(layer, short) the stored gradients;
    step: the dropout counter the step used; dense_splits[j]; slabs(layer, short): the number of
    partial slabs summed into that gradient."""


def _src_val(d, rec, src):
    if src.kind == "input":
        return f64(rec.x).reshape(rec.x.shape[0], -1)
    if src.kind == "conv":
        return f64(rec.conv_out[src.idx])[..., :d.convs[src.idx].Cout].reshape(rec.x.shape[0], -1)
    return f64(rec.dense_out[src.idx])[:, :d.denses[src.idx].N]


def check_forward(d, rec, training):
    """Every stage output, argmax code and padding channel of a step's forward (dropout only in
    a training step).  Returns ([Res], {stage name: near-tie share})."""
    res, shares = [], {}
    xin = f64(rec.x)
    for g, cs in zip(d.convs, d.plan.convs):
        w = bf16(rec.w(cs.conv, "kernel"))
        b = rec.w(cs.conv, "bias") if cs.conv.use_bias else None
        z, A = conv_forward(xin, w, b, cs.stride, cs.conv.padding)
        assert tuple(z.shape[1:3]) == (g.Ho, g.Wo)
        p = relu_pool(z, (g.KH * g.KW * g.Cin + 1 + 2) * U * A, g.relu, g.pool)
        val, bnd = p.value, p.bound
        if training and g.rate > 0:
            val, bnd, _ = dropout(val, bnd, g.rate, d.seed, g.stream, rec.step)
        got = f64(rec.conv_out[g.i])
        name = "conv%d" % g.i
        res.append(compare_bf16(name + " out", got[..., :g.Cout], val, bnd))
        res.append(exact_zero(name + " out pad", got[..., g.Cout:]))
        if g.pool:
            r, shares[name] = compare_codes(name, rec.conv_code[g.i][..., :g.Cout], p)
            res += r
        xin = got[..., :g.Cout]
    for g, ds in zip(d.denses, d.plan.denses):
        a = _src_val(d, rec, g.src)
        b = rec.w(ds.dense, "bias") if ds.dense.use_bias else None
        z, _, zb = dense_forward(a, bf16(rec.w(ds.dense, "kernel")), b, rec.dense_splits[g.j])
        p = relu_pool(z, zb, g.relu, False)
        val, bnd = p.value, p.bound
        if training and g.rate > 0:
            val, bnd, _ = dropout(val, bnd, g.rate, d.seed, g.stream, rec.step)
        got = f64(rec.dense_out[g.j])
        res.append(compare_bf16("dense%d out" % g.j, got[:, :g.N], val, bnd))
        res.append(exact_zero("dense%d out pad" % g.j, got[:, g.N:]))
    if getattr(rec, "probs", None) is not None:
        hd = d.plan.head
        b = rec.w(hd.dense, "bias") if hd.dense.use_bias else None
        pr, tol = head_probs(_src_val(d, rec, d.head_src), rec.w(hd.dense, "kernel"), b, hd.activation)
        res.append(compare("probs", rec.probs, pr, tol))
    return res, shares


def _stage(d, src):
    return {"input": [None], "conv": d.convs, "dense": d.denses}[src.kind][src.idx]


def _route(d, rec, name, dx, bound, pg, res):
    """Compare dx (+ bound) wrt stage pg's output, through pg's masks, with the stored gradient."""
    if pg.kind == "conv":
        out, got = f64(rec.conv_out[pg.i])[..., :pg.Cout], f64(rec.conv_dy[pg.i])
    else:
        out, got = f64(rec.dense_out[pg.j])[:, :pg.N], f64(rec.dense_dh[pg.j])
    dx, bound = through(dx.reshape(out.shape), bound.reshape(out.shape), out, pg.relu, pg.rate, d.seed, pg.stream,
                        rec.step)
    res.append(compare_bf16(name, got[..., :pg.C], dx, bound))
    res.append(exact_zero(name + " pad", got[..., pg.C:]))


def check_backward(d, rec):
    """Every weight / bias gradient and every routed gradient of a training step, each from the
    saved inputs of the kernel that wrote it."""
    res = []
    bs = rec.x.shape[0]
    for g, ds in reversed(list(zip(d.denses, d.plan.denses))):
        a, dh = _src_val(d, rec, g.src), f64(rec.dense_dh[g.j])[:, :g.N]
        dw, db, Aw, Ab = dense_wgrad(a, dh)
        name = "dense%d" % g.j
        res.append(compare_f32(name + " wgrad", rec.g(ds.dense, "kernel"), dw, Aw, bs, rec.slabs(ds.dense, "kernel"),
                               ("in", "out")))
        if ds.dense.use_bias:
            res.append(compare_f32(name + " bgrad", rec.g(ds.dense, "bias"), db, Ab, bs, rec.slabs(ds.dense, "bias")))
        pg = _stage(d, g.src)
        if pg is not None:
            dx, A = dense_dx(dh, bf16(rec.w(ds.dense, "kernel")))
            _route(d, rec, "%s dX>%s%d" % (name, pg.kind, pg.idx), dx, (g.N + 1 + 2) * U * A, pg, res)
    for g, cs in reversed(list(zip(d.convs, d.plan.convs))):
        xin = f64(rec.x) if g.i == 0 else f64(rec.conv_out[g.i - 1])[..., :g.Cin]
        dy = f64(rec.conv_dy[g.i])[..., :g.Cout]
        if g.pool:
            dy = unpool(dy, rec.conv_code[g.i][..., :g.Cout], (g.Ho, g.Wo))
        dw, db, Aw, Ab = conv_wgrad(xin, dy, (g.KH, g.KW), cs.stride, cs.conv.padding)
        name, P = "conv%d" % g.i, bs * g.Ho * g.Wo
        res.append(compare_f32(name + " wgrad", rec.g(cs.conv, "kernel"), dw, Aw, P, rec.slabs(cs.conv, "kernel"),
                               W_AXES))
        if cs.conv.use_bias:
            res.append(compare_f32(name + " bgrad", rec.g(cs.conv, "bias"), db, Ab, P, rec.slabs(cs.conv, "bias")))
        if g.i > 0:
            dx, A = conv_dgrad(dy, bf16(rec.w(cs.conv, "kernel")), (g.H, g.W), cs.stride, cs.conv.padding)
            _route(d, rec, "%s dgrad>conv%d" % (name, g.i - 1), dx, (g.KH * g.KW * g.Cout + 1 + 2) * U * A,
                   d.convs[g.i - 1], res)
    return res


def report(tag, results, shares=None):
    """One line per quantity; returns the failure messages."""
    for r in results:
        print("%-28s %s" % (tag, r))
    for k, v in (shares or {}).items():
        print("%-28s %-22s near-tie share %.3f %%" % (tag, k, 100 * v))
    return ["%s %s" % (tag, r) for r in results if not r.ok]

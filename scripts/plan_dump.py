"""Dump the step plans of the HIP backend as one JSON document, to compare two commits.

    python scripts/plan_dump.py --out plans.json [--tunes scripts/plan_dump_tunes.txt]
    python scripts/plan_dump.py --compare a.json b.json

For every line of the tune file (an INTML_TUNE string; ``default`` = none) and every
(model, mode, batch size) below, a fresh model's plan is built through
``HipExecutor._plan_for`` -- no step runs -- and reduced to what decides the step: the
(name, tag) launch list, the kernel entry points and scalars each launch callable binds, every
public scalar of every argument struct in ``Launch.args``
(nested structs included, device addresses as buffer name + offset: the plan's public buffers by
name, any other tensor reachable from the plan or the executor as ``t<k>[shape,dtype]``, numbered
by first reference in the dump, so the name does not depend on the attribute that holds it), the
wgrad slab shapes,
the bucket spans and table block counts, the reduction groups, the early reductions and the
plan's path flags.  It reads only ``Launch.args`` and public attributes, so the same file runs
on any commit that has them; a host-side refactor must leave the document unchanged.

Not in the dump: knobs of the data-parallel step (they need a live reducer) and values read
when a launch is issued rather than when the plan is built (early_rfirst, opt_tiles, skip).
"""
import argparse
import dataclasses
import json
import os
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = ("train", "eval", "predict")


def models():
    """name -> (builder, batch sizes, weighted plans too): the three bench models, the odd-shaped test
    model (also with AMSGrad, a STANDALONE_KINDS kind), and small models with table activations,
    BatchNormalization stages, weight regularizers and gradient clipping."""
    from cori_intml_examples_amd import optim, regularizers
    from cori_intml_examples_amd.apps import zoo
    from cori_intml_examples_amd.models import (ELU, Activation, BatchNormalization, Conv2D, Dense, Dropout, Flatten,
                                                Input, LeakyReLU, MaxPooling2D, Model)

    def done(inp, out, opt="Adam", loss="categorical_crossentropy", **kw):
        m = Model(inp, out, device="cuda", **kw)
        m.compile(optimizer=opt, loss=loss, metrics=["accuracy"])
        return m

    def odd(opt="Adam"):  # tests/test_hip_model.py "odd": 19x17x2, odd channels and pooled grid, two denses
        inp = Input(shape=(19, 17, 2))
        h = MaxPooling2D((2, 2))(Conv2D(5, (3, 3), activation="relu", padding="same")(inp))
        h = MaxPooling2D((2, 2))(Conv2D(12, (3, 3), activation="relu")(h))
        h = Dropout(0.2)(Dense(20, activation="relu")(Flatten()(h)))
        return done(inp, Dense(3, activation="softmax")(Dense(9, activation="relu")(h)), opt)

    def act():          # the dropout on a pooled tanh conv and on a LeakyReLU dense; an un-pooled ELU conv
        inp = Input(shape=(19, 17, 2))
        h = Dropout(0.2)(MaxPooling2D((2, 2))(Conv2D(5, (3, 3), activation="tanh", padding="same")(inp)))
        h = ELU(0.5)(Conv2D(12, (3, 3))(h))
        h = Dropout(0.2)(LeakyReLU(0.3)(Dense(20)(Flatten()(h))))
        return done(inp, Dense(3, activation="softmax")(Dense(9, activation="relu")(h)))

    def bn_odd():       # tests/helpers/bn_models.py odd, drop 0.2: BN + relu, BN + tanh, and a gamma-free
        inp = Input(shape=(19, 17, 2))                 # dense BN + tanh whose act_fwd carries the dropout
        h = Activation("relu")(BatchNormalization()(Conv2D(5, (3, 3), padding="same")(inp)))
        h = MaxPooling2D((2, 2))(h)
        h = Activation("tanh")(BatchNormalization()(Conv2D(12, (3, 3))(h)))
        h = Dropout(0.2)(Activation("tanh")(BatchNormalization(scale=False)(Dense(20)(Flatten()(h)))))
        return done(inp, Dense(3, activation="softmax")(Dense(9, activation="relu")(h)))

    def bn_tiny():      # tests/helpers/bn_models.py tiny, drop 0.25: the dropout on a pooled conv + BN stage
        h = inp = Input(shape=(16, 16, 3))
        for c in (4, 8, 8):
            h = Activation("relu")(BatchNormalization()(Conv2D(c, kernel_size=(3, 3), padding="same")(h)))
            h = MaxPooling2D(pool_size=(2, 2))(h)
        h = Flatten()(Dropout(0.25)(h))
        h = Dropout(0.25)(Activation("relu")(BatchNormalization()(Dense(16)(h))))
        return done(inp, Dense(1, activation="sigmoid")(h), loss="binary_crossentropy", name="RPVClassifier")

    def reg_clip():     # rpv_cnn((32, 32, 3), [8, 16], [32], 0.2) with regularized kernels and a clipping Adam
        h = inp = Input(shape=(32, 32, 3))
        for c in (8, 16):
            h = Conv2D(c, kernel_size=(3, 3), activation="relu", padding="same",
                       kernel_regularizer=regularizers.l2(1e-2))(h)
            h = MaxPooling2D(pool_size=(2, 2))(h)
        h = Flatten()(Dropout(0.2)(h))
        h = Dropout(0.2)(Dense(32, activation="relu", kernel_regularizer=regularizers.l1_l2(1e-3, 1e-2))(h))
        return done(inp, Dense(1, activation="sigmoid")(h), optim.Adam(clipnorm=1.0, clipvalue=0.5),
                    "binary_crossentropy", name="RPVClassifier")

    return {
        "rpv": (lambda: zoo.rpv_cnn((64, 64, 3), conv_sizes=[16, 32, 64], fc_sizes=[128], dropout=0.2,
                                    optimizer="Adam", lr=1e-3, device="cuda"), (128, 5), False),
        "mnist": (lambda: zoo.mnist_cnn(32, 64, 128, 0.25, 0.5, lr=1.0, device="cuda"), (128, 5), False),
        "legacy": (lambda: zoo.rpv_legacy_cnn((64, 64, 3), device="cuda"), (8,), False),
        "odd": (odd, (128, 5), True),
        "act": (act, (32, 5), False),
        "bn_odd": (bn_odd, (32, 5), False),
        "bn_tiny": (bn_tiny, (32, 5), False),
        "reg_clip": (reg_clip, (32, 5), False),
        "amsgrad": (lambda: odd(optim.Adam(amsgrad=True)), (32, 5), False),
    }


class Dumper:
    """Reduces one plan's objects to JSON values; device addresses become buffer name + offset."""

    def __init__(self, bp):
        self.kmod = type(bp.ex.K.WgradArgs()).__module__
        self.bufs = []
        ex = bp.ex

        def add(name, t):
            if t is None:
                return
            if isinstance(t, (list, tuple)):
                for i, u in enumerate(t):
                    add("%s[%d]" % (name, i), u)
            elif hasattr(t, "data_ptr") and t.numel():
                self.bufs.append((t.data_ptr(), t.numel() * t.element_size(), name))

        for name in ("xb", "yb", "wb", "conv_out", "conv_code", "conv_dy", "dense_out", "dense_part", "dense_dh",
                     "probs", "head_wslab", "head_bslab", "srcidx", "wgrad_slabs"):
            add(name, getattr(bp, name, None))
        for name in ("state", "arena", "slots", "routes"):
            add("ex." + name, getattr(ex, name, None))
        add("store.master", ex.store.master)
        add("store.grad", ex.store.grad)
        # every other tensor reachable from the plan and the executor: (base, bytes, shape, dtype)
        self.others, self.numbered, self.unnamed = set(), {}, set()
        seen = set()

        def walk(v):
            if id(v) in seen:
                return
            seen.add(id(v))
            if hasattr(v, "data_ptr"):
                if v.numel():
                    self.others.add((v.data_ptr(), v.numel() * v.element_size(), tuple(v.shape),
                                     str(v.dtype).replace("torch.", "")))
            elif isinstance(v, (list, tuple)):
                for u in v:
                    walk(u)
            elif isinstance(v, dict):
                for u in v.values():
                    walk(u)
            elif isinstance(v, SimpleNamespace) or (dataclasses.is_dataclass(v) and not isinstance(v, type)):
                walk(vars(v))

        walk(vars(bp))
        walk(vars(ex))

    def address(self, v):
        for base, nbytes, name in self.bufs:
            if base <= v < base + nbytes:
                return "%s+%d" % (name, v - base)
        # the smallest reachable tensor that holds the address, whichever attribute holds the tensor
        hit = min((t for t in self.others if t[0] <= v < t[0] + t[1]), key=lambda t: (t[1], t[0], t[2], t[3]),
                  default=None)
        if hit is None:
            self.unnamed.add(v)
            return "ptr"                  # some other device address: non-null
        k = self.numbered.setdefault(hit, len(self.numbered))
        return "t%d[%s,%s]+%d" % (k, "x".join(map(str, hit[2])), hit[3], v - hit[0])

    def value(self, v):
        if isinstance(v, bool) or v is None or isinstance(v, str):
            return v
        if isinstance(v, int):
            return v if v < (1 << 32) else self.address(v)
        if isinstance(v, float):
            return repr(v)
        if isinstance(v, (list, tuple)):
            return [self.value(u) for u in v]
        if isinstance(v, dict):
            return {str(k): self.value(u) for k, u in v.items()}
        if type(v).__module__ == self.kmod:
            return self.struct(v)
        if hasattr(v, "shape"):
            return {"shape": list(v.shape)}
        return type(v).__name__

    def struct(self, o):
        out = {"_": type(o).__name__}
        for f in dir(o):
            if not f.startswith("_"):
                v = getattr(o, f)
                if not callable(v):
                    out[f] = self.value(v)
        return out


def dump_plan(bp, unnamed=None):
    d = Dumper(bp)
    out = {
        "launches": [[it.name, it.tag] for it in bp.launches],
        "args": [{role: d.value(v) for role, v in sorted(it.args.items())} for it in bp.launches],
        # what a launch callable binds besides its structs: the kernel entry points it names and
        # its scalar defaults (n-tiles, wave counts, grid orders)
        "calls": [[list(it.fn.__code__.co_names),
                   [v for v in (it.fn.__defaults__ or ()) if isinstance(v, (bool, int, str, tuple))]]
                  for it in bp.launches],
        "wgrad_slabs": [[list(t.shape) if t is not None else None for t in pair] for pair in bp.wgrad_slabs],
        "buckets": [[lo, hi, d.value(tab)] for lo, hi, tab in bp.bucket_tables],
        "bucket_ready": list(bp.bucket_ready),
        "red_groups": [[g.lo, g.hi, g.ready, [d.value(tuple(x)) for x in g.descs]] for g in bp.red_groups],
        "early_red": {nm: [d.value(e[0]), list(e[1]), bool(e[2])] for nm, e in bp.early_red.items()},
        "dense_fused_opt": [n for _, n in bp.dense_fused_opt],
        "pack_readers": [list(r) for r in bp.pack_readers],
    }
    for name in ("pro_free", "optim_fused", "dense_opt_ok", "dense_opt_all", "dense_splits", "stack_splits",
                 "head_blocks", "weighted", "comm_in_graph", "optim_on_comm"):
        out[name] = d.value(getattr(bp, name, None))
    if unnamed is not None:
        unnamed.append(len(d.unnamed))
    return out


def build_all(tunes):
    """{tune: {model/mode/bs[/w]: plan dump}}, the seconds spent inside _plan_for, and how many
    distinct device addresses per plan key matched no tensor (rendered "ptr")."""
    import gc
    import torch
    from cori_intml_examples_amd.utils import set_random_seed
    doc, secs, unnamed = {}, 0.0, {}
    zoo_models = models()
    for tv in tunes:
        os.environ["INTML_TUNE"] = "" if tv == "default" else tv
        plans = doc.setdefault(tv, {})
        for name, (make, sizes, weighted) in zoo_models.items():
            set_random_seed(1234)
            ex = make()._executor
            for mode in MODES:
                for bs in sizes:
                    for w in ((False, True) if weighted else (False,)):
                        t0 = time.perf_counter()
                        bp = ex._plan_for(bs, mode, True) if w else ex._plan_for(bs, mode)
                        torch.cuda.synchronize()
                        secs += time.perf_counter() - t0
                        n = []
                        plans["%s/%s/%d%s" % (name, mode, bs, "/w" if w else "")] = dump_plan(bp, n)
                        unnamed[name] = unnamed.get(name, 0) + n[0]
            del ex, bp
            gc.collect()
    os.environ.pop("INTML_TUNE", None)
    return doc, secs, unnamed


def compare(pa, pb):
    with open(pa) as fa, open(pb) as fb:
        a, b = json.load(fa), json.load(fb)
    keys = sorted({(t, p) for doc in (a, b) for t, plans in doc.items() for p in plans})
    diff = [k for k in keys if a.get(k[0], {}).get(k[1]) != b.get(k[0], {}).get(k[1])]
    launches = [sum(len(p["launches"]) for plans in doc.values() for p in plans.values()) for doc in (a, b)]
    print("tune strings: %d / %d, plans: %d / %d, launches: %d / %d" % (
        len(a), len(b), sum(map(len, a.values())), sum(map(len, b.values())), launches[0], launches[1]))
    print("plans that differ: %d" % len(diff))
    for t, p in diff[:20]:
        print("  differs: %s  [%s]" % (p, t))
    return 1 if diff else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tunes", default=os.path.join(ROOT, "scripts", "plan_dump_tunes.txt"))
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar="JSON")
    args = ap.parse_args()
    if args.compare:
        return compare(*args.compare)
    with open(args.tunes) as fh:
        tunes = [ln.strip() for ln in fh if ln.strip()]
    doc, secs, unnamed = build_all(tunes)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, sort_keys=True, separators=(",", ":"))
    print("%d tune strings, %d plans, plan build %.2f s -> %s" % (
        len(doc), sum(map(len, doc.values())), secs, args.out))
    print("addresses that match no tensor (\"ptr\"), per model: %s" % (
        ", ".join("%s %d" % kv for kv in sorted(unnamed.items()) if kv[1]) or "none"))
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Dump the step plans of the HIP backend as one JSON document, to compare two commits.

    python scripts/plan_dump.py --out plans.json [--tunes scripts/plan_dump_tunes.txt]
    python scripts/plan_dump.py --compare a.json b.json

For every line of the tune file (an INTML_TUNE string; ``default`` = none) and every
(model, mode, batch size) below, a fresh model's plan is built through
``HipExecutor._plan_for`` -- no step runs -- and reduced to what decides the step: the
(name, tag) launch list, the kernel entry points and scalars each launch callable binds, every
public scalar of every argument struct in ``Launch.args``
(nested structs included, device addresses as buffer name + offset), the wgrad slab shapes,
the bucket spans and table block counts, the reduction groups, the early reductions and the
plan's path flags.  It reads only ``Launch.args`` and public attributes, so the same file runs
on any commit that has them; a host-side refactor must leave the document unchanged.

Not in the dump: knobs of the data-parallel step (they need a live reducer) and values read
when a launch is issued rather than when the plan is built (early_rfirst, opt_tiles, skip).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = ("train", "eval", "predict")


def models():
    """name -> (builder, batch sizes): the three bench models and the odd-shaped test model."""
    from cori_intml_examples_amd import Conv2D, Dense, Dropout, Flatten, Input, MaxPooling2D, Model
    from cori_intml_examples_amd.apps import zoo

    def odd():          # tests/test_hip_model.py "odd": 19x17x2, odd channels and pooled grid, two denses
        inp = Input(shape=(19, 17, 2))
        h = MaxPooling2D((2, 2))(Conv2D(5, (3, 3), activation="relu", padding="same")(inp))
        h = MaxPooling2D((2, 2))(Conv2D(12, (3, 3), activation="relu")(h))
        h = Dropout(0.2)(Dense(20, activation="relu")(Flatten()(h)))
        out = Dense(3, activation="softmax")(Dense(9, activation="relu")(h))
        m = Model(inp, out, device="cuda")
        m.compile(optimizer="Adam", loss="categorical_crossentropy", metrics=["accuracy"])
        return m

    return {
        "rpv": (lambda: zoo.rpv_cnn((64, 64, 3), conv_sizes=[16, 32, 64], fc_sizes=[128], dropout=0.2,
                                    optimizer="Adam", lr=1e-3, device="cuda"), (128, 5)),
        "mnist": (lambda: zoo.mnist_cnn(32, 64, 128, 0.25, 0.5, lr=1.0, device="cuda"), (128, 5)),
        "legacy": (lambda: zoo.rpv_legacy_cnn((64, 64, 3), device="cuda"), (8,)),
        "odd": (odd, (128, 5)),
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

    def value(self, v):
        if isinstance(v, bool) or v is None or isinstance(v, str):
            return v
        if isinstance(v, int):
            if v < (1 << 32):
                return v
            for base, nbytes, name in self.bufs:
                if base <= v < base + nbytes:
                    return "%s+%d" % (name, v - base)
            return "ptr"                  # some other device address: non-null
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


def dump_plan(bp):
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
    return out


def build_all(tunes):
    """{tune: {model/mode/bs: plan dump}}, and the seconds spent inside _plan_for."""
    import gc
    import torch
    from cori_intml_examples_amd.utils import set_random_seed
    doc, secs = {}, 0.0
    zoo_models = models()
    for tv in tunes:
        os.environ["INTML_TUNE"] = "" if tv == "default" else tv
        plans = doc.setdefault(tv, {})
        for name, (make, sizes) in zoo_models.items():
            set_random_seed(1234)
            ex = make()._executor
            for mode in MODES:
                for bs in sizes:
                    t0 = time.perf_counter()
                    bp = ex._plan_for(bs, mode)
                    torch.cuda.synchronize()
                    secs += time.perf_counter() - t0
                    plans["%s/%s/%d" % (name, mode, bs)] = dump_plan(bp)
            del ex, bp
            gc.collect()
    os.environ.pop("INTML_TUNE", None)
    return doc, secs


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
    doc, secs = build_all(tunes)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, sort_keys=True, separators=(",", ":"))
    print("%d tune strings, %d plans, plan build %.2f s -> %s" % (
        len(doc), sum(map(len, doc.values())), secs, args.out))
    return 0


if __name__ == "__main__":
    sys.exit(main())

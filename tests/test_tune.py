"""The INTML_TUNE knob table (utils/tune.py): the table itself, its agreement with every
``tune(...)`` call in the package, parsing, validation of the environment string, per-layer
resolution, the generated docs/TUNES.md and the committed sweep files.  No GPU.

Expected values are written out by hand from the rules in utils/tune.py's docstrings, not
computed by the code under test."""
import ast
import os

import pytest

from cori_intml_examples_amd.utils import tune as T
from cori_intml_examples_amd.utils.tune import KNOBS, tune

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cori_intml_examples_amd")
BY_KEY = {k.key: k for k in KNOBS}


@pytest.fixture
def env(monkeypatch):
    monkeypatch.delenv("INTML_TUNE", raising=False)
    return lambda s: monkeypatch.setenv("INTML_TUNE", s)


# ----------------------------------------------------------------------------- the table
def test_table_sanity():
    keys = [k.key for k in KNOBS]
    assert len(keys) == len(set(keys))
    for k in KNOBS:
        assert k.doc.strip() and k.kind in ("exact", "path", "ablation"), k.key
        assert k.per_layer in ("", T.LAYER, T.LAYER_ONLY), k.key
        assert type(k.default) in (bool, int, float, str), k.key
        assert not k.auto or k.default == 0, k.key
        for v in (k.layer_defaults or {}).values():
            assert k.per_layer and type(v) is type(k.default), k.key
    for key in ("skip", "pro_dbg", "stack_dbg"):
        assert BY_KEY[key].kind == "ablation"
    assert type(BY_KEY["dense_opt"].default) is str


def _tune_calls():
    """(file, line, Call) of every call of a function named ``tune`` in the package."""
    for dirpath, _, files in os.walk(PKG):
        for f in files:
            if not f.endswith(".py"):
                continue
            path = os.path.join(dirpath, f)
            with open(path) as fh:
                tree = ast.parse(fh.read(), path)
            for node in ast.walk(tree):
                if isinstance(node, ast.Call):
                    fn = node.func
                    name = fn.id if isinstance(fn, ast.Name) else fn.attr if isinstance(fn, ast.Attribute) else None
                    if name == "tune":
                        yield os.path.relpath(path, ROOT), node.lineno, node


def test_call_sites_agree_with_table():
    read = set()
    for path, line, call in _tune_calls():
        where = "%s:%d" % (path, line)
        assert len(call.args) == 1, where + ": tune() takes the key alone (no default argument)"
        key = call.args[0]
        assert isinstance(key, ast.Constant) and isinstance(key.value, str), where + ": key must be a string literal"
        assert key.value in BY_KEY, where + ": unregistered key " + key.value
        assert [kw.arg for kw in call.keywords] in ([], ["layer"]), where
        assert bool(call.keywords) == bool(BY_KEY[key.value].per_layer), where + ": layer= goes with per-layer knobs"
        read.add(key.value)
    assert len(read) > 50                       # the walk found the call sites at all
    assert sorted(set(BY_KEY) - read) == [], "registered knobs no call reads"


def test_unregistered_key_at_a_call_site_is_a_keyerror(env):
    with pytest.raises(KeyError):
        tune("no_such_knob")
    with pytest.raises(KeyError):
        tune("wgrad_splits")                    # per-layer: needs layer=
    with pytest.raises(KeyError):
        tune("conv_stack", layer=1)


# ----------------------------------------------------------------------------- parsing
@pytest.mark.parametrize("text,want", [("0", False), ("false", False), ("off", False), ("no", False), ("", False),
                                        ("False", False), ("1", True), ("yes", True)])
def test_bool_values(text, want, env):
    assert BY_KEY["conv_stack"].default is True and BY_KEY["head_generic"].default is False
    for key in ("conv_stack", "head_generic"):
        env("%s=%s" % (key, text))
        assert tune(key) is want


def test_int_float_string_values_and_defaults(env, monkeypatch):
    env("dense_waves= 64 ,wt=0,dense_opt=1,xchg_at=end,skip=head/reduce_b0,comm_fork=0")
    assert tune("dense_waves") == 64 and type(tune("dense_waves")) is int
    assert tune("wt") == 0 and type(tune("wt")) is int
    assert tune("dense_opt") == "1" and tune("xchg_at") == "end" and tune("skip") == "head/reduce_b0"
    assert tune("comm_fork") == "0"
    # a float default parses as float (no registered knob has one)
    v = T.Knob("f", 0.5, "path", "doc").parse("2")
    assert v == 2.0 and type(v) is float
    monkeypatch.delenv("INTML_TUNE")
    # unset: the registered default, with its type
    for key, want in (("conv_stack", True), ("head_generic", False), ("wt", 7), ("dense_waves", 2048),
                      ("red_lanes", 16), ("stack_spec", 2), ("dense_opt", "auto"), ("xchg_at", "dual"),
                      ("skip", ""), ("stack_splits", 0), ("dx_ntc", 0), ("conv_big_min", 512)):
        assert tune(key) == want and type(tune(key)) is type(want), key


# ----------------------------------------------------------------------------- validation
def test_unknown_key_names_the_closest(env):
    env("wgrad_split=512")
    with pytest.raises(ValueError) as e:
        tune("conv_stack")
    assert "wgrad_split" in str(e.value) and "wgrad_splits" in str(e.value)
    assert "'wgrad_split'" in str(e.value)      # the offending key itself, not only its neighbour


@pytest.mark.parametrize("text", ["conv_stack1=0", "foo", "conv_stack=1,foo", "dgrad_tm=2", "wgrad_fit=0",
                                  "wgrad_rowdiv=0", "wgrad_tile_order=1", "wgrad_ring=2", "=1", "wgrad_splits2x=1"])
def test_rejected_strings(text, env):
    env(text)
    with pytest.raises(ValueError):
        tune("conv_stack")
    with pytest.raises(ValueError):             # not cached as accepted
        tune("conv_stack")


def test_value_of_the_wrong_type_names_its_key(env):
    env("conv_stack=0,dense_waves=many")
    with pytest.raises(ValueError) as e:
        tune("conv_stack")
    assert "dense_waves=many" in str(e.value)


def test_accepted_strings_and_change_takes_effect(env):
    env("dense_waves=64,")
    assert tune("dense_waves") == 64
    env("")
    assert tune("dense_waves") == 2048
    env("dense_waves=64,,  ,wt=3")
    assert (tune("dense_waves"), tune("wt")) == (64, 3)
    env("dense_waves=128")
    assert (tune("dense_waves"), tune("wt")) == (128, 7)
    env("dgrad_tm1=2,wgrad_fit0=0")             # knobs that exist only with a layer number
    assert [tune("dgrad_tm", layer=i) for i in range(3)] == [0, 2, 0]
    assert [tune("wgrad_fit", layer=i) for i in range(3)] == [False, True, True]


# ----------------------------------------------------------------------------- per-layer knobs
def test_per_layer_resolution(env):
    env("wgrad_splits2=128")
    assert [tune("wgrad_splits", layer=i) for i in range(3)] == [0, 0, 128]
    env("wgrad_splits=64,wgrad_splits1=192")
    assert [tune("wgrad_splits", layer=i) for i in range(3)] == [64, 192, 64]
    env("wgrad_splits=64,wgrad_splits1=0")      # 0 = auto falls through, as the `or` chain did
    assert [tune("wgrad_splits", layer=i) for i in range(3)] == [64, 64, 64]
    env("")
    assert [tune("wgrad_block_px", layer=i) for i in range(3)] == [512, 256, 256]
    assert [tune("wgrad_max_rows", layer=i) for i in range(3)] == [8, 8, 8]
    env("wgrad_block_px=128")
    assert [tune("wgrad_block_px", layer=i) for i in range(3)] == [128, 128, 128]
    env("wgrad_block_px=128,wgrad_block_px0=64,wgrad_max_rows12=0")
    assert [tune("wgrad_block_px", layer=i) for i in range(3)] == [64, 128, 128]
    assert tune("wgrad_max_rows", layer=12) == 0 and tune("wgrad_max_rows", layer=1) == 8   # not a 0 = auto knob


# ----------------------------------------------------------------------------- docs, sweep files
def test_generated_docs_are_current():
    with open(os.path.join(ROOT, "docs", "TUNES.md")) as fh:
        assert fh.read() == T.markdown()


def _sweep_lines():
    out = [("bench.py", "xchg_at=end"), ("bench.py", "pro_free=0,xchg_at=end")]
    for name in ("tunes_default.txt", "tunes_rpv_wsplits.txt", "plan_dump_tunes.txt"):
        with open(os.path.join(ROOT, "scripts", name)) as fh:
            lines = [ln.strip() for ln in fh]
        assert lines, name
        out += [(name, ln) for ln in lines]
    return out


def test_sweep_files_parse(env):
    for name, line in _sweep_lines():
        env("" if line == "default" else line)
        try:
            tune("conv_stack")
        except ValueError as e:
            raise AssertionError("%s: %r: %s" % (name, line, e))

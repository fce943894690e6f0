"""The default training step programs of the three bench models, pinned: the (name, stream tag)
sequence BatchPlan builds, and the kernel argument roles each launch carries in Launch.args.
Plan build only -- no step runs.  A reordering of the step shows up here as a one-line diff.

The sequences were recorded from the commit before the step builder was split into stages
(profiles/step_program_snapshot.txt), not from the code under test.  Those of bn_odd, act and
reg_clip (the models of scripts/plan_dump.py with BatchNormalization stages, table activations,
and weight regularizers + gradient clipping) were recorded at batch 8 from the commit before the
stage record (profiles/stage_record_plan_compare.txt), not from the code under test either."""
import importlib.util
import os

import pytest

from cori_intml_examples_amd.apps import zoo
from cori_intml_examples_amd.models.executor_hip import Launch

pytestmark = pytest.mark.gpu

SEQUENCES = {
    "rpv": (128, [
        ("conv_stack_fwd", "main"), ("dense_fwd0", "main"), ("head", "main"), ("dense_bwd0", "main"),
        ("wgrad_dgrad_conv2", "main"), ("wgrad_dgrad_conv1", "main"), ("wgrad_conv0", "side"), ("reduce_b0", "side")]),
    "mnist": (128, [
        ("conv_stack_fwd", "main"), ("dense_fwd0", "main"), ("head", "main"), ("dense_bwd0", "main"),
        ("wgrad_dgrad_conv1", "main"), ("wgrad_conv0", "side"), ("reduce_b0", "side")]),
    "legacy": (8, [
        ("prologue", "main"), ("conv_fwd0", "main"), ("conv_fwd1", "main"), ("conv_fwd2", "main"), ("conv_fwd3", "main"),
        ("dense_fwd0", "main"), ("head", "main"), ("dense_dx0", "main"), ("wgrad_dense0", "main"),
        ("wgrad_conv3", "side"), ("dgrad_conv3", "main"), ("wgrad_conv2", "side"), ("dgrad_conv2", "main"),
        ("wgrad_conv1", "side"), ("dgrad_conv1", "main"), ("wgrad_conv0", "side"), ("reduce_b0", "side")]),
    "bn_odd": (8, [
        ("prologue", "main"), ("conv_fwd0", "main"), ("bn_stats_c0", "main"), ("bn_apply_fwd_c0", "main"),
        ("conv_fwd1", "main"), ("bn_stats_c1", "main"), ("bn_apply_fwd_c1", "main"), ("act_fwd_c1", "main"),
        ("dense_fwd0", "main"), ("dense_epi0", "main"), ("bn_stats_d0", "main"), ("bn_apply_fwd_d0", "main"),
        ("act_fwd_d0", "main"), ("dense_fwd1", "main"), ("head", "main"), ("dense_bwd1", "main"),
        ("act_bwd_d0", "main"), ("bn_bwd_reduce_d0", "main"), ("bn_bwd_apply_d0", "main"), ("dense_bwd0", "main"),
        ("act_bwd_c1", "main"), ("bn_bwd_reduce_c1", "main"), ("bn_bwd_apply_c1", "main"),
        ("wgrad_dgrad_conv1", "main"), ("bn_bwd_reduce_c0", "main"), ("bn_bwd_apply_c0", "main"),
        ("wgrad_conv0", "side"), ("reduce_b0", "side")]),
    "act": (8, [
        ("prologue", "main"), ("conv_fwd0", "main"), ("act_fwd_c0", "main"), ("conv_fwd1", "main"),
        ("act_fwd_c1", "main"), ("dense_fwd0", "main"), ("dense_epi0", "main"), ("act_fwd_d0", "main"),
        ("dense_fwd1", "main"), ("head", "main"), ("dense_bwd1", "main"), ("act_bwd_d0", "main"),
        ("dense_bwd0", "main"), ("act_bwd_c1", "main"), ("wgrad_dgrad_conv1", "main"), ("act_bwd_c0", "main"),
        ("wgrad_conv0", "side"), ("reduce_b0", "side")]),
    "reg_clip": (8, [
        ("conv_stack_fwd", "main"), ("dense_fwd0", "main"), ("head", "main"), ("dense_bwd0", "main"),
        ("wgrad_dgrad_conv1", "main"), ("wgrad_conv0", "side"), ("reduce_b0", "side"), ("weight_reg", "main"),
        ("grad_sqnorm", "main")]),
}

# launch name prefix -> the roles its Launch.args holds (longest prefix first)
ROLES = [
    ("wgrad_dgrad_conv", {"ca", "ntc", "wa", "cfg"}),
    ("conv_stack_fwd", {"stack"}),
    ("grad_sqnorm", {"clip"}),
    ("weight_reg", {"reg"}),
    ("wgrad_dense", {"wa", "cfg"}),
    ("wgrad_conv", {"wa", "cfg"}),
    ("dgrad_conv", {"ca"}),
    ("dense_bwd", {"wa", "cfg", "da"}),
    ("dense_fwd", {"da"}),
    ("dense_epi", {"epi"}),
    ("dense_dx", {"da"}),
    ("conv_fwd", {"ca"}),
    ("act_fwd_", {"act"}),
    ("act_bwd_", {"act"}),
    ("prologue", {"pro"}),
    ("reduce_b", set()),
    ("head", {"head"}),
    ("bn_", {"bn"}),
]
STRUCTS = {"ca": "ConvMMArgs", "wa": "WgradArgs", "da": "DenseFwdArgs", "epi": "DenseEpiArgs", "pro": "PrologueArgs",
           "stack": "ConvStackArgs", "head": "HeadArgs", "bn": "BnArgs", "act": "ActArgs", "reg": "RegArgs",
           "clip": "ClipArgs"}


def _dump_models():
    spec = importlib.util.spec_from_file_location(
        "plan_dump", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "plan_dump.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.models()


def _model(kind):
    if kind in ("bn_odd", "act", "reg_clip"):
        return _dump_models()[kind][0]()
    if kind == "rpv":
        return zoo.rpv_cnn((64, 64, 3), conv_sizes=[16, 32, 64], fc_sizes=[128], dropout=0.2, optimizer="Adam",
                           lr=1e-3, device="cuda")
    if kind == "mnist":
        return zoo.mnist_cnn(32, 64, 128, dropout=0.3, optimizer="Adam", lr=1e-3, input_shape=(28, 28, 1),
                             device="cuda")
    return zoo.rpv_legacy_cnn((64, 64, 3), optimizer="Adam", lr=1e-3, device="cuda")


@pytest.mark.parametrize("kind", sorted(SEQUENCES))
def test_default_train_program(kind, monkeypatch):
    monkeypatch.delenv("INTML_TUNE", raising=False)
    bs, want = SEQUENCES[kind]
    plan = _model(kind)._executor._plan_for(bs, "train")
    assert [(it.name, it.tag) for it in plan.launches] == want
    for it in plan.launches:
        assert type(it) is Launch and callable(it.fn)
        roles = next(r for prefix, r in ROLES if it.name.startswith(prefix))
        assert set(it.args) == roles, (it.name, sorted(it.args))
        for role, v in it.args.items():
            if role in STRUCTS:
                assert type(v).__name__ == STRUCTS[role], (it.name, role, type(v).__name__)
        if "cfg" in it.args:
            cfg = it.args["cfg"]
            assert len(cfg) == 3 and cfg[2] >= 1, (it.name, cfg)       # (tile, tile, splits)
        if "ntc" in it.args:
            assert it.args["ntc"] >= 1

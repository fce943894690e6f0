"""The optimizer-kind table: the Python copy (optim/optimizers.py KINDS) against every optimizer
class and against the table the extension exports from csrc/kernels/common.h, and the host
launchers' refusals of a kind their kernel has no instance of (argument errors thrown before
anything is launched)."""
import pytest

from cori_intml_examples_amd import optim
from cori_intml_examples_amd.optim import optimizers as O


def test_kind_table_agrees_with_optimizer_classes():
    from cori_intml_examples_amd.models.executor_hip import OPT_KIND, STANDALONE_KINDS
    from cori_intml_examples_amd.parallel.dist import RCCL_ONLY_KINDS
    opts = [cls() for cls in O._BY_NAME.values()] + [optim.SGD(momentum=0.9), optim.Adam(amsgrad=True)]
    for o in opts:
        assert o.kind in O.KINDS, o.kind
        assert o.n_slots >= O.KINDS[o.kind][1], (o.kind, o.n_slots)
    assert {o.kind for o in opts} == set(O.KINDS)                   # no row without a class
    ams = optim.Adam(amsgrad=True)
    assert (ams.kind, ams.n_slots, O.KINDS["amsgrad"][1]) == ("amsgrad", 3, 3)
    assert sorted(v[0] for v in O.KINDS.values()) == list(range(len(O.KINDS)))   # ids: 0 .. n-1, distinct
    assert OPT_KIND == {k: v[0] for k, v in O.KINDS.items()}
    no_rt = {k for k, v in O.KINDS.items() if not v[2]}
    assert STANDALONE_KINDS == RCCL_ONLY_KINDS == no_rt == {"adagrad", "adamax", "amsgrad"}


def test_kernel_args_filled_from_one_place():
    """fill_kernel_args writes the fields a struct has, with the defaults of an optimizer
    that lacks the attribute."""
    import types
    a = types.SimpleNamespace(kind=-1, beta1=0, beta2=0, eps=0, rho=0, momentum=0, nesterov=-1)
    O.fill_kernel_args(optim.SGD(momentum=0.5, nesterov=True), a)
    assert vars(a) == dict(kind=0, beta1=0.9, beta2=0.999, eps=1e-7, rho=0.95, momentum=0.5, nesterov=1)
    sb = types.SimpleNamespace(opt_kind=-1, beta1=0, beta2=0, decay=-1, schedule_decay=0)
    O.fill_kernel_args(optim.Nadam(beta_1=0.8, schedule_decay=0.01), sb, "opt_kind")
    assert vars(sb) == dict(opt_kind=4, beta1=0.8, beta2=0.999, decay=0.0, schedule_decay=0.01)
    O.fill_kernel_args(optim.Adam(decay=0.25, amsgrad=True), sb, "opt_kind")
    assert (sb.opt_kind, sb.decay, sb.schedule_decay) == (7, 0.25, 0.004)


@pytest.mark.gpu
def test_extension_table_and_refusals():
    import torch
    from cori_intml_examples_amd.ops.hip import kernels
    from test_comm import _fake_xgmi
    K = kernels()
    assert dict(K.OPT_KINDS) == O.KINDS
    ids = O.KIND_IDS
    buf = torch.zeros(64, device="cuda")          # real addresses; no launch ever reads them
    ptr = buf.data_ptr()

    def args(kind):
        a = K.OptimArgs()
        a.p = a.g = a.st = ptr
        a.n, a.kind, a.grad_only = 64, kind, 0
        return a

    tab = K.RedTable()
    tab.add(4096, 256, 2, 16, 0, 256, 2, 1, 1, 16, 16, 16, -1)     # RED_FLATW float4, elements [0, 256)
    assert tab.nblocks > 0
    # a kind outside the table: every instance's dispatcher refuses it
    with pytest.raises(ValueError, match="optim: no kernel instance for optimizer kind 99"):
        K.optim(args(99), K.PackTable(), 0)
    with pytest.raises(ValueError, match="reduce_optim: no kernel instance for optimizer kind 99"):
        K.reduce_optim(0, tab, args(99), 0)
    # the run-time-switch kernels are five-way: an updating xGMI table, the dense wgrad's fused update
    x, _, _ = _fake_xgmi(rank=0, size=2, chunk=1024)
    with pytest.raises(ValueError, match="no kernel instance for optimizer kind %d" % ids["adagrad"]):
        K.reduce_optim(0, tab, args(ids["adagrad"]), 0, x.push_args(0, mode=2, nblk=tab.nblocks))
    w = K.WgradArgs()
    w.Cs_in, w.Cs_dy, w.px_per_split, w.P, w.NT, w.KH, w.KW = 32, 16, 32, 32, 1, 1, 1
    w.opt, w.opt_w = args(ids["adagrad"]), 0
    with pytest.raises(ValueError, match="dense_wgrad: no fused update for optimizer kind %d" % ids["adagrad"]):
        K.dense_wgrad(w, 2, 1, 1, 0)
    # AMSGrad's instances touch three state buffers unconditionally
    a = args(ids["amsgrad"])
    a.s0 = a.s1 = ptr
    with pytest.raises(ValueError, match="optimizer kind %d: missing state buffer" % ids["amsgrad"]):
        K.optim(a, K.PackTable(), 0)
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0          # nothing ran

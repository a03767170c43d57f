"""The training-mode executor of one BATS cell operation (training.CELL_OPS, training.cell_op_train) on a machine without
a GPU: the switch, the decline rules — each falls through to ``_CellOp._forward`` without a native call or a counter
moving — and the argument checks of the new hipops wrappers, which raise before anything touches a device."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import bnn_amd as bnn
from bnn_amd import fastpath, hipops, models, native, training
from bnn_amd.native import NativeError
from bnn_amd.ops import AdvancedInputBinarizer, BasicInputBinarizer, BasicScaleBinarizer, XNORWeightBinarizer
from tests.golden.cellops_cases import CELL_CASES


def binarise(m, pre=BasicInputBinarizer, post=bnn.Identity):
    cfg = bnn.BConfig(activation_pre_process=pre, activation_post_process=post, weight_pre_process=XNORWeightBinarizer)
    return bnn.prepare_binary_model(m, cfg)


def build(case, **recipe):
    m = binarise(case.build(models), **recipe)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict({k: torch.from_numpy(v) for k, v in case.state(shapes).items()})
    return m.train()


@pytest.fixture
def cell_ops_on(monkeypatch):
    monkeypatch.setattr(training, "CELL_OPS", True)


def untouched(m, x):
    """``m(x)`` is ``m._forward(x)`` on a module with the same state, no native call was made and no counter moved."""
    import copy
    twin = copy.deepcopy(m)
    launches, stats = native.launch_count(), fastpath.stats()
    y = m(x)
    assert native.launch_count() == launches and fastpath.stats() == stats
    assert torch.equal(y, twin._forward(x))
    return y


def test_the_switch_follows_the_environment_and_is_off_without_it():
    assert training.CELL_OPS is (os.environ.get("BNN_AMD_TRAIN_CELL_OPS", "0") == "1")
    assert "cell_op_train" in fastpath.stats()


@pytest.mark.parametrize("case", CELL_CASES, ids=[c.name for c in CELL_CASES])
def test_a_cpu_module_in_training_mode_runs_its_own_forward(cell_ops_on, case):
    m = build(case)
    x = torch.from_numpy(case.input()).requires_grad_()
    y = untouched(m, x)
    y.sum().backward()
    assert x.grad is not None and m.op[1].weight.grad is not None
    assert training.cell_op_train(m, x) is None


def test_each_decline_rule_falls_through(cell_ops_on):
    case = CELL_CASES[0]
    x = torch.from_numpy(case.input())
    # eval mode (no fused inference executor on a CPU tensor either)
    m = build(case).eval()
    untouched(m, x)
    assert training.cell_op_train(m, x) is None
    # a hook on the operation, on a sub-module, on a hook module of the convolution
    for pick in (lambda m: m, lambda m: m.op[0], lambda m: m.op[1], lambda m: m.op[2],
                 lambda m: m.op[1].activation_pre_process, lambda m: m.op[1].weight_pre_process):
        m = build(case)
        seen = []
        pick(m).register_forward_hook(lambda mod, i, o: seen.append(1))
        untouched(m, x)
        assert seen and training.cell_op_train(m, x) is None
    m = build(case)
    m.op[1].register_full_backward_hook(lambda mod, gi, go: None)
    assert training.cell_op_train(m, x) is None
    # a bias
    m = build(case)
    m.op[1].bias = nn.Parameter(torch.zeros(case.C_out))
    untouched(m, x)
    assert training.cell_op_train(m, x) is None
    # BasicScaleBinarizer behind the convolution; AdvancedInputBinarizer in front of it (another backward)
    for recipe in (dict(post=BasicScaleBinarizer), dict(pre=AdvancedInputBinarizer)):
        m = build(case, **recipe)
        untouched(m, x)
        assert training.cell_op_train(m, x) is None
    # BatchNorm without running statistics, a BatchNorm subclass, padding as a string, autograd off, the master switch
    m = build(case)
    m.op[0] = nn.BatchNorm2d(case.C_in, track_running_stats=False)
    assert training.cell_op_train(m, x) is None
    m = build(case)
    m.op[0] = nn.SyncBatchNorm(case.C_in)
    assert training.cell_op_train(m, x) is None
    m = build(case)
    with torch.no_grad():
        untouched(m, x)
        assert training.cell_op_train(m, x) is None
    with torch.autocast("cpu", dtype=torch.bfloat16):
        assert training.cell_op_train(m, x) is None
    assert training.cell_op_train(nn.Sequential(m), x) is None                 # not a cell operation


def _binary(m, **recipe):
    return binarise(m, **recipe).train()


def _conv(k=3, bias=False, **recipe):
    return _binary(nn.Conv2d(8, 8, k, padding=k // 2, bias=bias), **recipe)


def _with(m, change):
    """``m`` after ``change(m)`` (a hook registered, an attribute replaced)."""
    change(m)
    return m


def _hook(kind, pick=lambda m: m):
    register = {"forward": lambda m: m.register_forward_hook(lambda mod, i, o: None),
                "forward_pre": lambda m: m.register_forward_pre_hook(lambda mod, i: None),
                "backward": lambda m: m.register_full_backward_hook(lambda mod, gi, go: None),
                "backward_pre": lambda m: m.register_full_backward_pre_hook(lambda mod, go: None)}[kind]
    return lambda m: register(pick(m))


def _transposed_weight(m):
    m.weight = nn.Parameter(m.weight.detach().transpose(-1, -2))        # same shape (square), other strides


def _padding_same(m):
    m.padding = "same"


def _no_running_var(m):
    m.running_var = None


def _wpre(m):
    return m.weight_pre_process


def _fusable(conv):
    return training._fusable_binary_conv(conv, fastpath._recognise(conv, conv.out_channels))


# (rule, what it is asked, its answer): one row per reason to decline, and the plain module each was derived from
ADMISSION = [
    ("bn: plain", lambda: training._batch_stat_bn(nn.BatchNorm2d(8)), True),
    ("bn: not affine", lambda: training._batch_stat_bn(nn.BatchNorm2d(8, affine=False)), True),
    ("bn: a subclass", lambda: training._batch_stat_bn(nn.SyncBatchNorm(8)), False),
    ("bn: no running statistics", lambda: training._batch_stat_bn(nn.BatchNorm2d(8, track_running_stats=False)), False),
    ("bn: one running statistic", lambda: training._batch_stat_bn(_with(nn.BatchNorm2d(8), _no_running_var)), False),
    ("bn: eval mode", lambda: training._batch_stat_bn(nn.BatchNorm2d(8).eval()), False),
    ("bn: not a BatchNorm", lambda: training._batch_stat_bn(None), False),
    ("conv: plain", lambda: _fusable(_conv()), True),
    ("conv: bias", lambda: _fusable(_conv(bias=True)), False),
    ("conv: post scale", lambda: _fusable(_conv(post=BasicScaleBinarizer)), False),
    ("conv: AdvancedInputBinarizer", lambda: _fusable(_conv(pre=AdvancedInputBinarizer)), False),
    ("conv: string padding", lambda: _fusable(_with(_conv(), _padding_same)), False),
    ("conv: not recognised", lambda: training._fusable_binary_conv(_conv(), None), False),
    ("hook: plain conv", lambda: training._fused_weight_hook(_conv(), 4, backward_hooks=True), True),
    ("hook: 32 x 32 taps", lambda: training._fused_weight_hook(_conv(k=32), 4, backward_hooks=True), True),
    ("hook: non-contiguous weight", lambda: training._fused_weight_hook(_with(_conv(), _transposed_weight), 4, True), False),
    ("hook: kh * kw > 1024", lambda: training._fused_weight_hook(_conv(k=33), 4, backward_hooks=True), False),
    ("hook: a Linear asked as a Conv2d", lambda: training._fused_weight_hook(_binary(nn.Linear(8, 8)), 4, True), False),
    ("hook: plain Linear", lambda: training._fused_weight_hook(_binary(nn.Linear(8, 8)), 2, backward_hooks=False), True),
    ("hook: non-contiguous Linear weight",
     lambda: training._fused_weight_hook(_with(_binary(nn.Linear(8, 8)), _transposed_weight), 2, False), False),
    ("hook: forward hook on the binarizer, per-layer site",
     lambda: training._fused_weight_hook(_with(_conv(), _hook("forward", _wpre)), 4, backward_hooks=False), False),
    ("hook: forward-pre hook on the binarizer, fused-op site",
     lambda: training._fused_weight_hook(_with(_conv(), _hook("forward_pre", _wpre)), 4, backward_hooks=True), False),
    ("hook: backward hook on the binarizer, fused-op site",
     lambda: training._fused_weight_hook(_with(_conv(), _hook("backward", _wpre)), 4, backward_hooks=True), False),
    ("hook: backward hook on the binarizer, per-layer site (never asked there)",
     lambda: training._fused_weight_hook(_with(_conv(), _hook("backward", _wpre)), 4, backward_hooks=False), True),
    ("no_hooks: plain, and None skipped", lambda: training._no_hooks(nn.ReLU(), None, nn.BatchNorm2d(8)), True),
    ("no_hooks: forward", lambda: training._no_hooks(nn.ReLU(), _with(nn.ReLU(), _hook("forward"))), False),
    ("no_hooks: forward, forward-only site",
     lambda: training._no_hooks(_with(nn.ReLU(), _hook("forward")), backward=False), False),
    ("no_hooks: forward-pre", lambda: training._no_hooks(_with(nn.ReLU(), _hook("forward_pre")), backward=False), False),
    ("no_hooks: backward", lambda: training._no_hooks(_with(nn.ReLU(), _hook("backward"))), False),
    ("no_hooks: backward-pre", lambda: training._no_hooks(_with(nn.ReLU(), _hook("backward_pre"))), False),
    ("no_hooks: backward, forward-only site",
     lambda: training._no_hooks(_with(nn.ReLU(), _hook("backward")), backward=False), True),
    ("device: a CPU tensor", lambda: training._f32_on_one_device(torch.zeros(2)), False),
    ("device: a CPU tensor among the others",
     lambda: training._f32_on_one_device(torch.zeros(2, device="meta"), torch.zeros(2)), False),
]


@pytest.mark.parametrize("name,ask,answer", ADMISSION, ids=[r[0] for r in ADMISSION])
def test_each_admission_rule_answers_on_its_own(name, ask, answer):
    """Through ``cell_op_train`` / ``reduce_train`` every decline on a CPU module ends in the same None (the device rule
    declines last); asked directly, each rule shows its own answer.  No native call is made."""
    launches = native.launch_count()
    assert ask() is answer
    assert native.launch_count() == launches


def test_the_fused_weight_hook_rule_follows_its_switch(monkeypatch):
    conv = _conv()
    assert training._fused_weight_hook(conv, 4, backward_hooks=True)
    monkeypatch.setattr(training, "FUSED_WEIGHT_HOOK", False)
    assert not training._fused_weight_hook(conv, 4, backward_hooks=True)
    assert training._binary_conv_plan(conv) is None


def test_the_plan_of_a_fusable_convolution():
    plan = training._binary_conv_plan(_conv())
    assert plan is not None and plan.ste and plan.scale is None
    assert training._binary_conv_plan(nn.Conv2d(8, 8, 3)) is None                       # not a binary layer
    assert training._binary_conv_plan(_conv(bias=True)) is None
    assert training._binary_conv_plan(_with(_conv(), _hook("backward", _wpre))) is None


def test_master_switches_turn_the_path_off(monkeypatch):
    case = CELL_CASES[0]
    m, x = build(case), torch.from_numpy(case.input())
    monkeypatch.setattr(training, "CELL_OPS", False)
    called = []
    monkeypatch.setattr(training, "cell_op_train", lambda op, x: called.append(1))
    m(x)
    assert not called                           # switch off: the module is not even offered
    monkeypatch.setattr(training, "CELL_OPS", True)
    m(x)
    assert called == [1]                        # on: offered (and, the stand-in returning None, its own forward ran)
    with torch.no_grad():
        m(x)
    m.eval()
    m(x)
    assert called == [1]


def test_the_new_wrappers_reject_wrong_ranks_and_dtypes_before_touching_the_gpu():
    launches = native.launch_count()
    x4, x3 = torch.zeros(2, 8, 3, 3), torch.zeros(2, 8, 9)
    c = torch.ones(8)
    for bad in (x3, x4.double(), x4.half(), x4.int()):
        with pytest.raises(NativeError):
            hipops.bn_act_pack_ste(bad, c, c)
        with pytest.raises(NativeError):
            hipops.bn_train_pack_ste(bad, c, c, c.clone(), c.clone(), 0.1, 1e-5)
        with pytest.raises(NativeError):
            hipops.prelu_shuffle_backward(bad, bad, c, 4)
        with pytest.raises(NativeError):
            hipops.bn_train_backward_add(bad, bad, c, c, c, bad)
    with pytest.raises(NativeError):
        hipops.bn_act_pack_ste(x4, c, None)                      # scale and shift come together
    with pytest.raises(NativeError):
        hipops.bn_act_pack_ste(x4)                               # a CPU tensor
    assert native.launch_count() == launches


def test_the_library_validates_the_new_entry_points_without_a_gpu():
    """Null pointers, sizes and the shuffle / slope rules are refused by the C side before any launch."""
    lib = native.require()
    launches = native.launch_count()
    p = 0x10000
    INV = native.ERR_INVALID_ARG
    assert lib.bnn_hip_bn_act_pack_ste_f32(None, 1, 8, 3, 3, None, None, p, p, p, None) == INV
    assert lib.bnn_hip_bn_act_pack_ste_f32(p, 1, 8, 3, 3, p, None, p, p, p, None) == INV        # scale without shift
    assert lib.bnn_hip_bn_act_pack_ste_f32(p, 1, 8, 3, 3, None, None, p, p, None, None) == INV  # no T plane
    assert lib.bnn_hip_bn_act_pack_ste_f32(p, 0, 8, 3, 3, None, None, p, p, p, None) == INV
    assert lib.bnn_hip_bn_train_pack_ste_f32(p, 1, 8, 3, 3, None, None, 1e-5, 0.1, None, None, p, p, p, p, p, p, p, None,
                                             None) == INV                                             # no workspace
    assert lib.bnn_hip_bn_train_pack_ste_f32(p, 1, 8, 3, 3, None, None, 1e-5, 0.1, p, None, p, p, p, p, p, p, p, p,
                                             None) == INV                                             # one running buffer
    assert lib.bnn_hip_bn_train_pack_ste_f32(p, 1, 8, 3, 3, None, None, -1.0, 0.1, None, None, p, p, p, p, p, p, p, p,
                                             None) == INV                                             # eps < 0
    assert lib.bnn_hip_bn_train_backward_add_f32(None, None, p, p, p, None, p, 1, 8, 9, p, p, p, p, None) == INV
    assert lib.bnn_hip_bn_train_backward_add_f32(p, None, p, p, p, None, p + 2, 1, 8, 9, p, p, p, p, None) == INV
    need = lib.bnn_hip_prelu_shuffle_backward_workspace_bytes(2, 48, 100)
    assert need == 48 * 2 * 8 and lib.bnn_hip_prelu_shuffle_backward_workspace_bytes(0, 48, 100) == 0
    q = 0x20000
    args = dict(gy=p, z=q, slope=p, count=48, N=2, O=48, HW=100, sg=4, gz=q, ds=p, ws=p, nbytes=need)

    def call(**kw):
        a = dict(args, **kw)
        return lib.bnn_hip_prelu_shuffle_backward_f32(a["gy"], a["z"], a["slope"], a["count"], a["N"], a["O"], a["HW"],
                                                      a["sg"], a["gz"], a["ds"], a["ws"], a["nbytes"], None)
    assert call(sg=5) == INV and call(sg=0) == INV              # shuffle groups must divide O
    assert call(count=2) == INV                                  # 1 or O slopes
    assert call(gz=p) == INV                                     # gz must not be gy (gz == z is the in-place form)
    assert call(nbytes=need - 1) == INV and call(ws=None) == INV
    assert call(z=None) == INV and call(N=0) == INV
    assert native.launch_count() == launches


def test_counter_and_saved_bytes_exist():
    assert fastpath.stats()["cell_op_train"] >= 0
    assert isinstance(training.saved_input_bytes(), int)
    assert set(training.CELL_OP_SHUFFLE) == {"SepConv", "DilConv", "ReLUConvBN"}
    assert np.all([v in (1, 4) for v in training.CELL_OP_SHUFFLE.values()])

"""The training-mode executor of ``FactorizedReduce`` (training.CELL_OPS, training.reduce_train) on a machine without a
GPU: the switch, the decline rules — each falls through to the module's own forward without a native call or a counter
moving — and the argument checks of the new entry points, which refuse before anything touches a device."""
import copy
import os

import pytest
import torch
import torch.nn as nn

import bnn_amd as bnn
from bnn_amd import fastpath, hipops, models, native, training
from bnn_amd.ops import AdvancedInputBinarizer, BasicInputBinarizer, BasicScaleBinarizer, XNORWeightBinarizer
from tests.golden import gen

C_IN, C_OUT, SHAPE = 24, 16, (2, 24, 6, 4)


def binarise(m, pre=BasicInputBinarizer, post=bnn.Identity):
    cfg = bnn.BConfig(activation_pre_process=pre, activation_post_process=post, weight_pre_process=XNORWeightBinarizer)
    return bnn.prepare_binary_model(m, cfg)


def build(float_module=None, **recipe):
    m = binarise(float_module if float_module is not None else models.FactorizedReduce(C_IN, C_OUT), **recipe)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict({k: torch.from_numpy(v) for k, v in gen.model_state(shapes, gen.seed_of("reduce-train-cpu")).items()})
    return m.train()


def the_input(shape=SHAPE):
    return torch.from_numpy(gen.activation("normal", gen.seed_of("reduce-train-cpu", "x"), shape))


@pytest.fixture
def cell_ops_on(monkeypatch):
    monkeypatch.setattr(training, "CELL_OPS", True)


def untouched(m, x):
    """``m(x)`` with the switch on is the tensor ``m(x)`` gives with the switch off on a module of the same state; no
    native call was made and no counter moved."""
    twin = copy.deepcopy(m)
    launches, stats = native.launch_count(), fastpath.stats()
    y = m(x)
    assert native.launch_count() == launches and fastpath.stats() == stats
    on, training.CELL_OPS = training.CELL_OPS, False
    try:
        want = twin(x)
    finally:
        training.CELL_OPS = on
    assert torch.equal(y, want)
    assert training.reduce_train(m, x) is None
    return y


def test_the_switch_is_off_by_default_and_read_per_call(monkeypatch):
    assert training.CELL_OPS is (os.environ.get("BNN_AMD_TRAIN_CELL_OPS", "0") == "1")
    assert fastpath.stats()["reduce_train"] >= 0
    m, x = build(), the_input()
    called = []
    monkeypatch.setattr(training, "reduce_train", lambda mod, x: called.append(1))
    monkeypatch.setattr(training, "CELL_OPS", False)
    m(x)
    assert not called                           # off: the module is not even offered
    monkeypatch.setattr(training, "CELL_OPS", True)
    m(x)
    assert called == [1]                        # on: offered (the stand-in returns None: the module's own forward ran)
    with torch.no_grad():
        m(x)
    m.eval()
    m(x)
    assert called == [1]                        # not without autograd, not in eval mode


def test_a_cpu_module_in_training_mode_runs_its_own_forward(cell_ops_on):
    m = build()
    x = the_input().requires_grad_()
    y = untouched(m, x)
    assert y.shape == (SHAPE[0], C_OUT, SHAPE[2] // 2, SHAPE[3] // 2)
    y.sum().backward()
    assert x.grad is not None and m.conv_1[0].weight.grad is not None and m.conv_2[0].weight.grad is not None


def with_convs(**kw):
    """A module of FactorizedReduce's structure whose convolutions are built with ``kw`` instead of 1x1 / stride 2."""
    f = models.FactorizedReduce(C_IN, C_OUT)
    conf = dict(kernel_size=1, stride=2, padding=0, bias=False)
    conf.update(kw)
    f.conv_1 = nn.Sequential(nn.Conv2d(C_IN, C_OUT // 2, **conf))
    f.conv_2 = nn.Sequential(nn.Conv2d(C_IN, C_OUT // 2, **conf))
    return f


def test_each_decline_rule_falls_through(cell_ops_on):
    x = the_input()
    # a hook: on the module, its BatchNorm, a convolution, the PReLU, a hook module of a convolution
    for pick in (lambda m: m, lambda m: m.bn, lambda m: m.conv_1[0], lambda m: m.conv_2, lambda m: m.activation,
                 lambda m: m.conv_2[0].activation_pre_process, lambda m: m.conv_1[0].weight_pre_process):
        m = build()
        seen = []
        pick(m).register_forward_hook(lambda mod, i, o: seen.append(1))
        untouched(m, x)
        assert seen
    m = build()
    m.conv_2[0].register_full_backward_hook(lambda mod, gi, go: None)
    assert training.reduce_train(m, x) is None
    # a bias
    m = build()
    m.conv_1[0].bias = nn.Parameter(0.1 * torch.ones(C_OUT // 2))
    untouched(m, x)
    # BasicScaleBinarizer behind the convolutions; AdvancedInputBinarizer in front of them (another backward)
    for recipe in (dict(post=BasicScaleBinarizer), dict(pre=AdvancedInputBinarizer)):
        untouched(build(**recipe), x)
    # 3x3 convolutions, stride 1, groups = 2 (the module's own forward takes any of them)
    untouched(build(with_convs(kernel_size=3, padding=1)), x)
    f = with_convs()                            # (stride 1 in the second branch: on 2x2 images both halves are 1x1)
    f.conv_2 = nn.Sequential(nn.Conv2d(C_IN, C_OUT // 2, 1, stride=1, padding=0, bias=False))
    untouched(build(f), the_input((3, C_IN, 2, 2)))
    m = build(with_convs(stride=1))             # (in both: the halves never have one shape, torch.cat refuses as before)
    with pytest.raises(RuntimeError):
        m(x)
    assert training.reduce_train(m, x) is None
    untouched(build(with_convs(groups=2)), x)
    # eval-mode BatchNorm inside a training module; BatchNorm without running statistics; a BatchNorm subclass
    m = build()
    m.bn.eval()
    untouched(m, x)
    m = build()
    m.bn = nn.BatchNorm2d(C_IN, track_running_stats=False)
    untouched(m, x)
    m = build()
    m.bn = nn.SyncBatchNorm(C_IN)
    assert training.reduce_train(m, x) is None
    # autocast, autograd off, eval mode, another class of the same structure
    m = build()
    with torch.autocast("cpu", dtype=torch.bfloat16):
        untouched(m, x)
    with torch.no_grad():
        untouched(m, x)
    untouched(build().eval(), x)
    assert training.reduce_train(nn.Sequential(build()), x) is None


def test_master_switches(monkeypatch, cell_ops_on):
    m, x = build(), the_input()
    for name in ("ENABLED", "BINARY_GRADS", "FUSED_WEIGHT_HOOK"):
        monkeypatch.setattr(training, name, False)
        untouched(m, x)
        monkeypatch.setattr(training, name, True)


def test_the_new_wrappers_reject_wrong_inputs_before_touching_the_gpu():
    # (native.NativeError looked up at the call: tests/test_native_cpu.py reloads that module, which makes a new class)
    launches = native.launch_count()
    x4, x3 = torch.zeros(2, 8, 4, 4), torch.zeros(2, 8, 16)
    c = torch.ones(8)
    for bad in (x3, x4.double(), x4.half(), x4.int(), x4):          # (x4 itself: a CPU tensor)
        with pytest.raises(native.NativeError):
            hipops.bn_act_pack_ste_s2(bad, c, c)
        with pytest.raises(native.NativeError):
            hipops.bn_train_pack_ste_s2(bad, c, c, c.clone(), c.clone(), 0.1, 1e-5)
        with pytest.raises(native.NativeError):
            hipops.bn_train_backward_s2(bad, bad, bad, c, c, c)
    with pytest.raises(native.NativeError):
        hipops.bn_act_pack_ste_s2(x4, c, None)                       # scale and shift come together
    assert native.launch_count() == launches


def test_the_library_validates_the_new_entry_points_without_a_gpu():
    """Odd H or W, null or misaligned pointers, a missing workspace and sizes past the 32-bit limits are refused by the C
    side, with the documented status, before any launch."""
    lib = native.require()
    launches = native.launch_count()
    p = 0x10000
    INV, BIG = native.ERR_INVALID_ARG, native.ERR_TOO_LARGE

    def pack(x=p, N=1, C=8, H=4, W=4, a=None, b=None, P=p, M=p, T=p):
        return lib.bnn_hip_bn_act_pack_ste_s2_f32(x, N, C, H, W, a, b, P, M, T, None)
    assert pack(H=3) == INV and pack(W=5) == INV                                  # the lattices need even H and W
    assert pack(x=None) == INV and pack(P=None) == INV and pack(M=None) == INV and pack(T=None) == INV
    assert pack(a=p) == INV                                                       # scale without shift
    assert pack(T=p + 4) == INV and pack(P=p + 4) == INV and pack(x=p + 2) == INV and pack(a=p + 2, b=p) == INV
    assert pack(N=0) == INV and pack(C=0) == INV and pack(H=0) == INV
    assert pack(N=1 << 20, H=1 << 6, W=1 << 6) == BIG                             # N * H * W past 2^31 - 1

    def fwd(x=p, N=1, C=8, H=4, W=4, eps=1e-5, rm=None, rv=None, T=p, mean=p, ws=p):
        return lib.bnn_hip_bn_train_pack_ste_s2_f32(x, N, C, H, W, None, None, eps, 0.1, rm, rv, p, p, T, mean, p, p, p, ws,
                                                    None)
    assert fwd(H=6, W=3) == INV and fwd(H=1) == INV
    assert fwd(ws=None) == INV and fwd(ws=p + 4) == INV                           # no workspace / not 8-byte aligned
    assert fwd(rm=p) == INV and fwd(eps=-1.0) == INV and fwd(mean=None) == INV and fwd(T=None) == INV and fwd(x=None) == INV
    assert fwd(N=1 << 20, H=1 << 6, W=1 << 6) == BIG

    def bwd(g0=p, g1=p, x=p, N=1, C=8, H=4, W=4, dx=p, ws=p):
        return lib.bnn_hip_bn_train_backward_s2_f32(g0, g1, x, p, p, None, N, C, H, W, dx, p, p, ws, None)
    assert bwd(H=5) == INV and bwd(W=7) == INV and bwd(H=0) == INV
    assert bwd(g0=None) == INV and bwd(g1=None) == INV and bwd(x=None) == INV and bwd(dx=None) == INV
    assert bwd(ws=None) == INV and bwd(ws=p + 4) == INV
    assert bwd(x=p + 4) == INV and bwd(dx=p + 4) == INV and bwd(g1=p + 2) == INV  # rows of x / dx move as float2
    assert bwd(N=1 << 12, C=1 << 12, H=1 << 6, W=1 << 6) == BIG                   # N * C * H * W past 4 (2^31 - 1)
    # the workspace is that of the other training BatchNorm entry points, sized by the FULL pixel count; a size the
    # validators refuse has none
    assert lib.bnn_hip_bn_train_workspace_bytes(2, 48, 8 * 8) >= 48 * 2 * 2 * 8 + 3 * 48 * 4
    assert lib.bnn_hip_bn_train_workspace_bytes(0, 48, 64) == 0
    assert native.launch_count() == launches


def test_counter_and_symbols_exist():
    assert "reduce_train" in fastpath.stats()
    for sym in ("bnn_hip_bn_act_pack_ste_s2_f32", "bnn_hip_bn_train_pack_ste_s2_f32", "bnn_hip_bn_train_backward_s2_f32"):
        assert sym in native.EXPORTED_SYMBOLS
    assert callable(training.reduce_train) and callable(training.ReduceTrainFn.apply)

"""Grouped and depthwise binary convolutions on the HIP path (csrc/bconv_grouped.hip, bnn_hip_bconv2d_grouped): packing,
the integer dot against the CPU oracle applied group by group, the float output bit for bit against the oracle's epilogue
and within 1e-3 of the reference (tests/golden/grouped.npz), and the drop-in layers — Conv2d / Conv1d with groups > 1 —
taking that path under inference while training and the fused executors keep the composition."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import bnn_amd as bnn
import oracle
from bnn_amd import fastpath, hipops
from bnn_amd.inference import FusedResNet, FusionError, per_layer_forward
from bnn_amd.models import resnet18
from bnn_amd.native import NativeError
from bnn_amd.ops import BasicInputBinarizer, BasicScaleBinarizer, XNORWeightBinarizer
from tests.golden import gen
from tests.golden.grouped_cases import GROUPED_CASES, OP_C, OP_CASES, op_input
from tests.grouped_util import as_2d, oracle_dot, window_pack

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IDS = [c.name for c in GROUPED_CASES]


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def close(a, ref):
    return np.allclose(a, ref, rtol=1e-3, atol=1e-5 * np.abs(ref).max())


@pytest.fixture(scope="module")
def golden(golden_dir):
    import os
    return np.load(os.path.join(golden_dir, "grouped.npz"))


def _layer(case, w, b, sc):
    """The drop-in binary layer of a case (prepare_binary_model on the float module), on the GPU, eval mode."""
    if case.conv1d:
        conv = nn.Conv1d(case.C, case.O, case.kw, stride=case.stride, padding=case.pad[1], dilation=case.dilation,
                         groups=case.groups, bias=case.bias)
    else:
        conv = nn.Conv2d(case.C, case.O, (case.kh, case.kw), stride=case.stride, padding=case.pad,
                         dilation=case.dilation, groups=case.groups, bias=case.bias)
    conv.weight.data.copy_(torch.from_numpy(w))
    if b is not None:
        conv.bias.data.copy_(torch.from_numpy(b))
    cfg = bnn.BConfig(activation_pre_process=BasicInputBinarizer,
                      activation_post_process=BasicScaleBinarizer if case.post == "scale" else bnn.Identity,
                      weight_pre_process=XNORWeightBinarizer.with_args(compute_alpha=case.compute_alpha,
                                                                       center_weights=case.center))
    layer = bnn.prepare_binary_model(conv, cfg)
    if sc is not None:
        layer.activation_post_process.alpha.data.copy_(
            torch.from_numpy(sc).view(1, -1, *([1] * (1 if case.conv1d else 2))))
    return layer.to(DEV).eval()


@pytest.mark.parametrize("case", GROUPED_CASES, ids=IDS)
def test_grouped_pack_equals_the_oracle_layout_and_the_dense_alpha(case):
    _, w, _, _ = case.tensors()
    w4 = w[:, :, None, :] if case.conv1d else w
    pw = hipops.pack_weight_grouped(dev(w), case.groups, case.center, case.compute_alpha)
    assert pw.groups == case.groups and pw.windowed and pw.shape == w4.shape
    wb, wz = window_pack(w4, case.groups, case.center)
    assert np.array_equal(pw.wbits.cpu().numpy().view(np.uint32), wb)
    assert np.array_equal(pw.wnz.cpu().numpy().view(np.uint32), wz)
    dense = hipops.pack_weight(dev(w), case.center, case.compute_alpha)
    assert torch.equal(pw.alpha, dense.alpha)
    assert pw.has_zero == dense.has_zero == (case.winit == "withzeros")


@pytest.mark.parametrize("case", GROUPED_CASES, ids=IDS)
def test_every_case_through_bconv2d_grouped(golden, case):
    x, w, b, sc = case.tensors()
    x2, w2, stride, pad, dil = as_2d(case, x, w)
    act = hipops.pack_act(dev(x2))
    pw = hipops.pack_weight_grouped(dev(w2), case.groups, case.center, case.compute_alpha)
    dot = hipops.bconv2d_grouped(act, pw, stride=stride, padding=pad, dilation=dil, raw_dot=True).cpu().numpy()
    ref_dot = oracle_dot(x2, w2, case.groups, stride, pad, dil, case.center)
    assert np.array_equal(dot, ref_dot)
    out = hipops.bconv2d_grouped(act, pw, dev(b), dev(sc), stride, pad, dil).cpu().numpy()
    alpha = pw.alpha[:case.O].cpu().numpy()
    assert np.array_equal(out, oracle.epilogue(dot, alpha, b, sc))
    ref = golden[case.name + "/out"]
    assert close(out.reshape(ref.shape), ref)


@pytest.mark.parametrize("zeros", [False, True])
def test_groups_1_through_the_grouped_entry_equals_bconv2d(zeros):
    x = gen.activation("sparse", 5, (2, 200, 9, 9))
    w = gen.conv_weight("withzeros" if zeros else "kaiming", 6, (72, 200, 3, 3))
    b = (0.1 * gen.normal(7, (72,))).astype(np.float32)
    act = hipops.pack_act(dev(x))
    pg = hipops.pack_weight_grouped(dev(w), 1)
    pd = hipops.pack_weight(dev(w))
    pd.has_zero = True      # BNN_HIP_FLAG_WEIGHT_ZEROS: the zero-aware kernels, the grouped entry's contract
    for s, p in ((1, 1), (2, 0)):
        assert torch.equal(hipops.bconv2d_grouped(act, pg, stride=s, padding=p, raw_dot=True),
                           hipops.bconv2d(act, pd, stride=s, padding=p, raw_dot=True))
        assert torch.equal(hipops.bconv2d_grouped(act, pg, dev(b), None, s, p),
                           hipops.bconv2d(act, pd, dev(b), None, s, p))


def test_dense_entry_points_refuse_a_grouped_pack():
    w = gen.conv_weight("kaiming", 3, (48, 4, 3, 3))
    pw = hipops.pack_weight_grouped(dev(w), 12)
    x = dev(gen.activation("normal", 4, (1, 48, 6, 6)))
    act = hipops.pack_act(x)
    with pytest.raises(NativeError):
        hipops.bconv2d(act, pw, padding=1)
    with pytest.raises(NativeError):
        hipops.bconv2d_direct(x, pw, padding=1)
    with pytest.raises(NativeError):
        hipops.bconv2d_fused(act, pw, padding=1)
    with pytest.raises(NativeError):   # and the grouped entry refuses a dense pack
        hipops.bconv2d_grouped(act, hipops.pack_weight(dev(gen.conv_weight("kaiming", 3, (48, 48, 3, 3)))), padding=1)


@pytest.mark.parametrize("case", GROUPED_CASES, ids=IDS)
def test_layer_forward_takes_the_hip_path(golden, case):
    x, w, b, sc = case.tensors()
    layer = _layer(case, w, b, sc)
    key = "conv1d" if case.conv1d else "conv2d"
    for _ in range(2):
        before = fastpath.stats()
        with torch.no_grad():
            y = layer(dev(x)).cpu().numpy()
        after = fastpath.stats()
        assert after[key] == before[key] + 1, "the grouped layer did not take the HIP path"
        ref = golden[case.name + "/out"]
        assert close(y, ref)
    # and it is the grouped kernel's result, bit for bit
    x2, w2, stride, pad, dil = as_2d(case, x, w)
    direct = hipops.bconv2d_grouped(hipops.pack_act(dev(x2)),
                                    hipops.pack_weight_grouped(dev(w2), case.groups, case.center, case.compute_alpha),
                                    dev(b), dev(sc), stride, pad, dil).cpu().numpy()
    assert np.array_equal(y, direct.reshape(y.shape))


def _channel_shuffle(x, groups):
    n, c, h, w = x.shape
    return x.view(n, groups, c // groups, h, w).transpose(1, 2).contiguous().view(n, -1, h, w)


class _BatsOp(nn.Module):
    """The reference's SepConv / DilConv at stride 1 (bnn/models/layers/bats_ops.py:108-173): BatchNorm -> grouped conv
    (groups = 12) -> PReLU, channel shuffle (4) and the skip add."""

    def __init__(self, C, kernel_size, padding, dilation):
        super().__init__()
        self.op = nn.Sequential(nn.BatchNorm2d(C),
                                nn.Conv2d(C, C, kernel_size, 1, padding, dilation=dilation, groups=12, bias=False),
                                nn.PReLU(num_parameters=C))

    def forward(self, x):
        return x + _channel_shuffle(self.op(x), 4)


@pytest.mark.parametrize("name", list(OP_CASES))
def test_bats_ops_run_their_binary_conv_on_hip(golden, name):
    kw = OP_CASES[name]
    op = _BatsOp(OP_C, kw["kernel_size"], kw["padding"], kw["dilation"])
    cfg = bnn.BConfig(activation_pre_process=BasicInputBinarizer, activation_post_process=bnn.Identity,
                      weight_pre_process=XNORWeightBinarizer)
    op = bnn.prepare_binary_model(op, cfg)
    keys = [str(k) for k in golden["op/" + name + "/keys"]]
    assert list(op.state_dict().keys()) == keys
    shapes = {k: tuple(v.shape) for k, v in op.state_dict().items()}
    op.load_state_dict({k: torch.from_numpy(v) for k, v in gen.model_state(shapes, gen.seed_of("grouped-op", name)).items()})
    op = op.to(DEV).eval()
    n_binary = sum(1 for m in op.modules() if isinstance(m, bnn.layers.Conv2d))
    assert n_binary == 1
    before = fastpath.stats()["conv2d"]
    with torch.no_grad():
        y = op(dev(op_input(name))).cpu().numpy()
    assert fastpath.stats()["conv2d"] == before + n_binary
    assert close(y, golden["op/" + name + "/out"])


def test_half_precision_grouped_layer():
    case = GROUPED_CASES[1]     # 3x3, groups 4, bias
    x, w, b, sc = case.tensors()
    layer = _layer(case, w, b, sc).half()
    xh = dev(x).half()
    before = fastpath.stats()["conv2d"]
    with torch.no_grad():
        y = layer(xh)
    assert fastpath.stats()["conv2d"] == before + 1 and y.dtype == torch.float16
    exp = hipops.bconv2d_grouped(hipops.pack_act(xh), hipops.pack_weight_grouped(layer.weight, case.groups),
                                 layer.bias.float(), None, 1, case.pad).half()
    assert torch.equal(y, exp)
    with torch.no_grad():
        comp = F.conv2d(torch.sign(xh), torch.sign(layer.weight) * layer.weight.abs().mean(dim=(1, 2, 3), keepdim=True),
                        layer.bias, 1, case.pad, 1, case.groups)
    assert torch.allclose(y.float(), comp.float(), rtol=1e-2, atol=1e-2)


def test_strict_weights_and_cache_rebuild(monkeypatch):
    case = GROUPED_CASES[0]
    x, w, b, sc = case.tensors()
    layer = _layer(case, w, b, sc)
    xd = dev(x)
    with torch.no_grad():
        y0 = layer(xd)
        packs = fastpath.stats()["weight_packs"]
        y1 = layer(xd)
        assert fastpath.stats()["weight_packs"] == packs and torch.equal(y0, y1)    # cached
        layer.weight.mul_(-1)                                                        # version bump: rebuilt
        y2 = layer(xd)
        assert fastpath.stats()["weight_packs"] == packs + 1 and torch.equal(y2, -y0)
        layer.weight.data.mul_(-1)                                                   # .data write: not seen ...
        assert torch.equal(layer(xd), y2)
        assert fastpath.invalidate(layer) == 1                                       # ... until invalidate()
        assert torch.equal(layer(xd), y0)
    monkeypatch.setenv("BNN_AMD_STRICT_WEIGHTS", "1")
    with torch.no_grad():
        packs = fastpath.stats()["weight_packs"]
        layer.weight.data.mul_(-1)                                                   # strict: every call re-derives
        assert torch.equal(layer(xd), y2)
        assert torch.equal(layer(xd), y2)
        assert fastpath.stats()["weight_packs"] == packs + 2


def test_training_forward_keeps_the_composition():
    case = GROUPED_CASES[1]
    x, w, b, sc = case.tensors()
    layer = _layer(case, w, b, sc).train()
    ref = copy.deepcopy(layer)
    xa = dev(x).requires_grad_()
    xb = dev(x).requires_grad_()
    before = fastpath.stats()
    y = layer(xa)
    after = fastpath.stats()
    assert after["conv2d"] == before["conv2d"] and after["conv2d_train"] == before["conv2d_train"]
    # the composition the reference runs (bnn/layers/conv.py:90-97), written out
    yr = ref.activation_post_process(
        ref._conv_forward(ref.activation_pre_process(xb), ref.weight_pre_process(ref.weight), ref.bias), xb)
    assert torch.allclose(y, yr, rtol=1e-6, atol=1e-7)
    g = dev(gen.normal(9, tuple(y.shape)))
    y.backward(g)
    yr.backward(g)
    # (the library's convolution backward may pick atomics-based algorithms: equal up to summation order)
    for a, r in ((xa.grad, xb.grad), (layer.weight.grad, ref.weight.grad), (layer.bias.grad, ref.bias.grad)):
        assert torch.allclose(a, r, rtol=1e-5, atol=1e-6 * float(r.abs().max()))


def test_fused_resnet_declines_a_grouped_conv_and_model_call_still_matches():
    net = resnet18()
    net.layer1[0].conv1 = nn.Conv2d(64, 64, 3, padding=1, groups=4, bias=False)
    cfg = bnn.BConfig(activation_pre_process=BasicInputBinarizer, activation_post_process=bnn.Identity,
                      weight_pre_process=XNORWeightBinarizer)
    net = bnn.prepare_binary_model(net, cfg, custom_config_layers_name={"conv1": bnn.BConfig(), "fc": bnn.BConfig()})
    assert net.layer1[0].conv1.groups == 4
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict({k: torch.from_numpy(v) for k, v in gen.model_state(shapes, 1).items()})
    net = net.to(DEV).eval()
    with pytest.raises(FusionError):
        FusedResNet(net)
    x = dev(gen.normal(gen.seed_of("grouped-r18"), (2, 3, 64, 64)))
    with torch.no_grad():
        before = fastpath.stats()["conv2d"]
        y = net(x)
        assert fastpath.stats()["conv2d"] > before          # the per-layer path ran, the grouped layer on HIP
        with per_layer_forward():
            y_ref = net(x)
    assert torch.equal(y, y_ref)


def test_full_size_stem_like_shape_at_batch_256():
    """BATS ImageNet stem-like 3x3 / stride 2, 40 -> 80, groups 4 (two-word windows), 112 x 112, batch 256."""
    G = 4
    x = dev(gen.activation("normal", 21, (16, 40, 112, 112))).repeat(16, 1, 1, 1)
    x[16:] = -x[16:].roll(1, dims=2)          # distinct images past the first 16
    w = dev(gen.conv_weight("kaiming", 22, (80, 10, 3, 3)))
    act = hipops.pack_act(x)
    pw = hipops.pack_weight_grouped(w, G)
    d1 = hipops.bconv2d_grouped(act, pw, stride=2, padding=1, raw_dot=True)
    d2 = hipops.bconv2d_grouped(act, pw, stride=2, padding=1, raw_dot=True)
    assert torch.equal(d1, d2)
    ref = F.conv2d(torch.sign(x[:16]).double(), torch.sign(w).double(), None, 2, 1, 1, G)
    assert torch.equal(d1[:16].double(), ref)
    o1 = hipops.bconv2d_grouped(act, pw, stride=2, padding=1)
    o2 = hipops.bconv2d_grouped(act, pw, stride=2, padding=1)
    assert torch.equal(o1, o2)
    torch.cuda.synchronize()

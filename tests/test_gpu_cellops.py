"""The BATS cell operations as fused HIP launches: the grouped kernel's cell epilogue (bnn_hip_bconv2d_grouped_fused —
PReLU, channel shuffle as the store index, skip) bit for bit against its NumPy float32 restatement on the CPU oracle's
dot; bnn_amd.models.{SepConv, DilConv, ReLUConvBN} dispatching to cellops.FusedCellOp under eval() / no_grad() against
the reference's fixtures (tests/golden/cellops.npz); the executor's cache; determinism at batch 256."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import bnn_amd as bnn
import oracle
from bnn_amd import fastpath, hipops, models
from bnn_amd.cellops import FusedCellOp
from bnn_amd.inference import FusionError, fold_bn, per_layer_forward
from bnn_amd.native import NativeError
from bnn_amd.ops import BasicInputBinarizer, XNORWeightBinarizer
from tests.golden import gen
from tests.golden.cellops_cases import CELL_CASES
from tests.golden.grouped_cases import GROUPED_CASES
from tests.grouped_util import as_2d, oracle_dot

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def close(a, ref):
    """The project's layer bar."""
    return np.allclose(a, ref, rtol=1e-3, atol=1e-5 * np.abs(ref).max())


def binarise(op):
    cfg = bnn.BConfig(activation_pre_process=BasicInputBinarizer, activation_post_process=bnn.Identity,
                      weight_pre_process=XNORWeightBinarizer)
    return bnn.prepare_binary_model(op, cfg)


def build(case, ns=models):
    op = binarise(case.build(ns))
    shapes = {k: tuple(v.shape) for k, v in op.state_dict().items()}
    op.load_state_dict({k: torch.from_numpy(v) for k, v in case.state(shapes).items()})
    return op.to(DEV).eval()


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "cellops.npz"))


# ---- the kernel, bit for bit ---------------------------------------------------------------------------------------
def slopes(O, seed):
    """Per-channel PReLU slopes mixing < 0, 0, (0, 1) and > 1."""
    base = np.array([-0.5, 0.0, 0.25, 1.75], np.float32)[np.arange(O) % 4]
    return (base * (1.0 + 0.1 * gen.uniform(seed, (O,)))).astype(np.float32)


def cell_reference(v, a, sg, res):
    """NumPy float32: PReLU, the permuted assignment, the skip add — each operation rounded on its own."""
    v = v.astype(np.float32)
    if a is not None:
        v = np.where(v >= 0, v, a.astype(np.float32)[None, :, None, None] * v).astype(np.float32)
    O = v.shape[1]
    o = np.arange(O)
    dst = (o % (O // sg)) * sg + o // (O // sg) if sg > 1 else o
    out = np.empty_like(v)
    out[:, dst] = v
    return (res + out).astype(np.float32) if res is not None else out


@pytest.mark.parametrize("case", GROUPED_CASES, ids=[c.name for c in GROUPED_CASES])
def test_cell_epilogue_equals_its_float32_restatement(case):
    x, w, b, sc = case.tensors()
    x2, w2, stride, pad, dil = as_2d(case, x, w)
    act = hipops.pack_act(dev(x2))
    pw = hipops.pack_weight_grouped(dev(w2), case.groups, case.center, case.compute_alpha)
    dot = oracle_dot(x2, w2, case.groups, stride, pad, dil, case.center)
    alpha = pw.alpha[:case.O].cpu().numpy()
    v = oracle.epilogue(dot, alpha, b, sc)
    assert not np.isnan(v).any()
    plain = hipops.bconv2d_grouped(act, pw, dev(b), dev(sc), stride, pad, dil)
    # all three switches off: the bits of bnn_hip_bconv2d_grouped
    off = hipops.bconv2d_grouped_fused(act, pw, dev(b), dev(sc), stride, pad, dil)
    assert torch.equal(off, plain)
    a = slopes(case.O, gen.seed_of("cell-slope", case.name))
    res = gen.normal(gen.seed_of("cell-res", case.name), v.shape)
    n = 0
    for sg in (1, 2, 4):
        if case.O % sg:
            continue
        for prelu in (None, a):
            for r in (None, res):
                y = hipops.bconv2d_grouped_fused(act, pw, dev(b), dev(sc), stride, pad, dil, prelu=dev(prelu),
                                                 shuffle_groups=sg, residual=dev(r)).cpu().numpy()
                want = cell_reference(v, prelu, sg, r)
                assert np.array_equal(y, want), (case.name, sg, prelu is not None, r is not None,
                                                 float(np.abs(y - want).max()))
                n += 1
    assert n >= 8


def test_wrapper_refuses_a_dense_pack_and_bad_arguments():
    x = dev(gen.activation("normal", 4, (1, 48, 6, 6)))
    act = hipops.pack_act(x)
    dense = hipops.pack_weight(dev(gen.conv_weight("kaiming", 3, (48, 48, 3, 3))))
    pw = hipops.pack_weight_grouped(dev(gen.conv_weight("kaiming", 3, (48, 4, 3, 3))), 12)
    with pytest.raises(NativeError):
        hipops.bconv2d_grouped_fused(act, dense, padding=1)
    with pytest.raises(NativeError):
        hipops.bconv2d_grouped_fused(act, pw, padding=1, shuffle_groups=5)
    with pytest.raises(NativeError):
        hipops.bconv2d_grouped_fused(act, pw, padding=1, residual=x[:, :24])
    with pytest.raises(NativeError):
        hipops.bconv2d_grouped_fused(act, pw, padding=1, prelu=torch.ones(3, device=DEV))


# ---- the modules ---------------------------------------------------------------------------------------------------
def explicit(op, x):
    """The two-call composition through hipops, every derived value made from scratch."""
    bn, conv, act = op.op
    a, b = fold_bn(bn)
    planes = hipops.bn_act_pack(x, a, b, relu=False)
    O = conv.out_channels
    slope = act.weight.detach().reshape(-1)
    slope = (slope.expand(O) if slope.numel() == 1 else slope).contiguous()
    if conv.groups != 1:
        pw = hipops.pack_weight_grouped(conv.weight.detach(), conv.groups)
        return hipops.bconv2d_grouped_fused(planes, pw, None, None, conv.stride, conv.padding, conv.dilation, prelu=slope,
                                            shuffle_groups=4, residual=x if op.stride == 1 else None)
    pw = hipops.pack_weight(conv.weight.detach())
    keep = op.stride == 1 and conv.in_channels == conv.out_channels
    return hipops.bconv2d_fused(planes, pw, prelu=slope, residual=x if keep else None, residual_after_act=True,
                                stride=conv.stride, padding=conv.padding, dilation=conv.dilation)[0]


@pytest.mark.parametrize("case", CELL_CASES, ids=[c.name for c in CELL_CASES])
def test_module_call_is_the_fused_pair_of_launches(golden, case):
    op = build(case)
    x = dev(case.input())
    ref = golden[case.name + "/out"]
    for _ in range(2):
        before = fastpath.stats()
        with torch.no_grad():
            y = op(x)
        after = fastpath.stats()
        assert after["cell_op"] == before["cell_op"] + 1, "the operation did not take the fused path"
        assert after["conv2d"] == before["conv2d"]
        err = float(np.abs(y.cpu().numpy() - ref).max())
        print(f"{case.name}: max |y - ref| = {err:.3g}, max |ref| = {np.abs(ref).max():.3g}")
        assert close(y.cpu().numpy(), ref)
    assert op.__dict__["_bnn_auto_op"].calls["fused"] == 2
    assert torch.equal(y, explicit(op, x))
    before = fastpath.stats()
    with torch.no_grad(), per_layer_forward():
        y_layer = op(x)
    after = fastpath.stats()
    assert after["cell_op"] == before["cell_op"] and after["conv2d"] == before["conv2d"] + 1
    assert close(y_layer.cpu().numpy(), ref)
    assert close(y_layer.cpu().numpy(), y.cpu().numpy())
    # training mode and autograd keep the composition
    before = fastpath.stats()["cell_op"]
    assert close(op(x).detach().cpu().numpy(), ref)
    assert fastpath.stats()["cell_op"] == before


def test_prelu_with_one_parameter_is_broadcast():
    case = CELL_CASES[0]
    op = build(case)
    op.op[2] = nn.PReLU(num_parameters=1, init=0.3).to(DEV)
    x = dev(case.input())
    before = fastpath.stats()["cell_op"]
    with torch.no_grad():
        y = op(x)
        assert fastpath.stats()["cell_op"] == before + 1
        with per_layer_forward():
            y_layer = op(x)
    assert close(y.cpu().numpy(), y_layer.cpu().numpy())


def test_environment_switches_and_hooks_decline(monkeypatch):
    case = CELL_CASES[2]
    op = build(case)
    x = dev(case.input())

    def fused_calls(fn):
        before = fastpath.stats()["cell_op"]
        with torch.no_grad():
            fn()
        return fastpath.stats()["cell_op"] - before

    assert fused_calls(lambda: op(x)) == 1
    monkeypatch.setenv("BNN_AMD_AUTOFUSE", "0")
    assert fused_calls(lambda: op(x)) == 0
    monkeypatch.delenv("BNN_AMD_AUTOFUSE")
    monkeypatch.setenv("BNN_AMD_STRICT_WEIGHTS", "1")
    assert fused_calls(lambda: op(x)) == 0
    monkeypatch.delenv("BNN_AMD_STRICT_WEIGHTS")
    h = op.op[1].register_forward_hook(lambda m, i, o: None)
    assert fused_calls(lambda: op(x)) == 0                       # the hook must fire: per layer
    h.remove()
    assert fused_calls(lambda: op(x)) == 1
    with torch.no_grad():
        assert op.__dict__["_bnn_auto_op"].run(op, x[:0]) is None    # an empty batch is declined
    with pytest.raises(FusionError):                             # fp16 / 3-D inputs are not the executor's
        FusedCellOp(op)(x.half())
    with pytest.raises(FusionError):
        FusedCellOp(op)(x[0])


class _BatsOp(nn.Module):
    """The right layout under a class name that is not one of the three."""

    def __init__(self, C):
        super().__init__()
        self.stride, self.skip = 1, True
        self.op = nn.Sequential(nn.BatchNorm2d(C), nn.Conv2d(C, C, 3, 1, 1, groups=12, bias=False),
                                nn.PReLU(num_parameters=C))

    def forward(self, x):
        return x + models.channel_shuffle(self.op(x), 4)


def test_recognition_is_by_the_three_class_names():
    with pytest.raises(FusionError):
        FusedCellOp(binarise(_BatsOp(48)).to(DEV).eval())

    # a class of ANOTHER package with one of the names and the layout (the reference's own), handed over explicitly
    SepConv = type("SepConv", (_BatsOp,), {})
    case = CELL_CASES[0]
    ours = build(case)
    theirs = binarise(SepConv(48)).to(DEV).eval()
    theirs.load_state_dict(ours.state_dict())
    x = dev(case.input())
    before = fastpath.stats()["cell_op"]
    with torch.no_grad():
        y = FusedCellOp(theirs)(x)
        assert fastpath.stats()["cell_op"] == before + 1
        assert torch.equal(y, ours(x))
        assert fastpath.stats()["cell_op"] == before + 2
        theirs(x)                                                # its own forward does not dispatch
        assert fastpath.stats()["cell_op"] == before + 2


# ---- the cache -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [CELL_CASES[0], CELL_CASES[6]], ids=lambda c: c.name)
def test_parameter_writes_reach_the_executor(case):
    op = build(case)
    x = dev(case.input())
    with torch.no_grad():
        y0 = op(x)
        eng = op.__dict__["_bnn_auto_op"].engine
        assert eng is not None and torch.equal(op(x), y0)
        assert op.__dict__["_bnn_auto_op"].engine is eng        # cached

        def data_write(t, fn):
            """A write the version counters do not see: picked up after invalidate()."""
            fn(t.data)
            stale = op(x)
            assert torch.equal(stale, y_prev[0]), "a .data write is not seen before invalidate()"
            fastpath.invalidate(op)
            assert "_bnn_auto_op" not in op.__dict__
            y = op(x)
            assert torch.equal(y, explicit(op, x)) and not torch.equal(y, y_prev[0])
            y_prev[0] = y

        y_prev = [y0]
        data_write(op.op[1].weight, lambda t: t.mul_(-1))
        data_write(op.op[2].weight, lambda t: t.mul_(0.5))
        data_write(op.op[0].running_mean, lambda t: t.add_(0.7))
        data_write(op.op[0].running_var, lambda t: t.mul_(1.5))

        # version-bumping writes need nothing
        for t, fn in ((op.op[1].weight, lambda t: t.mul_(-1)), (op.op[2].weight, lambda t: t.add_(0.25)),
                      (op.op[0].running_mean, lambda t: t.sub_(0.7)), (op.op[0].bias, lambda t: t.add_(0.1))):
            fn(t)
            y = op(x)
            assert torch.equal(y, explicit(op, x)) and not torch.equal(y, y_prev[0])
            y_prev[0] = y

        # train() -> eval() re-derives (writes through .data made in between included)
        op.train()
        op.op[2].weight.data.mul_(2)
        op.eval()
        before = fastpath.stats()["cell_op"]
        y = op(x)
        assert fastpath.stats()["cell_op"] == before + 1
        assert torch.equal(y, explicit(op, x)) and not torch.equal(y, y_prev[0])

    # an explicit executor: refresh()
    with torch.no_grad():
        eng = FusedCellOp(op)
        y1 = eng(x)
        op.op[1].weight.data.mul_(-1)
        assert torch.equal(eng(x), y1)
        eng.refresh()
        assert torch.equal(eng(x), explicit(op, x)) and not torch.equal(eng(x), y1)


# ---- full size -----------------------------------------------------------------------------------------------------
def test_full_size_sepconv_at_batch_256_is_deterministic():
    """SepConv 3x3, 96 channels, groups 12, 32 x 32, batch 256 (the first line of tools/bench_cellops.py)."""
    C, G, HW = 96, 12, 32
    op = binarise(models.SepConv(C, C, 3, 1, 1, groups=G))
    shapes = {k: tuple(v.shape) for k, v in op.state_dict().items()}
    op.load_state_dict({k: torch.from_numpy(v) for k, v in gen.model_state(shapes, gen.seed_of("cell-256")).items()})
    op = op.to(DEV).eval()
    x = dev(gen.activation("normal", 31, (16, C, HW, HW))).repeat(16, 1, 1, 1)
    x[16:] = -x[16:].roll(1, dims=2)          # distinct images past the first 16
    a, b = fold_bn(op.op[0])
    a64, b64 = a.double().view(1, -1, 1, 1), b.double().view(1, -1, 1, 1)
    # no sign() of the checked images may depend on how BatchNorm is rounded: move the few inputs that are too close
    near = (x[:8].double() * a64 + b64).abs() < 1e-4
    x[:8] = torch.where(near, x[:8] + 0.05, x[:8])
    assert float((x[:8].double() * a64 + b64).abs().min()) >= 1e-5
    before = fastpath.stats()["cell_op"]
    with torch.no_grad():
        y1 = op(x)
        y2 = op(x)
    assert fastpath.stats()["cell_op"] == before + 2
    assert torch.equal(y1, y2)
    # the float64 composition of the first 8 images, with the same sign() decisions
    w = op.op[1].weight.detach()
    s = torch.sign(x[:8].double() * a64 + b64)
    dot = F.conv2d(s, torch.sign(w).double(), None, 1, 1, 1, G)
    planes = hipops.bn_act_pack(x[:8], a, b, relu=False)
    pw = hipops.pack_weight_grouped(w, G)
    assert torch.equal(hipops.bconv2d_grouped(planes, pw, stride=1, padding=1, raw_dot=True).double(), dot)
    alpha = w.double().abs().mean(dim=(1, 2, 3)).view(1, -1, 1, 1)
    v = alpha * dot
    v = torch.where(v >= 0, v, op.op[2].weight.detach().double().view(1, -1, 1, 1) * v)
    ref = x[:8].double() + models.channel_shuffle(v, 4)
    # fp32 against float64 with identical integers: alpha is a 72-term fp32 mean (<= 72 * 2^-24 ~ 4e-6 relative), the fma,
    # the slope product and the skip add round once each (2^-24 relative to their results)
    err = float((y1[:8].double() - ref).abs().max())
    print(f"batch 256: max |y - ref64| = {err:.3g}, max |ref| = {float(ref.abs().max()):.3g}")
    assert torch.allclose(y1[:8].double(), ref, rtol=1e-5, atol=1e-5 * float(ref.abs().max()))
    torch.cuda.synchronize()

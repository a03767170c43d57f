"""FactorizedConv ('conv_7x1_1x7') as one HIP launch (bnn_hip_fconv_fused, csrc/fconv.hip) and 'sep_conv_7x7' on the
fused paths: the kernel bit for bit against its NumPy float32 restatement on the CPU oracle's dot (tests/fconv_ref.py)
and against the three-launch composition of the launches the library already had; bnn_amd.models.FactorizedConv
dispatching to cellops.FusedFactorizedConv under eval() / no_grad() against the reference's fixtures
(tests/golden/fconv.npz); the declines; the executor's cache; determinism; sep_conv_7x7 through FusedCellOp / FusedCell."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import bnn_amd as bnn
from bnn_amd import fastpath, hipops, models
from bnn_amd.cellops import FusedCell, FusedCellOp, FusedFactorizedConv
from bnn_amd.inference import FusionError, fold_bn, no_cell_fusion, per_layer_forward
from bnn_amd.native import NativeError
from bnn_amd.ops import BasicInputBinarizer, BasicScaleBinarizer, XNORWeightBinarizer
from tests import fconv_ref
from tests.golden import gen
from tests.golden.fconv_cases import FACTORIZED, SEP7

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def close(a, ref):
    """The project's layer bar."""
    return np.allclose(a, ref, rtol=1e-3, atol=1e-5 * np.abs(ref).max())


def binarise(op, post=bnn.Identity):
    cfg = bnn.BConfig(activation_pre_process=BasicInputBinarizer, activation_post_process=post,
                      weight_pre_process=XNORWeightBinarizer)
    return bnn.prepare_binary_model(op, cfg)


def build(case, ns=models):
    op = binarise(case.build(ns))
    shapes = {k: tuple(v.shape) for k, v in op.state_dict().items()}
    op.load_state_dict({k: torch.from_numpy(v) for k, v in case.state(shapes).items()})
    return op.to(DEV).eval()


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "fconv.npz"))


# ---- (a), (b): the kernel, bit for bit -----------------------------------------------------------------------------
def slopes(O, seed):
    """Per-channel PReLU slopes mixing < 0, 0, (0, 1) and > 1."""
    base = np.array([-0.5, 0.0, 0.25, 1.75], np.float32)[np.arange(O) % 4]
    return (base * (1.0 + 0.1 * gen.uniform(seed, (O,)))).astype(np.float32)


# (name, C, K, stride, N, H, W): the fixture shapes; three plane words with more rows and pixels than one wave; an image
# whose planes of t exceed the 64 KB of LDS (6144 bytes a row at C 192, Wm 128: two bands of three output rows, each
# with its halo); and the other kernel extents, K = 1 with the wide chunks of the 1 x 1 weight layout (C 256: cwc 8)
KERNEL_SHAPES = [(c.name, c.C, 7, c.stride, c.N, c.H, c.W) for c in FACTORIZED] + [
    ("c192", 192, 7, 1, 1, 18, 21),
    ("k3_c192_s2_bands", 192, 3, 2, 1, 11, 255),
    ("k5_c80_s2", 80, 5, 2, 2, 9, 11),
    ("k3_c48", 48, 3, 1, 2, 6, 7),
    ("k1_c256_s2", 256, 1, 2, 2, 5, 6),
]


def composition(planes, p1, p2, mid_a, mid_b, K, s, st1, st2, sg, res):
    """The three-launch composition of the launches the library had before the one-launch kernel."""
    _, t = hipops.bconv2d_fused(planes, p1, stride=(1, s), padding=(0, K // 2), pack_scale=mid_a, pack_shift=mid_b,
                                out_f32=False, out_packed=True, **st1)
    y, _ = hipops.bconv2d_fused(t, p2, stride=(s, 1), padding=(K // 2, 0), **st2)
    y = models.channel_shuffle(y, sg) if sg > 1 else y
    return res + y if res is not None else y.contiguous()


@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=[s[0] for s in KERNEL_SHAPES])
def test_kernel_equals_its_restatement_and_the_three_launch_composition(shape):
    name, C, K, s, N, H, W = shape
    seed = gen.seed_of("fconv-kernel", name)
    x = gen.activation("sparse", seed, (N, C, H, W))            # exact zeros, a dead channel, a zero row: ternary planes
    planes = hipops.pack_act(dev(x))
    a1, a2 = slopes(C, seed + 1), slopes(C, seed + 2)[::-1].copy()
    sign = np.where(gen.uniform(seed + 3, (C,)) < 0.3, -1.0, 1.0)
    mid_a = (sign * (0.5 + gen.uniform(seed + 4, (C,)))).astype(np.float32)
    mid_b = (0.3 * gen.normal(seed + 5, (C,))).astype(np.float32)
    b1, b2 = (0.1 * gen.normal(seed + 6, (C,))).astype(np.float32), (0.1 * gen.normal(seed + 7, (C,))).astype(np.float32)
    sc1, sc2 = (0.5 + gen.uniform(seed + 8, (C,))).astype(np.float32), (0.5 + gen.uniform(seed + 9, (C,))).astype(np.float32)
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    res = gen.normal(seed + 10, (N, C, Ho, Wo))
    n = 0
    for zeros in (False, True):
        kind = "withzeros" if zeros else "kaiming"
        w1, w2 = gen.conv_weight(kind, seed + 11, (C, C, 1, K)), gen.conv_weight(kind, seed + 12, (C, C, K, 1))
        p1, p2 = hipops.pack_weight(dev(w1)), hipops.pack_weight(dev(w2))
        assert p1.has_zero == zeros and p2.has_zero == zeros
        al1, al2 = p1.alpha.cpu().numpy(), p2.alpha.cpu().numpy()
        for extras in (False, True):
            e1 = dict(bias1=b1, scale1=sc1) if extras else {}
            e2 = dict(bias2=b2, scale2=sc2) if extras else {}
            v, t = fconv_ref.fconv(x, w1, w2, al1, al2, mid_a, mid_b, s, prelu1=a1, prelu2=a2, **e1, **e2)
            assert not np.isnan(v).any() and v.shape == (N, C, Ho, Wo)
            assert (t != 0).any()
            st1 = dict(bias=dev(b1) if extras else None, post_scale=dev(sc1) if extras else None, prelu=dev(a1))
            st2 = dict(bias=dev(b2) if extras else None, post_scale=dev(sc2) if extras else None, prelu=dev(a2))
            for sg in (1, 4):
                for r in (None, res):
                    y = hipops.fconv_fused(planes, p1, p2, dev(mid_a), dev(mid_b), stride=s, bias1=st1["bias"],
                                           post_scale1=st1["post_scale"], prelu1=st1["prelu"], bias2=st2["bias"],
                                           post_scale2=st2["post_scale"], prelu2=st2["prelu"], shuffle_groups=sg,
                                           residual=dev(r))
                    want = fconv_ref.shuffle_add(v, sg, r)
                    got = y.cpu().numpy()
                    assert np.array_equal(got, want), (name, zeros, extras, sg, r is not None,
                                                       float(np.abs(got - want).max()), int((got != want).sum()))
                    assert torch.equal(y, composition(planes, p1, p2, dev(mid_a), dev(mid_b), K, s, st1, st2, sg, dev(r)))
                    n += 1
    assert n == 16


@pytest.mark.parametrize("stride, H, W", [(1, 5, 256), (2, 9, 511)])
def test_bands_of_the_7_tap_kernel_equal_the_composition(stride, H, W):
    """C 128 at Wm 256: 8192 bytes a row of t, so 8 rows fit: bands of two output rows at stride 1 (three bands, the last
    of one row), of one row at stride 2 (five bands); every band has rows of t outside the image or in its neighbour."""
    C, K, seed = 128, 7, gen.seed_of("fconv-bands", stride)
    planes = hipops.pack_act(dev(gen.activation("sparse", seed, (2, C, H, W))))
    p1 = hipops.pack_weight(dev(gen.conv_weight("kaiming", seed + 1, (C, C, 1, K))))
    p2 = hipops.pack_weight(dev(gen.conv_weight("withzeros", seed + 2, (C, C, K, 1))))
    mid_a, mid_b = dev((0.5 + gen.uniform(seed + 3, (C,))).astype(np.float32)), dev(0.3 * gen.normal(seed + 4, (C,)))
    st1 = dict(bias=dev(0.1 * gen.normal(seed + 5, (C,))), post_scale=None, prelu=dev(slopes(C, seed + 6)))
    st2 = dict(bias=None, post_scale=None, prelu=dev(slopes(C, seed + 7)))
    res = dev(gen.normal(seed + 8, (2, C, (H - 1) // stride + 1, (W - 1) // stride + 1)))
    assert hipops.fconv_supported(2, C, H, W, K, stride)
    y = hipops.fconv_fused(planes, p1, p2, mid_a, mid_b, stride=stride, bias1=st1["bias"], prelu1=st1["prelu"],
                           prelu2=st2["prelu"], shuffle_groups=4, residual=res)
    assert torch.equal(y, composition(planes, p1, p2, mid_a, mid_b, K, stride, st1, st2, 4, res))
    assert not hipops.fconv_supported(2, C, H, 2 * W * stride, K, stride)      # not even K rows fit: the composition runs


def test_no_prelu_and_wrapper_argument_checks():
    name, C, K, s, N, H, W = KERNEL_SHAPES[0]
    x = gen.activation("normal", 5, (N, C, H, W))
    planes = hipops.pack_act(dev(x))
    w1, w2 = gen.conv_weight("kaiming", 6, (C, C, 1, K)), gen.conv_weight("kaiming", 7, (C, C, K, 1))
    p1, p2 = hipops.pack_weight(dev(w1)), hipops.pack_weight(dev(w2))
    one, zero = np.ones(C, np.float32), np.zeros(C, np.float32)
    y = hipops.fconv_fused(planes, p1, p2, dev(one), dev(zero), stride=s)
    v, _ = fconv_ref.fconv(x, w1, w2, p1.alpha.cpu().numpy(), p2.alpha.cpu().numpy(), one, zero, s)
    assert np.array_equal(y.cpu().numpy(), v)
    assert hipops.fconv_supported(N, C, H, W, K, s) and not hipops.fconv_supported(1, 512, 224, 224, 7, 1)
    with pytest.raises(NativeError):
        hipops.fconv_fused(planes, p2, p1, dev(one), dev(zero))                       # the weights the wrong way round
    with pytest.raises(NativeError):
        hipops.fconv_fused(planes, p1, p2, dev(one), dev(zero), shuffle_groups=5)
    with pytest.raises(NativeError):
        hipops.fconv_fused(planes, p1, p2, dev(one[:3]), dev(zero))
    with pytest.raises(NativeError):
        hipops.fconv_fused(planes, p1, p2, dev(one), dev(zero), residual=dev(x)[:, :24])
    with pytest.raises(NativeError, match="unsupported|status -2"):                   # stride 3: no kernel
        hipops.fconv_fused(planes, p1, p2, dev(one), dev(zero), stride=3)


# ---- (c): the module -----------------------------------------------------------------------------------------------
def vec(act, C):
    w = act.weight.detach().reshape(-1)
    return (w.expand(C) if w.numel() == 1 else w).contiguous()


def explicit(op, x, fused=True):
    """The executor's launches through hipops, every derived value made from scratch."""
    bn1, c1, a1, bn2, c2, a2 = op.op
    C, K, s = c1.in_channels, c1.kernel_size[1], op.stride
    (a, b), (ma, mb) = fold_bn(bn1), fold_bn(bn2)
    planes = hipops.bn_act_pack(x, a, b, relu=False)
    p1, p2 = hipops.pack_weight(c1.weight.detach()), hipops.pack_weight(c2.weight.detach())
    sc = [getattr(c.activation_post_process, "alpha", None) for c in (c1, c2)]
    sc = [None if t is None else t.detach().reshape(-1) for t in sc]
    res = x if s == 1 else None
    if fused:
        return hipops.fconv_fused(planes, p1, p2, ma, mb, stride=s, bias1=c1.bias, post_scale1=sc[0], prelu1=vec(a1, C),
                                  bias2=c2.bias, post_scale2=sc[1], prelu2=vec(a2, C), shuffle_groups=4, residual=res)
    return composition(planes, p1, p2, ma, mb, K, s, dict(bias=c1.bias, post_scale=sc[0], prelu=vec(a1, C)),
                       dict(bias=c2.bias, post_scale=sc[1], prelu=vec(a2, C)), 4, res)


@pytest.mark.parametrize("case", FACTORIZED, ids=[c.name for c in FACTORIZED])
def test_module_call_is_the_pack_and_one_fused_launch(golden, case):
    op = build(case)
    x = dev(case.input())
    ref = golden[case.name + "/out"]
    for _ in range(2):
        before = fastpath.stats()
        with torch.no_grad():
            y = op(x)
        after = fastpath.stats()
        assert after["fconv"] == before["fconv"] + 1, "the operation did not take the fused launch"
        assert after["conv2d"] == before["conv2d"] and after["cell_op"] == before["cell_op"]
        err = float(np.abs(y.cpu().numpy() - ref).max())
        print(f"{case.name}: max |y - ref| = {err:.3g}, max |ref| = {np.abs(ref).max():.3g}")
        assert close(y.cpu().numpy(), ref)
    assert op.__dict__["_bnn_auto_op"].calls["fused"] == 2
    assert torch.equal(y, explicit(op, x)) and torch.equal(y, explicit(op, x, fused=False))
    before = fastpath.stats()
    with torch.no_grad(), per_layer_forward():
        y_layer = op(x)
    after = fastpath.stats()
    assert after["fconv"] == before["fconv"] and after["conv2d"] == before["conv2d"] + 2
    assert close(y_layer.cpu().numpy(), ref)
    assert close(y_layer.cpu().numpy(), y.cpu().numpy())
    # training mode and autograd keep the module's own forward
    before = fastpath.stats()["fconv"]
    assert close(op(x).detach().cpu().numpy(), ref)
    op.train()
    with torch.no_grad():
        op(x)
    assert fastpath.stats()["fconv"] == before


def test_post_scale_bias_and_a_one_parameter_prelu_reach_the_launch():
    case = FACTORIZED[1]
    op = case.build(models)
    op.op[1] = nn.Conv2d(case.C, case.C, (1, 7), stride=(1, case.stride), padding=(0, 3), bias=True)
    op.op[5] = nn.PReLU(num_parameters=1, init=0.3)
    op = binarise(op, post=BasicScaleBinarizer)
    shapes = {k: tuple(v.shape) for k, v in op.state_dict().items()}
    op.load_state_dict({k: torch.from_numpy(v) for k, v in gen.model_state(shapes, gen.seed_of("fconv-scale")).items()})
    op = op.to(DEV).eval()
    assert any(k.endswith("alpha") for k in shapes) and "op.1.bias" in shapes
    x = dev(case.input())
    before = fastpath.stats()["fconv"]
    with torch.no_grad():
        y = op(x)
        assert fastpath.stats()["fconv"] == before + 1
        assert torch.equal(y, explicit(op, x)) and torch.equal(y, explicit(op, x, fused=False))
        with per_layer_forward():
            y_layer = op(x)
    assert close(y.cpu().numpy(), y_layer.cpu().numpy())


def test_where_the_kernel_is_not_taken_the_composition_gives_the_same_bits(monkeypatch):
    case = FACTORIZED[0]
    op = build(case)
    x = dev(case.input())
    with torch.no_grad():
        y = op(x)
        monkeypatch.setitem(fastpath.FCONV_DECLINED_SHAPES, (case.C, case.H, case.W, case.stride), (0.0, 0.0))
        eng = FusedFactorizedConv(op)
        before = fastpath.stats()
        y2 = eng(x)
        after = fastpath.stats()
    assert not eng.takes_fused(x.shape)
    assert after["fconv"] == before["fconv"] and after["conv2d"] == before["conv2d"]
    assert torch.equal(y, y2)


# ---- (d): the declines ---------------------------------------------------------------------------------------------
def test_environment_switches_hooks_and_inputs_decline(monkeypatch):
    case = FACTORIZED[2]
    op = build(case)
    x = dev(case.input())

    def fused_calls(fn):
        before = fastpath.stats()["fconv"]
        fn()
        return fastpath.stats()["fconv"] - before

    def call():
        with torch.no_grad():
            op(x)

    assert fused_calls(call) == 1
    monkeypatch.setenv("BNN_AMD_AUTOFUSE", "0")
    assert fused_calls(call) == 0
    monkeypatch.delenv("BNN_AMD_AUTOFUSE")
    monkeypatch.setenv("BNN_AMD_STRICT_WEIGHTS", "1")
    assert fused_calls(call) == 0
    monkeypatch.delenv("BNN_AMD_STRICT_WEIGHTS")
    h = op.op[4].register_forward_hook(lambda m, i, o: None)
    assert fused_calls(call) == 0                                # the hook must fire: per layer
    h.remove()
    assert fused_calls(call) == 1
    assert fused_calls(lambda: op(x)) == 0                       # autograd recording
    op.train()
    assert fused_calls(call) == 0                                # training mode
    op.eval()
    with torch.no_grad(), per_layer_forward():
        assert fused_calls(lambda: op(x)) == 0
    assert fused_calls(call) == 1
    tier = op.__dict__["_bnn_auto_op"]
    with torch.no_grad():
        assert tier.run(op, x[:0]) is None                       # an empty batch
        assert tier.run(op, x.half()) is None                    # fp16
        assert tier.run(op, x[0]) is None                        # not 4-D
    with pytest.raises(FusionError):
        FusedFactorizedConv(op)(x.half())
    with pytest.raises(FusionError):
        FusedFactorizedConv(op)(x[0])


# ---- (e): the cache ------------------------------------------------------------------------------------------------
def test_parameter_writes_reach_the_executor():
    case = FACTORIZED[0]
    op = build(case)
    x = dev(case.input())
    with torch.no_grad():
        y0 = op(x)
        eng = op.__dict__["_bnn_auto_op"].engine
        assert isinstance(eng, FusedFactorizedConv) and torch.equal(op(x), y0)
        assert op.__dict__["_bnn_auto_op"].engine is eng        # cached
        y_prev = [y0]

        def data_write(t, fn):
            """A write the version counters do not see: picked up after invalidate()."""
            fn(t.data)
            assert torch.equal(op(x), y_prev[0]), "a .data write is not seen before invalidate()"
            fastpath.invalidate(op)
            assert "_bnn_auto_op" not in op.__dict__
            y = op(x)
            assert torch.equal(y, explicit(op, x)) and not torch.equal(y, y_prev[0])
            y_prev[0] = y

        data_write(op.op[1].weight, lambda t: t.mul_(-1))
        data_write(op.op[4].weight, lambda t: t.mul_(-1))
        data_write(op.op[5].weight, lambda t: t.mul_(0.5))
        data_write(op.op[3].running_mean, lambda t: t.add_(0.7))

        # version-bumping writes need nothing
        for t, fn in ((op.op[4].weight, lambda t: t.mul_(-1)), (op.op[2].weight, lambda t: t.sub_(0.8)),
                      (op.op[3].running_var, lambda t: t.mul_(1.5)), (op.op[0].bias, lambda t: t.add_(0.1)),
                      (op.op[3].bias, lambda t: t.add_(0.2))):
            fn(t)
            y = op(x)
            assert torch.equal(y, explicit(op, x)) and not torch.equal(y, y_prev[0])
            y_prev[0] = y

        # train() -> eval() re-derives (writes through .data made in between included)
        op.train()
        op.op[5].weight.data.mul_(2)
        op.eval()
        before = fastpath.stats()["fconv"]
        y = op(x)
        assert fastpath.stats()["fconv"] == before + 1
        assert torch.equal(y, explicit(op, x)) and not torch.equal(y, y_prev[0])

        # an explicit executor: refresh()
        eng = FusedFactorizedConv(op)
        y1 = eng(x)
        op.op[1].weight.data.mul_(-1)
        assert torch.equal(eng(x), y1)
        eng.refresh()
        assert torch.equal(eng(x), explicit(op, x)) and not torch.equal(eng(x), y1)


# ---- (f): recognition ----------------------------------------------------------------------------------------------
class _Factorized(nn.Module):
    """The reference's layout and forward, without any dispatch."""

    def __init__(self, C, K=7, stride=1):
        super().__init__()
        self.stride, self.skip = stride, True
        self.op = nn.Sequential(nn.BatchNorm2d(C), nn.Conv2d(C, C, (1, K), (1, stride), (0, K // 2), bias=False),
                                nn.PReLU(num_parameters=C), nn.BatchNorm2d(C),
                                nn.Conv2d(C, C, (K, 1), (stride, 1), (K // 2, 0), bias=False), nn.PReLU(num_parameters=C))

    def forward(self, x):
        y = models.channel_shuffle(self.op(x), 4)
        return x + y if self.stride == 1 else y


def test_recognition_is_by_the_class_name_and_structure():
    case = FACTORIZED[0]
    with pytest.raises(FusionError):
        FusedFactorizedConv(binarise(_Factorized(case.C)).to(DEV).eval())
    FactorizedConv = type("FactorizedConv", (_Factorized,), {})     # a class of ANOTHER package with the name and layout
    ours = build(case)
    theirs = binarise(FactorizedConv(case.C)).to(DEV).eval()
    theirs.load_state_dict(ours.state_dict())
    x = dev(case.input())
    before = fastpath.stats()["fconv"]
    with torch.no_grad():
        y = FusedFactorizedConv(theirs)(x)
        assert fastpath.stats()["fconv"] == before + 1
        assert torch.equal(y, ours(x))
        assert fastpath.stats()["fconv"] == before + 2
        y_own = theirs(x)                                            # its own forward does not dispatch
        assert fastpath.stats()["fconv"] == before + 2
    assert close(y.cpu().numpy(), y_own.cpu().numpy())
    with pytest.raises(FusionError):
        FusedCellOp(ours)                                            # and it is not one of the three cell operations


# ---- (g): determinism ----------------------------------------------------------------------------------------------
def test_two_runs_at_64x48x16x16_are_bit_equal():
    C = 48
    op = binarise(models.FactorizedConv(C, 7, 1))
    shapes = {k: tuple(v.shape) for k, v in op.state_dict().items()}
    op.load_state_dict({k: torch.from_numpy(v) for k, v in gen.model_state(shapes, gen.seed_of("fconv-64")).items()})
    op = op.to(DEV).eval()
    x = dev(gen.activation("normal", 33, (64, C, 16, 16)))
    before = fastpath.stats()["fconv"]
    with torch.no_grad():
        y1 = op(x)
        y2 = op(x)
        assert fastpath.stats()["fconv"] == before + 2
        assert torch.equal(y1, y2)
        assert torch.equal(y1, explicit(op, x, fused=False))
        with per_layer_forward():
            y_layer = op(x)
    # the per-layer path rounds both BatchNorms its own way: a sign() within rounding of zero may differ, rarely
    same = (y1 == y_layer).float().mean().item()
    print(f"64x48x16x16: {100 * same:.3f} % of the elements equal the per-layer path's bit for bit")
    torch.cuda.synchronize()


# ---- (h): sep_conv_7x7 ---------------------------------------------------------------------------------------------
def explicit_sep(op, x):
    bn, conv, act = op.op
    a, b = fold_bn(bn)
    planes = hipops.bn_act_pack(x, a, b, relu=False)
    pw = hipops.pack_weight_grouped(conv.weight.detach(), conv.groups)
    return hipops.bconv2d_grouped_fused(planes, pw, None, None, conv.stride, conv.padding, conv.dilation,
                                        prelu=vec(act, conv.out_channels), shuffle_groups=4,
                                        residual=x if op.stride == 1 else None)


@pytest.mark.parametrize("case", SEP7, ids=[c.name for c in SEP7])
def test_sep_conv_7x7_takes_the_cell_operation_executor(golden, case):
    op = build(case)
    assert type(op).__name__ == "SepConv" and op.op[1].kernel_size == (7, 7) and op.op[1].groups == 12
    x = dev(case.input())
    ref = golden[case.name + "/out"]
    before = fastpath.stats()
    with torch.no_grad():
        y = op(x)
        after = fastpath.stats()
        assert after["cell_op"] == before["cell_op"] + 1 and after["conv2d"] == before["conv2d"]
        assert isinstance(op.__dict__["_bnn_auto_op"].engine, FusedCellOp)
        print(f"{case.name}: max |y - ref| = {float(np.abs(y.cpu().numpy() - ref).max()):.3g}")
        assert close(y.cpu().numpy(), ref)
        assert torch.equal(y, explicit_sep(op, x))
        with per_layer_forward():
            assert close(op(x).cpu().numpy(), ref)


def test_a_cell_with_sep_conv_7x7_takes_the_cell_executor_and_one_with_a_factorized_conv_fuses_op_by_op():
    def cell_of(normal):
        g = models.Genotype(normal=normal, normal_concat=[2, 3], reduce=normal, reduce_concat=[2, 3])
        cell = binarise(models.Cell(g, 48, 48, 48, False, False))
        shapes = {k: tuple(v.shape) for k, v in cell.state_dict().items()}
        cell.load_state_dict({k: torch.from_numpy(v) for k, v in gen.model_state(shapes, gen.seed_of("fconv-cell")).items()})
        return cell.to(DEV).eval()

    s0, s1 = dev(gen.activation("normal", 41, (2, 48, 8, 8))), dev(gen.activation("normal", 42, (2, 48, 8, 8)))
    cell = cell_of([("sep_conv_7x7", 0), ("sep_conv_3x3", 1), ("sep_conv_7x7", 1), ("skip_connect", 2)])
    before = fastpath.stats()
    with torch.no_grad():
        y = cell(s0, s1, 0.0)
        after = fastpath.stats()
        assert after["cell"] == before["cell"] + 1 and after["cell_op"] == before["cell_op"]
        with no_cell_fusion():
            y_ops = cell(s0, s1, 0.0)
        assert fastpath.stats()["cell"] == after["cell"]
    assert torch.equal(y, y_ops)

    cell = cell_of([("conv_7x1_1x7", 0), ("sep_conv_7x7", 1), ("sep_conv_3x3", 0), ("conv_7x1_1x7", 2)])
    with pytest.raises(FusionError):
        FusedCell(cell)
    before = fastpath.stats()
    with torch.no_grad():
        y = cell(s0, s1, 0.0)
        after = fastpath.stats()
        # the cell runs its own forward; inside it every operation fuses by itself
        assert after["cell"] == before["cell"] and after["fconv"] == before["fconv"] + 2
        assert after["cell_op"] == before["cell_op"] + 4 and after["conv2d"] == before["conv2d"]
        with per_layer_forward():
            y_layer = cell(s0, s1, 0.0)
    assert y.shape == (2, 96, 8, 8) and torch.isfinite(y).all()
    print(f"cell with FactorizedConv: max |fused - per layer| = {float((y - y_layer).abs().max()):.3g}")
    torch.cuda.synchronize()

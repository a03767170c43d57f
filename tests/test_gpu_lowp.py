"""GPU tests of the 16-bit inference path: bf16 sign planes, bf16 input to the one-launch layer and the row-major Linear
kernel, the in-kernel 16-bit output store of ``bnn_hip_bconv2d_direct``, the layers of a ``.bfloat16()`` model and under
autocast in both 16-bit dtypes, and the boundaries of the admission.

Bars: bit-equal to the CPU oracle on the widened input and to the two-launch form; the 16-bit store equal, as int16
patterns with equal NaN positions, to the existing fp32 launch followed by torch's two roundings; modules bit-equal to the
recipe composed from pre-existing pieces, within ``8 u (|ref| + max |ref|)`` of the GPU torch composition in D (u: unit
roundoff of D), and — under autocast — equal to the reference's own stored outputs (tests/golden/lowp_layers.npz).
"""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import bnn_amd as bnn
import oracle
from bnn_amd import fastpath, hipops, native
from bnn_amd.inference import auto_fusion, per_layer_forward
from bnn_amd.models import resnet18
from bnn_amd.ops import BasicInputBinarizer, BasicScaleBinarizer, XNORWeightBinarizer
from tests.golden import gen
from tests.golden import make_golden_lowp as glp
from tests.golden.cases import LAYER_CASES_BY_NAME

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16, BF16 = torch.float16, torch.bfloat16
UNIT = {BF16: 2.0 ** -9, F16: 2.0 ** -11}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bf16_round(a: np.ndarray) -> np.ndarray:
    return glp.round_to(a, "bf16")


def same_patterns(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Equal as int16 patterns, NaN positions equal (a NaN's payload is not compared)."""
    assert a.dtype == b.dtype and a.dtype in (F16, BF16) and a.shape == b.shape
    na, nb = torch.isnan(a), torch.isnan(b)
    return bool(torch.equal(na, nb) and torch.equal(a.view(torch.int16)[~na], b.view(torch.int16)[~nb]))


SPECIAL_BF16 = np.array([0.0, -0.0, np.nan, -np.nan, np.inf, -np.inf, 2.0 ** -133, -2.0 ** -133, 1e-39, -1e-39, 3.0, -2.0],
                        np.float32)


def special_field(seed, shape):
    """Values in bf16 with every special in every bit position of a word (channel c and pixel index are coprime-stepped)."""
    rng = np.random.default_rng(seed)
    x = bf16_round(rng.standard_normal(shape).astype(np.float32))
    idx = (np.arange(x.size).reshape(shape) + np.arange(shape[1]).reshape(1, -1, 1, 1) * 5) % (2 * len(SPECIAL_BF16))
    pick = idx < len(SPECIAL_BF16)
    x[pick] = SPECIAL_BF16[idx[pick]]
    return x


# ---- 1. planes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 3, 4, 6), (3, 70, 3, 6), (2, 96, 5, 7), (2, 70, 8, 8), (3, 3, 5, 7), (1, 96, 1, 2)],
                         ids=str)
def test_bf16_planes_equal_the_oracle_on_the_widened_tensor(shape):
    x = special_field(11, shape)
    a = hipops.pack_act(dev(x).to(BF16))
    P, M = oracle.pack_act(x)
    assert np.array_equal(a.P.cpu().numpy().view(np.uint64), P) and np.array_equal(a.M.cpu().numpy().view(np.uint64), M)


def at_odd_element(x: np.ndarray) -> torch.Tensor:
    """The bf16 tensor of ``x`` as a contiguous view that starts one element into its storage: 2-byte aligned only."""
    flat = torch.empty(x.size + 1, dtype=BF16, device=DEV)
    view = flat[1:].view(x.shape)
    view.copy_(dev(x))
    assert view.data_ptr() % 4 == 2 and view.is_contiguous()
    return view


@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (2, 70, 4, 6), (2, 96, 3, 6), (2, 71, 3, 5)], ids=str)
def test_bf16_planes_of_a_view_at_an_odd_element(shape):
    """HW divisible by 4 or by 2 with a base that is not: the 2-byte-aligned (one pixel per load) kernel has to run."""
    x = special_field(12, shape)
    a = hipops.pack_act(at_odd_element(x))
    P, M = oracle.pack_act(x)
    assert np.array_equal(a.P.cpu().numpy().view(np.uint64), P) and np.array_equal(a.M.cpu().numpy().view(np.uint64), M)
    x3 = special_field(14, (3, 3, 5, 7))                       # the issue's own form: x[1:] with C*H*W odd
    view = dev(x3).to(BF16)[1:]
    assert view.data_ptr() % 4 == 2
    a = hipops.pack_act(view)
    P, M = oracle.pack_act(x3[1:])
    assert np.array_equal(a.P.cpu().numpy().view(np.uint64), P) and np.array_equal(a.M.cpu().numpy().view(np.uint64), M)


# ---- 2. the one-launch layer, bf16 in, fp32 out ---------------------------------------------------------------------
@pytest.mark.parametrize("name", ["l1_64x56", "l2_0_c1_s2", "l2_128x28", "l3_256x14", "l4_512x7", "l2_ds_1x1",
                                  "c1024_1x1", "c2_normal", "special_vals", "tail_c3", "tail_c96", "tail_c200_o5",
                                  "k5_generic", "k3_dil2_generic", "zero_weights", "center_bias_scale"])
def test_direct_layer_bf16_input(name):
    case = LAYER_CASES_BY_NAME[name]
    x, w, b, sc = case.tensors()
    pw = hipops.pack_weight(dev(w), case.center, case.compute_alpha)
    kw = dict(stride=case.stride, padding=case.pad, dilation=case.dilation)
    xb = bf16_round(x)
    bt, st = (None if b is None else dev(b)), (None if sc is None else dev(sc))
    xd = dev(xb).to(BF16)
    out = hipops.bconv2d_direct(xd, pw, bt, st, **kw)
    assert out.dtype == torch.float32
    ref_out, _ = oracle.binary_conv2d_int(xb, w, b, sc, case.stride, case.pad, case.dilation, case.center,
                                          case.compute_alpha)
    assert np.array_equal(out.cpu().numpy(), ref_out)
    assert torch.equal(out, hipops.bconv2d(hipops.pack_act(xd), pw, bt, st, **kw))


def test_direct_layer_bf16_sign_semantics_and_odd_start():
    x = special_field(13, (3, 70, 5, 7))
    w = gen.conv_weight("kaiming", 91, (40, 70, 3, 3))
    pw = hipops.pack_weight(dev(w))
    ref, _ = oracle.binary_conv2d_int(x, w, None, None, 1, 1, 1)
    assert np.array_equal(hipops.bconv2d_direct(at_odd_element(x), pw, padding=1, route="direct").cpu().numpy(), ref)


# ---- 3. the 16-bit store ---------------------------------------------------------------------------------------------
def _plan(images=1, rows=0, waves=8, obw=1):
    p = native.FlyPlan()
    p.images_per_band, p.rows_per_band, p.waves, p.blocks_per_unit = images, rows, waves, obw
    p.pack_ahead = p.fine_head = p.fine_tail = p.producers = -1
    return p


def _store_case(seed, N, C, O, H, W, k, stride, pad, zero_weights=False, big_scale=False, bias=True, scale=True):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, C, H, W)).astype(np.float32)
    w = (rng.standard_normal((O, C, k, k)) * 0.1).astype(np.float32)
    if zero_weights:
        w[rng.random(w.shape) < 0.2] = 0.0
        w[1] = 0.0
    b = rng.standard_normal(O).astype(np.float32) if bias else None
    sc = (0.25 + 3 * rng.random(O)).astype(np.float32) if scale else None
    if big_scale:
        sc[::2] = 1e6
    return x, w, b, sc, dict(stride=stride, padding=pad)


STORE_CASES = {
    "odd_5x7_o5": dict(N=3, C=70, O=5, H=5, W=7, k=3, stride=1, pad=1),                # Ho*Wo = 35: odd image offsets
    "o37_s2": dict(N=2, C=64, O=37, H=9, W=7, k=3, stride=2, pad=1),                   # Ho*Wo = 5*4
    "k1_o37": dict(N=3, C=96, O=37, H=5, W=7, k=1, stride=1, pad=0),
    "full_blocks": dict(N=2, C=128, O=64, H=14, W=14, k=3, stride=1, pad=1),            # the straight-line (FULL) epilogue
    "zero_weights": dict(N=2, C=70, O=37, H=5, W=7, k=3, stride=1, pad=1, zero_weights=True),
    "scale_1e6": dict(N=2, C=64, O=40, H=5, W=7, k=3, stride=1, pad=1, big_scale=True),  # fp16 overflows to inf
    "no_bias_no_scale": dict(N=2, C=8, O=6, H=5, W=5, k=3, stride=1, pad=1, bias=False, scale=False),
    "generic_k5": dict(N=2, C=8, O=5, H=7, W=7, k=5, stride=1, pad=2),
}


def _store_both(D, x, w, b, sc, kw, **extra):
    pw = hipops.pack_weight(dev(w))
    xd = dev(x).to(D)
    bt, st = (None if b is None else dev(b)), (None if sc is None else dev(sc))
    launches = native.launch_count()
    got = hipops.bconv2d_direct(xd, pw, bt, st, out_dtype=D, route="direct", **kw, **extra)
    assert native.launch_count() == launches + 1                   # ONE launch: the store needs no second pass
    want = hipops.bconv2d_direct(xd, pw, bt, None, route="direct", **kw, **extra).to(D)   # the existing fp32 launch + torch
    if st is not None:
        want.mul_(st.view(1, -1, 1, 1))
    assert got.dtype == D
    return got, want, pw, xd, bt, st


@pytest.mark.parametrize("D", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("name", list(STORE_CASES))
def test_16_bit_store_equals_fp32_launch_plus_torch_roundings(name, D):
    x, w, b, sc, kw = _store_case(21, **STORE_CASES[name])
    got, want, *_ = _store_both(D, x, w, b, sc, kw)
    assert same_patterns(got, want)
    if name == "scale_1e6" and D is F16:
        assert torch.isinf(got).any()


@pytest.mark.parametrize("D", [BF16, F16], ids=["bf16", "f16"])
def test_16_bit_store_with_one_row_bands_and_generic_unit(D):
    x, w, b, sc, kw = _store_case(22, N=3, C=70, O=37, H=5, W=7, k=3, stride=1, pad=1)
    got, want, pw, xd, bt, st = _store_both(D, x, w, b, sc, kw, plan=_plan(rows=1, waves=4))   # bands start at odd elements
    assert same_patterns(got, want)
    gen_out = hipops.bconv2d_direct(xd, pw, bt, st, out_dtype=D, force_generic=True, **kw)
    assert same_patterns(gen_out, want)


@pytest.mark.parametrize("D", [BF16, F16], ids=["bf16", "f16"])
def test_16_bit_store_of_a_batch_split_over_launches(D, monkeypatch):
    x, w, b, sc, kw = _store_case(23, N=5, C=70, O=5, H=5, W=7, k=3, stride=1, pad=1)
    whole, want, pw, xd, bt, st = _store_both(D, x, w, b, sc, kw)
    monkeypatch.setattr(hipops, "_MAX_ELEMS", 2 * 70 * 5 * 7)       # two images per launch (the input is the largest tensor)
    launches = native.launch_count()
    split = hipops.bconv2d_direct(xd, pw, bt, st, out_dtype=D, route="direct", **kw)
    assert native.launch_count() == launches + 3
    assert same_patterns(split, want) and same_patterns(whole, want)
    monkeypatch.setattr(hipops, "_MAX_ELEMS", 70 * 5 * 7)           # one image per launch: the output of image 1 starts at
    split1 = hipops.bconv2d_direct(xd, pw, bt, st, out_dtype=D, route="direct", **kw)     # element 5 * 35 = 175, an odd one
    assert same_patterns(split1, want)


@pytest.mark.parametrize("D", [BF16, F16], ids=["bf16", "f16"])
def test_other_routes_apply_the_same_roundings_with_torch(D):
    # tiny images with a 3x3 kernel prefer pack_act + bconv2d (hipops._prefers_two_launches): round_lowp on their fp32 result
    x, w, b, sc, kw = _store_case(24, N=3, C=70, O=37, H=3, W=3, k=3, stride=1, pad=1)
    pw = hipops.pack_weight(dev(w))
    xd, bt, st = dev(x).to(D), dev(b), dev(sc)
    got = hipops.bconv2d_direct(xd, pw, bt, st, out_dtype=D, **kw)
    packed = hipops.bconv2d_direct(xd, pw, bt, st, out_dtype=D, route="packed", **kw)
    one = hipops.bconv2d_direct(xd, pw, bt, st, out_dtype=D, route="direct", **kw)
    want = hipops.bconv2d_direct(xd, pw, bt, None, **kw).to(D).mul_(st.view(1, -1, 1, 1))
    assert got.dtype == D and same_patterns(got, want) and same_patterns(packed, want) and same_patterns(one, want)
    with pytest.raises(ValueError):
        hipops.bconv2d_direct(xd, pw, bt, st, out_dtype=torch.float64, **kw)


@pytest.mark.parametrize("flag", [native.FLAG_OUT_F16, native.FLAG_OUT_BF16])
def test_every_other_fused_entry_point_refuses_the_option(flag):
    lib = native.require()
    x, w, b, sc, kw = _store_case(25, N=2, C=64, O=64, H=6, W=6, k=3, stride=1, pad=1)
    pw, a = hipops.pack_weight(dev(w)), hipops.pack_act(dev(x))
    out = torch.empty((2, 64, 6, 6), device=DEV)
    d = native.ConvDesc(2, 64, 6, 6, 64, 3, 3, 1, 1, 1, 1, 1, 1, flag)
    epi = native.Epilogue(alpha=pw.alpha.data_ptr(), out_f32=out.data_ptr())
    launches = native.launch_count()
    ops = (a.P.data_ptr(), a.M.data_ptr(), pw.wbits.data_ptr(), pw.wnz.data_ptr())
    bad = native.ERR_INVALID_ARG
    assert lib.bnn_hip_bconv2d(ctypes.byref(d), *ops, pw.alpha.data_ptr(), None, None, out.data_ptr(), None) == bad
    assert lib.bnn_hip_bconv2d_fused(ctypes.byref(d), *ops, ctypes.byref(epi), None) == bad
    assert lib.bnn_hip_bconv2d_grouped(ctypes.byref(d), 1, *ops, pw.alpha.data_ptr(), None, None, out.data_ptr(), None) == bad
    assert lib.bnn_hip_bconv2d_grouped_fused(ctypes.byref(d), 1, *ops, pw.alpha.data_ptr(), None, None, None, 1, None,
                                             out.data_ptr(), None) == bad
    assert lib.bnn_hip_bconv2d_mfma_supported(ctypes.byref(d), ctypes.byref(epi)) != 1
    assert lib.bnn_hip_bconv2d_mfma_fused(ctypes.byref(d), ops[0], ops[1], ops[2], ctypes.byref(epi), None) == bad
    assert lib.bnn_hip_bconv2d_dot(ctypes.byref(d), *ops, out.data_ptr(), None) == bad
    assert lib.bnn_hip_bconv2d_f32(ctypes.byref(d), dev(x).data_ptr(), ops[2], ops[3], pw.alpha.data_ptr(), None, None,
                                   out.data_ptr(), out.data_ptr(), None) == bad
    assert native.launch_count() == launches


# ---- 4. the row-major Linear kernel ---------------------------------------------------------------------------------
def test_linear_routes_with_bf16_input():
    rng = np.random.default_rng(31)
    x = special_field(31, (70, 100, 1, 1)).reshape(70, 100)
    w = (rng.standard_normal((37, 100)) * 0.1).astype(np.float32)
    b, sc = rng.standard_normal(37).astype(np.float32), (0.5 + rng.random(37)).astype(np.float32)
    pw = hipops.pack_weight(dev(w))
    xd = dev(x).to(BF16)
    row = hipops.linear(xd, pw, dev(b), dev(sc), route="blinear")
    conv = hipops.linear(xd, pw, dev(b), dev(sc), route="conv")
    assert row.dtype == torch.float32 and torch.equal(row, conv)
    ref, _ = oracle.binary_conv2d_int(x[:, :, None, None], w[:, :, None, None], b, sc)
    assert np.array_equal(row.cpu().numpy(), ref.reshape(70, 37))
    # F odd: the view x[1:] starts at an odd element (2-byte aligned rows)
    x2 = special_field(32, (71, 99, 1, 1)).reshape(71, 99)
    pw2 = hipops.pack_weight(dev(w[:, :99]))
    view = dev(x2).to(BF16)[1:]
    assert view.data_ptr() % 4 == 2
    ref2, _ = oracle.binary_conv2d_int(x2[1:, :, None, None], w[:, :99, None, None])
    assert np.array_equal(hipops.linear(view, pw2, route="blinear").cpu().numpy(), ref2.reshape(70, 37))
    assert np.array_equal(hipops.linear(view, pw2, route="conv").cpu().numpy(), ref2.reshape(70, 37))


# ---- 5. modules ------------------------------------------------------------------------------------------------------
def _cfg(center, scale):
    return bnn.BConfig(activation_pre_process=BasicInputBinarizer,
                       activation_post_process=BasicScaleBinarizer if scale else bnn.Identity,
                       weight_pre_process=XNORWeightBinarizer.with_args(compute_alpha=True, center_weights=center))


def _module(kind, seed, center=True, scale=True):
    torch.manual_seed(seed)
    float_layer = {"conv2d": lambda: nn.Conv2d(70, 37, 3, stride=2, padding=1),
                   "grouped": lambda: nn.Conv2d(96, 96, 3, padding=1, groups=8),
                   "conv1d": lambda: nn.Conv1d(70, 37, 3, padding=1),
                   "linear": lambda: nn.Linear(100, 37)}[kind]()
    layer = bnn.prepare_binary_model(float_layer, _cfg(center, scale))
    if scale:
        layer.activation_post_process.alpha.data.uniform_(0.25, 3.0)
    shape = {"conv2d": (3, 70, 9, 7), "grouped": (2, 96, 5, 7), "conv1d": (3, 70, 11), "linear": (5, 100)}[kind]
    return layer.to(DEV).eval(), torch.randn(shape, device=DEV)


def _recipe(layer, kind, x, D):
    """The layer's value from pre-existing pieces: What_D by the layer's hook, the fp32 pack of its widening with alpha
    replaced by max |What_D|, the fp32 launch, torch's two roundings."""
    what = layer.weight_pre_process(layer.weight).to(D).float()
    groups = getattr(layer, "groups", 1)
    pw = hipops.pack_weight_grouped(what, groups, center=False) if groups != 1 else hipops.pack_weight(what, center=False)
    pw.alpha[:what.shape[0]] = what.abs().flatten(1).amax(1)
    bias = None if layer.bias is None else layer.bias.to(D).float()
    post = layer.activation_post_process
    sc = post.alpha.float() if isinstance(post, BasicScaleBinarizer) else None
    if kind == "linear":
        out = hipops.linear(x, pw, bias, None).to(D)
        return out if sc is None else out.mul_(sc.view(1, -1))
    x4 = x.unsqueeze(2) if kind == "conv1d" else x
    geo = [(1, v[0]) if i != 1 else (0, v[0]) for i, v in enumerate((layer.stride, layer.padding, layer.dilation))] \
        if kind == "conv1d" else [layer.stride, layer.padding, layer.dilation]
    if groups != 1:
        out = hipops.bconv2d_grouped(hipops.pack_act(x4), pw, bias, None, *geo)
    else:
        out = hipops.bconv2d_direct(x4, pw, bias, None, *geo)
    out = out.to(D)
    if sc is not None:
        out.mul_(sc.view(1, -1, 1, 1))
    return out.squeeze(2) if kind == "conv1d" else out


def _composition(layer, x):
    """The torch composition of the same layer (what runs when the HIP path declines), on the GPU."""
    old = fastpath._eligible
    fastpath._eligible = lambda *a: False
    try:
        return layer(x)
    finally:
        fastpath._eligible = old


MODES = [("model", BF16), ("autocast", BF16), ("autocast", F16)]


@pytest.mark.parametrize("mode,D", MODES, ids=["bf16_model", "autocast_bf16", "autocast_f16"])
@pytest.mark.parametrize("kind", ["conv2d", "grouped", "conv1d", "linear"])
def test_modules_in_16_bits(kind, mode, D):
    layer, x = _module(kind, 41)
    counter = "conv2d" if kind == "grouped" else kind
    if mode == "model":
        layer = layer.to(D)
    x = x.to(D)
    with torch.no_grad(), torch.autocast("cuda", dtype=D, enabled=mode == "autocast"):
        n0 = fastpath.stats()[counter]
        y = layer(x)
        assert fastpath.stats()[counter] == n0 + 1 and y.dtype == D
        want = _recipe(layer, kind, x, D)
        n1 = fastpath.stats()[counter]
        ref = _composition(layer, x)
        assert fastpath.stats()[counter] == n1 and ref.dtype == D
    assert same_patterns(y, want)
    r = ref.float()
    err = (y.float() - r).abs()
    bound = 8 * UNIT[D] * (r.abs() + r.abs().max())
    assert bool((err <= bound).all()), float((err / bound).max())


def test_module_without_centring_scale_or_bias_under_autocast():
    layer = bnn.prepare_binary_model(nn.Conv2d(8, 6, 3, padding=1, bias=False), _cfg(False, False)).to(DEV).eval()
    x = torch.randn(2, 8, 5, 5, device=DEV).to(BF16)
    with torch.no_grad(), torch.autocast("cuda", dtype=BF16):
        y = layer(x)
        assert y.dtype == BF16 and same_patterns(y, _recipe(layer, "conv2d", x, BF16))


# ---- 6. golden -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden_lowp():
    with np.load(os.path.join(ROOT, "tests", "golden", "lowp_layers.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name,D", [("bf16", BF16), ("f16", F16)])
@pytest.mark.parametrize("i", range(len(glp.CASES)))
def test_layers_under_autocast_reproduce_the_reference_patterns(golden_lowp, i, name, D):
    t = {k.split("/", 1)[1]: v for k, v in golden_lowp.items() if k.startswith(f"s{i}/")}
    c = dict(zip(glp.FIELDS, t["meta"].tolist()))
    conv = nn.Conv2d(c["C"], c["O"], c["k"], stride=c["stride"], padding=c["pad"], groups=c["groups"], bias=bool(c["bias"]))
    conv.weight.data.copy_(torch.from_numpy(t["w"]))
    if c["bias"]:
        conv.bias.data.copy_(torch.from_numpy(t["b"]))
    layer = bnn.prepare_binary_model(conv, _cfg(bool(c["center"]), bool(c["scale"])))
    if c["scale"]:
        layer.activation_post_process.alpha.data.copy_(torch.from_numpy(t["sc"]).view(1, -1, 1, 1))
    layer = layer.to(DEV).eval()
    x = dev(t["x_" + name]).to(D)
    n0 = fastpath.stats()["conv2d"]
    with torch.no_grad(), torch.autocast("cuda", dtype=D):
        y = layer(x)
    assert fastpath.stats()["conv2d"] == n0 + 1 and y.dtype == D
    want = dev(t["out_" + name]).view(D)
    assert same_patterns(y, want)


# ---- 7. boundaries ---------------------------------------------------------------------------------------------------
def test_cache_keeps_one_pack_per_case():
    layer, x = _module("conv2d", 51)
    with torch.no_grad():
        s0 = fastpath.stats()
        first = layer(x).clone()
        with torch.autocast("cuda", dtype=BF16):
            yb = layer(x.to(BF16))
        with torch.autocast("cuda", dtype=F16):
            yh = layer(x.to(F16))
        again = layer(x)
        s1 = fastpath.stats()
        assert first.dtype == again.dtype == torch.float32 and torch.equal(first, again)
        assert yb.dtype == BF16 and yh.dtype == F16
        assert s1["weight_packs"] == s0["weight_packs"] + 3 and s1["conv2d"] == s0["conv2d"] + 4
        with torch.autocast("cuda", dtype=BF16):                       # every pack is still there
            assert same_patterns(layer(x.to(BF16)), yb)
        with torch.autocast("cuda", dtype=F16):
            assert same_patterns(layer(x.to(F16)), yh)
        assert fastpath.stats()["weight_packs"] == s1["weight_packs"]
        layer.weight.data.mul_(-1.0)                                    # a `.data` write: invalidate() drops all three
        assert fastpath.invalidate(layer) == 3
        with torch.autocast("cuda", dtype=BF16):
            assert not same_patterns(layer(x.to(BF16)), yb)


def test_fp32_input_under_autocast_still_returns_fp32_from_the_hip_path():
    layer, x = _module("conv2d", 52)
    with torch.no_grad():
        plain = layer(x)
        n0 = fastpath.stats()["conv2d"]
        with torch.autocast("cuda", dtype=BF16):
            y = layer(x)
        assert fastpath.stats()["conv2d"] == n0 + 1 and y.dtype == torch.float32 and torch.equal(y, plain)


def test_half_model_is_unchanged():
    layer, x = _module("conv2d", 53)
    layer, xh = layer.half(), x.half()
    with torch.no_grad():
        n0 = fastpath.stats()
        y = layer(xh)
        assert fastpath.stats()["conv2d"] == n0["conv2d"] + 1 and y.dtype == F16
        # the `.half()` rule: alpha rounded to fp16, ONE rounding of the scaled fp32 result
        pw = hipops.pack_weight(layer.weight, True, True)
        want = hipops.bconv2d_direct(xh, pw, layer.bias.float(), layer.activation_post_process.alpha.float(),
                                     layer.stride, layer.padding, layer.dilation).half()
        assert torch.equal(y, want)
        assert fastpath.LOWP_KEY not in layer.__dict__


def test_16_bit_input_with_fp32_weight_and_no_autocast_reaches_the_composition():
    layer, x = _module("conv2d", 54)
    n0 = fastpath.stats()["conv2d"]
    with torch.no_grad(), pytest.raises(RuntimeError):
        layer(x.to(BF16))
    assert fastpath.stats()["conv2d"] == n0


def test_training_under_autocast_stays_on_the_composition():
    layer, x = _module("conv2d", 55)
    layer.train()
    n0 = fastpath.stats()
    with torch.autocast("cuda", dtype=BF16):
        y = layer(x.to(BF16))
    assert y.dtype == BF16 and y.requires_grad
    n1 = fastpath.stats()
    assert n1["conv2d"] == n0["conv2d"] and n1["conv2d_train"] == n0["conv2d_train"]


def test_fused_executor_declines_a_bf16_resnet_and_the_model_runs_per_layer():
    net = bnn.prepare_binary_model(resnet18(), _cfg(False, False),
                                   custom_config_layers_name={"conv1": bnn.BConfig(), "fc": bnn.BConfig()})
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict({k: torch.from_numpy(v) for k, v in gen.model_state(shapes, 1).items()})
    net = net.to(DEV).eval().bfloat16()
    x = torch.randn(2, 3, 32, 32, device=DEV).to(BF16)
    st = auto_fusion(net)
    with torch.no_grad():
        n0 = fastpath.stats()["conv2d"]
        with per_layer_forward():
            per_layer = net(x)
        n1 = fastpath.stats()["conv2d"]
        assert n1 - n0 == 19 and per_layer.dtype == BF16                 # every binary conv on the 16-bit HIP path
        declined = st.calls["declined"]
        y = net(x)          # asks the model tier and, inside the model's own forward, every block tier: a bf16 input, all decline
        assert st.calls["declined"] == declined + 1 and st.engine is None
        assert fastpath.stats()["conv2d"] - n1 == 19 and same_patterns(y, per_layer)
        assert all(b.__dict__[fastpath.BLOCK_KEY].calls["fused"] == 0 for b in net.modules()
                   if fastpath.BLOCK_KEY in b.__dict__)


def test_real_weight_layer_still_declines_under_autocast(monkeypatch):
    monkeypatch.setattr(fastpath, "REAL_WEIGHTS", True)
    cfg = bnn.BConfig(activation_pre_process=BasicInputBinarizer, activation_post_process=BasicScaleBinarizer,
                      weight_pre_process=nn.Identity)
    layer = bnn.prepare_binary_model(nn.Conv2d(64, 64, 3, padding=1), cfg).to(DEV).eval()
    x = torch.randn(2, 64, 8, 8, device=DEV)
    with torch.no_grad():
        n0 = fastpath.stats()
        layer(x)
        assert fastpath.stats()["conv2d_real"] == n0["conv2d_real"] + 1             # the switch is on and the layer takes it
        with torch.autocast("cuda", dtype=BF16):
            y = layer(x.to(BF16))
            y32 = layer(x)
        n1 = fastpath.stats()
        assert y.dtype == BF16 and y32.dtype == BF16                                 # the composition, under autocast
        assert n1["conv2d_real"] == n0["conv2d_real"] + 1 and n1["conv2d"] == n0["conv2d"]

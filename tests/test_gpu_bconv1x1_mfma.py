"""The 1x1 binary convolution on the FP4 matrix cores (csrc/bconv1x1_mfma.hip: v_mfma_f32_16x16x128_f8f6f4 with E2M1
operands) against the popcount kernels, bit for bit.

Every case runs bnn_hip_bconv1x1_mfma4_fused and bnn_hip_bconv2d_fused on the same operands and compares with
torch.equal: fp32 outputs as bit patterns (through an int32 view) and both planes word for word.  The plain profile with
alpha = 1 is also compared with the CPU oracle's integer dot.

Shapes: the smallest that reach each way the kernel can go wrong — see SHAPES.  Epilogues: the forms (a) to (f) the fused
executor issues for the 1x1 launches of a Bottleneck and of a PreBottleneck — see epilogue()."""
import functools

import numpy as np
import pytest
import torch

import oracle
from bnn_amd import hipops, native
from tests.golden import gen
from tests.test_gpu_bconv_mfma import same
from tests.test_gpu_bconv_routes import affine, dev, packed_input

pytestmark = pytest.mark.gpu

SHAPES = {      # name -> (N, C, H, W, O)
    # one k-step, 189 pixels: one ragged 256 x 64 tile spanning three images
    "c128-o64-3x9x7": (3, 128, 9, 7, 64),
    # the other tile shape, 128 x 128: two tiles, the second ragged
    "c128-o128-3x9x7": (3, 128, 9, 7, 128),
    # two k-steps, three 64-channel tiles (no power of two), 245 pixels
    "c256-o192-5x7x7": (5, 256, 7, 7, 192),
    # four k-steps, 18 pixels
    "c512-o64-2x3x3": (2, 512, 3, 3, 64),
    # sixteen k-steps, the widest layer, a tile that is almost all padding columns
    "c2048-o64-1x2x2": (1, 2048, 2, 2, 64),
    # 544 pixels: full tiles plus a ragged one, several channel blocks
    "c128-o256-2x17x16": (2, 128, 17, 16, 256),
}
FIRST = "c128-o64-3x9x7"
FORMS = ("PLAIN", "PLAIN1", "BIAS", "SCALE",                    # (a)
         "MID", "MIDT",                                         # (b) BN + ReLU -> planes, without / with thresholds
         "DS",                                                  # (c) BN -> fp32: the shortcut convolution
         "LAST", "OUT",                                         # (d) BN + residual + ReLU -> fp32, without / with planes
         "E_RELU", "E_PRELU",                                   # (e) activation -> pack affine -> planes only
         "F_RELU", "F_PRELU", "F_RELU_PACK", "F_PRELU_PACK")    # (f) activation -> late residual -> fp32 [+ planes]


@functools.lru_cache(maxsize=None)
def operands(shape_id, nn, wz):
    """Input (ternary with exact zeros planted, or non-negative), weight, computed once and shared read-only."""
    N, C, H, W, O = SHAPES[shape_id]
    s = gen.seed_of("mfma1x1", shape_id, nn, wz)
    x = gen.activation("relu" if nn else "normal", s, (N, C, H, W)).copy()
    x.reshape(-1)[:: 7] = 0.0                          # exact zeros: neither plane
    w = gen.conv_weight("withzeros" if wz else "kaiming", s + 1, (O, C, 1, 1))
    x.setflags(write=False)
    w.setflags(write=False)
    return x, w


def epilogue(form, O, out_shape, seed):
    a, b = affine(O, seed)
    pa, pb = affine(O, seed + 10)
    res = gen.normal(seed + 2, out_shape)
    bias = (0.1 * gen.normal(seed + 3, (O,))).astype(np.float32)
    scale = (0.5 + gen.uniform(seed + 4, (O,))).astype(np.float32)
    slope = (0.05 + 0.4 * gen.uniform(seed + 5, (O,))).astype(np.float32)      # PReLU, positive slopes
    bn = dict(bn_scale=a, bn_shift=b)
    aff = dict(pack_scale=pa, pack_shift=pb)
    late = dict(residual=res, residual_after_act=True, out_f32=True)
    return {
        "PLAIN": dict(), "PLAIN1": dict(), "BIAS": dict(bias=bias), "SCALE": dict(post_scale=scale),
        "MID": dict(**bn, relu=True, out_f32=False, out_packed=True),
        "MIDT": dict(**bn, relu=True, out_f32=False, out_packed=True),
        "DS": dict(**bn, out_f32=True, out_packed=False),
        "LAST": dict(**bn, residual=res, relu=True, out_f32=True, out_packed=False),
        "OUT": dict(**bn, residual=res, relu=True, out_f32=True, out_packed=True),
        "E_RELU": dict(relu=True, **aff, out_f32=False, out_packed=True),
        "E_PRELU": dict(prelu=slope, **aff, out_f32=False, out_packed=True),
        "F_RELU": dict(relu=True, **late, out_packed=False),
        "F_PRELU": dict(prelu=slope, **late, out_packed=False),
        "F_RELU_PACK": dict(relu=True, **late, **aff, out_packed=True),
        "F_PRELU_PACK": dict(prelu=slope, **late, **aff, out_packed=True),
    }[form]


def run_both(shape_id, form, nn, wz=False):
    """(FP4 result, popcount result, (x, w)); the matrix-core call is exactly one launch."""
    N, C, H, W, O = SHAPES[shape_id]
    x, w = operands(shape_id, nn, wz)
    act = packed_input(x, nn)
    pw = hipops.pack_weight(dev(w))
    assert pw.has_zero == wz
    if form == "PLAIN1":
        pw.alpha[:] = 1.0
    w4 = hipops.pack_weight1x1_f4(pw)
    assert w4 is not None and 2 * w4.numel() == O * C
    kw = {k: dev(v) if isinstance(v, np.ndarray) else v
          for k, v in epilogue(form, O, (N, O, H, W), gen.seed_of("mfma1x1-epi", shape_id, form)).items()}
    if form == "MIDT":
        kw["sign_thresholds"] = hipops.sign_thresholds(pw, kw["bn_scale"], kw["bn_shift"])
    geo = dict(stride=1, padding=0, dilation=1)
    want = hipops.bconv2d_fused(act, pw, **kw, **geo)
    before = native.launch_count()
    got = hipops.bconv1x1_mfma4_fused(act, pw, w4, **kw, **geo)
    assert native.launch_count() == before + 1
    return got, want, (x, w)


def check(shape_id, form, nn, wz=False):
    (y, pk), (y_pop, pk_pop), (x, w) = run_both(shape_id, form, nn, wz)
    assert (y is None) == (y_pop is None) and (pk is None) == (pk_pop is None)
    assert same(y, y_pop) and same(pk, pk_pop)
    if form == "PLAIN1":      # alpha = 1, no bias: the fp32 output IS the integer dot — against the oracle's
        _, dot = oracle.binary_conv2d_int(x, w, None, None, 1, 0, 1)
        assert np.array_equal(y.cpu().numpy(), dot.astype(np.float32))


# the plain form (on ternary input: both planes live) and form (d) with fp32 and planes on every shape
CASES = [(s, f, nn) for s in SHAPES for f, nn in (("PLAIN1", False), ("OUT", True))]
# every form, both input kinds, on the first shape
CASES += [(FIRST, f, nn) for f in FORMS for nn in (False, True) if (FIRST, f, nn) not in CASES]
# the pre-activation forms once in the 128 x 128 tile and over several k-steps
CASES += [("c128-o128-3x9x7", f, False) for f in ("E_PRELU", "F_PRELU_PACK", "MIDT", "DS")]
CASES += [("c256-o192-5x7x7", f, False) for f in ("E_RELU", "F_RELU_PACK")]


@pytest.mark.parametrize("shape_id,form,nn", CASES, ids=lambda v: str(v))
def test_fp4_1x1_conv_equals_the_popcount_conv(shape_id, form, nn):
    check(shape_id, form, nn)


@pytest.mark.parametrize("form,nn", [("PLAIN1", False), ("OUT", True), ("F_PRELU_PACK", False)])
def test_zero_weights_are_honoured(form, nn):
    check(FIRST, form, nn, wz=True)


def test_the_same_launch_twice_gives_the_same_bits():
    first = run_both("c256-o192-5x7x7", "OUT", True)[0]
    second = run_both("c256-o192-5x7x7", "OUT", True)[0]
    assert same(first[0], second[0]) and same(first[1], second[1])


REFUSED = {     # what -> (C, O, kernel, geometry and epilogue keywords)
    "C = 64": (64, 64, 1, dict()),
    "C = 192": (192, 64, 1, dict()),
    "O = 96": (128, 96, 1, dict()),
    "3x3": (128, 64, 3, dict(padding=1)),
    "stride 2": (128, 64, 1, dict(stride=2)),
    "padding 1": (128, 64, 1, dict(padding=1)),
    "dilation 2": (128, 64, 1, dict(dilation=2)),
    "folded shortcut": (128, 128, 1, dict(shortcut=True)),
    "channel window": (128, 64, 1, dict(window=True)),
    "forced generic": (128, 64, 1, dict(force_generic=True)),
}


@pytest.mark.parametrize("what", list(REFUSED))
def test_refused_cases_raise_and_launch_nothing(what):
    C, O, k, kw = REFUSED[what]
    kw = dict(kw)
    N, H, W = 2, 9, 7
    x = gen.activation("relu", 5, (N, C, H, W))
    act, pw = packed_input(x, True), hipops.pack_weight(dev(gen.conv_weight("kaiming", 6, (O, C, k, k))))
    geo = dict(stride=kw.pop("stride", 1), padding=kw.pop("padding", 0), dilation=kw.pop("dilation", 1))
    query = dict(geo)
    if kw.pop("shortcut", False):
        a, b = (dev(v) for v in affine(O, 9))
        sw = hipops.pack_weight(dev(gen.conv_weight("kaiming", 7, (O, 64, 1, 1))))
        kw = dict(shortcut=(packed_input(gen.activation("relu", 8, (N, 64, H, W)), True), sw, a, b), bn_scale=a, bn_shift=b,
                  relu=True, out_f32=True, out_packed=True)
        query.update(bn=True, relu=True, out_packed=True, shortcut=True)
    if kw.pop("window", False):
        kw = dict(out=torch.zeros((N, 80, H, W), device="cuda:0"), out_c_offset=3)
        query.update(out_c_total=80)
    if kw.get("force_generic"):
        assert hipops.bconv1x1_mfma4_supported(act.shape, pw, nonneg=True, **query)     # the flag alone refuses it
    else:
        assert not hipops.bconv1x1_mfma4_supported(act.shape, pw, nonneg=True, **query)
    # any aligned buffer stands in for the pack: a refused call must not get as far as reading it
    w4 = hipops.pack_weight1x1_f4(pw)
    if w4 is None:
        assert what in ("C = 64", "C = 192", "O = 96", "3x3")
        w4 = torch.zeros(max(int(native.require().bnn_hip_weight1x1_f4_bytes(O, C)), 16), dtype=torch.int8, device="cuda:0")
    torch.cuda.synchronize()
    before = native.launch_count()
    with pytest.raises(native.NativeError):
        hipops.bconv1x1_mfma4_fused(act, pw, w4, **geo, **kw)
    assert native.launch_count() == before

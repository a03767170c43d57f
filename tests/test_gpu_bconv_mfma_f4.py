"""The FP4 form of the matrix-core convolution (csrc/bconv_mfma.hip, F4: v_mfma_f32_16x16x128_f8f6f4 with E2M1 operands)
against the popcount kernels AND the int8 form, bit for bit.

Every case runs bnn_hip_bconv2d_mfma4_fused, bnn_hip_bconv2d_fused and bnn_hip_bconv2d_mfma_fused on the same operands
and compares with torch.equal: fp32 outputs as bit patterns (through an int32 view) and both planes word for word.  The
plain profile with alpha = 1 is also compared with the CPU oracle's integer dot.

Shapes: the smallest that reach each way the FP4 form can go wrong — see SHAPES."""
import numpy as np
import pytest
import torch

import oracle
from bnn_amd import hipops, native
from tests import test_gpu_bconv_mfma as i8
from tests.golden import gen
from tests.test_gpu_bconv_mfma import PROFILES, epilogue, same
from tests.test_gpu_bconv_routes import affine, dev, packed_input

pytestmark = pytest.mark.gpu

# name -> (N, C, H, W, O, stride); operands() of the int8 tests reads them from its own table
SHAPES = {
    # a 256 x 64 tile spanning all three images, one k-step per tap (one 128-channel group)
    "f4-c128-o64-3x9x7": (3, 128, 9, 7, 64, 1),
    # the 128 x 128 tile: two tiles, the second ragged
    "f4-c128-o128-3x9x7": (3, 128, 9, 7, 128, 1),
    # two k-steps per tap, three 64-channel tiles (no power of two), 245 pixels: a ragged tile
    "f4-c256-o192-5x7x7": (5, 256, 7, 7, 192, 1),
    # four k-steps per tap, an image smaller than its halo
    "f4-c512-o64-2x3x3": (2, 512, 3, 3, 64, 1),
    # stride 2 in both tiles, even and odd extents.  (At stride 2 an even width costs four input pixels per output pixel,
    # so the patch of a 256-pixel tile never fits the LDS: choose_tile refuses 14x14 -> O = 64 for the int8 form too — see
    # REFUSED_BY_BOTH.  The 256 x 64 tile therefore meets stride 2 at even H x odd W — all four patch slots per thread —
    # and even x even extents meet it in the 128 x 128 tile.)
    "f4-c128-o64-2x14x7-s2": (2, 128, 14, 7, 64, 2),
    "f4-c128-o128-2x14x14-s2": (2, 128, 14, 14, 128, 2),
    "f4-c128-o256-3x9x7-s2": (3, 128, 9, 7, 256, 2),
}
REFUSED_BY_BOTH = (2, 128, 14, 14, 64, 2)
i8.SHAPES.update(SHAPES)          # (new names only: the int8 cases keep theirs)
FIRST = "f4-c128-o64-3x9x7"


def run_all(shape_id, profile, nn, wz=False):
    """(FP4 result, popcount result, int8 result, (x, w, stride)); each matrix-core call is exactly one launch."""
    N, C, H, W, O, stride = SHAPES[shape_id]
    x, w = i8.operands(shape_id, nn, wz)
    act = packed_input(x, nn)
    pw = hipops.pack_weight(dev(w))
    assert pw.has_zero == wz
    if profile == "PLAIN1":
        pw.alpha[:] = 1.0
    w8, w4 = hipops.pack_weight_i8(pw), hipops.pack_weight_f4(pw)
    assert w8 is not None and w4 is not None and 2 * w4.numel() == w8.numel() == 9 * O * C
    ho, wo = hipops.conv_out_hw(H, W, 3, 3, stride, 1, 1)
    kw = {k: dev(v) if isinstance(v, np.ndarray) else v
          for k, v in epilogue(profile, O, (N, O, ho, wo), gen.seed_of("mfma-epi", shape_id, profile)).items()}
    if profile == "MIDT":
        kw["sign_thresholds"] = hipops.sign_thresholds(pw, kw["bn_scale"], kw["bn_shift"])
    geo = dict(stride=stride, padding=1, dilation=1)
    popcount = hipops.bconv2d_fused(act, pw, **kw, **geo)
    int8 = hipops.bconv2d_mfma_fused(act, pw, w8, **kw, **geo)
    before = native.launch_count()
    got = hipops.bconv2d_mfma4_fused(act, pw, w4, **kw, **geo)
    assert native.launch_count() == before + 1
    return got, popcount, int8, (x, w, stride)


def check(shape_id, profile, nn, wz=False):
    (y, pk), (y_pop, pk_pop), (y_i8, pk_i8), (x, w, stride) = run_all(shape_id, profile, nn, wz)
    assert same(y, y_pop) and same(pk, pk_pop)
    assert same(y, y_i8) and same(pk, pk_i8)
    if profile == "PLAIN1":      # alpha = 1, no bias: the fp32 output IS the integer dot — against the oracle's
        _, dot = oracle.binary_conv2d_int(x, w, None, None, stride, 1, 1)
        assert np.array_equal(y.cpu().numpy(), dot.astype(np.float32))


# PLAIN1 on ternary input with exact zeros planted: both planes live, M -> 0xA; MID and OUT on non-negative input
CASES = [(s, p, nn) for s in SHAPES for p, nn in (("PLAIN1", False), ("MID", True), ("OUT", True))]
# every profile, both input kinds, on the first shape
CASES += [(FIRST, p, nn) for p in PROFILES for nn in (False, True) if (FIRST, p, nn) not in CASES]


@pytest.mark.parametrize("shape_id,profile,nn", CASES, ids=lambda v: str(v))
def test_fp4_conv_equals_the_popcount_and_the_int8_conv(shape_id, profile, nn):
    check(shape_id, profile, nn)


@pytest.mark.parametrize("profile,nn", [("PLAIN1", False), ("OUT", True)])
def test_zero_weights_are_honoured(profile, nn):
    check(FIRST, profile, nn, wz=True)


def test_the_same_launch_twice_gives_the_same_bits():
    first = run_all("f4-c256-o192-5x7x7", "OUT", True)[0]
    second = run_all("f4-c256-o192-5x7x7", "OUT", True)[0]
    assert same(first[0], second[0]) and same(first[1], second[1])


def test_a_tile_that_fits_no_lds_is_refused_like_the_int8_form():
    N, C, H, W, O, stride = REFUSED_BY_BOTH
    x = gen.activation("relu", 15, (N, C, H, W))
    act, pw = packed_input(x, True), hipops.pack_weight(dev(gen.conv_weight("kaiming", 16, (O, C, 3, 3))))
    assert not hipops.bconv2d_mfma_supported(act.shape, pw, nonneg=True, stride=stride, padding=1)
    assert not hipops.bconv2d_mfma4_supported(act.shape, pw, nonneg=True, stride=stride, padding=1)
    w4 = hipops.pack_weight_f4(pw)
    torch.cuda.synchronize()
    before = native.launch_count()
    with pytest.raises(native.NativeError, match=r"status -2"):
        hipops.bconv2d_mfma4_fused(act, pw, w4, stride=stride, padding=1, dilation=1)
    assert native.launch_count() == before


@pytest.mark.parametrize("what", ["c64", "c192", "shortcut"])
def test_refused_shapes_launch_nothing(what):
    N, C, H, W, O = 2, {"c64": 64, "c192": 192, "shortcut": 128}[what], 9, 7, 128
    x = gen.activation("relu", 5, (N, C, H, W))
    w = gen.conv_weight("kaiming", 6, (O, C, 3, 3))
    act, pw = packed_input(x, True), hipops.pack_weight(dev(w))
    kw = {}
    if what == "shortcut":
        sx = gen.activation("relu", 8, (N, 64, H, W))
        a, b = (dev(v) for v in affine(O, 9))
        kw = dict(shortcut=(packed_input(sx, True), hipops.pack_weight(dev(gen.conv_weight("kaiming", 7, (O, 64, 1, 1)))),
                            a, b), bn_scale=a, bn_shift=b, relu=True, out_f32=True, out_packed=True)
        assert hipops.bconv2d_mfma4_supported(act.shape, pw, nonneg=True, padding=1)
        assert not hipops.bconv2d_mfma4_supported(act.shape, pw, nonneg=True, padding=1, bn=True, relu=True,
                                                  out_packed=True, shortcut=True)
    else:
        assert hipops.bconv2d_mfma_supported(act.shape, pw, nonneg=True, padding=1)        # the int8 form takes it
        assert not hipops.bconv2d_mfma4_supported(act.shape, pw, nonneg=True, padding=1)
    # any aligned buffer stands in for the pack: an unsupported call must not get as far as reading it
    w4 = hipops.pack_weight_f4(pw)
    if w4 is None:
        assert what in ("c64", "c192")
        w4 = torch.zeros(9 * O * C // 2, dtype=torch.int8, device="cuda:0")
    torch.cuda.synchronize()
    before = native.launch_count()
    with pytest.raises(native.NativeError):
        hipops.bconv2d_mfma4_fused(act, pw, w4, stride=1, padding=1, dilation=1, **kw)
    assert native.launch_count() == before

"""The int8 matrix-core convolution (csrc/bconv_mfma.hip) against the popcount kernels, bit for bit.

Every case runs bnn_hip_bconv2d_mfma_fused and bnn_hip_bconv2d_fused on the same operands and compares with torch.equal:
fp32 outputs as bit patterns (through an int32 view, so that a NaN equals the same NaN) and both planes word for word.
The plain profile with alpha = 1 is also compared with the CPU oracle's integer dot, so the MFMA kernel meets the oracle
directly and not only through the popcount kernels.

Shapes: the smallest that reach each way the kernel can go wrong — see SHAPES."""
import functools

import numpy as np
import pytest
import torch

import oracle
from bnn_amd import hipops, native
from tests.golden import gen
from tests.test_gpu_bconv_routes import affine, dev, packed_input

pytestmark = pytest.mark.gpu

# name -> (N, C, H, W, O, stride)
SHAPES = {
    # odd sizes, a 256-pixel tile that spans all three images, borders on every side
    "c64-o64-3x9x7": (3, 64, 9, 7, 64, 1),
    # 245 pixels: one ragged tile; three 64-channel tiles (no power of two); two k-steps per tap
    "c128-o192-5x7x7": (5, 128, 7, 7, 192, 1),
    # an image smaller than the halo (every pixel touches a border), four k-steps per tap, 18 pixels in one tile
    "c256-o64-2x3x3": (2, 256, 3, 3, 64, 1),
    # stride 2, even and odd extents; O = 128 with C = 64 keeps the 256 x 64 tile
    "c64-o128-2x14x14-s2": (2, 64, 14, 14, 128, 2),
    "c64-o128-3x9x7-s2": (3, 64, 9, 7, 128, 2),
    # the widest patch per output pixel: stride 2 in the 256-pixel tile (O = 64 has no other)
    "c64-o64-3x9x7-s2": (3, 64, 9, 7, 64, 2),
    # the 128-pixel x 128-channel tile (C >= 128, O % 128 == 0): two tiles, the second ragged; and at stride 2
    "c128-o128-3x9x7": (3, 128, 9, 7, 128, 1),
    "c128-o256-3x9x7-s2": (3, 128, 9, 7, 256, 2),
}
PROFILES = ("PLAIN", "PLAIN1", "BIAS", "SCALE", "MID", "MIDT", "OUT", "OUTP", "LAST", "RUNTIME")


@functools.lru_cache(maxsize=None)
def operands(shape_id, nn, wz):
    """Input (ternary with exact zeros planted, or non-negative), weight, computed once and shared read-only."""
    N, C, H, W, O, stride = SHAPES[shape_id]
    s = gen.seed_of("mfma", shape_id, nn, wz)
    x = gen.activation("relu" if nn else "normal", s, (N, C, H, W)).copy()
    x.reshape(-1)[:: 7] = 0.0                          # exact zeros: neither plane
    w = gen.conv_weight("withzeros" if wz else "kaiming", s + 1, (O, C, 3, 3))
    x.setflags(write=False)
    w.setflags(write=False)
    return x, w


def epilogue(profile, O, out_shape, seed):
    a, b = affine(O, seed)
    res = gen.normal(seed + 2, out_shape)
    bias = (0.1 * gen.normal(seed + 3, (O,))).astype(np.float32)
    scale = (0.5 + gen.uniform(seed + 4, (O,))).astype(np.float32)
    return {
        "PLAIN": dict(), "PLAIN1": dict(), "BIAS": dict(bias=bias), "SCALE": dict(post_scale=scale),
        "MID": dict(bn_scale=a, bn_shift=b, relu=True, out_f32=False, out_packed=True),
        "MIDT": dict(bn_scale=a, bn_shift=b, relu=True, out_f32=False, out_packed=True),
        "OUT": dict(bn_scale=a, bn_shift=b, residual=res, relu=True, out_f32=True, out_packed=True),
        "OUTP": dict(bn_scale=a, bn_shift=b, residual=res, relu=True, out_f32=False, out_packed=True),
        "LAST": dict(bn_scale=a, bn_shift=b, residual=res, relu=True, out_f32=True, out_packed=False),
        # a mix no compiled profile covers: bias + BatchNorm + residual, no ReLU -> fp32 + both planes
        "RUNTIME": dict(bias=bias, bn_scale=a, bn_shift=b, residual=res, out_f32=True, out_packed=True),
    }[profile]


def same(a, b):
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, hipops.PackedAct):
        return torch.equal(a.P, b.P) and torch.equal(a.M, b.M) and a.nonneg == b.nonneg
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def run_both(shape_id, profile, nn, wz=False):
    N, C, H, W, O, stride = SHAPES[shape_id]
    x, w = operands(shape_id, nn, wz)
    act = packed_input(x, nn)
    pw = hipops.pack_weight(dev(w))
    assert pw.has_zero == wz
    if profile == "PLAIN1":
        pw.alpha[:] = 1.0
    w8 = hipops.pack_weight_i8(pw)
    assert w8 is not None and w8.numel() == 9 * O * C
    ho, wo = hipops.conv_out_hw(H, W, 3, 3, stride, 1, 1)
    kw = {k: dev(v) if isinstance(v, np.ndarray) else v
          for k, v in epilogue(profile, O, (N, O, ho, wo), gen.seed_of("mfma-epi", shape_id, profile)).items()}
    if profile == "MIDT":
        kw["sign_thresholds"] = hipops.sign_thresholds(pw, kw["bn_scale"], kw["bn_shift"])
    geo = dict(stride=stride, padding=1, dilation=1)
    want = hipops.bconv2d_fused(act, pw, **kw, **geo)
    before = native.launch_count()
    got = hipops.bconv2d_mfma_fused(act, pw, w8, **kw, **geo)
    assert native.launch_count() == before + 1
    return got, want, (x, w, stride)


CASES = [(s, p, nn) for s in SHAPES for p, nn in (("PLAIN1", False), ("MID", True), ("OUT", True))]
# every profile, both input kinds, on the first shape; the remaining profiles once on a 128 x 128-tile shape
CASES += [("c64-o64-3x9x7", p, nn) for p in PROFILES for nn in (False, True)
          if ("c64-o64-3x9x7", p, nn) not in CASES]
CASES += [("c128-o128-3x9x7", p, True) for p in ("MIDT", "OUTP", "LAST", "RUNTIME", "BIAS")]


@pytest.mark.parametrize("shape_id,profile,nn", CASES, ids=lambda v: str(v))
def test_mfma_conv_equals_the_popcount_conv(shape_id, profile, nn):
    (y, pk), (y_ref, pk_ref), (x, w, stride) = run_both(shape_id, profile, nn)
    assert same(y, y_ref)
    assert same(pk, pk_ref)
    if profile == "PLAIN1":      # alpha = 1, no bias: the fp32 output IS the integer dot — against the oracle's
        _, dot = oracle.binary_conv2d_int(x, w, None, None, stride, 1, 1)
        assert np.array_equal(y.cpu().numpy(), dot.astype(np.float32))


@pytest.mark.parametrize("profile,nn", [("PLAIN1", False), ("OUT", True), ("MID", False)])
def test_zero_weights_are_honoured(profile, nn):
    (y, pk), (y_ref, pk_ref), (x, w, stride) = run_both("c64-o64-3x9x7", profile, nn, wz=True)
    assert same(y, y_ref) and same(pk, pk_ref)
    if profile == "PLAIN1":
        _, dot = oracle.binary_conv2d_int(x, w, None, None, stride, 1, 1)
        assert np.array_equal(y.cpu().numpy(), dot.astype(np.float32))


def test_the_same_launch_twice_gives_the_same_bits():
    first, _, _ = run_both("c128-o192-5x7x7", "OUT", True)
    second, _, _ = run_both("c128-o192-5x7x7", "OUT", True)
    assert same(first[0], second[0]) and same(first[1], second[1])


@pytest.mark.parametrize("what", ["k5", "dilation", "pad0", "c96", "o96", "prelu", "channel-window", "late-residual"])
def test_unsupported_shapes_launch_nothing(what):
    N, C, H, W, O, k, pad, dil = 2, 64, 9, 7, 64, 3, 1, 1
    kw = {}
    if what == "k5":
        k, pad = 5, 2
    elif what == "dilation":
        dil, pad = 2, 2
    elif what == "pad0":
        pad = 0
    elif what == "c96":
        C = 96
    elif what == "o96":
        O = 96
    x = gen.activation("normal", 5, (N, C, H, W))
    w = gen.conv_weight("kaiming", 6, (O, C, k, k))
    act, pw = packed_input(x, False), hipops.pack_weight(dev(w))
    ho, wo = hipops.conv_out_hw(H, W, k, k, 1, pad, dil)
    if what == "prelu":
        kw = dict(prelu=dev(np.full((O,), 0.25, np.float32)))
    elif what == "channel-window":
        kw = dict(out=torch.zeros((N, O + 8, ho, wo), device="cuda:0"), out_c_offset=3)
    elif what == "late-residual":
        kw = dict(residual=dev(gen.normal(7, (N, O, ho, wo))), residual_after_act=True)
    # any aligned buffer stands in for the pack: an unsupported call must not get as far as reading it
    w8 = hipops.pack_weight_i8(pw)
    if w8 is None:
        assert what in ("k5", "c96", "o96")
        w8 = torch.zeros(1024, dtype=torch.int8, device="cuda:0")
    torch.cuda.synchronize()
    before = native.launch_count()
    with pytest.raises(native.NativeError, match=r"status -2"):
        hipops.bconv2d_mfma_fused(act, pw, w8, stride=1, padding=pad, dilation=dil, **kw)
    assert native.launch_count() == before

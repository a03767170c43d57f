"""The last convolution of a down-sampling block with its shortcut folded in, both dots on the int8 matrix cores
(``bnn_hip_bconv2d_mfma_fold_fused``, csrc/bconv_mfma.hip, the DS form), against

* the popcount fold on the same operands (``hipops.bconv2d_fused(..., shortcut=...)``),
* reference A — the unfolded composition: the 1x1 convolution writes fp32, the 3x3 convolution reads it as ``residual``,
* reference B — the CPU oracle's route,

the last two as tests/test_gpu_ds_fold_stream.py builds them (its inputs: a window that is zero in every channel, clipped
windows at odd edges, per-channel word patterns and alphas in the shortcut weight, negative BatchNorm slopes).  fp32
output (compared as int32) and both sign planes are BIT-equal to all three.

Shapes, the smallest that reach each way the kernel can go: 64 / 128 / 256 shortcut channels (1 / 2 / 4 shortcut k-steps);
the 128 x 128 tile (C = O = 128, 256, 512) and the 256 x 64 tile (C = O = 192: O no multiple of 128; C = O = 64); the
block input un-pooled at 8x8 and at 7x7 (clipped windows) and pre-pooled at 4x4; batch 2 (32 pixels), batch 3 (48 pixels:
a ragged tile spanning images), batch 9 / 17 (144 / 272 pixels: two tiles of 128 / 256, the second ragged);
BNN_HIP_FLAG_THROUGHPUT on and off."""
import pytest
import torch

from bnn_amd import hipops, native
from tests.test_gpu_ds_fold_stream import _case, u64

import numpy as np

pytestmark = pytest.mark.gpu


def _tile(C, O):
    """choose_tile of csrc/bconv_mfma.hip at these image sizes: pixels per workgroup."""
    return 128 if (O % 128 == 0 and C >= 128) else 256


def _check(N, Cs, O, h, w, throughput, form):
    c = _case(N, Cs, O, h, w)
    act2, pw2, pws = c["act2"], c["pw2"], c["pws"]
    w8, sc_w8 = hipops.pack_weight_i8(pw2), hipops.pack_shortcut_weight_i8(pws)
    assert w8 is not None and sc_w8 is not None and sc_w8.numel() == O * Cs
    sa = c[form]
    unpooled = None if form == "pooled" else tuple(sa.shape[2:])
    assert hipops.bconv2d_mfma_fold_supported(act2.shape, pw2, Cs, nonneg=True, unpooled_hw=unpooled, throughput=throughput)
    kw = dict(shortcut=(sa, pws, *c["bns"]), bn_scale=c["bn2"][0], bn_shift=c["bn2"][1], relu=True, stride=1, padding=1,
              out_f32=True, out_packed=True, throughput=throughput)
    n0 = native.launch_count()
    y, p = hipops.bconv2d_mfma_fold_fused(act2, pw2, w8, sc_w8, **kw)
    assert native.launch_count() - n0 == 1
    yp, pp = hipops.bconv2d_fused(act2, pw2, **kw)                                     # the popcount fold
    assert torch.equal(y.view(torch.int32), yp.view(torch.int32)) and torch.equal(p.P, pp.P) and torch.equal(p.M, pp.M)
    assert p.nonneg and not bool(p.M.any())
    ya, pa = c["y_a"][throughput], c["p_a"][throughput]                                # reference A
    assert torch.equal(y.view(torch.int32), ya.view(torch.int32)) and torch.equal(p.P, pa.P) and torch.equal(p.M, pa.M)
    i = c["imgs"]                                                                      # reference B
    assert np.array_equal(y.cpu().numpy().view(np.uint32)[i], c["y_b"].view(np.uint32))
    assert np.array_equal(u64(p.P)[i], c["P_b"]) and np.array_equal(u64(p.M)[i], c["M_b"])


# (shortcut channels, C = O of conv2, pixels per workgroup)
WIDTHS = [(64, 128, 128), (128, 256, 128), (256, 512, 128), (128, 192, 256), (64, 64, 256)]


@pytest.mark.parametrize("form", ["pooled", "big"], ids=["prepooled", "unpooled"])
@pytest.mark.parametrize("throughput", [False, True], ids=["latency", "throughput"])
@pytest.mark.parametrize("hw", [(8, 8), (7, 7)], ids=["8x8", "7x7"])
@pytest.mark.parametrize("N", [2, 3])
@pytest.mark.parametrize("width", WIDTHS, ids=lambda v: f"{v[0]}to{v[1]}")
def test_mfma_fold_is_bit_equal(width, N, hw, throughput, form):
    Cs, O, tile = width
    assert _tile(O, O) == tile
    _check(N, Cs, O, *hw, throughput, form)


@pytest.mark.parametrize("form", ["pooled", "big"], ids=["prepooled", "unpooled"])
@pytest.mark.parametrize("shape", [(9, 64, 128, 8, 8), (9, 256, 512, 7, 7), (17, 128, 192, 7, 7)],
                         ids=["9x64to128", "9x256to512", "17x128to192"])
def test_two_tiles_the_second_ragged(shape, form):
    N, Cs, O, h, w = shape
    pix, tile = N * 16, _tile(O, O)
    assert tile < pix < 2 * tile and pix % tile != 0
    _check(N, Cs, O, h, w, False, form)


def test_refusals_launch_nothing():
    """What the admission excludes is refused before anything is launched."""
    c = _case(2, 64, 128, 8, 8)
    act2, pw2, pws = c["act2"], c["pw2"], c["pws"]
    w8, sc_w8 = hipops.pack_weight_i8(pw2), hipops.pack_shortcut_weight_i8(pws)
    kw = dict(bn_scale=c["bn2"][0], bn_shift=c["bn2"][1], relu=True, stride=1, padding=1, out_f32=True, out_packed=True)
    n0 = native.launch_count()
    with pytest.raises(native.NativeError):                     # no shortcut at all
        hipops.bconv2d_mfma_fold_fused(act2, pw2, w8, sc_w8, **kw)
    with pytest.raises(native.NativeError):                     # planes only: not the fold's epilogue
        hipops.bconv2d_mfma_fold_fused(act2, pw2, w8, sc_w8, shortcut=(c["pooled"], pws, *c["bns"]),
                                       **{**kw, "out_f32": False})
    with pytest.raises(native.NativeError):                     # the plain entry point keeps refusing the fold
        hipops.bconv2d_mfma_fused(act2, pw2, w8, shortcut=(c["pooled"], pws, *c["bns"]), **kw)
    assert native.launch_count() == n0
    assert not hipops.bconv2d_mfma_fold_supported(act2.shape, pw2, 64, nonneg=False)
    assert not hipops.bconv2d_mfma_fold_supported(act2.shape, pw2, 96)

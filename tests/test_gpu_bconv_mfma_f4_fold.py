"""The last convolution of a down-sampling block with its shortcut folded in, the 3x3 dot on the FP4 matrix-core
instruction (``bnn_hip_bconv2d_mfma4_fold_fused``, csrc/bconv_mfma.hip, the DS + F4 form; the shortcut's 1x1 prologue stays
on the int8 instruction), against

* the popcount fold on the same operands (``hipops.bconv2d_fused(..., shortcut=...)``),
* reference A — the unfolded composition: the 1x1 convolution writes fp32, the 3x3 convolution reads it as ``residual``,
* reference B — the CPU oracle's route,

as tests/test_gpu_bconv_mfma_fold.py does for the int8 form, on the cases of tests/test_gpu_ds_fold_stream.py.  fp32
output (compared as int32) and both sign planes are BIT-equal to all three.

Shapes: 64 / 128 / 256 shortcut channels in front of 1 / 2 / 4 FP4 k-steps per tap (C = O = 128, 256, 512: the
128 x 128 tile); the block input un-pooled at 8x8 and at 7x7 (clipped windows) and pre-pooled at 4x4; batch 2 (32
pixels), batch 3 (48 pixels: a ragged tile spanning images), batch 9 (144 pixels: two tiles, the second ragged);
BNN_HIP_FLAG_THROUGHPUT on and off."""
import numpy as np
import pytest
import torch

from bnn_amd import hipops, native
from tests.test_gpu_ds_fold_stream import _case, u64

pytestmark = pytest.mark.gpu


def _check(N, Cs, O, h, w, throughput, form):
    c = _case(N, Cs, O, h, w)
    act2, pw2, pws = c["act2"], c["pw2"], c["pws"]
    w4, sc_w8 = hipops.pack_weight_f4(pw2), hipops.pack_shortcut_weight_i8(pws)
    assert w4 is not None and w4.numel() == 9 * O * O // 2 and sc_w8 is not None and sc_w8.numel() == O * Cs
    sa = c[form]
    unpooled = None if form == "pooled" else tuple(sa.shape[2:])
    assert hipops.bconv2d_mfma4_fold_supported(act2.shape, pw2, Cs, nonneg=True, unpooled_hw=unpooled,
                                               throughput=throughput)
    kw = dict(shortcut=(sa, pws, *c["bns"]), bn_scale=c["bn2"][0], bn_shift=c["bn2"][1], relu=True, stride=1, padding=1,
              out_f32=True, out_packed=True, throughput=throughput)
    n0 = native.launch_count()
    y, p = hipops.bconv2d_mfma4_fold_fused(act2, pw2, w4, sc_w8, **kw)
    assert native.launch_count() - n0 == 1
    yp, pp = hipops.bconv2d_fused(act2, pw2, **kw)                                     # the popcount fold
    assert torch.equal(y.view(torch.int32), yp.view(torch.int32)) and torch.equal(p.P, pp.P) and torch.equal(p.M, pp.M)
    assert p.nonneg and not bool(p.M.any())
    ya, pa = c["y_a"][throughput], c["p_a"][throughput]                                # reference A
    assert torch.equal(y.view(torch.int32), ya.view(torch.int32)) and torch.equal(p.P, pa.P) and torch.equal(p.M, pa.M)
    i = c["imgs"]                                                                      # reference B
    assert np.array_equal(y.cpu().numpy().view(np.uint32)[i], c["y_b"].view(np.uint32))
    assert np.array_equal(u64(p.P)[i], c["P_b"]) and np.array_equal(u64(p.M)[i], c["M_b"])


# (shortcut channels, C = O of conv2)
WIDTHS = [(64, 128), (128, 256), (256, 512)]


@pytest.mark.parametrize("form", ["pooled", "big"], ids=["prepooled", "unpooled"])
@pytest.mark.parametrize("throughput", [False, True], ids=["latency", "throughput"])
@pytest.mark.parametrize("hw", [(8, 8), (7, 7)], ids=["8x8", "7x7"])
@pytest.mark.parametrize("N", [2, 3])
@pytest.mark.parametrize("width", WIDTHS, ids=lambda v: f"{v[0]}to{v[1]}")
def test_fp4_fold_is_bit_equal(width, N, hw, throughput, form):
    Cs, O = width
    _check(N, Cs, O, *hw, throughput, form)


@pytest.mark.parametrize("form", ["pooled", "big"], ids=["prepooled", "unpooled"])
@pytest.mark.parametrize("shape", [(9, 64, 128, 8, 8), (9, 256, 512, 7, 7)], ids=["9x64to128", "9x256to512"])
def test_two_tiles_the_second_ragged(shape, form):
    N, Cs, O, h, w = shape
    pix, tile = N * 16, 128                 # choose_tile: O % 128 == 0 and C >= 128
    assert tile < pix < 2 * tile and pix % tile != 0
    _check(N, Cs, O, h, w, False, form)


def test_refusals_launch_nothing():
    """What the admission excludes is refused before anything is launched."""
    c = _case(2, 64, 128, 8, 8)
    act2, pw2, pws = c["act2"], c["pw2"], c["pws"]
    w4, sc_w8 = hipops.pack_weight_f4(pw2), hipops.pack_shortcut_weight_i8(pws)
    kw = dict(bn_scale=c["bn2"][0], bn_shift=c["bn2"][1], relu=True, stride=1, padding=1, out_f32=True, out_packed=True)
    n0 = native.launch_count()
    with pytest.raises(native.NativeError):                     # no shortcut at all
        hipops.bconv2d_mfma4_fold_fused(act2, pw2, w4, sc_w8, **kw)
    with pytest.raises(native.NativeError):                     # planes only: not the fold's epilogue
        hipops.bconv2d_mfma4_fold_fused(act2, pw2, w4, sc_w8, shortcut=(c["pooled"], pws, *c["bns"]),
                                        **{**kw, "out_f32": False})
    with pytest.raises(native.NativeError):                     # the dense entry point refuses the fold
        hipops.bconv2d_mfma4_fused(act2, pw2, w4, shortcut=(c["pooled"], pws, *c["bns"]), **kw)
    assert native.launch_count() == n0
    assert not hipops.bconv2d_mfma4_fold_supported(act2.shape, pw2, 64, nonneg=False)
    assert not hipops.bconv2d_mfma4_fold_supported(act2.shape, pw2, 96)
    # no whole 128-channel group: the int8 form takes these, the FP4 form launches nothing
    for Cs, O in ((128, 192), (64, 64)):
        c = _case(2, Cs, O, 8, 8)
        act2, pw2, pws = c["act2"], c["pw2"], c["pws"]
        assert hipops.pack_weight_f4(pw2) is None
        assert hipops.bconv2d_mfma_fold_supported(act2.shape, pw2, Cs, nonneg=True)
        assert not hipops.bconv2d_mfma4_fold_supported(act2.shape, pw2, Cs, nonneg=True)
        stand_in = torch.zeros(9 * O * O // 2, dtype=torch.int8, device=act2.P.device)
        sc_w8 = hipops.pack_shortcut_weight_i8(pws)
        torch.cuda.synchronize()
        n0 = native.launch_count()
        with pytest.raises(native.NativeError):
            hipops.bconv2d_mfma4_fold_fused(act2, pw2, stand_in, sc_w8, shortcut=(c["pooled"], pws, *c["bns"]),
                                            bn_scale=c["bn2"][0], bn_shift=c["bn2"][1], relu=True, stride=1, padding=1,
                                            out_f32=True, out_packed=True)
        assert native.launch_count() == n0

"""The folded shortcut convolution with streamed 1x1 weights (csrc/bconv_core.h: shortcut_values_full): the last conv
of a down-sampling block, driven through ``bnn_hip_bconv2d_fused`` with the ``sc_*`` fields, against

* reference A — the unfolded composition of existing entry points: the 1x1 convolution with its own epilogue writes an
  fp32 tensor, the 3x3 convolution reads it as ``residual``;
* reference B — the CPU oracle's route (pack -> integer dot -> fused epilogue, twice).

fp32 output and sign planes are BIT-equal to both.  Shapes are the smallest that reach every path: 64 / 128 / 256
shortcut channels (2 / 4 / 8 words per pixel; a single-chunk conv2, two chunks, four chunks), batch 2 and batch 3
(3 x 16 = 48 pixels: a ragged 64-pixel tile), a block input of 8x8 and of 7x7 (odd: clipped 2x2 windows in the
un-pooled form), the shortcut plane pre-pooled and un-pooled, both multi-chunk kernel families, ragged last blocks."""
import functools

import numpy as np
import pytest
import torch

import oracle
from bnn_amd import hipops
from tests.golden import gen

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def kernel_family(N, O, c_mid, Ho, Wo, throughput):
    """The selection rule of csrc/bconv.hip (launch_sgpr_t) for a 3x3 conv2 with the fold: which instantiation family of
    bconv_sgpr_kernel<.., DS = true> a launch takes."""
    cw32 = 2 * ((c_mid + 63) // 64)
    cwc = 4 if cw32 % 4 == 0 else 2
    if cw32 // cwc == 1:
        return "single"
    if cwc != 4:
        return "unsplit"                       # (only the 4-word chunk has the split form)
    tiles = (N * Ho * Wo + 63) // 64
    waves = 8 * ((tiles + 7) // 8) * 2 * ((O + 63) // 64)     # XCD-padded pixel tiles x 32-channel blocks (pack mode)
    split = ((not throughput) or waves < 2048) and waves <= 16384
    return "split" if split else "unsplit"


def _bn(seed, O):
    """A folded BatchNorm with every fifth slope negative."""
    a = (0.5 + gen.uniform(seed, (O,))).astype(np.float32) * np.where(np.arange(O) % 5 == 0, -1, 1).astype(np.float32)
    return a, (0.3 * gen.normal(seed + 1, (O,))).astype(np.float32)


def _shortcut_weight(Cs, O):
    """Kaiming weights; every third channel replaced by a prefix pattern (+ on the first (7 o mod Cs) + 1 inputs, - on
    the rest, its own magnitude): no two such channels share a word pattern or an alpha, so a weight word or a constant
    taken from a neighbouring channel — across the seam of two scalar pieces of the stream, or of two 32-channel blocks —
    changes the result.  Channel 0 is all +1 but one input, channel 3's pattern ends inside word 0."""
    w = gen.conv_weight("kaiming", 22, (O, Cs, 1, 1))
    for o in range(0, O, 3):
        k = (7 * o) % Cs + 1
        w[o, :k, 0, 0] = 1.0 + o / O
        w[o, k:, 0, 0] = -(1.0 + o / O)
    return w


def _block_input(N, Cs, h, w, seed):
    """The block's input (ReLU output) at twice the output resolution, with the edge cases of the shortcut field:
    image 0, output pixel (0, 0): the whole 2x2 window zero in every channel (no non-zero input: nz == 0);
    image 1, output pixel (1, 1): channels 0..31 positive (an all-ones word), and output pixel (0, 1): all Cs channels."""
    x = gen.activation("relu", seed, (N, Cs, h, w))
    x[0, :, 0:2, 0:2] = 0.0
    x[1, :32, 2:4, 2:4] = 1.0
    x[1, :, 0:2, 2:4] = 0.5
    return x


@functools.lru_cache(maxsize=None)
def _case(N, Cs, O, h, w):
    """Inputs and both references of one shape, computed once (shared by the kernel-family and plane-form variants)."""
    ho, wo = (h + 1) // 2, (w + 1) // 2
    seed = gen.seed_of("ds_fold_stream", N, Cs, O, h, w)
    x2 = gen.activation("relu", seed, (N, O, ho, wo))              # conv2 of a BasicBlock: O -> O at the output size
    big = _block_input(N, Cs, h, w, seed + 1)
    w2 = gen.conv_weight("kaiming", 21, (O, O, 3, 3))
    ws = _shortcut_weight(Cs, O)
    (a2, b2), (as_, bs_) = _bn(31, O), _bn(41, O)
    # reference B: the CPU oracle, op for op.  (The 2048-wave batches: on images 0, 1, N / 2 and N - 1 — the oracle takes
    # seconds for a whole one, images are independent of each other, and reference A covers every image.)
    imgs = list(range(N)) if N <= 8 else [0, 1, N // 2, N - 1]
    x2_b = np.ascontiguousarray(x2[imgs])
    pooled = oracle.avgpool_ceil(np.ascontiguousarray(big[imgs]), 2)
    Ps, Ms = oracle.pack_act(pooled)
    assert not Ms.any() and not Ps[0, :, 0, 0].any() and int(Ps[1, 0, 1, 1]) & 0xFFFFFFFF == 0xFFFFFFFF
    sb, sz, salpha, _ = oracle.pack_weight(ws)
    res = oracle.fused_epilogue(oracle.bconv_dot(Ps, Ms, sb, sz, pooled.shape, ws.shape), salpha[:O], bn_a=as_, bn_b=bs_)
    P2, M2 = oracle.pack_act(x2_b)
    wb, wz, alpha2, _ = oracle.pack_weight(w2)
    dot = oracle.bconv_dot(P2, M2, wb, wz, x2_b.shape, w2.shape, stride=1, padding=1)
    y_b = oracle.fused_epilogue(dot, alpha2[:O], bn_a=a2, bn_b=b2, res=res, relu=True)
    P_b, M_b = oracle.pack_act(y_b)
    # device operands + reference A: the 1x1 convolution as a launch of its own, its fp32 output read as the residual
    act2 = hipops.pack_act(dev(x2)); act2.nonneg = True
    bigp = hipops.pack_act(dev(big)); bigp.nonneg = True
    poolp = hipops.orpool_packed(bigp, 2)
    assert np.array_equal(u64(poolp.P)[imgs], Ps)
    pw2, pws = hipops.pack_weight(dev(w2)), hipops.pack_weight(dev(ws))
    bn2, bns = (dev(a2), dev(b2)), (dev(as_), dev(bs_))
    idn, _ = hipops.bconv2d_fused(poolp, pws, bn_scale=bns[0], bn_shift=bns[1], out_f32=True, out_packed=False)
    y_a, p_a = {}, {}
    for thr in (False, True):
        y_a[thr], p_a[thr] = hipops.bconv2d_fused(act2, pw2, residual=idn, bn_scale=bn2[0], bn_shift=bn2[1], relu=True,
                                                  stride=1, padding=1, out_f32=True, out_packed=True, throughput=thr)
    return dict(act2=act2, big=bigp, pooled=poolp, pw2=pw2, pws=pws, bn2=bn2, bns=bns, y_a=y_a, p_a=p_a,
                y_b=y_b, P_b=P_b, M_b=M_b, imgs=imgs)


def _check(N, Cs, O, h, w, throughput, form):
    c = _case(N, Cs, O, h, w)
    assert hipops.shortcut_fold_supported(c["act2"], c["pw2"], Cs, 1, 1, 1, throughput=throughput)
    y, p = hipops.bconv2d_fused(c["act2"], c["pw2"], shortcut=(c[form], c["pws"], *c["bns"]), bn_scale=c["bn2"][0],
                                bn_shift=c["bn2"][1], relu=True, stride=1, padding=1, out_f32=True, out_packed=True,
                                throughput=throughput)
    ya, pa = c["y_a"][throughput], c["p_a"][throughput]
    assert torch.equal(y, ya) and torch.equal(p.P, pa.P) and torch.equal(p.M, pa.M)              # reference A
    i = c["imgs"]
    assert np.array_equal(y.cpu().numpy().view(np.uint32)[i], c["y_b"].view(np.uint32))           # reference B
    assert np.array_equal(u64(p.P)[i], c["P_b"]) and np.array_equal(u64(p.M)[i], c["M_b"]) and not c["M_b"].any()


WIDTHS = [(64, 128, "single"), (128, 256, "split"), (256, 512, "split")]


@pytest.mark.parametrize("form", ["pooled", "big"], ids=["prepooled", "unpooled"])
@pytest.mark.parametrize("throughput", [False, True], ids=["latency", "throughput"])
@pytest.mark.parametrize("hw", [(8, 8), (7, 7)], ids=["8x8", "7x7"])
@pytest.mark.parametrize("N", [2, 3])
@pytest.mark.parametrize("width", WIDTHS, ids=lambda v: f"{v[0]}to{v[1]}")
def test_streamed_fold_is_bit_equal_to_both_references(width, N, hw, throughput, form):
    """Full blocks on every width, batch 2 and the ragged tile of batch 3.  At these sizes a multi-chunk launch has
    fewer than 2048 waves and keeps the two-piece split with BNN_HIP_FLAG_THROUGHPUT too (kernel_family)."""
    Cs, O, family = width
    assert kernel_family(N, O, O, 4, 4, throughput) == family
    _check(N, Cs, O, *hw, throughput, form)


@pytest.mark.parametrize("form", ["pooled", "big"], ids=["prepooled", "unpooled"])
@pytest.mark.parametrize("shape", [(1024, 128, 256), (512, 256, 512)], ids=["128to256", "256to512"])
def test_streamed_fold_in_the_unsplit_throughput_kernel(shape, form):
    """BNN_HIP_FLAG_THROUGHPUT on a launch of 2048 waves: the multi-chunk kernel that keeps all 32 channels of a block in
    one wave (32 shortcut values in one run); without the flag the same shape takes the split kernel."""
    N, Cs, O = shape
    assert kernel_family(N, O, O, 4, 4, True) == "unsplit" and kernel_family(N, O, O, 4, 4, False) == "split"
    _check(N, Cs, O, 8, 8, True, form)
    _check(N, Cs, O, 8, 8, False, form)


@pytest.mark.parametrize("form", ["pooled", "big"], ids=["prepooled", "unpooled"])
@pytest.mark.parametrize("throughput", [False, True], ids=["latency", "throughput"])
@pytest.mark.parametrize("shape", [(64, 80, "single"), (128, 272, "unsplit")], ids=["64to80", "128to272"])
def test_ragged_last_block_keeps_the_guarded_form(shape, throughput, form):
    """The fold admits any output-channel count: 80 = two full blocks + 16 channels (single-chunk conv2), 272 = eight
    full blocks + 16 (five 2-word chunks).  The full blocks stream, the last one takes the guarded code."""
    Cs, O, family = shape
    assert kernel_family(3, O, O, 4, 4, throughput) == family
    _check(3, Cs, O, 7, 7, throughput, form)

"""Every fp32-to-planes producer of csrc/pack_act.hip and csrc/pack_ste.hip against the CPU oracle, bit for bit: the planes
against oracle.pack_act of the value the oracle computes in float32 with a true fmaf (oracle.bn_act, avgpool2, avgpool_ceil,
bn_maxpool, pack_ste_mask: pinned on the CPU by tests/test_pack_oracle_cpu.py), the fp32 outputs word for word, no element
left out.  Each case states the host-side condition that selects its kernel (vector width from H W and the alignment of the
first element, K <= 2, W % 4, the pixel-word count of avgpool2_bn_pack2) and asserts it, launches more than one workgroup
with a ragged last one where the mapping has one, and carries the planted affine cases and 2x2 windows of the CPU test's
known-answer table."""
import ctypes

import numpy as np
import pytest
import torch

import oracle
from bnn_amd import hipops, native
from bnn_amd.native import NativeError
from tests.golden import gen
from tests.test_pack_oracle_cpu import (AFFINE_CASES, MAXPOOL_GEOMETRIES, WINDOW_CASES, maxpool_input, plane_cls,
                                        same_f32)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -12345.5
# launch_avgpool2_bn_pack2 (csrc/pack_act.hip): N (H/2) (W/2) * 2 ceil(C/64) pixel-words from which the one-thread-per-word
# ("wide") kernel runs instead of the LDS form
WIDE_PIXEL_WORDS = 150000


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def carve(value, off=0):
    """``value`` as a contiguous device tensor whose first element lies ``off`` elements into a 16-byte aligned buffer."""
    v = torch.from_numpy(np.ascontiguousarray(value))
    flat = torch.full((v.numel() + 8,), SENTINEL, dtype=v.dtype, device=DEV)
    assert flat.data_ptr() % 16 == 0
    t = flat[off:off + v.numel()].view(v.shape)
    t.copy_(v)
    assert t.is_contiguous() and t.data_ptr() == flat.data_ptr() + off * v.element_size()
    return t


def assert_planes(pk, value, tag=None):
    """The planes of ``pk`` are the planes of sign(value), every word of them."""
    Pw, Mw = oracle.pack_act(value)
    gp, gm = u64(pk.P), u64(pk.M)
    assert gp.shape == Pw.shape, tag
    assert np.array_equal(gp, Pw), (tag, "P words that differ:", int((gp != Pw).sum()))
    assert np.array_equal(gm, Mw), (tag, "M words that differ:", int((gm != Mw).sum()))


def assert_same_planes(a, b, tag=None):
    assert torch.equal(a.P, b.P) and torch.equal(a.M, b.M), tag


def affines(K, C, seed):
    """K BatchNorm-like affines whose zero crossings fall inside the data, a fifth of the scales negative."""
    a = (0.5 + gen.uniform(seed, (K, C))) * np.where(gen.uniform(seed + 1, (K, C)) < 0.2, -1, 1)
    return a.astype(np.float32), (0.4 * gen.normal(seed + 2, (K, C))).astype(np.float32)


def plant_affine(x, a, b, positions, rot=0, first=0):
    """Planted affine case ``first + j`` goes to channel ``rot + j`` (both cyclic): its (a, b) into the channel's affine and
    its x to ``positions`` [(y, x)] of every image.  Returns [(channel, class, class under ReLU, name)]."""
    C = x.shape[1]
    planted = []
    for j in range(min(C, len(AFFINE_CASES))):
        name, xv, av, bv, cls, cls_relu = AFFINE_CASES[(first + j) % len(AFFINE_CASES)]
        c = (rot + j) % C
        a[c], b[c] = av, bv
        for y, xx in positions:
            x[:, c, y, xx] = xv
        planted.append((c, cls, cls_relu, name))
    return planted


def check_planted(pk, planted, positions, relu, tag=None):
    """The hand-written classes of the planted affine cases, read back from the kernel's planes."""
    Pw, Mw = u64(pk.P), u64(pk.M)
    for c, cls, cls_relu, name in planted:
        for n in range(Pw.shape[0]):
            for y, xx in positions:
                assert plane_cls(Pw, Mw, n, c, y, xx) == (cls_relu if relu else cls), (tag, name, n, c)


def plant_windows(x, k):
    """The planted 2x2 windows at the top-left of pooling windows of ``x`` (the rest of such a window zeroed), spread over
    images and channels; the last window of an image is left alone.  Returns [(n, c, oy, ox, class of the 2x2 average)]."""
    N, C, H, W = x.shape
    step = max(k, 2)
    nY, nX = max(1, H // step), max(1, W // step)
    wins = [(oy, ox) for oy in range(nY) for ox in range(nX)]
    if len(wins) > 1:
        wins = wins[:-1]
    slots = N * C * len(wins)
    cases = WINDOW_CASES[:slots]
    stride = max(1, slots // len(cases))
    planted = []
    for i, (name, vals, cls) in enumerate(cases):
        s = i * stride
        n, c, (oy, ox) = s // (C * len(wins)), (s // len(wins)) % C, wins[s % len(wins)]
        y0, x0 = oy * step, ox * step
        x[n, c, y0:y0 + step, x0:x0 + step] = 0.0
        x[n, c, y0:y0 + 2, x0:x0 + 2] = np.array(vals, np.float32).reshape(2, 2)
        planted.append((n, c, oy, ox, cls))
    return planted


# ---- 1. the streaming mapping: pack_act, bn_act_pack, pack_act_ste ---------------------------------------------------
def stream_vp(t):
    """Pixels per thread launch_pack_act_t / launch_bn_act_pack / launch_pack_ste choose for ``t``."""
    hw, es, p = t.shape[2] * t.shape[3], t.element_size(), t.data_ptr()
    return 4 if hw % 4 == 0 and p % (4 * es) == 0 else 2 if hw % 2 == 0 and p % (2 * es) == 0 else 1


# (shape, element offset of the base, H W % 4, pixels per thread)
STREAM_CASES = [
    ((5, 70, 16, 17), 0, 0, 4),     # 340 threads: two workgroups, the last ragged; group 1 = a 6-channel half + an empty half
    ((7, 33, 10, 9), 0, 2, 2),      # H W = 90: 315 threads
    ((5, 31, 7, 9), 0, 3, 1),       # H W = 63: 315 threads
    ((1, 200, 4, 6), 0, 0, 4),      # four groups, the last with 8 channels
    ((5, 70, 16, 17), 2, 0, 2),     # an 8-byte base (fp16: 4-byte) demotes the first shape
    ((5, 70, 16, 17), 1, 0, 1),     # a 4-byte base (fp16: 2-byte)
]
STREAM_IDS = [f"{'x'.join(map(str, s))}-off{o}-vp{v}" for s, o, _, v in STREAM_CASES]
POS = [(0, 0), (-1, -1)]        # where the planted affine inputs sit in every image


def stream_input(shape, tag):
    x = gen.activation("special", gen.seed_of("pack-family", tag, shape), shape)
    a, b = affines(1, shape[1], gen.seed_of("pack-family-aff", tag, shape))
    planted = plant_affine(x, a[0], b[0], POS, rot=shape[1] - 5)       # wraps round the last channel
    return x, a[0], b[0], planted


@pytest.mark.parametrize("dtype", [np.float32, np.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("shape,off,hw4,vp", STREAM_CASES, ids=STREAM_IDS)
def test_pack_act_streaming(shape, off, hw4, vp, dtype):
    x = stream_input(shape, "pack")[0].astype(dtype)
    t = carve(x, off)
    assert shape[2] * shape[3] % 4 == hw4 and t.data_ptr() % (4 * t.element_size()) == off * t.element_size()
    assert stream_vp(t) == vp
    got = hipops.pack_act(t)
    assert_planes(got, x.astype(np.float32))          # sign of an fp16 value = sign of its exact widening
    assert not got.nonneg
    if off:
        assert_same_planes(got, hipops.pack_act(carve(x, 0)))


@pytest.mark.parametrize("shape,off,hw4,vp", STREAM_CASES, ids=STREAM_IDS)
def test_bn_act_pack_streaming(shape, off, hw4, vp):
    x, a, b, planted = stream_input(shape, "bnpack")
    t = carve(x, off)
    assert shape[2] * shape[3] % 4 == hw4 and t.data_ptr() % 16 == 4 * off
    assert stream_vp(t) == vp
    aligned = carve(x, 0) if off else None
    for bn in (False, True):
        aff = (a, b) if bn else (None, None)
        for relu in (False, True):
            got = hipops.bn_act_pack(t, dev(aff[0]), dev(aff[1]), relu)
            assert_planes(got, oracle.bn_act(x, *aff, relu), (bn, relu))
            assert got.nonneg == relu
            if bn:
                check_planted(got, planted, POS, relu, (bn, relu))
            if off:
                assert_same_planes(got, hipops.bn_act_pack(aligned, dev(aff[0]), dev(aff[1]), relu), (bn, relu))


@pytest.mark.parametrize("shape,off,hw4,vp", STREAM_CASES, ids=STREAM_IDS)
def test_pack_act_ste_streaming(shape, off, hw4, vp):
    x = stream_input(shape, "ste")[0]
    flat = x.reshape(-1)
    flat[3::37], flat[5::41] = 1.0, -1.0                                   # |x| == 1: T = 0
    flat[7::43] = np.nextafter(np.float32(1), np.float32(0))               # the largest value with T = 1
    flat[11::47] = -np.nextafter(np.float32(1), np.float32(0))
    t = carve(x, off)
    assert shape[2] * shape[3] % 4 == hw4 and t.data_ptr() % 16 == 4 * off
    assert stream_vp(t) == vp
    sv = hipops.pack_act_ste(t)
    assert_planes(sv.sign, x)
    T = oracle.pack_ste_mask(x)
    assert np.array_equal(u64(sv.T), T), int((u64(sv.T) != T).sum())
    with np.errstate(invalid="ignore"):
        assert T.any() and np.isnan(x).any() and (np.abs(x) == 1).any()
    if off:
        al = hipops.pack_act_ste(carve(x, 0))
        assert_same_planes(sv.sign, al.sign)
        assert torch.equal(sv.T, al.T)


# ---- 2. K plane sets from one read of a channel-slice view -----------------------------------------------------------
def multi_vp(K, hw, ptr):
    """launch_multi_k: four pixels per thread only up to K = 2."""
    return 4 if K <= 2 and hw % 4 == 0 and ptr % 16 == 0 else 2 if hw % 2 == 0 and ptr % 8 == 0 else 1


def pack_multi(whole, c_off, C, a, b, relu):
    """bn_act_pack_multi on channels [c_off, c_off + C) of ``whole``.  A base that does not start its storage goes through
    the C ABI itself: hipops.channel_view takes a slice apart by its storage offset and has no such base to find."""
    if whole.storage_offset() == 0:
        return hipops.bn_act_pack_multi(whole[:, c_off:c_off + C], a, b, relu=relu)
    N, c_total, H, W = whole.shape
    K = a.shape[0]
    sets = torch.empty((2, K, N, (C + 63) // 64, H, W), dtype=torch.int64, device=DEV)
    view = native.F32View(whole.data_ptr(), c_off, c_total)
    native.check(native.require().bnn_hip_bn_act_pack_multi_f32(
        ctypes.byref(view), N, C, H, W, K, a.data_ptr(), b.data_ptr(), int(relu), sets[0].data_ptr(), sets[1].data_ptr(),
        torch.cuda.current_stream().cuda_stream), "bnn_hip_bn_act_pack_multi_f32")
    return [hipops.PackedAct(sets[0, k], sets[1, k], (N, C, H, W), relu) for k in range(K)]


# (shape, c_off, c_total, element offset of the base, view start % 16)
MULTI_CASES = [
    ((5, 70, 16, 17), 3, 80, 0, 0),     # K <= 2: four pixels; K >= 3: the forced two-pixel branch
    ((5, 70, 16, 17), 3, 80, 2, 8),     # two pixels by alignment
    ((5, 70, 16, 17), 3, 80, 1, 4),     # one pixel by alignment
    ((7, 33, 10, 9), 2, 40, 0, 0),      # H W = 90: c_off 2 starts on 16 bytes, two pixels
    ((7, 33, 10, 9), 1, 40, 0, 8),      # c_off 1 on 8 bytes
    ((5, 31, 7, 9), 1, 36, 0, 12),      # H W = 63: c_off 1 on 4 bytes only, one pixel
]


@pytest.mark.parametrize("K", [1, 2, 3, 4])
@pytest.mark.parametrize("shape,c_off,c_total,off,align", MULTI_CASES,
                         ids=[f"{'x'.join(map(str, c[0]))}-c{c[1]}-off{c[3]}" for c in MULTI_CASES])
def test_bn_act_pack_multi_against_oracle(shape, c_off, c_total, off, align, K):
    N, C, H, W = shape
    x = gen.activation("special", gen.seed_of("pack-family-multi", shape), shape)
    a, b = affines(K, C, gen.seed_of("pack-family-multi-aff", shape, K))
    pos = [[(0, k), (H - 1, W - 1 - k)] for k in range(K)]              # set k reads its planted inputs at its own pixels
    planted = [plant_affine(x, a[k], b[k], pos[k], rot=7 * k + 3) for k in range(K)]     # and in its own channels
    whole = carve(np.full((N, c_total, H, W), SENTINEL, np.float32), off)
    view = whole[:, c_off:c_off + C]
    view.copy_(dev(x))
    assert not view.is_contiguous() and view.data_ptr() % 16 == align
    vp = multi_vp(K, H * W, view.data_ptr())
    assert vp == {0: 4 if K <= 2 and H * W % 4 == 0 else 2, 8: 2, 4: 1, 12: 1}[align]
    for relu in (False, True):
        got = pack_multi(whole, c_off, C, dev(a), dev(b), relu)
        assert len(got) == K
        for k in range(K):
            assert_planes(got[k], oracle.bn_act(x, a[k], b[k], relu), (K, k, relu, vp))
            check_planted(got[k], planted[k], pos[k], relu, (K, k, relu))
            assert got[k].nonneg == relu
    assert float(whole[:, :c_off].min()) == SENTINEL == float(whole[:, c_off + C:].max())    # the read left x alone


# ---- 3. the two phases FactorizedReduce reads ------------------------------------------------------------------------
@pytest.mark.parametrize("as_view", [False, True], ids=["contiguous", "slice"])
@pytest.mark.parametrize("shape", [(5, 70, 12, 18), (2, 33, 2, 2), (3, 40, 6, 2)], ids=lambda s: "x".join(map(str, s)))
def test_bn_act_pack_s2_against_oracle(shape, as_view):
    N, C, H, W = shape                  # 5x70x12x18: 270 threads, two workgroups
    x = gen.activation("special", gen.seed_of("pack-family-s2", shape), shape)
    a, b = affines(1, C, gen.seed_of("pack-family-s2-aff", shape))
    planted = plant_affine(x, a[0], b[0], [(0, 0), (1, 1)], rot=C - 5)  # pixel (0, 0) of phase 0 and of phase 1
    if as_view:
        whole = torch.full((N, C + 11, H, W), SENTINEL, dtype=torch.float32, device=DEV)
        t = whole[:, 5:5 + C]
        t.copy_(dev(x))
        assert not t.is_contiguous()
    else:
        t = dev(x)
    phases = (x[:, :, ::2, ::2], x[:, :, 1::2, 1::2])
    for bn in (False, True):
        aff = (a[0], b[0]) if bn else (None, None)
        for relu in (False, True):
            got = hipops.bn_act_pack_s2(t, dev(aff[0]), dev(aff[1]), relu=relu)
            for ph in range(2):
                assert got[ph].shape == (N, C, H // 2, W // 2)
                assert_planes(got[ph], oracle.bn_act(phases[ph], *aff, relu), (bn, relu, ph))
                if bn:
                    check_planted(got[ph], planted, [(0, 0)], relu, (relu, ph))


# ---- 4. average pool + sign ------------------------------------------------------------------------------------------
def avgpool_kernel(t, k):
    """launch_avgpool_pack's choice."""
    H, W, p = t.shape[2], t.shape[3], t.data_ptr()
    if k == 2 and H % 2 == 0 and W % 4 == 0 and p % 16 == 0:
        return "pair"           # avgpool2_pack_kernel: one float4 per row, two outputs
    if k == 2 and H % 2 == 0 and W % 2 == 0 and p % 8 == 0:
        return "float2"         # avgpool2_pack_f2_kernel
    return "generic"            # avgpool_pack_kernel


AVGPOOL_CASES = [
    ((11, 70, 12, 20), 2, 0, "pair"),       # 330 pairs: two workgroups, the last ragged
    ((11, 33, 12, 10), 2, 0, "float2"),     # 330 outputs
    ((3, 70, 9, 5), 2, 0, "generic"),       # odd H and W: clipped windows
    ((2, 40, 13, 10), 3, 0, "generic"),
    ((2, 70, 3, 4), 5, 0, "generic"),       # k larger than the image
    ((5, 70, 7, 9), 1, 0, "generic"),       # k = 1: pack_act
    ((11, 70, 12, 20), 2, 2, "float2"),     # the pair shape on an 8-byte base
    ((11, 70, 12, 20), 2, 1, "generic"),    # and on a 4-byte base
]


@pytest.mark.parametrize("shape,k,off,kernel", AVGPOOL_CASES,
                         ids=[f"{'x'.join(map(str, c[0]))}-k{c[1]}-off{c[2]}-{c[3]}" for c in AVGPOOL_CASES])
def test_avgpool_pack_against_oracle(shape, k, off, kernel):
    N, C, H, W = shape
    x = gen.activation("special", gen.seed_of("pack-family-avg", shape, k), shape)
    planted = plant_windows(x, k)
    t = carve(x, off)
    assert avgpool_kernel(t, k) == kernel and t.data_ptr() % 16 == 4 * off
    got = hipops.avgpool_pack(t, k)
    assert_planes(got, oracle.avgpool_ceil(x, k), kernel)
    if k == 2:
        Pw, Mw = u64(got.P), u64(got.M)
        for n, c, oy, ox, cls in planted:
            assert plane_cls(Pw, Mw, n, c, oy, ox) == cls, (n, c, oy, ox, x[n, c, 2 * oy:2 * oy + 2, 2 * ox:2 * ox + 2])
    if k == 1:
        assert_same_planes(got, hipops.pack_act(t))
    if off:
        assert_same_planes(got, hipops.avgpool_pack(carve(x, 0), k))
    if k == 2 and H % 2 == 0 and W % 2 == 0 and not off:
        # the two producers that stand in front of a ResNet stage agree: avgpool2_bn_pack2 under an identity affine
        one, zero = dev(np.ones(C, np.float32)), dev(np.zeros(C, np.float32))
        via_bn = hipops.avgpool2_bn_pack2(t, (one, zero), False)[0]
        assert_same_planes(got, via_bn, "avgpool_pack(k=2) vs avgpool2_bn_pack2(identity)")


@pytest.mark.parametrize("shape,k", [((5, 200, 9, 10), 2),      # 500 words: two workgroups; C = 200
                                     ((2, 70, 6, 6), 1), ((2, 70, 3, 4), 5), ((3, 200, 13, 10), 3)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"k{v}")
def test_orpool_packed_against_oracle(shape, k):
    """Non-negative data with no denormals (the OR cannot see an average that underflows): normal values and exact zeros,
    whole windows of zeros among them."""
    x = gen.activation("relu", gen.seed_of("pack-family-or", shape, k), shape)
    x[gen.uniform(gen.seed_of("pack-family-or-z", shape), shape[:2] + (1, 1))[:, :, 0, 0] < 0.3] = 0.0   # dead channels
    x[:, :, : shape[2] // 2, : shape[3] // 2] *= (gen.uniform(5, shape[:2] + (1, 1)) < 0.5)               # zero corners
    assert x.min() == 0 and (x[x > 0] >= np.float32(2.0 ** -126)).all()
    t = dev(x)
    act = hipops.pack_act(t)
    act.nonneg = True
    got = hipops.orpool_packed(act, k)
    assert_planes(got, oracle.avgpool_ceil(x, k))
    assert got.nonneg and not u64(got.M).any()
    assert_same_planes(got, hipops.avgpool_pack(t, k, nonneg=True))
    if k == 1:
        assert torch.equal(got.P, act.P)


# ---- 5. AvgPool2d(2, 2) + two BatchNorm branches ---------------------------------------------------------------------
def pixel_words(shape):
    N, C, H, W = shape
    return N * (H // 2) * (W // 2) * 2 * ((C + 63) // 64)


def pool2_input(shape, kind="special", first=0):
    """Data with the planted windows, two affine branches, and the planted affine inputs as windows of four equal values
    (their average is the value itself) at the last pooled pixel of every image."""
    N, C, H, W = shape
    x = gen.activation(kind, gen.seed_of("pack-family-pool2", shape), shape)
    plant_windows(x, 2)
    a, b = affines(2, C, gen.seed_of("pack-family-pool2-aff", shape))
    x4 = np.zeros((N, C, 1, 1), np.float32)
    planted = plant_affine(x4, a[0], b[0], [(0, 0)], rot=max(0, C - 5), first=first)
    for c, *_ in planted:
        x[:, c, H - 2:, W - 2:] = x4[:, c]
        a[1, c], b[1, c] = a[0, c], b[0, c]
    return x, a, b, planted


def pool2_reference(x, a, b):
    """(pooled fp32, {(branch, relu): value whose sign is packed})"""
    t = oracle.avgpool2(x)
    return t, {(br, relu): oracle.bn_act(t, a[br], b[br], relu) for br in (0, 1) for relu in (False, True)}


def check_pool2(t_dev, x_shape, a, b, ref, planted, combos, tag):
    t, vals = ref
    last = [(x_shape[2] // 2 - 1, x_shape[3] // 2 - 1)]
    bn = [(dev(a[0]), dev(b[0])), (dev(a[1]), dev(b[1]))]
    for relu1, relu2 in combos:
        for out_f32 in (False, True):
            p1, p2, tp = hipops.avgpool2_bn_pack2(t_dev, bn[0], relu1, bn[1], relu2, out_f32=out_f32)
            assert_planes(p1, vals[0, relu1], (tag, "branch 1", relu1, relu2, out_f32))
            assert_planes(p2, vals[1, relu2], (tag, "branch 2", relu1, relu2, out_f32))
            check_planted(p1, planted, last, relu1, (tag, 1))
            check_planted(p2, planted, last, relu2, (tag, 2))
            assert (p1.nonneg, p2.nonneg) == (relu1, relu2)
            assert (tp is not None) == out_f32
            if out_f32:
                assert same_f32(tp.cpu().numpy(), t), (tag, "pooled fp32")
    for relu1 in (False, True):                      # one branch only
        q1, q2, tq = hipops.avgpool2_bn_pack2(t_dev, bn[1], relu1)
        assert q2 is None and tq is None
        assert_planes(q1, vals[1, relu1], (tag, "single branch", relu1))


ALL_RELU = [(False, False), (False, True), (True, False), (True, True)]


@pytest.mark.parametrize("shape,first", [((3, 70, 10, 14), 0),      # 105 pixels: two 64-pixel workgroups, the last ragged;
                                         ((2, 3, 6, 10), 6),        # wave pieces of 6 channels (64..69) and of 3
                                         ((2, 200, 4, 6), 0)],      # eight words, the last with one 8-channel piece
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"case{v}")
def test_avgpool2_bn_pack2_lds_form(shape, first):
    assert pixel_words(shape) < WIDE_PIXEL_WORDS
    x, a, b, planted = pool2_input(shape, first=first)
    check_pool2(dev(x), shape, a, b, pool2_reference(x, a, b), planted, ALL_RELU, "lds")


@pytest.fixture(scope="module")
def wide():
    """6x200x112x112 (60 MB), the smallest batch of this image over the threshold: one generated image under six exact
    scales, the planted windows and affines on top; its reference is computed once and shared."""
    shape = (6, 200, 112, 112)
    one = gen.activation("special", gen.seed_of("pack-family-wide"), (1,) + shape[1:])
    x = np.concatenate([one * np.float32(s) for s in (1, -1, 0.5, -2, 4, -0.25)])
    plant_windows(x, 2)
    a, b = affines(2, shape[1], gen.seed_of("pack-family-wide-aff"))
    x4 = np.zeros((shape[0], shape[1], 1, 1), np.float32)
    planted = plant_affine(x4, a[0], b[0], [(0, 0)], rot=shape[1] - 5)
    for c, *_ in planted:
        x[:, c, -2:, -2:] = x4[:, c]
        a[1, c], b[1, c] = a[0, c], b[0, c]
    return dict(shape=shape, x=dev(x), a=a, b=b, planted=planted, ref=pool2_reference(x, a, b))


def test_avgpool2_bn_pack2_wide_form(wide):
    assert pixel_words(wide["shape"]) == 150528 >= WIDE_PIXEL_WORDS
    check_pool2(wide["x"], wide["shape"], wide["a"], wide["b"], wide["ref"], wide["planted"], ALL_RELU, "wide")


def test_avgpool2_bn_pack2_just_under_the_switch(wide):
    """The same tensor without its last image: 125440 pixel-words, the LDS form on a 19600-workgroup grid."""
    shape = (5,) + wide["shape"][1:]
    assert pixel_words(shape) == 125440 < WIDE_PIXEL_WORDS
    t, vals = wide["ref"]
    ref = (t[:5], {key: v[:5] for key, v in vals.items()})
    check_pool2(wide["x"][:5], shape, wide["a"], wide["b"], ref, wide["planted"], ALL_RELU, "lds-large")


def test_avgpool2_bn_pack2_refuses_a_four_byte_base():
    shape = (2, 70, 6, 10)
    x, a, b, _ = pool2_input(shape, "normal")
    t = carve(x, 1)
    assert t.data_ptr() % 8 == 4
    before = native.launch_count()
    with pytest.raises(NativeError):
        hipops.avgpool2_bn_pack2(t, (dev(a[0]), dev(b[0])), True, (dev(a[1]), dev(b[1])), False, out_f32=True)
    assert native.launch_count() == before


# ---- 6. BatchNorm -> max pool -> ReLU -> fp32 and planes -------------------------------------------------------------
def maxpool_kernel(t, k, s, p):
    """launch_bn_relu_maxpool_pack's choice (torch's own allocations for the output are 8-byte aligned)."""
    W = t.shape[3]
    vec = (k, s, p) == (3, 2, 1) and W % 4 == 0 and (W + 2 * p - k) // s + 1 == W // 2 and t.data_ptr() % 16 == 0
    return "vector" if vec else "generic"


MAXPOOL_CASES = [
    ((3, 70, 7, 8), (3, 2, 1), 0, "vector"),        # odd H
    ((2, 33, 8, 4), (3, 2, 1), 0, "vector"),        # one pair per row
    ((5, 70, 20, 24), (3, 2, 1), 0, "vector"),      # 300 pairs: two workgroups
    ((2, 70, 9, 11), (3, 2, 1), 0, "generic"),      # the same geometry, W % 4 != 0
    ((5, 70, 20, 24), (3, 2, 1), 1, "generic"),     # the vector shape on a 4-byte base
    ((2, 70, 9, 11), (2, 2, 0), 0, "generic"),
    ((3, 70, 9, 11), (3, 1, 1), 0, "generic"),      # 297 outputs
]
assert {c[1] for c in MAXPOOL_CASES} == set(MAXPOOL_GEOMETRIES)


@pytest.mark.parametrize("shape,geo,off,kernel", MAXPOOL_CASES,
                         ids=[f"{'x'.join(map(str, c[0]))}-k{c[1][0]}s{c[1][1]}p{c[1][2]}-off{c[2]}-{c[3]}" for c in MAXPOOL_CASES])
def test_bn_relu_maxpool_pack_against_oracle(shape, geo, off, kernel):
    """No NaN inside a window (the kernel drops it through fmaxf where torch propagates it: a separate decision)."""
    N, C, H, W = shape
    k, s, p = geo
    x = maxpool_input(gen.seed_of("pack-family-max", shape, geo), shape)
    a, b = affines(1, C, gen.seed_of("pack-family-max-aff", shape))
    assert (a < 0).any() and not np.isnan(x).any()
    t = carve(x, off)
    assert maxpool_kernel(t, k, s, p) == kernel and t.data_ptr() % 16 == 4 * off
    aligned = carve(x, 0) if off else None
    for aff in ((a[0], b[0]), (None, None)):
        for relu in (True, False):
            want = oracle.bn_maxpool(x, *aff, relu, k, s, p)
            tag = (aff[0] is not None, relu)
            y, pk = hipops.bn_relu_maxpool_pack(t, dev(aff[0]), dev(aff[1]), relu, k, s, p)
            assert same_f32(y.cpu().numpy(), want), (tag, int((y.cpu().numpy() != want).sum()))
            assert_planes(pk, want, tag)
            assert pk.nonneg == relu and (relu or u64(pk.M).any())
            y2, none = hipops.bn_relu_maxpool_pack(t, dev(aff[0]), dev(aff[1]), relu, k, s, p, out_packed=False)
            assert none is None and torch.equal(y2.view(torch.int32), y.view(torch.int32))
            none, pk3 = hipops.bn_relu_maxpool_pack(t, dev(aff[0]), dev(aff[1]), relu, k, s, p, out_f32=False)
            assert none is None
            assert_same_planes(pk3, pk, tag)
            if off:
                ya, pka = hipops.bn_relu_maxpool_pack(aligned, dev(aff[0]), dev(aff[1]), relu, k, s, p)
                assert maxpool_kernel(aligned, k, s, p) == "vector"
                assert torch.equal(ya.view(torch.int32), y.view(torch.int32))
                assert_same_planes(pka, pk, tag)

"""The dense gradient kernels (csrc/grad.hip: dgrad and wgrad on the matrix cores) and the weight hook of a training step
(csrc/xnor_train.hip) against the float64 / integer references of tests/grad_ref.py, bit for bit.

No comparison here has a tolerance.  The real operand of dgrad / wgrad is small integers times a power of two, so every
product and every partial sum in any order is exact in fp32 (tests/grad_ref.py: assert_exact_inputs proves it per case, in
integer arithmetic); the weights of the hook are dyadic, so its double sums are exact (assert_exact_weight_inputs).  Each
case of the table states the host-side condition that selects its kernel instantiation and asserts it; completeness
assertions over the table keep every reachable instantiation, slot width and image split in it."""
import functools

import numpy as np
import pytest
import torch

import bnn_amd as bnn
from bnn_amd import hipops, native, training
from bnn_amd.native import NativeError
from bnn_amd.ops import BasicInputBinarizer, XNORWeightBinarizer
from tests import grad_ref as R
from tests.golden import gen

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = np.float32, np.float64
ONE_BELOW = np.nextafter(F32(1), F32(0))
# every sign class and both sides of the STE boundary |x| < 1
X_VALUES = np.array([0.0, -0.0, 0.5, -0.5, 1.0, -1.0, ONE_BELOW, -ONE_BELOW, 2.0, -2.0, np.nan, np.inf, -np.inf, 1e-45,
                     -1e-45], F32)
G_SHIFTS = (0, -40, 20)


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)          # (a copy: the cached inputs are read-only)


def ints(seed, shape, lo, hi):
    return np.floor(gen.uniform(seed, shape) * (hi - lo + 1)).astype(np.int64) + lo


def dirty(nbytes):
    """The allocator's next block of this size starts as garbage: an element a kernel leaves out is not a lucky 0."""
    torch.empty(int(nbytes), dtype=torch.uint8, device=DEV).fill_(0xAB)


def assert_same_bits(got, want64, tag):
    """`got` (fp32, device) is `want64` (float64, exactly representable) in every bit of every element."""
    want = np.asarray(want64, F64)
    w32 = want.astype(F32)
    assert (w32.astype(F64) == want).all(), (tag, "the reference is not an fp32 number")
    assert tuple(got.shape) == want.shape, (tag, tuple(got.shape), want.shape)
    ok = torch.equal(got.view(torch.int32).cpu(), torch.from_numpy(w32.view(np.int32)))
    if not ok:
        g = got.cpu().numpy()
        bad = np.argwhere(g.view(np.uint32) != w32.view(np.uint32))
        first = [(tuple(int(v) for v in i), float(g[tuple(i)]), float(w32[tuple(i)])) for i in bad[:8]]
        raise AssertionError(f"{tag}: {len(bad)} of {g.size} elements differ; (index, got, want): {first}; "
                             f"per axis: {[sorted(set(bad[:, a].tolist()))[:12] for a in range(bad.shape[1])]}")


# ---- the geometry of csrc/grad.hip, restated ---------------------------------------------------------------------------
def geo(H, W, ks, stride, dgrad):
    """make_geo: the pixel domain the 64-slot chunks tile (x for a stride-1 dgrad, else the g grid), its slot width,
    rows per chunk R and chunks per image."""
    Hg, Wg = (H - 1) // stride + 1, (W - 1) // stride + 1
    h, w = (H, W) if dgrad and stride == 1 else (Hg, Wg)
    slot = 8
    while slot < w:
        slot *= 2
    RR = 64 // slot
    Rr = min(RR, h)
    return dict(h=h, w=w, slot=slot, RR=RR, R=Rr, chunks=-(-h // Rr))


def dgrad_inst(C, ks, stride):
    """launch_dgrad_t: (NSUB, KS, S2)"""
    return (2 if C > 64 else 1, ks, stride == 2)


def wgrad_si(H, W, ks, stride):
    """launch_wgrad_k: sign(x) fill items of a chunk = 16 NC (ST RR + 2 PD) (slot / 8), NC = 2 (3x3) or 8 (1x1); SI = items
    per thread of the 256."""
    q = geo(H, W, ks, stride, False)
    items = 16 * (2 if ks == 3 else 8) * (stride * q["RR"] + 2 * (ks // 2)) * (q["slot"] // 8)
    return -(-items // 256)


def default_splits(N, O, C, ks):
    """grad_wgrad_splits: ~1024 workgroups, at most one per image, then evened out."""
    cb = 32 if ks == 3 else 128
    blocks = -(-O // 64) * -(-C // cb)
    s = max(1, min(N, -(-1024 // blocks)))
    per = -(-N // s)
    return -(-N // per)


def test_the_reachable_wgrad_fill_widths():
    """SI over every geometry the entry points accept (x is at most 64 wide, so the g grid of a stride-2 layer at most
    32): 2 or 3 for 3x3 stride 1, 3 for stride 2, 4 for 1x1.  SI = 1 is instantiated and never launched."""
    reach = {(st, ks): {wgrad_si(H, W, ks, st) for H in (1, 2, 3, 5, 9, 64) for W in range(1, 65)}
             for st, ks in ((1, 3), (2, 3), (1, 1))}
    assert reach == {(1, 3): {2, 3}, (2, 3): {3}, (1, 1): {4}}


# ---- the case table ------------------------------------------------------------------------------------------------------
# (id, N, O, C, H, W, ks, stride, every valid split?, then what the case reaches: dgrad slot, wgrad slot, dgrad chunks per
#  image, ragged last chunk of the dgrad / wgrad domain, SI)
CASES = [
    # 3x3 / stride 1: the slot is of W; both sides of 8 | 16 | 32 | 64
    ("s1-w1-h1", 2, 1, 1, 1, 1, 3, 1, False, 8, 8, 1, False, 2),        # H = 1 < RR
    ("s1-w8", 2, 8, 15, 9, 8, 3, 1, False, 8, 8, 2, True, 2),           # H % R = 1; waves 1-3 of the fill lie past O
    ("s1-w9", 2, 31, 16, 5, 9, 3, 1, False, 16, 16, 2, True, 2),
    ("s1-w16", 2, 32, 17, 3, 16, 3, 1, False, 16, 16, 1, False, 2),     # H < RR: R = H
    ("s1-w17", 2, 33, 33, 3, 17, 3, 1, False, 32, 32, 2, True, 2),      # a second block of 32 o with one channel
    ("s1-w32", 2, 70, 64, 4, 32, 3, 1, False, 32, 32, 2, False, 2),
    ("s1-w33", 2, 8, 65, 2, 33, 3, 1, False, 64, 64, 2, False, 3),      # NSUB 2 with one channel in the upper half
    ("s1-w64", 2, 33, 130, 3, 64, 3, 1, False, 64, 64, 3, False, 3),    # two channel blocks of 128
    ("s1-n5", 5, 8, 16, 4, 16, 3, 1, True, 16, 16, 1, False, 2),        # one chunk per image: advance() crosses at y0 = 0
    ("s1-n7", 7, 33, 17, 5, 32, 3, 1, True, 32, 32, 3, True, 2),        # three chunks, the last ragged
    # 3x3 / stride 2: the slot is of Wg; every parity of H and W, images where parity classes have no pixel
    ("s2-1x1", 2, 8, 1, 1, 1, 3, 2, False, 8, 8, 1, False, 3),
    ("s2-1x2", 2, 1, 15, 1, 2, 3, 2, False, 8, 8, 1, False, 3),
    ("s2-2x1", 2, 31, 16, 2, 1, 3, 2, False, 8, 8, 1, False, 3),
    ("s2-w15", 2, 32, 17, 17, 15, 3, 2, False, 8, 8, 2, True, 3),       # odd x odd, Hg = 9 = 8 + 1
    ("s2-w16", 2, 33, 33, 4, 16, 3, 2, False, 8, 8, 1, False, 3),       # even x even
    ("s2-w17", 2, 70, 64, 10, 17, 3, 2, False, 16, 16, 2, True, 3),     # even x odd
    ("s2-w33", 2, 8, 65, 5, 33, 3, 2, False, 32, 32, 2, True, 3),       # odd x odd, NSUB 2
    ("s2-w64", 2, 33, 130, 5, 64, 3, 2, False, 32, 32, 2, True, 3),     # odd x even
    ("s2-n5", 5, 8, 16, 8, 8, 3, 2, True, 8, 8, 1, False, 3),
    ("s2-n7", 7, 33, 17, 9, 33, 3, 2, True, 32, 32, 3, True, 3),
    # 1x1
    ("k1-w1", 2, 1, 1, 1, 1, 1, 1, False, 8, 8, 1, False, 4),
    ("k1-w8", 2, 8, 15, 9, 8, 1, 1, False, 8, 8, 2, True, 4),
    ("k1-w9", 2, 31, 64, 5, 9, 1, 1, False, 16, 16, 2, True, 4),
    ("k1-w17", 2, 32, 65, 3, 17, 1, 1, False, 32, 32, 2, True, 4),
    ("k1-w33", 2, 70, 130, 2, 33, 1, 1, False, 64, 64, 2, False, 4),    # wgrad: two channel blocks of 128
    ("k1-w64", 2, 33, 17, 2, 64, 1, 1, False, 64, 64, 2, False, 4),
    ("k1-n5", 5, 8, 16, 8, 8, 1, 1, True, 8, 8, 1, False, 4),
    ("k1-n7", 7, 33, 33, 5, 32, 1, 1, True, 32, 32, 3, True, 4),
    # the library's own split with more than one image per workgroup: 20 images in 7 slabs of 3, 3, 3, 3, 3, 3, 2
    ("big-s1", 20, 512, 512, 7, 7, 3, 1, False, 8, 8, 1, False, 2),
    ("big-s2", 20, 512, 512, 14, 14, 3, 2, False, 8, 8, 1, False, 3),
]
IDS = [c[0] for c in CASES]


def test_the_table_reaches_every_instantiation_slot_and_split():
    d_inst, w_inst, d_slots, w_slots, pers = set(), set(), set(), set(), set()
    for cid, N, O, C, H, W, ks, st, every, dslot, wslot, dchunks, ragged, si in CASES:
        qd, qw = geo(H, W, ks, st, True), geo(H, W, ks, st, False)
        assert (qd["slot"], qw["slot"], qd["chunks"], wgrad_si(H, W, ks, st)) == (dslot, wslot, dchunks, si), cid
        assert ragged == (qd["h"] % qd["R"] != 0), cid
        assert N <= 7 or cid.startswith("big"), cid
        d_inst.add(dgrad_inst(C, ks, st))
        w_inst.add((st, ks, si))
        d_slots.add((st, ks, dslot))
        w_slots.add((st, ks, wslot))
        for s in (R.valid_splits(N) if every else [default_splits(N, O, C, ks)]):
            rg = R.split_ranges(N, s)
            pers.add((st, ks, qw["chunks"] > 1, rg[0][1] - rg[0][0], rg[-1][1] - rg[-1][0] != rg[0][1] - rg[0][0]))
    # (each runs from the fp32 x and from the planes: XP off and on)
    assert d_inst == {(n, k, s2) for n in (1, 2) for k, s2 in ((3, False), (3, True), (1, False))}        # 6 x XP = 12
    assert w_inst == {(1, 3, 2), (1, 3, 3), (2, 3, 3), (1, 1, 4)}
    assert d_slots >= {(1, k, s) for k in (1, 3) for s in (8, 16, 32, 64)} | {(2, 3, s) for s in (8, 16, 32)}
    assert w_slots >= {(1, k, s) for k in (1, 3) for s in (8, 16, 32, 64)} | {(2, 3, s) for s in (8, 16, 32)}
    for st, ks in ((1, 3), (2, 3), (1, 1)):
        for multi in (False, True):          # one chunk per image and several
            got = {(per, rag) for a, b, m, per, rag in pers if (a, b, m) == (st, ks, multi)}
            assert got >= {(1, False), (2, True), (3, True), (5, False) if not multi else (7, False)}, (st, ks, multi, got)
    assert {W for c in CASES for W in [c[5]] if c[7] == 1 and c[6] == 3} >= {1, 8, 9, 16, 17, 32, 33, 64}
    assert {W for c in CASES for W in [c[5]] if c[7] == 2} >= {1, 2, 15, 16, 17, 33, 64}
    assert {c[3] for c in CASES} >= {1, 15, 16, 17, 33, 64, 65, 130} and {c[2] for c in CASES} >= {1, 8, 31, 32, 33, 70}
    assert {(c[4] % 2, c[5] % 2) for c in CASES if c[7] == 2} == {(0, 0), (0, 1), (1, 0), (1, 1)}


@functools.lru_cache(maxsize=None)
def case_data(cid):
    """Inputs and references of a case at g shift 0 (the others are exact multiples), computed once."""
    _, N, O, C, H, W, ks, st, every = next(c for c in CASES if c[0] == cid)[:9]
    seed = gen.seed_of("grad-exact", cid)
    Hg, Wg = (H - 1) // st + 1, (W - 1) // st + 1
    g = ints(seed, (N, O, Hg, Wg), -7, 7).astype(F32)
    alpha = (2.0 ** -(np.arange(O) % 5)).astype(F32)
    w_sign = ints(seed + 1, (O, C, ks, ks), -2, 2).clip(-1, 1).astype(F32)          # 1/5 zeros
    if O >= 3:
        alpha[2] = 0.0
    if O >= 4:
        w_sign[3] = 0.0                      # an output channel without weights
    if C >= 3:
        w_sign[:, 2] = 0.0                   # an input channel without weights
    x = X_VALUES[ints(seed + 2, (N, C, H, W), 0, len(X_VALUES) - 1)]
    splits = sorted(set((R.valid_splits(N) if every else []) + [default_splits(N, O, C, ks)]))
    for s in splits:
        for sh in G_SHIFTS:
            R.assert_exact_inputs(np.ldexp(g.astype(F64), sh), alpha, x.shape, ks, st, R.split_ranges(N, s))
    gx = R.dgrad_ref(g, x, w_sign, alpha, ks, st)
    slabs = {s: R.wgrad_ref(g, x, ks, st, R.split_ranges(N, s)) for s in splits}
    for a in (g, alpha, w_sign, x, gx, *slabs.values()):
        a.setflags(write=False)
    return dict(g=g, alpha=alpha, w_sign=w_sign, x=x, splits=splits, gx=gx, slabs=slabs)


@pytest.mark.parametrize("cid", IDS)
def test_input_gradient_equals_the_integer_answer_in_every_bit(cid):
    _, N, O, C, H, W, ks, st = next(c for c in CASES if c[0] == cid)[:8]
    d = case_data(cid)
    assert hipops.grad_supported(d["x"].shape, d["w_sign"].shape, st, ks // 2, 1)
    x = dev(d["x"])
    sv = hipops.pack_act_ste(x)
    # the fragments from the signs themselves, alpha on its own: an alpha of 0 does not hide its channel's signs
    packed, one = hipops.grad_pack_weight(dev(d["w_sign"]))
    assert np.array_equal(packed.cpu().numpy(), R.grad_fragments_ref(d["w_sign"], O, C, ks))
    assert np.array_equal(one.cpu().numpy(), np.abs(d["w_sign"]).reshape(O, -1).max(1))
    alpha = dev(d["alpha"])
    for sh in G_SHIFTS:
        g = dev(np.ldexp(d["g"], sh))
        want = np.ldexp(d["gx"], sh)
        for form, xin in (("fp32", x), ("planes", sv)):
            dirty(x.numel() * 4)
            gx = hipops.bconv_grad_input(g, xin, packed, alpha, ks, st)
            assert_same_bits(gx, want, (cid, "dgrad", form, f"g * 2^{sh}"))


@pytest.mark.parametrize("cid", IDS)
def test_weight_gradient_slabs_equal_the_integer_answer_in_every_bit(cid):
    _, N, O, C, H, W, ks, st, every = next(c for c in CASES if c[0] == cid)[:9]
    d = case_data(cid)
    lib = native.require()
    default = int(lib.bnn_hip_bconv_grad_weight_splits(N, O, C, ks))
    assert default == default_splits(N, O, C, ks)
    if cid.startswith("big"):
        assert default == 7 and -(-N // default) == 3          # more than one image per workgroup, the last split ragged
    x = dev(d["x"])
    sv = hipops.pack_act_ste(x)
    g0 = dev(d["g"])
    for form, xin in (("fp32", x), ("planes", sv)):
        for s in d["splits"]:
            dirty(s * O * C * ks * ks * 4)
            part = hipops.bconv_grad_weight(g0, xin, ks, st, reduce=False, splits=s)
            assert_same_bits(part, d["slabs"][s], (cid, "wgrad", form, f"splits {s}"))
        for sh in G_SHIFTS[1:]:
            part = hipops.bconv_grad_weight(dev(np.ldexp(d["g"], sh)), xin, ks, st, reduce=False)
            assert part.shape[0] == default
            assert_same_bits(part, np.ldexp(d["slabs"][default], sh), (cid, "wgrad", form, f"g * 2^{sh}"))
        whole = hipops.bconv_grad_weight(g0, xin, ks, st)          # reduce=True: the slabs, added (integers: exact)
        assert_same_bits(whole, d["slabs"][default].sum(0) + 0.0, (cid, "wgrad", form, "reduced"))


def test_the_wrapper_refuses_an_image_split_the_kernel_cannot_run():
    g, x = torch.zeros((5, 8, 4, 4), device=DEV), torch.zeros((5, 8, 4, 4), device=DEV)
    for bad in (6, 4, 0, -1):
        for xin in (x, hipops.pack_act_ste(x)):
            with pytest.raises(NativeError):
                hipops.bconv_grad_weight(g, xin, 3, 1, reduce=False, splits=bad)
    assert hipops.bconv_grad_weight(g, x, 3, 1, reduce=False, splits=3).shape == (3, 8, 8, 3, 3)


# ---- C. the weight operand of dgrad, byte for byte ------------------------------------------------------------------------
def dyadic_weights(seed, shape):
    """Multiples of 2^-6 in (-3, 3), with exact zeros, -0 and |w| == 1 planted."""
    w = (ints(seed, shape, -191, 191) / 64.0).astype(F32)
    flat = w.reshape(-1)
    flat[::9] = 0.0
    flat[4::31] = -0.0
    flat[2::37] = 1.0
    flat[3::41] = -1.0
    return w


@pytest.mark.parametrize("O", [1, 31, 33, 70])
@pytest.mark.parametrize("C", [1, 15, 17, 130])
def test_sign_fragments_and_alpha_equal_the_documented_layout_byte_for_byte(O, C):
    for ks in (1, 3):
        w = dyadic_weights(gen.seed_of("frag", O, C, ks), (O, C, ks, ks))
        if O > 1:
            w[1] = 0.0                                   # a channel whose signs are all 0: alpha 0
        for center in (False, True):
            for compute_alpha in (False, True):
                tag = (O, C, ks, center, compute_alpha)
                R.assert_exact_weight_inputs(w, np.zeros_like(w), center, compute_alpha)
                nbytes = -(-O // 32) * ks * ks * -(-C // 16) * 64 * 16
                # one launch, from W
                dirty(nbytes)
                got_p, got_a = hipops.xnor_grad_pack_weight(dev(w), center, compute_alpha)
                assert got_p.numel() == nbytes
                assert np.array_equal(got_p.cpu().numpy(), R.grad_fragments_ref(R.centred_sign_ref(w, center), O, C, ks)), tag
                assert_same_bits(got_a, R.alpha_ref(w, center, compute_alpha), tag)
                if O > 1:
                    assert float(got_a[1]) == 0.0
                # from What
                what, alpha = R.xnor_what_ref(w, center, compute_alpha)
                dirty(nbytes)
                got_p, got_a = hipops.grad_pack_weight(dev(what))
                assert np.array_equal(got_p.cpu().numpy(), R.grad_fragments_ref(what, O, C, ks)), tag
                assert_same_bits(got_a, np.abs(what).reshape(O, -1).max(1), tag)


@pytest.mark.parametrize("center", [False, True], ids=["plain", "centred"])
def test_one_launch_weight_prep_keeps_the_finite_signs_of_a_channel_with_a_nan_weight(center):
    """The documented behaviour of xnor_grad_pack_kernel: the channel keeps the signs of its finite weights (centred: of the
    taps whose mean is finite), its alpha is NaN; every other channel is untouched."""
    O, C, ks = 33, 17, 3
    w = dyadic_weights(gen.seed_of("frag-nan"), (O, C, ks, ks))
    clean = w.copy()
    w[5, 3, 1, 1] = np.nan
    clean[5] = 0.0                                       # (the sums of the other channels are proven exact)
    R.assert_exact_weight_inputs(clean, np.zeros_like(w), center, True)
    dirty(2 * 9 * 2 * 64 * 16)
    got_p, got_a = hipops.xnor_grad_pack_weight(dev(w), center, True)
    sign = R.centred_sign_ref(w, center)
    assert sign[5, 3, 1, 1] == 0 and (sign[5] != 0).any() and ((sign[5, :, 1, 1] == 0).all() == center)
    assert np.array_equal(got_p.cpu().numpy(), R.grad_fragments_ref(sign, O, C, ks))
    want = R.alpha_ref(w, center, True)
    a = got_a.cpu().numpy()
    assert np.isnan(want[5]) and np.isnan(a[5])
    keep = np.arange(O) != 5
    assert np.array_equal(a[keep].view(np.uint32), want[keep].view(np.uint32))


# ---- D. xnor_what / xnor_weight_backward, bit for bit ---------------------------------------------------------------------
HOOK_SHAPES = [
    (3, 5, 3, 3),        # K = 45: fewer elements than threads
    (4, 33, 3, 3),       # C < 256 with centring, K % 256 != 0
    (5, 1, 3, 3), (5, 1, 1, 1),      # one input channel: centred, every Wc is 0
    (4, 70, 1, 1),       # taps 1
    (3, 17, 5, 5),       # taps 25 do not divide 256, K = 425: the running index t = (t + 256) % taps
    (2, 9, 7, 7),        # taps 49
    (2, 300, 3, 3),      # C > 256: the channel loop of the centring runs twice
    (512, 512, 3, 3),
]


def hook_weights(shape):
    """Dyadic weights with the STE boundary planted before centring (|w| == 1, the float below 1) and, in channel 0 / tap
    0 of a layer with >= 12 input channels, after it: a column of mean 1/2 with 3/2, -1/2, 3/2 - 2^-23 and -1/2 + 2^-23."""
    O, C, kh, kw = shape
    w = dyadic_weights(gen.seed_of("hook-w", shape), shape)
    T = kh * kw
    for o in range(min(O, 8)):               # (in +- pairs per tap column: the column sums stay multiples of 2^-6, and the
        for t in range(o % 2, T, 5):         # rounded mean with them far above the last bit of a double sum)
            w[o, (o + t) % C, t // kw, t % kw] = ONE_BELOW
            if C > 1:
                w[o, (o + t + 1) % C, t // kw, t % kw] = -ONE_BELOW
    if C >= 12:
        col = np.where(np.arange(C) % 2 == 0, 0.25, 0.75).astype(F32)
        col[0], col[1], col[2], col[3] = 1.5, -0.5, F32(1.5) - F32(2.0 ** -23), F32(-0.5) + F32(2.0 ** -23)
        if C % 2:
            col[-1] = 0.5
        w[0, :, 0, 0] = col
    return w


def hook_dwhat(shape, slabs, pow2):
    """Small integers; with `pow2` every slab sum is 0 or +-2^k, k <= 3, so that its product with any alpha is exact."""
    seed = gen.seed_of("hook-d", shape, slabs, pow2)
    k = ints(seed, shape, -4, 4)
    total = (np.sign(k) * 2.0 ** (np.abs(k) - 1)).astype(F32) if pow2 else ints(seed, shape, -7, 7).astype(F32)
    if slabs == 1:
        return total
    rest = ints(seed + 1, (slabs - 1,) + tuple(shape), -5, 5).astype(F32)
    return np.concatenate([rest, (total - rest.sum(0))[None]]).astype(F32)


@pytest.mark.parametrize("shape", HOOK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_weight_hook_equals_the_reference_in_every_bit(shape):
    """dWhat alpha is exact by construction (dWhat a power of two where alpha is computed), so whether the compiler
    contracts `ste + sgn * gk` — or the STE product with it — into an fma cannot change a bit: sgn * gk is exact too."""
    O, C = shape[:2]
    w = hook_weights(shape)
    wd = dev(w)
    for center in (False, True):
        v = R.centred_weight_ref(w, center).reshape(O, C, -1)
        if (not center and w.size > 50) or (center and C >= 12):       # both sides of the STE boundary are there
            assert (np.abs(v) == 1).any() and ((np.abs(v) < 1) & (np.abs(v) > 0.9999)).any()
        if center and C >= 12:               # the planted column: |Wc| == 1 exactly and the float below, after centring
            assert abs(v[0, 0, 0]) == 1 and abs(v[0, 1, 0]) == 1 and abs(v[0, 2, 0]) == ONE_BELOW - F32(2.0 ** -24)
        for compute_alpha in (False, True):
            tag = (shape, center, compute_alpha)
            want, want_a = R.xnor_what_ref(w, center, compute_alpha)
            dirty(w.nbytes)
            what, alpha = hipops.xnor_what(wd, center, compute_alpha, return_alpha=True)
            for slabs in (1, 3):
                dwhat = hook_dwhat(shape, slabs, compute_alpha)
                R.assert_exact_weight_inputs(w, dwhat, center, compute_alpha)
                if slabs == 1:               # (the proof covers the forward's sums: the same centre and alpha)
                    assert_same_bits(what, want, tag)
                    assert_same_bits(alpha, want_a, tag)
                    assert torch.equal(hipops.xnor_what(wd, center, compute_alpha), what)
                dirty(w.nbytes)
                dw = hipops.xnor_weight_backward(wd, dev(dwhat), center, compute_alpha)
                assert_same_bits(dw, R.xnor_weight_backward_ref(w, dwhat, center, compute_alpha), tag + (slabs,))
            if compute_alpha and shape[0] <= 8 and shape[2] <= 5:
                # the inference path's packer rounds the same mean: on sums that are exact, the same bits
                pw = hipops.pack_weight(wd, center=center, compute_alpha=True)
                assert_same_bits(pw.alpha.view(-1)[:O], want_a, tag + ("pack_weight",))


@pytest.mark.parametrize("center", [False, True], ids=["plain", "centred"])
def test_weight_hook_with_a_nan_weight(center):
    """One NaN weight: its channel's alpha is NaN; where the reference is NaN the kernel is NaN, everything else — the
    other channels, and the elements of the channel that the STE masks — has the reference's bits."""
    shape = (4, 33, 3, 3)
    w = hook_weights(shape)
    clean = w.copy()
    w[2, 7, 1, 2] = np.nan
    clean[2] = 0.25
    dwhat = hook_dwhat(shape, 3, True)
    R.assert_exact_weight_inputs(clean, dwhat, center, True)
    want, want_a = R.xnor_what_ref(w, center, True)
    want_dw = R.xnor_weight_backward_ref(w, dwhat, center, True)
    assert np.isnan(want_a[2]) and np.isnan(want[2]).all() and not np.isnan(np.delete(want, 2, 0)).any()
    assert np.isnan(want_dw[2]).any() and not np.isnan(np.delete(want_dw, 2, 0)).any()
    what, alpha = hipops.xnor_what(dev(w), center, True, return_alpha=True)
    dw = hipops.xnor_weight_backward(dev(w), dev(dwhat), center, True)
    for got, ref in ((what, want), (alpha, want_a), (dw, want_dw)):
        got = got.cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(ref))
        assert np.array_equal(np.nan_to_num(got).view(np.uint32), np.nan_to_num(ref).view(np.uint32))


# ---- end to end: one training step of a converted Conv2d ---------------------------------------------------------------------
def test_training_step_of_a_converted_conv_gives_the_integer_weight_gradient(monkeypatch):
    """N = 20, 512 -> 512, 7 x 7: dL/dW goes through bconv_grad_weight(reduce=False) — 7 slabs of 3, 3, 3, 3, 3, 3, 2 images —
    and xnor_weight_backward with the slabs; both and dL/dx equal the references bit for bit.  The weights are +-1/2 and
    +-3/2 in equal numbers (alpha = 1, half of them outside the STE) in the even channels, +-1/4 and +-3/4 (alpha = 1/2)
    in the odd ones, so dWhat alpha is exact for any integer dWhat."""
    N, O, C, H, W = 20, 512, 512, 7, 7
    seed = gen.seed_of("grad-exact-e2e")
    mag = np.where(np.argsort(gen.uniform(seed, (O, C * 9)), axis=1) % 2 == 0, 0.5, 1.5)
    mag = mag * np.where(np.arange(O) % 2 == 0, 1.0, 0.5)[:, None]
    w = (mag * np.where(gen.uniform(seed + 1, (O, C * 9)) < 0.5, -1, 1)).astype(F32).reshape(O, C, 3, 3)
    x = X_VALUES[ints(seed + 2, (N, C, H, W), 0, len(X_VALUES) - 1)]
    g = ints(seed + 3, (N, O, H, W), -7, 7).astype(F32)
    ranges = R.split_ranges(N, 7)
    what, alpha = R.xnor_what_ref(w, False, True)
    assert np.array_equal(alpha, np.where(np.arange(O) % 2 == 0, 1.0, 0.5))
    R.assert_exact_inputs(g, alpha, x.shape, 3, 1, ranges)
    slabs = R.wgrad_ref(g, x, 3, 1, ranges).astype(F32)
    R.assert_exact_weight_inputs(w, slabs, False, True)

    conv = torch.nn.Conv2d(C, O, 3, padding=1, bias=False)
    conv.weight.data.copy_(torch.from_numpy(w))
    cfg = bnn.BConfig(activation_pre_process=BasicInputBinarizer, activation_post_process=bnn.Identity,
                      weight_pre_process=XNORWeightBinarizer)
    layer = bnn.prepare_binary_model(conv, cfg).to(DEV).train()
    seen = {}
    real_wgrad, real_hook = hipops.bconv_grad_weight, hipops.xnor_weight_backward

    def spy_wgrad(*a, **k):
        out = real_wgrad(*a, **k)
        seen["wgrad"] = (k.get("reduce"), out.clone())
        return out

    def spy_hook(w_, dwhat, *a, **k):
        seen["hook"] = tuple(dwhat.shape)
        return real_hook(w_, dwhat, *a, **k)
    monkeypatch.setattr(hipops, "bconv_grad_weight", spy_wgrad)
    monkeypatch.setattr(hipops, "xnor_weight_backward", spy_hook)
    xt = dev(x).requires_grad_(True)
    from bnn_amd.inference import per_layer_forward
    with per_layer_forward():
        layer(xt).backward(dev(g))
    assert seen["wgrad"][0] is False and seen["hook"] == (7, O, C, 3, 3)
    assert_same_bits(seen["wgrad"][1], slabs, "the slabs of the step")
    assert_same_bits(layer.weight.grad, R.xnor_weight_backward_ref(w, slabs, False, True), "dL/dW")
    assert_same_bits(xt.grad, R.dgrad_ref(g, x, np.sign(w), alpha, 3, 1), "dL/dx")
    assert training.ENABLED and training.BINARY_GRADS

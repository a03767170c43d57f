"""Every kernel route of launch_bconv() (csrc/bconv.hip) against the CPU oracle, bit for bit.

A declared table: each case names its shape, its epilogue, its flags and the route it is meant to exercise.  The test
first asks the launch ladder itself (bnn_hip_bconv2d_route) and asserts the declared route — a constant or a profile mask
that moves the case to another instantiation fails there, loudly — then launches and compares with the oracle:

* the fp32 output with oracle.fused_epilogue / fused_epilogue2 of the dot of oracle.binary_conv2d_int,
* the planes with oracle.pack_act of the oracle's pack value, M all zero where the launch claims non-negative planes,
* for an output into a channel slice, the rest of the canvas with what it held.

The oracle is the only reference (no case compares two HIP launches) and there is no tolerance.  fp32 values are compared
as bit patterns, except that a NaN matches any NaN (the payload of a NaN is not part of the contract; BatchNorm shifts of
NaN are among the constants).  The completeness tests at the end assert that the table reaches every compiled launch
statement and holds the whole product of chunk class x profile x non-negative promise."""
import functools
import itertools
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import pytest
import torch

import oracle
from bnn_amd import hipops, native
from tests.golden import gen

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SITE, EP = native.SITE, native.ROUTE_PROFILES

# launch statements no case can reach, with the reason (an empty dict is the goal)
EXCLUDED_SITES = {
    SITE["SINGLE_SPLIT"]: "compiled out: BNN_SINGLE_GSPLIT == 1 in csrc/bconv.hip (#if BNN_SINGLE_GSPLIT > 1)",
}

CHUNKS_3X3 = {64: (2, 1), 128: (4, 1), 192: (2, 3), 256: (4, 2), 512: (4, 4)}     # C -> (cwc, nchunk)
CHUNKS_1X1 = {512: (16, 1), 256: (8, 1), 128: (4, 1), 64: (2, 1), 192: (2, 3)}
PROFILES_3X3 = ("PLAIN", "RUNTIME", "MID", "MIDT", "OUT", "OUTP", "LAST", "HB", "HB3")
PROFILES_1X1 = ("PLAIN", "RUNTIME", "DS")
SPLIT_PROFILES = ("MID", "MIDT", "OUT", "OUTP", "LAST")
PACKS = {"RUNTIME", "MID", "MIDT", "OUT", "OUTP", "HB"}                          # profiles (as used here) that write planes

# (N, H, W, stride, pad): ragged last tile and a tile count that is no multiple of 8 everywhere; 9 tiles = two per XCD slot
SHAPES = ((2, 9, 7, 1, 1),       # 126 pixels, 2 tiles
          (3, 14, 13, 1, 1),     # 546 pixels, 9 tiles
          (2, 14, 13, 2, 1),     # stride 2: 7 x 7, 98 pixels
          (3, 11, 9, 1, 0))      # pad 0: 9 x 7, 189 pixels, 3 tiles
SHAPES_1X1 = ((2, 9, 7, 1, 0), (3, 14, 13, 1, 0), (2, 14, 13, 2, 0))
OUT_CHANNELS = (40, 64, 96, 5)   # ragged 32-block (40, 5), all-zero tail block in pack mode (5, 40 -> no; 96 -> yes), full
# the unsplit multi-chunk kernels need >= 2048 waves under BNN_HIP_FLAG_THROUGHPUT: C = O = 256 -> 8 blocks x 8 * ceil(250 / 8)
UNSPLIT = (3, 73, 73, 1, 1)      # 15987 pixels = 250 tiles (ragged, six idle slots): exactly 2048 waves


@dataclass(frozen=True)
class Case:
    id: str
    C: int
    O: int
    shape: tuple                     # (N, H, W, stride, pad)
    profile: str
    nn: bool                         # non-negative input + BNN_HIP_FLAG_ACT_NONNEG
    route: tuple                     # declared: sorted (field, value) pairs of bnn_hip_conv_route
    k: int = 3
    dil: int = 1
    throughput: bool = False
    wz: bool = False                 # weights with exact zeros (BNN_HIP_FLAG_WEIGHT_ZEROS)
    entry: str = "fused"             # "fused": bnn_hip_bconv2d_fused, "plain": bnn_hip_bconv2d, "dot": bnn_hip_bconv2d_dot
    fold: Optional[tuple] = None     # (shortcut channels, pooled planes?)
    key: tuple = field(default=(), compare=False)      # its place in the product (completeness test)


def blocks_of(O, packed):
    return 2 * ((O + 63) // 64) if packed else (O + 31) // 32


def declare(site, profile, C, k, nn, *, pieces=1, bpw=1, fold=False, wz=False, tiled=True):
    cwc, nchunk = (CHUNKS_3X3 if k == 3 else CHUNKS_1X1).get(C, (2, C // 64))
    if not tiled:
        return tuple(sorted(dict(tiled=0, kh=k, kw=k, cwc=cwc, nchunk=nchunk, profile=EP["RUNTIME"], nonneg=0,
                                 weight_zeros=int(wz), multi=0, pieces=1, blocks_per_wave=1, shortcut_fold=0,
                                 site=SITE[site]).items()))
    multi = int(SITE[site] >= SITE["MULTI4_SPLIT4"] and site != "WZ_SINGLE")
    return tuple(sorted(dict(tiled=1, kh=k, kw=k, cwc=cwc, nchunk=nchunk, profile=EP[profile],
                             nonneg=int(nn and k == 3 and not wz), weight_zeros=int(wz), multi=multi, pieces=pieces,
                             blocks_per_wave=bpw, shortcut_fold=int(fold), site=SITE[site]).items()))


def build_table():
    cases = []
    # -- 3x3 chunk classes x profile x NN, latency mode, small shapes
    for C, (pi, prof), nn in itertools.product((64, 128, 192, 256), enumerate(PROFILES_3X3), (False, True)):
        cwc, nchunk = CHUNKS_3X3[C]
        shape = SHAPES[(pi + nn + C // 64) % 4]
        O = OUT_CHANNELS[(pi + 2 * nn + C // 128) % 4]
        if nchunk == 1:
            obw = prof == "PLAIN" and blocks_of(O, False) >= 2
            route = declare("SINGLE_OBW" if obw else "SINGLE", prof, C, 3, nn, bpw=2 if obw else 1)
        elif cwc == 4:
            four = prof in ("MID", "MIDT")
            route = declare("MULTI4_SPLIT4" if four else "MULTI4_SPLIT2", prof, C, 3, nn, pieces=4 if four else 2)
        else:
            route = declare("CHUNKS", prof, C, 3, nn)
        cases.append(Case(f"k3-c{C}-{prof}-{'nn' if nn else 'pm'}-o{O}-{'x'.join(map(str, shape))}", C, O, shape, prof, nn,
                          route, key=("class", C, prof, nn)))
    # (every single-chunk class needs both PLAIN kernels: one block per wave and BNN_SGPR_OBW blocks per wave)
    for C, nn, O in ((64, True, 5), (128, False, 5), (64, False, 96), (128, True, 96)):
        obw = O > 32
        cases.append(Case(f"k3-c{C}-PLAIN-{'nn' if nn else 'pm'}-o{O}-entry", C, O, SHAPES[1], "PLAIN", nn,
                          declare("SINGLE_OBW" if obw else "SINGLE", "PLAIN", C, 3, nn, bpw=2 if obw else 1), entry="plain",
                          key=("plain-entry", C, O)))
    cases.append(Case("k3-c512-OUT-nn-o40", 512, 40, SHAPES[0], "OUT", True,
                      declare("MULTI4_SPLIT2", "OUT", 512, 3, True, pieces=2), key=("class", 512)))
    for C, nn in ((128, True), (256, False), (192, True)):          # the raw integer dot: a run-time switch of EP_RUNTIME
        site = {128: "SINGLE", 256: "MULTI4_SPLIT2", 192: "CHUNKS"}[C]
        cases.append(Case(f"k3-c{C}-dot-{'nn' if nn else 'pm'}", C, 40, SHAPES[3], "RUNTIME", nn,
                          declare(site, "RUNTIME", C, 3, nn, pieces=2 if C == 256 else 1), entry="dot", key=("dot", C)))
    # -- 1x1 chunk widths x profile
    for (ci, C), (pi, prof) in itertools.product(enumerate((512, 256, 128, 64, 192)), enumerate(PROFILES_1X1)):
        shape, O, nn = SHAPES_1X1[(ci + pi) % 3], OUT_CHANNELS[(ci + pi) % 4], (ci + pi) % 2 == 1
        cases.append(Case(f"k1-c{C}-{prof}-{'nn' if nn else 'pm'}-o{O}-{'x'.join(map(str, shape))}", C, O, shape, prof, nn,
                          declare("CHUNKS", prof, C, 1, nn), k=1, key=("1x1", C, prof)))
    # -- the split axis of the multi-chunk C = 256 class
    for mode, prof, nn in itertools.product(("latency", "throughput", "unsplit"), SPLIT_PROFILES, (False, True)):
        if mode == "latency":
            four = prof in ("MID", "MIDT")
            shape, O, thr = SHAPES[1], 96, False
            route = declare("MULTI4_SPLIT4" if four else "MULTI4_SPLIT2", prof, 256, 3, nn, pieces=4 if four else 2)
        elif mode == "throughput":
            shape, O, thr = SHAPES[2], 40, True
            route = declare("MULTI4_SPLIT2", prof, 256, 3, nn, pieces=2)
        else:
            shape, O, thr = UNSPLIT, 256, True
            route = declare("MULTI4", prof, 256, 3, nn)
        cases.append(Case(f"split-{mode}-{prof}-{'nn' if nn else 'pm'}", 256, O, shape, prof, nn, route, throughput=thr,
                          key=("split", mode, prof, nn)))
    # -- the folded shortcut: four launch statements x shortcut channels x pooled / un-pooled planes
    for (site, C, shape, O0, thr), sc_C, pooled in itertools.product(
            (("SINGLE_FOLD", 128, SHAPES[0], 40, False), ("MULTI4_SPLIT2_FOLD", 256, SHAPES[0], 64, False),
             ("MULTI4_FOLD", 256, UNSPLIT, 256, True), ("CHUNKS_FOLD", 192, SHAPES[0], 96, False)),
            (64, 128, 256), (True, False)):
        if site == "MULTI4_FOLD" and not pooled and sc_C != 64:
            continue          # (un-pooled 145 x 145 planes of 128 / 256 channels: seconds of input generation, no other path)
        O = O0 if site == "MULTI4_FOLD" else OUT_CHANNELS[(OUT_CHANNELS.index(O0) + sc_C // 128) % 3]
        cases.append(Case(f"fold-{site}-sc{sc_C}-{'pooled' if pooled else 'unpooled'}-o{O}", C, O, shape, "OUT", True,
                          declare(site, "OUT", C, 3, True, pieces=2 if site == "MULTI4_SPLIT2_FOLD" else 1, fold=True),
                          throughput=thr, fold=(sc_C, pooled), key=("fold", site, sc_C, pooled)))
    cases.append(Case("fold-SINGLE_FOLD-c64-sc64-unpooled-o40", 64, 40, SHAPES[0], "OUT", True,
                      declare("SINGLE_FOLD", "OUT", 64, 3, True, fold=True), fold=(64, False), key=("fold", "c64")))
    # -- zero-weight kernels
    for C, k, site, entry in ((64, 3, "WZ_SINGLE", "plain"), (128, 3, "WZ_SINGLE", "fused"), (256, 3, "WZ_CHUNKS", "plain"),
                              (192, 3, "WZ_CHUNKS", "fused"), (128, 1, "WZ_CHUNKS", "fused"), (64, 3, "WZ_SINGLE", "dot")):
        prof = "PLAIN" if entry == "plain" else "RUNTIME"
        cases.append(Case(f"wz-k{k}-c{C}-{entry}", C, 40, SHAPES[1] if k == 3 else SHAPES_1X1[1], prof, entry == "fused", declare(
            site, prof, C, k, False, wz=True), k=k, wz=True, entry=entry, key=("wz", site, entry)))
    # -- shape-generic kernels: 5x5, dilation 2, each with and without zero weights
    for (name, k, dil, shape), wz, entry in itertools.product(
            (("k5", 5, 1, (2, 9, 7, 1, 2)), ("dil2", 3, 2, (3, 14, 13, 1, 2))), (False, True), ("plain", "fused")):
        prof = "PLAIN" if entry == "plain" else "RUNTIME"
        cases.append(Case(f"generic-{name}-{'wz' if wz else 'dense'}-{entry}", 64, 40, shape, prof, entry == "fused", declare(
            "GENERIC_WZ" if wz else "GENERIC", prof, 64, k, False, wz=wz, tiled=False), k=k, dil=dil, wz=wz, entry=entry,
            key=("generic", name, wz, entry)))
    return cases


CASES = build_table()


# ------------------------------------------------------------------------------------------------ inputs and the oracle
@functools.lru_cache(maxsize=None)
def layer(N, C, H, W, O, k, stride, pad, dil, nn, wz):
    """Input, weight, the oracle's dot and the layer's alpha (channel 3: 0), computed once and shared read-only."""
    s = gen.seed_of("routes", N, C, H, W, O, k, stride, pad, dil, nn, wz)
    x = gen.activation("relu" if nn else "sparse", s, (N, C, H, W))
    w = gen.conv_weight("withzeros" if wz else "kaiming", s + 1, (O, C, k, k))
    _, dot = oracle.binary_conv2d_int(x, w, None, None, stride, pad, dil)
    alpha = oracle.pack_weight(w)[2][:O].copy()
    if O > 3:
        alpha[3] = 0.0                   # what an all-zero weight channel has (set here: zero weights take another kernel)
    for a in (x, w, dot, alpha):
        a.setflags(write=False)
    return x, w, dot, alpha


def layer_of(c: Case):
    N, H, W, s, p = c.shape
    return layer(N, c.C, H, W, c.O, c.k, s, p, c.dil, c.nn, c.wz)


def affine(O, seed):
    """BatchNorm-like constants with every special channel of test_integer_sign_thresholds_give_the_float_epilogue_bits."""
    a = ((0.5 + gen.uniform(seed, (O,))) * np.where(np.arange(O) % 3 == 0, -1, 1)).astype(np.float32)
    b = (2.0 * gen.normal(seed + 1, (O,))).astype(np.float32)
    for o, (va, vb) in {1: (0.0, 0.25), 2: (0.0, -0.25), 5: (1e30, 1.0), 6: (1e-30, -1e-38), 7: (None, np.nan),
                        8: (1.0, 0.0)}.items():          # constant +, constant -, huge, denormal products, NaN, T at dot = 0
        if o < O:
            if va is not None:
                a[o] = va
            b[o] = vb
    return a, b


def or_pool(x):
    """Ceil-mode 2 x 2 "any > 0" of a non-negative tensor: the sign of AvgPool2d(2, ceil_mode=True) the kernel ORs."""
    N, C, H, W = x.shape
    p = np.zeros((N, C, 2 * ((H + 1) // 2), 2 * ((W + 1) // 2)), bool)
    p[:, :, :H, :W] = x > 0
    return (p[:, :, 0::2, 0::2] | p[:, :, 0::2, 1::2] | p[:, :, 1::2, 0::2] | p[:, :, 1::2, 1::2]).astype(np.float32)


def epilogue_of(c: Case, dot, alpha):
    """(keyword arguments of hipops.bconv2d_fused as numpy arrays, expected fp32 or None, expected pack value or None)."""
    O = c.O
    N, _, ho, wo = dot.shape
    s = gen.seed_of("routes-epi", c.id)
    a, b = affine(O, s)
    p = c.profile
    if c.fold is not None:
        sc_C, pooled = c.fold
        xs = gen.activation("relu", s + 10, (N, sc_C, ho, wo) if pooled else (N, sc_C, 2 * ho - 1, 2 * wo - 1))
        ws = gen.conv_weight("kaiming", s + 11, (O, sc_C, 1, 1))
        a_s, b_s = affine(O, s + 12)
        _, dot1 = oracle.binary_conv2d_int(xs if pooled else or_pool(xs), ws)
        alpha_s = oracle.pack_weight(ws)[2][:O]
        res = oracle.fused_epilogue(dot1, alpha_s, None, None, a_s, b_s, None, None, False)      # the EP_DS formula
        y = oracle.fused_epilogue(dot, alpha, None, None, a, b, res, None, True)
        return dict(bn_scale=a, bn_shift=b, relu=True, out_f32=True, out_packed=True, shortcut=(xs, ws, a_s, b_s)), y, y
    if p == "PLAIN":
        bias, sc = (0.1 * gen.normal(s + 3, (O,))).astype(np.float32), (0.5 + gen.uniform(s + 4, (O,))).astype(np.float32)
        return dict(bias=bias, post_scale=sc), oracle.fused_epilogue(dot, alpha, bias, sc), None
    if p == "DS":
        return dict(bn_scale=a, bn_shift=b), oracle.fused_epilogue(dot, alpha, None, None, a, b), None
    if p == "RUNTIME":
        bias = (0.1 * gen.normal(s + 3, (O,))).astype(np.float32)
        res, pre = gen.normal(s + 2, dot.shape), (0.25 * gen.uniform(s + 5, (O,))).astype(np.float32)
        y = oracle.fused_epilogue(dot, alpha, bias, None, a, b, res, pre, False)
        return dict(bias=bias, bn_scale=a, bn_shift=b, residual=res, prelu=pre, out_f32=True, out_packed=True), y, y
    if p in ("MID", "MIDT"):
        pv = oracle.fused_epilogue(dot, alpha, None, None, a, b, None, None, True)
        return dict(bn_scale=a, bn_shift=b, relu=True, out_f32=False, out_packed=True), None, pv
    if p in ("OUT", "OUTP", "LAST"):
        res = gen.normal(s + 2, dot.shape)
        y = oracle.fused_epilogue(dot, alpha, None, None, a, b, res, None, True)
        return (dict(bn_scale=a, bn_shift=b, residual=res, relu=True, out_f32=p != "OUTP", out_packed=p != "LAST"),
                y if p != "OUTP" else None, y if p != "LAST" else None)
    assert p in ("HB", "HB3")
    c_off, c_tot = 3, O + 8                                    # the convolution owns a slice of a wider tensor
    canvas = gen.normal(s + 6, (N, c_tot, ho, wo))
    res = gen.normal(s + 2, canvas.shape)
    hb = p == "HB"
    y, pv = oracle.fused_epilogue2(dot, alpha, None, None, None, None, res, None, False, res_late=True, pack_pre=True,
                                   pack_a=a if hb else None, pack_b=b if hb else None, pack_relu=hb, out=canvas.copy(),
                                   c_off=c_off)
    kw = dict(residual=res, residual_after_act=True, pack_before_residual=True, out=canvas, out_c_offset=c_off,
              out_f32=True, out_packed=hb)
    if hb:
        kw.update(pack_scale=a, pack_shift=b, pack_relu=True)
    return kw, y, pv if hb else None


# ------------------------------------------------------------------------------------------------------------ the device
def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)          # (a copy: the shared inputs are read-only)


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def same_f32(got, want):
    """Bit patterns equal; a NaN matches any NaN."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    if got.shape != want.shape:
        return False
    eq = got.view(np.uint32) == want.view(np.uint32)
    return bool((eq | (np.isnan(got) & np.isnan(want))).all())


def packed_input(x, nn):
    act = hipops.pack_act(dev(x))
    if nn:
        assert not bool(act.M.any())
        act.nonneg = True
    return act


def packed_weight(w, alpha, wz):
    pw = hipops.pack_weight(dev(w))
    assert pw.has_zero == wz
    O = w.shape[0]
    assert same_f32(np.where(np.arange(O) == 3, 0, pw.alpha[:O].cpu().numpy()), alpha)     # the device's alpha IS the oracle's
    pw.alpha[:O] = dev(alpha)
    return pw


def on_device(kw):
    out = {}
    for k, v in kw.items():
        if k == "shortcut":
            xs, ws, a_s, b_s = v
            sw = hipops.pack_weight(dev(ws))
            assert not sw.has_zero
            out[k] = (packed_input(xs, True), sw, dev(a_s), dev(b_s))
        else:
            out[k] = dev(v) if isinstance(v, np.ndarray) else v
    return out


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_route_against_the_oracle(case):
    x, w, dot, alpha = layer_of(case)
    N, H, W, stride, pad = case.shape
    O = case.O
    act, pw = packed_input(x, case.nn), packed_weight(w, alpha, case.wz)
    geo = dict(stride=stride, padding=pad, dilation=case.dil)
    kw_np, y_ref, pv_ref = epilogue_of(case, dot, alpha)
    if case.entry == "dot":
        r = hipops.bconv2d_route(act, pw, fused=False, raw_dot=True, **geo)
        assert tuple(sorted((k, v) for k, v in r.items() if k != "waves")) == case.route
        got = hipops.bconv2d(act, pw, raw_dot=True, **geo)
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), dot)
        return
    kw = on_device(kw_np)
    if case.entry == "plain":
        r = hipops.bconv2d_route(act, pw, fused=False, **kw, **geo)
    else:
        if case.profile == "MIDT":
            kw["sign_thresholds"] = hipops.sign_thresholds(pw, kw["bn_scale"], kw["bn_shift"])
        geo["throughput"] = case.throughput
        r = hipops.bconv2d_route(act, pw, **kw, **geo)
    waves = r.pop("waves")
    assert tuple(sorted(r.items())) == case.route, (sorted(r.items()), case.route)
    tiles = (dot.shape[0] * dot.shape[2] * dot.shape[3] + 63) // 64
    if r["tiled"]:
        nb = blocks_of(O, bool(kw.get("out_packed")))
        assert waves == 8 * ((tiles + 7) // 8) * ((nb + r["blocks_per_wave"] - 1) // r["blocks_per_wave"]) * r["pieces"]
    before = native.launch_count()
    if case.entry == "plain":
        y, pk = hipops.bconv2d(act, pw, **kw, **geo), None
    else:
        y, pk = hipops.bconv2d_fused(act, pw, **kw, **geo)
    assert native.launch_count() == before + 1
    if y_ref is None:
        assert y is None
    else:
        assert same_f32(y.cpu().numpy(), y_ref)          # (a channel slice: the whole canvas, the untouched part included)
    if pv_ref is None:
        assert pk is None
    else:
        P, M = oracle.pack_act(pv_ref)
        assert np.array_equal(u64(pk.P), P) and np.array_equal(u64(pk.M), M)
        if pk.nonneg:
            assert not M.any()
        assert pk.nonneg == (case.profile in ("MID", "MIDT", "OUT", "OUTP", "HB"))


MIDT_SHAPES = sorted({(c.C, c.O): c for c in CASES if c.profile == "MIDT"}.values(), key=lambda c: c.id)


@pytest.mark.parametrize("case", MIDT_SHAPES, ids=lambda c: f"c{c.C}-o{c.O}")
def test_sign_threshold_table_is_the_oracle_predicate_on_every_dot(case):
    """bnn_hip_sign_thresholds_f32 for the EP_MIDT cases above: `(dot >= T) XOR flip` against the oracle's float
    BN -> ReLU -> sign for EVERY integer dot in [-9C, 9C] — the whole range csrc/thresholds.hip bisects over (kmax = C * 9)
    — and every channel; pad channels "never"."""
    _, w, _, alpha = layer_of(case)
    C, O = case.C, case.O
    a, b = affine(O, gen.seed_of("routes-epi", case.id))
    pw = packed_weight(w, alpha, False)
    thr = hipops.sign_thresholds(pw, dev(a), dev(b)).cpu().numpy()
    o_pad = (O + 31) // 32 * 32
    assert thr.shape == (o_pad, 4)
    dots = np.arange(-9 * C, 9 * C + 1, dtype=np.int32)
    pv = oracle.fused_epilogue(np.ascontiguousarray(np.broadcast_to(dots, (1, O, 1, dots.size))), alpha, None, None, a, b,
                               None, None, True)
    with np.errstate(invalid="ignore"):
        want = (pv[0, :, 0, :] > 0).T                                  # [dot, channel]: sign(relu(bn(alpha * dot))) == +1
    T = thr[:, 0].astype(np.int64)
    ch = np.arange(o_pad)
    flip = (thr[ch - ch % 32, 1].astype(np.int64) & 0xFFFFFFFF) >> (ch % 32) & 1
    got = (dots[:, None].astype(np.int64) >= T[None, :]) ^ flip[None, :].astype(bool)
    assert not got[:, O:].any() and (T[O:] == 0x40000000).all() and not flip[O:].any()                  # pad channels
    assert np.array_equal(got[:, :O], want)
    assert want.any() and not want.all()


# ----------------------------------------------------------------------------------------------------------- completeness
def sites_of_the_table():
    return {dict(c.route)["site"] for c in CASES}


def test_the_table_reaches_every_compiled_launch_statement():
    assert set(EXCLUDED_SITES) <= set(range(native.ROUTE_SITES))
    assert sites_of_the_table() == set(range(native.ROUTE_SITES)) - set(EXCLUDED_SITES)


def test_the_table_holds_the_whole_product():
    keys = {c.key for c in CASES}
    assert len({c.id for c in CASES}) == len(CASES)
    missing = [k for k in itertools.product(("class",), (64, 128, 192, 256), PROFILES_3X3, (False, True)) if k not in keys]
    missing += [k for k in itertools.product(("1x1",), (512, 256, 128, 64, 192), PROFILES_1X1) if k not in keys]
    missing += [k for k in itertools.product(("split",), ("latency", "throughput", "unsplit"), SPLIT_PROFILES, (False, True))
                if k not in keys]
    missing += [k for k in itertools.product(("fold",), ("SINGLE_FOLD", "MULTI4_SPLIT2_FOLD", "CHUNKS_FOLD"), (64, 128, 256),
                                             (True, False)) if k not in keys]
    missing += [k for k in itertools.product(("fold",), ("MULTI4_FOLD",), (64, 128, 256), (True,)) if k not in keys]
    missing += [k for k in (("fold", "MULTI4_FOLD", 64, False), ("class", 512)) if k not in keys]
    missing += [k for k in itertools.product(("wz",), ("WZ_SINGLE", "WZ_CHUNKS"), ("plain", "fused")) if k not in keys]
    missing += [k for k in itertools.product(("generic",), ("k5", "dil2"), (False, True), ("plain", "fused")) if k not in keys]
    assert not missing, missing
    # per chunk class: a stride-2 and a pad-0 case, a ragged and a full 32-channel block, the all-zero tail block of pack mode
    for C in (64, 128, 192, 256):
        mine = [c for c in CASES if c.key[:2] == ("class", C)]
        assert any(c.shape[3] == 2 for c in mine) and any(c.shape[4] == 0 for c in mine), C
        assert {c.O for c in mine} == set(OUT_CHANNELS), C
        assert any(c.profile in PACKS and c.O % 64 in range(1, 33) for c in mine), C
    # every profile meets every special BatchNorm channel (index 8 is the last) in at least one case
    for prof in PROFILES_3X3:
        assert any(c.O > 8 for c in CASES if c.profile == prof), prof

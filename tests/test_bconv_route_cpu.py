"""The launch ladder of csrc/bconv.hip, asked without a GPU: bnn_hip_bconv2d_route / bnn_hip_bconv2d_dot_route run the
statements of launch_bconv() with the launch itself skipped, so the edges of every threshold and every profile mask can be
pinned from both sides here.  Descriptors and epilogues only: pointers are never read (any aligned non-null value)."""
import ctypes
import itertools

import pytest

from bnn_amd import native

PTR = 0x1000            # "given": only compared with NULL and checked for alignment
NN, THROUGHPUT = native.FLAG_ACT_NONNEG, native.FLAG_THROUGHPUT
WZ, GENERIC = native.FLAG_WEIGHT_ZEROS, native.FLAG_FORCE_GENERIC
EP, SITE = native.ROUTE_PROFILES, native.SITE
# the constants of csrc/bconv.hip the edges below are derived from
GSPLIT_MAX_WAVES, GSPLIT4_MAX_WAVES, THROUGHPUT_SPLIT_BELOW, OBW = 16384, 8192, 2048, 2

RES_AFTER_ACT, PACK_BEFORE_RES, PACK_RELU = native.EPI_RES_AFTER_ACT, native.EPI_PACK_BEFORE_RES, native.EPI_PACK_RELU
BN = dict(bn_scale=PTR, bn_shift=PTR)
PLANES = dict(out_P=PTR, out_M=PTR)
PROFILE_FIELDS = {      # the epilogue that selects each compiled profile
    "PLAIN": dict(out_f32=PTR),
    "RUNTIME": dict(relu=1, out_f32=PTR),
    "MID": dict(**BN, relu=1, **PLANES),
    "MIDT": dict(**BN, relu=1, **PLANES, sign_thresholds=PTR),
    "OUT": dict(**BN, residual=PTR, relu=1, out_f32=PTR, **PLANES),
    "OUTP": dict(**BN, residual=PTR, relu=1, **PLANES),
    "LAST": dict(**BN, residual=PTR, relu=1, out_f32=PTR),
    "HB": dict(residual=PTR, flags=RES_AFTER_ACT | PACK_BEFORE_RES | PACK_RELU, pack_scale=PTR, pack_shift=PTR,
               out_f32=PTR, **PLANES),
    "HB3": dict(residual=PTR, flags=RES_AFTER_ACT | PACK_BEFORE_RES, out_f32=PTR),
    "DS": dict(**BN, out_f32=PTR),
}
PROFILES_3X3 = ("PLAIN", "RUNTIME", "MID", "MIDT", "OUT", "OUTP", "LAST", "HB", "HB3")


def epilogue(profile="PLAIN", **extra):
    e = native.Epilogue()
    e.alpha = PTR
    for k, v in {**PROFILE_FIELDS[profile], **extra}.items():
        setattr(e, k, v)
    return e


def desc(N, C, H, W, O, k=3, stride=1, pad=None, dil=1, flags=0):
    pad = (k // 2) * dil if pad is None else pad
    return native.ConvDesc(N, C, H, W, O, k, k, stride, stride, pad, pad, dil, dil, flags)


def query(d, e=None):
    r = native.ConvRoute()
    st = native.require().bnn_hip_bconv2d_route(ctypes.byref(d), None if e is None else ctypes.byref(e), ctypes.byref(r))
    return st, r


def route(d, e=None):
    st, r = query(d, e)
    assert st == 0, st
    assert r.reserved == 0
    return r


def row(tpx, extra=0):
    """H, W of a one-row image whose 3x3 / pad 1 (or 1x1) output has exactly ``8 * tpx`` pixel tiles of 64 (plus ``extra``
    pixels): tiles_per_xcd == tpx, or tpx + 1 with one more pixel."""
    return 1, 512 * tpx + extra


def oblocks(O, packed):
    return 2 * ((O + 63) // 64) if packed else (O + 31) // 32


def test_the_query_is_a_host_function_with_the_launch_validator():
    lib = native.require()
    d = desc(2, 64, 9, 7, 40)
    r = native.ConvRoute()
    assert lib.bnn_hip_bconv2d_route(None, None, ctypes.byref(r)) == -1
    assert lib.bnn_hip_bconv2d_route(ctypes.byref(d), None, None) == -1
    assert lib.bnn_hip_bconv2d_dot_route(ctypes.byref(d), None) == -1
    before = native.launch_count()
    assert query(d)[0] == 0 and native.launch_count() == before          # nothing launched, nothing counted
    # what bnn_hip_bconv2d_fused refuses, the query refuses with the same status
    assert query(desc(0, 64, 9, 7, 40))[0] == -1
    assert query(desc(2, 64, 2, 2, 40, pad=0))[0] == -1                   # empty output
    assert query(desc(1 << 14, 64, 1 << 10, 1 << 10, 32))[0] == -4        # beyond one launch's addressing
    e = epilogue(); e.alpha = None
    assert query(d, e)[0] == -1                                           # no alpha
    e = epilogue(); e.out_f32 = None
    assert query(d, e)[0] == -1                                           # no output at all
    assert query(d, epilogue("MID", bn_shift=None))[0] == -1              # BatchNorm: both or neither
    assert query(d, epilogue("MID", out_M=None))[0] == -1                 # planes: both or neither
    assert query(d, epilogue("MID", out_P=PTR + 4))[0] == -1              # planes: 8-byte aligned
    assert query(d, epilogue("MIDT", sign_thresholds=PTR + 2))[0] == -1   # table: 4-byte aligned
    assert query(d, epilogue("HB3", out_c_offset=8, out_c_total=40))[0] == -1     # the slice does not fit
    assert query(d, epilogue("HB3", out_c_offset=8, out_c_total=48))[0] == 0
    assert query(d, epilogue("OUT", sc_wbits=PTR))[0] == -1               # shortcut fields: all or none


def test_waves_are_the_grid_of_the_launch():
    """waves == 8 * ceil(tiles / 8) * blocks [* pieces], blocks counting the all-zero tail word of pack mode."""
    lib = native.require()
    shapes = [(2, 9, 7, 1, 1), (3, 14, 13, 1, 1), (2, 12, 10, 2, 1), (2, 9, 9, 1, 0), (5, 31, 29, 1, 1), (1, 1, 1, 1, 1)]
    seen_tail = False
    for (N, H, W, s, p), C, O, prof, flags in itertools.product(
            shapes, (64, 128, 192, 256, 512), (5, 32, 40, 64, 70, 96, 130), PROFILES_3X3, (0, NN, THROUGHPUT)):
        d = desc(N, C, H, W, O, 3, s, p, flags=flags)
        r = route(d, epilogue(prof))
        ho, wo = (H + 2 * p - 3) // s + 1, (W + 2 * p - 3) // s + 1
        tiles = (N * ho * wo + 63) // 64
        packed = "out_P" in PROFILE_FIELDS[prof]
        nb = oblocks(O, packed)
        seen_tail |= packed and nb > (O + 31) // 32
        assert r.blocks_per_wave in (1, OBW) and r.pieces in (1, 2, 4)
        assert r.waves == 8 * ((tiles + 7) // 8) * ((nb + r.blocks_per_wave - 1) // r.blocks_per_wave) * r.pieces, (d.C, O, prof)
        L = native.WLayout()
        assert lib.bnn_hip_weight_layout(O, C, 3, 3, ctypes.byref(L)) == 0
        assert (r.tiled, r.kh, r.kw, r.cwc, r.nchunk) == (1, 3, 3, L.cwc, L.nchunk)
        assert r.multi == (L.nchunk > 1) and r.nonneg == (flags == NN) and r.weight_zeros == 0 and r.shortcut_fold == 0
    assert seen_tail
    # the shape-generic kernel: a 2-D grid of pixel tiles x blocks
    r = route(desc(2, 64, 9, 7, 70, 5), epilogue("MID"))
    assert r.tiled == 0 and r.waves == ((2 * 9 * 7 + 63) // 64) * oblocks(70, True)


@pytest.mark.parametrize("nn", [0, NN], ids=["two-plane", "nonneg"])
def test_split_or_unsplit_in_latency_mode(nn):
    """One batch at a time: a multi-chunk 128-channel-chunk layer is split while the UNSPLIT grid has at most
    BNN_GSPLIT_MAX_WAVES waves."""
    for prof, O in (("OUT", 256), ("LAST", 64), ("MID", 512), ("RUNTIME", 32)):
        nb = oblocks(O, "out_P" in PROFILE_FIELDS[prof])
        assert GSPLIT_MAX_WAVES % (8 * nb) == 0
        tpx = GSPLIT_MAX_WAVES // (8 * nb)
        r = route(desc(1, 256, *row(tpx), O, flags=nn), epilogue(prof))
        assert (r.site, r.pieces, r.waves, r.multi) == (SITE["MULTI4_SPLIT2"], 2, 2 * GSPLIT_MAX_WAVES, 1), prof
        r = route(desc(1, 256, *row(tpx, 1), O, flags=nn), epilogue(prof))
        assert (r.site, r.pieces, r.waves, r.multi) == (SITE["MULTI4"], 1, GSPLIT_MAX_WAVES + 8 * nb, 1), prof
        assert r.nonneg == bool(nn) and r.profile == EP[prof]


@pytest.mark.parametrize("nn", [0, NN], ids=["two-plane", "nonneg"])
def test_split_or_unsplit_in_throughput_mode(nn):
    """Several batches in flight: only launches of FEWER than 2048 unsplit waves keep the split, and never four pieces."""
    for prof, O in (("OUT", 256), ("LAST", 32), ("MID", 64), ("MIDT", 256), ("PLAIN", 32)):
        nb = oblocks(O, "out_P" in PROFILE_FIELDS[prof])
        tpx = THROUGHPUT_SPLIT_BELOW // (8 * nb)
        below = route(desc(1, 256, *row(tpx - 1), O, flags=nn | THROUGHPUT), epilogue(prof))
        assert below.waves == 2 * (THROUGHPUT_SPLIT_BELOW - 8 * nb) and (below.site, below.pieces) == (SITE["MULTI4_SPLIT2"], 2)
        at = route(desc(1, 256, *row(tpx), O, flags=nn | THROUGHPUT), epilogue(prof))
        assert at.waves == THROUGHPUT_SPLIT_BELOW and (at.site, at.pieces) == (SITE["MULTI4"], 1), prof
    # one block (8 waves per eighth of the tiles): 2040 is the largest grid below 2048
    assert route(desc(1, 256, *row(255), 32, flags=nn | THROUGHPUT), epilogue("LAST")).waves == 2 * 2040
    # the same grids in latency mode stay split
    assert route(desc(1, 256, *row(32), 256, flags=nn), epilogue("OUT")).pieces == 2


@pytest.mark.parametrize("prof", ["MID", "MIDT"])
def test_four_pieces_or_two(prof):
    """conv1-type layers, one batch at a time: four pieces while TWO pieces give at most BNN_GSPLIT4_MAX_WAVES waves."""
    for O, nn in itertools.product((64, 256), (0, NN)):
        nb = oblocks(O, True)
        tpx = GSPLIT4_MAX_WAVES // 2 // (8 * nb)
        r = route(desc(1, 256, *row(tpx), O, flags=nn), epilogue(prof))
        assert (r.site, r.pieces, r.waves) == (SITE["MULTI4_SPLIT4"], 4, 2 * GSPLIT4_MAX_WAVES)
        r = route(desc(1, 256, *row(tpx, 1), O, flags=nn), epilogue(prof))
        assert (r.site, r.pieces, r.waves) == (SITE["MULTI4_SPLIT2"], 2, GSPLIT4_MAX_WAVES + 16 * nb)
        # throughput mode never takes four
        r = route(desc(1, 256, *row(1), O, flags=nn | THROUGHPUT), epilogue(prof))
        assert (r.site, r.pieces) == (SITE["MULTI4_SPLIT2"], 2)
    # the smallest grid there is: every other profile keeps two pieces
    for other in ("OUT", "OUTP", "LAST", "PLAIN", "RUNTIME", "HB", "HB3"):
        r = route(desc(1, 256, 1, 1, 64, flags=NN), epilogue(other))
        assert (r.site, r.pieces, r.profile) == (SITE["MULTI4_SPLIT2"], 2, EP[other]), other


def test_blocks_per_wave_of_the_plain_single_chunk_kernel():
    for C, nn in itertools.product((64, 128), (0, NN)):
        for O, site, bpw, groups in ((32, "SINGLE", 1, 1), (5, "SINGLE", 1, 1), (64, "SINGLE_OBW", OBW, 1),
                                     (96, "SINGLE_OBW", OBW, 2), (33, "SINGLE_OBW", OBW, 1)):
            r = route(desc(2, C, 9, 7, O, flags=nn))              # e == NULL: bnn_hip_bconv2d
            assert (r.site, r.blocks_per_wave, r.waves, r.profile) == (SITE[site], bpw, 8 * groups, EP["PLAIN"]), (C, O)
            assert (r.multi, r.pieces, r.nonneg) == (0, 1, bool(nn))
            r2 = route(desc(2, C, 9, 7, O, flags=nn), epilogue("PLAIN", bias=PTR, post_scale=PTR))
            assert r2.as_dict() == r.as_dict()                    # bias and post-scale stay in the drop-in kernel
        # any fused epilogue, and every multi-chunk layer: one block per wave
        assert route(desc(2, C, 9, 7, 96, flags=nn), epilogue("RUNTIME")).blocks_per_wave == 1
    assert route(desc(2, 256, 9, 7, 96)).blocks_per_wave == 1 and route(desc(2, 192, 9, 7, 96)).blocks_per_wave == 1


@pytest.mark.parametrize("C,cwc,nchunk", [(64, 2, 1), (128, 4, 1), (192, 2, 3), (256, 4, 2), (512, 4, 4), (70, 4, 1),
                                          (320, 2, 5)])
def test_profile_selection_3x3(C, cwc, nchunk):
    single = nchunk == 1
    for prof, nn in itertools.product(PROFILES_3X3, (0, NN)):
        r = route(desc(2, C, 9, 7, 40, flags=nn), epilogue(prof))
        assert (r.profile, r.nonneg, r.cwc, r.nchunk, r.multi) == (EP[prof], bool(nn), cwc, nchunk, not single), prof
        if single:
            assert r.site == SITE["SINGLE_OBW" if prof == "PLAIN" else "SINGLE"] and r.pieces == 1   # (O = 40: two blocks)
        elif cwc == 4:
            assert r.site == (SITE["MULTI4_SPLIT4"] if prof in ("MID", "MIDT") else SITE["MULTI4_SPLIT2"])
        else:
            assert r.site == SITE["CHUNKS"] and r.pieces == 1
    # a profile's mask plus anything else is the run-time epilogue
    for prof in PROFILES_3X3[2:]:
        for extra in (dict(bias=PTR), dict(post_scale=PTR), dict(prelu=PTR)):
            assert route(desc(2, C, 9, 7, 40), epilogue(prof, **extra)).profile == EP["RUNTIME"], (prof, extra)
    assert route(desc(2, C, 9, 7, 40), epilogue("PLAIN", prelu=PTR)).profile == EP["RUNTIME"]
    assert route(desc(2, C, 9, 7, 40), epilogue("DS")).profile == EP["RUNTIME"]        # the 1x1 mask on a 3x3 layer
    assert route(desc(2, C, 9, 7, 40), epilogue("PLAIN", sign_thresholds=PTR)).profile == EP["PLAIN"]   # table ignored
    assert route(desc(2, C, 9, 7, 40), epilogue("HB", flags=RES_AFTER_ACT | PACK_RELU)).profile == EP["RUNTIME"]
    # the raw integer dot is a run-time switch
    r = native.ConvRoute()
    d = desc(2, C, 9, 7, 40, flags=NN)
    assert native.require().bnn_hip_bconv2d_dot_route(ctypes.byref(d), ctypes.byref(r)) == 0
    assert (r.profile, r.nonneg, r.blocks_per_wave, r.tiled) == (EP["RUNTIME"], 1, 1, 1)
    assert r.waves == 8 * 2 * (1 if single or cwc == 2 else 2)


@pytest.mark.parametrize("C,cwc", [(512, 16), (256, 8), (128, 4), (64, 2), (192, 2), (1024, 16), (768, 8), (384, 4)])
def test_profile_selection_1x1(C, cwc):
    for prof, want in (("PLAIN", "PLAIN"), ("RUNTIME", "RUNTIME"), ("DS", "DS"), ("MID", "RUNTIME"), ("MIDT", "RUNTIME"),
                       ("OUT", "RUNTIME"), ("OUTP", "RUNTIME"), ("LAST", "RUNTIME"), ("HB", "RUNTIME"), ("HB3", "RUNTIME")):
        for flags in (0, NN, NN | THROUGHPUT):
            r = route(desc(2, C, 9, 7, 40, 1, flags=flags), epilogue(prof))
            assert (r.tiled, r.kh, r.kw, r.cwc, r.nchunk) == (1, 1, 1, cwc, C // (32 * cwc))
            assert (r.profile, r.nonneg, r.site, r.pieces, r.blocks_per_wave) == (EP[want], 0, SITE["CHUNKS"], 1, 1)
            assert r.multi == 1                               # the 1x1 kernels walk their chunks, also a single one
    assert route(desc(2, C, 9, 7, 40, 1), epilogue("DS", bias=PTR)).profile == EP["RUNTIME"]


def test_zero_weight_kernels_ignore_profiles_and_promises():
    for C, k, site in ((64, 3, "WZ_SINGLE"), (128, 3, "WZ_SINGLE"), (256, 3, "WZ_CHUNKS"), (192, 3, "WZ_CHUNKS"),
                       (64, 1, "WZ_CHUNKS"), (512, 1, "WZ_CHUNKS")):
        for prof in PROFILES_3X3 + ("DS",):
            r = route(desc(2, C, 9, 7, 96, k, flags=WZ | NN), epilogue(prof))
            want = "PLAIN" if prof == "PLAIN" else "RUNTIME"
            assert (r.site, r.profile, r.weight_zeros, r.nonneg, r.pieces, r.blocks_per_wave) == \
                (SITE[site], EP[want], 1, 0, 1, 1), (C, k, prof)
            assert r.multi == (site == "WZ_CHUNKS")
    d = desc(2, 64, 9, 7, 40, flags=WZ | NN)
    assert query(d, epilogue("OUT", residual=None, sc_P=PTR, sc_wbits=PTR, sc_alpha=PTR, sc_bn_scale=PTR,
                             sc_bn_shift=PTR, sc_C=64))[0] == -2


def test_generic_fallbacks():
    for d in (desc(2, 64, 12, 10, 40, 3, dil=2), desc(2, 64, 9, 7, 40, flags=GENERIC), desc(2, 64, 9, 7, 40, 5),
              desc(2, 64, 4100, 4100, 16), desc(2, 64, 9, 7, 40, 1, flags=GENERIC), desc(2, 128, 9, 7, 40, 7)):
        for prof, flags in itertools.product(("PLAIN", "MID", "OUTP"), (0, NN, WZ)):
            d.flags = (d.flags & GENERIC) | flags
            r = route(d, epilogue(prof))
            assert (r.tiled, r.profile, r.nonneg, r.pieces, r.blocks_per_wave, r.multi) == (0, EP["RUNTIME"], 0, 1, 1, 0)
            assert r.weight_zeros == (flags == WZ) and r.site == SITE["GENERIC_WZ" if flags == WZ else "GENERIC"]
            assert (r.kh, r.kw) == (d.KH, d.KW)
    assert route(desc(2, 64, 2040, 4096, 16), epilogue("MID")).tiled == 1      # just inside the 24-bit index factors
    # a kernel size without a tiled kernel; 1 x 3 is neither
    d = native.ConvDesc(2, 64, 9, 7, 40, 1, 3, 1, 1, 0, 1, 1, 1, 0)
    assert route(d).tiled == 0


def fold(sc_C, **extra):
    return epilogue("OUT", **{**dict(residual=None, sc_P=PTR, sc_wbits=PTR, sc_alpha=PTR, sc_bn_scale=PTR,
                                     sc_bn_shift=PTR, sc_C=sc_C), **extra})


def test_folded_shortcut_sites_and_refusals():
    for sc_C in (64, 128, 256):
        r = route(desc(2, 128, 9, 7, 40, flags=NN), fold(sc_C))
        assert (r.site, r.shortcut_fold, r.profile, r.nonneg, r.pieces) == (SITE["SINGLE_FOLD"], 1, EP["OUT"], 1, 1)
        assert route(desc(2, 64, 9, 7, 40, flags=NN), fold(sc_C)).site == SITE["SINGLE_FOLD"]
        r = route(desc(2, 256, 9, 7, 40, flags=NN), fold(sc_C))
        assert (r.site, r.shortcut_fold, r.pieces) == (SITE["MULTI4_SPLIT2_FOLD"], 1, 2)
        r = route(desc(1, 256, *row(32), 256, flags=NN | THROUGHPUT), fold(sc_C))
        assert (r.site, r.shortcut_fold, r.pieces, r.waves) == (SITE["MULTI4_FOLD"], 1, 1, 2048)
        r = route(desc(1, 256, *row(GSPLIT_MAX_WAVES // 64, 1), 256, flags=NN), fold(sc_C))
        assert (r.site, r.pieces) == (SITE["MULTI4_FOLD"], 1)
        r = route(desc(2, 192, 9, 7, 40, flags=NN), fold(sc_C))
        assert (r.site, r.shortcut_fold, r.pieces, r.cwc, r.nchunk) == (SITE["CHUNKS_FOLD"], 1, 1, 2, 3)
    # un-pooled shortcut planes: (H << 16) | W with ceil(H / 2) == Ho, ceil(W / 2) == Wo
    assert route(desc(2, 128, 9, 7, 40, flags=NN), fold(64, sc_in_hw=(17 << 16) | 13)).site == SITE["SINGLE_FOLD"]
    assert query(desc(2, 128, 9, 7, 40, flags=NN), fold(64, sc_in_hw=(17 << 16) | 12))[0] == -1
    # where ds_fold_applies() says no, the launch refuses — and so does the query
    lib = native.require()
    for d, sc_C in ((desc(2, 128, 9, 7, 40), 64),                          # two-plane activations
                    (desc(2, 128, 9, 7, 40, flags=NN), 96),                # channel count
                    (desc(2, 128, 9, 7, 40, flags=NN | WZ), 64),
                    (desc(2, 128, 9, 7, 40, flags=NN | GENERIC), 64),
                    (desc(2, 128, 9, 7, 40, 1, flags=NN), 64),             # a 1x1 layer
                    (desc(2, 128, 12, 10, 40, dil=2, flags=NN), 64)):
        assert lib.bnn_hip_shortcut_fold_supported(ctypes.byref(d), sc_C) == 0
        assert query(d, fold(sc_C))[0] == -2
    for extra in (dict(out_f32=None), dict(out_P=None, out_M=None), dict(relu=0), dict(bias=PTR)):   # not the conv2-type epilogue
        assert query(desc(2, 128, 9, 7, 40, flags=NN), fold(64, **extra))[0] == -2, extra
    assert query(desc(2, 128, 9, 7, 40, flags=NN), fold(64, residual=PTR))[0] == -1


def test_python_constants_are_the_headers():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "bnn_hip.h")).read()
    sites = dict(re.findall(r"BNN_HIP_SITE_([A-Z0-9_]+) = (\d+)", text))
    assert {k: int(v) for k, v in sites.items()} == native.SITE
    assert int(re.search(r"BNN_HIP_ROUTE_SITES = (\d+)", text).group(1)) == native.ROUTE_SITES == len(native.SITE)
    profiles = dict(re.findall(r"BNN_HIP_ROUTE_EP_([A-Z0-9]+) = (\d+)", text))
    assert {k: int(v) for k, v in profiles.items()} == native.ROUTE_PROFILES

"""The folded-shortcut form of the int8 matrix-core convolution (csrc/bconv_mfma.hip, DS) without a GPU: the documented
byte layout of the shortcut's int8 pack as a numpy model, the host-only admission query at every edge — each condition
of the admission turns it to 0 alone — and the C-ABI bookkeeping."""
import ctypes
import os
import re

import numpy as np
import pytest

from bnn_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bnn_hip_shortcut_weight_i8_bytes", "bnn_hip_pack_shortcut_weight_i8", "bnn_hip_bconv2d_mfma_fold_supported",
       "bnn_hip_bconv2d_mfma_fold_fused")
PTR = 0x10000          # an aligned stand-in: the query never dereferences an operand
NONNEG = native.FLAG_ACT_NONNEG


# ------------------------------------------------------------------------------------------------- the layout, modelled
def shortcut_bits_model(sign):
    """bnn_hip_pack_weight_f32's wbits of a 1x1 weight [O, C] of 64 / 128 / 256 channels: one chunk, [o][C / 32] words,
    bit b of word cw = input channel 32 cw + b."""
    O, C = sign.shape
    L = native.weight_layout(O, C, 1, 1)
    assert (L.nchunk, L.cwc, L.cw32, L.taps) == (1, C // 32, C // 32, 1)
    wbits = np.zeros((O, C // 32), np.uint32)
    for o in range(O):
        for cw in range(C // 32):
            wbits[o, cw] = sum(1 << b for b in range(32) if sign[o, 32 * cw + b] > 0)
    return wbits


def shortcut_i8_from_bits(wbits, O, C):
    """What bnn_hip_pack_shortcut_weight_i8 computes, as its kernel indexes the words: bit ? +1 : -1 at
    sc_w8[o / 64][g][ct][lane][e]."""
    w8 = np.zeros((O // 64, C // 64, 4, 64, 16), np.int8)
    for ob, g, ct, lane, e in np.ndindex(*w8.shape):
        o, c = 64 * ob + 16 * ct + (lane & 15), 64 * g + 16 * (lane >> 4) + e
        w8[ob, g, ct, lane, e] = 1 if (int(wbits[o, c // 32]) >> (c % 32)) & 1 else -1
    return w8


def shortcut_i8_documented(sign):
    """sc_w8[o / 64][g][ct][lane][e] = W[64 (o / 64) + 16 ct + (lane & 15)][64 g + 16 (lane >> 4) + e]."""
    O, C = sign.shape
    s = sign.reshape(O // 64, 4, 16, C // 64, 4, 16)             # [ob][ct][row][g][lane >> 4][e]
    return np.ascontiguousarray(s.transpose(0, 3, 1, 4, 2, 5)).reshape(O // 64, C // 64, 4, 64, 16).astype(np.int8)


@pytest.mark.parametrize("O,C", [(64, 64), (128, 128), (64, 256)])
def test_shortcut_pack_layout_is_the_documented_one(O, C):
    rng = np.random.default_rng(O + C)
    sign = (2 * rng.integers(0, 2, size=(O, C)) - 1).astype(np.int8)
    got = shortcut_i8_from_bits(shortcut_bits_model(sign), O, C)
    assert np.array_equal(got, shortcut_i8_documented(sign))
    assert got.nbytes == native.require().bnn_hip_shortcut_weight_i8_bytes(O, C) == O * C


def test_the_parked_dot_fits_int16_and_the_zero_window_gives_zero():
    """|dot| <= sc_C <= 256 over a P plane of 0 / 1 and weights of +-1; an all-zero window gives dot 0 (no nz term)."""
    for C in (64, 128, 256):
        x = np.ones(C, np.int64)
        assert abs(int(x @ np.ones(C, np.int64))) <= 256 < 2 ** 15 and int(np.zeros(C, np.int64) @ -x) == 0


def test_shortcut_weight_i8_bytes_edges():
    lib = native.require()
    for C in (64, 128, 256):
        assert lib.bnn_hip_shortcut_weight_i8_bytes(512, C) == 512 * C
    for O, C in ((96, 64), (64, 96), (64, 32), (64, 192), (64, 512), (0, 64), (64, 0), (-64, 64), (64, -64)):
        assert lib.bnn_hip_shortcut_weight_i8_bytes(O, C) == 0
    before = native.launch_count()
    assert lib.bnn_hip_pack_shortcut_weight_i8(None, 64, 64, PTR, None) == native.ERR_INVALID_ARG
    assert lib.bnn_hip_pack_shortcut_weight_i8(PTR, 64, 64, None, None) == native.ERR_INVALID_ARG
    assert lib.bnn_hip_pack_shortcut_weight_i8(PTR + 4, 64, 64, PTR, None) == native.ERR_INVALID_ARG
    assert lib.bnn_hip_pack_shortcut_weight_i8(PTR, 64, 64, PTR + 8, None) == native.ERR_INVALID_ARG
    assert lib.bnn_hip_pack_shortcut_weight_i8(PTR, 96, 64, PTR, None) == native.ERR_UNSUPPORTED
    assert lib.bnn_hip_pack_shortcut_weight_i8(PTR, 64, 192, PTR, None) == native.ERR_UNSUPPORTED
    assert native.launch_count() == before
    # the 3x3 entry points keep refusing a 1x1
    assert lib.bnn_hip_weight_i8_bytes(64, 64, 1, 1) == 0
    assert lib.bnn_hip_pack_weight_i8(PTR, PTR, 64, 64, 1, 1, PTR, None) == native.ERR_UNSUPPORTED


# --------------------------------------------------------------------------------------------------- the admission query
def desc(N=2, C=128, H=4, W=4, O=128, k=3, stride=1, pad=1, dil=1, flags=NONNEG, stride_w=None):
    return native.ConvDesc(N, C, H, W, O, k, k, stride, stride if stride_w is None else stride_w, pad, pad, dil, dil, flags)


def epi(**kw):
    """The fold's epilogue: alpha, BatchNorm, ReLU -> fp32 + planes, the shortcut in sc_* (sc_wbits not needed)."""
    f = dict(alpha=PTR, bias=None, post_scale=None, bn_scale=PTR, bn_shift=PTR, residual=None, prelu=None, relu=1, flags=0,
             out_f32=PTR, out_P=PTR, out_M=PTR, pack_scale=None, pack_shift=None, out_c_offset=0, out_c_total=0,
             sign_thresholds=None, sc_P=PTR, sc_wbits=None, sc_alpha=PTR, sc_bn_scale=PTR, sc_bn_shift=PTR, sc_C=64,
             sc_in_hw=0)
    f.update(kw)
    return native.Epilogue(*f.values())


def supported(d, e):
    return native.require().bnn_hip_bconv2d_mfma_fold_supported(ctypes.byref(d), ctypes.byref(e))


def test_supported_shapes():
    for d in (desc(), desc(C=64, O=64), desc(C=128, O=192), desc(C=512, O=512, H=7, W=7, N=256),
              desc(C=128, O=128, H=28, W=28, N=256), desc(C=256, O=256, H=14, W=14, N=256), desc(N=3), desc(N=1, H=1, W=1),
              desc(flags=NONNEG | native.FLAG_THROUGHPUT)):
        for sc_C in (64, 128, 256):
            assert supported(d, epi(sc_C=sc_C)) == 1
            assert supported(d, epi(sc_C=sc_C, sc_wbits=PTR)) == 1
    # the un-pooled plane: (H << 16) | W of the block input, 2 Ho - 1 or 2 Ho
    assert supported(desc(), epi(sc_in_hw=(8 << 16) | 8)) == 1
    assert supported(desc(), epi(sc_in_hw=(7 << 16) | 7)) == 1
    assert supported(desc(), epi(out_c_total=128)) == 1
    # the plain query keeps refusing the same launch
    assert native.require().bnn_hip_bconv2d_mfma_supported(ctypes.byref(desc()), ctypes.byref(epi(sc_wbits=PTR))) == 0


@pytest.mark.parametrize("what,d,e", [
    # the dense rule
    ("C not a multiple of 64", desc(C=96), epi()),
    ("O not a multiple of 64", desc(O=96), epi()),
    ("5x5", desc(k=5, pad=2), epi()),
    ("1x1", desc(k=1, pad=0), epi()),
    ("dilation 2", desc(dil=2, pad=2), epi()),
    ("padding 0", desc(pad=0, H=6, W=6), epi()),
    ("stride 3", desc(stride=3), epi()),
    ("strides differ", desc(stride=1, stride_w=2), epi()),
    ("forced generic", desc(flags=NONNEG | native.FLAG_FORCE_GENERIC), epi()),
    ("PReLU", desc(), epi(prelu=PTR)),
    ("pack relu", desc(), epi(flags=native.EPI_PACK_RELU)),
    ("pack affine", desc(), epi(pack_scale=PTR, pack_shift=PTR)),
    ("channel window", desc(), epi(out_c_offset=3, out_c_total=160)),
    # kFlagsOut and nothing else
    ("no shortcut", desc(), epi(sc_P=None, sc_alpha=None, sc_bn_scale=None, sc_bn_shift=None)),
    ("no fp32 output", desc(), epi(out_f32=None)),
    ("no planes", desc(), epi(out_P=None, out_M=None)),
    ("no ReLU", desc(), epi(relu=0)),
    ("no BatchNorm", desc(), epi(bn_scale=None, bn_shift=None)),
    ("a bias", desc(), epi(bias=PTR)),
    ("a post scale", desc(), epi(post_scale=PTR)),
    ("a residual beside the shortcut", desc(), epi(residual=PTR)),
    # non-negative activations
    ("activations may be negative", desc(flags=0), epi()),
    # no zero weights
    ("zero weights", desc(flags=NONNEG | native.FLAG_WEIGHT_ZEROS), epi()),
    # sc_C
    ("sc_C 32", desc(), epi(sc_C=32)),
    ("sc_C 96", desc(), epi(sc_C=96)),
    ("sc_C 192", desc(), epi(sc_C=192)),
    ("sc_C 512", desc(), epi(sc_C=512)),
    ("sc_C 0", desc(), epi(sc_C=0)),
    # the LDS fit: the patch of 256 (or 128) pixels with a row above and below, plus the parked dots, within 80 KB
    ("row too wide for the LDS", desc(N=1, H=4, W=400), epi()),
    # operands
    ("shortcut constants missing", desc(), epi(sc_alpha=None)),
    ("misaligned shortcut plane", desc(), epi(sc_P=PTR + 4)),
    ("un-pooled plane of the wrong size", desc(), epi(sc_in_hw=(10 << 16) | 8)),
    ("misaligned fp32 output", desc(), epi(out_f32=PTR + 2)),
    ("misaligned planes", desc(), epi(out_P=PTR + 4)),
    ("no alpha", desc(), epi(alpha=None)),
    ("empty batch", desc(N=0), epi()),
], ids=lambda v: v if isinstance(v, str) else "")
def test_unsupported_edges(what, d, e):
    assert supported(desc(), epi()) == 1
    assert supported(d, e) == 0, what


def test_the_lds_edge():
    """The plain form fits a 64 KB patch; the fold needs the patch plus 36 KB of parked dots within 80 KB, so rows the plain
    form still takes are too wide for it."""
    lib = native.require()
    plain = native.Epilogue(PTR, None, None, PTR, PTR, PTR, None, 1, 0, PTR, PTR, PTR, None, None, 0, 0, None)
    widths = [w for w in range(100, 420, 20)]
    fold_ok = [w for w in widths if supported(desc(N=1, H=4, W=w), epi())]
    plain_ok = [w for w in widths if lib.bnn_hip_bconv2d_mfma_supported(ctypes.byref(desc(N=1, H=4, W=w)), ctypes.byref(plain))]
    assert fold_ok and fold_ok == widths[:len(fold_ok)] and set(fold_ok) < set(plain_ok)
    # (128 + 2 W + 2 patch pixels + the zero row) x 64 B + 36864 B <= 81920 B  <=>  W <= 286
    assert max(fold_ok) == 280 and supported(desc(N=1, H=4, W=286), epi()) == 1 and supported(desc(N=1, H=4, W=287), epi()) == 0


def test_null_and_misaligned_arguments():
    lib = native.require()
    assert lib.bnn_hip_bconv2d_mfma_fold_supported(None, ctypes.byref(epi())) == 0
    assert lib.bnn_hip_bconv2d_mfma_fold_supported(ctypes.byref(desc()), None) == 0
    d, e = desc(), epi()
    run = lib.bnn_hip_bconv2d_mfma_fold_fused
    before = native.launch_count()
    assert run(ctypes.byref(d), PTR, PTR, None, PTR, ctypes.byref(e), None) == native.ERR_INVALID_ARG
    assert run(ctypes.byref(d), PTR, PTR, PTR, None, ctypes.byref(e), None) == native.ERR_INVALID_ARG
    assert run(ctypes.byref(d), PTR, PTR, PTR + 8, PTR, ctypes.byref(e), None) == native.ERR_INVALID_ARG
    assert run(ctypes.byref(d), PTR, PTR, PTR, PTR + 8, ctypes.byref(e), None) == native.ERR_INVALID_ARG
    assert run(ctypes.byref(d), PTR, PTR, PTR, PTR, None, None) == native.ERR_INVALID_ARG
    assert run(None, PTR, PTR, PTR, PTR, ctypes.byref(e), None) == native.ERR_INVALID_ARG
    assert run(ctypes.byref(d), None, PTR, PTR, PTR, ctypes.byref(e), None) == native.ERR_INVALID_ARG
    assert run(ctypes.byref(d), PTR + 8, PTR, PTR, PTR, ctypes.byref(e), None) == native.ERR_INVALID_ARG
    # unsupported: nothing is launched
    for dd, ee in ((desc(k=5, pad=2), e), (d, epi(sc_C=96)), (desc(flags=0), e), (d, epi(out_f32=None)),
                   (d, epi(sc_P=None, sc_alpha=None, sc_bn_scale=None, sc_bn_shift=None))):
        assert run(ctypes.byref(dd), PTR, PTR, PTR, PTR, ctypes.byref(ee), None) == native.ERR_UNSUPPORTED
    assert native.launch_count() == before


# ------------------------------------------------------------------------------------------------------ the bookkeeping
def test_header_exports_and_prototypes_agree_and_the_abi_is_16():
    text = open(os.path.join(ROOT, "include", "bnn_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(native.lib_path())
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, code), f"{s} not declared"
        assert hasattr(lib, s), f"{s} not exported"
        assert s in native.EXPORTED_SYMBOLS and getattr(native.require(), s).argtypes
    assert native.require().bnn_hip_shortcut_weight_i8_bytes.restype is ctypes.c_size_t
    assert len(native.require().bnn_hip_bconv2d_mfma_fold_fused.argtypes) == 7
    assert native.require().bnn_hip_abi_version() == 16
    assert re.search(r"#define\s+BNN_HIP_ABI_VERSION\s+16\b", text)


def test_the_switch_and_its_table():
    from bnn_amd import fastpath
    assert fastpath.MFMA_FOLD in ("0", "1", "all")
    for (C, O, H, sc_C), (popcount, mfma) in fastpath.MFMA_FOLD_SHAPES.items():
        assert C % 64 == 0 and O % 64 == 0 and sc_C in (64, 128, 256)
        assert mfma < popcount, "a listed shape measured faster"
    assert all(fold is False for *_, fold in fastpath.MFMA_CONV_SHAPES)

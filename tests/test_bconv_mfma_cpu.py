"""The int8 matrix-core convolution (csrc/bconv_mfma.hip) without a GPU: the documented byte layout of the int8 weight
pack as a numpy model, the host-only admission query at every edge, and the C-ABI bookkeeping."""
import ctypes
import os
import re

import numpy as np
import pytest

from bnn_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bnn_hip_weight_i8_bytes", "bnn_hip_pack_weight_i8", "bnn_hip_bconv2d_mfma_supported", "bnn_hip_bconv2d_mfma_fused")
PTR = 0x10000          # an aligned stand-in: the query never dereferences an operand


# ------------------------------------------------------------------------------------------------- the layout, modelled
def pack_bits_model(sign, L):
    """bnn_hip_pack_weight_f32's wbits / wnz for sign [O, C, 3, 3] in {-1, 0, +1} (include/bnn_hip.h:
    wbits[ob][chunk][j][tap][cwc], bit b of a word = input channel 32 * (chunk * cwc + cw) + b)."""
    O, C = sign.shape[:2]
    per_o = L.taps * L.cwc
    wbits = np.zeros(L.n_words, np.uint32)
    wnz = np.zeros(L.n_words, np.uint32)
    s = sign.reshape(O, C, 9)
    for o in range(O):
        for t in range(9):
            for cwa in range(L.cw32):
                ch, cw = divmod(cwa, L.cwc)
                i = ((o // 32 * L.nchunk + ch) * 32 + o % 32) * per_o + t * L.cwc + cw
                v = s[o, 32 * cwa:32 * cwa + 32, t]
                wbits[i] = sum(1 << b for b in range(len(v)) if v[b] > 0)
                wnz[i] = sum(1 << b for b in range(len(v)) if v[b] != 0)
    return wbits, wnz


def pack_i8_from_bits(wbits, wnz, O, C, L):
    """What bnn_hip_pack_weight_i8 computes, word by word as its kernel indexes them: wnz ? (wbits ? +1 : -1) : 0 at
    w8[o / 64][g][tap][ct][lane][e]."""
    G, per_o = C // 64, L.taps * L.cwc
    w8 = np.zeros((O // 64, G, 9, 4, 64, 16), np.int8)
    for ob, g, t, ct, lane, e in np.ndindex(*w8.shape):
        o, c = 64 * ob + 16 * ct + (lane & 15), 64 * g + 16 * (lane >> 4) + e
        ch, cw = divmod(c // 32, L.cwc)
        i = ((o // 32 * L.nchunk + ch) * 32 + o % 32) * per_o + t * L.cwc + cw
        nz, bit = (int(wnz[i]) >> (c % 32)) & 1, (int(wbits[i]) >> (c % 32)) & 1
        w8[ob, g, t, ct, lane, e] = (1 if bit else -1) if nz else 0
    return w8


def pack_i8_documented(sign):
    """The documented layout straight from the weight tensor:
    w8[o / 64][g][tap][ct][lane][e] = sign(W[64 (o / 64) + 16 ct + (lane & 15)][64 g + 16 (lane >> 4) + e][tap])."""
    O, C = sign.shape[:2]
    s = sign.reshape(O // 64, 4, 16, C // 64, 4, 16, 9)        # [ob][ct][row][g][lane >> 4][e][tap]
    return np.ascontiguousarray(s.transpose(0, 3, 6, 1, 4, 2, 5)).reshape(O // 64, C // 64, 9, 4, 64, 16).astype(np.int8)


@pytest.mark.parametrize("O,C", [(64, 64), (128, 192)])
def test_int8_pack_layout_is_the_documented_one(O, C):
    rng = np.random.default_rng(O + C)
    sign = rng.integers(-1, 2, size=(O, C, 3, 3)).astype(np.int8)      # asymmetric, with zeros
    L = native.weight_layout(O, C, 3, 3)
    wbits, wnz = pack_bits_model(sign, L)
    got = pack_i8_from_bits(wbits, wnz, O, C, L)
    assert np.array_equal(got, pack_i8_documented(sign))
    assert got.nbytes == native.require().bnn_hip_weight_i8_bytes(O, C, 3, 3) == 9 * O * C


def test_fragments_of_the_layout_multiply_like_the_instruction():
    """One 16-channel tile x 16 pixels x one k-step through the lane maps the kernel relies on: lane l holds row / column
    l & 15 of A / B with the SAME 16 k-indices 16 (l >> 4) + e in both; D = A B then equals the plain integer product."""
    rng = np.random.default_rng(3)
    Wt = rng.integers(-1, 2, size=(16, 64))          # [channel][k]
    X = rng.integers(-1, 2, size=(64, 16))           # [k][pixel]
    a = np.zeros((64, 16), np.int64)
    b = np.zeros((64, 16), np.int64)
    for lane in range(64):
        ks = 16 * (lane >> 4) + np.arange(16)
        a[lane] = Wt[lane & 15, ks]
        b[lane] = X[ks, lane & 15]
    D = np.zeros((16, 16), np.int64)
    for la in range(64):
        for lb in range(64):
            if la >> 4 == lb >> 4:                   # the same k group meets
                D[la & 15, lb & 15] += int(a[la] @ b[lb])
    assert np.array_equal(D, Wt @ X)


def test_weight_i8_bytes_edges():
    lib = native.require()
    assert lib.bnn_hip_weight_i8_bytes(512, 512, 3, 3) == 9 * 512 * 512
    for O, C, KH, KW in ((96, 64, 3, 3), (64, 96, 3, 3), (64, 64, 1, 1), (64, 64, 5, 5), (64, 64, 3, 1), (0, 64, 3, 3),
                         (64, -64, 3, 3)):
        assert lib.bnn_hip_weight_i8_bytes(O, C, KH, KW) == 0
    assert lib.bnn_hip_pack_weight_i8(None, PTR, 64, 64, 3, 3, PTR, None) == native.ERR_INVALID_ARG
    assert lib.bnn_hip_pack_weight_i8(PTR, PTR, 64, 64, 3, 3, PTR + 4, None) == native.ERR_INVALID_ARG
    assert lib.bnn_hip_pack_weight_i8(PTR, PTR, 96, 64, 3, 3, PTR, None) == native.ERR_UNSUPPORTED
    assert lib.bnn_hip_pack_weight_i8(PTR, PTR, 64, 64, 1, 1, PTR, None) == native.ERR_UNSUPPORTED


# --------------------------------------------------------------------------------------------------- the admission query
def desc(N=2, C=64, H=9, W=7, O=64, k=3, stride=1, pad=1, dil=1, flags=0, stride_w=None):
    return native.ConvDesc(N, C, H, W, O, k, k, stride, stride if stride_w is None else stride_w, pad, pad, dil, dil, flags)


def epi(**kw):
    f = dict(alpha=PTR, bias=None, post_scale=None, bn_scale=None, bn_shift=None, residual=None, prelu=None, relu=0, flags=0,
             out_f32=PTR, out_P=None, out_M=None, pack_scale=None, pack_shift=None, out_c_offset=0, out_c_total=0,
             sign_thresholds=None)
    f.update(kw)
    e = native.Epilogue(*f.values())
    return e


def supported(d, e):
    return native.require().bnn_hip_bconv2d_mfma_supported(ctypes.byref(d), ctypes.byref(e))


def test_supported_profiles():
    bn = dict(bn_scale=PTR, bn_shift=PTR)
    planes = dict(out_P=PTR, out_M=PTR)
    for e in (epi(), epi(bias=PTR), epi(post_scale=PTR),
              epi(**bn, **planes, relu=1, out_f32=None), epi(**bn, **planes, relu=1, out_f32=None, sign_thresholds=PTR),
              epi(**bn, **planes, relu=1, residual=PTR), epi(**bn, **planes, relu=1, residual=PTR, out_f32=None),
              epi(**bn, relu=1, residual=PTR), epi(bias=PTR, **bn, **planes, residual=PTR)):
        for d in (desc(), desc(stride=2), desc(C=512, O=512, H=7, W=7, N=256), desc(C=64, O=64, H=56, W=56, N=256),
                  desc(C=64, O=128, H=56, W=56, N=256, stride=2), desc(flags=native.FLAG_ACT_NONNEG), desc(H=3, W=3, C=256),
                  desc(N=1, H=1, W=1)):
            assert supported(d, e) == 1
    assert supported(desc(), epi(out_c_total=64)) == 1          # the whole tensor named as its own window


@pytest.mark.parametrize("what,d,e", [
    ("C not a multiple of 64", desc(C=96), epi()),
    ("C below 64", desc(C=32), epi()),
    ("O not a multiple of 64", desc(O=96), epi()),
    ("5x5", desc(k=5, pad=2), epi()),
    ("1x1", desc(k=1, pad=0), epi()),
    ("dilation 2", desc(dil=2, pad=2), epi()),
    ("padding 0", desc(pad=0), epi()),
    ("padding 2", desc(pad=2), epi()),
    ("stride 3", desc(stride=3), epi()),
    ("strides differ", desc(stride=1, stride_w=2), epi()),
    ("forced generic", desc(flags=native.FLAG_FORCE_GENERIC), epi()),
    ("row too wide for the LDS patch", desc(N=1, H=4, W=2000), epi()),
    ("PReLU", desc(), epi(prelu=PTR)),
    ("residual after the activation", desc(), epi(residual=PTR, flags=native.EPI_RES_AFTER_ACT)),
    ("pack before residual", desc(), epi(residual=PTR, flags=native.EPI_RES_AFTER_ACT | native.EPI_PACK_BEFORE_RES)),
    ("pack relu", desc(), epi(out_P=PTR, out_M=PTR, flags=native.EPI_PACK_RELU)),
    ("pack affine", desc(), epi(out_P=PTR, out_M=PTR, pack_scale=PTR, pack_shift=PTR)),
    ("channel window", desc(), epi(out_c_offset=3, out_c_total=80)),
    ("wider tensor", desc(), epi(out_c_total=80)),
    ("misaligned planes", desc(), epi(out_P=PTR + 4, out_M=PTR)),
    ("misaligned fp32 output", desc(), epi(out_f32=PTR + 2)),
    ("misaligned thresholds", desc(), epi(out_f32=None, out_P=PTR, out_M=PTR, bn_scale=PTR, bn_shift=PTR, relu=1,
                                          sign_thresholds=PTR + 2)),
    ("no output", desc(), epi(out_f32=None)),
    ("one plane", desc(), epi(out_P=PTR)),
    ("no alpha", desc(), epi(alpha=None)),
    ("half a BatchNorm", desc(), epi(bn_scale=PTR)),
    ("empty batch", desc(N=0), epi()),
], ids=lambda v: v if isinstance(v, str) else "")
def test_unsupported_edges(what, d, e):
    assert supported(d, e) == 0, what


def test_folded_shortcut_is_not_taken():
    e = native.Epilogue(PTR, None, None, PTR, PTR, None, None, 1, 0, PTR, PTR, PTR, None, None, 0, 0, None,
                        PTR, PTR, PTR, PTR, PTR, 64, 0)
    assert supported(desc(C=128, O=128, flags=native.FLAG_ACT_NONNEG), e) == 0


def test_null_arguments():
    lib = native.require()
    assert lib.bnn_hip_bconv2d_mfma_supported(None, ctypes.byref(epi())) == 0
    assert lib.bnn_hip_bconv2d_mfma_supported(ctypes.byref(desc()), None) == 0
    d, e = desc(), epi()
    assert lib.bnn_hip_bconv2d_mfma_fused(ctypes.byref(d), PTR, PTR, None, ctypes.byref(e), None) == native.ERR_INVALID_ARG
    assert lib.bnn_hip_bconv2d_mfma_fused(ctypes.byref(d), PTR, PTR, PTR + 8, ctypes.byref(e), None) == native.ERR_INVALID_ARG
    assert lib.bnn_hip_bconv2d_mfma_fused(ctypes.byref(d), PTR, PTR, PTR, None, None) == native.ERR_INVALID_ARG
    before = native.launch_count()
    d5 = desc(k=5, pad=2)
    assert lib.bnn_hip_bconv2d_mfma_fused(ctypes.byref(d5), PTR, PTR, PTR, ctypes.byref(e), None) == native.ERR_UNSUPPORTED
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
    assert native.require().bnn_hip_weight_i8_bytes.restype is ctypes.c_size_t
    assert native.require().bnn_hip_abi_version() == 16
    assert re.search(r"#define\s+BNN_HIP_ABI_VERSION\s+16\b", text)


def test_the_switch_and_its_table():
    from bnn_amd import fastpath
    assert fastpath.MFMA_CONV in ("0", "1", "all")
    for (C, O, H, stride, fold), pairs in fastpath.MFMA_CONV_SHAPES.items():
        assert C % 64 == 0 and O % 64 == 0 and stride in (1, 2) and fold is False
        assert all(mfma < popcount for popcount, mfma in pairs), "a listed shape measured faster"

"""The FP4 form of the matrix-core convolution (csrc/bconv_mfma.hip, F4) without a GPU: the documented nibble layout of
the FP4 weight pack as a numpy model, one fragment pair through the lane maps, the host-only admission queries at every
edge, and the C-ABI bookkeeping."""
import ctypes
import os
import re

import numpy as np
import pytest

from bnn_amd import native
from tests.test_bconv_mfma_cpu import PTR, desc, epi, pack_bits_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bnn_hip_weight_f4_bytes", "bnn_hip_pack_weight_f4", "bnn_hip_bconv2d_mfma4_supported",
       "bnn_hip_bconv2d_mfma4_fused", "bnn_hip_bconv2d_mfma4_fold_supported", "bnn_hip_bconv2d_mfma4_fold_fused")
E2M1 = {1: 0x2, -1: 0xA, 0: 0x0}          # the three values the operands take, exact in E2M1
VALUE = {0x2: 1, 0xA: -1, 0x0: 0}


# ------------------------------------------------------------------------------------------------- the layout, modelled
def to_bytes(nib):
    """[..., 32] nibbles -> [..., 16] bytes: nibble e is the low (e even) or high (e odd) half of byte e / 2."""
    return (nib[..., 0::2] | (nib[..., 1::2] << 4)).astype(np.uint8)


def pack_f4_from_bits(wbits, wnz, O, C, L):
    """What bnn_hip_pack_weight_f4 computes, dword by dword as its kernel indexes them: eight consecutive channels of one
    32-bit word, wnz ? (wbits ? 0x2 : 0xA) : 0x0, at w4[o / 64][g][tap][ct][lane][e]."""
    G, per_o = C // 128, L.taps * L.cwc
    nib = np.zeros((O // 64, G, 9, 4, 64, 32), np.uint8)
    for ob, g, t, ct, lane, e8 in np.ndindex(O // 64, G, 9, 4, 64, 4):
        o, c0 = 64 * ob + 16 * ct + (lane & 15), 128 * g + 32 * (lane >> 4) + 8 * e8
        ch, cw = divmod(c0 // 32, L.cwc)
        i = ((o // 32 * L.nchunk + ch) * 32 + o % 32) * per_o + t * L.cwc + cw
        b, z = int(wbits[i]) >> (c0 % 32), int(wnz[i]) >> (c0 % 32)
        for k in range(8):
            nib[ob, g, t, ct, lane, 8 * e8 + k] = ((0x2 if (b >> k) & 1 else 0xA) if (z >> k) & 1 else 0x0)
    return to_bytes(nib)


def pack_f4_documented(sign):
    """The documented layout straight from the weight tensor:
    w4[o / 64][g][tap][ct][lane][e] = E2M1(sign(W[64 (o / 64) + 16 ct + (lane & 15)][128 g + 32 (lane >> 4) + e][tap]))."""
    O, C = sign.shape[:2]
    s = sign.reshape(O // 64, 4, 16, C // 128, 4, 32, 9)        # [ob][ct][row][g][lane >> 4][e][tap]
    s = np.ascontiguousarray(s.transpose(0, 3, 6, 1, 4, 2, 5)).reshape(O // 64, C // 128, 9, 4, 64, 32)
    nib = np.where(s > 0, 0x2, np.where(s < 0, 0xA, 0x0)).astype(np.uint8)
    return to_bytes(nib)


@pytest.mark.parametrize("O,C", [(64, 128), (192, 384), (64, 384), (192, 128)])
def test_fp4_pack_layout_is_the_documented_one(O, C):
    rng = np.random.default_rng(O + C)
    sign = rng.choice(np.array([-1, -1, 0, 1, 1, 1], np.int8), size=(O, C, 3, 3))      # asymmetric, with zeros
    L = native.weight_layout(O, C, 3, 3)
    wbits, wnz = pack_bits_model(sign, L)
    got = pack_f4_from_bits(wbits, wnz, O, C, L)
    assert np.array_equal(got, pack_f4_documented(sign))
    assert got.nbytes == native.require().bnn_hip_weight_f4_bytes(O, C, 3, 3) == 9 * O * C // 2
    assert set(np.unique(got & 15)) | set(np.unique(got >> 4)) <= {0x0, 0x2, 0xA}


def test_fragments_of_the_layout_multiply_like_the_instruction():
    """One 16-channel tile x 16 pixels x one 128-wide k-step through the lane maps the kernel relies on: lane l holds
    row / column l & 15 of A / B with the SAME 32 k-indices 32 (l >> 4) + e in both, as E2M1 nibbles; D = A B then equals
    the plain integer product."""
    rng = np.random.default_rng(4)
    Wt = rng.integers(-1, 2, size=(16, 128))          # [channel][k]
    X = rng.integers(-1, 2, size=(128, 16))           # [k][pixel]
    enc = np.vectorize(E2M1.get)
    a = np.zeros((64, 16), np.uint8)
    b = np.zeros((64, 16), np.uint8)
    for lane in range(64):
        ks = 32 * (lane >> 4) + np.arange(32)
        a[lane] = to_bytes(enc(Wt[lane & 15, ks]).astype(np.uint8))
        b[lane] = to_bytes(enc(X[ks, lane & 15]).astype(np.uint8))

    def values(frag):                                  # 16 bytes -> the 32 values they encode, nibble order
        nib = np.stack([frag & 15, frag >> 4], axis=-1).reshape(-1)
        return np.array([VALUE[int(n)] for n in nib], np.float32)

    D = np.zeros((16, 16), np.float32)                 # fp32 accumulation, as the instruction's
    for la in range(64):
        for lb in range(64):
            if la >> 4 == lb >> 4:                     # the same k group meets
                D[la & 15, lb & 15] += np.float32(values(a[la]) @ values(b[lb]))
    assert np.array_equal(D.astype(np.int64), Wt @ X)


def test_weight_f4_bytes_edges():
    lib = native.require()
    assert lib.bnn_hip_weight_f4_bytes(512, 512, 3, 3) == 9 * 512 * 512 // 2
    assert lib.bnn_hip_weight_f4_bytes(64, 128, 3, 3) == 9 * 64 * 128 // 2
    assert lib.bnn_hip_weight_f4_bytes(192, 384, 3, 3) == 9 * 192 * 384 // 2
    for O, C, KH, KW in ((64, 64, 3, 3), (64, 192, 3, 3), (96, 128, 3, 3), (64, 128, 1, 1), (64, 128, 5, 5),
                         (64, 128, 3, 1), (0, 128, 3, 3), (64, -128, 3, 3)):
        assert lib.bnn_hip_weight_f4_bytes(O, C, KH, KW) == 0
    assert lib.bnn_hip_pack_weight_f4(None, PTR, 64, 128, 3, 3, PTR, None) == native.ERR_INVALID_ARG
    assert lib.bnn_hip_pack_weight_f4(PTR, PTR, 64, 128, 3, 3, PTR + 4, None) == native.ERR_INVALID_ARG
    before = native.launch_count()
    assert lib.bnn_hip_pack_weight_f4(PTR, PTR, 64, 64, 3, 3, PTR, None) == native.ERR_UNSUPPORTED
    assert lib.bnn_hip_pack_weight_f4(PTR, PTR, 64, 192, 3, 3, PTR, None) == native.ERR_UNSUPPORTED
    assert lib.bnn_hip_pack_weight_f4(PTR, PTR, 96, 128, 3, 3, PTR, None) == native.ERR_UNSUPPORTED
    assert lib.bnn_hip_pack_weight_f4(PTR, PTR, 64, 128, 1, 1, PTR, None) == native.ERR_UNSUPPORTED
    assert native.launch_count() == before


# --------------------------------------------------------------------------------------------------- the admission queries
def supported(d, e, twin=False):
    lib = native.require()
    fn = lib.bnn_hip_bconv2d_mfma_supported if twin else lib.bnn_hip_bconv2d_mfma4_supported
    return fn(ctypes.byref(d), ctypes.byref(e))


def fold_epi(sc_C=64, **kw):
    """Exactly the fold's epilogue: alpha, BatchNorm, ReLU, fp32 + planes, the shortcut (sc_wbits is not read)."""
    f = dict(alpha=PTR, bias=None, post_scale=None, bn_scale=PTR, bn_shift=PTR, residual=None, prelu=None, relu=1, flags=0,
             out_f32=PTR, out_P=PTR, out_M=PTR, pack_scale=None, pack_shift=None, out_c_offset=0, out_c_total=0,
             sign_thresholds=None, sc_P=PTR, sc_wbits=None, sc_alpha=PTR, sc_bn_scale=PTR, sc_bn_shift=PTR, sc_C=sc_C,
             sc_in_hw=0)
    f.update(kw)
    return native.Epilogue(**f)


def fold_supported(d, e, twin=False):
    lib = native.require()
    fn = lib.bnn_hip_bconv2d_mfma_fold_supported if twin else lib.bnn_hip_bconv2d_mfma4_fold_supported
    return fn(ctypes.byref(d), ctypes.byref(e))


def test_supported_profiles():
    bn = dict(bn_scale=PTR, bn_shift=PTR)
    planes = dict(out_P=PTR, out_M=PTR)
    for e in (epi(), epi(bias=PTR), epi(post_scale=PTR),
              epi(**bn, **planes, relu=1, out_f32=None), epi(**bn, **planes, relu=1, out_f32=None, sign_thresholds=PTR),
              epi(**bn, **planes, relu=1, residual=PTR), epi(**bn, **planes, relu=1, residual=PTR, out_f32=None),
              epi(**bn, relu=1, residual=PTR), epi(bias=PTR, **bn, **planes, residual=PTR)):
        for d in (desc(C=128), desc(C=128, stride=2), desc(C=512, O=512, H=7, W=7, N=256),
                  desc(C=128, O=128, H=28, W=28, N=256), desc(C=128, O=256, H=28, W=28, N=256, stride=2),
                  desc(C=256, flags=native.FLAG_ACT_NONNEG), desc(H=3, W=3, C=256), desc(N=1, H=1, W=1, C=384, O=192)):
            assert supported(d, e) == 1 and supported(d, e, twin=True) == 1
    assert supported(desc(C=128), epi(out_c_total=64)) == 1


@pytest.mark.parametrize("what,d,e,twin", [
    ("C = 64", desc(C=64), epi(), 1),
    ("C = 192", desc(C=192), epi(), 1),
    ("C = 96", desc(C=96), epi(), 0),
    ("O = 96", desc(C=128, O=96), epi(), 0),
    ("5x5", desc(C=128, k=5, pad=2), epi(), 0),
    ("1x1", desc(C=128, k=1, pad=0), epi(), 0),
    ("dilation 2", desc(C=128, dil=2, pad=2), epi(), 0),
    ("padding 0", desc(C=128, pad=0), epi(), 0),
    ("stride 3", desc(C=128, stride=3), epi(), 0),
    ("strides differ", desc(C=128, stride=1, stride_w=2), epi(), 0),
    ("forced generic", desc(C=128, flags=native.FLAG_FORCE_GENERIC), epi(), 0),
    ("row too wide for the LDS patch", desc(C=128, N=1, H=4, W=2000), epi(), 0),
    ("PReLU", desc(C=128), epi(prelu=PTR), 0),
    ("residual after the activation", desc(C=128), epi(residual=PTR, flags=native.EPI_RES_AFTER_ACT), 0),
    ("pack before residual", desc(C=128), epi(residual=PTR, flags=native.EPI_RES_AFTER_ACT | native.EPI_PACK_BEFORE_RES), 0),
    ("pack relu", desc(C=128), epi(out_P=PTR, out_M=PTR, flags=native.EPI_PACK_RELU), 0),
    ("pack affine", desc(C=128), epi(out_P=PTR, out_M=PTR, pack_scale=PTR, pack_shift=PTR), 0),
    ("channel window", desc(C=128), epi(out_c_offset=3, out_c_total=80), 0),
    ("wider tensor", desc(C=128), epi(out_c_total=80), 0),
    ("misaligned planes", desc(C=128), epi(out_P=PTR + 4, out_M=PTR), 0),
    ("misaligned fp32 output", desc(C=128), epi(out_f32=PTR + 2), 0),
    ("no output", desc(C=128), epi(out_f32=None), 0),
    ("no alpha", desc(C=128), epi(alpha=None), 0),
    ("empty batch", desc(C=128, N=0), epi(), 0),
    ("a shortcut at the dense entry", desc(C=128, O=128, flags=native.FLAG_ACT_NONNEG), fold_epi(sc_wbits=PTR), 0),
], ids=lambda v: v if isinstance(v, str) else "")
def test_unsupported_edges(what, d, e, twin):
    """`twin`: what the int8 entry says to the same call — the FP4 entry refuses everything it refuses, and C = 64 / 192."""
    assert supported(d, e, twin=True) == twin, what
    assert supported(d, e) == 0, what


def test_fold_truth_table():
    nn = native.FLAG_ACT_NONNEG
    for C, sc in ((128, 64), (256, 128), (512, 256), (128, 128), (384, 64)):
        d = desc(C=C, O=C, H=8, W=8, flags=nn)
        assert fold_supported(d, fold_epi(sc)) == 1 and fold_supported(d, fold_epi(sc), twin=True) == 1
        assert fold_supported(d, fold_epi(sc, sc_in_hw=(16 << 16) | 16)) == 1
        assert fold_supported(desc(C=C, O=C, H=8, W=8, flags=nn | native.FLAG_THROUGHPUT), fold_epi(sc)) == 1
    for C in (64, 192):                                # whole 128-channel groups only: the int8 twin takes these
        d = desc(C=C, O=C, H=8, W=8, flags=nn)
        assert fold_supported(d, fold_epi(64), twin=True) == 1 and fold_supported(d, fold_epi(64)) == 0
    d = desc(C=128, O=128, H=8, W=8, flags=nn)
    refused = {
        "no shortcut": epi(bn_scale=PTR, bn_shift=PTR, relu=1, out_P=PTR, out_M=PTR),
        "planes only": fold_epi(out_f32=None),
        "fp32 only": fold_epi(out_P=None, out_M=None),
        "no ReLU": fold_epi(relu=0),
        "no BatchNorm": fold_epi(bn_scale=None, bn_shift=None),
        "a bias": fold_epi(bias=PTR),
        "a post-scale": fold_epi(post_scale=PTR),
        "a residual too": fold_epi(residual=PTR),
        "thresholds": fold_epi(sign_thresholds=PTR),
        "PReLU": fold_epi(prelu=PTR),
        "a pre-activation switch": fold_epi(flags=native.EPI_PACK_RELU),
        "a channel window": fold_epi(out_c_offset=3, out_c_total=160),
        "96 shortcut channels": fold_epi(96),
        "512 shortcut channels": fold_epi(512),
    }
    for what, e in refused.items():
        assert fold_supported(d, e, twin=True) == 0 and fold_supported(d, e) == 0, what
    for what, dd in {
        "ternary activations": desc(C=128, O=128, H=8, W=8),
        "zero weights": desc(C=128, O=128, H=8, W=8, flags=nn | native.FLAG_WEIGHT_ZEROS),
        "forced generic": desc(C=128, O=128, H=8, W=8, flags=nn | native.FLAG_FORCE_GENERIC),
        "dilation": desc(C=128, O=128, H=8, W=8, dil=2, pad=2, flags=nn),
        "5x5": desc(C=128, O=128, H=8, W=8, k=5, pad=2, flags=nn),
        "O = 96": desc(C=128, O=96, H=8, W=8, flags=nn),
    }.items():
        assert fold_supported(dd, fold_epi(64), twin=True) == 0 and fold_supported(dd, fold_epi(64)) == 0, what


def test_null_arguments_and_refusals_launch_nothing():
    lib = native.require()
    assert lib.bnn_hip_bconv2d_mfma4_supported(None, ctypes.byref(epi())) == 0
    assert lib.bnn_hip_bconv2d_mfma4_supported(ctypes.byref(desc(C=128)), None) == 0
    assert lib.bnn_hip_bconv2d_mfma4_fold_supported(None, ctypes.byref(fold_epi())) == 0
    assert lib.bnn_hip_bconv2d_mfma4_fold_supported(ctypes.byref(desc(C=128, O=128)), None) == 0
    d, e = desc(C=128), epi()
    by = ctypes.byref
    assert lib.bnn_hip_bconv2d_mfma4_fused(by(d), PTR, PTR, None, by(e), None) == native.ERR_INVALID_ARG
    assert lib.bnn_hip_bconv2d_mfma4_fused(by(d), PTR, PTR, PTR + 8, by(e), None) == native.ERR_INVALID_ARG
    assert lib.bnn_hip_bconv2d_mfma4_fused(by(d), PTR, PTR, PTR, None, None) == native.ERR_INVALID_ARG
    before = native.launch_count()
    for dd in (desc(C=64), desc(C=192), desc(C=128, k=5, pad=2)):
        assert lib.bnn_hip_bconv2d_mfma4_fused(by(dd), PTR, PTR, PTR, by(e), None) == native.ERR_UNSUPPORTED
    fd, fe = desc(C=128, O=128, H=8, W=8, flags=native.FLAG_ACT_NONNEG), fold_epi()
    assert lib.bnn_hip_bconv2d_mfma4_fold_fused(by(fd), PTR, PTR, None, PTR, by(fe), None) == native.ERR_INVALID_ARG
    assert lib.bnn_hip_bconv2d_mfma4_fold_fused(by(fd), PTR, PTR, PTR, PTR + 8, by(fe), None) == native.ERR_INVALID_ARG
    assert lib.bnn_hip_bconv2d_mfma4_fold_fused(by(fd), PTR, PTR, PTR, PTR, by(e), None) == native.ERR_UNSUPPORTED
    for C in (64, 192):
        fd = desc(C=C, O=C, H=8, W=8, flags=native.FLAG_ACT_NONNEG)
        assert lib.bnn_hip_bconv2d_mfma4_fold_fused(by(fd), PTR, PTR, PTR, PTR, by(fe), None) == native.ERR_UNSUPPORTED
    assert native.launch_count() == before


# ------------------------------------------------------------------------------------------------------ the bookkeeping
def test_header_exports_and_prototypes_agree_and_the_abi_is_16():
    text = open(os.path.join(ROOT, "include", "bnn_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(native.lib_path())
    proto = native.require()
    for s, twin in zip(NEW, ("bnn_hip_weight_i8_bytes", "bnn_hip_pack_weight_i8", "bnn_hip_bconv2d_mfma_supported",
                             "bnn_hip_bconv2d_mfma_fused", "bnn_hip_bconv2d_mfma_fold_supported",
                             "bnn_hip_bconv2d_mfma_fold_fused")):
        assert re.search(r"\b%s\s*\(" % s, code), f"{s} not declared"
        assert hasattr(lib, s), f"{s} not exported"
        assert s in native.EXPORTED_SYMBOLS and getattr(proto, s).argtypes
        assert getattr(proto, s).argtypes == getattr(proto, twin).argtypes, f"{s} mirrors {twin}"
        assert getattr(proto, s).restype is getattr(proto, twin).restype
    assert proto.bnn_hip_weight_f4_bytes.restype is ctypes.c_size_t
    assert proto.bnn_hip_abi_version() == 16
    assert re.search(r"#define\s+BNN_HIP_ABI_VERSION\s+16\b", text)


def test_the_switch_and_its_table():
    from bnn_amd import fastpath
    assert fastpath.MFMA_F4 in ("0", "1", "all")
    for key, (i8_us, f4_us) in fastpath.MFMA_F4_SHAPES.items():
        assert key[0] % 128 == 0 and len(key) in (4, 5), key
        if len(key) == 5:
            assert key[4] is False and key in fastpath.MFMA_CONV_SHAPES, "a dense key of a launch on the matrix cores"
        else:
            assert key in fastpath.MFMA_FOLD_SHAPES, "a fold key of a launch on the matrix cores"
        assert f4_us < i8_us, "a listed shape measured faster"
    saved = fastpath.MFMA_F4
    try:
        fastpath.MFMA_F4 = "0"
        assert not fastpath.mfma_f4_admitted((512, 512, 7, 1, False))
        fastpath.MFMA_F4 = "all"
        assert fastpath.mfma_f4_admitted((512, 512, 7, 1, False)) and fastpath.mfma_f4_admitted((128, 128, 28, 64))
        fastpath.MFMA_F4 = "1"
        assert fastpath.mfma_f4_admitted((512, 512, 7, 1, False)) == ((512, 512, 7, 1, False) in fastpath.MFMA_F4_SHAPES)
    finally:
        fastpath.MFMA_F4 = saved

"""The 1x1 convolution on the FP4 matrix cores (csrc/bconv1x1_mfma.hip) without a GPU: the documented nibble layout of its
weight pack and the kernel's activation indexing as numpy models, the host-only admission query at every edge, the C-ABI
bookkeeping, and the gfx950 code object (one matrix opcode, no spills)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from bnn_amd import fastpath, native
from tests.test_bconv_mfma_cpu import PTR, desc, epi
from tests.test_bconv_mfma_f4_cpu import fold_epi, to_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "binary-networks-pytorch_amd", "csrc", "bconv1x1_mfma.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
NEW = ("bnn_hip_weight1x1_f4_bytes", "bnn_hip_pack_weight1x1_f4", "bnn_hip_bconv1x1_mfma4_supported",
       "bnn_hip_bconv1x1_mfma4_fused")


def d1(C=128, O=64, **kw):
    kw.setdefault("k", 1)
    kw.setdefault("pad", 0)
    return desc(C=C, O=O, **kw)


def supported(d, e):
    return native.require().bnn_hip_bconv1x1_mfma4_supported(ctypes.byref(d), ctypes.byref(e))


# ------------------------------------------------------------------------------------------------- the layout, modelled
def pack_bits_1x1(sign, L):
    """bnn_hip_pack_weight_f32's wbits / wnz for sign [O, C] in {-1, 0, +1} (include/bnn_hip.h: wbits[ob][chunk][j][tap][cwc]
    with one tap; bit b of a word = input channel 32 * (chunk * cwc + cw) + b)."""
    O, C = sign.shape
    wbits, wnz = np.zeros(L.n_words, np.uint32), np.zeros(L.n_words, np.uint32)
    shifts = np.arange(32, dtype=np.uint64)
    for o in range(O):
        for cwa in range(L.cw32):
            ch, cw = divmod(cwa, L.cwc)
            i = ((o // 32 * L.nchunk + ch) * 32 + o % 32) * L.cwc + cw
            v = sign[o, 32 * cwa:32 * cwa + 32]
            wbits[i] = int(((v > 0).astype(np.uint64) << shifts).sum())
            wnz[i] = int(((v != 0).astype(np.uint64) << shifts).sum())
    return wbits, wnz


def pack_f4_from_bits(wbits, wnz, O, C, L):
    """What bnn_hip_pack_weight1x1_f4 computes, dword by dword as the pack kernel indexes them with one tap: eight
    consecutive channels of one 32-bit word, wnz ? (wbits ? 0x2 : 0xA) : 0x0, at w4[o / 64][g][ct][lane][e]."""
    G = C // 128
    nib = np.zeros((O // 64, G, 4, 64, 32), np.uint8)
    for ob, g, ct, lane, e8 in np.ndindex(O // 64, G, 4, 64, 4):
        o, c0 = 64 * ob + 16 * ct + (lane & 15), 128 * g + 32 * (lane >> 4) + 8 * e8
        ch, cw = divmod(c0 // 32, L.cwc)
        i = ((o // 32 * L.nchunk + ch) * 32 + o % 32) * L.cwc + cw
        b, z = int(wbits[i]) >> (c0 % 32), int(wnz[i]) >> (c0 % 32)
        for k in range(8):
            nib[ob, g, ct, lane, 8 * e8 + k] = ((0x2 if (b >> k) & 1 else 0xA) if (z >> k) & 1 else 0x0)
    return to_bytes(nib)


def pack_f4_documented(sign):
    """w4[o / 64][g][ct][lane][e] = E2M1(sign(W[64 (o / 64) + 16 ct + (lane & 15)][128 g + 32 (lane >> 4) + e]))."""
    O, C = sign.shape
    s = sign.reshape(O // 64, 4, 16, C // 128, 4, 32)          # [ob][ct][row][g][lane >> 4][e]
    s = np.ascontiguousarray(s.transpose(0, 3, 1, 4, 2, 5)).reshape(O // 64, C // 128, 4, 64, 32)
    return to_bytes(np.where(s > 0, 0x2, np.where(s < 0, 0xA, 0x0)).astype(np.uint8))


@pytest.mark.parametrize("O,C", [(64, 128), (192, 384), (64, 2048)])
def test_fp4_1x1_pack_layout_is_the_documented_one(O, C):
    rng = np.random.default_rng(O + C)
    sign = rng.choice(np.array([-1, -1, 0, 1, 1, 1], np.int8), size=(O, C))      # asymmetric, with zeros
    L = native.weight_layout(O, C, 1, 1)
    got = pack_f4_from_bits(*pack_bits_1x1(sign, L), O, C, L)
    assert np.array_equal(got, pack_f4_documented(sign))
    assert got.nbytes == native.require().bnn_hip_weight1x1_f4_bytes(O, C) == O * C // 2
    assert set(np.unique(got & 15)) | set(np.unique(got >> 4)) <= {0x0, 0x2, 0xA}


@pytest.mark.parametrize("N,C,H,W", [(3, 128, 9, 7), (2, 512, 3, 3), (1, 2048, 2, 2)])
def test_activation_half_words_of_a_lane_are_its_channels_and_stay_inside_the_planes(N, C, H, W):
    """The kernel's B operand: lane l of pixel tile pt reads ONE 32-bit half-word per k-step; its 32 bits must be channels
    128 k + 32 (l >> 4) + e of pixel min(q, N H W - 1) in the [N][C / 64][H][W] uint64 planes, and no index may pass them."""
    hw, G, npix = H * W, C // 128, N * H * W
    chan = np.arange(N * (C // 64) * hw * 2, dtype=np.int64)     # what each half-word holds: (pixel, first channel)
    words = chan // 2
    n, grp, r = words // ((C // 64) * hw), words // hw % (C // 64), words % hw
    first_channel, pixel = 64 * grp + 32 * (chan % 2), n * hw + r
    for q0 in range(0, npix, 256):
        for lane in range(64):
            lrow, lgrp = lane & 15, lane >> 4
            for pt in range(16):                                 # 4 waves x 4 tiles of a 256-pixel workgroup
                q = min(q0 + 16 * pt + lrow, npix - 1)
                nq, rq = divmod(q, hw)
                wi = 2 * ((nq * (2 * G) + (lgrp >> 1)) * hw + rq) + (lgrp & 1)
                for k in range(G):
                    i = wi + k * 4 * hw
                    assert 0 <= i < chan.size
                    assert pixel[i] == q and first_channel[i] == 128 * k + 32 * lgrp


def test_weight1x1_f4_bytes_edges():
    lib = native.require()
    assert lib.bnn_hip_weight1x1_f4_bytes(2048, 512) == 2048 * 512 // 2
    for O, C in ((64, 64), (64, 192), (96, 128), (0, 128), (64, -128), (64, 0)):
        assert lib.bnn_hip_weight1x1_f4_bytes(O, C) == 0
    assert lib.bnn_hip_pack_weight1x1_f4(None, PTR, 64, 128, 1, 1, PTR, None) == native.ERR_INVALID_ARG
    assert lib.bnn_hip_pack_weight1x1_f4(PTR, PTR, 64, 128, 1, 1, PTR + 4, None) == native.ERR_INVALID_ARG
    before = native.launch_count()
    for O, C, k in ((64, 64, 1), (64, 192, 1), (96, 128, 1), (64, 128, 3)):
        assert lib.bnn_hip_pack_weight1x1_f4(PTR, PTR, O, C, k, k, PTR, None) == native.ERR_UNSUPPORTED
    assert native.launch_count() == before
    # the existing queries keep their answers
    assert lib.bnn_hip_weight_f4_bytes(64, 128, 1, 1) == 0 and lib.bnn_hip_weight_i8_bytes(64, 128, 1, 1) == 0


# --------------------------------------------------------------------------------------------------- the admission query
BN = dict(bn_scale=PTR, bn_shift=PTR)
PLANES = dict(out_P=PTR, out_M=PTR)
AFF = dict(pack_scale=PTR, pack_shift=PTR)
LATE = dict(residual=PTR, flags=native.EPI_RES_AFTER_ACT)
FORMS = {
    "a plain": epi(), "a bias": epi(bias=PTR), "a post scale": epi(post_scale=PTR),
    "b BN + ReLU -> planes": epi(**BN, **PLANES, relu=1, out_f32=None),
    "b with thresholds": epi(**BN, **PLANES, relu=1, out_f32=None, sign_thresholds=PTR),
    "c BN -> fp32": epi(**BN),
    "d BN + residual + ReLU -> fp32": epi(**BN, relu=1, residual=PTR),
    "d with planes": epi(**BN, **PLANES, relu=1, residual=PTR),
    "e ReLU -> pack affine -> planes": epi(**PLANES, **AFF, relu=1, out_f32=None),
    "e PReLU -> pack affine -> planes": epi(**PLANES, **AFF, prelu=PTR, out_f32=None),
    "f ReLU -> late residual -> fp32": epi(relu=1, **LATE),
    "f PReLU -> late residual -> fp32": epi(prelu=PTR, **LATE),
    "f ReLU with pack-affine planes": epi(relu=1, **LATE, **PLANES, **AFF),
    "f PReLU with pack-affine planes": epi(prelu=PTR, **LATE, **PLANES, **AFF),
}


@pytest.mark.parametrize("form", list(FORMS))
def test_every_epilogue_form_is_taken(form):
    e = FORMS[form]
    for d in (d1(), d1(C=256, O=192, N=5, H=7, W=7), d1(C=2048, O=512, N=128, H=7, W=7), d1(C=256, O=64, N=128, H=56, W=56),
              d1(flags=native.FLAG_ACT_NONNEG), d1(flags=native.FLAG_WEIGHT_ZEROS), d1(N=1, H=1, W=1, C=2048)):
        assert supported(d, e) == 1, form
        # the 3x3 queries keep saying no to a 1x1 weight
        lib = native.require()
        assert lib.bnn_hip_bconv2d_mfma_supported(ctypes.byref(d), ctypes.byref(e)) == 0
        assert lib.bnn_hip_bconv2d_mfma4_supported(ctypes.byref(d), ctypes.byref(e)) == 0


REFUSED = [
    ("C = 64", d1(C=64), epi()),
    ("C = 192", d1(C=192), epi()),
    ("O = 96", d1(O=96), epi()),
    ("3x3", desc(C=128, k=3, pad=1), epi()),
    ("stride 2", d1(stride=2), epi()),
    ("padding 1", d1(pad=1), epi()),
    ("dilation 2", d1(dil=2), epi()),
    ("folded shortcut", d1(O=128, flags=native.FLAG_ACT_NONNEG), fold_epi(sc_wbits=PTR)),
    ("channel window", d1(), epi(out_c_offset=3, out_c_total=80)),
    ("wider tensor", d1(), epi(out_c_total=80)),
    ("forced generic", d1(flags=native.FLAG_FORCE_GENERIC), epi()),
    ("no output", d1(), epi(out_f32=None)),
    ("misaligned fp32 output", d1(), epi(out_f32=PTR + 2)),
    ("half a pack affine", d1(), epi(out_P=PTR, out_M=PTR, pack_scale=PTR)),
]


@pytest.mark.parametrize("what,d,e", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_edges_launch_nothing(what, d, e):
    lib = native.require()
    assert supported(d, e) == 0, what
    before = native.launch_count()
    st = lib.bnn_hip_bconv1x1_mfma4_fused(ctypes.byref(d), PTR, PTR, PTR, ctypes.byref(e), None)
    assert st in (native.ERR_UNSUPPORTED, native.ERR_INVALID_ARG), what
    assert native.launch_count() == before


def test_null_arguments():
    lib = native.require()
    d, e = d1(), epi()
    assert lib.bnn_hip_bconv1x1_mfma4_supported(None, ctypes.byref(e)) == 0
    assert lib.bnn_hip_bconv1x1_mfma4_supported(ctypes.byref(d), None) == 0
    assert lib.bnn_hip_bconv1x1_mfma4_fused(ctypes.byref(d), PTR, PTR, None, ctypes.byref(e), None) == native.ERR_INVALID_ARG
    assert lib.bnn_hip_bconv1x1_mfma4_fused(ctypes.byref(d), PTR, PTR, PTR + 8, ctypes.byref(e), None) == native.ERR_INVALID_ARG
    assert lib.bnn_hip_bconv1x1_mfma4_fused(ctypes.byref(d), PTR, PTR, PTR, None, None) == native.ERR_INVALID_ARG


# ------------------------------------------------------------------------------------------------------ the bookkeeping
def test_header_exports_and_prototypes_agree_and_the_abi_is_16():
    text = open(os.path.join(ROOT, "include", "bnn_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(native.lib_path())
    proto = native.require()
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, code), f"{s} not declared"
        assert hasattr(lib, s), f"{s} not exported"
        assert s in native.EXPORTED_SYMBOLS and getattr(proto, s).argtypes
    for s, twin in (("bnn_hip_pack_weight1x1_f4", "bnn_hip_pack_weight_f4"),
                    ("bnn_hip_bconv1x1_mfma4_supported", "bnn_hip_bconv2d_mfma4_supported"),
                    ("bnn_hip_bconv1x1_mfma4_fused", "bnn_hip_bconv2d_mfma4_fused")):
        assert getattr(proto, s).argtypes == getattr(proto, twin).argtypes, f"{s} mirrors {twin}"
        assert getattr(proto, s).restype is getattr(proto, twin).restype
    assert proto.bnn_hip_weight1x1_f4_bytes.restype is ctypes.c_size_t
    assert proto.bnn_hip_abi_version() == native.ABI_VERSION == 16
    assert re.search(r"#define\s+BNN_HIP_ABI_VERSION\s+16\b", text)


def test_the_switch_and_its_table():
    assert fastpath.MFMA_1X1 in ("0", "1", "all")
    for table in (fastpath.MFMA_1X1_SHAPES, fastpath.MFMA_1X1_TERNARY_SHAPES):
        for key, (pop_us, f4_us) in table.items():
            C, O, H, f32 = key
            assert C % 128 == 0 and O % 64 == 0 and H > 0 and isinstance(f32, bool), key
            assert f4_us < pop_us, "a listed shape measured faster"
    saved = fastpath.MFMA_1X1, fastpath.MFMA_CONV
    try:
        fastpath.MFMA_1X1 = "0"
        assert not fastpath.mfma_1x1_admitted(256, 64, 56, False)
        fastpath.MFMA_1X1 = "all"
        assert fastpath.mfma_1x1_admitted(256, 64, 56, False) and fastpath.mfma_1x1_admitted(512, 2048, 7, True)
        fastpath.MFMA_CONV = "0"
        assert not fastpath.mfma_1x1_admitted(256, 64, 56, False)
        fastpath.MFMA_CONV = saved[1]
        fastpath.MFMA_1X1 = "1"
        assert fastpath.mfma_1x1_admitted(256, 64, 56, False) == ((256, 64, 56, False) in fastpath.MFMA_1X1_SHAPES)
        assert fastpath.mfma_1x1_admitted(256, 64, 56, False, nonneg=False) == \
            ((256, 64, 56, False) in fastpath.MFMA_1X1_TERNARY_SHAPES)
        assert not fastpath.mfma_1x1_admitted(128, 64, 9, True) and not fastpath.mfma_1x1_admitted(128, 64, 9, True, False)
    finally:
        fastpath.MFMA_1X1, fastpath.MFMA_CONV = saved


# ------------------------------------------------------------------------------------------------------ the code object
@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = tmp_path_factory.mktemp("bconv1x1") / "k.s"
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", SRC, "-o", str(out)],
                   check=True, capture_output=True, timeout=600)
    return out.read_text()


def test_the_only_matrix_opcode_is_the_scaled_fp4_one(asm):
    """The source calls the builtin of v_mfma_scale_f32_16x16x128_f8f6f4 with both scales zero; the compiler prints that
    instruction without its (identity) scale operands, as v_mfma_f32_16x16x128_f8f6f4.  Either spelling is the one
    instruction; every use names E2M1 for both operands (cbsz:4 blgp:4)."""
    lines = re.findall(r"^\s*(v_(?:mfma|smfmac)\w+)(.*)$", asm, re.M)
    ops = {op for op, _ in lines}
    assert ops and ops <= {"v_mfma_scale_f32_16x16x128_f8f6f4", "v_mfma_f32_16x16x128_f8f6f4"}, ops
    assert all("cbsz:4" in rest and "blgp:4" in rest for _, rest in lines)


def test_no_kernel_spills(asm):
    """Scratch use would mean the accumulators or the double-buffered fragments left the register file."""
    sizes = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s*(\d+)", asm)]
    assert len(sizes) == 14 and not any(sizes), sizes

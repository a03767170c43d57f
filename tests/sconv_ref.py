"""numpy references of the convolution with binary activations and real weights (csrc/sconv.hip): the three-term bf16
split of the weight with its row exponent, the byte layout of the packed weight, the float64 convolution, the proof that a
case's sums are exact in fp32 and the tolerance of the cases whose sums are not.  No torch, no GPU."""
import numpy as np

from tests.grad_ref import sign0

F32, F64 = np.float32, np.float64


def _trunc_bf16(v):
    """The upper 16 bits of fp32 numbers: truncation to bf16, returned as fp32."""
    return (np.ascontiguousarray(v, F32).view(np.uint32) & np.uint32(0xFFFF0000)).view(F32)


def split_table():
    """The finite values every split must reproduce: both zeros, both ends of the subnormals, both neighbours of 1, a
    full 24-bit significand at four exponents (the lowest one where all 24 bits exist: 2^(-149+24) per unit would be
    subnormal below it) and the largest finite float — with both signs."""
    full = [F32((2 ** 24 - 1) * 2.0 ** e) for e in (-149 + 24, -24, 0, 100)]
    pos = [F32(0.0), F32(2.0 ** -149), np.nextafter(F32(2.0 ** -126), F32(0)), np.nextafter(F32(1), F32(0)),
           F32(1 + 2.0 ** -23)] + full + [np.finfo(F32).max]
    return np.array(pos + [-v for v in pos], F32)


def row_exp_ref(w):
    """kexp[o] of `w` [O, ...]: 1 - exponent of the row's largest |w| when that lies in (0, 1) — the scaled row's
    largest is then in [1, 2) — else 0 (NaN is skipped as fmaxf skips it; an infinite maximum is >= 1)."""
    a = np.abs(np.asarray(w, F32).reshape(len(w), -1))
    m = np.where(np.isnan(a), F32(0), a).max(axis=1) if a.shape[1] else np.zeros(len(w), F32)
    _, e = np.frexp(m)                        # m = f * 2^e, f in [0.5, 1); subnormals included
    return np.where((m > 0) & (m < 1), 1 - e, 0).astype(np.int32)


def split3_ref(w, kexp=None):
    """(hi, mid, lo, kexp) of fp32 `w`: the terms of w * 2^kexp (fp32 arrays whose low 16 bits are zero), each the
    truncation to bf16 of what is left, the remainders computed in fp32.  `kexp` None: every element is the largest of a
    row of its own (the table of the CPU test); else one exponent per leading index of `w`."""
    w = np.asarray(w, F32)
    if kexp is None:
        kexp = row_exp_ref(w.reshape(-1, 1)).reshape(w.shape)
        kb = kexp
    else:
        kexp = np.asarray(kexp, np.int32)
        kb = kexp.reshape((-1,) + (1,) * (w.ndim - 1))
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.ldexp(w, kb).astype(F32)
        hi = _trunc_bf16(v)
        r1 = (v - hi).astype(F32)
        mid = _trunc_bf16(r1)
        lo = _trunc_bf16((r1 - mid).astype(F32))
    return hi, mid, lo, kexp


def pack_bytes_ref(O, C, k):
    return ((C + 31) // 32) * k * k * ((O + 15) // 16) * 3 * 64 * 16 + ((O + 15) // 16) * 16 * 4


def sconv_fragments_ref(w):
    """The bytes of bnn_hip_sconv2d_pack_weight_f32 (include/bnn_hip.h):
    Wp[cb][tap][os][term][lane][e] = term(w[16 os + (lane & 15)][32 cb + 8 (lane >> 4) + e][tap] * 2^kexp[o]) as bf16,
    zero for pad channels, then kexp[16 OS] int32."""
    w = np.asarray(w, F32)
    O, C, k, _ = w.shape
    CB, OS, T = (C + 31) // 32, (O + 15) // 16, k * k
    kexp = np.zeros(16 * OS, np.int32)
    kexp[:O] = row_exp_ref(w)
    wp = np.zeros((16 * OS, 32 * CB, T), F32)
    wp[:O, :C] = w.reshape(O, C, T)
    terms = np.stack(split3_ref(wp, kexp)[:3])                              # [term][o][c][tap]
    bf = (terms.view(np.uint32) >> np.uint32(16)).astype(np.uint16)
    # o = 16 os + li, c = 32 cb + 8 lg + e, lane = 16 lg + li
    bf = bf.reshape(3, OS, 16, CB, 4, 8, T)                                  # [term][os][li][cb][lg][e][tap]
    bf = bf.transpose(3, 6, 1, 0, 4, 2, 5)                                   # [cb][tap][os][term][lg][li][e]
    return np.concatenate([np.ascontiguousarray(bf).view(np.uint8).reshape(-1), kexp.view(np.uint8)])


def out_shape(x_shape, O, stride):
    N, _, H, W = x_shape
    return N, O, (H - 1) // stride + 1, (W - 1) // stride + 1


def sconv_ref(x, w, bias=None, scale=None, stride=1):
    """(conv2d(s(x), w, padding k // 2, stride) + bias[o]) * scale[o] in float64; s(x) = +1 / -1 / 0 for x > 0 / x < 0 /
    anything else (sign0).  Non-finite weights propagate as IEEE products do (0 * inf = NaN)."""
    x, w = np.asarray(x), np.asarray(w, F64)
    O, C, k, _ = w.shape
    N, Cx, H, W = x.shape
    assert Cx == C and k in (1, 3)
    p = k // 2
    sx = np.zeros((N, C, H + 2 * p, W + 2 * p), F64)
    sx[:, :, p:p + H, p:p + W] = sign0(x)
    _, _, Ho, Wo = out_shape(x.shape, O, stride)
    y = np.zeros((N, O, Ho, Wo), F64)
    with np.errstate(invalid="ignore", over="ignore"):
        for ky in range(k):
            for kx in range(k):
                patch = sx[:, :, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride]
                y += np.einsum("nchw,oc->nohw", patch, w[:, :, ky, kx])
        if bias is not None:
            y = y + np.asarray(bias, F64)[None, :, None, None]
        if scale is not None:
            y = y * np.asarray(scale, F64)[None, :, None, None]
    return y


def assert_exact_inputs(w, bias=None):
    """Proof that every sum of the layer on these weights is exact in fp32 whatever the ternary operand and the order:
    all terms of an output channel (its weights and its bias) are multiples of one unit and sum |terms| / unit < 2^24.
    Returns the worst figure."""
    w = np.asarray(w, F64)
    O = w.shape[0]
    t = w.reshape(O, -1)
    if bias is not None:
        t = np.concatenate([t, np.asarray(bias, F64).reshape(O, 1)], axis=1)
    assert np.isfinite(t).all() and (t.astype(F32).astype(F64) == t).all()
    worst = 0.0
    for row in t:
        nz = np.abs(row[row != 0])
        if nz.size == 0:
            continue
        assert nz.min() >= 2.0 ** -100 and nz.max() < 2.0 ** 100, "too close to the fp32 range's ends"
        m, e = np.frexp(nz)                                   # nz = m * 2^e, m * 2^53 an integer
        mi = (m * 2.0 ** 53).astype(np.int64)
        tz = np.array([(int(v) & -int(v)).bit_length() - 1 for v in mi])
        unit = int((e - 53 + tz).min())                       # the lowest set bit of any term
        total = float(np.sum(nz / 2.0 ** unit))
        assert total < 2.0 ** 24, f"sum |terms| / unit = {total} >= 2^24"
        worst = max(worst, total)
    return worst


def tolerance(w, y64):
    """B[n,o,p] = 3 C k^2 2^-23 sum_{c,tap} |w[o,c,tap]| + 2^-22 |y64|: every product is exact, so the only error of
    the sum is the fp32 accumulation of at most 3 C k^2 terms in an unknown order (truncating adders allowed for: one
    2^-23 relative step per addition, each partial sum at most sum |w|); the second term is the bias add and the scale
    multiply, one rounding each (the cases keep |scale| <= 1, so the scaled accumulation error stays inside the first term)."""
    w = np.asarray(w, F64)
    O, C, k, _ = w.shape
    return 3.0 * C * k * k * 2.0 ** -23 * np.abs(w).reshape(O, -1).sum(1)[None, :, None, None] + 2.0 ** -22 * np.abs(y64)


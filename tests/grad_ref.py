"""Float64 / integer references of the dense gradient kernels (csrc/grad.hip) and of the weight hook of a training step
(csrc/xnor_train.hip), numpy on the CPU, pinned by tests/test_grad_ref_cpu.py against torch autograd in float64 and a
hand-written table.

Why the GPU results can be compared bit for bit (tests/test_gpu_grad_exact.py): the ternary operand is exact in bf16, a
value of at most 8 significant bits is its own first bf16 term, every product is exact in fp32, the accumulation is fp32.
If every term of a sum is an integer multiple of one power of two (`unit`) and sum |terms| / unit < 2^24, every partial sum
in any order is an fp32 number: the result has one right answer per bit.  The same holds for the double sums of the weight
hook with 2^53.  `assert_exact_inputs` / `assert_exact_weight_inputs` prove that for the inputs of a case, in integer
arithmetic; a case that violates it fails."""
import numpy as np

F32, F64 = np.float32, np.float64
BF16_ONE, BF16_MINUS_ONE = 0x3F80, 0xBF80


def sign0(a):
    """{-1, 0, +1} in float64; sign(+-0) = sign(NaN) = 0."""
    a = np.asarray(a)
    with np.errstate(invalid="ignore"):
        return np.where(a > 0, 1.0, np.where(a < 0, -1.0, 0.0))


def ste_mask(x):
    """1[|x| < 1]; NaN gives False."""
    with np.errstate(invalid="ignore"):
        return np.abs(np.asarray(x)) < 1


def _geometry(x_shape, ks, stride):
    N, C, H, W = x_shape
    return N, C, H, W, (H - 1) // stride + 1, (W - 1) // stride + 1, ks // 2


def _taps(H, W, Hg, Wg, ks, stride, pad):
    """Per tap (ky, kx): the slices of the g grid and of x that meet, y = yo * stride + ky - pad inside the image."""
    for ky in range(ks):
        for kx in range(ks):
            ys = [yo for yo in range(Hg) if 0 <= yo * stride + ky - pad < H]
            xs = [xo for xo in range(Wg) if 0 <= xo * stride + kx - pad < W]
            if ys and xs:
                gy, gx = slice(ys[0], ys[-1] + 1), slice(xs[0], xs[-1] + 1)
                yy = slice(ys[0] * stride + ky - pad, ys[-1] * stride + ky - pad + 1, stride)
                xx = slice(xs[0] * stride + kx - pad, xs[-1] * stride + kx - pad + 1, stride)
                yield ky, kx, gy, gx, yy, xx


def dgrad_ref(g, x, w_sign, alpha, ks, stride):
    """dL/dx = conv_backward_input(g, w_sign * alpha) * 1[|x| < 1] in float64: [N, C, H, W].  A NaN in x gives 0; masked
    positions (and sums that cancel) are +0."""
    g, w_sign, alpha = np.asarray(g, F64), np.asarray(w_sign, F64), np.asarray(alpha, F64)
    N, C, H, W, Hg, Wg, pad = _geometry(x.shape, ks, stride)
    O = g.shape[1]
    assert g.shape == (N, O, Hg, Wg) and w_sign.shape == (O, C, ks, ks) and alpha.shape == (O,)
    ga = np.ascontiguousarray((g * alpha[None, :, None, None]).transpose(0, 2, 3, 1))     # [N, Hg, Wg, O]
    out = np.zeros((N, H, W, C), F64)
    for ky, kx, gy, gx, yy, xx in _taps(H, W, Hg, Wg, ks, stride, pad):
        patch = np.ascontiguousarray(ga[:, gy, gx, :])                       # (contiguous operands: the BLAS path)
        out[:, yy, xx, :] += (patch.reshape(-1, O) @ np.ascontiguousarray(w_sign[:, :, ky, kx])).reshape(patch.shape[:3] + (C,))
    out = out.transpose(0, 3, 1, 2)
    return np.where(ste_mask(x), out, 0.0) + 0.0          # (+ 0.0: a -0 of the matrix product becomes +0)


def wgrad_ref(g, x, ks, stride, image_ranges):
    """One slab per image range (n0, n1) of dL/dWhat[o, c, ky, kx] = sum_{n, y, x} g[n, o, y, x] sign(x)[n, c, y s + ky - p,
    x s + kx - p] in float64: [len(image_ranges), O, C, ks, ks]."""
    g, sx = np.asarray(g, F64), sign0(x)
    N, C, H, W, Hg, Wg, pad = _geometry(x.shape, ks, stride)
    O = g.shape[1]
    assert g.shape == (N, O, Hg, Wg)
    out = np.zeros((len(image_ranges), ks, ks, O, C), F64)
    for ky, kx, gy, gx, yy, xx in _taps(H, W, Hg, Wg, ks, stride, pad):
        a = g[:, :, gy, gx].reshape(N, O, -1)                                   # [N, O, pixels] (copies: contiguous)
        b = np.ascontiguousarray(sx[:, :, yy, xx].reshape(N, C, -1).transpose(0, 2, 1))
        per_image = np.matmul(a, b)                                             # [N, O, C]
        for s, (n0, n1) in enumerate(image_ranges):
            out[s, ky, kx] = per_image[n0:n1].sum(0)
    return np.ascontiguousarray(out.transpose(0, 3, 4, 1, 2)) + 0.0


def split_ranges(N, splits):
    """The image ranges of launch_wgrad (csrc/grad.hip): per = ceil(N / splits) images per workgroup, the last ragged.
    `splits` is valid when ceil(N / per) == splits."""
    per = -(-N // splits)
    assert 1 <= splits <= N and -(-N // per) == splits, (N, splits)
    return [(n, min(N, n + per)) for n in range(0, N, per)]


def valid_splits(N):
    return [s for s in range(1, N + 1) if -(-N // -(-N // s)) == s]


def grad_fragments_ref(w_sign, O, C, ks):
    """The sign fragments the input-gradient kernel reads (the layout comment above grad_alpha_kernel in csrc/grad.hip and
    above xnor_grad_pack_kernel in csrc/xnor_train.hip), as bytes:
        Bp[ob][tap][cs][lane][e] = sign(W[o = 32 ob + 8 (lane >> 4) + e][c = 16 cs + (lane & 15)][tap])     (bf16)
    channels past O and C are zeros."""
    T, OB, CS = ks * ks, (O + 31) // 32, (C + 15) // 16
    s = sign0(np.asarray(w_sign, F64).reshape(O, C, T))
    code = np.zeros((OB * 32, CS * 16, T), np.uint16)
    code[:O, :C][s > 0] = BF16_ONE
    code[:O, :C][s < 0] = BF16_MINUS_ONE
    frag = code.reshape(OB, 4, 8, CS, 16, T).transpose(0, 5, 3, 1, 4, 2)        # [ob, tap, cs, lane >> 4, lane & 15, e]
    return np.ascontiguousarray(frag).astype("<u2").reshape(OB, T, CS, 64, 8).view(np.uint8).reshape(-1)


# ---- sums whose exactness is proven in integer arithmetic ------------------------------------------------------------
def _low_bit_exp(t):
    """Per element of the float64 array `t`: (e, tz) with |t| = M 2^(e - 53), M < 2^53 an integer with tz trailing zeros;
    zeros get e = tz = 0 and are flagged in the third result."""
    m, e = np.frexp(np.abs(t))
    M = np.ldexp(m, 53).astype(np.int64)
    zero = M == 0
    low = np.where(zero, 1, M & -M)
    tz = np.frexp(low.astype(F64))[1] - 1
    return M, e.astype(np.int64), tz.astype(np.int64), zero


def exact_sum(terms, axis, limit_bits, what, ratios=None):
    """sum(terms, axis) of finite float64 `terms`, computed in integers: unit = the largest power of two that divides every
    term of a sum, ints = terms / unit, the sum of the ints as Python integers.  Appends max sum |ints| to `ratios` (the
    figure that must stay below 2^limit_bits for every partial sum in any order to be exact) and returns the sum as
    float64, or raises when a single |term| / unit already reaches 2^limit_bits."""
    t = np.moveaxis(np.asarray(terms, F64), axis, -1)
    assert np.isfinite(t).all(), what
    M, e, tz, zero = _low_bit_exp(t)
    big = np.int64(1) << 40
    ue = np.where(zero, big, e - 53 + tz).min(-1, keepdims=True)              # log2(unit) per sum
    ue = np.where(ue == big, 0, ue)
    top = np.where(zero, -big, e - ue).max()
    if top > limit_bits:
        raise AssertionError(f"{what}: a term is >= 2^{int(top) - 1} units, the sums are not exact below 2^{limit_bits}")
    shift = np.where(zero, 0, e - 53 + tz - ue)
    ints = np.where(zero, 0, (M >> tz) << shift)                            # < 2^limit_bits <= 2^53
    ints = np.where(t < 0, -ints, ints)

    def total(v):
        hi, lo = v >> 27, v & ((1 << 27) - 1)                              # two limbs: no int64 overflow in the sum
        return (hi.sum(-1).astype(object) << 27) + lo.sum(-1).astype(object)
    mag = total(np.abs(ints))
    worst = max([0] + [int(v) for v in np.ravel(mag)])
    if ratios is not None:
        ratios.append((what, worst))
    s = total(ints)
    out = np.array([float(v) for v in np.ravel(s)], F64).reshape(s.shape)
    return np.ldexp(out, ue[..., 0].astype(np.int64))


def assert_exact_inputs(g, alpha, x_shape, ks, stride, image_ranges=None):
    """Proof, in integer arithmetic, that every accumulated sum of dgrad (terms g alpha sign(W)) and, with `image_ranges`,
    of wgrad (terms g sign(x)) on these inputs is exact in fp32: all terms are multiples of `unit` and sum |terms| / unit
    < 2^24 per output element (bounded from above with |sign| = 1 at every tap, so the proof holds for any ternary
    operand).  Also: g, alpha and g alpha are fp32 numbers and nothing underflows.  Returns the two worst figures."""
    g64, a64 = np.asarray(g, F64), np.asarray(alpha, F64)
    N, C, H, W, Hg, Wg, pad = _geometry(x_shape, ks, stride)
    O = g64.shape[1]
    assert g64.shape == (N, O, Hg, Wg) and np.isfinite(g64).all() and np.isfinite(a64).all()
    assert (g64.astype(F32).astype(F64) == g64).all() and (a64.astype(F32).astype(F64) == a64).all()
    ga = g64 * a64[None, :, None, None]                 # (two 24-bit significands: exact in float64)
    with np.errstate(over="ignore", under="ignore"):
        assert (ga.astype(F32).astype(F64) == ga).all(), "g * alpha is not exact in fp32"
    for v in (g64, ga):
        nz = np.abs(v[v != 0])
        assert nz.size == 0 or (nz.min() >= 2.0 ** -100 and nz.max() < 2.0 ** 100), "too close to the fp32 range's ends"

    def units(v):
        """(integers v / unit, unit) over the whole tensor"""
        M, e, tz, zero = _low_bit_exp(v)
        if zero.all():
            return np.zeros(v.shape, np.int64), 1.0
        ue = int(np.where(zero, np.int64(1) << 40, e - 53 + tz).min())
        assert int(np.where(zero, ue, e).max()) - ue <= 24, "a single term is >= 2^24 units"
        return np.where(zero, 0, (M >> tz) << np.where(zero, 0, e - 53 + tz - ue)), 2.0 ** ue
    # dgrad: an output pixel sums, over the taps, all O channels of the g pixels it meets
    ti, _ = units(ga)
    per_pixel = ti.sum(1)                                # [N, Hg, Wg] int64
    bound = np.zeros((N, H, W), np.int64)
    for ky, kx, gy, gx, yy, xx in _taps(H, W, Hg, Wg, ks, stride, pad):
        bound[:, yy, xx] += per_pixel[:, gy, gx]
    worst_d = int(bound.max())
    assert worst_d < 2 ** 24, f"dgrad: sum |terms| / unit = {worst_d} >= 2^24"
    worst_w = 0
    if image_ranges is not None:
        gi, _ = units(g64)
        for n0, n1 in image_ranges:                      # wgrad: an output element sums all pixels of all images of a split
            worst_w = max(worst_w, int(gi[n0:n1].sum((0, 2, 3)).max()))
        assert worst_w < 2 ** 24, f"wgrad: sum |terms| / unit = {worst_w} >= 2^24"
    return worst_d, worst_w


# ---- the weight hook: XNORWeightBinarizer forward value and backward (head of csrc/xnor_train.hip) --------------------
def _centre_and_alpha(w, center, compute_alpha, ratios):
    """(mean [O, 1, T] fp32, v = fp32(w - mean) [O, C, T], alpha [O] fp32): centre and alpha are float32(float64 sum /
    count), v is computed in float32."""
    O, C, T = w.shape
    with np.errstate(invalid="ignore"):
        if center:
            mean = np.full((O, 1, T), np.nan, F32)
            fin = np.isfinite(w).all(1)                                        # [O, T]: a NaN weight makes its tap's mean NaN
            s = exact_sum(np.where(fin[:, None, :], w, 0).astype(F64), 1, 53, "centre", ratios)
            mean[:, 0, :] = np.where(fin, (s / F64(C)).astype(F32), np.nan)
        else:
            mean = np.zeros((O, 1, T), F32)
        v = (w - mean).astype(F32)
        if not compute_alpha:
            return mean, v, np.ones(O, F32)
        a = np.abs(v).astype(F64).reshape(O, -1)
        fin = np.isfinite(a).all(1)
        s = exact_sum(np.where(fin[:, None], a, 0), 1, 53, "alpha", ratios)
        return mean, v, np.where(fin, (s / F64(C * T)).astype(F32), np.nan).astype(F32)


def _w3(w):
    w = np.asarray(w)
    assert w.dtype == F32 and w.ndim == 4
    return w.reshape(w.shape[0], w.shape[1], -1)


def xnor_what_ref(w, center, compute_alpha, ratios=None):
    """(What = sign(Wc) alpha as fp32 [O, C, kh, kw], alpha [O] fp32)."""
    w3 = _w3(w)
    _, v, alpha = _centre_and_alpha(w3, center, compute_alpha, ratios)
    with np.errstate(invalid="ignore"):
        what = sign0(v).astype(F32) * alpha[:, None, None]
    return what.reshape(w.shape), alpha


def alpha_ref(w, center, compute_alpha):
    """alpha[O] as the input-gradient kernel gets it from xnor_grad_pack_weight: the binarizer's alpha, or 0 for a channel
    whose signs are all 0 (the three-launch form's max |What|)."""
    _, v, alpha = _centre_and_alpha(_w3(w), center, compute_alpha, None)
    any_nz = (sign0(v) != 0).reshape(v.shape[0], -1).any(1)
    return np.where(any_nz, alpha, F32(0)).astype(F32)


def centred_weight_ref(w, center):
    """Wc = float32(w) - float32(mean) in float32, [O, C, kh, kw] (w itself when not centred)."""
    _, v, _ = _centre_and_alpha(_w3(w), center, False, None)
    return v.reshape(np.asarray(w).shape)


def centred_sign_ref(w, center):
    """sign(Wc) [O, C, kh, kw] in float64 (what grad_fragments_ref lays out for xnor_grad_pack_weight)."""
    _, v, _ = _centre_and_alpha(_w3(w), center, False, None)
    return sign0(v).reshape(np.asarray(w).shape)


def xnor_weight_backward_ref(w, dwhat, center, compute_alpha, ratios=None):
    """dL/dW [O, C, kh, kw] fp32 from dL/dWhat (w's shape, or slabs [splits, *w.shape], added in slab order in float32):
        dWc = dWhat alpha 1[|Wc| < 1] + sign(Wc) (sum dWhat sign(Wc)) / K      (compute_alpha; else dWhat 1[|Wc| < 1])
        dW  = dWc - mean_c(dWc) when centred, else dWc
    with Wc = float32(w) - float32(mean) in float32, every sum in float64, every quotient rounded to float32."""
    w3 = _w3(w)
    O, C, T = w3.shape
    d = np.asarray(dwhat)
    assert d.dtype == F32
    d = d.reshape((-1,) + w3.shape)
    dwo = d[0].copy()
    for s in range(1, d.shape[0]):
        dwo = (dwo + d[s]).astype(F32)
    _, v, alpha = _centre_and_alpha(w3, center, compute_alpha, ratios)
    sg = sign0(v).astype(F32)
    with np.errstate(invalid="ignore"):
        gk = np.zeros(O, F32)
        if compute_alpha:
            s = exact_sum((dwo.astype(F64) * sg).reshape(O, -1), 1, 53, "sum dWhat sign(Wc)", ratios)
            gk = (s / F64(C * T)).astype(F32)                                 # (a NaN weight has sign 0: the sum stays finite)
        ste = np.where(np.abs(v) < 1, (dwo * alpha[:, None, None]).astype(F32), F32(0)).astype(F32)
        dvc = (ste + (sg * gk[:, None, None]).astype(F32)).astype(F32)
        if not center:
            return (dvc - F32(0)).reshape(w.shape)
        fin = np.isfinite(dvc).all(1)
        s = exact_sum(np.where(fin[:, None, :], dvc, 0).astype(F64), 1, 53, "centre of dWc", ratios)
        dmean = np.where(fin, (s / F64(C)).astype(F32), np.nan).astype(F32)
        return (dvc - dmean[:, None, :]).astype(F32).reshape(w.shape)


def assert_exact_weight_inputs(w, dwhat, center, compute_alpha):
    """Proof, in integer arithmetic, that the double sums of xnor_what / xnor_weight_backward on these inputs are exact:
    per sum, all terms are multiples of `unit` and sum |terms| / unit < 2^53.  Also: the slab sum of `dwhat` is exact in
    float32 and dWhat alpha is exact in float32 (so that contracting `ste + sgn * gk` into an fma cannot change a bit).
    Returns {sum: worst figure}."""
    w3 = _w3(w)
    assert np.isfinite(w3).all(), "exactness is claimed for finite weights"
    ratios = []
    xnor_weight_backward_ref(w, dwhat, center, compute_alpha, ratios)
    worst = {}
    for what, r in ratios:
        worst[what] = max(worst.get(what, 0), r)
        assert r < 2 ** 53, f"{what}: sum |terms| / unit = {r} >= 2^53"
    d = np.asarray(dwhat, F64).reshape((-1,) + w3.shape)
    acc32, acc64 = d[0].astype(F32), d[0].copy()
    for s in range(1, d.shape[0]):
        acc32, acc64 = (acc32 + d[s].astype(F32)).astype(F32), acc64 + d[s]
        assert (acc32.astype(F64) == acc64).all(), "the slab sum rounds in float32"
    _, _, alpha = _centre_and_alpha(w3, center, compute_alpha, None)
    prod = acc64 * alpha.astype(F64)[:, None, None]
    assert (prod.astype(F32).astype(F64) == prod).all(), "dWhat * alpha is not exact in float32"
    return worst

"""numpy oracle of the 7x7 stem (csrc/stem_rows.hip, csrc/stem.hip, csrc/stem_wgrad.hip): float64 references, a
per-element error bound that is a function of the inputs only, numpy emulations of the three arithmetics, inputs on which
every arithmetic is exact (exact_grid) with value patterns planted on them, named wrong variants (MUTANTS), the host and
kernel rules that decide a launch's code paths restated once (paths), and the one table of cases (CASES).  No GPU and no
import of the library.

The bound.  u = 2^-24 is the relative error of one fp32 rounding to nearest.  An output of the convolution is a sum of
K = 147 products x_k * w_k.  An fp32 fmaf chain over them rounds once per term; each rounding is at most u times a partial
sum, and every partial sum is at most S = sum |x_k| |w_k| in magnitude (first order in u), so

    |fl32(conv) - conv| <= K * u * S = 147 * 2^-24 * (|x| conv |w|)          =: B32   (bound_fp32)

whatever the order of the chain.  The exact-fp32 kernel is such a chain.  The split arithmetic (`f16x3`) claims the same
class: it is held to B32 as well.  What it spends of it: hi + lo represents an operand to 2^-22 relative while lo is a
normal fp16 number (|lo| >= 2^-14), the dropped product lo * lo is at most 2^-22 |x w|, and the fp32 accumulation of the
three partial products adds a few u S: about 16 u S of the 147.  When lo is subnormal its error is ABSOLUTE, 2^-25: for a
weight of magnitude 2^-12 that is 2^-13 relative and the product has left the class.  weight_scale is the rule by which
the kernel keeps lo normal: a channel whose largest |w| is below 2^-5 is multiplied by the power of two that brings it
into [1, 2) before the split, and the fused per-channel multiplier by its inverse (both exact).  The image is not
rescaled: the bound holds for images whose largest magnitude is at most 2^15 (hi stays finite in fp16) and whose typical
magnitude is at least 2^-8 (X_SCALES; below that the lo halves of the PIXELS go subnormal).

`fp16` (one product of the rounded operands): each operand carries 2^-11, the chain its 147 u: held to the same form with
2^-11 in place of 2^-24 (bound_fp16).

The fused output is p = maxpool3x3/2/1(relu(fl32(fma(y, a, b)))).  The fma rounds once: an element before the pool is
within |a| B + u |a y + b|; relu is 1-Lipschitz and exact; |max s - max t| <= max |s - t|, so the bound of p is the
MAXIMUM of the element bounds over its window (bound_pooled).  The planes are sign(p); those behind pack_affine are the
planes of relu(fl32(fma(p, pa, pb))) (P = the value is positive, M = 0: a pre-activation block's bn1 + ReLU), and the
value is within |pa| bound(p) + u |pa p + pb| of the reference's (bound_affine).
A sign may differ from the float64 reference's only where the reference lies within its bound of zero.

The weight gradient is a sum of T = N * Hc * Wc products dy * x per weight: the same form with T terms (bound_wgrad; the
kernel adds fp32 partial sums of at most T terms in double and rounds once more, inside the T u S).
"""
import numpy as np

import oracle
from tests.golden import gen

F16, F32, F64 = np.float16, np.float32, np.float64
U, U16 = 2.0 ** -24, 2.0 ** -11
CIN, KS, COUT, K = 3, 7, 64, 147
X_SCALES = (-8, 15)          # admitted image scales: 2^-8 times a unit-variance image .. largest magnitude 2^15


def half(n):
    """Output extent of a stride-2 stage of the stem: conv 7/2/3 and MaxPool 3/2/1 alike."""
    return (n - 1) // 2 + 1


# ---------------------------------------------------------------------------------------------------- references
def cols(x, pad=3, shift=(0, 0)):
    """im2col of the convolution: float64 [N, 147, Hc, Wc], k = (c * 7 + ky) * 7 + kx (zero padding).  `pad` and `shift`
    (rows, columns added to every tap) exist for the mutants."""
    x = np.asarray(x, F64)
    N, C, H, W = x.shape
    Hc, Wc = half(H), half(W)
    m = 8
    xp = np.zeros((N, C, H + 2 * m + 8, W + 2 * m + 8))
    xp[:, :, m:m + H, m:m + W] = x
    out = np.empty((N, K, Hc, Wc))
    for c in range(CIN):
        for ky in range(KS):
            for kx in range(KS):
                y0, x0 = m - pad + ky + shift[0], m - pad + kx + shift[1]
                out[:, (c * KS + ky) * KS + kx] = xp[:, c, y0:y0 + 2 * Hc:2, x0:x0 + 2 * Wc:2]
    return out


def conv_ref(x, w):
    """conv 7x7 / stride 2 / pad 3, 3 -> 64, float64."""
    return np.einsum("nkhw,ok->nohw", cols(x), np.asarray(w, F64).reshape(COUT, K), optimize=True)


def pool_ref(z, fill=-np.inf):
    """MaxPool 3x3 / stride 2 / pad 1 of float64 [N, C, H, W] (padding = `fill`)."""
    N, C, H, W = z.shape
    Hp, Wp = half(H), half(W)
    zp = np.full((N, C, 2 * Hp + 2, 2 * Wp + 2), fill, F64)
    zp[:, :, 1:1 + H, 1:1 + W] = z
    out = np.full((N, C, Hp, Wp), -np.inf)
    for dy in range(3):
        for dx in range(3):
            out = np.maximum(out, zp[:, :, dy:dy + 2 * Hp:2, dx:dx + 2 * Wp:2])
    return out


def _ch(v):
    return np.asarray(v, F64).reshape(1, -1, 1, 1)


def planes_of(v):
    """Sign planes (P, M) of a float64 tensor, through the oracle's packer (the sign is taken in float64)."""
    return oracle.pack_act(np.sign(v).astype(F32))


def stem_ref(x, w, a, b):
    """(float64 pooled output, (P, M)) of conv -> a * y + b -> ReLU -> MaxPool(3, 2, 1)."""
    p = pool_ref(np.maximum(conv_ref(x, w) * _ch(a) + _ch(b), 0.0))
    return p, planes_of(p)


def affine_planes_ref(y, pa, pb):
    """Planes of relu(pa * y + pb) of a pooled output y (what pack_affine asks for: P = positive, M = 0), the sign taken
    in float64."""
    return planes_of(np.maximum(np.asarray(y, F64) * _ch(pa) + _ch(pb), 0.0))


def wgrad_ref(x, dy):
    """dW[o][c][ky][kx] = sum over n, y, x of dy * in (zero padding), float64 [64, 3, 7, 7]."""
    return np.einsum("nohw,nkhw->ok", np.asarray(dy, F64), cols(x), optimize=True).reshape(COUT, CIN, KS, KS)


# ---------------------------------------------------------------------------------------------------- bounds
def bound_fp32(x, w):
    return K * U * conv_ref(np.abs(x), np.abs(w))


def bound_fp16(x, w):
    return K * U16 * conv_ref(np.abs(x), np.abs(w))


def bound_pooled(x, w, a, b, conv_bound=bound_fp32):
    pre = conv_ref(x, w) * _ch(a) + _ch(b)
    return pool_ref(np.abs(_ch(a)) * conv_bound(x, w) + U * np.abs(pre), fill=0.0)


def bound_affine(x, w, a, b, pa, pb, conv_bound=bound_fp32):
    p = stem_ref(x, w, a, b)[0]
    return np.abs(_ch(pa)) * bound_pooled(x, w, a, b, conv_bound) + U * np.abs(p * _ch(pa) + _ch(pb))


def bound_wgrad(x, dy):
    T = dy.shape[0] * dy.shape[2] * dy.shape[3]
    s = np.einsum("nohw,nkhw->ok", np.abs(np.asarray(dy, F64)), cols(np.abs(x)), optimize=True)
    return (T * U * s).reshape(COUT, CIN, KS, KS)


# ---------------------------------------------------------------------------------------------------- emulations
def weight_scale(w):
    """The kernel's per-channel power of two (stem_rows.hip): 1 for a channel whose largest |w| is at least 2^-5 (or
    is zero or subnormal in fp32), else 2^(127 - biased exponent of that maximum), which brings it into [1, 2)."""
    m = np.abs(np.asarray(w, F32)).reshape(COUT, -1).max(1)
    e = (m.view(np.uint32) >> 23).astype(np.int64)
    return np.where((e >= 1) & (e <= 121), 2.0 ** (127 - e), 1.0)


def _split(v):
    v = np.asarray(v, F32)
    hi = v.astype(F16)
    lo = (v - hi.astype(F32)).astype(F16)
    return hi.astype(F64), lo.astype(F64)


def emulate(x, w, arith="f16x3", prescale=True, drop_lohi=False):
    """The convolution as the kernels' arithmetic gives it, fp32 [N, 64, Hc, Wc].
    f16x3: operands split into fp16 hi + lo as stem_rows.hip does (weights first multiplied by weight_scale, result
    divided back, with `prescale`), hi*hi + lo*hi + hi*lo with products and sum in float64 (the accumulation's own
    rounding comes on top).  fp16: hi*hi alone.  fp32: an fmaf chain in k order."""
    w2 = np.asarray(w, F32).reshape(COUT, K)
    c = cols(x).astype(F32)
    if arith == "fp32":
        acc = np.zeros((c.shape[0], COUT) + c.shape[2:], F32)
        for k in range(K):
            acc = (acc.astype(F64) + c[:, None, k].astype(F64) * w2[None, :, k, None, None].astype(F64)).astype(F32)
        return acc
    s = weight_scale(w) if prescale else np.ones(COUT)
    wh, wl = _split((w2.astype(F64) * s[:, None]).astype(F32))
    xh, xl = _split(c)
    out = np.einsum("nkhw,ok->nohw", xh, wh, optimize=True)
    if arith == "f16x3":
        out += np.einsum("nkhw,ok->nohw", xl, wh, optimize=True)
        if not drop_lohi:
            out += np.einsum("nkhw,ok->nohw", xh, wl, optimize=True)
    else:
        assert arith == "fp16"
    return (out / s[None, :, None, None]).astype(F32)


def emulate_stem(x, w, a, b, arith="f16x3", **kw):
    """The fused output as fp32 operations on the emulated convolution."""
    y = emulate(x, w, arith, **kw).astype(F64)
    return pool_ref(np.maximum((y * _ch(a) + _ch(b)).astype(F32), 0).astype(F64)).astype(F32)


# ---------------------------------------------------------------------------------------------------- host / kernel rules
PTH, PTW, WPW, ITH, NPC = 4, 14, 7, 23, 32          # stem_rows.hip: pooled tile, strip, patch rows, fetched column pairs
FETCH = ("pair_interior", "pair_edge", "scalar_odd_w", "scalar_rows", "scalar_misaligned")
TILE_LISTS = ("chunk_in_strip", "strips_round_robin")
WP_CLASSES, HP_CLASSES = (1, 6, 7, 8, 13, 14, 15), (1, 3, 4, 5, 9)
PATHS = FETCH + TILE_LISTS + tuple(f"Wp{v}" for v in WP_CLASSES) + tuple(f"Hp{v}" for v in HP_CLASSES) + \
    ("smallest", "batch_split")


def tile_list(N, H, W, cus=256):
    """(grid, seg_len, nseg, tiles_y, tiles_x) of launch_stem_rows_t."""
    Hp, Wp = half(half(H)), half(half(W))
    ty, tx = -(-Hp // PTH), -(-Wp // PTW)
    ntiles, want = N * ty * tx, 2 * cus
    grid = (ntiles + 7) // 8 * 8 if ntiles < want else want
    strips = N * tx
    if strips >= grid:
        return grid, ty, -(-strips // grid), ty, tx
    return grid, -(-ntiles // grid), 1, ty, tx


def paths(N, H, W, aligned=True, cus=256):
    """The code paths of stem_rows.hip a launch of this shape takes (names of PATHS)."""
    out = set()
    Hp, Wp = half(half(H)), half(half(W))
    grid, seg_len, nseg, tiles_y, tiles_x = tile_list(N, H, W, cus)
    pair = W % 2 == 0 and aligned
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            iy0, ixe = 4 * ty * PTH - 5, 4 * tx * PTW - 6
            rows_in = iy0 >= 0 and iy0 + ITH <= H
            if rows_in and pair and ixe >= 0 and ixe + 2 * NPC <= W:
                out.add("pair_interior")
            elif rows_in and pair:
                out.add("pair_edge")
            elif W % 2:
                out.add("scalar_odd_w")
            elif not aligned:
                out.add("scalar_misaligned")
            else:
                out.add("scalar_rows")
    if Wp in WP_CLASSES:
        out.add(f"Wp{Wp}")
    if Hp in HP_CLASSES:
        out.add(f"Hp{Hp}")
    if N * tiles_x >= grid:
        if nseg > 1 and (N * tiles_x) % grid:
            out.add("strips_round_robin")
    elif any((g * seg_len) % tiles_y for g in range(grid) if g * seg_len < N * tiles_y * tiles_x):
        out.add("chunk_in_strip")        # a workgroup's chunk starts below the top of a strip: it computes the kept row
    if (N, H, W) == (1, 1, 1):
        out.add("smallest")
    return out


# name -> ((N, H, W), aligned, unique images, the paths it is there for).  The entry points admit every N, H, W >= 1
# (capi.hip: only the byte sizes are limited; stem7x7_wgrad: rows up to ~950 pixels), so the smallest image is 1 x 1.
# `unique`: a large batch repeats that many images (the references are computed on those).
CASES = {
    "smallest":      ((1, 1, 1), True, None, ("smallest", "Hp1", "Wp1", "scalar_odd_w")),
    "hp1_wp6":       ((2, 3, 24), True, None, ("Hp1", "Wp6", "scalar_rows")),
    "hp3_wp7_odd":   ((2, 10, 27), True, None, ("Hp3", "Wp7", "scalar_odd_w")),
    "hp4_wp8":       ((1, 15, 30), True, None, ("Hp4", "Wp8", "scalar_rows")),
    "hp5_wp13":      ((2, 18, 50), True, None, ("Hp5", "Wp13")),
    "hp9_wp14_edge": ((1, 35, 56), True, None, ("Hp9", "Wp14", "pair_edge")),
    "hp5_wp15":      ((3, 20, 58), True, None, ("Hp5", "Wp15")),
    "interior":      ((1, 40, 114), True, None, ("pair_interior", "pair_edge", "scalar_rows")),
    "misaligned":    ((1, 40, 114), False, None, ("scalar_misaligned",)),
    "chunks":        ((1, 100, 20), True, None, ("chunk_in_strip",)),
    "round_robin":   ((600, 40, 10), True, 6, ("strips_round_robin",)),
    "batch_split":   ((3, 7, 9), True, None, ("batch_split",)),
}
MAX_INPUT_BYTES = 3 << 20


def check_cases():
    """Every path has a case that is there for it and reaches it; no case above the size limit."""
    covered = set()
    for name, ((N, H, W), aligned, unique, why) in CASES.items():
        assert N * 3 * H * W * 4 <= MAX_INPUT_BYTES, name
        reached = paths(N, H, W, aligned) | ({"batch_split"} if name == "batch_split" else set())
        assert set(why) <= reached, (name, set(why) - reached)
        covered |= set(why)
    assert covered == set(PATHS), set(PATHS) - covered
    return True


# ---------------------------------------------------------------------------------------------------- inputs
def _seed(*parts):
    return gen.seed_of("stem-edges", *parts)


def _ints(seed, shape, lo, hi):
    return np.floor(gen.uniform(seed, shape).astype(F64) * (hi - lo + 1) + lo).clip(lo, hi)


def exact_grid(shape, seed):
    """(x, w, a, b, pa, pb) on which every arithmetic of the stem is exact: x an integer in [-8, 8], w a multiple of 2^-6
    in [-1, 1], a (and pa) one of +-0.5, +-1, +-2 with negative channels, b (and pb) a multiple of 2^-6.  Every product is
    a multiple of 2^-6 and 147 of them stay below 2^11: 17 bits, exact in fp32 in any order; both operands are fp16
    numbers (lo = 0); a * y + b needs 20 bits.  Channels 5 and 37 can never be positive (b = -4096), channel 11 has zero
    weights and b = 0 (y == 0 exactly)."""
    N, H, W = shape
    x = _ints(seed, (N, CIN, H, W), -8, 8)
    w = _ints(seed + 1, (COUT, CIN, KS, KS), -64, 64) / 64.0
    mag = np.array([0.5, 1.0, 2.0])
    o = np.arange(COUT)
    a = mag[o % 3] * np.where(o % 5 == 2, -1.0, 1.0)
    b = _ints(seed + 2, (COUT,), -256, 256) / 64.0
    b[[5, 37]] = -4096.0
    w[11] = 0.0
    b[11] = 0.0
    pa = mag[(o + 1) % 3] * np.where(o % 4 == 1, -1.0, 1.0)
    pb = _ints(seed + 3, (COUT,), -512, 512) / 64.0
    return tuple(v.astype(F32) for v in (x, w, a, b, pa, pb))


def grid_dy(shape, seed):
    """An integer output gradient in [-4, 4] for the grid: N * Hc * Wc products of at most 32 stay below 2^24."""
    N, H, W = shape
    assert N * half(H) * half(W) * 32 < 2 ** 24
    return _ints(seed + 4, (N, COUT, half(H), half(W)), -4, 4).astype(F32)


def pattern_pixel_walk(seed):
    """147 images of 13 x 13 with ONE non-zero pixel each: image (c * 7 + ky) * 7 + kx holds it where tap (c, ky, kx)
    of conv output (3, 3) reads.  Grid weights."""
    x = np.zeros((K, CIN, 13, 13), F32)
    for k in range(K):
        c, ky, kx = k // 49, k // 7 % 7, k % 7
        x[k, c, 2 * 3 - 3 + ky, 2 * 3 - 3 + kx] = 1 + k % 8
    return (x,) + exact_grid((1, 13, 13), seed)[1:]


def pattern_single_weight(seed, j):
    """Grid image; channel o has ONE non-zero weight, at tap 64 * j + o (j = 0, 1, 2; no tap beyond 146)."""
    x, w, a, b, pa, pb = exact_grid((2, 18, 23), seed)
    w1 = np.zeros((COUT, K), F32)
    for o in range(COUT):
        if 64 * j + o < K:
            w1[o, 64 * j + o] = w.reshape(COUT, K)[o, 64 * j + o] or 0.5
    return x, w1.reshape(w.shape), a, b, pa, pb


def pattern_pool_positions():
    """Nine images of 10 x 13 (conv 5 x 7: the last window row and column are cut by the border, as the first are); the
    weight of every channel is 1 at the centre tap of input channel o % 3, so conv = x[2i, 2j]; image 3 dy + dx has the
    value 8 at conv position (2 py - 1 + dy, 2 px - 1 + dx) of the windows py in {0, 2}, px in {0, 3} (the four corner
    windows, each cut by two borders) where that position exists, and values <= 0 elsewhere: the only maximum of such a
    window sits at window position (dy, dx)."""
    H, W = 10, 13
    x = -_ints(_seed("pool"), (9, CIN, H, W), 0, 8)
    for d in range(9):
        dy, dx = d // 3, d % 3
        for py in (0, 2):
            for px in (0, 3):
                i, j = 2 * py - 1 + dy, 2 * px - 1 + dx
                if 0 <= i < half(H) and 0 <= j < half(W):
                    x[d, :, 2 * i, 2 * j] = 8
    w = np.zeros((COUT, CIN, KS, KS))
    w[np.arange(COUT), np.arange(COUT) % 3, 3, 3] = 1.0
    a, b = np.ones(COUT), np.zeros(COUT)
    a[1::4] = -1.0                                      # the maximum of -y sits elsewhere
    pa, pb = np.ones(COUT), -np.full(COUT, 4.0)
    return tuple(v.astype(F32) for v in (x, w, a, b, pa, pb))


def pattern_zero_image(seed):
    """Grid batch of three whose middle image is all zero."""
    t = exact_grid((3, 18, 27), seed)
    t[0][1] = 0.0
    return t


def real_inputs(name, kind, xscale=0):
    """(x, w, a, b, pa, pb, dy) of a case for the real-valued tests.  kind: normal | uniform | constant images (times
    2^xscale); Kaiming weights with channel o scaled by 2^-(o % 21); a of either sign and scaled back up as a BatchNorm
    behind the convolution would; pa, pb an affine of either sign."""
    (N, H, W), _, unique, _ = CASES[name]
    n = unique or N
    s = _seed(name, kind)
    if kind == "normal":
        x = gen.normal(s, (n, CIN, H, W))
    elif kind == "uniform":
        x = gen.uniform(s, (n, CIN, H, W))
    else:
        x = np.full((n, CIN, H, W), 0.7265625, F32) * np.array([1, -1.5, 0.25], F32).reshape(1, 3, 1, 1)
    x = (x.astype(F64) * 2.0 ** xscale).astype(F32)
    o = np.arange(COUT)
    w = gen.conv_weight("kaiming", s + 1, (COUT, CIN, KS, KS)).astype(F64) * (2.0 ** -(o % 21)).reshape(-1, 1, 1, 1)
    a = (0.5 + gen.uniform(s + 2, (COUT,))) * np.where(o % 7 == 0, -1.0, 1.0) * 2.0 ** (o % 21) * 2.0 ** -xscale
    b = 0.3 * gen.normal(s + 3, (COUT,))
    pa = (0.5 + gen.uniform(s + 4, (COUT,))) * np.where(o % 5 == 3, -1.0, 1.0)
    pb = 0.5 * gen.normal(s + 5, (COUT,))
    dy = gen.normal(s + 6, (n, COUT, half(H), half(W)))
    return tuple(np.ascontiguousarray(v, F32) for v in (x, w, a, b, pa, pb, dy))


def batch_index(name):
    """Which unique image each image of the case's batch is."""
    (N, _, _), _, unique, _ = CASES[name]
    return np.arange(N) % (unique or N)


# ---------------------------------------------------------------------------------------------------- mutants
def _mut_tap(x, w, a, b):
    return pool_ref(np.maximum(np.einsum("nkhw,ok->nohw", cols(x, shift=(0, 1)), np.asarray(w, F64).reshape(COUT, K))
                               * _ch(a) + _ch(b), 0.0))


def _mut_pad2(x, w, a, b):
    return pool_ref(np.maximum(np.einsum("nkhw,ok->nohw", cols(x, pad=2), np.asarray(w, F64).reshape(COUT, K))
                               * _ch(a) + _ch(b), 0.0))


def _mut_pool_edge(x, w, a, b):
    """The last window column and row stop one conv pixel early."""
    z = np.maximum(conv_ref(x, w) * _ch(a) + _ch(b), 0.0)
    p = pool_ref(z)
    Hc, Wc = z.shape[2:]
    if Wc > 1:
        p[..., -1] = pool_ref(z[..., :Wc - 1])[..., p.shape[3] - 1] if half(Wc - 1) == p.shape[3] else 0.0
    if Hc > 1:
        q = pool_ref(z[:, :, :Hc - 1])
        p[:, :, -1] = q[:, :, p.shape[2] - 1] if half(Hc - 1) == p.shape[2] else 0.0
    return p


def _mut_relu_after_pool(x, w, a, b):
    """NOT wrong: max and relu commute, so ReLU after the pool with a -inf border equals the reference (stem_rows.hip
    pools first).  Kept under EQUIVALENT so that the CPU test states it; the wrong neighbour is relu_dropped."""
    return np.maximum(pool_ref(conv_ref(x, w) * _ch(a) + _ch(b)), 0.0)


def _mut_zero_border_no_relu(x, w, a, b):
    """The -inf border and no ReLU at all: wrong wherever a whole window is negative."""
    return pool_ref(conv_ref(x, w) * _ch(a) + _ch(b))


def _mut_drop_lohi(x, w, a, b):
    y = emulate(x, w, "f16x3", drop_lohi=True).astype(F64)
    return pool_ref(np.maximum(y * _ch(a) + _ch(b), 0.0))


# name -> (function of (x, w, a, b) giving the pooled output, the input it is detected on: "grid" or "real")
MUTANTS = {
    "tap_shifted": (_mut_tap, "grid"),
    "pad2": (_mut_pad2, "grid"),
    "pool_edge": (_mut_pool_edge, "grid"),
    "relu_dropped": (_mut_zero_border_no_relu, "grid"),
    "lohi_dropped": (_mut_drop_lohi, "real"),
}
EQUIVALENT = {"relu_after_pool_inf_border": _mut_relu_after_pool}


def mut_affine_unpooled(x, w, a, b, pa, pb):
    """pack_affine applied to the un-pooled value, then pooled: differs where pa < 0."""
    z = np.maximum(conv_ref(x, w) * _ch(a) + _ch(b), 0.0)
    return planes_of(np.maximum(pool_ref(z * _ch(pa) + _ch(pb)), 0.0))


def mut_wgrad_offset(x, dy, shift):
    """The weight gradient with every tap read `shift` = (rows, columns) off."""
    return np.einsum("nohw,nkhw->ok", np.asarray(dy, F64), cols(x, shift=shift), optimize=True).reshape(COUT, CIN, KS, KS)

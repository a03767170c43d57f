"""The root oracle of the activation-plane producers (oracle.bn_act, avgpool2, bn_maxpool, pack_ste_mask, avgpool_ceil),
pinned on the CPU before tests/test_gpu_pack_family.py trusts it on the GPU: against ATen's CPU operators, against float64
compositions, and against a known-answer table written out by hand.  The GPU test plants the same table."""
import numpy as np
import torch
import torch.nn.functional as F

import oracle
from tests.golden import gen

P, M, Z = "P", "M", "-"             # the class of one packed element: P bit, M bit, or neither
NAN, INF = float("nan"), float("inf")
TINY = 2.0 ** -149                  # the smallest float32 denormal (np.float32(1e-45))
EPS12, EPS11 = 2.0 ** -12, 2.0 ** -11

# (name, x, a, b, class without ReLU, class with ReLU): v = fmaf(x, a, b) in float32; every value is an exact float32
AFFINE_CASES = [
    ("nan",               NAN,            1.0,            0.0,             Z, Z),
    ("inf-times-zero",    INF,            0.0,            0.0,             Z, Z),     # the product is NaN
    ("inf-negative-scale", INF,          -1.0,            0.0,             M, Z),
    ("zero-scale-plus0",  1.5,            0.0,            0.0,             Z, Z),
    ("zero-scale-minus0", 1.5,            0.0,           -0.0,             Z, Z),
    ("exact-zero",        3.0,            0.5,           -1.5,             Z, Z),
    # x a = 1 + 2^-11 + 2^-24 exactly: fmaf keeps the 2^-24; a rounded product is the tie 1 + 2^-11 and the sum 0
    ("fused-residue",     1.0 + EPS12,    1.0 + EPS12,   -(1.0 + EPS11),   P, P),
    ("denormal-result",   2.0 ** -100,    2.0 ** -49,     0.0,             P, P),     # 2^-149: lost if denormals flush
    ("underflow",         2.0 ** -100,    2.0 ** -51,     0.0,             Z, Z),
    ("underflow-tie",     2.0 ** -100,    2.0 ** -50,     0.0,             Z, Z),     # 2^-150 rounds to even: 0
    ("tiny-pos-pos",      TINY,           1.0,            0.0,             P, P),
    ("tiny-pos-neg",      TINY,          -1.0,            0.0,             M, Z),
    ("tiny-neg-pos",     -TINY,           1.0,            0.0,             M, Z),
    ("tiny-neg-neg",     -TINY,          -1.0,            0.0,             P, P),
]

# (name, (x00, x01, x10, x11), class of the 2x2 average in ATen's order (((x00 + x01) + x10) + x11) / 4)
WINDOW_CASES = [
    ("plus-zeros",        (0.0, 0.0, 0.0, 0.0),          Z),
    ("mixed-zeros",       (0.0, -0.0, -0.0, 0.0),        Z),
    ("cancel",            (1.0, -1.0, 0.0, 0.0),         Z),
    ("order",             (1e8, 1.0, -1e8, 0.0),         Z),     # column-first or pairwise: 1, so P
    ("inf-minus-inf",     (INF, -INF, 1.0, 1.0),         Z),
    ("nan",               (NAN, 1.0, 1.0, 1.0),          Z),
    ("inf",               (INF, 1.0, -1.0, 0.0),         P),
    ("underflow",         (TINY, 0.0, 0.0, 0.0),         Z),     # 2^-149 / 4 is 0: the SUM is positive, the average is not
    ("underflow-neg",     (-TINY, 0.0, 0.0, 0.0),        Z),
    ("four-tiny",         (TINY, TINY, TINY, TINY),      P),
]


def cls_of(v) -> str:
    v = np.float32(v)
    return P if v > 0 else M if v < 0 else Z


def plane_cls(Pw, Mw, n, c, y, x) -> str:
    """The class a pair of [N, cw64, H, W] uint64 planes holds for element (n, c, y, x)."""
    p = (int(Pw[n, c // 64, y, x]) >> (c % 64)) & 1
    m = (int(Mw[n, c // 64, y, x]) >> (c % 64)) & 1
    assert not (p and m)
    return P if p else M if m else Z


def same_f32(got, want) -> bool:
    """Bit for bit: the same float32 words, +0 and -0 told apart; a NaN matches a NaN (its payload is the machine's)."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]))


def affine_case_tensors():
    """One channel per planted affine case: x [1, C, 1, 1], a [C], b [C]."""
    x = np.array([c[1] for c in AFFINE_CASES], np.float32).reshape(1, -1, 1, 1)
    a = np.array([c[2] for c in AFFINE_CASES], np.float32)
    b = np.array([c[3] for c in AFFINE_CASES], np.float32)
    return x, a, b


def window_case_tensor():
    """One channel per planted window: [1, C, 2, 2]."""
    return np.array([c[1] for c in WINDOW_CASES], np.float32).reshape(1, -1, 2, 2)


# ---- the hand-written table against the C oracle ---------------------------------------------------------------------
def test_planted_values_are_exact_float32():
    for _, x, a, b, _, _ in AFFINE_CASES:
        for v in (x, a, b):
            assert np.isnan(v) or float(np.float32(v)) == v
    for name, w, _ in WINDOW_CASES:
        for v in w:
            assert np.isnan(v) or float(np.float32(v)) == v, name
    assert np.float32(1e-45) == np.float32(TINY) and np.float32(TINY) > 0


def test_affine_known_answers():
    x, a, b = affine_case_tensors()
    for relu in (False, True):
        v = oracle.bn_act(x, a, b, relu)
        Pw, Mw = oracle.pack_act(v)
        for c, case in enumerate(AFFINE_CASES):
            want = case[5] if relu else case[4]
            assert cls_of(v[0, c, 0, 0]) == want, (case[0], relu, v[0, c, 0, 0])
            assert plane_cls(Pw, Mw, 0, c, 0, 0) == want, (case[0], relu)
        assert not relu or not Mw.any()
    names = [c[0] for c in AFFINE_CASES]
    v = oracle.bn_act(x, a, b, False)[0, :, 0, 0]
    assert v[names.index("fused-residue")] == np.float32(2.0 ** -24)
    assert v[names.index("denormal-result")] == np.float32(TINY)
    assert np.isnan(v[names.index("inf-times-zero")]) and np.isnan(v[names.index("nan")])
    # ReLU keeps NaN
    assert np.isnan(oracle.bn_act(x, a, b, True)[0, names.index("nan"), 0, 0])
    # the case that tells fmaf from multiply-then-add does: the rounded product loses the residue
    i = names.index("fused-residue")
    two_step = np.float32(np.float32(x[0, i, 0, 0] * a[i]) + b[i])
    assert two_step == 0 and v[i] > 0


def test_window_known_answers():
    w = window_case_tensor()
    t2, tc = oracle.avgpool2(w), oracle.avgpool_ceil(w, 2)
    for c, (name, vals, want) in enumerate(WINDOW_CASES):
        assert cls_of(t2[0, c, 0, 0]) == want, (name, t2[0, c, 0, 0])
        assert cls_of(tc[0, c, 0, 0]) == want, (name, tc[0, c, 0, 0])
    # the order case does pin the order: column-first and pairwise sums are positive
    x00, x01, x10, x11 = (np.float32(v) for v in dict((n, v) for n, v, _ in WINDOW_CASES)["order"])
    assert ((x00 + x10) + x01) + x11 > 0 and (x00 + x10) + (x01 + x11) > 0
    # the underflow case does separate the sum from the average
    assert ((np.float32(TINY) + 0) + 0) + 0 > 0 and np.float32(TINY) * np.float32(0.25) == 0


# ---- against ATen on the CPU -----------------------------------------------------------------------------------------
def _with_windows(x):
    """x [N, C, H, W] with the planted windows in channels 0.. at the top-left 2x2 window."""
    x = x.copy()
    w = window_case_tensor()[0]
    n = min(len(w), x.shape[1])
    x[0, :n, :2, :2] = w[:n]
    return x


def _aten_avgpool2(x):
    """F.avg_pool2d(x, 2, 2) on the CPU.  One correction: where a negative average underflows to zero ATen's CPU kernel
    returns +0 and IEEE arithmetic -0 (a zero either way: no plane can tell); those zeros get the IEEE sign."""
    t = torch.from_numpy(x)
    want = F.avg_pool2d(t, 2, 2).numpy()
    with np.errstate(all="ignore"):
        exact = F.avg_pool2d(t.double(), 2, 2).numpy()       # no float64 sum of four float32 values underflows
    underflowed = (want == 0) & (exact < 0)
    want[underflowed] = np.float32(-0.0)
    return want


def test_avgpool2_is_atens_avg_pool2d_bit_for_bit():
    for shape, kind in (((2, 12, 6, 10), "special"), ((3, 5, 4, 2), "normal"), ((1, 70, 10, 14), "special")):
        x = _with_windows(gen.activation(kind, gen.seed_of("orc-avgpool2", shape), shape))
        x[-1, -1] *= np.float32(1e38)               # overflowing sums
        assert same_f32(oracle.avgpool2(x), _aten_avgpool2(x)), shape
    w = window_case_tensor()
    assert same_f32(oracle.avgpool2(w), _aten_avgpool2(w))


def test_avgpool_ceil_has_the_sign_of_atens_ceil_mode_pool():
    w = window_case_tensor()
    want = F.avg_pool2d(torch.from_numpy(w), 2, 2, ceil_mode=True, count_include_pad=False).numpy()
    Pw, Mw = oracle.pack_act(oracle.avgpool_ceil(w, 2))
    Pt, Mt = oracle.pack_act(want)
    assert np.array_equal(Pw, Pt) and np.array_equal(Mw, Mt)
    for c, (name, _, cls) in enumerate(WINDOW_CASES):
        assert cls_of(want[0, c, 0, 0]) == cls, name          # the table states what ATen computes
    for shape, k in (((2, 12, 9, 5), 2), ((1, 20, 13, 10), 3), ((2, 7, 3, 4), 5)):
        x = _with_windows(gen.activation("special", gen.seed_of("orc-ceil", shape), shape))
        want = F.avg_pool2d(torch.from_numpy(x), k, k, ceil_mode=True, count_include_pad=False).numpy()
        Pw, Mw = oracle.pack_act(oracle.avgpool_ceil(x, k))
        Pt, Mt = oracle.pack_act(want)
        assert np.array_equal(Pw, Pt) and np.array_equal(Mw, Mt), (shape, k)


def maxpool_input(seed, shape):
    """Normal data with +-inf, ties and all-negative windows, and no NaN and no -0 (max(+0, -0) has no stated sign)."""
    x = gen.normal(seed, shape)
    u = gen.uniform(seed + 1, shape)
    x[u < 0.03] = np.inf
    x[(u >= 0.03) & (u < 0.08)] = -np.inf
    x[(u >= 0.08) & (u < 0.2)] = np.float32(0.75)          # ties
    x[0, 0] = -np.abs(x[0, 0]) - 1                           # windows that are all negative
    x[-1, -1, :3, :3] = -np.inf                              # a window that holds nothing finite
    return x


MAXPOOL_GEOMETRIES = [(3, 2, 1), (2, 2, 0), (3, 1, 1)]


def test_bn_maxpool_without_batchnorm_is_atens_max_pool2d_bit_for_bit():
    for shape in ((2, 9, 7, 8), (1, 5, 9, 11), (2, 3, 8, 4)):
        x = maxpool_input(gen.seed_of("orc-maxpool", shape), shape)
        for k, s, p in MAXPOOL_GEOMETRIES:
            t = F.max_pool2d(torch.from_numpy(x), k, s, p)
            assert same_f32(oracle.bn_maxpool(x, None, None, False, k, s, p), t.numpy()), (shape, k, s, p)
            assert same_f32(oracle.bn_maxpool(x, None, None, True, k, s, p), torch.relu(t).numpy()), (shape, k, s, p)


def test_bn_maxpool_with_batchnorm_is_within_one_ulp_of_float64():
    shape = (2, 9, 9, 11)
    x = gen.normal(gen.seed_of("orc-bnmax", shape), shape)
    C = shape[1]
    a = ((0.5 + gen.uniform(3, (C,))) * np.where(np.arange(C) % 3 == 0, -1, 1)).astype(np.float32)
    b = (0.4 * gen.normal(4, (C,))).astype(np.float32)
    for k, s, p in MAXPOOL_GEOMETRIES:
        for relu in (False, True):
            v = torch.from_numpy(x).double() * torch.from_numpy(a).double().view(1, -1, 1, 1) + \
                torch.from_numpy(b).double().view(1, -1, 1, 1)
            want = F.max_pool2d(v, k, s, p)
            want = (torch.relu(want) if relu else want).numpy()
            got = oracle.bn_maxpool(x, a, b, relu, k, s, p)
            assert got.shape == want.shape
            ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
            assert np.all(np.abs(got.astype(np.float64) - want) <= ulp), (k, s, p, relu)


def test_bn_act_has_the_sign_of_the_float64_composition():
    shape = (3, 70, 9, 7)
    x = gen.normal(gen.seed_of("orc-bnact", shape), shape)
    C = shape[1]
    a = ((0.5 + gen.uniform(1, (C,))) * np.where(np.arange(C) % 4 == 0, -1, 1)).astype(np.float32)
    b = (0.4 * gen.normal(2, (C,))).astype(np.float32)
    for relu in (False, True):
        v = x.astype(np.float64) * a.astype(np.float64).reshape(1, -1, 1, 1) + b.astype(np.float64).reshape(1, -1, 1, 1)
        if relu:
            v = np.maximum(v, 0)
        got = oracle.bn_act(x, a, b, relu)
        assert np.array_equal(np.sign(got), np.sign(v).astype(np.float32))
        assert np.allclose(got, v, rtol=1e-6, atol=1e-7)
        assert same_f32(oracle.bn_act(x, None, None, relu), np.maximum(x, 0) if relu else x)


def test_ste_mask_is_abs_below_one():
    x = np.array([0.0, -0.0, 0.5, -0.5, 1.0, -1.0, np.nextafter(np.float32(1), np.float32(0)), NAN, INF, -INF, TINY, 2.0],
                 np.float32).reshape(1, -1, 1, 1)
    T = oracle.pack_ste_mask(x)
    bits = [(int(T[0, 0, 0, 0]) >> c) & 1 for c in range(x.shape[1])]
    assert bits == [1, 1, 1, 1, 0, 0, 1, 0, 0, 0, 1, 0]
    t = torch.from_numpy(x)
    kept = torch.ones_like(t).masked_fill(t.abs() >= 1, 0)[0, :, 0, 0].numpy()
    assert [int(v) for v in kept][:7] == bits[:7] and bits[7] == 0        # NaN: the project's convention (0)

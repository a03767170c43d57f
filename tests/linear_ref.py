"""Float64 / integer references of the binary Linear kernels (csrc/blinear.hip): forward, input gradient and the
per-split weight gradient of  out = F.linear(sign(x), sign(Wc) alpha) [+ bias] [* scale]  on a row-major [M, F] input,
numpy on the CPU.  They are the references of tests/grad_ref.py on the [M, F, 1, 1] view (a 1x1 convolution over 1x1
images) and `oracle.binary_linear_float`; tests/test_linear_ref_cpu.py pins them against torch autograd in float64.

A declared table of "exact" cases and their generator: dyadic g, alpha and weights for which `assert_exact_inputs` of
tests/grad_ref.py holds, so that every fp32 partial sum of the kernels in any order is exact and the GPU results have one
right answer per bit (tests/test_gpu_blinear.py compares on the int32 view)."""
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

import oracle
from tests import grad_ref as R
from tests.golden import gen

F32, F64 = np.float32, np.float64
split_ranges, valid_splits = R.split_ranges, R.valid_splits


def _4d(a):
    a = np.asarray(a)
    assert a.ndim == 2, a.shape
    return a[:, :, None, None]


def forward_ref(x, w, bias=None, post_scale=None, center=False, compute_alpha=True):
    """fp32 [M, O]: `oracle.binary_linear_float`."""
    return oracle.binary_linear_float(x, w, bias, post_scale, center=center, compute_alpha=compute_alpha)


def weight_sign_ref(w, center=False):
    """sign(Wc) [O, F] in float64."""
    return R.centred_sign_ref(_4d(np.asarray(w, F32)), center)[:, :, 0, 0]


def alpha_ref(w, center=False, compute_alpha=True):
    """alpha [O] fp32 as the weight pack holds it."""
    return R.alpha_ref(_4d(np.asarray(w, F32)), center, compute_alpha)


def dgrad_ref(g, x, w_sign, alpha):
    """gx [M, F] float64 = (sum_o g[m, o] alpha[o] sign(Wc)[o, f]) 1[|x[m, f]| < 1]; masked positions are +0."""
    return R.dgrad_ref(_4d(g), _4d(x), _4d(w_sign), alpha, 1, 1)[:, :, 0, 0]


def wgrad_ref(g, x, row_ranges):
    """One slab per row range: [len(row_ranges), O, F] float64 = sum over the rows of g[m, o] sign(x)[m, f]."""
    return R.wgrad_ref(_4d(g), _4d(x), 1, 1, row_ranges)[:, :, :, 0, 0]


def default_splits(M, O, F):
    """bnn_hip_blinear_grad_weight_splits (csrc/blinear.hip): ~1024 workgroups of 64 channels x 256 features in total, at
    least 32 rows per split, then made valid."""
    blocks = -(-O // 64) * -(-F // 256)
    s = max(1, min(-(-1024 // blocks), -(-M // 32), M))
    per = -(-M // s)
    return -(-M // per)


def assert_exact(g, alpha, x_shape, row_ranges=None):
    """`assert_exact_inputs` of tests/grad_ref.py on the 1x1 view: every sum of dgrad and (with `row_ranges`) of every
    wgrad slab is exact in fp32.  Raises AssertionError otherwise."""
    M, F = x_shape
    return R.assert_exact_inputs(_4d(g), alpha, (M, F, 1, 1), 1, 1, row_ranges)


# x values on both sides of zero and of the STE boundary; +-1 exactly (masked: |x| < 1 is false), the float below 1 (kept)
X_VALUES = np.array([0.0, -0.0, 0.5, -0.5, 1.0, -1.0, np.nextafter(F32(1), F32(0)), -np.nextafter(F32(1), F32(0)), 2.0, -2.0,
                     np.inf, -np.inf, 1e-45, -1e-45, np.nan], F32)


@dataclass(frozen=True)
class ExactCase:
    name: str
    M: int
    F: int
    O: int
    splits: Optional[Tuple[int, ...]] = None      # None: the library's default split only
    g_exp: int = 0                                # g = integers in [-7, 7] times 2^g_exp
    big_rows: Tuple[int, ...] = ()                # rows with |x| >= 1 everywhere
    one_rows: Tuple[int, ...] = ()                # rows with |x| == 1 exactly everywhere


EXACT_CASES = [
    ExactCase("m5_every_split", 5, 70, 33, splits=tuple(valid_splits(5)), big_rows=(1,), one_rows=(3,)),
    ExactCase("m7_every_split", 7, 10, 3, splits=tuple(valid_splits(7)), g_exp=-40, one_rows=(0,)),
    ExactCase("m130_default", 130, 100, 70, big_rows=(64,), one_rows=(129,)),
    ExactCase("m65_tails_scaled", 65, 300, 130, g_exp=20, big_rows=(0, 64)),
    ExactCase("m100_long_splits", 100, 64, 33, splits=(1, 2, 3), one_rows=(99,)),      # 100, 50 and 34 rows: several k-steps
]
EXACT_CASES_BY_NAME = {c.name: c for c in EXACT_CASES}


def _ints(seed, shape, lo, hi):
    return np.floor(gen.uniform(seed, shape) * (hi - lo + 1)).astype(np.int64) + lo


def exact_inputs(case: ExactCase):
    """(x [M, F] fp32, w [O, F] fp32, alpha [O] fp32, g [M, O] fp32) of an exact case: x from X_VALUES (with the case's rows
    of |x| >= 1 and |x| == 1), w from {0, +-0.5, +-1, +-2} (exact zeros included), alpha[o] = 2^-(o mod 5) with one 0, g small
    integers times a power of two."""
    seed = gen.seed_of("linear-exact", case.name)
    x = X_VALUES[_ints(seed, (case.M, case.F), 0, len(X_VALUES) - 1)]
    for r in case.big_rows:
        x[r] = np.where(_ints(seed + 5, (case.F,), 0, 1) == 1, F32(2.0), F32(-1.5))
    for r in case.one_rows:
        x[r] = np.where(_ints(seed + 6, (case.F,), 0, 1) == 1, F32(1.0), F32(-1.0))
    wv = np.array([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0], F32)
    w = wv[_ints(seed + 1, (case.O, case.F), 0, len(wv) - 1)]
    alpha = (2.0 ** -(np.arange(case.O) % 5)).astype(F32)
    alpha[case.O // 2] = 0.0
    g = (_ints(seed + 2, (case.M, case.O), -7, 7).astype(F64) * 2.0 ** case.g_exp).astype(F32)
    return x, w, alpha, g


def case_splits(case: ExactCase):
    return tuple(case.splits) if case.splits is not None else (default_splits(case.M, case.O, case.F),)

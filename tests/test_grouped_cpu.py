"""Grouped / depthwise binary convolutions, the parts that need no GPU: the windowed weight layout of the C-ABI against
its Python restatement, and the reference's grouped outputs (tests/golden/grouped.npz) against the CPU oracle applied
group by group — the decomposition the GPU tests (tests/test_gpu_grouped.py) rely on."""
import itertools
import os

import numpy as np
import pytest

import oracle
from bnn_amd import native
from tests.golden.grouped_cases import GROUPED_CASES
from tests.grouped_util import as_2d, layout, oracle_dot, oracle_float

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grouped.npz")


def _grid():
    for Cg, Og, G in itertools.product((1, 2, 3, 5, 8, 10, 12, 16, 20, 31, 32, 33, 48, 64, 100, 128),
                                       (1, 2, 3, 8, 16, 20, 31, 32, 33, 64, 96), (1, 2, 3, 4, 12, 40)):
        yield Cg * G, Og * G, G


def test_grouped_layout_matches_its_restatement():
    n = 0
    for C, O, G in _grid():
        for KH, KW in ((1, 1), (3, 3), (1, 7)):
            L = native.grouped_weight_layout(O, C, G, KH, KW)
            ref = layout(O, C, G, KH, KW)
            assert (L.cw32, L.cwc, L.nchunk, L.taps, L.o_pad, L.n_words) == \
                (ref["S"], ref["S"], 1, KH * KW, ref["o_pad"], ref["n_words"]), (O, C, G, KH, KW)
            n += 1
    assert n > 1000


def test_grouped_layout_window_sizes():
    """Depthwise is one word per tap; a group that fits a word is one word; windows never exceed the plane words."""
    assert native.grouped_weight_layout(256, 256, 256, 3, 3).cw32 == 1
    assert native.grouped_weight_layout(130, 130, 130, 3, 3).cw32 == 1
    assert native.grouped_weight_layout(96, 96, 12, 3, 3).cw32 == 1           # SepConv-like: 4 groups of 8 per block
    assert native.grouped_weight_layout(80, 40, 4, 3, 3).cw32 == 2            # BATS stem-like: Cg = 10, Og = 20
    assert native.grouped_weight_layout(144, 144, 12, 3, 3).cw32 == 3
    g1 = native.grouped_weight_layout(64, 200, 1, 3, 3)
    assert g1.cw32 == (200 + 31) // 32                                        # groups == 1: ceil(C / 32) words
    for C, O, G in _grid():
        assert native.grouped_weight_layout(O, C, G, 1, 1).cw32 <= 2 * ((C + 63) // 64)


def test_grouped_layout_rejects_bad_groups():
    lib = native.require()
    L = native.WLayout()
    import ctypes
    assert lib.bnn_hip_grouped_weight_layout(96, 96, 0, 3, 3, ctypes.byref(L)) == -1
    assert lib.bnn_hip_grouped_weight_layout(96, 100, 12, 3, 3, ctypes.byref(L)) == -1
    assert lib.bnn_hip_grouped_weight_layout(100, 96, 12, 3, 3, ctypes.byref(L)) == -1
    assert lib.bnn_hip_grouped_weight_layout(1 << 30, 1 << 30, 1 << 30, 3, 3, ctypes.byref(L)) == -4


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("case", GROUPED_CASES, ids=lambda c: c.name)
def test_fixture_equals_the_oracle_group_by_group(golden, case):
    x, w, b, sc = case.tensors()
    x2, w2, stride, pad, dil = as_2d(case, x, w)
    dot = oracle_dot(x2, w2, case.groups, stride, pad, dil, case.center)
    ref_dot = golden[case.name + "/dot"]
    assert np.array_equal(dot.reshape(ref_dot.shape), ref_dot)
    out = oracle_float(x2, w2, case.groups, b, sc, stride, pad, dil, case.center, case.compute_alpha)
    ref = golden[case.name + "/out"]
    out = out.reshape(ref.shape)
    assert np.allclose(out, ref, rtol=1e-3, atol=1e-5 * np.abs(ref).max())
    # and the emulated-integer route: the same dot through the oracle's fmaf epilogue
    alpha = np.concatenate([oracle.xnor_weight(w2[g * (case.O // case.groups):(g + 1) * (case.O // case.groups)],
                                               case.center, case.compute_alpha)[2] for g in range(case.groups)])
    e = oracle.epilogue(dot, alpha, b, sc).reshape(ref.shape)
    assert np.allclose(e, ref, rtol=1e-3, atol=1e-5 * np.abs(ref).max())

"""The public surface of ``bnn_amd.hipops`` against its recorded signatures (tests/golden/hipops_api.json, written by
tests/golden/make_hipops_api.py before the wrappers were restated), and the one place a batch is cut: ``_split`` and
``_desc_slices``."""
import inspect
import json
import os

import pytest

from bnn_amd import hipops, native


def test_every_recorded_public_name_keeps_its_signature(golden_dir):
    with open(os.path.join(golden_dir, "hipops_api.json")) as f:
        recorded = json.load(f)
    assert len(recorded) == 94
    missing = sorted(n for n in recorded if not hasattr(hipops, n))
    assert not missing, missing
    changed = {n: (sig, str(inspect.signature(getattr(hipops, n)))) for n, sig in recorded.items()
               if str(inspect.signature(getattr(hipops, n))) != sig}
    assert not changed, changed


def test_private_names_other_modules_use_are_still_there():
    for name in ("_batch_step", "_desc", "_hblock_desc", "_prefers_two_launches", "_require_cuda_f32"):
        assert callable(getattr(hipops, name)), name
    for name in ("_MAX_ELEMS", "_MAX_INDEX_FACTOR", "_MAX_DESC_BYTES", "_LINEAR_MAX_ELEMS", "_STEM3X3_MAX_ELEMS",
                 "_STEM_S2_MAX_ELEMS"):
        assert isinstance(getattr(hipops, name), int), name


@pytest.mark.parametrize("n, step, want", [
    (0, 1, []), (0, 5, []),                                  # an empty batch: no launch
    (3, 3, [(0, 3)]), (3, 8, [(0, 3)]), (1, 1, [(0, 1)]),    # step >= n: one slice
    (7, 3, [(0, 3), (3, 6), (6, 7)]),                        # a ragged tail: 3 + 3 + 1
    (6, 3, [(0, 3), (3, 6)]), (3, 1, [(0, 1), (1, 2), (2, 3)]),
])
def test_split(n, step, want):
    assert list(hipops._split(n, step)) == want


def _conv_desc(N):
    return hipops._desc((N, 8, 5, 7), (16, 8, 3, 3), 1, 1, 1, native.FLAG_WEIGHT_ZEROS)


def _fconv_desc(N):
    return native.FconvDesc(N, 48, 6, 7, 3, 2, native.FLAG_WEIGHT_ZEROS, 0)


@pytest.mark.parametrize("make", [_conv_desc, _fconv_desc], ids=["ConvDesc", "FconvDesc"])
def test_desc_slices_yields_copies_of_the_batch_runs(make):
    d = make(7)
    before = bytes(d)
    runs = list(hipops._desc_slices(d, 3))
    assert [(n0, n1) for n0, n1, _ in runs] == [(0, 3), (3, 6), (6, 7)]
    for n0, n1, dd in runs:
        assert type(dd) is type(d) and dd is not d and dd.N == n1 - n0
        for name, _ in d._fields_:
            assert name == "N" or getattr(dd, name) == getattr(d, name), name
        dd.N = 99                                            # a copy: writing it does not reach the original
    assert bytes(d) == before and d.N == 7
    assert list(hipops._desc_slices(make(0), 3)) == []
    (n0, n1, dd), = hipops._desc_slices(make(2), 5)
    assert (n0, n1, dd.N) == (0, 2, 2)

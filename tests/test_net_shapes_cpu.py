"""tests/net_shapes.py on the CPU: the conditions on the table's inputs (float32 against float64 stays inside the judge's
caps, and inside the ``D`` its header states), the judge against planted errors, and the plane unpacker against
``oracle.pack_act``."""
import functools

import numpy as np
import pytest
import torch

import oracle
from tests import net_shapes as ns
from tests.golden import gen


@functools.lru_cache(maxsize=None)
def _r32_against_r64(case):
    family, shape = case
    ref = ns.r64(case)
    r32 = ns.reference(ns.cpu_net(family), ns.input_of(shape), torch.float32)
    assert r32.names == ref.names
    return ns.judge(r32.values, r32.logits, ref)


# ---------------------------------------------------------------------------------------------- the table and its inputs
def test_the_table_is_the_one_the_header_describes():
    assert ns.B == 8 * ns.D and len(ns.CASES) == 30 and len(set(ns.CASES)) == 30
    assert [s[0] for s in ns.INPUTS] == [2, 2, 3, 5, 1, 2]


@pytest.mark.parametrize("family", list(ns.FAMILIES))
def test_stage_sizes(family):
    """The sizes the table promises: the output of layer1 .. layer4 for every input."""
    net = ns.cpu_net(family)
    for shape in ns.INPUTS:
        seen, hooks = [], []
        for stage in (net.layer1, net.layer2, net.layer3, net.layer4):
            hooks.append(stage.register_forward_hook(lambda m, i, o: seen.append(tuple(o.shape[2:]))))
        try:
            with torch.no_grad():
                y = net(ns.input_of(shape))
        finally:
            for h in hooks:
                h.remove()
        assert seen == ns.STAGES[shape] and y.shape == (shape[0], 1000)


@pytest.mark.parametrize("case", ns.CASES, ids=ns.case_id)
def test_float32_against_float64_stays_inside_the_caps_and_inside_d(case):
    v = _r32_against_r64(case)
    print(ns.case_id(case), v.report())
    assert not v.failures, v.failures
    assert v.logit_dev <= ns.LOGIT_TOL
    assert v.value_dev is not None and v.value_dev <= ns.D, v.value_dev


def test_at_most_one_image_in_four_diverges_over_the_whole_table():
    verdicts = [_r32_against_r64(case) for case in ns.CASES]
    images, diverged = sum(v.images for v in verdicts), sum(len(v.diverged) for v in verdicts)
    assert images == 5 * (2 + 2 + 3 + 5 + 1 + 2) and diverged <= ns.MAX_DIVERGED * images


# ------------------------------------------------------------------------------------------ the judge, planted errors
PLANT = ("basic_relu", (3, 3, 75, 61))


@pytest.fixture(scope="module")
def planted():
    ref = ns.r64(PLANT)
    name = "layer2.1.conv1"                 # a layer in the middle: relu output, 128 x 10 x 8 per image
    assert name in ref.names and ref.values[name].shape == (3, 128, 10, 8)
    return ref, name


def _flat_order(ref, name, image):
    """Element indices of one image's tensor, by |v64| ascending."""
    a = np.abs(ref.values[name][image]).ravel()
    return np.argsort(a, kind="stable"), a


def _flip(signs, name, image, flat_indices):
    s = signs[name][image].reshape(-1)      # a view: writes land in ``signs``
    for i in flat_indices:
        s[i] = 1 if s[i] <= 0 else -1
    return signs


def test_the_unchanged_reference_passes(planted):
    ref, _ = planted
    v = ns.judge(ref.all_signs(), ref.logits, ref)
    assert not v.failures and not v.diverged and v.logit_dev == 0.0


def test_one_ordinary_element_flipped_fails(planted):
    ref, name = planted
    order, a = _flat_order(ref, name, 1)
    mid = order[-len(order) // 4]           # the upper quartile of |v64|: an ordinary value
    assert a[mid] > 1e-2 * a.max()
    v = ns.judge(_flip(ref.all_signs(), name, 1, [mid]), ref.logits, ref)
    assert v.failures and v.diverged[1][:2] == (name, 1) and "knife edge" in v.failures[0]


def test_one_knife_edge_flipped_passes(planted):
    ref, name = planted
    order, a = _flat_order(ref, name, 1)
    assert a[order[0]] <= ns.B * a.max()
    v = ns.judge(_flip(ref.all_signs(), name, 1, order[:1]), ref.logits, ref)
    assert not v.failures and v.diverged == {1: (name, 1, a[order[0]] / a.max())}


def test_a_knife_edge_just_outside_the_bound_fails(planted):
    """The bound is B, not "small": the same element judged with a bound below its |v64| / max."""
    ref, name = planted
    order, a = _flat_order(ref, name, 2)
    first = order[np.nonzero(a[order] > 0)[0][0]]       # the smallest non-zero value
    ratio = a[first] / a.max()
    signs = _flip(ref.all_signs(), name, 2, [first])
    assert ns.judge(signs, ref.logits, ref, bound=0.5 * ratio).failures
    assert not ns.judge(signs, ref.logits, ref, bound=2 * ratio).failures


def test_five_knife_edges_of_one_image_fail(planted):
    ref, name = planted
    order, a = _flat_order(ref, name, 0)
    assert a[order[4]] <= ns.B * a.max()
    assert not ns.judge(_flip(ref.all_signs(), name, 0, order[:4]), ref.logits, ref).failures
    v = ns.judge(_flip(ref.all_signs(), name, 0, order[:5]), ref.logits, ref)
    assert len(v.failures) == 1 and "5 elements differ" in v.failures[0]


def test_a_layer_shifted_by_one_pixel_fails(planted):
    ref, name = planted
    signs = ref.all_signs()
    signs[name] = np.roll(signs[name], 1, axis=3)
    v = ns.judge(signs, ref.logits, ref)
    assert len(v.diverged) == 3 and all(d[0] == name and d[1] > ns.MAX_ELEMS for d in v.diverged.values())
    assert any("knife edge" in f for f in v.failures) and any("elements differ" in f for f in v.failures)


def test_only_the_first_diverging_layer_of_an_image_is_judged(planted):
    """Behind a knife edge decided the other way everything may differ: layers after it, and the logits, are not judged
    for that image — and still are for the others."""
    ref, name = planted
    order, _ = _flat_order(ref, name, 1)
    signs = _flip(ref.all_signs(), name, 1, order[:1])
    later = ref.names[ref.names.index(name) + 1]
    signs[later][1] = -signs[later][1]
    logits = ref.logits.copy()
    logits[1] += 1.0
    assert not ns.judge(signs, logits, ref).failures
    logits[2] += 1e-3 * np.abs(ref.logits).max()
    v = ns.judge(signs, logits, ref)
    assert len(v.failures) == 1 and v.failures[0].startswith("image 2: no differing sign")


def test_a_missing_layer_or_a_wrong_shape_fails(planted):
    ref, name = planted
    signs = ref.all_signs()
    del signs[name]
    assert ns.judge(signs, ref.logits, ref).failures
    signs = ref.all_signs()
    signs[name] = signs[name][:, :, :-1]
    assert ns.judge(signs, ref.logits, ref).failures


# -------------------------------------------------------------------------------------------------- the plane unpacker
@pytest.mark.parametrize("C", [3, 64, 70, 130])
def test_unpack_planes_inverts_the_oracle_packer(C):
    x = gen.activation("sparse", gen.seed_of("net-shapes-unpack", C), (2, C, 5, 7))       # -1, 0 and +1 all occur
    want = np.sign(x).astype(np.int8)
    assert set(np.unique(want)) == {-1, 0, 1}
    P, M = oracle.pack_act(x)
    assert P.shape == (2, (C + 63) // 64, 5, 7)
    got = ns.unpack_planes(P, M, C)
    assert got.dtype == torch.int8 and np.array_equal(got.numpy(), want)
    as_tensors = ns.unpack_planes(torch.from_numpy(P.view(np.int64)), torch.from_numpy(M.view(np.int64)), C)
    assert torch.equal(as_tensors, got)
    relu = np.maximum(x, 0)
    P, M = oracle.pack_act(relu)
    assert not M.any()
    garbage = np.full_like(M, np.uint64(0xFFFFFFFFFFFFFFFF))                                # a plane nobody may read
    assert np.array_equal(ns.unpack_planes(P, garbage, C, nonneg=True).numpy(), np.sign(relu).astype(np.int8))

"""tests/linear_ref.py pinned on the CPU: against torch autograd in float64 in the reference's own formulation
(F.linear(SignActivation(x), XNORWeightBinarizer(W)) of this package's `ops`), the exactness proofs of its case table, and
the host-side half of the Linear entry points (symbols, the split rule, the training plan's switches).
tests/test_gpu_blinear.py compares the HIP kernels of csrc/blinear.hip with these references."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import bnn_amd as bnn
from bnn_amd import fastpath, native, training
from bnn_amd.ops import BasicInputBinarizer, SignActivation, XNORWeightBinarizer
from tests import linear_ref as L
from tests.golden import gen

F32, F64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("bnn_hip_blinear_direct", "bnn_hip_blinear_grad_input_f32", "bnn_hip_blinear_grad_weight_f32",
               "bnn_hip_blinear_grad_weight_splits")


def _autograd(x, w, g, center, bias=None):
    """(y, dL/dx, dL/dWhat, What) of F.linear(SignActivation(x), XNORWeightBinarizer(W)) in float64."""
    xt = torch.from_numpy(np.asarray(x, F64)).requires_grad_(True)
    wt = torch.from_numpy(np.asarray(w, F64)).requires_grad_(True)
    w_hat = XNORWeightBinarizer(center_weights=center)(wt)
    w_hat.retain_grad()
    y = torch.nn.functional.linear(SignActivation.apply(xt), w_hat, None if bias is None else torch.from_numpy(bias.astype(F64)))
    y.backward(torch.from_numpy(np.asarray(g, F64)))
    return y.detach().numpy(), xt.grad.numpy(), w_hat.grad.numpy(), w_hat.detach().numpy()


@pytest.mark.parametrize("M,F,O,center", [(5, 70, 33, False), (7, 10, 3, True), (33, 130, 70, False), (1, 64, 1, True)])
def test_references_equal_autograd_in_float64(M, F, O, center):
    seed = gen.seed_of("linear-ref", M, F, O, center)
    x = (gen.normal(seed, (M, F)) * 0.9).astype(F32)
    x[0, : min(F, 4)] = [0.0, -0.0, 1.0, -1.0][: min(F, 4)]
    w = gen.normal(seed + 1, (O, F)).astype(F32)
    b = (0.1 * gen.normal(seed + 2, (O,))).astype(F32)
    g = gen.normal(seed + 3, (M, O)).astype(F64)
    y, gx, gwhat, what = _autograd(x, w, g, center, b)
    sgn = L.weight_sign_ref(w, center)
    alpha = np.abs(what).max(1)                                    # the float64 hook's own alpha
    assert np.array_equal(np.sign(what), sgn)
    assert np.allclose(L.forward_ref(x, w, b, None, center=center), y, rtol=1e-5, atol=1e-5 * np.abs(y).max())
    assert np.allclose(L.alpha_ref(w, center), alpha, rtol=1e-6)
    assert np.allclose(L.dgrad_ref(g, x, sgn, alpha), gx, rtol=1e-12, atol=1e-12)
    assert ((L.dgrad_ref(g, x, sgn, alpha) == 0) | (np.abs(x) < 1)).all()
    for splits in L.valid_splits(M):
        slabs = L.wgrad_ref(g, x, L.split_ranges(M, splits))
        assert slabs.shape == (splits, O, F)
        assert np.allclose(slabs.sum(0), gwhat, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("case", L.EXACT_CASES, ids=lambda c: c.name)
def test_exact_cases_pass_the_exactness_proofs(case):
    x, w, alpha, g = L.exact_inputs(case)
    assert x.shape == (case.M, case.F) and w.shape == (case.O, case.F) and g.shape == (case.M, case.O)
    assert (w == 0).any() and np.isnan(x).any() and (alpha == 0).sum() == 1
    for r in case.big_rows:
        assert (np.abs(x[r]) >= 1).all()
    for r in case.one_rows:
        assert (np.abs(x[r]) == 1).all()
    for splits in L.case_splits(case):
        worst_d, worst_w = L.assert_exact(g, alpha, x.shape, L.split_ranges(case.M, splits))
        assert worst_d < 2 ** 24 and worst_w < 2 ** 24
    # the references on exact inputs are fp32 numbers: the comparison on the int32 view has one right answer
    gx = L.dgrad_ref(g, x, L.weight_sign_ref(w), alpha)
    assert (gx.astype(F32).astype(F64) == gx).all()
    for splits in L.case_splits(case):
        slabs = L.wgrad_ref(g, x, L.split_ranges(case.M, splits))
        assert (slabs.astype(F32).astype(F64) == slabs).all()


def test_a_case_that_violates_a_proof_fails():
    case = L.EXACT_CASES_BY_NAME["m5_every_split"]
    x, w, alpha, g = L.exact_inputs(case)
    bad = g.copy()
    bad[0, 0] = F32(1.0) + F32(2.0 ** -23)                         # 24 significant bits next to multiples of 1: > 2^24 units
    bad[1, 0] = F32(2.0 ** 10)
    with pytest.raises(AssertionError):
        L.assert_exact(bad, alpha, x.shape, L.split_ranges(case.M, 1))
    with pytest.raises(AssertionError):
        L.assert_exact(g, (alpha * F32(1.0 / 3.0)).astype(F32), x.shape)     # g * alpha is not an fp32 number
    with pytest.raises(AssertionError):
        L.split_ranges(5, 4)                                       # 5 rows in 4 splits: ceil(5 / 2) = 3


def test_new_symbols_are_in_header_exports_and_bindings_with_abi_16():
    text = open(os.path.join(ROOT, "include", "bnn_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = native.require()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, code), f"{s} is not declared in include/bnn_hip.h"
        assert s in native.EXPORTED_SYMBOLS and getattr(lib, s).argtypes, s
    assert lib.bnn_hip_abi_version() == native.ABI_VERSION == 16
    assert re.search(r"#define\s+BNN_HIP_ABI_VERSION\s+16\b", text)
    # bnn_hip_blinear keeps its signature
    assert len(native._PROTOTYPES["bnn_hip_blinear"][1]) == 13


def _binary_linear(F=70, O=33):
    cfg = bnn.BConfig(activation_pre_process=BasicInputBinarizer, activation_post_process=bnn.Identity,
                      weight_pre_process=XNORWeightBinarizer)
    return bnn.prepare_binary_model(nn.Linear(F, O), cfg).train()


def test_plan_linear_train_declines_with_the_flag_off_and_under_autocast(monkeypatch):
    layer = _binary_linear()
    x = torch.zeros(4, 70, requires_grad=True)
    # the device half of the rule (fp32 on one HIP device, autograd recording) is `_eligible_train`; taken as given here
    monkeypatch.setattr(fastpath, "_eligible_train", lambda layer, x: True)
    monkeypatch.setattr(training, "LINEAR", True)
    plan = fastpath.plan_linear_train(layer, x)
    assert plan is not None and plan.ste and plan.compute_alpha and not plan.center and plan.scale is None
    monkeypatch.setattr(training, "LINEAR", False)
    assert fastpath.plan_linear_train(layer, x) is None            # off (the default: read at every call)
    monkeypatch.setattr(training, "LINEAR", True)
    was = torch.is_autocast_enabled()
    torch.set_autocast_enabled(True)
    try:
        assert fastpath.plan_linear_train(layer, x) is None        # under autocast the composition runs
    finally:
        torch.set_autocast_enabled(was)
    handle = layer.weight_pre_process.register_forward_hook(lambda m, i, o: o)
    assert fastpath.plan_linear_train(layer, x) is None            # a hook on the weight binarizer would not fire
    handle.remove()
    assert fastpath.plan_linear_train(layer, x) is not None
    assert "linear_train" in fastpath.stats()
    # without a HIP device the real rule declines and the layer runs the composition
    monkeypatch.undo()
    monkeypatch.setattr(training, "LINEAR", True)
    assert fastpath.plan_linear_train(layer, x) is None
    before = fastpath.stats()["linear_train"]
    assert layer(x).shape == (4, 33) and fastpath.stats()["linear_train"] == before


def test_weight_gradient_entry_point_refuses_an_invalid_split_on_the_host():
    lib = native.require()
    p = 1 << 20                                                    # aligned, never dereferenced: the refusal comes first
    for M, splits in ((5, 4), (5, 0), (5, 6), (7, 5), (7, 6), (7, -1)):
        assert splits not in L.valid_splits(M)
        assert lib.bnn_hip_blinear_grad_weight_f32(p, p, p, p, splits, M, 3, 10, None) == native.ERR_INVALID_ARG, (M, splits)
    assert lib.bnn_hip_blinear_grad_weight_f32(p, p, p, p, 1, 0, 3, 10, None) == native.ERR_INVALID_ARG
    assert lib.bnn_hip_blinear_grad_weight_f32(None, p, p, p, 1, 5, 3, 10, None) == native.ERR_INVALID_ARG
    assert lib.bnn_hip_blinear_grad_weight_f32(p, p + 4, p, p, 1, 5, 3, 10, None) == native.ERR_INVALID_ARG   # plane alignment
    assert lib.bnn_hip_blinear_grad_weight_f32(p, p, p, p, 1, 1 << 20, 3, 1 << 12, None) == native.ERR_TOO_LARGE
    # the default split is a valid one and equals the reference's statement of it
    for M, O, F in ((5, 33, 70), (7, 3, 10), (130, 70, 100), (8192, 1024, 1024), (50176, 3072, 768), (33, 10, 130)):
        s = lib.bnn_hip_blinear_grad_weight_splits(M, O, F)
        per = -(-M // s)
        assert s == L.default_splits(M, O, F) and 1 <= s <= M and -(-M // per) == s, (M, O, F, s)
    assert lib.bnn_hip_blinear_grad_weight_splits(0, 3, 10) == native.ERR_INVALID_ARG

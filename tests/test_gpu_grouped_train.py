"""Grouped binary convolutions in a training step on the HIP path (csrc/grad_grouped.hip, training.GROUPED): the two
gradient kernels through hipops against a float64 oracle, the drop-in layer with the switch on against its own torch
composition evaluated in float64 (bnn/layers/conv.py:90-97 with the STE of bnn/ops.py:63-73), the BATS cell operations
in train() mode with the switch on against the switch off, and one whole cell taking a training step.

Tolerances are those of tests/test_gpu_training.py: y and gx  rtol 1e-4, atol 1e-5 max|ref|;  parameter gradients
rtol 1e-3, atol 1e-4 max|ref| + 1e-7.

One convention differs from torch and is the project's own (include/bnn_hip.h, bnn_hip_pack_act_ste_f32: "T = |x| < 1
(NaN -> 0)"; csrc/grad.hip does the same for dense layers): a NaN INPUT element gets gradient +0.0, where
``masked_fill(x.abs() >= 1, 0)`` lets the gradient through.  Only the case with act="special" holds NaN; there the
comparison with the float64 composition covers every other element and the NaN positions must be exactly +0.0."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import bnn_amd as bnn
from bnn_amd import fastpath, hipops, models, training
from bnn_amd.native import NativeError
from bnn_amd.ops import BasicInputBinarizer, BasicScaleBinarizer, XNORWeightBinarizer
from tests.golden import cells_cases, gen
from tests.golden.cellops_cases import CELL_CASES as OP_CASES
from tests.golden.grouped_cases import GROUPED_CASES, GroupedCase

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

CASES_2D = [c for c in GROUPED_CASES if not c.conv1d]
# rows wider than a wave; BATS-like stride 2 / dilation 2 with five images (uneven split over 3 slabs)
WIDE = GroupedCase("w70_g2", 1, 8, 3, 70, 8, 2, 3, 3, pad=(1, 1))
SPLIT = GroupedCase("n5_g12_s2_d2", 5, 24, 6, 6, 24, 12, 3, 3, stride=2, pad=(2, 2), dilation=2)
K2 = GroupedCase("k2x2_g4", 2, 16, 7, 7, 16, 4, 2, 2, pad=(1, 1))          # four taps: the weight gradient's small tap tile
KERNEL_CASES = CASES_2D + [WIDE, SPLIT, K2]


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def close(a, ref, rtol=1e-4, afac=1e-5, aabs=0.0):
    a, ref = a.detach().cpu(), ref.detach().cpu().to(torch.float64)
    atol = afac * float(ref.abs().max()) + aabs
    ok = bool(torch.allclose(a.to(torch.float64), ref, rtol=rtol, atol=atol))
    if not ok:
        print("max |a - ref| =", float((a.to(torch.float64) - ref).abs().max()), "atol =", atol, "max|ref| =", float(ref.abs().max()))
    return ok


def close_param(a, ref):
    return close(a, ref, rtol=1e-3, afac=1e-4, aabs=1e-7)


@pytest.fixture
def grouped_on():
    old = training.GROUPED
    training.GROUPED = True
    try:
        yield
    finally:
        training.GROUPED = old


def _layer(case, w, b, sc):
    """The drop-in binary layer of a 2-D case (prepare_binary_model on the float module), on the GPU, train mode."""
    conv = nn.Conv2d(case.C, case.O, (case.kh, case.kw), stride=case.stride, padding=case.pad, dilation=case.dilation,
                     groups=case.groups, bias=case.bias)
    conv.weight.data.copy_(torch.from_numpy(w))
    if b is not None:
        conv.bias.data.copy_(torch.from_numpy(b))
    cfg = bnn.BConfig(activation_pre_process=BasicInputBinarizer,
                      activation_post_process=BasicScaleBinarizer if case.post == "scale" else bnn.Identity,
                      weight_pre_process=XNORWeightBinarizer.with_args(compute_alpha=case.compute_alpha,
                                                                       center_weights=case.center))
    layer = bnn.prepare_binary_model(conv, cfg)
    if sc is not None:
        layer.activation_post_process.alpha.data.copy_(torch.from_numpy(sc).view(1, -1, 1, 1))
    return layer.to(DEV).train()


def planted(x):
    """The case's input with exact +1.0, -1.0, +0.0 and -0.0 planted (the edges of sign() and of the mask |x| < 1)."""
    x = np.array(x, np.float32, copy=True)
    flat = x.reshape(-1)
    for i, v in enumerate((1.0, -1.0, 0.0, -0.0)):
        flat[3 + i::29] = np.float32(v)
    return x


def geometry(case):
    return (case.groups, (case.stride, case.stride), tuple(case.pad), (case.dilation, case.dilation))


def supported(case):
    G, s, p, d = geometry(case)
    return hipops.grouped_grad_supported(case.xshape, case.wshape, G, s, p, d)


def test_the_rule_accepts_the_bats_geometries_and_most_cases():
    got = {c.name: supported(c) for c in CASES_2D}
    assert sum(got.values()) >= 9, got
    assert not got["g2_cg128_dil2"]                       # 128 channels per group
    assert supported(WIDE) and supported(SPLIT)


# ---- the kernels against the float64 oracle --------------------------------------------------------------------------
def kernel_oracle(x, what, g, case):
    """gx and gWhat in float64: autograd of conv2d on sign(x), masked by T = |x| < 1 (NaN -> masked)."""
    G, s, p, d = geometry(case)
    x = x.cpu()
    xs = torch.sign(x).double().requires_grad_()
    w64 = what.cpu().double().requires_grad_()
    y = F.conv2d(xs, w64, None, s, p, d, G)
    gx, gw = torch.autograd.grad(y, (xs, w64), g.cpu().double())
    return gx.masked_fill(~(x.abs() < 1), 0), gw


@pytest.mark.parametrize("case", KERNEL_CASES, ids=[c.name for c in KERNEL_CASES])
def test_gradient_kernels_against_the_float64_oracle(case):
    xn, wn, _, _ = case.tensors()
    x, w = dev(planted(xn)), dev(wn)
    G, s, p, d = geometry(case)
    sv = hipops.pack_act_ste(x)
    what = hipops.xnor_what(w, case.center, case.compute_alpha)
    ho, wo = hipops.conv_out_hw(case.H, case.W, case.kh, case.kw, s, p, d)
    g1 = dev(gen.normal(gen.seed_of("grouped-train-g", case.name), (case.N, case.O, ho, wo)))
    if not supported(case):
        with pytest.raises(NativeError, match="unsupported"):
            hipops.bconv_grouped_grad_input(g1, sv, what, G, s, p, d)
        with pytest.raises(NativeError, match="unsupported"):
            hipops.bconv_grouped_grad_weight(g1, sv, w.shape, G, s, p, d)
        return
    masked = ~(x.abs() < 1)
    assert bool(masked.any()) and bool((~masked).any())
    for scale in (1.0, 1e-6):
        g = (g1 * scale).contiguous()
        ref_gx, ref_gw = kernel_oracle(x, what, g, case)
        gx = hipops.bconv_grouped_grad_input(g, sv, what, G, s, p, d)
        assert torch.equal(gx, hipops.bconv_grouped_grad_input(g, sv, what, G, s, p, d))        # bit-reproducible
        assert close(gx, ref_gx)
        assert bool((gx[masked] == 0).all()) and not bool(torch.signbit(gx[masked]).any())        # exactly +0.0
        slabs = hipops.bconv_grouped_grad_weight(g, sv, w.shape, G, s, p, d, reduce=False)
        assert torch.equal(slabs, hipops.bconv_grouped_grad_weight(g, sv, w.shape, G, s, p, d, reduce=False))
        assert 1 <= slabs.shape[0] <= case.N and tuple(slabs.shape[1:]) == tuple(w.shape)
        assert close_param(slabs.sum(0), ref_gw)
        assert close_param(hipops.bconv_grouped_grad_weight(g, sv, w.shape, G, s, p, d), ref_gw)


@pytest.mark.parametrize("splits", [1, 3])
def test_weight_gradient_slabs_with_an_uneven_image_split(splits):
    case = SPLIT
    xn, wn, _, _ = case.tensors()
    x, w = dev(planted(xn)), dev(wn)
    G, s, p, d = geometry(case)
    sv = hipops.pack_act_ste(x)
    what = hipops.xnor_what(w, case.center, case.compute_alpha)
    ho, wo = hipops.conv_out_hw(case.H, case.W, case.kh, case.kw, s, p, d)
    for scale in (1.0, 1e-6):
        g = dev(gen.normal(77, (case.N, case.O, ho, wo))) * scale
        slabs = hipops.bconv_grouped_grad_weight(g, sv, w.shape, G, s, p, d, reduce=False, splits=splits)
        assert slabs.shape[0] == splits
        assert torch.equal(slabs, hipops.bconv_grouped_grad_weight(g, sv, w.shape, G, s, p, d, reduce=False, splits=splits))
        assert close_param(slabs.sum(0), kernel_oracle(x, what, g, case)[1])
        if splits == 3:     # slab s holds the images [s N / 3, (s + 1) N / 3): 1, 2 and 2 of the five
            for i, (n0, n1) in enumerate(((0, 1), (1, 3), (3, 5))):
                only = torch.zeros_like(g)
                only[n0:n1] = g[n0:n1]
                assert close_param(slabs[i], kernel_oracle(x, what, only, case)[1])
    with pytest.raises(NativeError):
        hipops.bconv_grouped_grad_weight(g, sv, w.shape, G, s, p, d, splits=case.N + 1)


# ---- the drop-in layer, switch on, against its float64 composition ---------------------------------------------------
def layer_run(layer, x, g):
    for q in layer.parameters():
        q.grad = None
    xa = x.clone().requires_grad_()
    y = layer(xa)
    y.backward(g.to(y.dtype))
    return y.detach(), xa.grad, {n: q.grad for n, q in layer.named_parameters()}


def check_layer(case, binary_grads):
    xn, wn, bn_, scn = case.tensors()
    layer = _layer(case, wn, bn_, scn)
    ref = copy.deepcopy(layer).double().cpu()
    x = dev(xn)
    G, s, p, d = geometry(case)
    ho, wo = hipops.conv_out_hw(case.H, case.W, case.kh, case.kw, s, p, d)
    g = dev(gen.normal(gen.seed_of("grouped-train-layer", case.name), (case.N, case.O, ho, wo)))
    yr, gxr, pr = layer_run(ref, x.double().cpu(), g.double().cpu())
    before, _ = fastpath.stats()["conv2d_train"], training.saved_input_bytes(reset=True)
    old = training.BINARY_GRADS
    training.BINARY_GRADS = binary_grads
    try:
        y, gx, pg = layer_run(layer, x, g)
    finally:
        training.BINARY_GRADS = old
    assert fastpath.stats()["conv2d_train"] == before + 1
    kept = training.saved_input_bytes(reset=True)
    if binary_grads and supported(case):
        assert kept == 3 * 8 * case.N * ((case.C + 63) // 64) * case.H * case.W          # P, M and T: nothing else of x
    else:
        assert kept == 4 * x.numel()
    assert y.dtype == torch.float32 and close(y, yr)
    nan_in = torch.isnan(x)
    if binary_grads and supported(case) and bool(nan_in.any()):     # (module docstring: NaN inputs are masked)
        assert bool((gx[nan_in] == 0).all()) and not bool(torch.signbit(gx[nan_in]).any())
        gx, gxr = gx.masked_fill(nan_in, 0), gxr.masked_fill(nan_in.cpu(), 0)
    assert close(gx, gxr)
    assert set(pg) == set(pr) and "weight" in pg
    assert (case.bias) == ("bias" in pg) and (case.post == "scale") == ("activation_post_process.alpha" in pg)
    for name in pr:
        assert pg[name] is not None and close_param(pg[name], pr[name]), name


@pytest.mark.parametrize("case", CASES_2D, ids=[c.name for c in CASES_2D])
def test_layer_with_the_switch_on_against_the_float64_composition(grouped_on, case):
    check_layer(case, binary_grads=True)


@pytest.mark.parametrize("case", CASES_2D, ids=[c.name for c in CASES_2D])
def test_layer_with_the_library_backward_forced(grouped_on, case):
    check_layer(case, binary_grads=False)


# depthwise, a ragged batch (three images), every pixel of the 5 x 5 image within one tap of the border
DW_SMALL = GroupedCase("dw16_n3_5x5", 3, 16, 5, 5, 16, 16, 3, 3, pad=(1, 1))


@pytest.mark.parametrize("fused", [True, False], ids=["fused_hook", "torch_hook"])
def test_layer_with_and_without_the_fused_weight_hook(grouped_on, monkeypatch, fused):
    """``training.FUSED_WEIGHT_HOOK`` off: ``What = weight_pre_process(W)`` is made by torch under autograd and the grouped
    gradient kernels return dL/dWhat (slabs summed) instead of feeding ``xnor_weight_backward``."""
    hook_kernel = []
    real = hipops.xnor_weight_backward
    monkeypatch.setattr(hipops, "xnor_weight_backward", lambda *a: hook_kernel.append(1) or real(*a))
    monkeypatch.setattr(training, "FUSED_WEIGHT_HOOK", fused)
    assert supported(DW_SMALL)
    check_layer(DW_SMALL, binary_grads=True)
    assert len(hook_kernel) == (1 if fused else 0)


def test_the_switch_is_off_by_default_and_read_at_every_call(monkeypatch):
    assert training.GROUPED is (os.environ.get("BNN_AMD_TRAIN_GROUPED", "0") == "1")      # off unless the environment asks
    case = GROUPED_CASES[1]
    xn, wn, bn_, scn = case.tensors()
    layer = _layer(case, wn, bn_, scn)
    x = dev(xn).requires_grad_()
    monkeypatch.setattr(training, "GROUPED", False)
    before = fastpath.stats()["conv2d_train"]
    layer(x)
    assert fastpath.stats()["conv2d_train"] == before
    monkeypatch.setattr(training, "GROUPED", True)
    layer(x)
    assert fastpath.stats()["conv2d_train"] == before + 1
    monkeypatch.setattr(training, "GROUPED", False)
    layer(x)
    assert fastpath.stats()["conv2d_train"] == before + 1


# ---- the BATS cell operations in train() mode: switch on against switch off ------------------------------------------
def binarise(m):
    cfg = bnn.BConfig(activation_pre_process=BasicInputBinarizer, activation_post_process=bnn.Identity,
                      weight_pre_process=XNORWeightBinarizer)
    return bnn.prepare_binary_model(m, cfg)


def build(case):
    m = binarise(case.build(models))
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict({k: torch.from_numpy(v) for k, v in case.state(shapes).items()})
    return m.to(DEV).train()


GROUPED_OPS = [c for c in OP_CASES if c.kind in ("SepConv", "DilConv")]


@pytest.mark.parametrize("case", GROUPED_OPS, ids=[c.name for c in GROUPED_OPS])
def test_cell_operation_in_training_mode_switch_on_against_switch_off(case):
    """Both sides are the same fp32 module on the GPU and run the same torch BatchNorm on the same input, so no sign()
    decision can differ between them.  One other decision could: the PReLU behind the convolution has its kink at 0, and
    7-15 % of these convolutions' outputs ARE 0 (an even number of +-alpha[o] terms whose integer dot is 0).  The HIP
    forward returns alpha * 0 = +0.0 there; the library's fp32 sum of +-alpha[o] leaves a residue of a few 1e-9 of
    either sign (float64 does too, at 1e-17), and a positive residue takes the PReLU's other slope in the backward.  The
    reference side therefore has that residue removed: an output below alpha[o] / 2 (a non-zero dot gives at least
    alpha[o]) is set to exactly 0 with its gradient passed through unchanged."""
    off, on = build(case), build(case)
    conv = off.op[1]
    half_alpha = 0.5 * conv.weight_pre_process(conv.weight).detach().abs().amax(dim=(1, 2, 3)).view(1, -1, 1, 1)
    removed = []

    def drop_residue(mod, inp, out):
        r = out.detach() * (out.detach().abs() < half_alpha)
        removed.append(r.abs().amax(dim=(0, 2, 3)))
        return out - r
    conv.register_forward_hook(drop_residue)
    x = dev(case.input())
    g = None
    res = []
    previous = training.GROUPED
    for m, flag in ((off, False), (on, True)):
        training.GROUPED = flag
        try:
            before = fastpath.stats()["conv2d_train"]
            xa = x.clone().requires_grad_()
            y = m(xa)
            if g is None:
                g = dev(gen.normal(case.seed + 5, tuple(y.shape)))
            y.backward(g)
            res.append((y.detach(), xa.grad, fastpath.stats()["conv2d_train"] - before))
        finally:
            training.GROUPED = previous
    (y0, gx0, n0), (y1, gx1, n1) = res
    assert n0 == 0 and n1 == 1
    # what was removed is summation residue, not a forward error: an fp32 sum of n = Cg KH KW terms +-alpha[o] whose
    # partial sums stay below n alpha[o] is off by at most n^2 2^-24 alpha[o] (each of n additions rounds by 2^-24 of it)
    n_terms = conv.weight[0].numel()
    assert len(removed) == 1 and bool((removed[0] <= n_terms * n_terms * 2.0 ** -24 * 2 * half_alpha.view(-1)).all())
    assert close(y1, y0) and close(gx1, gx0)
    for (name, p0), (_, p1) in zip(off.named_parameters(), on.named_parameters()):
        assert p0.grad is not None and p1.grad is not None and close_param(p1.grad, p0.grad), name
    for (name, b0), (_, b1) in zip(off.named_buffers(), on.named_buffers()):
        assert torch.equal(b0, b1), name                                   # BatchNorm running statistics, bit for bit


# ---- a cell trains ---------------------------------------------------------------------------------------------------
def test_a_cell_takes_a_training_step_and_returns_to_the_fused_executor(grouped_on):
    """No element-wise comparison here: behind the first BatchNorm of the cell a rounding may flip a sign(), so two
    correct paths may differ in single elements by a whole unit.  What is checked: the step runs on the grouped HIP path
    (counter), loss and gradients are finite, and eval() afterwards is FusedCell again on the updated weights."""
    case = cells_cases.CELL_CASES[0]
    cell = binarise(case.build(models))
    shapes = {k: tuple(v.shape) for k, v in cell.state_dict().items()}
    cell.load_state_dict({k: torch.from_numpy(v) for k, v in case.state(shapes).items()})
    cell = cell.to(DEV)
    s0, s1 = (dev(a) for a in case.inputs())
    cell.eval()
    with torch.no_grad():
        c0 = fastpath.stats()["cell"]
        y_before = cell(s0, s1, 0.0).clone()
        assert fastpath.stats()["cell"] == c0 + 1

    cell.train()
    ran = {"grouped": 0, "dense": 0}
    hooks = [m.register_forward_hook(lambda mod, i, o: ran.__setitem__("grouped" if mod.groups > 1 else "dense",
                                                                       ran["grouped" if mod.groups > 1 else "dense"] + 1))
             for m in cell.modules() if isinstance(m, torch.nn.Conv2d) and hasattr(m, "activation_pre_process")]
    training.GROUPED = False            # the same forward without the switch: only the dense layers take conv2d_train
    before = fastpath.stats()["conv2d_train"]
    cell(s0.clone().requires_grad_(), s1.clone().requires_grad_(), 0.0)
    dense = fastpath.stats()["conv2d_train"] - before
    training.GROUPED = True
    ran.update(grouped=0, dense=0)
    before = fastpath.stats()["conv2d_train"]
    a0, a1 = s0.clone().requires_grad_(), s1.clone().requires_grad_()
    loss = cell(a0, a1, 0.0).square().mean()
    loss.backward()
    for h in hooks:
        h.remove()
    assert ran["grouped"] >= 4
    assert fastpath.stats()["conv2d_train"] - before == dense + ran["grouped"]     # rose by the grouped convolutions
    assert bool(torch.isfinite(loss))
    for name, q in cell.named_parameters():
        assert q.grad is not None and bool(torch.isfinite(q.grad).all()), name
    assert bool(torch.isfinite(a0.grad).all()) and bool(torch.isfinite(a1.grad).all())

    with torch.no_grad():
        for q in cell.parameters():
            q.add_(q.grad, alpha=-0.05)
    cell.eval()
    with torch.no_grad():
        c0 = fastpath.stats()["cell"]
        y_after = cell(s0, s1, 0.0)
        assert fastpath.stats()["cell"] == c0 + 1
        assert bool(torch.isfinite(y_after).all()) and not torch.equal(y_after, y_before)   # weights re-derived

"""The binary Linear kernels of csrc/blinear.hip on the GPU: the row-major forward against today's route (a 1x1 convolution
over 1x1 images) on the int32 view, its bit-plane by-product against pack_act_ste, the two gradient kernels against
tests/linear_ref.py bit for bit on the exact table and against the torch composition on random data, the dispatch under
`training.LINEAR`, the operator's autograd formula, and three SGD steps of a binary MLP."""
import dataclasses

import numpy as np
import pytest
import torch
import torch.nn as nn

import bnn_amd as bnn
from bnn_amd import fastpath, hipops, native, training
from bnn_amd.ops import BasicInputBinarizer, BasicScaleBinarizer, XNORWeightBinarizer
from tests import linear_ref as L
from tests.golden import gen
from tests.golden.cases import LINEAR_CASES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
SPECIALS = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1e-45, -1e-45, 1e-39, -1e-39, 1.0, -1.0], F32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def close(a, b):   # the fixture tolerance of tests/test_gpu_parity.py / tests/test_oracle_cpu.py
    scale = max(1.0, float(np.nanmax(np.abs(b))))
    return np.allclose(a, b, rtol=1e-3, atol=1e-5 * scale, equal_nan=True)


def _inputs(M, F, O, half, bias, scale, zeros, seed):
    x = gen.normal(seed, (M, F)).astype(F32)
    idx = np.floor(gen.uniform(seed + 1, (M, F)) * 4 * len(SPECIALS)).astype(np.int64)
    x = np.where(idx < len(SPECIALS), SPECIALS[np.minimum(idx, len(SPECIALS) - 1)], x).astype(F32)   # a quarter specials
    w = gen.normal(seed + 2, (O, F)).astype(F32)
    if zeros:
        w[gen.uniform(seed + 3, (O, F)) < 0.2] = 0.0
    b = (0.1 * gen.normal(seed + 4, (O,))).astype(F32) if bias else None
    s = (0.5 + gen.uniform(seed + 5, (O,))).astype(F32) if scale else None
    xt = dev(x).half() if half else dev(x)
    return xt, dev(w), None if b is None else dev(b), None if s is None else dev(s)


def _through_blinear_entry(x, pw, b, s):
    """pack_act + bnn_hip_blinear: the pre-packed form of today's route."""
    M, F = x.shape
    act = hipops.pack_act(x[:, :, None, None])
    out = torch.empty((M, pw.shape[0]), device=DEV)
    native.check(native.require().bnn_hip_blinear(
        M, F, pw.shape[0], act.P.data_ptr(), act.M.data_ptr(), pw.wbits.data_ptr(), pw.wnz.data_ptr(), int(pw.has_zero),
        pw.alpha.data_ptr(), None if b is None else b.data_ptr(), None if s is None else s.data_ptr(), out.data_ptr(),
        torch.cuda.current_stream().cuda_stream), "bnn_hip_blinear")
    return out


# (M, F, O, fp16, bias, post-scale, center, zero weights, LDS pass words): every tail of M (64-row tiles), F (chunks of 2 / 4 /
# 8 / 16 words, a ragged last word, two full chunks + a ragged word at F = 138 and 1506) and O (32-channel blocks); the
# plans of the kernel: one LDS pass (0), one pass per chunk, a ragged last pass (32 of 48 words), 8 waves (F = 2200: more
# than 32 KB of planes), more than one channel block per wave (M = 4737 x O = 1000).
FORWARD = [
    (1, 10, 3, False, False, False, False, False, 0),
    (3, 64, 33, True, True, False, False, False, 0),
    (65, 70, 70, False, True, True, True, False, 0),
    (130, 100, 1000, False, False, True, False, True, 0),
    (130, 250, 3, True, True, False, False, True, 0),
    (65, 138, 33, False, True, False, False, False, 0),
    (65, 138, 33, False, True, False, False, True, 2),
    (3, 1506, 70, False, True, True, False, False, 0),
    (3, 1506, 70, False, True, True, True, False, 16),
    (3, 1506, 70, True, False, False, False, True, 32),
    (3, 2200, 33, True, True, True, False, False, 0),
    (4737, 70, 1000, False, True, True, False, False, 0),
]


@pytest.mark.parametrize("M,F,O,half,bias,scale,center,zeros,lds_words", FORWARD,
                         ids=lambda v: str(int(v)) if not isinstance(v, bool) else "ny"[v])
def test_forward_and_planes_equal_todays_route_bit_for_bit(M, F, O, half, bias, scale, center, zeros, lds_words):
    x, w, b, s = _inputs(M, F, O, half, bias, scale, zeros, gen.seed_of("blinear-fwd", M, F, O))
    pw = hipops.pack_weight(w, center, True)
    assert pw.has_zero == zeros
    want = hipops.bconv2d_direct(x[:, :, None, None], pw, b, s)[:, :, 0, 0]
    assert same_bits(_through_blinear_entry(x, pw, b, s), want)
    got = hipops.blinear_direct(x, pw, b, s, lds_words=lds_words)
    assert same_bits(got, want)
    got2, sv = hipops.blinear_direct(x, pw, b, s, want_planes=True, lds_words=lds_words)
    assert same_bits(got2, want) and sv.shape == (M, F, 1, 1)
    ref = hipops.pack_act_ste(x.float()[:, :, None, None])
    for name, a, r in (("P", sv.sign.P, ref.sign.P), ("M", sv.sign.M, ref.sign.M), ("T", sv.T, ref.T)):
        assert a.shape == r.shape == (M, (F + 63) // 64, 1, 1) and torch.equal(a, r), name    # pad bits included
    assert sv.nbytes() == 3 * 8 * M * ((F + 63) // 64)


@pytest.mark.parametrize("case", LINEAR_CASES, ids=lambda c: c.name)
def test_forward_is_close_to_the_reference_fixtures(case, golden_layers):
    x, w, b, sc = case.tensors()
    pw = hipops.pack_weight(dev(w), case.center, True)
    bt, st = (None if b is None else dev(b)), (None if sc is None else dev(sc))
    out = hipops.blinear_direct(dev(x), pw, bt, st)
    assert close(out.cpu().numpy(), golden_layers["linear/" + case.name + "/out"])
    assert same_bits(out, hipops.linear(dev(x), pw, bt, st, route="conv"))
    assert same_bits(out, hipops.linear(dev(x), pw, bt, st))                  # whichever route the dispatcher takes


def test_forward_leading_dimensions_and_a_non_contiguous_view():
    x, w, b, s = _inputs(10, 70, 33, False, True, True, False, 77)
    pw = hipops.pack_weight(w)
    want = hipops.bconv2d_direct(x[:, :, None, None], pw, b, s)[:, :, 0, 0]
    x3 = x.reshape(2, 5, 70)
    for route in ("blinear", "conv", None):
        y = hipops.linear(x3, pw, b, s, route=route)
        assert y.shape == (2, 5, 33) and same_bits(y.reshape(10, 33), want)
    wide = torch.zeros((10, 140), device=DEV)
    wide[:, ::2] = x
    view = wide[:, ::2]
    assert not view.is_contiguous()
    assert same_bits(hipops.blinear_direct(view, pw, b, s), want)
    y, sv = hipops.blinear_direct(x3, pw, b, s, want_planes=True)
    assert y.shape == (2, 5, 33) and sv.shape == (10, 70, 1, 1)
    assert same_bits(torch.ops.bnn_amd.binary_linear(x3, w, b, s, False, True).reshape(10, 33), want)


# ---- gradients on the exact table: one right answer per bit ------------------------------------------------------------
@pytest.mark.parametrize("case", L.EXACT_CASES, ids=lambda c: c.name)
def test_gradients_equal_the_references_bit_for_bit(case):
    x, w, alpha, g = L.exact_inputs(case)
    splits = L.case_splits(case)
    for s in splits:
        L.assert_exact(g, alpha, x.shape, L.split_ranges(case.M, s))
    pw = hipops.pack_weight(dev(w))
    assert pw.has_zero
    a = torch.zeros_like(pw.alpha)
    a[: case.O] = dev(alpha)
    pw = dataclasses.replace(pw, alpha=a)
    _, sv = hipops.blinear_direct(dev(x), pw, want_planes=True)
    gd = dev(g)
    gx = hipops.blinear_grad_input(gd, sv, pw)
    want = dev(L.dgrad_ref(g, x, L.weight_sign_ref(w), alpha).astype(F32))
    assert same_bits(gx, want)
    masked = np.abs(x) >= 1
    masked |= np.isnan(x)
    assert (gx.cpu().numpy().view(np.int32)[masked] == 0).all()                        # +0 where |x| >= 1 (and exactly 1)
    for s in splits:
        part = hipops.blinear_grad_weight(gd, sv, reduce=False, splits=s)
        want = dev(L.wgrad_ref(g, x, L.split_ranges(case.M, s)).astype(F32))
        assert part.shape == (s, case.O, case.F) and same_bits(part, want), s
    if case.splits is None:
        part = hipops.blinear_grad_weight(gd, sv, reduce=False)
        assert part.shape[0] == splits[0] == hipops.blinear_grad_weight_splits(case.M, case.O, case.F)
        assert same_bits(part, want)
    with pytest.raises(native.NativeError):
        hipops.blinear_grad_weight(gd, sv, reduce=False, splits=case.M + 1)


# ---- gradients on random inputs, against the composition ---------------------------------------------------------------
def _layer(F, O, bias, scale, center, seed):
    lin = nn.Linear(F, O, bias=bias)
    lin.weight.data.copy_(torch.from_numpy(gen.normal(seed, (O, F)).astype(F32) * 0.1))
    if bias:
        lin.bias.data.copy_(torch.from_numpy(0.1 * gen.normal(seed + 1, (O,)).astype(F32)))
    cfg = bnn.BConfig(activation_pre_process=BasicInputBinarizer,
                      activation_post_process=BasicScaleBinarizer if scale else bnn.Identity,
                      weight_pre_process=XNORWeightBinarizer.with_args(center_weights=center))
    layer = bnn.prepare_binary_model(lin, cfg)
    if scale:
        layer.activation_post_process.alpha.data.copy_(
            torch.from_numpy((0.5 + gen.uniform(seed + 2, (O,))).astype(F32)).view(1, -1))
    return layer.to(DEV).train()


@pytest.fixture
def linear_flag():
    was = training.LINEAR
    training.LINEAR = True
    yield
    training.LINEAR = was


def _grads(layer, x_np, g_np, enabled):
    training.ENABLED = enabled
    try:
        for p in layer.parameters():
            p.grad = None
        x = dev(x_np).requires_grad_(True)
        y = layer(x)
        y.backward(dev(g_np))
        return y.detach(), x.grad.clone(), {n: p.grad.clone() for n, p in layer.named_parameters()}
    finally:
        training.ENABLED = True


def _tol(ref):
    return dict(rtol=1e-4, atol=1e-5 * float(ref.abs().max()))


@pytest.mark.parametrize("lead,F,O,bias,scale,center", [
    ((33,), 70, 40, True, True, True), ((2, 17), 100, 10, False, False, False), ((130,), 300, 70, True, True, False)])
def test_training_forward_and_gradients_match_the_composition(linear_flag, lead, F, O, bias, scale, center):
    layer = _layer(F, O, bias, scale, center, seed=F + O)
    x = (gen.normal(5, lead + (F,)) * 0.8).astype(F32)                # |x| straddles the STE threshold 1
    g = gen.normal(6, lead + (O,)).astype(F32)
    before = fastpath.stats()["linear_train"]
    y1, gx1, gp1 = _grads(layer, x, g, enabled=True)
    assert fastpath.stats()["linear_train"] == before + 1              # the HIP path ran
    y0, gx0, gp0 = _grads(layer, x, g, enabled=False)
    assert fastpath.stats()["linear_train"] == before + 1              # ... and not in the control run
    for name, a, r in (("y", y1, y0), ("gx", gx1, gx0)):
        print(name, float((a - r).abs().max()), float(r.abs().max()))
        assert torch.allclose(a, r, **_tol(r)), name
    assert ((gx1 == 0) == (gx0 == 0)).all()
    assert gp1.keys() == gp0.keys() and ("bias" in gp0) == bias and any("alpha" in n for n in gp0) == scale
    for n in gp0:
        print(n, float((gp1[n] - gp0[n]).abs().max()), float(gp0[n].abs().max()))
        assert torch.allclose(gp1[n], gp0[n], **_tol(gp0[n])), n


@pytest.mark.parametrize("fused", [True, False], ids=["fused_hook", "torch_hook"])
def test_training_gradients_with_and_without_the_fused_weight_hook(linear_flag, monkeypatch, fused):
    """``training.FUSED_WEIGHT_HOOK`` off: ``What = weight_pre_process(W)`` is made by torch under autograd and the weight
    gradient kernel's slabs are summed into dL/dWhat instead of feeding ``xnor_weight_backward``.  65 rows: one full
    64-row workgroup and a tail."""
    hook_kernel = []
    real = hipops.xnor_weight_backward
    monkeypatch.setattr(hipops, "xnor_weight_backward", lambda *a: hook_kernel.append(1) or real(*a))
    monkeypatch.setattr(training, "FUSED_WEIGHT_HOOK", fused)
    test_training_forward_and_gradients_match_the_composition(None, (65,), 70, 33, True, False, False)
    assert len(hook_kernel) == (1 if fused else 0)


# ---- dispatch -----------------------------------------------------------------------------------------------------------
def test_flag_moves_a_linear_onto_the_hip_path_and_keeps_three_bits_per_element():
    layer = _layer(70, 33, True, False, False, seed=3)
    x_np = (gen.normal(8, (37, 70)) * 0.8).astype(F32)
    g_np = gen.normal(9, (37, 33)).astype(F32)
    was = training.LINEAR
    try:
        training.LINEAR = False
        n0 = fastpath.stats()["linear_train"]
        training.saved_input_bytes(reset=True)
        y_off, gx_off, gp_off = _grads(layer, x_np, g_np, enabled=True)
        assert fastpath.stats()["linear_train"] == n0 and training.saved_input_bytes() == 0   # the composition ran
        y_ctl, gx_ctl, _ = _grads(layer, x_np, g_np, enabled=False)
        assert torch.equal(y_off, y_ctl) and torch.equal(gx_off, gx_ctl)
        training.LINEAR = True
        for k in (1, 2):
            training.saved_input_bytes(reset=True)
            y_on, gx_on, gp_on = _grads(layer, x_np, g_np, enabled=True)
            assert fastpath.stats()["linear_train"] == n0 + k
            assert training.saved_input_bytes() == 3 * 8 * 37 * ((70 + 63) // 64)
        with torch.no_grad():                                          # inference: the same bits as the training forward
            n_inf = fastpath.stats()["linear"]
            assert torch.equal(layer(dev(x_np)), y_on) and fastpath.stats()["linear"] == n_inf + 1
        assert fastpath.stats()["linear_train"] == n0 + 2
    finally:
        training.LINEAR = was
    # the operator's autograd formula: the same kernels, whatever the flag says
    x = dev(x_np).requires_grad_(True)
    w = layer.weight.detach().clone().requires_grad_(True)
    b = layer.bias.detach().clone().requires_grad_(True)
    y = torch.ops.bnn_amd.binary_linear(x, w, b, None, False, True)
    y.backward(dev(g_np))
    assert torch.equal(y.detach(), y_on)
    for name, a, r in (("gx", x.grad, gx_on), ("gw", w.grad, gp_on["weight"]), ("gb", b.grad, gp_on["bias"])):
        assert torch.allclose(a, r, **_tol(r)), name
    assert ((x.grad == 0) == (gx_on == 0)).all()


def test_operator_gradient_of_the_post_scale():
    layer = _layer(64, 10, True, True, True, seed=12)
    x_np, g_np = (gen.normal(1, (5, 64)) * 0.8).astype(F32), gen.normal(2, (5, 10)).astype(F32)
    y0, gx0, gp0 = _grads(layer, x_np, g_np, enabled=False)
    x = dev(x_np).requires_grad_(True)
    leaves = {n: p.detach().clone().requires_grad_(True) for n, p in layer.named_parameters()}
    sname = next(n for n in leaves if "alpha" in n)
    y = torch.ops.bnn_amd.binary_linear(x, leaves["weight"], leaves["bias"], leaves[sname], True, True)
    y.backward(dev(g_np))
    assert torch.allclose(y.detach(), y0, **_tol(y0)) and torch.allclose(x.grad, gx0, **_tol(gx0))
    for n in gp0:
        assert torch.allclose(leaves[n].grad, gp0[n], **_tol(gp0[n])), n


# ---- end to end ---------------------------------------------------------------------------------------------------------
def test_three_sgd_steps_of_a_binary_mlp_agree_with_the_composition(linear_flag):
    def run(flag):
        training.LINEAR = flag
        torch.manual_seed(0)
        net = nn.Sequential(nn.Linear(70, 130), nn.Linear(130, 130), nn.Linear(130, 10))
        for i, m in enumerate(net):
            m.weight.data.copy_(torch.from_numpy(gen.normal(40 + i, tuple(m.weight.shape)).astype(F32) * 0.1))
            m.bias.data.copy_(torch.from_numpy(gen.normal(50 + i, tuple(m.bias.shape)).astype(F32) * 0.1))
        cfg = bnn.BConfig(activation_pre_process=BasicInputBinarizer, activation_post_process=bnn.Identity,
                          weight_pre_process=XNORWeightBinarizer)
        net = bnn.prepare_binary_model(net, cfg).to(DEV).train()
        opt = torch.optim.SGD(net.parameters(), lr=0.05)
        x, t = dev((gen.normal(60, (33, 70)) * 0.8).astype(F32)), dev(gen.normal(61, (33, 10)).astype(F32))
        n0, losses = fastpath.stats()["linear_train"], []
        for _ in range(3):
            opt.zero_grad()
            loss = (net(x) - t).square().mean()
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        assert fastpath.stats()["linear_train"] - n0 == (9 if flag else 0)
        return losses, [p.detach().clone() for p in net.parameters()]

    l1, p1 = run(True)
    l0, p0 = run(False)
    print("losses", l1, l0)
    assert np.allclose(l1, l0, rtol=1e-4, atol=1e-5 * max(l0))
    for a, r in zip(p1, p0):
        assert torch.allclose(a, r, **_tol(r))

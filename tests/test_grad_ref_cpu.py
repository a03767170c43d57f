"""tests/grad_ref.py pinned on the CPU: against torch autograd in float64 in the reference's own formulation
(conv2d(sign(x), sign(Wc) alpha) with the hard-tanh STE; XNORWeightBinarizer under autograd) on random data, and against a
small hand-written table.  tests/test_gpu_grad_exact.py compares the HIP kernels with these references bit for bit."""
import numpy as np
import pytest
import torch

from bnn_amd.ops import SignActivation, XNORWeightBinarizer
from tests import grad_ref as R
from tests.golden import gen

F32, F64 = np.float32, np.float64


def ints(seed, shape, lo, hi):
    return np.floor(gen.uniform(seed, shape) * (hi - lo + 1)).astype(np.int64) + lo


def autograd_conv(g, x, w_hat, ks, stride):
    """(dL/dx, dL/dWhat) of conv2d(SignActivation(x), What) in float64."""
    xt = torch.from_numpy(np.asarray(x, F64)).requires_grad_(True)
    wt = torch.from_numpy(np.asarray(w_hat, F64)).requires_grad_(True)
    y = torch.nn.functional.conv2d(SignActivation.apply(xt), wt, None, stride, ks // 2)
    y.backward(torch.from_numpy(np.asarray(g, F64)))
    return xt.grad.numpy(), wt.grad.numpy()


@pytest.mark.parametrize("shape,ks,stride", [
    ((3, 5, 7, 6, 9), 3, 1), ((2, 4, 3, 7, 8), 3, 2), ((2, 4, 3, 8, 7), 3, 2), ((2, 6, 5, 1, 1), 3, 2),
    ((2, 6, 5, 1, 2), 3, 2), ((2, 3, 5, 2, 1), 3, 2), ((3, 7, 5, 4, 5), 1, 1), ((1, 2, 2, 1, 1), 3, 1),
], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_conv_gradient_references_equal_autograd_in_float64(shape, ks, stride):
    N, O, C, H, W = shape
    Hg, Wg = (H - 1) // stride + 1, (W - 1) // stride + 1
    seed = gen.seed_of("grad-ref", shape, ks, stride)
    w_sign = ints(seed, (O, C, ks, ks), -1, 1).astype(F64)
    # exact data: integers, power-of-two alpha, x on both sides of the STE boundary and of zero (no NaN: torch.sign(NaN)
    # is NaN, the kernels' sign(NaN) is 0 — the table below states that case)
    vals = np.array([0.0, -0.0, 0.5, -0.5, 1.0, -1.0, np.nextafter(F32(1), F32(0)), 2.0, -2.0, np.inf, -np.inf, 1e-45], F32)
    x = vals[ints(seed + 1, (N, C, H, W), 0, len(vals) - 1)]
    g = ints(seed + 2, (N, O, Hg, Wg), -7, 7).astype(F64)
    alpha = 2.0 ** -(np.arange(O) % 5)
    gx, gw = autograd_conv(g, x, w_sign * alpha[:, None, None, None], ks, stride)
    assert np.array_equal(R.dgrad_ref(g, x, w_sign, alpha, ks, stride), gx)
    whole = R.wgrad_ref(g, x, ks, stride, [(0, N)])
    assert np.array_equal(whole[0], gw)
    for splits in R.valid_splits(N):
        slabs = R.wgrad_ref(g, x, ks, stride, R.split_ranges(N, splits))
        assert slabs.shape == (splits, O, C, ks, ks) and np.array_equal(slabs.sum(0), gw)
    # random real data: float64 rounding only
    g = gen.normal(seed + 3, (N, O, Hg, Wg)).astype(F64)
    x = (gen.normal(seed + 4, (N, C, H, W)) * 0.9).astype(F32)
    alpha = 0.5 + gen.uniform(seed + 5, (O,))
    gx, gw = autograd_conv(g, x, w_sign * alpha[:, None, None, None], ks, stride)
    assert np.allclose(R.dgrad_ref(g, x, w_sign, alpha, ks, stride), gx, rtol=1e-12, atol=1e-12)
    assert np.allclose(R.wgrad_ref(g, x, ks, stride, [(0, N)])[0], gw, rtol=1e-12, atol=1e-12)


def test_conv_gradient_references_equal_the_hand_written_table():
    nan = np.nan
    # 1x1: g[o, x], sign(W)[o, c], x[c, x]
    g = np.array([[1, 2], [3, -1]], F64).reshape(1, 2, 1, 2)
    w = np.array([[1, -1], [0, 1]], F64).reshape(2, 2, 1, 1)
    x = np.array([[0.5, 1.0], [nan, -0.0]], F32).reshape(1, 2, 1, 2)
    alpha = np.array([2.0, 0.5])
    gx = R.dgrad_ref(g, x, w, alpha, 1, 1)
    assert np.array_equal(gx.reshape(2, 2), [[2.0, 0.0], [0.0, -4.5]])
    assert not np.signbit(gx).reshape(2, 2)[0, 1] and not np.signbit(gx).reshape(2, 2)[1, 0]      # masked: +0
    assert np.array_equal(R.wgrad_ref(g, x, 1, 1, [(0, 1)]).reshape(2, 2), [[3, 0], [2, 0]])
    # 3x3 / stride 2 on a 3 x 5 image: the g grid is 2 x 3
    g = np.array([[1, 2, 3], [4, 5, 6]], F64).reshape(1, 1, 2, 3)
    w = np.array([[1, 0, -1], [1, 1, 0], [-1, 1, 1]], F64).reshape(1, 1, 3, 3)
    x = np.full((3, 5), 0.5, F32)
    x[0, 0], x[1, 2], x[2, 4] = -2.0, 1.0, 0.0
    x = x.reshape(1, 1, 3, 5)
    gx = R.dgrad_ref(g, x, w, np.array([1.0]), 3, 2)
    assert np.array_equal(gx.reshape(3, 5), [[0, 2, 2, 3, 3], [1, 0, 0, 0, 3], [4, 5, 5, 6, 6]])
    assert not np.signbit(gx).any()
    assert np.array_equal(R.wgrad_ref(g, x, 3, 2, [(0, 1)]).reshape(3, 3), [[11, 15, 9], [16, 13, 12], [5, 6, 3]])
    # sign(NaN) = sign(+-0) = 0 in the weight gradient, and the slabs of an image split
    g2 = np.array([1.0, 2.0, 4.0]).reshape(3, 1, 1, 1)
    x2 = np.array([nan, -3.0, -0.0], F32).reshape(3, 1, 1, 1)
    assert np.array_equal(R.wgrad_ref(g2, x2, 1, 1, [(0, 2), (2, 3)]).reshape(2), [-2.0, 0.0])
    assert R.split_ranges(5, 3) == [(0, 2), (2, 4), (4, 5)] and R.valid_splits(5) == [1, 2, 3, 5]
    assert R.valid_splits(7) == [1, 2, 3, 4, 7]


def test_sign_fragments_follow_the_documented_layout():
    """Bp[ob][tap][cs][lane][e] = sign(W[32 ob + 8 (lane >> 4) + e][16 cs + (lane & 15)][tap]) as bf16, zeros past O, C."""
    O, C, ks = 33, 17, 3
    w = ints(5, (O, C, ks, ks), -1, 1).astype(F64)
    frag = R.grad_fragments_ref(w, O, C, ks).view("<u2").reshape(2, 9, 2, 64, 8)
    assert frag.nbytes == 2 * 9 * 2 * 64 * 16
    code = {1.0: 0x3F80, -1.0: 0xBF80, 0.0: 0}
    for ob, tap, cs, lane, e in [(0, 0, 0, 0, 0), (0, 4, 0, 17, 3), (0, 8, 1, 0, 7), (1, 2, 0, 5, 0), (0, 5, 0, 63, 7),
                                 (1, 2, 0, 5, 1), (0, 3, 1, 1, 2), (1, 8, 1, 63, 7)]:
        o, c = 32 * ob + 8 * (lane >> 4) + e, 16 * cs + (lane & 15)
        want = code[w[o, c, tap // 3, tap % 3]] if o < O and c < C else 0
        assert frag[ob, tap, cs, lane, e] == want, (ob, tap, cs, lane, e)
    assert (frag[1, :, :, 16:, :] == 0).all() and (frag[1, :, :, :16, 1:] == 0).all()     # o >= 33
    assert (frag[:, :, 1, :, :].reshape(2, 9, 4, 16, 8)[:, :, :, 1:, :] == 0).all()       # c >= 17
    one = R.grad_fragments_ref(np.array([[[[-1.0]]]]), 1, 1, 1).view("<u2")
    assert one.size == 512 and one[0] == 0xBF80 and not one[1:].any()


def test_exactness_proofs_accept_exact_inputs_and_refuse_the_rest():
    g = ints(3, (2, 4, 3, 3), -7, 7).astype(F64)
    alpha = np.array([1.0, 0.5, 0.0, 0.0625])
    d, w = R.assert_exact_inputs(g, alpha, (2, 5, 3, 3), 3, 1, [(0, 2)])
    assert 0 < d <= 7 * 16 * 4 * 9 and 0 < w <= 7 * 2 * 9
    R.assert_exact_inputs(g * 2.0 ** -40, alpha, (2, 5, 3, 3), 3, 1, [(0, 1), (1, 2)])
    with pytest.raises(AssertionError):                       # a term of 2^24 units
        R.assert_exact_inputs(g + 2.0 ** -22, alpha, (2, 5, 3, 3), 3, 1)
    with pytest.raises(AssertionError):                       # sum |terms| reaches 2^24 units
        R.assert_exact_inputs(np.where(g == 0, 1, g) * (1 + 2.0 ** -18), alpha, (2, 5, 3, 3), 3, 1, [(0, 2)])
    with pytest.raises(AssertionError):                       # not an fp32 number
        R.assert_exact_inputs(g + 2.0 ** -30, alpha, (2, 5, 3, 3), 3, 1)
    # sums in integers: the value, the figure, the refusal
    r = []
    s = R.exact_sum(np.array([[0.75, -0.25, 2.0 ** -20], [0.0, 0.0, 0.0]]), 1, 53, "t", r)
    assert np.array_equal(s, [0.5 + 2.0 ** -20, 0.0]) and r == [("t", 2 ** 20 + 1)]
    with pytest.raises(AssertionError):
        R.exact_sum(np.array([1.0, 2.0 ** -60]), 0, 53, "t")
    wd = (ints(7, (3, 5, 3, 3), -191, 191) / 64.0).astype(F32)
    dw = ints(8, (3, 5, 3, 3), -2, 2).astype(F32)
    worst = R.assert_exact_weight_inputs(wd, np.sign(dw) * 2.0 ** np.abs(dw), True, True)
    assert set(worst) == {"centre", "alpha", "sum dWhat sign(Wc)", "centre of dWc"} and max(worst.values()) < 2 ** 53
    with pytest.raises(AssertionError, match="alpha"):       # dWhat * alpha rounds in float32
        R.assert_exact_weight_inputs(wd, np.full_like(wd, 3.0) + 2.0 ** -20, False, True)
    bad = wd.copy()
    bad[0, 0, 0, 0], bad[0, 1, 0, 0] = 2.0, 2.0 ** -60
    with pytest.raises(AssertionError, match="2\\^53"):
        R.assert_exact_weight_inputs(bad, dw, True, False)


@pytest.mark.parametrize("center", [False, True], ids=["plain", "centred"])
@pytest.mark.parametrize("compute_alpha", [False, True], ids=["sign", "alpha"])
@pytest.mark.parametrize("shape", [(4, 6, 3, 3), (3, 1, 3, 3), (5, 17, 1, 1), (2, 9, 5, 5)], ids=lambda s: "x".join(map(str, s)))
def test_weight_hook_references_equal_autograd_of_the_binarizer(shape, center, compute_alpha):
    seed = gen.seed_of("xnor-ref", shape)
    w = (gen.normal(seed, shape) * 0.8).astype(F32)
    dwhat = gen.normal(seed + 1, (3,) + shape).astype(F32)
    wt = torch.from_numpy(w.astype(F64)).requires_grad_(True)
    what = XNORWeightBinarizer(compute_alpha=compute_alpha, center_weights=center)(wt)
    what.backward(torch.from_numpy(dwhat.astype(F64).sum(0)))
    got, alpha = R.xnor_what_ref(w, center, compute_alpha)
    assert got.dtype == F32 and got.shape == shape and alpha.dtype == F32
    tol = 2.0 ** -22                                        # a few float32 roundings of values of order 1
    assert np.allclose(got, what.detach().numpy(), rtol=tol, atol=tol)
    assert np.array_equal(got, np.sign(got) * alpha[:, None, None, None])
    dw = R.xnor_weight_backward_ref(w, dwhat, center, compute_alpha)
    ref = wt.grad.numpy()
    assert dw.dtype == F32 and np.allclose(dw, ref, rtol=0, atol=4 * tol * max(1.0, float(np.abs(ref).max())))
    one = R.xnor_weight_backward_ref(w, dwhat[0], center, compute_alpha)
    assert np.array_equal(one, R.xnor_weight_backward_ref(w, dwhat[:1], center, compute_alpha))
    # (one input channel, centred: every Wc is 0, and the input-gradient kernel's alpha with it)
    live = (R.centred_sign_ref(w, center) != 0).reshape(shape[0], -1).any(1)
    assert np.array_equal(R.alpha_ref(w, center, compute_alpha), np.where(live, alpha, 0))
    assert live.all() != (center and shape[1] == 1)


def test_weight_hook_references_equal_the_hand_written_table():
    # a centred weight with elements at |Wc| == 1: mean 0.5, Wc = [1, -1, 0.25, -0.25], alpha = 2.5 / 4
    w = np.array([1.5, -0.5, 0.75, 0.25], F32).reshape(1, 4, 1, 1)
    what, alpha = R.xnor_what_ref(w, True, True)
    assert np.array_equal(alpha, [0.625]) and np.array_equal(what.reshape(4), [0.625, -0.625, 0.625, -0.625])
    # sum dWhat sign = 2 - 4 + 8 + 4 = 10, / 4 = 2.5; STE: [0, 0, 8 * 0.625, -4 * 0.625]; mean of dWc = 2.5 / 4
    dwhat = np.array([2, 4, 8, -4], F32).reshape(1, 4, 1, 1)
    dw = R.xnor_weight_backward_ref(w, dwhat, True, True)
    assert np.array_equal(dw.reshape(4), [1.875, -3.125, 6.875, -5.625])
    assert np.array_equal(R.xnor_weight_backward_ref(w, dwhat, True, False).reshape(4), [-1.0, -1.0, 7.0, -5.0])
    # not centred: |w| >= 1 is masked, sign(+-0) = 0; slabs are added first
    w = np.array([1.5, -0.5, 0.0, -0.0, -1.0, np.nextafter(F32(1), F32(0))], F32).reshape(1, 6, 1, 1)
    what, alpha = R.xnor_what_ref(w, False, False)
    assert np.array_equal(what.reshape(6), [1, -1, 0, 0, -1, 1]) and not np.signbit(what).reshape(6)[2:4].any()
    slabs = np.array([[1, 2, 3, 4, 5, 6], [1, 1, 1, 1, 1, 1]], F32).reshape(2, 1, 6, 1, 1)
    assert np.array_equal(R.xnor_weight_backward_ref(w, slabs, False, False).reshape(6), [0, 3, 4, 5, 0, 7])
    # a NaN weight: its sign is 0, alpha is NaN, the all-zero channel has alpha 0 for the input-gradient kernel
    w = np.array([[0.5, np.nan, -0.25], [0.0, -0.0, 0.0]], F32).reshape(2, 3, 1, 1)
    what, alpha = R.xnor_what_ref(w, False, True)
    assert np.isnan(alpha[0]) and alpha[1] == 0 and np.isnan(what[0]).all() and not what[1].any()
    a = R.alpha_ref(w, False, True)
    assert np.isnan(a[0]) and a[1] == 0
    assert np.array_equal(R.centred_sign_ref(w, False).reshape(2, 3), [[1, 0, -1], [0, 0, 0]])
    assert np.array_equal(R.centred_weight_ref(np.array([1.5, -0.5], F32).reshape(1, 2, 1, 1), True).reshape(2), [1.0, -1.0])
    assert np.array_equal(R.alpha_ref(np.zeros((1, 2, 1, 1), F32), False, False), [0.0])

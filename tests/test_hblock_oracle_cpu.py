"""tests/hblock_oracle.py, the CPU restatement the one-launch hierarchical-block tests compare against, checked here
before any GPU result depends on it: against the reference's op sequence (bnn/models/layers/hierarchical_block.py:38-60,
the one of test_gpu_hblock.py::test_against_the_float_formulation) evaluated in float64 torch, on every data kind."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle
from tests import hblock_oracle as hbo


@pytest.mark.parametrize("shape", [(1, 3, 4, 4), (2, 5, 7, 9), (3, 2, 13, 9), (1, 1, 1, 1), (2, 4, 1, 5), (1, 3, 6, 1)],
                         ids=lambda s: "x".join(map(str, s)))
def test_avgpool_ceil_is_atens_avg_pool2d_bit_for_bit(shape):
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(*shape, generator=g) * 3
    x[..., 0, 0] = 0.0
    want = F.avg_pool2d(x, 2, 2, ceil_mode=True, count_include_pad=False)
    got = oracle.avgpool_ceil(x.numpy(), 2)
    assert got.shape == tuple(want.shape) and np.array_equal(got, want.numpy())


def _binconv(t, w, padding):
    """bnn/layers/conv.py: sign(input) conv sign(W) * mean|W| (XNOR binarizer), float64."""
    w = torch.from_numpy(w).double()
    alpha = w.abs().mean(dim=(1, 2, 3), keepdim=True)
    return F.conv2d(torch.sign(t), torch.sign(w) * alpha, padding=padding)


def _affine(t, bn):
    """bn(t) in float64.  The float convolution sums +-alpha terms with rounding, so an exact zero (alpha * dot * a + b
    == 0: a zero dot with a zero shift, or a tie) can come out as a residue near 1e-17: those are set back to zero (a
    non-zero value is at least alpha * |a| / 2^24 away from it)."""
    v = t * torch.from_numpy(bn[0]).double()[None, :, None, None] + torch.from_numpy(bn[1]).double()[None, :, None, None]
    return torch.where(v.abs() < 1e-12, torch.zeros_like(v), v)


def _float_block(d, form):
    """Float64 torch evaluation of the block: (y, pre-sign values in front of conv2 / conv3 (before the ReLU))."""
    if form == "shortcut":
        res = _binconv(torch.from_numpy(d["s_sc"]).double(), d["w_sc"], 0)
    else:
        res = torch.from_numpy(d["res"]).double()
    o1 = _binconv(torch.from_numpy(d["s_in"]).double(), d["ws"][0], 1)
    v2 = _affine(o1, d["bn2"])
    o2 = _binconv(torch.relu(v2), d["ws"][1], 1)
    v3 = _affine(o2, d["bn3"])
    o3 = _binconv(torch.relu(v3), d["ws"][2], 1)
    return torch.cat((o1, o2, o3), 1) + res, (v2, v3)


def _assert_signs(P, M, v, relu):
    """The planes equal sign(act(v)) wherever v is not within 1e-6 of zero (and where it is exactly zero)."""
    v = v.numpy()
    want = np.sign(np.maximum(v, 0.0) if relu else v)
    got = hbo.signs_of(P, M, v.shape[1])
    mask = (np.abs(v) > 1e-6) | (v == 0.0)
    assert mask.sum() > 0.5 * mask.size
    assert np.array_equal(got[mask], want[mask])
    return int((v == 0.0).sum())


BLOCKS = [(64, 64, 2, 5, 7), (128, 128, 1, 4, 6), (64, 128, 2, 6, 4)]   # c_in, planes, N, H, W


@pytest.mark.parametrize("kind", hbo.KINDS)
@pytest.mark.parametrize("form", ["plain", "pool", "shortcut"])
def test_restatement_matches_the_float_formulation(form, kind):
    c_in, planes, N, H, W = BLOCKS[("plain", "pool", "shortcut").index(form)]
    d = hbo.draw(17, c_in, planes, N, H, W, kind, form)
    got = hbo.run(d, form)
    y64, (v2, v3) = _float_block(d, form)
    # no pre-sign value inside the block lies next to zero without being exactly zero: every later value is comparable
    for v in (v2, v3):
        assert not bool(((v.abs() <= 1e-6) & (v != 0)).any())
    y = got["y"]
    assert y.dtype == np.float32
    assert np.allclose(y, y64.numpy(), rtol=1e-5, atol=1e-5 * float(y64.abs().max()))
    zeros = 0
    if form == "pool":
        t64 = F.avg_pool2d(y64, 2, 2, ceil_mode=True, count_include_pad=False)
        zeros += _assert_signs(got["P1"], got["M1"], _affine(t64, d["bn1"]), True)
        zeros += _assert_signs(got["P2"], got["M2"], _affine(t64, d["bn_ds"]), False)
        assert not got["M1"].any()
    else:
        zeros += _assert_signs(got["P"], got["M"], _affine(y64, d["nbn"]), True)
        assert not got["M"].any()
    if kind == "ties":   # the ties are there, exactly, and both routes give them sign 0
        assert zeros > 0 and bool((v2 == 0).any()) and bool((v3 == 0).any())
    if kind == "cancel" and form != "shortcut":
        assert (y == 0).mean() > 0.1
    if kind in ("all_set", "none_set"):
        full = np.uint64(0xFFFFFFFFFFFFFFFF)
        P, M = (got["P1"], got["M1"]) if form == "pool" else (got["P"], got["M"])
        assert np.all(P == (full if kind == "all_set" else 0)) and not M.any()
        if form == "pool":
            assert np.all(got["P2" if kind == "all_set" else "M2"] == full)


def test_the_float64_sign_is_the_sign_of_the_epilogues_fmaf():
    """The restatement binarises in float64; the oracle's fused epilogue (and the kernels) take sign(fmaf(v, a, b)) in
    float32 — the same decision, ties included."""
    for kind in ("neg_scales", "ties"):
        d = hbo.draw(5, 64, 64, 2, 6, 6, kind)
        P_in = d["P_in"]
        wb, wz, alpha, _ = oracle.pack_weight(d["ws"][0])
        dot = oracle.bconv_dot(P_in, np.zeros_like(P_in), wb, wz, (2, 64, 6, 6), d["ws"][0].shape, padding=1)
        _, pv = oracle.fused_epilogue2(dot, alpha[:32], res=d["res"], res_late=True, pack_pre=True, pack_a=d["bn2"][0],
                                       pack_b=d["bn2"][1], pack_relu=True, out=np.zeros_like(d["res"]), c_off=0)
        pre = hbo.plain(P_in, d["ws"], d["bn2"], d["bn3"], d["res"])["pre"][0]
        s = hbo.sign_affine(pre, *d["bn2"], relu=True)
        assert np.array_equal(np.sign(pv).astype(np.int8), s)
        if kind == "ties":
            assert bool((s == 0).any()) and bool((s == 1).any())

"""A BATS cell operation in a training step as fused HIP launches (training.CELL_OPS: training.CellOpTrainFn).

The new kernels one by one — BatchNorm + sign + STE mask as three bit planes (csrc/pack_ste.hip) bit for bit against
the existing entry points and the CPU oracle, the PReLU + shuffle backward (csrc/prelu_bwd.hip) against float64
autograd, the BatchNorm backward with an addend against the existing backward — then the assumption the backward rests
on (the un-fused convolution launch returns the pre-activation value the fused epilogue started from), the whole
operation against its float64 composition, the switch, and a cell taking a training step.

Tolerances are those of tests/test_gpu_grouped_train.py: outputs and input gradients rtol 1e-4, atol 1e-5 max|ref|;
parameter gradients rtol 1e-3, atol 1e-4 max|ref| + 1e-7."""
import copy
import dataclasses
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bnn_amd as bnn
import oracle
from bnn_amd import fastpath, hipops, models, training
from bnn_amd.models.bats_ops import channel_shuffle
from bnn_amd.ops import BasicInputBinarizer, XNORWeightBinarizer
from tests.golden import cells_cases, gen
from tests.golden.cellops_cases import CELL_CASES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OP_NAMES = ("SepConv", "DilConv", "ReLUConvBN")


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def close(a, ref, rtol=1e-4, afac=1e-5, aabs=0.0):
    a, ref = a.detach().cpu(), ref.detach().cpu().to(torch.float64)
    atol = afac * float(ref.abs().max()) + aabs
    err = float((a.to(torch.float64) - ref).abs().max())
    print("max |a - ref| =", err, "atol =", atol, "max|ref| =", float(ref.abs().max()))
    return bool(torch.allclose(a.to(torch.float64), ref, rtol=rtol, atol=atol))


def close_param(a, ref):
    return close(a, ref, rtol=1e-3, afac=1e-4, aabs=1e-7)


def binarise(m):
    cfg = bnn.BConfig(activation_pre_process=BasicInputBinarizer, activation_post_process=bnn.Identity,
                      weight_pre_process=XNORWeightBinarizer)
    return bnn.prepare_binary_model(m, cfg)


def build(case):
    m = binarise(case.build(models))
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict({k: torch.from_numpy(v) for k, v in case.state(shapes).items()})
    return m.to(DEV).train()


@pytest.fixture
def cell_ops_on(monkeypatch):
    monkeypatch.setattr(training, "CELL_OPS", True)


def same_planes(a, b):
    return torch.equal(a.sign.P, b.sign.P) and torch.equal(a.sign.M, b.sign.M) and torch.equal(a.T, b.T)


# ---- 1. the pack kernel, bit for bit ---------------------------------------------------------------------------------
PACK_SHAPES = [(3, 48, 10, 6),      # HW = 60: the float4 form, C < 64
               (2, 96, 7, 9),       # HW = 63: the scalar form, one and a half channel words
               (2, 70, 5, 5),       # a ragged second word
               (1, 8, 3, 70),       # rows wider than a wave
               (5, 24, 6, 6)]       # small HW
EPS, MOMENTUM = 1e-5, 0.1


def bn_params(C, seed, affine):
    if not affine:
        return None, None
    return dev((0.5 + gen.uniform(seed, (C,))).astype(np.float32)), dev((0.3 * gen.normal(seed + 1, (C,))).astype(np.float32))


@pytest.mark.parametrize("affine", [True, False], ids=["affine", "noaffine"])
@pytest.mark.parametrize("shape", PACK_SHAPES, ids=["x".join(map(str, s)) for s in PACK_SHAPES])
def test_bn_train_pack_ste_has_the_bits_of_batchnorm_then_pack(shape, affine):
    N, C, H, W = shape
    seed = gen.seed_of("cellops-train-pack", "x".join(map(str, shape)))
    x = dev((1.5 * gen.normal(seed, shape) + 0.25).astype(np.float32))
    gamma, beta = bn_params(C, seed + 7, affine)
    rm0, rv0 = dev((0.5 * gen.normal(seed + 2, (C,))).astype(np.float32)), dev((0.5 + gen.uniform(seed + 3, (C,))).astype(np.float32))
    rm1, rv1, rm2, rv2 = rm0.clone(), rv0.clone(), rm0.clone(), rv0.clone()
    # (a) against BatchNorm's own forward followed by pack_act_ste
    u, mean1, invstd1 = hipops.bn_train_forward(x, gamma, beta, rm1, rv1, MOMENTUM, EPS)
    want = hipops.pack_act_ste(u)
    sv, mean2, invstd2, scale, shift = hipops.bn_train_pack_ste(x, gamma, beta, rm2, rv2, MOMENTUM, EPS)
    assert tuple(sv.shape) == shape and sv.T.shape == (N, (C + 63) // 64, H, W)
    assert same_planes(sv, want)
    assert torch.equal(mean1, mean2) and torch.equal(invstd1, invstd2)
    assert torch.equal(rm1, rm2) and torch.equal(rv1, rv2) and not torch.equal(rm1, rm0) and not torch.equal(rv1, rv0)
    assert bool((u.abs() < 1).any()) and bool((u.abs() >= 1).any())
    # (b) against the CPU oracle on the scale / shift the kernel returned
    v = oracle.bn_act(x.cpu().numpy(), scale.cpu().numpy(), shift.cpu().numpy())
    Pw, Mw = oracle.pack_act(v)
    assert np.array_equal(u64(sv.sign.P), Pw) and np.array_equal(u64(sv.sign.M), Mw)
    assert np.array_equal(u64(sv.T), oracle.pack_ste_mask(v))
    assert np.array_equal(u.cpu().numpy().view(np.uint32), v.view(np.uint32))      # the fp32 value itself, word for word


# (name, x, a, b): u = fmaf(x, a, b) exactly representable; the edges of sign() and of the mask |u| < 1
ONE_DN, ONE_UP = 1.0 - 2.0 ** -24, 1.0 + 2.0 ** -23
EDGE_CASES = [("plus-zero", 3.0, 0.5, -1.5), ("minus-zero", -1.5, 0.0, -0.0), ("plus-one", 2.0, 0.5, 0.0),
              ("minus-one", 2.0, -0.5, 0.0), ("nan", float("nan"), 1.0, 0.0), ("below-one", ONE_DN, 1.0, 0.0),
              ("above-one", ONE_UP, 1.0, 0.0), ("above-minus-one", -ONE_DN, 1.0, 0.0), ("below-minus-one", ONE_UP, -1.0, 0.0),
              ("one-by-fma", 1.0, 0.5, 0.5), ("residue-below-one", 1.0, ONE_DN, 0.0)]
# expected (P, M, T) bits of those
EDGE_BITS = [(0, 0, 1), (0, 0, 1), (1, 0, 0), (0, 1, 0), (0, 0, 0), (1, 0, 1), (1, 0, 0), (0, 1, 1), (0, 1, 0), (1, 0, 0),
             (1, 0, 1)]


def plant_affine(x, a, b, positions, rot=0):
    """Edge case ``j`` goes to channel ``(rot + j) % C``: its (a, b) into the channel's affine and its x to ``positions``
    [(y, x)] of every image (the helper of tests/test_gpu_pack_family.py, for EDGE_CASES).  Returns [(channel, j)]."""
    C = x.shape[1]
    planted = []
    for j in range(min(C, len(EDGE_CASES))):
        _, xv, av, bv = EDGE_CASES[j]
        c = (rot + j) % C
        a[c], b[c] = av, bv
        for y, xx in positions:
            x[:, c, y, xx] = xv
        planted.append((c, j))
    return planted


@pytest.mark.parametrize("shape", PACK_SHAPES, ids=["x".join(map(str, s)) for s in PACK_SHAPES])
def test_bn_act_pack_ste_at_the_edges_of_sign_and_mask(shape):
    N, C, H, W = shape
    seed = gen.seed_of("cellops-train-edges", "x".join(map(str, shape)))
    x = (1.5 * gen.normal(seed, shape)).astype(np.float32)
    a = ((0.5 + gen.uniform(seed + 1, (C,))) * np.where(gen.uniform(seed + 2, (C,)) < 0.2, -1, 1)).astype(np.float32)
    b = (0.4 * gen.normal(seed + 3, (C,))).astype(np.float32)
    positions = [(0, 0), (H - 1, W - 1), (H // 2, W // 3)]
    planted = plant_affine(x, a, b, positions, rot=C - 3)       # (wraps: channels of both words where there are two)
    sv = hipops.bn_act_pack_ste(dev(x), dev(a), dev(b))
    v = oracle.bn_act(x, a, b)
    Pw, Mw = oracle.pack_act(v)
    assert np.array_equal(u64(sv.sign.P), Pw) and np.array_equal(u64(sv.sign.M), Mw)
    assert np.array_equal(u64(sv.T), oracle.pack_ste_mask(v))
    P, M, T = u64(sv.sign.P), u64(sv.sign.M), u64(sv.T)
    for c, j in planted:
        for n in range(N):
            for y, xx in positions:
                got = tuple(int((pl[n, c // 64, y, xx] >> np.uint64(c % 64)) & np.uint64(1)) for pl in (P, M, T))
                assert got == EDGE_BITS[j], (EDGE_CASES[j][0], n, c, got)
    # channels past C in the last word stay 0
    if C % 64:
        high = ~np.uint64((1 << (C % 64)) - 1)
        assert not (P[:, -1] & high).any() and not (M[:, -1] & high).any() and not (T[:, -1] & high).any()
    # without an affine: pack_act_ste itself
    assert same_planes(hipops.bn_act_pack_ste(dev(x)), hipops.pack_act_ste(dev(x)))
    assert same_planes(hipops.bn_act_pack_ste(dev(x), dev(a), dev(b)), hipops.pack_act_ste(dev(v)))


# The affine kernel at each vector width on the smallest shapes that reach it, and on bases 4 and 8 bytes off a 16-byte
# boundary (which demote the width).  (shape, pixels per thread on an aligned base)
WIDTH_SHAPES = [((2, 33, 3, 3), 1),     # H W = 9: a full half-word + a one-channel ragged one
                ((2, 33, 2, 3), 2),     # H W = 6
                ((1, 70, 2, 2), 4)]     # H W = 4: a full group, then a 6-channel half and an empty half


def carve(value, off):
    """``value`` as a contiguous device tensor whose first element lies ``off`` floats into a 16-byte aligned buffer
    (the helper of tests/test_gpu_pack_family.py)."""
    v = torch.from_numpy(np.ascontiguousarray(value))
    flat = torch.full((v.numel() + 8,), float("nan"), dtype=v.dtype, device=DEV)
    assert flat.data_ptr() % 16 == 0
    t = flat[off:off + v.numel()].view(v.shape)
    t.copy_(v)
    assert t.is_contiguous() and t.data_ptr() % 16 == 4 * off
    return t


@pytest.mark.parametrize("off", [0, 1, 2], ids=["aligned", "off4", "off8"])
@pytest.mark.parametrize("shape,vp", WIDTH_SHAPES, ids=["x".join(map(str, s)) for s, _ in WIDTH_SHAPES])
def test_bn_act_pack_ste_at_every_width_and_base(shape, vp, off):
    N, C, H, W = shape
    hw = H * W
    t_vp = 4 if hw % 4 == 0 and off == 0 else 2 if hw % 2 == 0 and off % 2 == 0 else 1
    assert (t_vp == vp) if off == 0 else (t_vp <= vp)
    seed = gen.seed_of("cellops-train-widths", "x".join(map(str, shape)))
    x = (1.5 * gen.normal(seed, shape)).astype(np.float32)
    a = ((0.5 + gen.uniform(seed + 1, (C,))) * np.where(gen.uniform(seed + 2, (C,)) < 0.2, -1, 1)).astype(np.float32)
    b = (0.4 * gen.normal(seed + 3, (C,))).astype(np.float32)
    positions = [(0, 0), (H - 1, W - 1)]
    planted = plant_affine(x, a, b, positions, rot=C - 3)       # (wraps: channels of the full and of the ragged half)
    for aff in ((a, b), (None, None)):
        sv = hipops.bn_act_pack_ste(carve(x, off), dev(aff[0]), dev(aff[1]))
        v = oracle.bn_act(x, *aff)
        Pw, Mw = oracle.pack_act(v)
        assert np.array_equal(u64(sv.sign.P), Pw) and np.array_equal(u64(sv.sign.M), Mw), (aff[0] is not None)
        assert np.array_equal(u64(sv.T), oracle.pack_ste_mask(v)), (aff[0] is not None)
        if off:
            assert same_planes(sv, hipops.bn_act_pack_ste(carve(x, 0), dev(aff[0]), dev(aff[1])))
    sv = hipops.bn_act_pack_ste(carve(x, off), dev(a), dev(b))
    P, M, T = u64(sv.sign.P), u64(sv.sign.M), u64(sv.T)
    for c, j in planted:
        for n in range(N):
            for y, xx in positions:
                got = tuple(int((pl[n, c // 64, y, xx] >> np.uint64(c % 64)) & np.uint64(1)) for pl in (P, M, T))
                assert got == EDGE_BITS[j], (EDGE_CASES[j][0], n, c, got)
    high = ~np.uint64((1 << (C % 64)) - 1)                      # channels past C in the last word stay 0
    assert not (P[:, -1] & high).any() and not (M[:, -1] & high).any() and not (T[:, -1] & high).any()


# ---- 2. PReLU + shuffle backward -------------------------------------------------------------------------------------
PRELU_SHAPES = [(3, 48, 10, 6), (2, 96, 7, 9), (5, 24, 3, 3)]


@pytest.mark.parametrize("single", [False, True], ids=["slopes", "one-slope"])
@pytest.mark.parametrize("G", [1, 4])
@pytest.mark.parametrize("shape", PRELU_SHAPES, ids=["x".join(map(str, s)) for s in PRELU_SHAPES])
def test_prelu_shuffle_backward_against_float64_autograd(shape, G, single):
    N, O, H, W = shape
    seed = gen.seed_of("cellops-train-prelu", "x".join(map(str, shape)), G, int(single))
    zn = gen.normal(seed, shape).astype(np.float32)
    flat = zn.reshape(-1)
    flat[3::31] = np.float32(0.0)
    flat[4::31] = np.float32(-0.0)
    z = dev(zn)
    zero = z == 0
    assert bool(zero.any()) and bool(torch.signbit(z[zero]).any()) and bool((~torch.signbit(z[zero])).any())
    slope = dev((0.05 + 0.4 * gen.uniform(seed + 1, (1 if single else O,))).astype(np.float32))
    g1 = dev(gen.normal(seed + 2, shape).astype(np.float32))
    for scale in (1.0, 1e-6):
        g = (g1 * scale).contiguous()
        z64 = z.double().cpu().requires_grad_()
        s64 = slope.double().cpu().requires_grad_()
        y = channel_shuffle(F.prelu(z64, s64), G)
        ref_gz, ref_gs = torch.autograd.grad(y, (z64, s64), g.double().cpu())
        gz, gs = hipops.prelu_shuffle_backward(g, z, slope, G)
        gz2, gs2 = hipops.prelu_shuffle_backward(g, z, slope, G)
        assert torch.equal(gz, gz2) and torch.equal(gs, gs2)                       # bit-reproducible
        assert gs.shape == slope.shape
        assert close(gz, ref_gz) and close_param(gs, ref_gs)
        # z == +-0 takes the slope branch ...
        gsh = g if G == 1 else g.view(N, O // G, G, H, W).transpose(1, 2).reshape(N, O, H, W)    # gy in z's channel order
        sl = slope.expand(O).view(1, O, 1, 1)
        assert torch.equal(gz[zero], (sl * gsh)[zero])
        assert torch.equal(gz[z > 0], gsh[z > 0])
        # ... and adds nothing to the slope gradient: the same call with those g zeroed gives the same bits
        gsh0 = gsh.masked_fill(zero, 0.0)
        g0 = gsh0 if G == 1 else channel_shuffle(gsh0, G).contiguous()
        assert torch.equal(hipops.prelu_shuffle_backward(g0, z, slope, G)[1], gs)
        # in place
        zc = z.clone()
        gzi, gsi = hipops.prelu_shuffle_backward(g, zc, slope, G, inplace=True)
        assert gzi.data_ptr() == zc.data_ptr() and torch.equal(gzi, gz) and torch.equal(gsi, gs)


# ---- 3. BatchNorm backward with an addend ----------------------------------------------------------------------------
@pytest.mark.parametrize("affine", [True, False], ids=["affine", "noaffine"])
@pytest.mark.parametrize("shape", PACK_SHAPES[:3], ids=["x".join(map(str, s)) for s in PACK_SHAPES[:3]])
def test_bn_backward_with_an_addend(shape, affine):
    N, C, H, W = shape
    seed = gen.seed_of("cellops-train-bnadd", "x".join(map(str, shape)))
    x = dev((1.5 * gen.normal(seed, shape) + 0.25).astype(np.float32))
    gamma, beta = bn_params(C, seed + 7, affine)
    _, mean, invstd = hipops.bn_train_forward(x, gamma, beta, None, None, MOMENTUM, EPS)
    gy = dev(gen.normal(seed + 4, shape).astype(np.float32))
    add = dev(gen.normal(seed + 5, shape).astype(np.float32))
    dx0, dg0, db0, _ = hipops.bn_train_backward(gy, None, x, mean, invstd, gamma)
    dx1, dg1, db1 = hipops.bn_train_backward_add(gy, x, mean, invstd, gamma, add)
    assert torch.equal(dg0, dg1) and torch.equal(db0, db1)
    assert close(dx1, dx0.double() + add.double())
    dx2, dg2, db2 = hipops.bn_train_backward_add(gy, x, mean, invstd, gamma, None)
    assert torch.equal(dx2, dx0) and torch.equal(dg2, dg0) and torch.equal(db2, db0)
    assert torch.equal(dx1, hipops.bn_train_backward_add(gy, x, mean, invstd, gamma, add)[0])


# ---- 4. the recomputed z is the forward's z --------------------------------------------------------------------------
def op_conf(m):
    conv = m.op[1]
    shuffle = training.CELL_OP_SHUFFLE[type(m).__name__]
    return (int(conv.groups), tuple(conv.stride), tuple(conv.padding), tuple(conv.dilation), shuffle)


def has_skip(m):
    conv = m.op[1]
    return bool(m.skip and m.stride == 1 and (conv.groups != 1 or conv.in_channels == conv.out_channels))


@pytest.mark.parametrize("case", CELL_CASES, ids=[c.name for c in CELL_CASES])
def test_the_unfused_launch_returns_the_pre_activation_value_of_the_fused_one(case):
    m = build(case)
    bn, conv, act = m.op
    x = dev(case.input())
    sv, _, _, _, _ = hipops.bn_train_pack_ste(x, bn.weight, bn.bias, bn.running_mean.clone(), bn.running_var.clone(), 0.1,
                                              bn.eps)
    plan = fastpath._recognise(conv, conv.out_channels)
    packed = fastpath.packed_weight(conv, plan, sync=False, fresh=True)
    conf = op_conf(m)
    slopes = act.weight.detach()
    skip = has_skip(m)
    assert skip == (case.stride == 1 and (case.kind != "ReLUConvBN" or case.C_in == case.C_out))
    y = training._cell_conv(sv.sign, packed, conf, prelu=slopes, residual=x if skip else None)
    z = training._cell_conv(sv.sign, packed, conf)
    assert bool((z == 0).any()) or case.kind == "ReLUConvBN"
    want = F.prelu(z, slopes)
    if conf[4] != 1:
        want = channel_shuffle(want, conf[4])
    if skip:
        want = x + want
    assert y.shape == want.shape and torch.equal(y, want.contiguous())


# ---- 5. the whole operation against its float64 composition ----------------------------------------------------------
WHOLE_CASES = CELL_CASES + [dataclasses.replace(CELL_CASES[0], name="sep3_c48_n3", N=3)]
U_MARGIN = 1e-3


def settled_input(case, m):
    """``case.input()`` with every element whose training-mode BatchNorm value u (float64, current batch statistics) lies
    within U_MARGIN of 0 or of +-1 moved to the x that gives u = 0.5, until none is left: sign() and the mask |u| < 1
    then do not depend on fp32 rounding (error in u: about 1e-6).  Returns (x fp32, rounds, elements moved)."""
    bn = m.op[0]
    C = bn.num_features
    gamma = (bn.weight.detach().double().cpu().numpy() if bn.weight is not None else np.ones(C)).reshape(1, C, 1, 1)
    beta = (bn.bias.detach().double().cpu().numpy() if bn.bias is not None else np.zeros(C)).reshape(1, C, 1, 1)
    x = case.input().astype(np.float32)
    moved = np.zeros(x.shape, bool)
    for rounds in range(1, 20):
        x64 = x.astype(np.float64)
        mean = x64.mean(axis=(0, 2, 3), keepdims=True)
        std = np.sqrt(x64.var(axis=(0, 2, 3), keepdims=True) + bn.eps)
        u = (x64 - mean) / std * gamma + beta
        bad = (np.abs(u) < U_MARGIN) | (np.abs(np.abs(u) - 1.0) < U_MARGIN)
        if not bad.any():
            return x, rounds - 1, int(moved.sum())
        target = mean + (0.5 - beta) / gamma * std
        x = np.where(bad, target, x64).astype(np.float32)
        moved |= bad
    raise AssertionError("the input did not settle")


def run_op(m, x, g):
    for q in m.parameters():
        q.grad = None
    xa = x.clone().requires_grad_()
    y = m(xa)
    y.backward(g.to(y.dtype))
    return y.detach(), xa.grad, {n: q.grad for n, q in m.named_parameters()}, xa


@pytest.mark.parametrize("gscale", [1.0, 1e-6], ids=["g1", "g1e-6"])
@pytest.mark.parametrize("case", WHOLE_CASES, ids=[c.name for c in WHOLE_CASES])
def test_whole_operation_against_the_float64_composition(cell_ops_on, case, gscale):
    m = build(case)
    ref = copy.deepcopy(m).double().cpu()
    xn, rounds, moved = settled_input(case, m)
    print("settling rounds:", rounds, "moved:", moved, "of", xn.size)
    assert rounds <= 5 and moved <= 0.01 * xn.size
    x = dev(xn)

    # the PReLU kink (tests/test_gpu_grouped_train.py): the HIP z is exactly +0.0 where the integer dot is 0, the float64
    # sum leaves a residue of either sign, removed on the reference side with the gradient passed through
    rconv = ref.op[1]
    half_alpha = 0.5 * rconv.weight_pre_process(rconv.weight).detach().abs().amax(dim=(1, 2, 3)).view(1, -1, 1, 1)
    removed = []

    def drop_residue(mod, inp, out):
        r = out.detach() * (out.detach().abs() < half_alpha)
        removed.append(r.abs().amax(dim=(0, 2, 3)))
        return out - r
    rconv.register_forward_hook(drop_residue)

    ho, wo = hipops.conv_out_hw(case.H, case.W, case.k, case.k, case.stride, case.pad, case.dilation)
    g = dev(gen.normal(case.seed + 5, (case.N, case.C_out, ho, wo)).astype(np.float32)) * gscale
    yr, gxr, pr, _ = run_op(ref, x.double().cpu(), g.double().cpu())
    n_terms = rconv.weight[0].numel()
    assert len(removed) == 1 and bool((removed[0] <= n_terms * n_terms * 2.0 ** -24 * 2 * half_alpha.view(-1)).all())

    before = fastpath.stats()
    training.saved_input_bytes(reset=True)
    saved = []

    def keep(t):
        saved.append(t)
        return t
    with torch.autograd.graph.saved_tensors_hooks(keep, lambda t: t):
        for q in m.parameters():
            q.grad = None
        xa = x.clone().requires_grad_()
        y = m(xa)
    after = fastpath.stats()
    assert after["cell_op_train"] == before["cell_op_train"] + 1 and after["conv2d_train"] == before["conv2d_train"]
    kept = training.saved_input_bytes(reset=True)
    assert kept == 3 * 8 * case.N * ((case.C_in + 63) // 64) * case.H * case.W             # P, M and T
    big = [t for t in saved if t.dtype == torch.float32 and t.numel() in (xa.numel(), y.numel())]
    assert all(t.data_ptr() == xa.data_ptr() for t in big) and len(big) <= 1, [tuple(t.shape) for t in big]
    assert sum(t.numel() * t.element_size() for t in saved if t.dtype == torch.int64) == kept
    y.backward(g)
    gx, pg = xa.grad, {n: q.grad for n, q in m.named_parameters()}

    assert y.dtype == torch.float32 and y.shape == yr.shape
    assert close(y, yr)
    assert close(gx, gxr)
    assert set(pg) == set(pr) and "op.1.weight" in pg and "op.2.weight" in pg
    assert ("op.0.weight" in pg) == case.affine
    for name in pr:
        assert pg[name] is not None and pr[name] is not None, name
        assert pg[name].shape == pr[name].shape and close_param(pg[name], pr[name]), name
    bn, rbn = m.op[0], ref.op[0]
    assert close(bn.running_mean, rbn.running_mean) and close(bn.running_var, rbn.running_var)
    assert int(bn.num_batches_tracked) == int(rbn.num_batches_tracked) == 1
    # two runs, the same bits (no atomics anywhere on the path)
    m2 = build(case)
    y2, gx2, pg2, _ = run_op(m2, x, g)
    assert torch.equal(y2, y.detach()) and torch.equal(gx2, gx)
    assert all(torch.equal(pg2[n], pg[n]) for n in pg)


def test_one_parameter_prelu_and_inputs_that_need_no_gradient(cell_ops_on):
    case = CELL_CASES[0]
    m = build(case)
    m.op[2] = torch.nn.PReLU(num_parameters=1, init=0.2).to(DEV)
    ref = copy.deepcopy(m).double().cpu()
    xn, _, _ = settled_input(case, m)
    x = dev(xn)
    rconv = ref.op[1]
    half_alpha = 0.5 * rconv.weight_pre_process(rconv.weight).detach().abs().amax(dim=(1, 2, 3)).view(1, -1, 1, 1)
    rconv.register_forward_hook(lambda mod, i, out: out - out.detach() * (out.detach().abs() < half_alpha))
    g = dev(gen.normal(case.seed + 5, case.xshape).astype(np.float32))
    before = fastpath.stats()["cell_op_train"]
    y = m(x)                                            # the input is data: only the parameters need gradients
    y.backward(g)
    assert fastpath.stats()["cell_op_train"] == before + 1
    yr = ref(x.double().cpu())
    yr.backward(g.double().cpu())
    assert close(y, yr)
    for (name, q), (_, r) in zip(m.named_parameters(), ref.named_parameters()):
        assert q.grad is not None and q.grad.shape == q.shape and close_param(q.grad, r.grad), name


# ---- 6. the switch ---------------------------------------------------------------------------------------------------
def test_the_switch_is_off_by_default_and_read_at_every_call(monkeypatch):
    assert training.CELL_OPS is (os.environ.get("BNN_AMD_TRAIN_CELL_OPS", "0") == "1")
    case = CELL_CASES[0]
    m = build(case)
    x = dev(case.input()).requires_grad_()
    monkeypatch.setattr(training, "GROUPED", True)
    seen = []
    for flag in (False, True, False):
        monkeypatch.setattr(training, "CELL_OPS", flag)
        before = fastpath.stats()
        y = m(x)
        after = fastpath.stats()
        seen.append((after["cell_op_train"] - before["cell_op_train"], after["conv2d_train"] - before["conv2d_train"]))
        assert y.shape == x.shape
    assert seen == [(0, 1), (1, 0), (0, 1)]             # off: the per-layer path, conv2d_train as before
    monkeypatch.setattr(training, "CELL_OPS", True)
    monkeypatch.setattr(training, "ENABLED", False)     # the master switch of the training paths
    before = fastpath.stats()
    m(x)
    assert fastpath.stats() == before


# ---- 7. a cell trains ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("drop_prob", [0.0, 0.2])
def test_a_cell_takes_a_training_step_on_the_fused_operations(monkeypatch, drop_prob):
    """No element-wise comparison (tests/test_gpu_grouped_train.py says why).  drop_prob > 0: Cell.forward rescales the
    function's output in place — which autograd accepts because the function does not save it."""
    monkeypatch.setattr(training, "CELL_OPS", True)
    monkeypatch.setattr(training, "GROUPED", True)
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
    n_ops = sum(1 for mod in cell.modules() if type(mod).__name__ in OP_NAMES)
    assert n_ops >= 4
    torch.manual_seed(1234)
    before = fastpath.stats()["cell_op_train"]
    a0, a1 = s0.clone().requires_grad_(), s1.clone().requires_grad_()
    loss = cell(a0, a1, drop_prob).square().mean()
    loss.backward()
    assert fastpath.stats()["cell_op_train"] == before + n_ops
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
        assert fastpath.stats()["cell"] == c0 + 1                               # FusedCell again
        assert bool(torch.isfinite(y_after).all()) and not torch.equal(y_after, y_before)

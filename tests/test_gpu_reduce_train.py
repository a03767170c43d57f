"""``FactorizedReduce`` in a training step as fused HIP launches (training.CELL_OPS: training.ReduceTrainFn).

The new kernels one by one — BatchNorm + sign + STE mask of the two pixel lattices as bit planes (csrc/pack_ste.hip:
bn_pack_ste_s2_kernel) bit for bit against the existing entry points and the CPU oracle, the BatchNorm backward of a
gradient that lives on those lattices (csrc/bn_train.hip) against float64 autograd — then the assumption the backward
rests on (the un-fused launches return the pre-activation value the fused ones started from), the whole module against
its float64 composition, the switch, and a reduction cell and the cell behind it taking a training step.

Tolerances are those of tests/test_gpu_cellops_train.py: outputs and input gradients rtol 1e-4, atol 1e-5 max|ref|;
parameter gradients rtol 1e-3, atol 1e-4 max|ref| + 1e-7."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bnn_amd as bnn
import oracle
from bnn_amd import fastpath, hipops, models, training
from bnn_amd.ops import BasicInputBinarizer, XNORWeightBinarizer
from tests.golden import cells_cases, gen

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OP_NAMES = ("SepConv", "DilConv", "ReLUConvBN")
EPS, MOMENTUM = 1e-5, 0.1

# (N, C, H, W) and the module's C_out
SHAPES = [(3, 72, 20, 18),      # cw64 = 2 with a ragged last word; 270 output pixels per word: two workgroups, the last one
                                # ragged; float2 rows; three images across splits
          (2, 24, 6, 10),       # C < 32; odd Wo
          (2, 96, 8, 8),        # float4 rows
          (5, 130, 4, 6),       # three words, the last one holding 2 channels
          (2, 48, 2, 2)]        # one output pixel per image
C_OUT = {72: 48, 24: 24, 96: 96, 130: 40, 48: 32}
IDS = ["x".join(map(str, s)) for s in SHAPES]


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


def build(C, affine=True, one_slope=False):
    """A binarised FactorizedReduce(C, C_OUT[C]) with deterministic state: gamma in [0.5, 1.5], beta in [-0.5, 0.5],
    slopes in [0.05, 0.45], kaiming weights."""
    m = models.FactorizedReduce(C, C_OUT[C], affine=affine)
    if one_slope:
        m.activation = torch.nn.PReLU(num_parameters=1)
    m = binarise(m)
    seed = gen.seed_of("reduce-train", C, int(affine), int(one_slope))
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    state = gen.model_state(shapes, seed)
    if affine:
        state["bn.bias"] = (gen.uniform(seed + 1, (C,)) - 0.5).astype(np.float32)
    state["activation.weight"] = (0.05 + 0.4 * gen.uniform(seed + 2, shapes["activation.weight"])).astype(np.float32)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    return m.to(DEV).train()


@pytest.fixture
def cell_ops_on(monkeypatch):
    monkeypatch.setattr(training, "CELL_OPS", True)


def same_planes(a, b):
    return torch.equal(a.sign.P, b.sign.P) and torch.equal(a.sign.M, b.sign.M) and torch.equal(a.T, b.T)


def phase(t, k):
    """The pixels (2i + k, 2j + k) of an NCHW array or tensor."""
    return t[:, :, k::2, k::2]


def bn_params(C, seed, affine):
    if not affine:
        return None, None
    return dev((0.5 + gen.uniform(seed, (C,))).astype(np.float32)), dev((gen.uniform(seed + 1, (C,)) - 0.5).astype(np.float32))


# ---- 1. the pack kernel, bit for bit ---------------------------------------------------------------------------------
# (name, x, a, b): u = fmaf(x, a, b) exactly representable; the edges of sign() and of the mask |u| < 1 (the table of
# tests/test_gpu_cellops_train.py)
ONE_DN, ONE_UP = 1.0 - 2.0 ** -24, 1.0 + 2.0 ** -23
EDGE_CASES = [("plus-zero", 3.0, 0.5, -1.5), ("minus-zero", -1.5, 0.0, -0.0), ("plus-one", 2.0, 0.5, 0.0),
              ("minus-one", 2.0, -0.5, 0.0), ("nan", float("nan"), 1.0, 0.0), ("below-one", ONE_DN, 1.0, 0.0),
              ("above-one", ONE_UP, 1.0, 0.0), ("above-minus-one", -ONE_DN, 1.0, 0.0), ("below-minus-one", ONE_UP, -1.0, 0.0),
              ("one-by-fma", 1.0, 0.5, 0.5), ("residue-below-one", 1.0, ONE_DN, 0.0)]
EDGE_BITS = [(0, 0, 1), (0, 0, 1), (1, 0, 0), (0, 1, 0), (0, 0, 0), (1, 0, 1), (1, 0, 0), (0, 1, 1), (0, 1, 0), (1, 0, 0),
             (1, 0, 1)]


def plant_affine(x, a, b, positions, rot):
    """Edge case ``j`` goes to channel ``(rot + j) % C``: its (a, b) into the channel's affine and its x to ``positions``
    [(y, x)] of every image.  Returns [(channel, j)]."""
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


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_bn_act_pack_ste_s2_planes_bit_for_bit(shape):
    N, C, H, W = shape
    seed = gen.seed_of("reduce-train-pack", "x".join(map(str, shape)))
    x = (1.5 * gen.normal(seed, shape)).astype(np.float32)
    a = ((0.5 + gen.uniform(seed + 1, (C,))) * np.where(gen.uniform(seed + 2, (C,)) < 0.2, -1, 1)).astype(np.float32)
    b = (0.4 * gen.normal(seed + 3, (C,))).astype(np.float32)
    # lattice positions of both phases: first and last pixel of each
    positions = sorted({(0, 0), (H - 2, W - 2), (1, 1), (H - 1, W - 1)})
    planted = plant_affine(x, a, b, positions, rot=C - 3)       # (wraps: channels of both words where there are two)
    got = hipops.bn_act_pack_ste_s2(dev(x), dev(a), dev(b))
    s2 = hipops.bn_act_pack_s2(dev(x), dev(a), dev(b), relu=False)
    assert len(got) == 2
    for k in range(2):
        xs = np.ascontiguousarray(phase(x, k))
        sv = got[k]
        assert tuple(sv.shape) == (N, C, H // 2, W // 2) and sv.T.shape == (N, (C + 63) // 64, H // 2, W // 2)
        assert sv.T.is_contiguous() and sv.sign.P.is_contiguous() and sv.sign.M.is_contiguous()
        # the existing three-plane kernel on a contiguous copy of the lattice; the existing two-plane lattice kernel
        assert same_planes(sv, hipops.bn_act_pack_ste(dev(xs), dev(a), dev(b)))
        assert torch.equal(sv.sign.P, s2[k].P) and torch.equal(sv.sign.M, s2[k].M)
        # the CPU oracle
        v = oracle.bn_act(xs, a, b)
        Pw, Mw = oracle.pack_act(v)
        P, M, T = u64(sv.sign.P), u64(sv.sign.M), u64(sv.T)
        assert np.array_equal(P, Pw) and np.array_equal(M, Mw)
        assert np.array_equal(T, oracle.pack_ste_mask(v))
        hit = 0
        for c, j in planted:
            for n in range(N):
                for y, xx in positions:
                    if y % 2 != k:
                        continue
                    bits = tuple(int((pl[n, c // 64, y // 2, xx // 2] >> np.uint64(c % 64)) & np.uint64(1)) for pl in (P, M, T))
                    assert bits == EDGE_BITS[j], (EDGE_CASES[j][0], k, n, c, bits)
                    hit += 1
        assert hit >= N * len(planted)
        if C % 64:      # channels past C in the last word stay 0
            high = ~np.uint64((1 << (C % 64)) - 1)
            assert not (P[:, -1] & high).any() and not (M[:, -1] & high).any() and not (T[:, -1] & high).any()
    # pixels off the lattices are not read: NaN and huge values there change no plane word
    x2 = x.copy()
    x2[:, :, 0::2, 1::2] = np.float32("nan")
    x2[:, :, 1::2, 0::2] = np.float32(3e38)
    x2[:, 0, 1::2, 0::2] = np.float32("-inf")
    got2 = hipops.bn_act_pack_ste_s2(dev(x2), dev(a), dev(b))
    assert same_planes(got2[0], got[0]) and same_planes(got2[1], got[1])
    # without an affine: pack_act_ste on the slices
    plain = hipops.bn_act_pack_ste_s2(dev(x))
    for k in range(2):
        assert same_planes(plain[k], hipops.pack_act_ste(dev(np.ascontiguousarray(phase(x, k)))))


# ---- 2. statistics + planes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("affine", [True, False], ids=["affine", "noaffine"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_bn_train_pack_ste_s2_has_the_statistics_of_bn_train_pack_ste(shape, affine):
    N, C, H, W = shape
    seed = gen.seed_of("reduce-train-stats", "x".join(map(str, shape)))
    x = dev((1.5 * gen.normal(seed, shape) + 0.25).astype(np.float32))
    gamma, beta = bn_params(C, seed + 7, affine)
    rm0, rv0 = dev((0.5 * gen.normal(seed + 2, (C,))).astype(np.float32)), dev((0.5 + gen.uniform(seed + 3, (C,))).astype(np.float32))
    rm1, rv1, rm2, rv2 = rm0.clone(), rv0.clone(), rm0.clone(), rv0.clone()
    _, mean1, invstd1, scale1, shift1 = hipops.bn_train_pack_ste(x, gamma, beta, rm1, rv1, MOMENTUM, EPS)
    phases, mean2, invstd2, scale2, shift2 = hipops.bn_train_pack_ste_s2(x, gamma, beta, rm2, rv2, MOMENTUM, EPS)
    assert torch.equal(mean1, mean2) and torch.equal(invstd1, invstd2)
    assert torch.equal(scale1, scale2) and torch.equal(shift1, shift2)
    assert torch.equal(rm1, rm2) and torch.equal(rv1, rv2) and not torch.equal(rm1, rm0) and not torch.equal(rv1, rv0)
    want = hipops.bn_act_pack_ste_s2(x, scale2, shift2)
    assert same_planes(phases[0], want[0]) and same_planes(phases[1], want[1])
    u = phase(x, 0) * scale2.view(1, C, 1, 1) + shift2.view(1, C, 1, 1)
    assert bool((u.abs() < 1).any()) and bool((u.abs() >= 1).any())


# ---- 3. BatchNorm backward from the two lattices ---------------------------------------------------------------------
def bn_backward_reference(x, gamma, g0, g1):
    """float64 autograd of F.batch_norm(training=True) with the gradient scattered onto the two lattices."""
    C = x.shape[1]
    x64 = x.double().cpu().requires_grad_()
    w64 = (gamma.double().cpu() if gamma is not None else torch.ones(C, dtype=torch.float64)).requires_grad_()
    b64 = torch.zeros(C, dtype=torch.float64, requires_grad=True)
    y = F.batch_norm(x64, None, None, w64, b64, True, MOMENTUM, EPS)
    gfull = torch.zeros_like(y)
    gfull[:, :, 0::2, 0::2] = g0.double().cpu()
    gfull[:, :, 1::2, 1::2] = g1.double().cpu()
    return torch.autograd.grad(y, (x64, w64, b64), gfull)


def offset_copy(x, nfloats=2):
    """A contiguous copy of ``x`` that starts ``nfloats`` floats into its storage."""
    store = torch.empty(x.numel() + nfloats, dtype=x.dtype, device=x.device)
    xo = store[nfloats:].view(x.shape)
    xo.copy_(x)
    return xo


BWD_CASES = [(s, False) for s in SHAPES] + [((2, 96, 8, 8), True)]


@pytest.mark.parametrize("affine", [True, False], ids=["gamma", "nogamma"])
@pytest.mark.parametrize("shape,offset", BWD_CASES, ids=IDS + ["2x96x8x8-8-bytes-in"])
def test_bn_train_backward_s2_against_float64_autograd(shape, offset, affine):
    N, C, H, W = shape
    seed = gen.seed_of("reduce-train-bnbwd", "x".join(map(str, shape)))
    x = dev((1.5 * gen.normal(seed, shape) + 0.25).astype(np.float32))
    if offset:      # the float4 shape demoted to float2 rows: x is 8, not 16, bytes aligned
        x = offset_copy(x)
        assert x.data_ptr() % 16 == 8 and x.is_contiguous()
    gamma, beta = bn_params(C, seed + 7, affine)
    _, mean, invstd = hipops.bn_train_forward(x, gamma, beta, None, None, MOMENTUM, EPS)
    gshape = (N, C, H // 2, W // 2)
    g0 = dev(gen.normal(seed + 4, gshape).astype(np.float32))
    g1 = dev(gen.normal(seed + 5, gshape).astype(np.float32))
    zero = torch.zeros_like(g0)
    for a0, a1 in ((g0, g1), (g0, zero), (zero, g1), (g0 * 1e-6, g1 * 1e-6)):
        dx, dgamma, dbeta = hipops.bn_train_backward_s2(a0, a1, x, mean, invstd, gamma)
        rdx, rdg, rdb = bn_backward_reference(x, gamma, a0, a1)
        assert dx.shape == x.shape and dx.is_contiguous()
        assert close(dx, rdx) and close_param(dgamma, rdg) and close_param(dbeta, rdb)
        dx2, dgamma2, dbeta2 = hipops.bn_train_backward_s2(a0, a1, x, mean, invstd, gamma)
        assert torch.equal(dx, dx2) and torch.equal(dgamma, dgamma2) and torch.equal(dbeta, dbeta2)   # bit-reproducible
    dx, dgamma, dbeta = hipops.bn_train_backward_s2(zero, zero, x, mean, invstd, gamma)
    assert bool((dx == 0).all()) and bool((dgamma == 0).all()) and bool((dbeta == 0).all())


# ---- 4. the recomputed z is the forward's z --------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_the_unfused_launches_return_the_pre_activation_value_of_the_fused_ones(shape):
    N, C, H, W = shape
    m = build(C)
    x = dev(gen.activation("normal", gen.seed_of("reduce-train-z", C), shape))
    bn = m.bn
    phases, _, _, _, _ = hipops.bn_train_pack_ste_s2(x, bn.weight, bn.bias, bn.running_mean.clone(), bn.running_var.clone(),
                                                     MOMENTUM, bn.eps)
    half = C_OUT[C] // 2
    slopes = m.activation.weight.detach()
    y = torch.empty((N, 2 * half, H // 2, W // 2), dtype=torch.float32, device=DEV)
    z = torch.empty_like(y)
    for k, conv in enumerate((m.conv_1[0], m.conv_2[0])):
        plan = fastpath._recognise(conv, conv.out_channels)
        packed = fastpath.packed_weight(conv, plan, sync=False, fresh=True)
        hipops.bconv2d_fused(phases[k].sign, packed, prelu=slopes[k * half:(k + 1) * half], out=y, out_c_offset=k * half)
        hipops.bconv2d_fused(phases[k].sign, packed, out=z, out_c_offset=k * half)
    want = F.prelu(z, slopes)
    assert bool((z[:, :half] != 0).any()) and bool((z[:, half:] != 0).any())
    assert torch.equal(y, want)


# ---- 5. the whole module against its float64 composition -------------------------------------------------------------
U_MARGIN = 1e-3


def settled_input(shape, m, seed):
    """A ``gen.activation("normal")`` input with every LATTICE element whose training-mode BatchNorm value u (float64,
    current batch statistics) lies within U_MARGIN of 0 or of +-1 moved to the x that gives u = 0.5, until none is left:
    sign() and the mask |u| < 1 then do not depend on fp32 rounding.  The other pixels pass no sign() and stay.  Returns
    (x fp32, rounds, elements moved)."""
    bn = m.bn
    C = bn.num_features
    gamma = (bn.weight.detach().double().cpu().numpy() if bn.weight is not None else np.ones(C)).reshape(1, C, 1, 1)
    beta = (bn.bias.detach().double().cpu().numpy() if bn.bias is not None else np.zeros(C)).reshape(1, C, 1, 1)
    x = gen.activation("normal", seed, shape).astype(np.float32)
    lattice = np.zeros(shape, bool)
    lattice[:, :, 0::2, 0::2] = True
    lattice[:, :, 1::2, 1::2] = True
    moved = np.zeros(shape, bool)
    for rounds in range(1, 20):
        x64 = x.astype(np.float64)
        mean = x64.mean(axis=(0, 2, 3), keepdims=True)
        std = np.sqrt(x64.var(axis=(0, 2, 3), keepdims=True) + bn.eps)
        u = (x64 - mean) / std * gamma + beta
        bad = lattice & ((np.abs(u) < U_MARGIN) | (np.abs(np.abs(u) - 1.0) < U_MARGIN))
        if not bad.any():
            return x, rounds - 1, int(moved.sum())
        target = mean + (0.5 - beta) / gamma * std
        x = np.where(bad, target, x64).astype(np.float32)
        moved |= bad
    raise AssertionError("the input did not settle")


def run_module(m, x, g):
    for q in m.parameters():
        q.grad = None
    xa = x.clone().requires_grad_()
    y = m(xa)
    y.backward(g.to(y.dtype))
    return y.detach(), xa.grad, {n: q.grad for n, q in m.named_parameters()}


VARIANTS = [(True, False), (False, True), (True, True), (False, False)]     # (affine BatchNorm, one-parameter PReLU)


@pytest.mark.parametrize("affine,one_slope", VARIANTS, ids=["affine-slopes", "noaffine-oneslope", "affine-oneslope",
                                                             "noaffine-slopes"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_whole_module_against_the_float64_composition(cell_ops_on, shape, affine, one_slope):
    N, C, H, W = shape
    seed = gen.seed_of("reduce-train-whole", "x".join(map(str, shape)))
    m = build(C, affine, one_slope)
    start = copy.deepcopy(m.state_dict())
    ref = copy.deepcopy(m).double().cpu()
    xn, rounds, moved = settled_input(shape, m, seed)
    print("settling rounds:", rounds, "moved:", moved, "of", xn.size)
    assert rounds <= 5 and moved <= 0.01 * xn.size
    x = dev(xn)

    # the PReLU kink (tests/test_gpu_grouped_train.py): the HIP z is exactly +0.0 where the integer dot is 0, the float64
    # sum leaves a residue of either sign, removed on the reference side with the gradient passed through
    removed, half_alphas = [], []
    for rconv in (ref.conv_1[0], ref.conv_2[0]):
        half_alpha = 0.5 * rconv.weight_pre_process(rconv.weight).detach().abs().amax(dim=(1, 2, 3)).view(1, -1, 1, 1)
        half_alphas.append(half_alpha)

        def drop_residue(mod, inp, out, half_alpha=half_alpha):
            r = out.detach() * (out.detach().abs() < half_alpha)
            removed.append(r.abs().amax(dim=(0, 2, 3)))
            return out - r
        rconv.register_forward_hook(drop_residue)

    gshape = (N, C_OUT[C], H // 2, W // 2)
    g1 = dev(gen.normal(seed + 5, gshape).astype(np.float32))
    first = None
    for gscale in (1.0, 1e-6):
        g = g1 * gscale
        ref.load_state_dict({k: v.double().cpu() for k, v in start.items()})
        del removed[:]
        yr, gxr, pr = run_module(ref, x.double().cpu(), g.double().cpu())
        n_terms = C
        assert len(removed) == 2
        for r, ha in zip(removed, half_alphas):
            assert bool((r <= n_terms * n_terms * 2.0 ** -24 * 2 * ha.view(-1)).all())

        m.load_state_dict(start)
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
        assert after["reduce_train"] == before["reduce_train"] + 1
        assert after["conv2d_train"] == before["conv2d_train"] and after["cell_op_train"] == before["cell_op_train"]
        kept = training.saved_input_bytes(reset=True)
        assert kept == 3 * 8 * 2 * N * ((C + 63) // 64) * (H // 2) * (W // 2)          # P, M and T of both phases
        big = [t for t in saved if t.dtype == torch.float32 and t.numel() in (xa.numel(), y.numel())]
        assert all(t.data_ptr() == xa.data_ptr() for t in big) and len(big) <= 1, [tuple(t.shape) for t in big]
        assert sum(t.numel() * t.element_size() for t in saved if t.dtype == torch.int64) == kept
        y.backward(g)
        gx, pg = xa.grad, {n: q.grad for n, q in m.named_parameters()}

        assert y.dtype == torch.float32 and y.shape == yr.shape == gshape
        assert close(y, yr)
        assert close(gx, gxr)
        assert set(pg) == set(pr) and {"conv_1.0.weight", "conv_2.0.weight", "activation.weight"} <= set(pg)
        assert ("bn.weight" in pg) == affine and ("bn.bias" in pg) == affine
        for name in pr:
            assert pg[name] is not None and pr[name] is not None, name
            assert pg[name].shape == pr[name].shape and close_param(pg[name], pr[name]), name
        assert close(m.bn.running_mean, ref.bn.running_mean) and close(m.bn.running_var, ref.bn.running_var)
        assert int(m.bn.num_batches_tracked) == int(ref.bn.num_batches_tracked) == 1
        if first is None:
            first = (y.detach().clone(), gx.clone(), {n: v.clone() for n, v in pg.items()})
    # a second run from equal state, the same bits (no atomics anywhere on the path)
    m.load_state_dict(start)
    y2, gx2, pg2 = run_module(m, x, g1)
    assert torch.equal(y2, first[0]) and torch.equal(gx2, first[1])
    assert all(torch.equal(pg2[n], first[2][n]) for n in pg2)


# ---- 6. switch and declines on the device ----------------------------------------------------------------------------
def test_the_switch_is_read_at_every_call_and_declines_fall_through(monkeypatch):
    assert training.CELL_OPS is (os.environ.get("BNN_AMD_TRAIN_CELL_OPS", "0") == "1")
    shape = SHAPES[1]
    m = build(shape[1])
    x = dev(gen.activation("normal", 11, shape)).requires_grad_()
    seen = []
    for flag in (False, True, False):
        monkeypatch.setattr(training, "CELL_OPS", flag)
        before = fastpath.stats()["reduce_train"]
        y = m(x)
        seen.append(fastpath.stats()["reduce_train"] - before)
        assert y.shape == (shape[0], C_OUT[shape[1]], shape[2] // 2, shape[3] // 2)
    assert seen == [0, 1, 0]
    monkeypatch.setattr(training, "CELL_OPS", True)
    monkeypatch.setattr(training, "ENABLED", False)     # the master switch of the training paths
    before = fastpath.stats()
    m(x)
    assert fastpath.stats() == before
    monkeypatch.setattr(training, "ENABLED", True)
    # odd H: the rule declines, and the module's own forward raises as before (its halves have two shapes)
    xo = dev(gen.activation("normal", 12, (2, shape[1], 5, 6))).requires_grad_()
    before = fastpath.stats()["reduce_train"]
    assert training.reduce_train(m, xo) is None
    with pytest.raises(RuntimeError):
        m(xo)
    assert fastpath.stats()["reduce_train"] == before


def declined_on_the_device(m, x, through_the_input=True):
    """With the switch on ``m(x)`` moves no ``reduce_train`` and equals, bit for bit, what a module of the same state
    returns with the switch off; it still trains (every parameter gets a finite gradient)."""
    twin = copy.deepcopy(m)
    assert training.CELL_OPS
    before = fastpath.stats()["reduce_train"]
    xa = x.clone().requires_grad_()
    y = m(xa)
    assert fastpath.stats()["reduce_train"] == before
    assert training.reduce_train(m, xa) is None
    training.CELL_OPS = False
    try:
        want = twin(x.clone().requires_grad_())
    finally:
        training.CELL_OPS = True
    assert torch.equal(y, want)
    y.square().mean().backward()
    behind = ("conv_1.0.weight", "conv_2.0.weight", "activation.weight")
    if through_the_input:
        assert bool(torch.isfinite(xa.grad).all())
    else:       # AdvancedInputBinarizer takes its sign under no_grad (ops.py): nothing reaches the BatchNorm or x
        assert xa.grad is None
    for name, q in m.named_parameters():
        if through_the_input or name in behind or name.endswith("bias") and name.startswith("conv"):
            assert q.grad is not None and bool(torch.isfinite(q.grad).all()), name


# (N, C, H, W) whose phases hold an ODD number of plane words, N * ceil(C / 64) * H/2 * W/2: the second phase of the one
# phase-major allocation then starts 8 bytes off a 16-byte boundary, which the convolution launch refuses
ODD_WORD_SHAPES = [(3, 24, 6, 6), (1, 24, 6, 6), (3, 48, 2, 2)]


@pytest.mark.parametrize("shape", ODD_WORD_SHAPES, ids=["x".join(map(str, s)) for s in ODD_WORD_SHAPES])
def test_an_odd_number_of_plane_words_per_phase_is_declined_and_still_trains(cell_ops_on, shape):
    N, C, H, W = shape
    assert (N * ((C + 63) // 64) * (H // 2) * (W // 2)) % 2 == 1
    m = build(C)
    x = dev(gen.activation("normal", gen.seed_of("reduce-train-odd", *shape), shape))
    declined_on_the_device(m, x)
    # the same module takes the path again on an even count
    even = dev(gen.activation("normal", 15, (2 * N, C, H, W))).requires_grad_()
    before = fastpath.stats()["reduce_train"]
    m(even).sum().backward()
    assert fastpath.stats()["reduce_train"] == before + 1
    # the planes themselves are written for any count: only the convolution launch needs the alignment
    a, b = dev((0.5 + gen.uniform(16, (C,))).astype(np.float32)), dev((gen.uniform(17, (C,)) - 0.5).astype(np.float32))
    got = hipops.bn_act_pack_ste_s2(x, a, b)
    for k in range(2):
        assert same_planes(got[k], hipops.bn_act_pack_ste(phase(x, k).contiguous(), a, b))
    assert got[1].sign.P.data_ptr() % 16 == 8


def binarise_with(m, **recipe):
    cfg = bnn.BConfig(**dict(dict(activation_pre_process=BasicInputBinarizer, activation_post_process=bnn.Identity,
                                  weight_pre_process=XNORWeightBinarizer), **recipe))
    return bnn.prepare_binary_model(m, cfg)


def load_state(m, seed):
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict({k: torch.from_numpy(v) for k, v in gen.model_state(shapes, seed).items()})
    return m.to(DEV).train()


DECLINES = ["bias", "hook-on-conv", "hook-on-binarizer", "backward-hook", "post-scale", "advanced-binarizer", "groups-2",
            "3x3", "bn-eval", "bn-no-running-stats"]


@pytest.mark.parametrize("what", DECLINES)
def test_each_decline_rule_on_the_device(cell_ops_on, what):
    """Every other condition of the rule holds (a HIP module, fp32, training mode, autograd, an even word count): the one
    named here is what makes ``reduce_train`` decline."""
    shape = SHAPES[1]
    N, C, H, W = shape
    O = C_OUT[C]
    x = dev(gen.activation("normal", gen.seed_of("reduce-train-decline", what), shape))
    seed = gen.seed_of("reduce-train-decline-state", what)
    f = models.FactorizedReduce(C, O)
    if what in ("groups-2", "3x3"):
        conf = dict(kernel_size=3, padding=1) if what == "3x3" else dict(kernel_size=1, groups=2)
        f.conv_1 = torch.nn.Sequential(torch.nn.Conv2d(C, O // 2, stride=2, bias=False, **conf))
        f.conv_2 = torch.nn.Sequential(torch.nn.Conv2d(C, O // 2, stride=2, bias=False, **conf))
    if what == "bn-no-running-stats":
        f.bn = torch.nn.BatchNorm2d(C, track_running_stats=False)
    if what == "post-scale":
        from bnn_amd.ops import BasicScaleBinarizer
        m = binarise_with(f, activation_post_process=BasicScaleBinarizer)
    elif what == "advanced-binarizer":
        from bnn_amd.ops import AdvancedInputBinarizer
        m = binarise_with(f, activation_pre_process=AdvancedInputBinarizer)
    else:
        m = binarise(f)
    m = load_state(m, seed)
    # the module as built takes the path, unless the condition is one of its construction
    built_in = what in ("groups-2", "3x3", "bn-no-running-stats", "post-scale", "advanced-binarizer")
    before = fastpath.stats()["reduce_train"]
    m(x.clone().requires_grad_())
    assert fastpath.stats()["reduce_train"] == before + (0 if built_in else 1)
    m = load_state(m.cpu(), seed)
    if what == "bias":
        m.conv_1[0].bias = torch.nn.Parameter(0.1 * torch.ones(O // 2, device=DEV))
    elif what == "hook-on-conv":
        m.conv_2[0].register_forward_hook(lambda mod, i, o: None)
    elif what == "hook-on-binarizer":
        m.conv_1[0].activation_pre_process.register_forward_hook(lambda mod, i, o: None)
    elif what == "backward-hook":
        m.activation.register_full_backward_hook(lambda mod, gi, go: None)
    elif what == "bn-eval":
        m.bn.eval()
    declined_on_the_device(m, x, through_the_input=what != "advanced-binarizer")


def test_inputs_that_need_no_gradient(cell_ops_on):
    shape = SHAPES[1]
    m = build(shape[1])
    x = dev(gen.activation("normal", 13, shape))
    g = dev(gen.normal(14, (shape[0], C_OUT[shape[1]], shape[2] // 2, shape[3] // 2)).astype(np.float32))
    start = copy.deepcopy(m.state_dict())
    _, gx, full = run_module(m, x, g)
    assert gx is not None
    m.load_state_dict(start)
    m.bn.weight.requires_grad_(False)
    m.bn.bias.requires_grad_(False)
    for q in m.parameters():
        q.grad = None
    before = fastpath.stats()["reduce_train"]
    y = m(x)                                            # the input is data and the BatchNorm is frozen
    y.backward(g)
    assert fastpath.stats()["reduce_train"] == before + 1
    assert m.bn.weight.grad is None and m.bn.bias.grad is None
    for name in ("conv_1.0.weight", "conv_2.0.weight", "activation.weight"):
        got = dict(m.named_parameters())[name].grad
        assert got is not None and torch.equal(got, full[name]), name          # the same kernels on the same operands


# ---- 7. a reduction cell and the cell behind it train ----------------------------------------------------------------
@pytest.mark.parametrize("drop_prob", [0.0, 0.2])
@pytest.mark.parametrize("case", cells_cases.CELL_CASES[1:3], ids=[c.name for c in cells_cases.CELL_CASES[1:3]])
def test_a_cell_with_factorized_reduce_takes_a_training_step(monkeypatch, case, drop_prob):
    """No element-wise comparison (tests/test_gpu_grouped_train.py says why).  drop_prob > 0: Cell.forward rescales the
    function's output in place — which autograd accepts because the function does not save it."""
    monkeypatch.setattr(training, "CELL_OPS", True)
    monkeypatch.setattr(training, "GROUPED", True)
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
    n_red = sum(1 for mod in cell.modules() if type(mod).__name__ == "FactorizedReduce")
    assert n_ops >= 4 and n_red >= 1
    torch.manual_seed(1234)
    before = fastpath.stats()
    a0, a1 = s0.clone().requires_grad_(), s1.clone().requires_grad_()
    loss = cell(a0, a1, drop_prob).square().mean()
    loss.backward()
    after = fastpath.stats()
    assert after["reduce_train"] == before["reduce_train"] + n_red
    assert after["cell_op_train"] == before["cell_op_train"] + n_ops
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

"""The fused ImageNet stems of a BATS network on the GPU: both kernels against their float64 restatements
(tests/batsnet_imagenet_ref.py) and the reference's fixture, the planes of the second against bn_act_pack_multi on its own
output bit for bit, and FusedBATSNetwork with the fused stems against a composed run of the same kernels as modules."""
import copy
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import bnn_amd as bnn
from bnn_amd import batsnet, hipops, models, native, ops
from bnn_amd.batsnet import LAUNCHES, FusedBATSNetwork
from bnn_amd.executor import fold_bn
from tests.batsnet_imagenet_ref import gconv3x3s2_f64, stem_s2x2_f64
from tests.golden import batsnet_imagenet_cases as case
from tests.golden import gen

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TH, TW = hipops.STEM_S2_TILE
# 1x1: eight of nine taps of both convolutions are padding; 2x3 / 7x9: odd H1 / W1 (far-edge padding of the second
# convolution) next to even ones; 16x16; 37x34: H1 = 19 odd, W1 = 17 odd.  The last shape of each list comes from the
# exported tile: two tiles in each dimension of the kernel's OUTPUT, the second one ragged (one row, one column).
HWS = [(1, 1), (2, 3), (7, 9), (16, 16), (37, 34)]
HWS_A = HWS + [(4 * (TH + 1) - 1, 4 * (TW + 1) - 2)]           # (a): output ceil(ceil(H / 2) / 2)
HWS_B = HWS + [(2 * (TH + 1) - 1, 2 * (TW + 1) - 1)]           # (b): output ceil(H / 2)
# (C, G): 80 / 4 puts channels 60..63 of group 3 in plane word 0 and 64..79 in word 1
WIDTHS = [(20, 1), (48, 2), (60, 3), (80, 4)]
ids_hw = lambda v: f"{v[0]}x{v[1]}"                            # noqa: E731
ids_cg = lambda v: f"C{v[0]}G{v[1]}"                           # noqa: E731


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def half(v):
    return (v + 1) // 2


def test_the_tile_shapes_span_two_ragged_tiles():
    for (H, W), out in ((HWS_A[-1], lambda v: half(half(v))), (HWS_B[-1], half)):
        assert TH < out(H) < 2 * TH and TW < out(W) < 2 * TW and out(H) % TH and out(W) % TW


def bn_consts(seed, C):
    """A folded BatchNorm: a quarter of the slopes negative; every other shift positive, so that max(t, 0) != 0 where a
    fused kernel might take the first convolution's value outside its map."""
    s = ((0.5 + gen.uniform(seed, (C,))) * np.where(gen.uniform(seed + 1, (C,)) < 0.25, -1, 1)).astype(np.float32)
    t = (0.3 * gen.normal(seed + 2, (C,))).astype(np.float32)
    t[::2] = np.abs(t[::2]) + 0.25
    return s, t


def affines(K, C, seed):
    """K BatchNorm-like affines, a fifth of the slopes negative, shift 0 in channel 1 of the first."""
    a = (0.5 + gen.uniform(seed, (K, C))).astype(np.float32) * np.where(gen.uniform(seed + 1, (K, C)) < 0.2, -1, 1)
    b = (0.4 * gen.normal(seed + 2, (K, C))).astype(np.float32)
    b[0, 1] = 0.0
    return a.astype(np.float32), b


# ---- kernel (a) ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_a(hw, cg, N):
    (H, W), (C, G) = hw, cg
    C1 = C // 2
    seed = gen.seed_of("stem_s2x2", H, W, C, G, N)
    x = gen.activation("normal", seed, (N, 3, H, W))
    w1 = gen.conv_weight("kaiming", seed + 1, (C1, 3, 3, 3))
    w2 = gen.conv_weight("kaiming", seed + 2, (C, C1 // G, 3, 3))
    (s1, t1), (s2, t2) = bn_consts(seed + 3, C1), bn_consts(seed + 6, C)
    assert (t1 > 0).any()
    host = tuple(torch.from_numpy(v) for v in (x, w1, s1, t1, w2, s2, t2))
    refs = {r: tuple(v.numpy() for v in stem_s2x2_f64(*host, G, r)) for r in (False, True)}
    return tuple(v.to(DEV) for v in host), refs


@pytest.mark.parametrize("hw", HWS_A, ids=ids_hw)
@pytest.mark.parametrize("cg", WIDTHS, ids=ids_cg)
def test_stem0_kernel_against_float64(hw, cg):
    for N in (1, 3):
        args, refs = case_a(hw, cg, N)
        for relu_out in (False, True):
            y = hipops.stem_s2x2(*args, cg[1], relu_out)
            y64, bound = refs[relu_out]
            assert tuple(y.shape) == y64.shape == (N, cg[0], half(half(hw[0])), half(half(hw[1])))
            err = np.abs(y.cpu().numpy().astype(np.float64) - y64)
            print(f"(a) {hw} {cg} N={N} relu_out={relu_out}: max err / bound = {float((err / bound).max()):.3g}")
            assert (err <= bound).all(), (N, relu_out, float((err / bound).max()))
            assert not relu_out or float(y.min()) >= 0.0


def test_stem0_wrapper_cuts_a_batch_that_is_too_large_and_checks_shapes(monkeypatch):
    hw, cg = (7, 9), (60, 3)
    args, _ = case_a(hw, cg, 3)
    whole = hipops.stem_s2x2(*args, cg[1], True)
    monkeypatch.setattr(hipops, "_STEM_S2_MAX_ELEMS", 2 * max(3 * 7 * 9, 60 * 2 * 3))     # two images per launch
    before = native.launch_count()
    cut = hipops.stem_s2x2(*args, cg[1], True)
    assert native.launch_count() - before == 2
    assert torch.equal(cut, whole)
    x, w1, s1, t1, w2, s2, t2 = args
    with pytest.raises(native.NativeError):
        hipops.stem_s2x2(x[:, :2], w1, s1, t1, w2, s2, t2, 3)                 # not three input channels
    with pytest.raises(native.NativeError):
        hipops.stem_s2x2(x, w1, s1, t1, w2, s2, t2, 2)                        # w2 is [60, 10, 3, 3]: not two groups
    with pytest.raises(native.NativeError):
        hipops.stem_s2x2(x, w1, s1[:-1], t1, w2, s2, t2, 3)
    with pytest.raises(native.NativeError):
        hipops.stem_s2x2(x.cpu(), w1, s1, t1, w2, s2, t2, 3)


# ---- kernel (b) ----------------------------------------------------------------------------------------------------
ZERO_CH = 1          # the ternary case: this output channel has all-zero weights and shift 0 (affines(): shift 0 too)


@functools.lru_cache(maxsize=None)
def case_b(hw, cg, N):
    (H, W), (C, G) = hw, cg
    seed = gen.seed_of("gconv3x3s2", H, W, C, G, N)
    x = gen.activation("normal", seed, (N, C, H, W))
    w = gen.conv_weight("kaiming", seed + 1, (C, C // G, 3, 3))
    s, t = bn_consts(seed + 2, C)
    w[ZERO_CH] = 0.0
    t[ZERO_CH] = 0.0
    host = tuple(torch.from_numpy(v) for v in (x, w, s, t))
    refs = {r: tuple(v.numpy() for v in gconv3x3s2_f64(*host, G, r)) for r in (False, True)}
    return tuple(v.to(DEV) for v in host), refs


@pytest.mark.parametrize("hw", HWS_B, ids=ids_hw)
@pytest.mark.parametrize("cg", WIDTHS, ids=ids_cg)
def test_stem1_kernel_against_float64_and_its_planes_against_pack_multi(hw, cg):
    C, G = cg
    zeros_seen = 0
    for N in (1, 3):
        args, refs = case_b(hw, cg, N)
        for relu_in in (False, True):
            y0, none = hipops.gconv3x3s2_bn_pack(*args, G, relu_in=relu_in)                      # K = 0
            y64, bound = refs[relu_in]
            assert none == [] and tuple(y0.shape) == y64.shape == (N, C, half(hw[0]), half(hw[1]))
            err = np.abs(y0.cpu().numpy().astype(np.float64) - y64)
            live = bound > 0                           # (the all-zero channel: err = bound = 0)
            print(f"(b) {hw} {cg} N={N} relu_in={relu_in}: max err / bound = {float((err[live] / bound[live]).max()):.3g}")
            assert (err <= bound).all(), (N, relu_in, float((err[live] / bound[live]).max()))
            for K in (1, 3):
                a, b = (dev(v) for v in affines(K, C, gen.seed_of("gconv-aff", C, K)))
                y, sets = hipops.gconv3x3s2_bn_pack(*args, G, a, b, relu_in=relu_in)
                blind, unseen = hipops.gconv3x3s2_bn_pack(*args, G, a, b, relu_in=relu_in, out_f32=False)
                assert torch.equal(y, y0) and blind is None                                      # K = 0 gives the same y
                want = hipops.bn_act_pack_multi(y, a, b, relu=False)
                assert len(sets) == len(unseen) == len(want) == K
                for k in range(K):
                    assert torch.equal(sets[k].P, want[k].P) and torch.equal(sets[k].M, want[k].M), (N, K, k)
                    assert torch.equal(unseen[k].P, sets[k].P) and torch.equal(unseen[k].M, sets[k].M), (N, K, k)
                    assert sets[k].shape == want[k].shape == tuple(y.shape) and not sets[k].nonneg
                # the ternary case: y = fma(0, s, 0) = 0 and u = fma(0, a, 0) = 0 in affine 0: both bits clear everywhere
                assert float(y[:, ZERO_CH].abs().max()) == 0.0
                bit = lambda plane: (plane[:, 0] >> ZERO_CH) & 1                                 # noqa: E731
                assert int((bit(sets[0].P) | bit(sets[0].M)).sum()) == 0
                zeros_seen += y[:, ZERO_CH].numel()
    assert zeros_seen > 0


def test_stem1_wrapper_cuts_a_batch_that_is_too_large_and_checks_shapes(monkeypatch):
    hw, cg = (7, 9), (80, 4)
    args, _ = case_b(hw, cg, 3)
    a, b = (dev(v) for v in affines(3, 80, gen.seed_of("gconv-aff", 80, 3)))
    y, sets = hipops.gconv3x3s2_bn_pack(*args, 4, a, b, relu_in=True)
    monkeypatch.setattr(hipops, "_STEM_S2_MAX_ELEMS", 2 * 80 * 7 * 9)          # two images per launch
    before = native.launch_count()
    y2, sets2 = hipops.gconv3x3s2_bn_pack(*args, 4, a, b, relu_in=True)
    assert native.launch_count() - before == 2
    assert torch.equal(y2, y)
    for k in range(3):
        assert torch.equal(sets2[k].P, sets[k].P) and torch.equal(sets2[k].M, sets[k].M)
    x, w, s, t = args
    with pytest.raises(native.NativeError):
        hipops.gconv3x3s2_bn_pack(x, w, s, t, 2)                               # w is [80, 20, 3, 3]: not two groups
    with pytest.raises(native.NativeError):
        hipops.gconv3x3s2_bn_pack(x, w, s, t, 4, out_f32=False)                # nothing would be written
    with pytest.raises(native.NativeError):
        hipops.gconv3x3s2_bn_pack(x, w, s, t, 4, a[:, :-1], b[:, :-1])
    with pytest.raises(native.NativeError):
        hipops.gconv3x3s2_bn_pack(x, w, s, t, 4, torch.cat([a, a]), torch.cat([b, b]))           # six affines


# ---- the reference's fixture ---------------------------------------------------------------------------------------
def build_real(layers_real=case.REAL_LAYERS):
    net = case.binarise_real_stems(bnn, ops, case.build(models))
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict({k: torch.from_numpy(v) for k, v in case.state(shapes).items()})
    return net.to(DEV).eval()


def stem_args(net):
    conv0, bn0, _, conv1, bn1 = net.stem0
    _, conv2, bn2 = net.stem1
    return (conv0.weight.detach(), *fold_bn(bn0), conv1.weight.detach(), *fold_bn(bn1)), conv1.groups, \
        (conv2.weight.detach(), *fold_bn(bn2)), conv2.groups


def test_both_kernels_reproduce_the_reference_fixture(golden_dir):
    golden = np.load(os.path.join(golden_dir, "batsnet_imagenet_stem.npz"))
    ref0, ref1 = (torch.from_numpy(golden[case.NAME + "/" + k]) for k in ("s0", "s1"))
    net = build_real()
    a0, g0, a1, g1 = stem_args(net)
    x = torch.from_numpy(case.inputs())
    s0 = hipops.stem_s2x2(x.to(DEV), *a0, g0, relu_out=True)       # the fixture's s0 was read after stem1's in-place ReLU
    y64, bound = stem_s2x2_f64(x, *(v.cpu() for v in a0), g0, True)
    for name, got in (("kernel", s0.cpu()), ("reference", ref0)):
        err = (got.double() - y64).abs()
        print(f"s0 {name}: max err / bound = {float((err / bound).max()):.3g}")
        assert bool((err <= bound).all()), name
    s1, _ = hipops.gconv3x3s2_bn_pack(s0, *a1, g1, relu_in=True)
    for name, got, src in (("kernel", s1.cpu(), s0.cpu()), ("reference", ref1, ref0)):
        y64, bound = gconv3x3s2_f64(src, *(v.cpu() for v in a1), g1, True)
        err = (got.double() - y64).abs()
        print(f"s1 {name}: max err / bound = {float((err / bound).max()):.3g}")
        assert bool((err <= bound).all()), name


# ---- the network ---------------------------------------------------------------------------------------------------
class ComposedStem0(nn.Module):
    """stem0 as a module that calls the kernel: what the executor runs as a ``module`` step."""

    def __init__(self, seq):
        super().__init__()
        self.seq = seq

    def forward(self, x):
        conv0, bn0, _, conv1, bn1 = self.seq
        return hipops.stem_s2x2(x, conv0.weight, *fold_bn(bn0), conv1.weight, *fold_bn(bn1), conv1.groups, relu_out=True)


class ComposedStem1(nn.Module):
    def __init__(self, seq):
        super().__init__()
        self.seq = seq

    def forward(self, x):
        _, conv, bn = self.seq
        return hipops.gconv3x3s2_bn_pack(x, conv.weight, *fold_bn(bn), conv.groups, relu_in=False)[0]


def composed(net):
    twin = copy.deepcopy(net)                   # the same parameters; only the two stems are swapped
    twin.stem0, twin.stem1 = ComposedStem0(twin.stem0), ComposedStem1(twin.stem1)
    return twin


def launches(fn):
    before = native.launch_count()
    out = fn()
    return out, native.launch_count() - before


def test_network_with_fused_stems_equals_the_composed_run_bit_for_bit(monkeypatch):
    monkeypatch.setattr(batsnet, "FUSE_IMAGENET_STEMS", True)
    net = build_real()
    x = dev(gen.activation("normal", gen.seed_of("batsnet-imagenet-x"), (2, 3, 224, 224)))
    twin = composed(net)
    eng, ref = FusedBATSNetwork(net), FusedBATSNetwork(twin)
    steps = eng.steps
    assert [k for k, _ in steps[:2]] == ["stem_s2x2", "stem_s2_pack"] and "module" not in [k for k, _ in steps]
    assert [k for k, _ in ref.steps[:3]] == ["module", "module", "pack_handoff"]
    with torch.no_grad():
        want = ref(x)[0]
        got, aux = eng(x)
        assert aux is None and torch.equal(got, want)
        (got2, _), n = launches(lambda: eng(x))
        assert torch.equal(got2, want)
        assert n == sum(LAUNCHES.get(k, 0) for k, _ in steps)
        # a write the version counters do not see is picked up by refresh()
        net.stem0[3].weight.data.mul_(-0.5)
        twin.stem0.seq[3].weight.data.mul_(-0.5)
        eng.refresh()
        ref.refresh()
        got3, want3 = eng(x)[0], ref(x)[0]
        assert torch.equal(got3, want3) and not torch.equal(got3, want)
        # the switch off: the module stems of the plan before (their logits differ by the library convolutions' rounding
        # in front of sign(), so only the plan and the shape are checked)
        monkeypatch.setattr(batsnet, "FUSE_IMAGENET_STEMS", False)
        eng.refresh()
        assert [k for k, _ in eng.steps[:2]] == ["module", "module"]
        assert eng(x)[0].shape == want.shape
    torch.cuda.synchronize()


def test_graph_replay_with_fused_stems_equals_the_eager_executor(monkeypatch):
    monkeypatch.setattr(batsnet, "FUSE_IMAGENET_STEMS", True)
    net = build_real()
    eager, eng = FusedBATSNetwork(net), FusedBATSNetwork(net)
    x = dev(gen.activation("normal", gen.seed_of("batsnet-imagenet-graph-x"), (1, 3, 224, 224)))
    x2 = dev(gen.activation("normal", gen.seed_of("batsnet-imagenet-graph-x2"), (1, 3, 224, 224)))
    with torch.no_grad():
        want, want2 = eager(x)[0], eager(x2)[0]
        assert not torch.equal(want, want2)
        assert eng.capture(x) is eng and eng.steps[0][0] == "stem_s2x2"
        assert torch.equal(eng.replay(), want)
        eng.input.copy_(x2)
        assert torch.equal(eng.replay(), want2)
    torch.cuda.synchronize()

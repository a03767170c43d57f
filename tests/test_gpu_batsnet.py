"""A whole BATS network as one executor on the GPU: the stem kernel against its float64 restatement and against
bn_act_pack_multi on its own output, cells taking planes made outside, FusedBATSNetwork against net(x) bit for bit and
against the reference's fixture (tests/golden/batsnet.npz), its cache, and its HIP graph."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bnn_amd as bnn
from bnn_amd import fastpath, hipops, models, native, ops
from bnn_amd.batsnet import LAUNCHES, FusedBATSNetwork
from bnn_amd.cellops import FusedCell
from bnn_amd.inference import FusionError
from tests.golden import gen
from tests.golden.batsnet_cases import BATSNET_CASE, binarise_real_ends
from tests.golden.cells_cases import CELL_CASES, GROUPS, IMAGENET_ARGS, NET_CASE, genotype

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def binarise(model):
    cfg = bnn.BConfig(activation_pre_process=ops.BasicInputBinarizer, activation_post_process=bnn.Identity,
                      weight_pre_process=ops.XNORWeightBinarizer)
    return bnn.prepare_binary_model(model, cfg)


def load(model, seed):
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(v) for k, v in gen.model_state(shapes, seed).items()})
    return model.to(DEV).eval()


def build(case):
    """test_gpu_cells.build: everything binary, the stem and the classifier included."""
    return load(binarise(case.build(models)), case.seed())


def build_real(case=BATSNET_CASE):
    return load(binarise_real_ends(bnn, ops, case.build(models)), case.seed())


def affines(K, C, seed):
    """test_gpu_cells.affines — K BatchNorm-like affines, a fifth of the slopes negative, so that zero crossings fall
    inside the (non-negative) data — with shift 0 in channel 1 of the first: there sign(0) = 0 wherever the ReLU cut."""
    a = (0.5 + gen.uniform(seed, (K, C))).astype(np.float32) * np.where(gen.uniform(seed + 1, (K, C)) < 0.2, -1, 1)
    b = (0.4 * gen.normal(seed + 2, (K, C))).astype(np.float32)
    b[0, 1] = 0.0
    return a.astype(np.float32), b


# ---- 1 + 2. the stem kernel ----------------------------------------------------------------------------------------
# 8x8: 4 pixels per thread up to K = 2 (16-byte vectors), else 2; 10x9: 2 per thread (8-byte); 7x9: 1 (odd on both
# sides); 1x1: eight of nine taps are padding.  O = 48: less than one 64-channel word; 72: one word + 8 bits (NET_CASE's
# 3C); 144: two words + 16.
HWS = [(8, 8), (10, 9), (7, 9), (1, 1)]
WIDTHS = [48, 72, 144]


@functools.lru_cache(maxsize=None)
def stem_case(hw, O, N):
    """Inputs and the float64 restatement y64 = max(s conv(x, w) + t, 0) with its bound, computed once per shape."""
    H, W = hw
    seed = gen.seed_of("stem3x3", H, W, O, N)
    x = gen.activation("normal", seed, (N, 3, H, W))
    w = gen.conv_weight("kaiming", seed + 1, (O, 3, 3, 3))
    s = ((0.5 + gen.uniform(seed + 2, (O,))) * np.where(gen.uniform(seed + 3, (O,)) < 0.25, -1, 1)).astype(np.float32)
    t = (0.3 * gen.normal(seed + 4, (O,))).astype(np.float32)
    x64, w64 = torch.from_numpy(x).double(), torch.from_numpy(w).double()
    s64, t64 = (torch.from_numpy(v).double().view(1, O, 1, 1) for v in (s, t))
    y64 = torch.clamp_min(s64 * F.conv2d(x64, w64, padding=1) + t64, 0.0)
    # gamma_28 (27 fused multiply-adds and the BatchNorm's) rounded up to 32 u, on the magnitudes; ReLU is 1-Lipschitz
    bound = 32 * 2.0 ** -24 * (s64.abs() * F.conv2d(x64.abs(), w64.abs(), padding=1) + t64.abs())
    return tuple(dev(v) for v in (x, w, s, t)) + (y64.numpy(), bound.numpy())


@pytest.mark.parametrize("hw", HWS, ids=lambda v: f"{v[0]}x{v[1]}")
@pytest.mark.parametrize("O", WIDTHS)
def test_stem_kernel_against_float64(hw, O):
    for N in (1, 3):
        x, w, s, t, y64, bound = stem_case(hw, O, N)
        for K in (1, 3):
            a, b = affines(K, O, gen.seed_of("stem-aff", O, K))
            y, sets = hipops.stem3x3_bn_relu_pack(x, w, s, t, dev(a), dev(b))
            assert y.shape == (N, O) + hw and len(sets) == K
            err = np.abs(y.cpu().numpy().astype(np.float64) - y64)
            print(f"{hw} O={O} N={N} K={K}: max err / bound = {float((err / bound).max()):.3g}")
            assert (err <= bound).all(), (N, K, float((err / bound).max()))
            assert float(y.min()) >= 0.0


@pytest.mark.parametrize("hw", HWS, ids=lambda v: f"{v[0]}x{v[1]}")
@pytest.mark.parametrize("O", WIDTHS)
def test_stem_planes_are_those_of_pack_multi_on_its_own_output(hw, O):
    zeros_seen = 0
    for N in (1, 3):
        x, w, s, t, _, _ = stem_case(hw, O, N)
        for K in (1, 3):
            a, b = affines(K, O, gen.seed_of("stem-aff", O, K))
            y, sets = hipops.stem3x3_bn_relu_pack(x, w, s, t, dev(a), dev(b))
            none, blind = hipops.stem3x3_bn_relu_pack(x, w, s, t, dev(a), dev(b), out_f32=False)
            want = hipops.bn_act_pack_multi(y, dev(a), dev(b), relu=False)
            assert none is None and len(sets) == len(blind) == len(want) == K
            for k in range(K):
                assert torch.equal(sets[k].P, want[k].P) and torch.equal(sets[k].M, want[k].M), (N, K, k)
                assert torch.equal(blind[k].P, sets[k].P) and torch.equal(blind[k].M, sets[k].M), (N, K, k)
                assert sets[k].shape == want[k].shape == (N, O) + hw and not sets[k].nonneg
            # channel 1 of affine 0 has shift 0: where the ReLU cut, u = fma(0, a, 0) = 0 and both bits are clear
            cut = (y[:, 1] == 0)
            bit = lambda plane: (plane[:, 0] >> 1) & 1                     # noqa: E731
            assert int((bit(sets[0].P)[cut] | bit(sets[0].M)[cut]).sum()) == 0
            assert int((bit(sets[0].P)[~cut] | bit(sets[0].M)[~cut]).min() if (~cut).any() else 1) == 1
            zeros_seen += int(cut.sum())
    assert hw == (1, 1) or zeros_seen > 0, "no exact zero behind the ReLU: the ternary case was not exercised"


def test_stem_wrapper_cuts_a_batch_that_is_too_large_and_checks_shapes(monkeypatch):
    x, w, s, t, _, _ = stem_case((10, 9), 72, 3)
    a, b = (dev(v) for v in affines(2, 72, 5))
    y, sets = hipops.stem3x3_bn_relu_pack(x, w, s, t, a, b)
    before = native.launch_count()
    monkeypatch.setattr(hipops, "_STEM3X3_MAX_ELEMS", 2 * 72 * 90)          # two images per launch: 2 + 1
    y2, sets2 = hipops.stem3x3_bn_relu_pack(x, w, s, t, a, b)
    assert native.launch_count() - before == 2
    assert torch.equal(y, y2) and all(torch.equal(p.P, q.P) and torch.equal(p.M, q.M) for p, q in zip(sets, sets2))
    monkeypatch.undo()
    for bad in (lambda: hipops.stem3x3_bn_relu_pack(x[:, :2], w, s, t, a, b),
                lambda: hipops.stem3x3_bn_relu_pack(x, w[:, :, :, :2], s, t, a, b),
                lambda: hipops.stem3x3_bn_relu_pack(x, w, s[:5], t, a, b),
                lambda: hipops.stem3x3_bn_relu_pack(x, w, s, t, a[:, :5], b),
                lambda: hipops.stem3x3_bn_relu_pack(x, w, s, t, torch.cat([a, a, a]), torch.cat([b, b, b]))):
        with pytest.raises(native.NativeError):
            bad()


# ---- 3. cells with planes made outside -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", CELL_CASES, ids=[c.name for c in CELL_CASES])
def test_cell_takes_planes_made_outside(case):
    cell = build(case)
    s = [dev(a) for a in case.inputs()]
    eng = FusedCell(cell)
    with torch.no_grad():
        want = eng(*s)
        pres = [eng.preprocessor(i) for i in (0, 1)]
        planes = []
        for i, pre in enumerate(pres):
            if pre.kind != "ReLUConvBN":
                planes.append(None)
                continue
            # one bn_act_pack_multi for this consumer and another one (what the network does for a tensor with two)
            other = (-pre.bn_a, pre.bn_b + 0.25)
            planes.append(hipops.bn_act_pack_multi(s[i], torch.stack([other[0], pre.bn_a]),
                                                   torch.stack([other[1], pre.bn_b]), relu=False)[1])
        handed = sum(p is not None for p in planes)
        assert handed >= 1
        before = native.launch_count()
        eng(*s)
        alone = native.launch_count() - before
        before = native.launch_count()
        got = eng(*s, planes=tuple(planes))
        assert native.launch_count() - before == alone - handed
        assert torch.equal(got, want)
        # the fp32 input is not needed where the preprocessor adds no skip
        # (a ReLUConvBN with C_in == C_out adds its input: both preprocessors of allconv_none do)
        bare = [None if p is not None and not pre.add_skip else t for t, p, pre in zip(s, planes, pres)]
        assert any(t is None for t in bare) == (case.name != "allconv_none")
        assert torch.equal(eng(*bare, planes=tuple(planes)), want)
        for i, pre in enumerate(pres):
            if planes[i] is not None and pre.add_skip:
                with pytest.raises(FusionError):
                    eng(*[None if j == i else t for j, t in enumerate(s)], planes=tuple(planes))
        assert torch.equal(eng(*s), want) and torch.equal(eng(*s, planes=(None, None)), want)
        assert [k for k, _ in eng.steps].count("pack") == handed               # the stand-alone plan is unchanged
        with pytest.raises(FusionError):
            eng(None, s[1])                                                     # an input is missing, no planes for it
        for i, pre in enumerate(pres):
            wrong = list(planes)
            if pre.kind == "ReLUConvBN":
                wrong[i] = hipops.pack_act(s[i][:, :8].contiguous())            # another channel count
            else:
                wrong[i] = hipops.pack_act(s[i])                                # a FactorizedReduce packs for itself
            with pytest.raises(FusionError):
                eng(*s, planes=tuple(wrong))


# ---- 4. the network, bit for bit -----------------------------------------------------------------------------------
def launches(fn):
    before = native.launch_count()
    out = fn()
    return out, native.launch_count() - before


def check_bit_identity(net, x, stems):
    eng = FusedBATSNetwork(net)
    with torch.no_grad():
        want, aux = net(x)
        (got, none) = eng(x)                                       # (every weight is packed by now)
        assert aux is None and none is None
        assert torch.equal(got, want)
        (want2, _), n_net = launches(lambda: net(x))
        before = fastpath.stats()["cell"]
        (got2, _), n_eng = launches(lambda: eng(x))
        assert fastpath.stats()["cell"] == before + len(net.cells)
        assert torch.equal(got2, want) and torch.equal(want2, want)
        # the stems, the pooling and the classifier of this network are binary: they run as modules, which dispatch
        # their own launches — counted here by calling them alone
        feed, n_mod = x, 0
        for name in stems:
            feed, n = launches(lambda: getattr(net, name)(feed))
            n_mod += n
        assert [d["name"] for k, d in eng.steps if k == "module"] == list(stems) + ["global_pooling", "classifier"]
        pooled = torch.zeros(x.shape[0], net.classifier.in_features, device=DEV)
        n_mod += launches(lambda: net.classifier(pooled))[1]
    steps = eng.steps
    n_steps = sum(k in LAUNCHES for k, _ in steps)
    assert all(LAUNCHES[k] == 1 for k, _ in steps if k in LAUNCHES)           # (no two-launch head in this plan)
    merged = sum(d["sets"] - 1 for k, d in steps if k == "pack_handoff")
    print(f"{type(net).__name__}: net(x) {n_net} launches, executor {n_eng} = {n_steps} launch steps + {n_mod} in "
          f"modules, {merged} consumers merged")
    assert n_eng == n_steps + n_mod
    assert merged >= 1 and n_net - n_eng == merged
    return eng


def test_cifar_network_equals_the_per_cell_path_bit_for_bit():
    net = build(NET_CASE)
    eng = check_bit_identity(net, dev(NET_CASE.inputs()[0]), ("stem",))
    assert [d["sets"] for k, d in eng.steps if k == "pack_handoff"] == [3, 1, 1]
    assert "pack_s2" in [k for k, _ in eng.steps]


def test_imagenet_network_equals_the_per_cell_path_bit_for_bit():
    # N = 2 at 224 x 224: the smallest input whose final map is the 7 x 7 that AvgPool2d(7) needs
    net = binarise(models.BATSNetworkImageNet(*IMAGENET_ARGS, genotype(models, "MIXED"), GROUPS))
    net.drop_path_prob = 0.0
    net = load(net, gen.seed_of("batsnet-imagenet"))
    x = dev(gen.activation("normal", gen.seed_of("batsnet-imagenet-x"), (2, 3, 224, 224)))
    eng = check_bit_identity(net, x, ("stem0", "stem1"))
    assert [(d["of"], d["sets"]) for k, d in eng.steps if k == "pack_handoff"][0] == ("stem1", 2)


# ---- 5. against the reference --------------------------------------------------------------------------------------
def test_real_stem_network_against_the_reference(golden_dir):
    ref = np.load(os.path.join(golden_dir, "batsnet.npz"))[BATSNET_CASE.name + "/out"]
    net = build_real()
    eng = FusedBATSNetwork(net)
    steps = eng.steps
    assert steps[0][0] == "stem3x3" and steps[0][1]["sets"] == 3 and steps[0][1]["y"] is False
    assert steps[-1][0] == "avgpool_fc" and "module" not in [k for k, _ in steps]
    x = dev(BATSNET_CASE.inputs()[0])
    with torch.no_grad():
        (logits, aux), n = launches(lambda: eng(x))
        assert n > 0
        (logits, aux), n = launches(lambda: eng(x))
    assert aux is None and n == sum(LAUNCHES.get(k, 0) for k, _ in steps)      # (the head is two launches)
    err = float(np.abs(logits.cpu().numpy() - ref).max())
    print(f"{BATSNET_CASE.name}: max |logits - ref| = {err:.3g}, max |ref| = {np.abs(ref).max():.3g}")
    assert err <= 1e-3 * np.abs(ref).max()


# ---- 6. the cache --------------------------------------------------------------------------------------------------
def test_parameter_writes_reach_the_network_executor():
    net = build_real()
    eng = FusedBATSNetwork(net)
    x = dev(BATSNET_CASE.inputs()[0])
    saved = [net.cells[0].preprocess1.op[0].running_mean.clone(), net.stem[1].running_mean.clone()]
    with torch.no_grad():
        y0 = eng(x)[0]
        assert torch.equal(eng(x)[0], y0)
        # version-bumping writes need nothing
        net.cells[1]._ops[0].op[1].weight.mul_(-1)
        y1 = eng(x)[0]
        assert not torch.equal(y1, y0)
        net.stem[1].running_mean.add_(0.7)
        y2 = eng(x)[0]
        assert not torch.equal(y2, y1)
        # writes the version counters do not see: picked up after invalidate() or refresh()
        net.cells[1]._ops[0].op[1].weight.data.mul_(-1)
        assert torch.equal(eng(x)[0], y2), "a .data write is not seen before invalidate()"
        fastpath.invalidate(net)
        y3 = eng(x)[0]
        assert not torch.equal(y3, y2)
        net.cells[0].preprocess1.op[0].running_mean.data.add_(0.7)
        assert torch.equal(eng(x)[0], y3)
        eng.refresh()
        y4 = eng(x)[0]
        assert not torch.equal(y4, y3)
        net.cells[0].preprocess1.op[0].running_mean.copy_(saved[0])
        net.stem[1].running_mean.copy_(saved[1])
        assert torch.equal(eng(x)[0], y0)                          # every write undone (the weight was negated twice)
    torch.cuda.synchronize()


# ---- 7. the graph --------------------------------------------------------------------------------------------------
def test_graph_replay_equals_the_eager_executor():
    net = build_real()
    eager, eng = FusedBATSNetwork(net), FusedBATSNetwork(net)
    x = dev(BATSNET_CASE.inputs()[0])
    x2 = dev(gen.activation("normal", gen.seed_of("batsnet-graph-x2"), tuple(x.shape)))
    with pytest.raises(FusionError):
        eng.replay()
    assert eng.input is None
    with torch.no_grad():
        want, want2 = eager(x)[0], eager(x2)[0]
        assert not torch.equal(want, want2)
        assert eng.capture(x) is eng
        assert eng.input is not None and eng.input.data_ptr() != x.data_ptr() and torch.equal(eng.input, x)
        assert torch.equal(eng.replay(), want)
        eng.input.copy_(x2)
        assert torch.equal(eng.replay(), want2)
        net.cells[2]._ops[0].op[1].weight.data.mul_(-1)            # (a write only refresh() can see)
        eng.refresh()                                              # re-captures
        eager.refresh()
        want3 = eager(x2)[0]
        assert not torch.equal(want3, want2)
        assert torch.equal(eng.replay(), want3)
        assert torch.equal(eng(x)[0], eager(x)[0])                 # the eager entry of a captured executor still works
    torch.cuda.synchronize()

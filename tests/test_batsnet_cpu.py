"""A whole BATS network as one executor, without a GPU: the stem entry point is declared, bound and exported alike and
rejects bad arguments before any device call; FusedBATSNetwork plans CPU-resident networks (steps) and refuses what it
does not cover; bnn_amd.models reproduces the reference's fixture of the real-stem network (tests/golden/batsnet.npz)."""
import copy
import ctypes
import os
import pickle
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import bnn_amd as bnn
from bnn_amd import batsnet, fastpath, inference, models, native, ops
from bnn_amd.batsnet import FusedBATSNetwork
from bnn_amd.inference import FusionError
from tests.golden.batsnet_cases import BATSNET_CASE, binarise_real_ends, sign_inputs
from tests.golden.cells_cases import GROUPS, IMAGENET_ARGS, MARGIN_FACTOR, NET_CASE, genotype, sign_margin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "bnn_hip_stem3x3_bn_relu_pack_f32"


def binarise(model):
    cfg = bnn.BConfig(activation_pre_process=ops.BasicInputBinarizer, activation_post_process=bnn.Identity,
                      weight_pre_process=ops.XNORWeightBinarizer)
    return bnn.prepare_binary_model(model, cfg)


def load(model, case):
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(v) for k, v in case.state(shapes).items()})
    return model.eval()


def real_net(layers=3):
    net = models.BATSNetworkCIFAR(24, 10, layers, False, genotype(models, "MIXED"), GROUPS)
    net.drop_path_prob = 0.0
    return binarise_real_ends(bnn, ops, net).eval()


# ---- the entry point -----------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_the_stem_symbol():
    text = open(os.path.join(ROOT, "include", "bnn_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % SYMBOL, text)
    assert decl, f"{SYMBOL} is not declared in include/bnn_hip.h"
    params = [p.strip() for p in decl.group(1).split(",")]
    assert SYMBOL in native.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(native.lib_path()), SYMBOL), "build with __graft_entry__.build() first"
    fn = getattr(native.require(), SYMBOL)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(params) == 15
    for p, t in zip(params, fn.argtypes):          # pointers are bound as pointers, ints as ints, in the header's order
        assert (t is ctypes.c_void_p) == ("*" in p) and (t is ctypes.c_int) == (p.startswith("int ")), (p, t)
    assert native.require().bnn_hip_abi_version() == native.ABI_VERSION == 16      # an additive entry point
    assert inference.FusedBATSNetwork is FusedBATSNetwork
    assert batsnet.MAX_PACK_SETS == 4


def test_stem_entry_point_rejects_bad_arguments_without_a_gpu():
    fn = getattr(native.require(), SYMBOL)
    X, Wt, S, T, A, B, P, M, Y = (0x100000 * (i + 1) for i in range(9))
    good = dict(x=X, w=Wt, s=S, t=T, a=A, b=B, N=2, O=72, H=8, W=8, K=3, P=P, M=M, y=Y)

    def call(**kw):
        a = dict(good, **kw)
        return fn(a["x"], a["w"], a["s"], a["t"], a["a"], a["b"], a["N"], a["O"], a["H"], a["W"], a["K"], a["P"], a["M"],
                  a["y"], None)
    bad, big = native.ERR_INVALID_ARG, native.ERR_TOO_LARGE
    for name in ("x", "w", "s", "t", "a", "b", "P", "M"):          # y alone may be null
        assert call(**{name: None}) == bad, name
    for k in (0, 5, -1):
        assert call(K=k) == bad
    for name in ("O", "N", "H", "W"):
        assert call(**{name: 0}) == bad and call(**{name: -3}) == bad, name
    assert call(x=X + 2) == bad and call(P=P + 4) == bad and call(y=Y + 1) == bad          # misaligned
    assert call(N=1 << 15, O=1 << 16, H=1, W=1) == big             # N O H W = 2^31
    assert call(N=1 << 20, O=1, H=32, W=32) == big                 # the output fits, x [N, 3, H, W] does not
    assert call(N=1 << 24, O=1 << 24, H=1 << 24, W=1 << 24) == big  # (products that would wrap 64 bits)
    assert call(O=64 * 65536, N=1, H=1, W=1) == native.ERR_UNSUPPORTED      # more channel groups than grid.y holds


# ---- the plan ------------------------------------------------------------------------------------------------------
def consumers_of(net):
    """Per tensor between the parts of a CIFAR network (the stem, then each cell's output): how many ReLUConvBN and how
    many FactorizedReduce preprocessors read it."""
    L = len(net.cells)
    reads = [0, 0] + [1 + k for k in range(L)]
    out = {j: [0, 0] for j in range(1 + L)}
    for k, cell in enumerate(net.cells):
        for i, name in enumerate(("preprocess0", "preprocess1")):
            out[reads[k + i]][type(getattr(cell, name)).__name__ == "FactorizedReduce"] += 1
    return out


def test_plan_of_the_binarised_network_packs_every_tensor_once():
    net = load(binarise(NET_CASE.build(models)), NET_CASE)
    eng = FusedBATSNetwork(net)                                    # recognised (the launch data waits for a HIP device)
    steps = eng.steps
    assert steps[0] == ("module", {"name": "stem"})                # binarise() makes the stem binary: the module runs
    assert "stem3x3" not in [k for k, _ in steps]
    want = consumers_of(net)
    names = ["stem"] + list(range(len(net.cells)))
    packs = {d["of"]: d for k, d in steps if k == "pack_handoff"}
    assert len(packs) == len([d for k, d in steps if k == "pack_handoff"])      # one launch per tensor
    for j, (n_rcb, n_red) in want.items():
        if n_rcb:
            assert packs[names[j]]["sets"] == n_rcb == len(packs[names[j]]["consumers"])
        else:
            assert names[j] not in packs
    assert packs["stem"]["consumers"] == [(0, 0), (0, 1), (1, 0)] and packs[0]["consumers"] == [(1, 1)]
    # cells[2].preprocess0 is a FactorizedReduce on cell 0's output: it packs for itself
    assert want[1] == [1, 1]
    assert ("pack_s2", {"op": "preprocess0", "cell": 2}) in steps
    # no cell packs a ReLUConvBN input itself any more
    assert not [d for k, d in steps if k == "pack"]
    # a binary classifier: pooling and classifier run as modules
    assert steps[-2:] == [("module", {"name": "global_pooling"}), ("module", {"name": "classifier"})]
    # the order: a tensor is packed after its producer and before its first consumer
    kinds = [(k, d.get("of"), d.get("cell")) for k, d in steps]
    assert kinds.index(("pack_handoff", "stem", None)) < min(i for i, s in enumerate(kinds) if s[2] == 0)
    assert max(i for i, s in enumerate(kinds) if s[2] == 0) < kinds.index(("pack_handoff", 0, None)) \
        < min(i for i, s in enumerate(kinds) if s[2] == 1)
    with pytest.raises(FusionError):
        eng(torch.from_numpy(NET_CASE.inputs()[0]))                # a CPU tensor


def test_plan_with_a_real_stem_starts_with_the_stem_kernel():
    eng = FusedBATSNetwork(real_net())
    kind, detail = eng.steps[0]
    assert kind == "stem3x3" and detail["sets"] == 3 and detail["y"] is False
    assert detail["consumers"] == [(0, 0), (0, 1), (1, 0)]
    assert not [d for k, d in eng.steps if k == "pack_handoff" and d["of"] == "stem"]
    assert eng.steps[-1] == ("avgpool_fc", {"window": "global"})   # AdaptiveAvgPool2d(1) + a real Linear
    one = FusedBATSNetwork(real_net(layers=1))
    assert one.steps[0][0] == "stem3x3" and one.steps[0][1]["sets"] == 2 and one.steps[0][1]["y"] is False
    assert not [d for k, d in one.steps if k == "pack_handoff"]    # the only cell's output feeds the head


def test_imagenet_network_plans_module_stems_and_the_7x7_head():
    net = binarise(models.BATSNetworkImageNet(*IMAGENET_ARGS, genotype(models, "MIXED"), GROUPS))
    net.drop_path_prob = 0.0
    steps = FusedBATSNetwork(net.eval()).steps
    assert steps[:2] == [("module", {"name": "stem0"}), ("module", {"name": "stem1"})]
    packs = [d for k, d in steps if k == "pack_handoff"]
    assert packs[0] == {"of": "stem1", "sets": 2, "consumers": [(0, 1), (1, 0)]}
    assert not [d for d in packs if d["of"] == "stem0"]            # cells[0].preprocess0 is a FactorizedReduce
    assert ("pack_s2", {"op": "preprocess0", "cell": 0}) in steps
    real = models.BATSNetworkImageNet(*IMAGENET_ARGS, genotype(models, "MIXED"), GROUPS)
    cfg = bnn.BConfig(activation_pre_process=ops.BasicInputBinarizer, activation_post_process=bnn.Identity,
                      weight_pre_process=ops.XNORWeightBinarizer)
    real = bnn.prepare_binary_model(real, cfg, custom_config_layers_name={"classifier": bnn.BConfig()}).eval()
    assert FusedBATSNetwork(real).steps[-1] == ("avgpool_fc", {"window": 7})


def test_what_the_network_executor_refuses():
    with pytest.raises(FusionError):
        FusedBATSNetwork(real_net().train())
    with pytest.raises(FusionError):
        FusedBATSNetwork(nn.Sequential(nn.Conv2d(3, 8, 3)).eval())             # not a BATS network
    with pytest.raises(FusionError):
        FusedBATSNetwork(real_net().cells[0])                                   # a Cell is not a network
    shake = real_net()
    shake.cells[1].use_shake_shake = True
    with pytest.raises(FusionError):
        FusedBATSNetwork(shake)
    biased = real_net()
    biased.stem[0].bias = nn.Parameter(torch.zeros(72))
    with pytest.raises(FusionError):
        FusedBATSNetwork(biased)
    float_net = NET_CASE.build(models).eval()                                   # not binarised: the cells are refused
    with pytest.raises(FusionError):
        FusedBATSNetwork(float_net)


def test_invalidate_reaches_the_executor_and_copies_start_without_it():
    net = real_net()
    eng = FusedBATSNetwork(net)
    assert eng._unchanged()
    fastpath.invalidate(net)
    assert not eng._unchanged()                                    # the next call re-derives
    eng.refresh()
    assert eng._unchanged()
    fastpath.invalidate(net.cells[0])                              # a part of the network: not the network's executor
    assert eng._unchanged()
    net.stem[1].running_mean.add_(0.5)                             # a version-bumping write is seen by itself
    assert not eng._unchanged()
    assert not copy.deepcopy(net).__dict__[fastpath.WATCH_KEY].refs
    assert not pickle.loads(pickle.dumps(net)).__dict__[fastpath.WATCH_KEY].refs


# ---- the fixture ---------------------------------------------------------------------------------------------------
def test_module_reproduces_the_real_stem_fixture(golden_dir):
    golden = np.load(os.path.join(golden_dir, "batsnet.npz"))
    case = BATSNET_CASE
    model = load(binarise_real_ends(bnn, ops, case.build(models)), case)
    assert list(model.state_dict().keys()) == [str(k) for k in golden[case.name + "/keys"]]
    assert int(golden[case.name + "/salt"]) == case.salt
    with torch.no_grad():
        y, seen = sign_inputs(model, case, tuple(torch.from_numpy(a) for a in case.inputs()))
    ref = golden[case.name + "/out"]
    margin, e_ref = sign_margin(seen), float(golden[case.name + "/e_ref"])
    print(f"{case.name}: max |y - ref| = {np.abs(y.numpy() - ref).max():.3g}, max |ref| = {np.abs(ref).max():.3g}, "
          f"sign margin {margin:.3g} (fixture {float(golden[case.name + '/margin']):.3g}), e_ref {e_ref:.3g}")
    assert np.abs(y.numpy() - ref).max() <= 1e-3 * np.abs(ref).max()
    assert margin >= MARGIN_FACTOR * e_ref

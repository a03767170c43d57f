"""The fused ImageNet stems of a BATS network, without a GPU: the two entry points are declared, bound and exported alike
and reject bad arguments before any device call; FusedBATSNetwork plans the real-stem network as two stem launches and
everything else as modules; bnn_amd.models' stems reproduce the reference's fixture
(tests/golden/batsnet_imagenet_stem.npz)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import bnn_amd as bnn
from bnn_amd import batsnet, hipops, models, native, ops
from bnn_amd.batsnet import FusedBATSNetwork
from bnn_amd.executor import fold_bn
from tests.batsnet_imagenet_ref import gconv3x3s2_f64, stem_s2x2_f64
from tests.golden import batsnet_imagenet_cases as case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEM0, STEM1 = "bnn_hip_stem_s2x2_f32", "bnn_hip_gconv3x3s2_bn_pack_f32"
BAD, BIG, UNSUPPORTED = native.ERR_INVALID_ARG, native.ERR_TOO_LARGE, native.ERR_UNSUPPORTED


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bnn_hip.h")).read(), flags=re.S)


# ---- the entry points ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("symbol,count", [(STEM0, 16), (STEM1, 18)])
def test_header_binding_and_library_agree_on_the_symbols(symbol, count):
    decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % symbol, header())
    assert decl, f"{symbol} is not declared in include/bnn_hip.h"
    params = [p.strip() for p in decl.group(1).split(",")]
    assert symbol in native.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(native.lib_path()), symbol), "build with __graft_entry__.build() first"
    fn = getattr(native.require(), symbol)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(params) == count
    for p, t in zip(params, fn.argtypes):          # pointers are bound as pointers, ints as ints, in the header's order
        assert (t is ctypes.c_void_p) == ("*" in p) and (t is ctypes.c_int) == (p.startswith("int ")), (p, t)
    assert native.require().bnn_hip_abi_version() == native.ABI_VERSION == 16      # additive entry points


def test_python_constants_are_the_headers():
    macros = dict(re.findall(r"#define\s+(BNN_HIP_\w+)\s+(\d+)", header()))
    assert hipops.STEM_S2_TILE == native.STEM_S2_TILE == (int(macros["BNN_HIP_STEM_S2_TILE_H"]),
                                                          int(macros["BNN_HIP_STEM_S2_TILE_W"]))
    assert native.STEM_S2X2_MAX_GROUP_CHANNELS == int(macros["BNN_HIP_STEM_S2X2_MAX_GROUP_CHANNELS"])
    assert native.GCONV3X3S2_MAX_GROUP_CHANNELS == int(macros["BNN_HIP_GCONV3X3S2_MAX_GROUP_CHANNELS"])
    assert batsnet.LAUNCHES["stem_s2x2"] == batsnet.LAUNCHES["stem_s2_pack"] == 1
    assert batsnet.FUSE_IMAGENET_STEMS in (True, False)


PTRS = {n: 0x100000 * (i + 1) for i, n in enumerate(("x", "w1", "s1", "t1", "w2", "s2", "t2", "y", "a", "b", "P", "M"))}


def call0(**kw):
    a = dict(PTRS, N=2, C1=30, C=60, G=3, H=20, W=18, relu=1)
    a.update(kw)
    return getattr(native.require(), STEM0)(a["x"], a["w1"], a["s1"], a["t1"], a["w2"], a["s2"], a["t2"], a["N"], a["C1"],
                                            a["C"], a["G"], a["H"], a["W"], a["relu"], a["y"], None)


def call1(**kw):
    a = dict(PTRS, N=2, Cin=60, O=60, G=3, H=5, W=5, relu=1, K=2)
    a.update(kw)
    return getattr(native.require(), STEM1)(a["x"], a["w1"], a["s1"], a["t1"], a["a"], a["b"], a["N"], a["Cin"], a["O"],
                                            a["G"], a["H"], a["W"], a["relu"], a["K"], a["P"], a["M"], a["y"], None)


def test_stem0_entry_point_rejects_bad_arguments_without_a_gpu():
    for name in ("x", "w1", "s1", "t1", "w2", "s2", "t2", "y"):
        assert call0(**{name: None}) == BAD, name                                      # null pointer
        assert call0(**{name: PTRS[name] + 2}) == BAD, name                            # misaligned pointer
    for name in ("N", "C1", "C", "G", "H", "W"):
        assert call0(**{name: 0}) == BAD and call0(**{name: -3}) == BAD, name          # size <= 0
    assert call0(G=4) == BAD and call0(C1=30, C=50, G=3) == BAD and call0(C1=31, C=60, G=3) == BAD   # G not dividing
    assert call0(N=1 << 20, H=32, W=32) == BIG                                         # x [N, 3, H, W] reaches 2^31
    assert call0(N=1 << 16, C1=8, C=1 << 15, G=1, H=1, W=1) == BIG                     # y [N, C, 1, 1] = 2^31
    assert call0(N=1 << 24, C1=1 << 24, C=1 << 24, G=1, H=1 << 24, W=1 << 24) == BIG   # products that would wrap 64 bits
    limit = native.STEM_S2X2_MAX_GROUP_CHANNELS
    assert call0(C1=limit + 1, C=2 * (limit + 1), G=1) == UNSUPPORTED                  # a group's channels exceed the LDS tile
    assert call0(C1=3 * (limit + 1), C=6 * (limit + 1), G=3) == UNSUPPORTED
    assert call0(C1=1 << 16, C=1 << 16, G=1 << 16, N=1, H=1, W=1) == UNSUPPORTED       # more groups than grid.y holds


def test_stem1_entry_point_rejects_bad_arguments_without_a_gpu():
    for name in ("x", "w1", "s1", "t1", "a", "b", "P", "M"):                           # y alone may be null (K >= 1)
        assert call1(**{name: None}) == BAD, name
    for name, off in (("x", 2), ("w1", 2), ("s1", 1), ("t1", 2), ("a", 2), ("b", 2), ("P", 4), ("M", 4), ("y", 2)):
        assert call1(**{name: PTRS[name] + off}) == BAD, name                          # misaligned pointer
    for name in ("N", "Cin", "O", "G", "H", "W"):
        assert call1(**{name: 0}) == BAD and call1(**{name: -3}) == BAD, name
    for k in (-1, 5, 9):
        assert call1(K=k) == BAD                                                       # K outside 0..4
    assert call1(K=0, y=None) == BAD                                                   # K = 0 with a NULL y
    assert call1(K=0, a=None, b=None, P=None, M=None, N=0) == BAD                      # (K = 0 needs no planes: N is what is wrong)
    assert call1(G=7) == BAD and call1(Cin=60, O=50, G=3) == BAD and call1(Cin=50, O=60, G=3) == BAD
    assert call1(N=1 << 16, Cin=1 << 15, O=8, G=1, H=1, W=1) == BIG                    # x reaches 2^31
    assert call1(N=1 << 16, Cin=8, O=1 << 15, G=1, H=1, W=1) == BIG                    # y reaches 2^31
    assert call1(N=1 << 24, Cin=1 << 24, O=1 << 24, G=1 << 24, H=1 << 24, W=1 << 24) == BIG
    limit = native.GCONV3X3S2_MAX_GROUP_CHANNELS
    assert call1(Cin=limit + 1, O=limit + 1, G=1) == UNSUPPORTED                       # a group's channels exceed the LDS tile
    assert call1(Cin=8, O=64 * 65536, G=1, N=1, H=1, W=1) == UNSUPPORTED               # more plane words than grid.y holds


# ---- the plan ------------------------------------------------------------------------------------------------------
def real_net(prepare=True):
    net = case.build(models)
    return case.binarise_real_stems(bnn, ops, net).eval() if prepare else net


def kinds(eng):
    return [k for k, _ in eng.steps]


def test_real_stem_imagenet_network_plans_two_stem_launches(monkeypatch):
    monkeypatch.setattr(batsnet, "FUSE_IMAGENET_STEMS", True)
    steps = FusedBATSNetwork(real_net()).steps
    assert [k for k, _ in steps[:2]] == ["stem_s2x2", "stem_s2_pack"]
    assert steps[0][1] == {"relu_out": True}                       # stem1's ReLU is in place: the cells see relu(s0)
    detail = steps[1][1]
    assert detail["consumers"] == [(0, 1), (1, 0)] and detail["sets"] == 2 and detail["y"] is True
    assert not [d for k, d in steps if k == "pack_handoff" and d["of"] in ("stem0", "stem1")]
    assert ("pack_s2", {"op": "preprocess0", "cell": 0}) in steps  # the FactorizedReduce on s0 packs for itself
    assert steps[-1] == ("avgpool_fc", {"window": 7})
    assert "module" not in [k for k, _ in steps]
    out_of_place = real_net()
    out_of_place.stem1[0] = nn.ReLU(inplace=False)
    assert FusedBATSNetwork(out_of_place).steps[0] == ("stem_s2x2", {"relu_out": False})


def module_stems(net):
    steps = FusedBATSNetwork(net).steps
    assert steps[:2] == [("module", {"name": "stem0"}), ("module", {"name": "stem1"})], steps[:2]
    assert [(d["of"], d["consumers"]) for k, d in steps if k == "pack_handoff"][0] == ("stem1", [(0, 1), (1, 0)])
    assert "stem_s2x2" not in [k for k, _ in steps] and "stem_s2_pack" not in [k for k, _ in steps]


def test_everything_else_keeps_the_module_stems_without_raising(monkeypatch):
    monkeypatch.setattr(batsnet, "FUSE_IMAGENET_STEMS", False)
    module_stems(real_net())                                       # the switch
    monkeypatch.setattr(batsnet, "FUSE_IMAGENET_STEMS", True)
    cfg = bnn.BConfig(activation_pre_process=ops.BasicInputBinarizer, activation_post_process=bnn.Identity,
                      weight_pre_process=ops.XNORWeightBinarizer)
    for binary in ("stem0.0", "stem0.3", "stem1.1"):               # one stem convolution left binary
        real = {n: bnn.BConfig() for n in case.REAL_LAYERS if n != binary}
        module_stems(bnn.prepare_binary_model(case.build(models), cfg, custom_config_layers_name=real).eval())
    biased = real_net()
    biased.stem0[3].bias = nn.Parameter(torch.zeros(biased.stem0[3].out_channels))
    module_stems(biased)                                           # a bias
    strided = real_net()
    strided.stem1[1].stride = (1, 1)
    module_stems(strided)                                          # stride 1 on one convolution
    wide = real_net()
    wide.stem0[3].groups = 1                                       # (recognition only: 30 channels per group fit, 41 do not)
    wide.stem1[1].groups = 1
    module_stems(wide)
    eng = FusedBATSNetwork(real_net())
    monkeypatch.setattr(batsnet, "FUSE_IMAGENET_STEMS", False)
    assert kinds(eng)[0] == "stem_s2x2"                            # read at refresh(), not before
    eng.refresh()
    assert kinds(eng)[:2] == ["module", "module"]


# ---- the fixture ---------------------------------------------------------------------------------------------------
def test_module_stems_reproduce_the_reference_fixture(golden_dir):
    golden = np.load(os.path.join(golden_dir, "batsnet_imagenet_stem.npz"))
    model = real_net()
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(v) for k, v in case.state(shapes).items()})
    model.eval()
    assert list(shapes) == [str(k) for k in golden[case.NAME + "/keys"]]
    x = torch.from_numpy(case.inputs())
    with torch.no_grad():
        raw, s0, s1 = case.run_stems(model, x)
    assert bool((raw < 0).any()) and torch.equal(s0, torch.relu(raw))     # raw before stem1 ran, rectified afterwards
    ref0, ref1 = (torch.from_numpy(golden[case.NAME + "/" + k]) for k in ("s0", "s1"))
    assert ref0.shape == s0.shape == (2, 60, 5, 5) and ref1.shape == s1.shape == (2, 60, 3, 3)
    conv0, bn0, _, conv1, bn1 = model.stem0
    _, conv2, bn2 = model.stem1
    (a1, b1), (a2, b2), (a3, b3) = fold_bn(bn0), fold_bn(bn1), fold_bn(bn2)
    y64, bound = stem_s2x2_f64(x, conv0.weight.detach(), a1, b1, conv1.weight.detach(), a2, b2, conv1.groups, True)
    for name, got in (("bnn_amd.models", s0), ("reference", ref0)):
        err = (got.double() - y64).abs()
        print(f"s0 {name}: max err / bound = {float((err / bound).max()):.3g}")
        assert bool((err <= bound).all()), name
    for name, got, src in (("bnn_amd.models", s1, s0), ("reference", ref1, ref0)):
        y64, bound = gconv3x3s2_f64(src, conv2.weight.detach(), a3, b3, conv2.groups, True)
        err = (got.double() - y64).abs()
        print(f"s1 {name}: max err / bound = {float((err / bound).max()):.3g}")
        assert bool((err <= bound).all()), name

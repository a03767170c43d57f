"""Whole BATS cells and networks without a GPU: bnn_amd.models.{Cell, BATSNetworkCIFAR, BATSNetworkImageNet, ...} against
the reference's fixtures (tests/golden/cells.npz), the sign margin the fixtures were chosen for, the cell dispatch
declining, the argument checks of the three cell entry points and what FusedCell refuses."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import bnn_amd as bnn
from bnn_amd import fastpath, inference, models, native
from bnn_amd.cellops import FusedCell
from bnn_amd.inference import FusionError, auto_cell_forward, no_cell_fusion
from bnn_amd.ops import BasicInputBinarizer, XNORWeightBinarizer
from tests.golden.cells_cases import (ALL_CASES, CELL_CASES, GROUPS, IMAGENET_ARGS, MARGIN_FACTOR, binary_inputs,
                                      genotype, sign_margin)

IDS = [c.name for c in ALL_CASES]


def close(a, ref):
    """The project's layer bar."""
    return np.allclose(a, ref, rtol=1e-3, atol=1e-5 * np.abs(ref).max())


def binarise(model):
    cfg = bnn.BConfig(activation_pre_process=BasicInputBinarizer, activation_post_process=bnn.Identity,
                      weight_pre_process=XNORWeightBinarizer)
    return bnn.prepare_binary_model(model, cfg)


def build(case):
    model = binarise(case.build(models))
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(v) for k, v in case.state(shapes).items()})
    return model.eval()


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "cells.npz"))


def test_the_new_names_are_exported():
    for name in ("Genotype", "PRIMITIVES", "OPS", "Zero", "FactorizedReduce", "drop_path", "Cell", "AuxiliaryHead",
                 "BATSNetworkCIFAR", "BATSNetworkImageNet"):
        assert hasattr(models, name) and name in models.__all__, name
    assert set(models.OPS) == set(models.PRIMITIVES)          # no 'sep_conv_7x7', no 'conv_7x1_1x7'
    assert "cell" in fastpath.stats()
    assert inference.FusedCell is FusedCell
    for name in ("CellFusion", "auto_cell_forward", "no_cell_fusion"):
        assert hasattr(inference, name)
    for sym in ("bnn_hip_bn_act_pack_multi_f32", "bnn_hip_bn_act_pack_s2_f32", "bnn_hip_bconv2d_grouped_node"):
        assert sym in native.EXPORTED_SYMBOLS


@pytest.mark.parametrize("case", ALL_CASES, ids=IDS)
def test_module_reproduces_the_reference_fixture(golden, case):
    model = build(case)
    assert list(model.state_dict().keys()) == [str(k) for k in golden[case.name + "/keys"]]
    assert int(golden[case.name + "/salt"]) == case.salt
    x = tuple(torch.from_numpy(a) for a in case.inputs())
    with torch.no_grad():
        y, seen = binary_inputs(model, case, x)
    ref = golden[case.name + "/out"]
    y = y.numpy()
    margin, e_ref = sign_margin(seen), float(golden[case.name + "/e_ref"])
    print(f"{case.name}: max |y - ref| = {np.abs(y - ref).max():.3g}, max |ref| = {np.abs(ref).max():.3g}, "
          f"sign margin {margin:.3g} (fixture {float(golden[case.name + '/margin']):.3g}), e_ref {e_ref:.3g}")
    assert y.shape == ref.shape
    assert close(y, ref)
    assert margin >= MARGIN_FACTOR * e_ref


def test_imagenet_network_has_the_reference_keys(golden):
    net = binarise(models.BATSNetworkImageNet(*IMAGENET_ARGS, genotype(models, "MIXED"), GROUPS))
    assert list(net.state_dict().keys()) == [str(k) for k in golden["imagenet/keys"]]


@pytest.mark.parametrize("case", CELL_CASES[:2], ids=IDS[:2])
def test_training_mode_with_drop_path_runs(case):
    cell = build(case).train()
    s0, s1 = (torch.from_numpy(a) for a in case.inputs())
    with torch.no_grad():
        want = cell(s0, s1, 0.0).shape
    torch.manual_seed(0)
    y = cell(s0, s1, 0.3)
    assert y.shape == want and torch.isfinite(y).all()
    y.sum().backward()
    assert all(p.grad is not None for p in cell.parameters())


def test_drop_path_masks_whole_samples_and_rescales():
    torch.manual_seed(1)
    x = torch.ones(64, 3, 2, 2)
    y = models.drop_path(x.clone(), 0.25)
    per_sample = y.reshape(64, -1)
    assert ((per_sample == 0).all(1) | (per_sample == 1 / 0.75).all(1)).all()
    assert 0 < int((per_sample == 0).all(1).sum()) < 64
    assert torch.equal(models.drop_path(x.clone(), 0.0), x)


def test_zero_and_factorized_reduce_shapes():
    assert models.Zero(2)(torch.ones(2, 4, 7, 9)).shape == (2, 4, 3, 4)
    assert float(models.Zero(1)(torch.ones(1, 2, 3, 3)).abs().sum()) == 0
    fr = models.FactorizedReduce(8, 12)
    assert list(fr.state_dict())[0] == "activation.weight"
    assert fr(torch.randn(2, 8, 6, 10)).shape == (2, 12, 3, 5)


def test_dispatch_hook_declines_on_the_cpu_and_under_the_switches():
    case = CELL_CASES[0]
    cell = build(case)
    s0, s1 = (torch.from_numpy(a) for a in case.inputs())
    with torch.no_grad():
        assert auto_cell_forward(cell, s0, s1) is None          # CPU tensors
        with no_cell_fusion():
            assert auto_cell_forward(cell, s0, s1) is None
    st = cell.__dict__["_bnn_auto_cell"]
    assert st.calls == {"fused": 0, "declined": 2}
    cell.train()
    assert "_bnn_auto_cell" not in cell.__dict__                 # the mode switch drops the executor state
    cell.eval()
    with torch.no_grad():
        auto_cell_forward(cell, s0, s1)
    assert fastpath.invalidate(cell) >= 0 and "_bnn_auto_cell" not in cell.__dict__
    import copy
    import pickle
    with torch.no_grad():
        auto_cell_forward(cell, s0, s1)
    assert copy.deepcopy(cell).__dict__["_bnn_auto_cell"].engine is None
    assert pickle.loads(pickle.dumps(cell)).__dict__["_bnn_auto_cell"].engine is None


def test_fused_cell_plans_and_refuses():
    case = CELL_CASES[3]                                         # allconv_none
    good = build(case)
    eng = FusedCell(good)                                        # recognised (the launch data waits for a HIP device)
    kinds = [k for k, _ in eng.steps]
    assert "torch_add" not in kinds and "copy" not in kinds
    assert kinds.count("grouped_node") == 7 and kinds.count("dense") == 2 and kinds.count("pack") == 2
    multi = [d for k, d in eng.steps if k == "pack_multi"]
    assert [(d["state"], d["sets"]) for d in multi] == [(0, 2), (1, 4), (2, 1)]
    reduce_kinds = [k for k, _ in FusedCell(build(CELL_CASES[1])).steps]
    assert "pack_s2" in reduce_kinds
    with pytest.raises(FusionError):
        eng(*(torch.from_numpy(a) for a in case.inputs()))      # CPU tensors
    with pytest.raises(FusionError):
        FusedCell(build(case).train())
    with pytest.raises(FusionError):
        FusedCell(case.build(models).eval())                     # not binarised
    shake = binarise(models.Cell(genotype(models, "MIXED"), 48, 48, 48, False, False, use_shake_shake=True)).eval()
    with pytest.raises(FusionError):
        FusedCell(shake)
    odd = build(case)
    odd._ops[0] = nn.ReLU()                                      # an operation that is none of the primitives
    with pytest.raises(FusionError):
        FusedCell(odd)
    with pytest.raises(FusionError):
        FusedCell(build(case)._ops[0])                           # not a Cell


def test_entry_points_reject_bad_arguments_without_a_gpu():
    lib = native.require()
    V = native.F32View
    P, M, A, B = 0x10000, 0x20000, 0x30000, 0x40000
    multi, s2, node = lib.bnn_hip_bn_act_pack_multi_f32, lib.bnn_hip_bn_act_pack_s2_f32, lib.bnn_hip_bconv2d_grouped_node
    x = V(0x100000, 8, 72)
    bad = native.ERR_INVALID_ARG
    assert multi(None, 2, 48, 8, 8, 2, A, B, 0, P, M, None) == bad
    for k in (0, 5, -1):
        assert multi(ctypes.byref(x), 2, 48, 8, 8, k, A, B, 0, P, M, None) == bad
    assert multi(ctypes.byref(x), 2, 48, 8, 8, 2, None, B, 0, P, M, None) == bad
    assert multi(ctypes.byref(V(0x100000, 30, 72)), 2, 48, 8, 8, 2, A, B, 0, P, M, None) == bad    # 30 + 48 > 72
    assert multi(ctypes.byref(V(0x100000, 8, 0)), 2, 48, 8, 8, 2, A, B, 0, P, M, None) == bad      # offset without total
    assert multi(ctypes.byref(V(0x100002, 0, 0)), 2, 48, 8, 8, 2, A, B, 0, P, M, None) == bad      # misaligned
    assert multi(ctypes.byref(V(None, 0, 0)), 2, 48, 8, 8, 2, A, B, 0, P, M, None) == bad
    assert s2(ctypes.byref(x), 2, 48, 7, 8, A, B, 0, P, M, None) == bad                             # odd H
    assert s2(ctypes.byref(x), 2, 48, 8, 9, A, B, 0, P, M, None) == bad                             # odd W
    assert s2(ctypes.byref(x), 2, 48, 8, 8, A, None, 0, P, M, None) == bad
    assert s2(None, 2, 48, 8, 8, A, B, 0, P, M, None) == bad

    d = native.ConvDesc(2, 48, 8, 8, 48, 3, 3, 1, 1, 1, 1, 1, 1, 0)
    out = 0x800000

    def call(res=None, add=None, o=out, off=8, tot=88, sg=4, alpha=0x50000):
        return node(ctypes.byref(d), 12, P, M, A, B, alpha, None, None, 0x60000, sg,
                    None if res is None else ctypes.byref(res), None if add is None else ctypes.byref(add), o, off, tot,
                    None)
    assert call(alpha=None) == bad and call(sg=5) == bad and call(o=None) == bad
    assert call(off=41) == bad                                   # 41 + 48 > 88
    assert call(off=8, tot=0) == bad
    assert call(res=V(out, 30, 88)) == bad                       # channels 30..78 of the output tensor overlap 8..56
    assert call(add=V(out, 56 - 47, 88)) == bad
    assert call(res=V(out + 4 * 64, 0, 48)) == bad               # another base inside the output tensor
    assert call(res=V(out, 56, 104)) == bad                      # same base, another c_total


"""A whole BATS cell as fused HIP launches: the three cell entry points bit for bit (bn_act_pack_multi and bn_act_pack_s2
against bn_act_pack on contiguous copies, bconv2d_grouped_node against its NumPy float32 restatement on the CPU oracle's
dot, through channel-slice views), bnn_amd.models.Cell dispatching to cellops.FusedCell under eval() / no_grad()
against the reference's fixtures (tests/golden/cells.npz), the plan it runs, and the executor's cache."""
import os

import numpy as np
import pytest
import torch

import bnn_amd as bnn
import oracle
from bnn_amd import fastpath, hipops, models, native
from bnn_amd.cellops import FusedCell
from bnn_amd.inference import no_cell_fusion, per_layer_forward
from bnn_amd.native import NativeError
from bnn_amd.ops import BasicInputBinarizer, XNORWeightBinarizer
from tests.golden import gen
from tests.golden.cells_cases import CELL_CASES, NET_CASE
from tests.golden.grouped_cases import GROUPED_CASES
from tests.grouped_util import as_2d, oracle_dot

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -12345.5


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


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
    return model.to(DEV).eval()


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "cells.npz"))


def sliced(value, c_off, c_total, fill=SENTINEL):
    """``value`` [N, C, H, W] (NumPy) as channels [c_off, c_off + C) of a sentinel-filled [N, c_total, H, W] device
    tensor: (the whole tensor, the slice view)."""
    N, C, H, W = value.shape
    whole = torch.full((N, c_total, H, W), fill, dtype=torch.float32, device=DEV)
    view = whole[:, c_off:c_off + C]
    view.copy_(dev(value))
    return whole, view


def affines(K, C, seed):
    """K BatchNorm-like affines whose zero crossings fall inside the data."""
    a = (0.5 + gen.uniform(seed, (K, C))).astype(np.float32) * np.where(gen.uniform(seed + 1, (K, C)) < 0.2, -1, 1)
    b = (0.4 * gen.normal(seed + 2, (K, C))).astype(np.float32)
    return a.astype(np.float32), b


# ---- 1. one read, K plane sets -------------------------------------------------------------------------------------
# 8x8: 16-byte path; 10x9 with the view starting at an odd multiple of 8 bytes: the 8-byte path; 7x9: scalar
@pytest.mark.parametrize("hw", [(8, 8), (10, 9), (7, 9)], ids=lambda v: f"{v[0]}x{v[1]}")
@pytest.mark.parametrize("C,c_off,c_total", [(48, 8, 72), (96, 1, 100)])
def test_pack_multi_equals_separate_packs(hw, C, c_off, c_total):
    H, W = hw
    x = gen.activation("normal", gen.seed_of("pack-multi", C, H, W), (2, C, H, W))
    whole, view = sliced(x, c_off, c_total)
    if (H, W) == (10, 9):       # view start = c_off * 90 floats: 8-byte aligned, and for odd c_off not 16-byte aligned
        assert view.data_ptr() % 8 == 0 and (c_off % 2 == 0 or view.data_ptr() % 16 == 8)
    assert not view.is_contiguous()
    copy = view.contiguous()
    for K in (1, 2, 4):
        a, b = affines(K, C, gen.seed_of("pack-multi-aff", C, K))
        for relu in (False, True):
            got = hipops.bn_act_pack_multi(view, dev(a), dev(b), relu=relu)
            assert len(got) == K
            for k in range(K):
                want = hipops.bn_act_pack(copy, dev(a[k]), dev(b[k]), relu=relu)
                assert torch.equal(got[k].P, want.P) and torch.equal(got[k].M, want.M), (K, k, relu)
                assert got[k].shape == want.shape and got[k].nonneg == want.nonneg
    assert float(whole[:, :c_off].min()) == SENTINEL == float(whole[:, c_off + C:].max())    # the read left x alone
    with pytest.raises(NativeError):
        hipops.bn_act_pack_multi(view, dev(np.ones((5, C), np.float32)), dev(np.zeros((5, C), np.float32)))
    with pytest.raises(NativeError):
        hipops.bn_act_pack_multi(whole[:, :, ::2], dev(a), dev(b))          # not a channel slice


# ---- 2. the two phases FactorizedReduce reads ----------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(8, 8), (6, 10), (2, 2)], ids=lambda v: f"{v[0]}x{v[1]}")
@pytest.mark.parametrize("C", [48, 72])
@pytest.mark.parametrize("as_view", [False, True], ids=["contiguous", "slice"])
def test_pack_s2_equals_packs_of_the_strided_copies(hw, C, as_view):
    H, W = hw
    x = gen.activation("normal", gen.seed_of("pack-s2", C, H, W), (2, C, H, W))
    view = sliced(x, 5, C + 11)[1] if as_view else dev(x)
    a, b = affines(1, C, gen.seed_of("pack-s2-aff", C))
    copy = view.contiguous()
    for relu in (False, True):
        for aff in ((dev(a[0]), dev(b[0])), (None, None)):
            got = hipops.bn_act_pack_s2(view, *aff, relu=relu)
            for k, sub in enumerate((copy[:, :, ::2, ::2], copy[:, :, 1::2, 1::2])):
                want = hipops.bn_act_pack(sub.contiguous(), *aff, relu=relu)
                assert torch.equal(got[k].P, want.P) and torch.equal(got[k].M, want.M), (k, relu)
                assert got[k].shape == want.shape


def test_pack_s2_refuses_odd_sizes():
    x = dev(gen.activation("normal", 3, (1, 48, 7, 8)))
    with pytest.raises(NativeError):
        hipops.bn_act_pack_s2(x)
    with pytest.raises(NativeError):
        hipops.bn_act_pack_s2(x.transpose(2, 3).contiguous())


# ---- 3. the node kernel, bit for bit -------------------------------------------------------------------------------
def slopes(O, seed):
    """Per-channel PReLU slopes mixing < 0, 0, (0, 1) and > 1."""
    base = np.array([-0.5, 0.0, 0.25, 1.75], np.float32)[np.arange(O) % 4]
    return (base * (1.0 + 0.1 * gen.uniform(seed, (O,)))).astype(np.float32)


def node_reference(v, a, sg, res, add):
    """NumPy float32 (test_gpu_cellops.py: cell_reference, plus the addend): PReLU, the permuted assignment, the skip
    add, the addend — each operation rounded on its own."""
    v = v.astype(np.float32)
    if a is not None:
        v = np.where(v >= 0, v, a.astype(np.float32)[None, :, None, None] * v).astype(np.float32)
    O = v.shape[1]
    o = np.arange(O)
    dst = (o % (O // sg)) * sg + o // (O // sg) if sg > 1 else o
    out = np.empty_like(v)
    out[:, dst] = v
    if res is not None:
        out = (res + out).astype(np.float32)
    if add is not None:
        out = (out + add).astype(np.float32)
    return out


CASES_2D = [c for c in GROUPED_CASES if not c.conv1d]


@pytest.mark.parametrize("case", CASES_2D, ids=[c.name for c in CASES_2D])
def test_node_epilogue_equals_its_float32_restatement(case):
    x, w, b, sc = case.tensors()
    x2, w2, stride, pad, dil = as_2d(case, x, w)
    act = hipops.pack_act(dev(x2))
    pw = hipops.pack_weight_grouped(dev(w2), case.groups, case.center, case.compute_alpha)
    dot = oracle_dot(x2, w2, case.groups, stride, pad, dil, case.center)
    v = oracle.epilogue(dot, pw.alpha[:case.O].cpu().numpy(), b, sc)
    assert not np.isnan(v).any()
    O = case.O
    a = slopes(O, gen.seed_of("node-slope", case.name))
    res_np = gen.normal(gen.seed_of("node-res", case.name), v.shape)
    add_np = gen.normal(gen.seed_of("node-add", case.name), v.shape)
    _, res_v = sliced(res_np, 2, O + 3)
    _, add_v = sliced(add_np, 16, O + 16)
    args = (act, pw, dev(b), dev(sc), stride, pad, dil)
    n = 0
    for sg in (1, 4):
        if O % sg:
            continue                                            # (not a shuffle of this width: the entry point refuses it)
        for prelu in (None, a):
            for r in (None, res_v):
                for ad in (None, add_v):
                    whole = torch.full((v.shape[0], O + 40) + v.shape[2:], SENTINEL, dtype=torch.float32, device=DEV)
                    y = hipops.bconv2d_grouped_node(*args, prelu=dev(prelu), shuffle_groups=sg, residual=r, addend=ad,
                                                    out=whole[:, 8:8 + O])
                    assert y.data_ptr() == whole[:, 8:8 + O].data_ptr()
                    want = node_reference(v, prelu, sg, None if r is None else res_np, None if ad is None else add_np)
                    got = whole.cpu().numpy()
                    mine = got[:, 8:8 + O]
                    assert np.array_equal(mine, want), (case.name, sg, prelu is not None, r is not None, ad is not None,
                                                        float(np.abs(mine - want).max()))
                    assert (got[:, :8] == SENTINEL).all() and (got[:, 8 + O:] == SENTINEL).all()
                    n += 1
        # plain tensors and no addend: the bits of bnn_hip_bconv2d_grouped_fused
        res_c = dev(res_np)
        assert torch.equal(hipops.bconv2d_grouped_node(*args, prelu=dev(a), shuffle_groups=sg, residual=res_c),
                           hipops.bconv2d_grouped_fused(*args, prelu=dev(a), shuffle_groups=sg, residual=res_c))
    assert n >= 8


def test_node_aliasing_rule():
    C, G = 48, 12
    x = dev(gen.activation("normal", 4, (2, C, 6, 6)))
    act = hipops.pack_act(x)
    pw = hipops.pack_weight_grouped(dev(gen.conv_weight("kaiming", 3, (C, C // G, 3, 3))), G)
    cellout = torch.zeros((2, 3 * C, 6, 6), device=DEV)
    cellout[:, :C] = x
    # a node reads one slice of the cell output and writes another
    y = hipops.bconv2d_grouped_node(act, pw, padding=1, shuffle_groups=4, residual=cellout[:, :C],
                                    addend=cellout[:, :C], out=cellout[:, C:2 * C])
    want = hipops.bconv2d_grouped_fused(act, pw, padding=1, shuffle_groups=4, residual=x) + x
    assert torch.equal(y, want) and torch.equal(cellout[:, :C], x) and float(cellout[:, 2 * C:].abs().max()) == 0
    for bad in (cellout[:, C:2 * C], cellout[:, C - 1:2 * C - 1], cellout[:, C + 8:2 * C + 8]):
        with pytest.raises(NativeError):
            hipops.bconv2d_grouped_node(act, pw, padding=1, residual=bad, out=cellout[:, C:2 * C])
        with pytest.raises(NativeError):
            hipops.bconv2d_grouped_node(act, pw, padding=1, addend=bad, out=cellout[:, C:2 * C])
    with pytest.raises(NativeError):
        hipops.bconv2d_grouped_node(act, pw, padding=1, residual=x[:, :24])


# ---- 4. the cells --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cells():
    """Every cell case built once: name -> (cell, s0, s1)."""
    return {c.name: (build(c),) + tuple(dev(a) for a in c.inputs()) for c in CELL_CASES}


@pytest.mark.parametrize("case", CELL_CASES, ids=[c.name for c in CELL_CASES])
def test_cell_call_is_the_fused_cell(golden, cells, case):
    cell, s0, s1 = cells[case.name]
    ref = golden[case.name + "/out"]
    with torch.no_grad():
        before = fastpath.stats()
        y = cell(s0, s1, 0.0)
        after = fastpath.stats()
        assert after["cell"] == before["cell"] + 1, "the cell did not take the fused path"
        assert after["cell_op"] == before["cell_op"] and after["conv2d"] == before["conv2d"]
        err = float(np.abs(y.cpu().numpy() - ref).max())
        print(f"{case.name}: max |y - ref| = {err:.3g}, max |ref| = {np.abs(ref).max():.3g}")
        assert close(y.cpu().numpy(), ref)
        before = fastpath.stats()
        with no_cell_fusion():
            y_ops = cell(s0, s1, 0.0)
        after = fastpath.stats()
        assert after["cell"] == before["cell"] and after["cell_op"] > before["cell_op"]
        assert torch.equal(y, y_ops)
        eng = FusedCell(cell)
        assert torch.equal(y, eng(s0, s1))
        before = fastpath.stats()
        with per_layer_forward():
            y_layer = cell(s0, s1, 0.0)
        after = fastpath.stats()
        assert after["cell"] == before["cell"] and after["cell_op"] == before["cell_op"]
        assert close(y_layer.cpu().numpy(), ref)
    kinds = [k for k, _ in eng.steps]
    if case.name in ("reduce", "after_reduce"):
        assert "pack_s2" in kinds
    # training mode and autograd keep the composition
    before = fastpath.stats()["cell"]
    assert close(cell(s0, s1, 0.0).detach().cpu().numpy(), ref)
    assert fastpath.stats()["cell"] == before


def test_allconv_cell_plan_and_launch_count(cells):
    cell, s0, s1 = cells["allconv_none"]
    eng = FusedCell(cell)
    kinds = [k for k, _ in eng.steps]
    assert "torch_add" not in kinds and "copy" not in kinds
    covers_state_1 = [d for k, d in eng.steps if k == "pack_multi" and d["state"] == 1]
    assert len(covers_state_1) == 1 and covers_state_1[0]["sets"] == 4
    with torch.no_grad():
        eng(s0, s1)                                               # (weights are packed by now)
        before = native.launch_count()
        eng(s0, s1)
    # packs: 2 preprocess + state 0 (K = 2) + state 1 (K = 4) + state 2 = 5; convolutions: 2 dense + 7 grouped = 9
    assert native.launch_count() - before == 14


# ---- 5. the network ------------------------------------------------------------------------------------------------
def test_cifar_network_runs_every_cell_fused(golden):
    net = build(NET_CASE)
    x = dev(NET_CASE.inputs()[0])
    ref = golden["cifar_net/out"]
    before = fastpath.stats()["cell"]
    with torch.no_grad():
        logits, aux = net(x)
    assert aux is None
    assert fastpath.stats()["cell"] == before + len(net.cells)
    assert all(c.__dict__["_bnn_auto_cell"].calls == {"fused": 1, "declined": 0} for c in net.cells)
    err = float(np.abs(logits.cpu().numpy() - ref).max())
    print(f"cifar_net: max |logits - ref| = {err:.3g}, max |ref| = {np.abs(ref).max():.3g}")
    assert err <= 1e-3 * np.abs(ref).max()


# ---- 6. the cache --------------------------------------------------------------------------------------------------
def test_parameter_writes_reach_the_cell_executor():
    case = CELL_CASES[0]
    cell = build(case)
    s0, s1 = (dev(a) for a in case.inputs())
    with torch.no_grad():
        y0 = cell(s0, s1, 0.0)
        st = cell.__dict__["_bnn_auto_cell"]
        eng = st.engine
        assert eng is not None and torch.equal(cell(s0, s1, 0.0), y0) and st.engine is eng        # cached
        # version-bumping writes need nothing
        cell._ops[0].op[1].weight.mul_(-1)
        y1 = cell(s0, s1, 0.0)
        assert not torch.equal(y1, y0)
        cell._ops[1].op[0].running_mean.add_(0.7)
        y2 = cell(s0, s1, 0.0)
        assert not torch.equal(y2, y1)
        with no_cell_fusion():
            assert torch.equal(cell(s0, s1, 0.0), y2)
        # a write the version counters do not see: picked up after invalidate()
        cell._ops[0].op[1].weight.data.mul_(-1)
        assert torch.equal(cell(s0, s1, 0.0), y2), "a .data write is not seen before invalidate()"
        fastpath.invalidate(cell)
        assert "_bnn_auto_cell" not in cell.__dict__
        y3 = cell(s0, s1, 0.0)
        assert not torch.equal(y3, y2)
        cell._ops[1].op[0].running_mean.sub_(0.7)
        assert torch.equal(cell(s0, s1, 0.0), y0)                # both writes undone
    torch.cuda.synchronize()

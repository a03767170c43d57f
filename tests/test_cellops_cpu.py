"""The BATS cell operations without a GPU: bnn_amd.models.{SepConv, DilConv, ReLUConvBN, channel_shuffle} against the
reference's fixtures (tests/golden/cellops.npz, grouped.npz), the dispatch hook declining, the argument checks of
bnn_hip_bconv2d_grouped_fused and what FusedCellOp refuses."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import bnn_amd as bnn
from bnn_amd import fastpath, models, native
from bnn_amd.cellops import FusedCellOp
from bnn_amd.inference import FusionError, auto_op_forward
from bnn_amd.ops import BasicInputBinarizer, XNORWeightBinarizer
from tests.golden import gen
from tests.golden.cellops_cases import CELL_CASES, MIN_BN_MARGIN, bn_margin
from tests.golden.grouped_cases import OP_C, OP_CASES, op_input

IDS = [c.name for c in CELL_CASES]


def close(a, ref):
    """The project's layer bar."""
    return np.allclose(a, ref, rtol=1e-3, atol=1e-5 * np.abs(ref).max())


def binarise(op):
    cfg = bnn.BConfig(activation_pre_process=BasicInputBinarizer, activation_post_process=bnn.Identity,
                      weight_pre_process=XNORWeightBinarizer)
    return bnn.prepare_binary_model(op, cfg)


def load(op, state_fn):
    shapes = {k: tuple(v.shape) for k, v in op.state_dict().items()}
    st = state_fn(shapes)
    op.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    return op.eval(), st


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "cellops.npz"))


@pytest.fixture(scope="module")
def golden_grouped(golden_dir):
    return np.load(os.path.join(golden_dir, "grouped.npz"))


def test_the_four_names_are_exported():
    for name in ("SepConv", "DilConv", "ReLUConvBN", "channel_shuffle"):
        assert hasattr(models, name) and name in models.__all__
    assert "cell_op" in fastpath.stats()
    from bnn_amd import inference
    assert inference.FusedCellOp is FusedCellOp


@pytest.mark.parametrize("case", CELL_CASES, ids=IDS)
def test_module_reproduces_the_reference_fixture(golden, case):
    op = binarise(case.build(models))
    assert isinstance(op.op[1], bnn.layers.Conv2d)
    assert list(op.state_dict().keys()) == [str(k) for k in golden[case.name + "/keys"]]
    op, st = load(op, case.state)
    x = case.input()
    assert bn_margin(x, st) >= MIN_BN_MARGIN
    with torch.no_grad():
        y = op(torch.from_numpy(x)).numpy()
    ref = golden[case.name + "/out"]
    assert y.shape == ref.shape
    err = np.abs(y - ref).max()
    print(f"{case.name}: max |y - ref| = {err:.3g}, max |ref| = {np.abs(ref).max():.3g}")
    assert close(y, ref)


@pytest.mark.parametrize("name", list(OP_CASES))
def test_module_reproduces_the_grouped_op_fixtures(golden_grouped, name):
    kw = OP_CASES[name]
    if name == "sepconv":
        op = models.SepConv(OP_C, OP_C, kw["kernel_size"], 1, kw["padding"], groups=12)
    else:
        op = models.DilConv(OP_C, OP_C, kw["kernel_size"], 1, kw["padding"], kw["dilation"], groups=12)
    op = binarise(op)
    assert list(op.state_dict().keys()) == [str(k) for k in golden_grouped["op/" + name + "/keys"]]
    op, _ = load(op, lambda shapes: gen.model_state(shapes, gen.seed_of("grouped-op", name)))
    with torch.no_grad():
        y = op(torch.from_numpy(op_input(name))).numpy()
    assert close(y, golden_grouped["op/" + name + "/out"])


@pytest.mark.parametrize("g", [1, 2, 4, 12])
def test_channel_shuffle_is_the_index_map(g):
    C = 48
    x = torch.from_numpy(gen.normal(3, (2, C, 3, 5)))
    y = models.channel_shuffle(x, g)
    o = np.arange(C)
    dst = (o % (C // g)) * g + o // (C // g)
    want = torch.empty_like(x)
    want[:, torch.from_numpy(dst)] = x
    assert torch.equal(y, want)
    assert sorted(dst.tolist()) == list(range(C))


def test_dispatch_hook_declines_on_the_cpu_and_in_training_mode_and_gradients_flow():
    case = CELL_CASES[0]
    op, _ = load(binarise(case.build(models)), case.state)
    x = torch.from_numpy(case.input())
    with torch.no_grad():
        assert auto_op_forward(op, x) is None                   # CPU tensor
    st = op.__dict__["_bnn_auto_op"]
    assert st.calls["fused"] == 0 and st.calls["declined"] == 1
    op.train()
    assert "_bnn_auto_op" not in op.__dict__                     # the mode switch drops the executor state
    with torch.no_grad():
        assert auto_op_forward(op, x) is None                   # training mode
    before = fastpath.stats()["cell_op"]
    xg = x.clone().requires_grad_()
    y = op(xg)
    y.sum().backward()
    assert fastpath.stats()["cell_op"] == before
    assert xg.grad is not None and float(xg.grad.abs().sum()) > 0
    for p in op.parameters():
        assert p.grad is not None
    import copy
    import pickle
    op.eval()
    with torch.no_grad():
        assert auto_op_forward(op, x) is None
    assert copy.deepcopy(op).__dict__["_bnn_auto_op"].engine is None
    assert pickle.loads(pickle.dumps(op)).__dict__["_bnn_auto_op"].engine is None


def test_entry_point_rejects_bad_arguments_without_a_gpu():
    lib = native.require()
    f = lib.bnn_hip_bconv2d_grouped_fused
    d = native.ConvDesc(1, 48, 8, 8, 48, 3, 3, 1, 1, 1, 1, 1, 1, 0)
    ok = dict(P=0x10000, M=0x20000, W=0x30000, Z=0x40000, alpha=0x50000, prelu=0x60000, res=0x70000, out=0x80000)

    def call(desc=d, groups=12, sg=4, bias=None, scale=None, **kw):
        a = dict(ok, **kw)
        return f(ctypes.byref(desc) if desc is not None else None, groups, a["P"], a["M"], a["W"], a["Z"], a["alpha"], bias,
                 scale, a["prelu"], sg, a["res"], a["out"], None)

    assert call(desc=None) == native.ERR_INVALID_ARG
    for k in ("P", "M", "W", "Z", "out"):
        assert call(**{k: None}) == native.ERR_INVALID_ARG, k
    assert call(alpha=None) == native.ERR_INVALID_ARG            # no raw-dot form
    assert call(sg=0) == native.ERR_INVALID_ARG
    assert call(sg=-4) == native.ERR_INVALID_ARG
    assert call(sg=5) == native.ERR_INVALID_ARG                  # 48 % 5 != 0
    assert call(sg=32) == native.ERR_INVALID_ARG
    assert call(res=ok["out"]) == native.ERR_INVALID_ARG         # no in-place skip
    assert call(res=0x70002) == native.ERR_INVALID_ARG           # misaligned residual
    assert call(groups=0) == native.ERR_INVALID_ARG              # and everything bnn_hip_bconv2d_grouped checks
    assert call(groups=5) == native.ERR_INVALID_ARG
    assert call(P=0x10008) == native.ERR_INVALID_ARG
    assert call(out=0x80002) == native.ERR_INVALID_ARG


class _Foreign(nn.Module):
    def forward(self, x):
        return torch.sign(x)


def test_fused_cell_op_refuses_what_it_does_not_cover():
    case = CELL_CASES[0]
    good, _ = load(binarise(case.build(models)), case.state)
    FusedCellOp(good)                                            # recognised (the launch data waits for a HIP device)
    with pytest.raises(FusionError):
        FusedCellOp(good)(torch.from_numpy(case.input()))       # a CPU tensor
    with pytest.raises(FusionError):                             # training mode
        FusedCellOp(load(binarise(case.build(models)), case.state)[0].train())

    op, _ = load(binarise(case.build(models)), case.state)
    op.op[1].activation_pre_process = _Foreign()                 # a foreign hook on the convolution
    with pytest.raises(FusionError):
        FusedCellOp(op)

    op = case.build(models)
    op.op[0] = nn.BatchNorm2d(case.C_in, track_running_stats=False)
    with pytest.raises(FusionError):
        FusedCellOp(binarise(op).eval())

    op = binarise(case.build(models)).eval()                     # a wrong `op` layout
    op.op = nn.Sequential(op.op[0], op.op[1], op.op[2], nn.Identity())
    with pytest.raises(FusionError):
        FusedCellOp(op)
    op = binarise(case.build(models)).eval()
    op.op = nn.Sequential(op.op[0], op.op[1], nn.ReLU())
    with pytest.raises(FusionError):
        FusedCellOp(op)
    with pytest.raises(FusionError):                             # not binarised: a stock nn.Conv2d
        FusedCellOp(case.build(models).eval())

    class Other(nn.Module):                                      # the right layout under another class name
        def __init__(self, inner):
            super().__init__()
            self.op, self.stride, self.skip = inner.op, inner.stride, inner.skip

    with pytest.raises(FusionError):
        FusedCellOp(Other(good).eval())

    op, _ = load(binarise(case.build(models)), case.state)
    op.stride = 2                                                # stride unlike the convolution's
    with pytest.raises(FusionError):
        FusedCellOp(op)
    op = binarise(models.SepConv(48, 48, 3, 1, 1, groups=12)).eval()
    op.op[1].padding_mode = "reflect"
    with pytest.raises(FusionError):
        FusedCellOp(op)
    with pytest.raises(FusionError):
        FusedCellOp(binarise(case.build(models)).eval().half())

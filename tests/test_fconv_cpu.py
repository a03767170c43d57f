"""FactorizedConv ('conv_7x1_1x7') and 'sep_conv_7x7' without a GPU: bnn_amd.models.{FactorizedConv, EXTENDED_OPS,
ALL_OPS} against the reference's fixtures (tests/golden/fconv.npz), the NumPy restatement of the one-launch kernel's
arithmetic (tests/fconv_ref.py) against the module, a Cell whose genotype names both primitives, the new C-ABI symbols,
and what FusedFactorizedConv refuses."""
import os

import numpy as np
import pytest
import torch

import bnn_amd as bnn
import oracle
from bnn_amd import fastpath, inference, models, native
from bnn_amd.cellops import FusedCell, FusedFactorizedConv
from bnn_amd.inference import FusionError, fold_bn
from bnn_amd.ops import BasicInputBinarizer, XNORWeightBinarizer
from tests import fconv_ref
from tests.golden.fconv_cases import FACTORIZED, FCONV_CASES

IDS = [c.name for c in FCONV_CASES]


def close(a, ref):
    """The project's layer bar."""
    return np.allclose(a, ref, rtol=1e-3, atol=1e-5 * np.abs(ref).max())


def binarise(model):
    cfg = bnn.BConfig(activation_pre_process=BasicInputBinarizer, activation_post_process=bnn.Identity,
                      weight_pre_process=XNORWeightBinarizer)
    return bnn.prepare_binary_model(model, cfg)


def build(case):
    op = binarise(case.build(models))
    shapes = {k: tuple(v.shape) for k, v in op.state_dict().items()}
    op.load_state_dict({k: torch.from_numpy(v) for k, v in case.state(shapes).items()})
    return op.eval()


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "fconv.npz"))


def test_the_new_names_are_exported(golden):
    for name in ("FactorizedConv", "EXTENDED_OPS", "ALL_OPS"):
        assert hasattr(models, name) and name in models.__all__, name
    ref_names = [str(n) for n in golden["ops"]]
    assert len(models.ALL_OPS) == len(ref_names) == 10 and set(models.ALL_OPS) == set(ref_names)
    assert set(models.EXTENDED_OPS) == {"sep_conv_7x7", "conv_7x1_1x7"}
    assert set(models.OPS) == set(models.PRIMITIVES) and not set(models.OPS) & set(models.EXTENDED_OPS)
    assert all(models.ALL_OPS[n] is models.OPS[n] for n in models.OPS)
    assert "fconv" in fastpath.stats()
    assert inference.FusedFactorizedConv is FusedFactorizedConv
    for name in ("FactorizedFusion", "auto_fconv_forward"):
        assert hasattr(inference, name)


def test_the_new_symbols_are_exported_and_the_abi_is_still_16():
    for sym in ("bnn_hip_fconv_supported", "bnn_hip_fconv_fused"):
        assert sym in native.EXPORTED_SYMBOLS
    lib = native.require()
    assert lib.bnn_hip_abi_version() == native.ABI_VERSION == 16
    # the HOST query: what fits the LDS rule, and what does not
    assert lib.bnn_hip_fconv_supported(native.FconvDesc(256, 48, 32, 32, 7, 1, 0, 0)) == 1
    assert lib.bnn_hip_fconv_supported(native.FconvDesc(256, 80, 28, 28, 7, 2, 0, 0)) == 1
    assert lib.bnn_hip_fconv_supported(native.FconvDesc(2, 48, 3, 5, 7, 1, 0, 0)) == 1
    for bad in ((2, 48, 8, 8, 4, 1), (2, 48, 8, 8, 9, 1), (2, 48, 8, 8, 7, 3), (2, 512, 224, 224, 7, 1), (0, 48, 8, 8, 7, 1)):
        assert lib.bnn_hip_fconv_supported(native.FconvDesc(*bad, 0, 0)) == 0, bad
    assert lib.bnn_hip_fconv_supported(None) == 0
    # and the entry point's argument checks need no device: null pointers are refused before anything is launched
    d = native.FconvDesc(2, 48, 8, 8, 7, 1, 0, 0)
    import ctypes
    st = native.FconvStage(None, None, None, None)
    assert lib.bnn_hip_fconv_fused(ctypes.byref(d), None, None, None, None, ctypes.byref(st), None, None, ctypes.byref(st),
                                   None, None, 4, None, None, None) == native.ERR_INVALID_ARG


@pytest.mark.parametrize("case", FCONV_CASES, ids=IDS)
def test_module_reproduces_the_reference_fixture(golden, case):
    op = build(case)
    assert type(op).__name__ == ("FactorizedConv" if case.kind == "conv_7x1_1x7" else "SepConv")
    assert list(op.state_dict().keys()) == [str(k) for k in golden[case.name + "/keys"]]
    with torch.no_grad():
        y = op(torch.from_numpy(case.input())).numpy()
    ref = golden[case.name + "/out"]
    print(f"{case.name}: max |y - ref| = {np.abs(y - ref).max():.3g}, max |ref| = {np.abs(ref).max():.3g}")
    assert y.shape == ref.shape
    assert close(y, ref)


def restate(op, x, **over):
    """tests/fconv_ref.fconv on the module's parameters: (out, t)."""
    bn1, c1, a1, bn2, c2, a2 = op.op
    (a, b), (ma, mb) = (tuple(t.numpy() for t in fold_bn(bn)) for bn in (bn1, bn2))
    w1, w2 = c1.weight.detach().numpy(), c2.weight.detach().numpy()
    kw = dict(prelu1=a1.weight.detach().numpy(), prelu2=a2.weight.detach().numpy(), shuffle_groups=4,
              residual=x if op.stride == 1 else None)
    kw.update(over)
    return fconv_ref.fconv(oracle.bn_act(x, a, b), w1, w2, oracle.xnor_weight(w1)[2], oracle.xnor_weight(w2)[2], ma, mb,
                           op.stride, **kw)


@pytest.mark.parametrize("case", FACTORIZED, ids=[c.name for c in FACTORIZED])
def test_restatement_agrees_with_the_module(golden, case):
    op = build(case)
    x = case.input()
    out, t = restate(op, x)
    assert set(np.unique(t)) <= {-1.0, 0.0, 1.0} and t.shape == (case.N, case.C, case.H, (case.W - 1) // case.stride + 1)
    with torch.no_grad():
        y = op(torch.from_numpy(x)).numpy()
    print(f"{case.name}: max |restatement - module| = {np.abs(out - y).max():.3g}")
    assert close(out, y)
    assert close(out, golden[case.name + "/out"])


def test_restatement_puts_zero_rows_not_signs_of_a_padded_dot_outside_the_image():
    """A bias in front of the middle sign makes sign(BN2(PReLU(0 + bias))) non-zero: rows of t outside the image must
    still count as zeros in the second convolution, as torch's zero padding of the binarised tensor does."""
    case = FACTORIZED[4]        # 3 x 5: every output row reads rows outside the image
    op = build(case)
    bias = (0.5 + np.arange(case.C, dtype=np.float32) / case.C)
    op.op[1].bias = torch.nn.Parameter(torch.from_numpy(bias))
    x = case.input()
    out, _ = restate(op, x, bias1=bias)
    with torch.no_grad():
        y = op(torch.from_numpy(x)).numpy()
    assert close(out, y)


def test_a_cell_naming_both_new_primitives_builds_and_runs():
    g = models.Genotype(normal=[("conv_7x1_1x7", 0), ("sep_conv_7x7", 1), ("sep_conv_3x3", 0), ("conv_7x1_1x7", 2)],
                        normal_concat=[2, 3],
                        reduce=[("sep_conv_7x7", 0), ("conv_7x1_1x7", 1), ("max_pool_3x3", 0), ("conv_7x1_1x7", 2)],
                        reduce_concat=[2, 3])
    x = torch.from_numpy(FCONV_CASES[0].input()[:, :, :8, :8].copy())
    for reduction in (False, True):
        cell = binarise(models.Cell(g, 48, 48, 48, reduction, False)).eval()
        kinds = [type(op).__name__ for op in cell._ops]
        assert kinds.count("FactorizedConv") == 2 and "SepConv" in kinds
        assert [op.stride for op in cell._ops if type(op).__name__ == "FactorizedConv"] == ([2, 1] if reduction else [1, 1])
        with torch.no_grad():
            y = cell(x, x, 0.0)
        assert y.shape == (2, 96, 4, 4) if reduction else y.shape == (2, 96, 8, 8)
        assert torch.isfinite(y).all()
        with pytest.raises(FusionError):            # the whole-cell executor keeps declining a FactorizedConv term
            FusedCell(cell)
    with pytest.raises(KeyError):
        models.Cell(models.Genotype([("conv_9x1_1x9", 0)] * 4, [2, 3], [("none", 0)] * 4, [2, 3]), 48, 48, 48, False, False)


def test_training_mode_keeps_the_modules_own_forward():
    op = build(FACTORIZED[0]).train()
    x = torch.from_numpy(FACTORIZED[0].input()).requires_grad_()
    y = op(x)
    y.sum().backward()
    assert x.grad is not None and all(p.grad is not None for p in op.parameters())
    assert "_bnn_auto_op" not in op.__dict__


def test_executor_refuses_what_it_does_not_cover():
    case = FACTORIZED[0]
    with pytest.raises(FusionError, match="prepare_binary_model"):
        FusedFactorizedConv(case.build(models).eval())                      # not binarised
    with pytest.raises(FusionError, match="eval"):
        FusedFactorizedConv(build(case).train())                            # training mode
    with pytest.raises(FusionError, match="FactorizedConv"):
        FusedFactorizedConv(build(FCONV_CASES[6]))                          # a SepConv
    op = build(case)
    op.op[4].stride = (1, 1) if case.stride != 1 else (2, 1)                # not the constructor's geometry
    with pytest.raises(FusionError, match="dense"):
        FusedFactorizedConv(op)
    op = build(case)
    op.op[3].track_running_stats, op.op[3].running_mean, op.op[3].running_var = False, None, None
    with pytest.raises(FusionError, match="running statistics"):
        FusedFactorizedConv(op)
    eng = FusedFactorizedConv(build(case))                                   # builds on the CPU; runs on a HIP device only
    assert eng.C == case.C and eng.K == 7 and eng.add_skip
    with pytest.raises(FusionError):
        eng(torch.from_numpy(case.input()))

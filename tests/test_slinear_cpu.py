"""The Linear with binary activations and real weights (csrc/slinear.hip) on a GPU-less machine: its two C-ABI symbols,
the validators of the entry points, the two plan functions of ``fastpath`` with every reason they decline for, the new
counters, and a numpy statement of the plane words the kernel writes."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import bnn_amd as bnn
from bnn_amd import fastpath, native
from bnn_amd.ops import AdvancedInputBinarizer, BasicInputBinarizer, BasicScaleBinarizer, XNORWeightBinarizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
SYMBOLS = ("bnn_hip_slinear_f32", "bnn_hip_ste_mask_f32")


# ---- the C-ABI -----------------------------------------------------------------------------------------------------
def test_header_exports_and_bindings_agree_on_the_two_symbols():
    text = open(os.path.join(ROOT, "include", "bnn_hip.h")).read()
    assert re.search(r"#define\s+BNN_HIP_ABI_VERSION\s+16\b", text)
    lib = native.require()
    assert lib.bnn_hip_abi_version() == native.ABI_VERSION == 16
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), f"{s} is not declared in include/bnn_hip.h"
        assert hasattr(lib, s), f"{s} is not exported"
        assert getattr(lib, s).argtypes is not None, f"{s} has no binding in native.py"
    assert len(lib.bnn_hip_slinear_f32.argtypes) == 12 and len(lib.bnn_hip_ste_mask_f32.argtypes) == 5


def test_entry_point_validators_without_a_gpu():
    lib = native.require()
    launches = native.launch_count()
    f = lib.bnn_hip_slinear_f32
    ok = dict(M=4, F=8, O=8, x=16, packed=16, bias=None, scale=None, out=16, P=None, Mn=None, T=None)

    def call(**kw):
        a = {**ok, **kw}
        return f(a["M"], a["F"], a["O"], a["x"], a["packed"], a["bias"], a["scale"], a["out"], a["P"], a["Mn"], a["T"], None)
    for kw in (dict(x=None), dict(packed=None), dict(out=None), dict(M=0), dict(F=0), dict(O=0), dict(M=-1), dict(F=-3),
               dict(O=-2), dict(packed=8), dict(x=2), dict(out=2), dict(bias=2), dict(scale=6),
               dict(P=16), dict(P=16, Mn=16), dict(Mn=16, T=16), dict(T=16),            # a partial set of planes
               dict(P=4, Mn=16, T=16), dict(P=16, Mn=16, T=12)):                        # planes: 8-byte aligned
        assert call(**kw) == native.ERR_INVALID_ARG, kw
    assert call(M=1 << 20, F=1 << 10) == native.ERR_TOO_LARGE                           # M * F = 2^30
    assert call(M=1 << 20, O=1 << 10) == native.ERR_TOO_LARGE                           # M * O = 2^30
    g = lib.bnn_hip_ste_mask_f32
    assert g(None, 16, 4, 8, None) == native.ERR_INVALID_ARG and g(16, None, 4, 8, None) == native.ERR_INVALID_ARG
    assert g(16, 16, 0, 8, None) == native.ERR_INVALID_ARG and g(16, 16, 4, -1, None) == native.ERR_INVALID_ARG
    assert g(2, 16, 4, 8, None) == native.ERR_INVALID_ARG and g(16, 4, 4, 8, None) == native.ERR_INVALID_ARG
    assert g(16, 16, 1 << 15, 1 << 15, None) == native.ERR_TOO_LARGE
    assert native.launch_count() == launches                                           # a refused call launches nothing


# ---- dispatch ------------------------------------------------------------------------------------------------------
STEP0 = dict(activation_pre_process=BasicInputBinarizer, activation_post_process=BasicScaleBinarizer,
             weight_pre_process=nn.Identity)


def layer(fin=8, fout=8, bias=True, **hooks):
    return bnn.layers.Linear.from_module(nn.Linear(fin, fout, bias), bnn.BConfig(**{**STEP0, **hooks}))


class FakeCuda:
    """The plan functions look at a tensor's device, dtype, shape and requires_grad, never at its values."""

    def __init__(self, shape, dtype=torch.float32, requires_grad=False):
        self.shape, self.dtype, self.requires_grad = torch.Size(shape), dtype, requires_grad
        self.is_cuda, self.device = True, torch.device("cuda", 0)

    def dim(self):
        return len(self.shape)


def on_fake_device(m, dtype=torch.float32):
    """The layer as the plan functions see it once it lives on a HIP device."""
    shape = m.weight.shape
    m.__dict__["weight"] = FakeCuda(shape, dtype, requires_grad=True)
    del m._parameters["weight"]
    return m


@pytest.fixture
def real_weights():
    old = fastpath.REAL_WEIGHTS
    fastpath.REAL_WEIGHTS = True
    yield
    fastpath.REAL_WEIGHTS = old


def test_plans_are_none_with_the_switch_off_and_the_counters_exist():
    assert fastpath.REAL_WEIGHTS is False                                       # the default
    m, x = on_fake_device(layer()), FakeCuda((3, 5, 8))
    assert fastpath.plan_linear_real(m, x) is None and fastpath.plan_linear_real_train(m, x) is None
    with torch.no_grad():
        assert fastpath.plan_linear_real(m, x) is None
    stats = fastpath.stats()
    assert stats["linear_real"] == 0 and stats["linear_real_train"] == 0


def test_plans_admit_the_step0_linear_and_state_each_decline_reason(real_weights, monkeypatch):
    x = FakeCuda((3, 5, 8))
    with torch.no_grad():                                                                   # no grad: inference only
        assert isinstance(fastpath.plan_linear_real(on_fake_device(layer()), x), fastpath.RealPlan)
        assert isinstance(fastpath.plan_linear_real(on_fake_device(layer()), FakeCuda((8,))), fastpath.RealPlan)
        assert fastpath.plan_linear_real_train(on_fake_device(layer()), x) is None          # autograd is not recording
    assert fastpath.plan_linear_real(on_fake_device(layer()), x) is None                    # grad: the weight needs one
    for kw in (dict(), dict(bias=False), dict(activation_post_process=bnn.Identity), dict(weight_pre_process=bnn.Identity)):
        plan = fastpath.plan_linear_real_train(on_fake_device(layer(**kw)), x)
        assert isinstance(plan, fastpath.RealPlan) and plan.ste
        assert (plan.scale is None) == ("activation_post_process" in kw)
    hooked = layer()
    hooked.weight_pre_process.register_forward_hook(lambda m, i, o: o)
    declines = {
        "XNOR weight hook": (layer(weight_pre_process=XNORWeightBinarizer), x, torch.float32),   # plan_linear's
        "hooked weight hook": (hooked, x, torch.float32),
        "fp16": (layer(), FakeCuda((3, 5, 8), torch.float16), torch.float16),
        "fp16 input only": (layer(), FakeCuda((3, 5, 8), torch.float16), torch.float32),
        "no input hook": (layer(activation_pre_process=nn.Identity), x, torch.float32),
        "CPU tensor": (layer(), torch.zeros(3, 5, 8), torch.float32),
    }
    for why, (m, xin, dtype) in declines.items():
        m = on_fake_device(m, dtype)
        assert fastpath.plan_linear_real_train(m, xin) is None, why
        with torch.no_grad():
            assert fastpath.plan_linear_real(m, xin) is None, why
    m = on_fake_device(layer())
    with monkeypatch.context() as mp:      # (device autocast cannot be entered without a device: the GPU test does)
        mp.setattr(torch, "is_autocast_enabled", lambda *a: True)
        assert fastpath.plan_linear_real_train(m, x) is None, "autocast"
        with torch.no_grad():
            assert fastpath.plan_linear_real(m, x) is None, "autocast"
    assert fastpath.plan_linear_real_train(m, x) is not None
    adv = on_fake_device(layer(activation_pre_process=AdvancedInputBinarizer))
    assert fastpath.plan_linear_real_train(adv, x) is None                                  # tanh STE: composition
    with torch.no_grad():
        plan = fastpath.plan_linear_real(adv, x)
        assert plan is not None and not plan.ste
    # the XNOR layer still belongs to plan_linear, and the real plans leave it alone
    xnor = on_fake_device(layer(weight_pre_process=XNORWeightBinarizer))
    with torch.no_grad():
        assert fastpath.plan_linear(xnor, x) is not None and fastpath.plan_linear_real(xnor, x) is None
        assert fastpath.plan_linear(on_fake_device(layer()), x) is None


def test_cpu_forward_is_the_composition_whatever_the_switch(real_weights):
    m = layer(33, 7)
    x = torch.randn(3, 5, 33)
    before = fastpath.stats()
    want = torch.nn.functional.linear(torch.sign(x), m.weight, m.bias) * m.activation_post_process.alpha
    assert torch.equal(m(x), want) and fastpath.stats() == before


# ---- the plane words -------------------------------------------------------------------------------------------------
def plane_words(x):
    """P / Mn / T of an fp32 [M, F] array as the kernel writes them: [M][ceil(F/64)] 64-bit words, feature f in bit f % 64
    of word f // 64, pad bits 0."""
    M, F = x.shape
    FW = (F + 63) // 64
    out = []
    with np.errstate(invalid="ignore"):
        for pred in (x > 0, x < 0, np.abs(x) < 1):
            bits = np.zeros((M, FW * 64), np.uint64)
            bits[:, :F] = pred
            out.append((bits.reshape(M, FW, 64) << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64))
    return out


@pytest.mark.parametrize("F", [1, 63, 64, 65])
def test_plane_words_have_zero_pad_bits(F):
    rng = np.random.default_rng(F)
    vals = np.array([0.0, -0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0, np.nan, np.inf, -np.inf, 1e-45, -1e-45], F32)
    x = vals[rng.integers(0, len(vals), (5, F))]
    x[0] = 0.25                                                    # every live bit of P and T set, none of Mn
    P, Mn, T = plane_words(x)
    FW = (F + 63) // 64
    assert P.shape == Mn.shape == T.shape == (5, FW)
    live = (1 << (F - 64 * (FW - 1))) - 1                          # the last word's live bits
    for w in (P, Mn, T):
        assert not (w[:, -1] & ~np.uint64(live)).any()
    assert int(P[0, -1]) == int(T[0, -1]) == live and not Mn[0].any()
    assert (P & Mn == 0).all()
    for m in range(5):
        for f in range(F):
            v = x[m, f]
            got = tuple(int(w[m, f // 64] >> np.uint64(f % 64)) & 1 for w in (P, Mn, T))
            assert got == (int(v > 0), int(v < 0), int(abs(v) < 1)), (m, f, v)

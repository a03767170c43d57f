"""bfloat16 models and autocast on the HIP inference path, on a GPU-less machine: the admission predicate's truth table,
the additive C-ABI pieces and their validators, and the fixture ``tests/golden/lowp_layers.npz`` against the two-rounding
model of a 16-bit layer stated in numpy (so that the fixture and the model cannot drift apart)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import bnn_amd as bnn
from bnn_amd import fastpath, hipops, native
from bnn_amd.ops import BasicInputBinarizer, BasicScaleBinarizer, XNORWeightBinarizer
from tests.golden import make_golden_lowp as glp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
XNOR = dict(activation_pre_process=BasicInputBinarizer, activation_post_process=BasicScaleBinarizer,
            weight_pre_process=XNORWeightBinarizer)


@pytest.fixture(scope="module")
def fixture():
    with np.load(os.path.join(ROOT, "tests", "golden", "lowp_layers.npz")) as z:
        return {k: z[k] for k in z.files}


# ---- dispatch --------------------------------------------------------------------------------------------------------
class FakeCuda:
    """The plan functions look at a tensor's device, dtype, shape and requires_grad, never at its values."""

    def __init__(self, shape, dtype=F32, requires_grad=False, device=0):
        self.shape, self.dtype, self.requires_grad = torch.Size(shape), dtype, requires_grad
        self.is_cuda, self.device = True, torch.device("cuda", device)

    def dim(self):
        return len(self.shape)


def on_fake_device(m, dtype=F32, requires_grad=False):
    m.__dict__["weight"] = FakeCuda(m.weight.shape, dtype, requires_grad)
    del m._parameters["weight"]
    if m.bias is not None:
        m.bias.requires_grad_(False)
    m.activation_post_process.alpha.requires_grad_(False)
    return m


def conv(dtype=F32, **kw):
    return on_fake_device(bnn.layers.Conv2d.from_module(nn.Conv2d(8, 8, 3, padding=1), bnn.BConfig(**XNOR)), dtype, **kw)


class cast:
    """The thread state ``torch.autocast("cuda", dtype)`` sets (the context manager itself turns into a no-op on a machine
    without a GPU) — or nothing for ``None``."""

    def __init__(self, dtype):
        self.dtype = dtype

    def __enter__(self):
        self.old = (torch.is_autocast_enabled("cuda"), torch.get_autocast_dtype("cuda"))
        if self.dtype is not None:
            torch.set_autocast_enabled("cuda", True)
            torch.set_autocast_dtype("cuda", self.dtype)

    def __exit__(self, *a):
        torch.set_autocast_enabled("cuda", self.old[0])
        torch.set_autocast_dtype("cuda", self.old[1])


# (weight dtype, input dtype, autocast dtype or None) -> D
TRUTH = {
    (BF16, BF16, None): BF16,        # case 1: a bf16 model
    (BF16, BF16, BF16): BF16,        #   ... under its own autocast: the casts are no-ops
    (BF16, BF16, F16): None,         #   ... under fp16 autocast the reference would compute in fp16
    (BF16, F32, None): None, (BF16, F16, None): None, (BF16, F32, BF16): None,
    (F32, BF16, BF16): BF16,         # case 2: autocast, both dtypes
    (F32, F16, F16): F16,
    (F32, BF16, F16): None, (F32, F16, BF16): None,      # an input that is not of the autocast dtype
    (F32, BF16, None): None, (F32, F16, None): None,     # 16-bit input, fp32 weight, no autocast: the composition raises
    (F32, F32, None): None, (F32, F32, BF16): None, (F32, F32, F16): None,   # fp32 input: today's path, not a new case
    (F16, F16, None): None, (F16, F16, F16): None, (F16, F16, BF16): None,   # `.half()` models keep their own rule
    (F16, BF16, None): None,
}


@pytest.mark.parametrize("wd,xd,ac", list(TRUTH), ids=lambda d: "none" if d is None else str(d).split(".")[-1])
def test_lowp_dtype_truth_table(wd, xd, ac):
    m, x = conv(wd), FakeCuda((2, 8, 5, 5), xd)
    with torch.no_grad(), cast(ac):
        assert fastpath.lowp_dtype(m, x) is TRUTH[(wd, xd, ac)]
        # what the plan function says: the new cases, plus the two it admitted before (fp32 / fp32 and fp16 / fp16)
        old = wd == xd and wd in (F32, F16)
        assert (fastpath.plan_conv2d(m, x) is not None) == (old or TRUTH[(wd, xd, ac)] is not None)


def test_lowp_dtype_needs_one_hip_device_and_no_autograd():
    m = conv(BF16)
    assert fastpath.lowp_dtype(m, FakeCuda((2, 8, 5, 5), BF16, device=1)) is None
    assert fastpath.lowp_dtype(m, torch.zeros(2, 8, 5, 5, dtype=BF16)) is None          # a CPU tensor
    with torch.no_grad():
        assert fastpath.plan_conv2d(m, FakeCuda((2, 8, 5, 5), BF16)) is not None
    with torch.enable_grad():                                                          # training stays on the composition
        assert fastpath.plan_conv2d(conv(BF16, requires_grad=True), FakeCuda((2, 8, 5, 5), BF16)) is None
        assert fastpath.plan_conv2d(m, FakeCuda((2, 8, 5, 5), BF16, requires_grad=True)) is None
        assert fastpath.plan_conv2d_train(conv(BF16, requires_grad=True), FakeCuda((2, 8, 5, 5), BF16)) is None
        with cast(BF16):
            assert fastpath.plan_conv2d(conv(F32, requires_grad=True), FakeCuda((2, 8, 5, 5), BF16)) is None


def test_conv1d_and_linear_take_the_same_predicate():
    c1 = on_fake_device(bnn.layers.Conv1d.from_module(nn.Conv1d(8, 8, 3), bnn.BConfig(**XNOR)), BF16)
    fc = on_fake_device(bnn.layers.Linear.from_module(nn.Linear(8, 8), bnn.BConfig(**XNOR)), F32)
    with torch.no_grad():
        assert fastpath.plan_conv1d(c1, FakeCuda((2, 8, 9), BF16)) is not None
        assert fastpath.plan_linear(fc, FakeCuda((2, 8), F16)) is None
        with cast(F16):
            assert fastpath.plan_linear(fc, FakeCuda((2, 8), F16)) is not None


def test_real_weight_path_still_declines_16_bits(monkeypatch):
    monkeypatch.setattr(fastpath, "REAL_WEIGHTS", True)
    step0 = dict(XNOR, weight_pre_process=nn.Identity)
    m = on_fake_device(bnn.layers.Conv2d.from_module(nn.Conv2d(8, 8, 3, padding=1), bnn.BConfig(**step0)), F32)
    with torch.no_grad():
        with cast(BF16):
            assert fastpath.plan_conv2d_real(m, FakeCuda((2, 8, 5, 5), BF16)) is None
            assert fastpath.plan_conv2d_real(m, FakeCuda((2, 8, 5, 5), F32)) is None
        m16 = on_fake_device(bnn.layers.Conv2d.from_module(nn.Conv2d(8, 8, 3, padding=1), bnn.BConfig(**step0)), BF16)
        assert fastpath.plan_conv2d_real(m16, FakeCuda((2, 8, 5, 5), BF16)) is None


def test_store_admission_table_is_keyed_by_shape():
    key = (BF16, 64, 64, 56, 56, 3, 1)
    assert fastpath.lowp_store_admitted(*key) == (key not in fastpath.LOWP_STORE_DECLINED_SHAPES)
    for k, v in fastpath.LOWP_STORE_DECLINED_SHAPES.items():
        assert k[0] in (F16, BF16) and len(k) == 7 and len(v) == 2 and v[1] > v[0]     # listed only where the store lost


# ---- the C-ABI -------------------------------------------------------------------------------------------------------
def test_header_declares_the_new_pieces():
    text = open(os.path.join(ROOT, "include", "bnn_hip.h")).read()
    assert re.search(r"#define\s+BNN_HIP_ABI_VERSION\s+16\b", text)
    assert re.search(r"\bbnn_hip_pack_act_bf16\s*\(", text)
    assert re.search(r"#define\s+BNN_HIP_DTYPE_BF16\s+2\b", text)
    assert re.search(r"#define\s+BNN_HIP_FLAG_OUT_F16\s+%d\b" % native.FLAG_OUT_F16, text)
    assert re.search(r"#define\s+BNN_HIP_FLAG_OUT_BF16\s+%d\b" % native.FLAG_OUT_BF16, text)
    assert native.DTYPE_BF16 == 2
    lib = native.require()
    assert lib.bnn_hip_abi_version() == native.ABI_VERSION == 16
    assert "bnn_hip_pack_act_bf16" in native.EXPORTED_SYMBOLS
    assert lib.bnn_hip_pack_act_bf16.argtypes == lib.bnn_hip_pack_act_f16.argtypes


def _desc(flags=0, **kw):
    f = dict(N=2, C=8, H=5, W=5, O=8, KH=3, KW=3, stride_h=1, stride_w=1, pad_h=1, pad_w=1, dil_h=1, dil_w=1, flags=flags)
    f.update(kw)
    return native.ConvDesc(**f)


def test_new_entry_points_refuse_bad_arguments_without_a_gpu():
    lib = native.require()
    launches = native.launch_count()
    f = lib.bnn_hip_pack_act_bf16
    assert f(None, 1, 8, 4, 4, 16, 16, None) == native.ERR_INVALID_ARG
    assert f(16, 1, 8, 4, 4, None, 16, None) == native.ERR_INVALID_ARG
    assert f(16, 1, 8, 4, 4, 16, None, None) == native.ERR_INVALID_ARG
    assert f(17, 1, 8, 4, 4, 16, 16, None) == native.ERR_INVALID_ARG                    # bf16: 2-byte aligned
    assert f(16, 0, 8, 4, 4, 16, 16, None) == native.ERR_INVALID_ARG
    g = lib.bnn_hip_bconv2d_direct
    d = _desc()

    def direct(desc, x=16, dtype=native.DTYPE_BF16, out=16):
        return g(ctypes.byref(desc), x, dtype, 16, 16, 16, None, None, out, None, None)
    assert direct(d, x=None) == native.ERR_INVALID_ARG and direct(d, out=None) == native.ERR_INVALID_ARG
    assert direct(d, x=17) == native.ERR_INVALID_ARG                                    # bf16 input: 2-byte aligned
    assert direct(d, dtype=3) == native.ERR_INVALID_ARG
    assert direct(d, out=18) == native.ERR_INVALID_ARG                                  # an fp32 output: 4-byte aligned
    assert direct(_desc(native.FLAG_OUT_BF16), out=17) == native.ERR_INVALID_ARG        # a 16-bit output: 2-byte aligned
    assert direct(_desc(native.FLAG_OUT_F16 | native.FLAG_OUT_BF16)) == native.ERR_INVALID_ARG     # at most one of them
    h = lib.bnn_hip_blinear_direct
    assert h(4, 8, 8, None, native.DTYPE_BF16, 16, 16, 0, 16, None, None, 16, None, None, None, 0, None) == native.ERR_INVALID_ARG
    assert h(4, 8, 8, 17, native.DTYPE_BF16, 16, 16, 0, 16, None, None, 16, None, None, None, 0, None) == native.ERR_INVALID_ARG
    assert h(4, 8, 8, 16, 3, 16, 16, 0, 16, None, None, 16, None, None, None, 0, None) == native.ERR_INVALID_ARG
    assert native.launch_count() == launches                                           # a refused call launches nothing


@pytest.mark.parametrize("flag", [native.FLAG_OUT_F16, native.FLAG_OUT_BF16])
def test_every_other_conv_entry_point_refuses_the_16_bit_store(flag):
    lib = native.require()
    launches = native.launch_count()
    d = _desc(flag)
    epi = native.Epilogue(alpha=16, out_f32=16)
    plan, route = native.FlyPlan(), native.ConvRoute()
    bad = native.ERR_INVALID_ARG
    assert lib.bnn_hip_bconv2d(ctypes.byref(d), 16, 16, 16, 16, 16, None, None, 16, None) == bad
    assert lib.bnn_hip_bconv2d_dot(ctypes.byref(d), 16, 16, 16, 16, 16, None) == bad
    assert lib.bnn_hip_bconv2d_fused(ctypes.byref(d), 16, 16, 16, 16, ctypes.byref(epi), None) == bad
    assert lib.bnn_hip_bconv2d_grouped(ctypes.byref(d), 1, 16, 16, 16, 16, 16, None, None, 16, None) == bad
    assert lib.bnn_hip_bconv2d_f32(ctypes.byref(d), 16, 16, 16, 16, None, None, 16, 16, None) == bad
    assert lib.bnn_hip_bconv2d_direct_plan(ctypes.byref(d), ctypes.byref(plan)) == bad
    assert lib.bnn_hip_bconv2d_route(ctypes.byref(d), ctypes.byref(epi), ctypes.byref(route)) == bad
    assert lib.bnn_hip_conv_workspace_bytes(ctypes.byref(d)) == 0
    assert native.launch_count() == launches


def test_hipops_refuses_other_output_types():
    with pytest.raises(ValueError):
        hipops.round_lowp(torch.zeros(1, 2, 1, 1), None, torch.float64)
    r = hipops.round_lowp(torch.tensor([[[[1.00390625]], [[70000.0]]]]), torch.tensor([3.0, 1.0]), F16)
    assert r.dtype == F16 and r.flatten().tolist() == [3.01171875, float("inf")]       # round, scale, round; overflow -> inf


# ---- the fixture and the model ---------------------------------------------------------------------------------------
def bits16(a: np.ndarray, name: str) -> np.ndarray:
    """int16 patterns of fp32 values that are representable in the format."""
    a = np.ascontiguousarray(a, np.float32)
    return (a.view(np.uint32) >> 16).astype(np.uint16).view(np.int16) if name == "bf16" else a.astype(np.float16).view(np.int16)


def model(t: dict, name: str) -> np.ndarray:
    """The 16-bit layer as the issue states it: What_D by the layer's hook, alpha = max |What_D[o]|, the integer dot,
    v = fmaf(alpha, dot, bias_D) in fp32, r = D(v), r = D(float(r) * scale)."""
    c = dict(zip(glp.FIELDS, t["meta"].tolist()))
    with torch.no_grad():
        what = XNORWeightBinarizer(compute_alpha=True, center_weights=bool(c["center"]))(torch.from_numpy(t["w"])).numpy()
    what = glp.round_to(what, name)
    alpha = np.abs(what).reshape(c["O"], -1).max(1)
    x = t["x_" + name]
    sx = np.where(np.isnan(x), 0.0, np.sign(x))
    dot = torch.nn.functional.conv2d(torch.from_numpy(sx).double(), torch.from_numpy(np.sign(what)).double(), None,
                                     c["stride"], c["pad"], 1, c["groups"]).numpy()
    bias = glp.round_to(t["b"], name).astype(np.float64) if "b" in t else np.zeros(c["O"])
    v = (alpha.astype(np.float64)[None, :, None, None] * dot + bias[None, :, None, None]).astype(np.float32)
    r = glp.round_to(v, name)
    if "sc" in t:
        with np.errstate(invalid="ignore", over="ignore"):
            r = glp.round_to(r * t["sc"][None, :, None, None], name)
    return r


def cases(fixture):
    n = len({k.split("/")[0] for k in fixture})
    return [{k.split("/", 1)[1]: v for k, v in fixture.items() if k.startswith(f"s{i}/")} for i in range(n)]


@pytest.mark.parametrize("name", ["bf16", "f16"])
def test_two_rounding_model_equals_the_reference_fixture(fixture, name):
    for i, t in enumerate(cases(fixture)):
        want = t["out_" + name]
        r = model(t, name)
        got = bits16(r, name)
        nan = np.isnan(r)
        want_f = (want.view(np.uint16).astype(np.uint32) << 16).view(np.float32) if name == "bf16" else want.view(np.float16)
        assert np.array_equal(nan, np.isnan(want_f)), f"case {i}: NaN positions differ"
        assert np.array_equal(got[~nan], want[~nan]), f"case {i}: {int((got[~nan] != want[~nan]).sum())} patterns differ"


def test_fixture_is_the_generator_s_and_keeps_its_two_conditions(fixture):
    got = cases(fixture)
    assert [tuple(t["meta"].tolist()) for t in got] == [tuple(c) for c in glp.CASES]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "lowp_layers.npz")) < 512 * 1024
    for i, t in enumerate(got):
        c = dict(zip(glp.FIELDS, t["meta"].tolist()))
        assert c["C"] // c["groups"] * c["k"] ** 2 <= glp.MAX_TERMS
        assert max(c["H"], c["W"]) <= 9 and min(c["H"], c["W"]) <= 7 and c["N"] == 2
        ref = glp.case_tensors(i, glp.CASES[i])                      # the inputs are the generator's, value for value
        for k, v in ref.items():
            assert np.array_equal(v, t[k], equal_nan=True), (i, k)
        with torch.no_grad():
            what = XNORWeightBinarizer(compute_alpha=True, center_weights=bool(c["center"]))(torch.from_numpy(t["w"]))
        alpha = what.abs().flatten(1).amax(1).numpy()
        for name in ("bf16", "f16"):
            assert (glp.boundary_distance(alpha, name) > glp.ALPHA_GUARD).all(), (i, name)
            x = t["x_" + name]
            assert np.array_equal(glp.round_to(x, name), x, equal_nan=True)           # already rounded to D
            for s in glp.specials(name):                                                  # every special value is there
                assert (np.isnan(x).any() if np.isnan(s) else ((x == s) & (np.signbit(x) == np.signbit(s))).any()), (i, name, s)

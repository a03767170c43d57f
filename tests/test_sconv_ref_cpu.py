"""The references of the real-weight convolution (tests/sconv_ref.py) pinned on a GPU-less machine, the C-ABI symbols
of csrc/sconv.hip, and the two plan functions of ``fastpath`` with every reason they decline for."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import bnn_amd as bnn
from bnn_amd import fastpath, hipops, native
from bnn_amd.ops import (AdvancedInputBinarizer, BasicInputBinarizer, BasicScaleBinarizer, SignActivation,
                         XNORWeightBinarizer)
from tests import sconv_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64
SYMBOLS = ("bnn_hip_sconv2d_weight_pack_bytes", "bnn_hip_sconv2d_pack_weight_f32", "bnn_hip_sconv2d_f32")


def test_split3_terms_add_up_to_the_weight_bit_for_bit():
    t = R.split_table()
    assert np.isfinite(t).all() and t[1] == F32(1e-45) and t[2].view(np.uint32) == 0x007FFFFF
    hi, mid, lo, kexp = R.split3_ref(t)
    for term in (hi, mid, lo):                     # every term is a bf16 number: the low 16 bits of its fp32 are zero
        assert not (term.view(np.uint32) & np.uint32(0xFFFF)).any()
    # hi + mid + lo == w * 2^kexp (float64 adds three bf16 numbers of one binade range exactly), then the epilogue's
    # exact power-of-two scaling back
    total = np.ldexp(hi.astype(F64) + mid.astype(F64) + lo.astype(F64), -kexp.astype(np.int64)).astype(F32)
    nz = t != 0
    assert np.array_equal(total[nz].view(np.uint32), t[nz].view(np.uint32)), (total, t)
    # (IEEE addition has no sum -0 + 0 + 0 == -0: a zero weight is `hi` with the weight's own bits, and nothing else)
    assert np.array_equal(hi[~nz].view(np.uint32), t[~nz].view(np.uint32)) and not mid[~nz].any() and not lo[~nz].any()
    assert ((np.abs(t) >= 1) | (t == 0) | (kexp > 0)).all() and (kexp[np.abs(t) >= 1] == 0).all()
    scaled = np.abs(np.ldexp(t.astype(F64), kexp.astype(np.int64)))
    assert ((scaled >= 1) & (scaled < 2))[(t != 0) & (np.abs(t) < 1)].all()
    # +-inf and NaN travel in hi
    bad = np.array([np.inf, -np.inf, np.nan], F32)
    assert not np.isfinite(R.split3_ref(bad)[0]).any() and (R.split3_ref(bad)[3] == 0).all()


def test_split3_of_a_row_shares_the_exponent_of_its_largest_weight():
    w = np.array([[2.0 ** -40 * 7, 2.0 ** -60 * 5, 0.0], [3.0, 2.0 ** -90, -1.5], [0.0, 0.0, 0.0],
                  [np.inf, 0.25, np.nan]], F32)
    assert R.row_exp_ref(w).tolist() == [38, 0, 0, 0]
    hi, mid, lo, kexp = R.split3_ref(w, R.row_exp_ref(w))
    back = np.ldexp(hi.astype(F64) + mid + lo, -kexp.astype(np.int64)[:, None])
    assert np.array_equal(back[:3], w[:3].astype(F64))


def test_fragment_layout_reference():
    """Every element of the byte layout, read back through the index formula of include/bnn_hip.h."""
    rng = np.random.default_rng(5)
    for (O, C, k) in ((33, 17, 3), (1, 1, 1), (16, 32, 1), (70, 130, 3)):
        w = (rng.standard_normal((O, C, k, k)) * 2.0 ** rng.integers(-30, 3, (O, 1, 1, 1))).astype(F32)
        w[O // 2] = 0
        raw = R.sconv_fragments_ref(w)
        assert raw.size == R.pack_bytes_ref(O, C, k)
        CB, OS, T = (C + 31) // 32, (O + 15) // 16, k * k
        frag = raw[:CB * T * OS * 3 * 1024].view(np.uint16).reshape(CB, T, OS, 3, 64, 8)
        kexp = raw[CB * T * OS * 3 * 1024:].view(np.int32)
        assert kexp.size == 16 * OS and np.array_equal(kexp[:O], R.row_exp_ref(w)) and not kexp[O:].any()
        terms = R.split3_ref(w, kexp[:O])[:3]
        for _ in range(200):
            cb, tap, os_, term, lane, e = (int(rng.integers(0, n)) for n in (CB, T, OS, 3, 64, 8))
            o, c = 16 * os_ + (lane & 15), 32 * cb + 8 * (lane >> 4) + e
            want = 0 if o >= O or c >= C else int(terms[term][o, c, tap // k, tap % k].view(np.uint32)) >> 16
            assert int(frag[cb, tap, os_, term, lane, e]) == want, (O, C, k, cb, tap, os_, term, lane, e)


CASES = [  # (N, C, O, H, W, k, stride)
    (2, 64, 64, 16, 16, 3, 1), (2, 130, 70, 9, 17, 3, 1), (2, 64, 64, 16, 16, 3, 2), (2, 130, 70, 9, 17, 3, 2),
    (2, 64, 64, 16, 16, 1, 1), (2, 130, 70, 9, 17, 1, 1)]


def random_case(seed, N, C, O, H, W, k):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, C, H, W)).astype(F32)
    w = rng.standard_normal((O, C, k, k)).astype(F32)
    b = rng.standard_normal(O).astype(F32)
    s = (rng.uniform(0.25, 1.0, O) * rng.choice([-1.0, 1.0], O)).astype(F32)     # |scale| <= 1: tests/sconv_ref.py
    return x, w, b, s


@pytest.mark.parametrize("case", CASES, ids=str)
def test_sconv_ref_is_the_float64_composition_and_fp32_torch_stays_inside_the_tolerance(case):
    N, C, O, H, W, k, st = case
    x, w, b, s = random_case(11, N, C, O, H, W, k)
    xt, wt, bt, at = (torch.from_numpy(v) for v in (x, w, b, s))

    def composition(dtype):
        return torch.nn.functional.conv2d(SignActivation.apply(xt.to(dtype)), wt.to(dtype), bt.to(dtype), stride=st,
                                          padding=k // 2) * at.to(dtype).view(1, -1, 1, 1)
    ref = R.sconv_ref(x, w, b, s, st)
    want = composition(torch.float64).numpy()
    assert ref.shape == want.shape == R.out_shape(x.shape, O, st)
    # float64 against float64: two summation orders of <= 1170 terms of magnitude ~1
    assert np.abs(ref - want).max() <= 2.0 ** -40 * max(1.0, np.abs(want).max())
    # the bound is not tighter than the reference's own fp32 arithmetic
    B = R.tolerance(w, ref)
    err = np.abs(composition(torch.float32).numpy().astype(F64) - ref)
    assert (err <= B).all(), float((err / B).max())


def test_sconv_ref_sign_predicate_and_padding():
    x = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1e-45, -1e-45, 0.5, -2.0], F32).reshape(1, 1, 3, 3)
    w = np.zeros((1, 1, 3, 3), F32)
    w[0, 0, 1, 1] = 3.0
    assert R.sconv_ref(x, w)[0, 0].reshape(-1).tolist() == [0, 0, 0, 3, -3, 3, -3, 3, -3]
    ones = np.ones((1, 1, 3, 3), F32)
    assert R.sconv_ref(np.ones((1, 1, 2, 2), F32), ones)[0, 0].tolist() == [[4, 4], [4, 4]]           # zero padding
    assert R.sconv_ref(np.ones((1, 1, 3, 3), F32), ones, stride=2)[0, 0].tolist() == [[4, 4], [4, 4]]


def test_assert_exact_inputs_accepts_dyadic_tables_and_rejects_long_sums():
    rng = np.random.default_rng(2)
    w = rng.integers(-7, 8, (4, 130, 3, 3)).astype(F64) * 2.0 ** -40
    assert R.assert_exact_inputs(w, rng.integers(-7, 8, 4) * 2.0 ** -40) < 2.0 ** 24
    with pytest.raises(AssertionError):
        R.assert_exact_inputs(np.concatenate([w.reshape(4, -1), np.full((4, 1), 2.0 ** -16)], 1).reshape(4, -1, 1, 1))
    with pytest.raises(AssertionError):
        R.assert_exact_inputs(rng.standard_normal((2, 64, 3, 3)).astype(F32))


# ---- the C-ABI -----------------------------------------------------------------------------------------------------
def test_header_exports_and_bindings_agree_on_the_three_symbols():
    text = open(os.path.join(ROOT, "include", "bnn_hip.h")).read()
    assert re.search(r"#define\s+BNN_HIP_ABI_VERSION\s+16\b", text)
    lib = native.require()
    assert lib.bnn_hip_abi_version() == native.ABI_VERSION == 16
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), f"{s} is not declared in include/bnn_hip.h"
        assert hasattr(lib, s), f"{s} is not exported"
        assert getattr(lib, s).argtypes is not None, f"{s} has no binding in native.py"
    assert len(lib.bnn_hip_sconv2d_f32.argtypes) == 13 and len(lib.bnn_hip_sconv2d_pack_weight_f32.argtypes) == 6


def test_entry_point_validators_without_a_gpu():
    lib = native.require()
    for (O, C, k) in ((33, 17, 3), (1, 1, 1), (70, 130, 3), (64, 64, 1)):
        assert lib.bnn_hip_sconv2d_weight_pack_bytes(O, C, k) == R.pack_bytes_ref(O, C, k)
    assert lib.bnn_hip_sconv2d_weight_pack_bytes(0, 8, 3) == 0 and lib.bnn_hip_sconv2d_weight_pack_bytes(8, 8, 5) == 0
    assert lib.bnn_hip_sconv2d_pack_weight_f32(None, 8, 8, 3, 16, None) == native.ERR_INVALID_ARG
    assert lib.bnn_hip_sconv2d_pack_weight_f32(16, 8, 8, 5, 16, None) == native.ERR_UNSUPPORTED
    assert lib.bnn_hip_sconv2d_pack_weight_f32(16, 8, 8, 3, 8, None) == native.ERR_INVALID_ARG      # packed: 16-byte aligned
    f = lib.bnn_hip_sconv2d_f32
    assert f(None, 16, None, None, 16, 1, 8, 8, 8, 8, 3, 1, None) == native.ERR_INVALID_ARG
    assert f(16, 16, None, None, 16, 0, 8, 8, 8, 8, 3, 1, None) == native.ERR_INVALID_ARG
    assert f(16, 8, None, None, 16, 1, 8, 8, 8, 8, 3, 1, None) == native.ERR_INVALID_ARG             # packed alignment
    assert f(16, 16, 2, None, 16, 1, 8, 8, 8, 8, 3, 1, None) == native.ERR_INVALID_ARG               # bias alignment
    for ks, st, W in ((5, 1, 8), (1, 2, 8), (3, 3, 8), (3, 1, 65), (2, 1, 8)):
        assert f(16, 16, None, None, 16, 1, 8, 8, 8, W, ks, st, None) == native.ERR_UNSUPPORTED, (ks, st, W)
    assert f(16, 16, None, None, 16, 1 << 20, 64, 64, 64, 64, 3, 1, None) == native.ERR_TOO_LARGE


def test_sconv_supported_is_grad_supported():
    for xs, ws, st, pd, dl in (((2, 8, 8, 8), (8, 8, 3, 3), 1, 1, 1), ((2, 8, 8, 8), (8, 8, 3, 3), 2, 1, 1),
                               ((2, 8, 8, 8), (8, 8, 1, 1), 1, 0, 1), ((2, 8, 8, 8), (8, 8, 1, 1), 2, 0, 1),
                               ((2, 8, 8, 8), (8, 8, 3, 3), 1, 0, 1), ((2, 8, 8, 8), (8, 8, 5, 5), 1, 2, 1),
                               ((2, 8, 8, 65), (8, 8, 3, 3), 1, 1, 1), ((2, 8, 8, 8), (8, 8, 3, 3), 1, 2, 2),
                               ((2, 8, 8, 64), (8, 8, 3, 3), (2, 2), (1, 1), (1, 1))):
        assert hipops.sconv_supported(xs, ws, st, pd, dl) == hipops.grad_supported(xs, ws, st, pd, dl)
    assert not hipops.sconv_supported((2, 8, 8, 8), (8, 4, 3, 3), 1, 1, 1)          # a grouped weight


# ---- dispatch ------------------------------------------------------------------------------------------------------
STEP0 = dict(activation_pre_process=BasicInputBinarizer, activation_post_process=BasicScaleBinarizer,
             weight_pre_process=nn.Identity)


def layer(cin=8, cout=8, k=3, stride=1, padding=None, dilation=1, groups=1, **hooks):
    conv = nn.Conv2d(cin, cout, k, stride, k // 2 if padding is None else padding, dilation, groups)
    return bnn.layers.Conv2d.from_module(conv, bnn.BConfig(**{**STEP0, **hooks}))


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


def test_recognise_keeps_declining_an_identity_weight_hook():
    for hooks in (dict(), dict(weight_pre_process=bnn.Identity), dict(activation_post_process=bnn.Identity)):
        m = layer(**hooks)
        assert fastpath._recognise(m, 8) is None
        plan = fastpath._recognise_real(m, 8)
        assert isinstance(plan, fastpath.RealPlan) and not isinstance(plan, fastpath.Plan) and plan.ste
        assert (plan.scale is None) == ("activation_post_process" in hooks)
    adv = fastpath._recognise_real(layer(activation_pre_process=AdvancedInputBinarizer), 8)
    assert adv is not None and not adv.ste                                      # tanh: inference only
    assert fastpath._recognise_real(layer(weight_pre_process=XNORWeightBinarizer), 8) is None
    assert fastpath._recognise_real(layer(activation_pre_process=nn.Identity), 8) is None


def test_plans_are_none_with_the_switch_off():
    assert fastpath.REAL_WEIGHTS is False                                       # the default
    m, x = on_fake_device(layer()), FakeCuda((2, 8, 8, 8))
    assert fastpath.plan_conv2d_real(m, x) is None and fastpath.plan_conv2d_real_train(m, x) is None
    assert set(("conv2d_real", "conv2d_real_train")) <= set(fastpath.stats())


def test_plans_admit_the_step0_layer_and_state_each_decline_reason(real_weights, monkeypatch):
    x = FakeCuda((2, 8, 8, 8))
    with torch.no_grad():
        assert isinstance(fastpath.plan_conv2d_real(on_fake_device(layer()), x), fastpath.RealPlan)
        assert fastpath.plan_conv2d_real_train(on_fake_device(layer()), x) is None          # autograd is not recording
    assert fastpath.plan_conv2d_real(on_fake_device(layer()), x) is None                    # the weight needs a gradient
    for geom in (dict(), dict(stride=2), dict(k=1)):
        assert isinstance(fastpath.plan_conv2d_real_train(on_fake_device(layer(**geom)), x), fastpath.RealPlan)
    hooked = layer()
    hooked.weight_pre_process.register_forward_hook(lambda m, i, o: o)
    declines = {
        "XNOR weight hook": (layer(weight_pre_process=XNORWeightBinarizer), x, torch.float32),
        "hooked Identity": (hooked, x, torch.float32),
        "fp16": (layer(), FakeCuda((2, 8, 8, 8), torch.float16), torch.float16),
        "groups 2": (layer(groups=2), x, torch.float32),
        "dilation 2": (layer(dilation=2, padding=2), x, torch.float32),
        "5x5": (layer(k=5), x, torch.float32),
        "strided 1x1": (layer(k=1, stride=2), x, torch.float32),
        "wide rows": (layer(), FakeCuda((2, 8, 8, 65)), torch.float32),
        "CPU tensor": (layer(), torch.zeros(2, 8, 8, 8), torch.float32),
    }
    for why, (m, xin, dtype) in declines.items():
        m = on_fake_device(m, dtype)
        assert fastpath.plan_conv2d_real_train(m, xin) is None, why
        with torch.no_grad():
            assert fastpath.plan_conv2d_real(m, xin) is None, why
    m = on_fake_device(layer())
    with monkeypatch.context() as mp:      # (device autocast cannot be entered without a device: tests/test_gpu_sconv.py does)
        mp.setattr(torch, "is_autocast_enabled", lambda *a: True)
        assert fastpath.plan_conv2d_real_train(m, x) is None, "autocast"
        with torch.no_grad():
            assert fastpath.plan_conv2d_real(m, x) is None, "autocast"
    assert fastpath.plan_conv2d_real_train(m, x) is not None
    adv = on_fake_device(layer(activation_pre_process=AdvancedInputBinarizer))
    assert fastpath.plan_conv2d_real_train(adv, x) is None                                  # tanh STE: composition
    with torch.no_grad():
        assert fastpath.plan_conv2d_real(adv, x) is not None


def test_cpu_forward_is_the_composition_whatever_the_switch(real_weights):
    m = layer()
    x = torch.randn(2, 8, 8, 8)
    before = fastpath.stats()
    want = torch.nn.functional.conv2d(SignActivation.apply(x), m.weight, m.bias, padding=1) * m.activation_post_process.alpha
    assert torch.equal(m(x), want) and fastpath.stats() == before

"""The convolution with binary activations and real weights (csrc/sconv.hip) against tests/sconv_ref.py: bit for bit
where the sums are exact (single-term weights from the split table; dyadic tables), inside the derived tolerance on random
data — and the layer, the cache, the training function and a two-step recipe on top of it.

Every "bit for bit" comparison is on the int32 view.  The shapes are the smallest that reach every path of the kernel:
each slot width (rows of 1 .. 64 output pixels), one and several chunks per image, channel tails on both sides, both
output-channel blockings (O <= 64 and above), stride 2 with even and odd extents, the 1x1 form."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

import bnn_amd as bnn
from bnn_amd import fastpath, hipops, native
from bnn_amd.engine import BinaryChef
from bnn_amd.native import NativeError
from bnn_amd.ops import BasicInputBinarizer, BasicScaleBinarizer, SignActivation
from tests import sconv_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = np.float32, np.float64
ONE_BELOW = np.nextafter(F32(1), F32(0))
X_VALUES = np.array([0.0, -0.0, 0.5, -0.5, 1.0, -1.0, ONE_BELOW, -ONE_BELOW, 2.0, -2.0, np.nan, np.inf, -np.inf, 1e-45,
                     -1e-45], F32)
SHIFTS = (0, -40, 20)


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(DEV)


def dirty(nbytes):
    """The allocator's next block of this size starts as garbage: an element the kernel leaves out is not a lucky 0."""
    torch.empty(int(nbytes), dtype=torch.uint8, device=DEV).fill_(0xAB)


def run(x, w, bias=None, scale=None, stride=1):
    packed = hipops.sconv_pack_weight(dev(w))
    dirty(4 * np.prod(R.out_shape(x.shape, w.shape[0], stride)))
    return hipops.sconv2d(dev(x), packed, dev(bias), dev(scale), stride=stride, padding=w.shape[2] // 2)


def assert_same_bits(got, want64, tag):
    want = np.asarray(want64, F64)
    w32 = want.astype(F32)
    assert (w32.astype(F64) == want).all(), (tag, "the reference is not an fp32 number")
    assert tuple(got.shape) == want.shape, (tag, tuple(got.shape), want.shape)
    if not torch.equal(got.view(torch.int32).cpu(), torch.from_numpy(w32.view(np.int32))):
        g = got.cpu().numpy()
        bad = np.argwhere(g.view(np.uint32) != w32.view(np.uint32))
        first = [(tuple(int(v) for v in i), float(g[tuple(i)]), float(w32[tuple(i)])) for i in bad[:8]]
        raise AssertionError(f"{tag}: {len(bad)} of {g.size} elements differ; (index, got, want): {first}")


# ---- single-term exactness: a dropped or misplaced hi / mid / lo term ------------------------------------------------
@pytest.mark.parametrize("k,stride", [(3, 1), (3, 2), (1, 1)])
def test_one_weight_per_output_channel_comes_out_bit_for_bit(k, stride):
    table = R.split_table()
    table = table[table != 0]
    T, C = k * k, 3
    O = len(table) * T                                   # 180 output channels for the 3x3: both blockings of O
    w = np.zeros((O, C, k, k), F32)
    for o in range(O):
        w[o, o % C, (o % T) // k, (o % T) % k] = table[o // T]      # every table value at every tap position
    rng = np.random.default_rng(1)
    x = np.array([0.5, -0.5, 2.0, -2.0, 1e-45, -1e-45], F32)[rng.integers(0, 6, (2, C, 5, 6))]
    got = run(x, w, stride=stride)
    want = R.sconv_ref(x, w, stride=stride)              # one product per output: exact in any arithmetic
    assert_same_bits(got, want, (k, stride))
    # and the statement itself: y is +w, -w or (zero padding) 0
    mag = np.abs(got.cpu().numpy())
    wmag = np.abs(table)[np.arange(O) // T][None, :, None, None]
    assert (((mag.view(np.uint32) == np.broadcast_to(wmag, mag.shape).view(np.uint32)) | (mag == 0)).all())
    assert (mag != 0).mean() > 0.5


# ---- dyadic tables ---------------------------------------------------------------------------------------------------
S1 = [(1, 1, 1, 1, 1), (5, 15, 31, 11, 8), (1, 17, 33, 5, 9), (1, 33, 70, 4, 16), (5, 130, 1, 3, 17), (1, 15, 70, 5, 32),
      (1, 17, 31, 3, 33), (1, 33, 33, 1, 64), (1, 1, 33, 3, 64), (1, 130, 70, 9, 17)]
S2 = [(1, 3, 5, 1, 1), (5, 17, 33, 1, 2), (1, 15, 31, 2, 1), (1, 33, 70, 15, 15), (1, 17, 33, 16, 16), (5, 15, 1, 17, 17),
      (1, 130, 31, 33, 33), (1, 17, 70, 5, 64), (1, 1, 33, 64, 9)]
P1 = [(1, 1, 1, 1, 1), (5, 15, 31, 9, 8), (1, 17, 33, 3, 9), (1, 130, 70, 5, 17), (1, 33, 70, 2, 33), (1, 15, 1, 3, 64)]
TABLE = [(s, 3, 1) for s in S1] + [(s, 3, 2) for s in S2] + [(s, 1, 1) for s in P1]


def test_the_table_covers_every_slot_width_tail_and_blocking():
    s1 = [s for s, k, st in TABLE if (k, st) == (3, 1)]
    assert {s[4] for s in s1} >= {1, 8, 9, 16, 17, 32, 33, 64} and 1 in {s[3] for s in s1}
    assert {s[0] for s in s1} == {1, 5} and {s[1] for s in s1} == {1, 15, 17, 33, 130} and {s[2] for s in s1} == {1, 31, 33, 70}
    assert (130, 70) in {(s[1], s[2]) for s in s1}
    s2 = {(s[3], s[4]) for s, k, st in TABLE if st == 2}
    assert s2 >= {(1, 1), (1, 2), (2, 1), (15, 15), (16, 16), (17, 17), (33, 33)} and 64 in {w for _, w in s2} | {h for h, _ in s2}
    assert {s[4] for s, k, st in TABLE if k == 1} == {1, 8, 9, 17, 33, 64}
    for (N, C, O, H, W), k, st in TABLE:
        assert hipops.sconv_supported((N, C, H, W), (O, C, k, k), st, k // 2, 1)
    # more than one chunk per image, and a last chunk that is not full
    assert any(k == 3 and st == 1 and W <= 8 and H > 8 and H % 8 for (N, C, O, H, W), k, st in TABLE)


@pytest.mark.parametrize("shape,k,stride", TABLE, ids=str)
def test_dyadic_tables_bit_for_bit(shape, k, stride):
    N, C, O, H, W = shape
    rng = np.random.default_rng(hash((shape, k, stride)) % (1 << 31))
    x = X_VALUES[rng.integers(0, len(X_VALUES), (N, C, H, W))]
    for sh in SHIFTS:
        w = rng.integers(-7, 8, (O, C, k, k)).astype(F32) * F32(2.0 ** sh)      # (zeros among them)
        if O > 1:
            w[O // 2] = 0                                                        # an all-zero output channel
        if C > 1:
            w[:, C // 2] = 0                                                     # an all-zero input channel
        bias = rng.integers(-7, 8, O).astype(F32) * F32(2.0 ** sh)
        scale = np.array([1.0, -2.0, 0.5, 4.0, -0.25], F32)[rng.integers(0, 5, O)]
        assert R.assert_exact_inputs(w, bias) < 2.0 ** 24
        packed = hipops.sconv_pack_weight(dev(w))
        assert np.array_equal(packed.data.cpu().numpy(), R.sconv_fragments_ref(w)), (sh, "weight fragments")
        for b, s in ((None, None), (bias, None), (None, scale), (bias, scale)):
            dirty(4 * np.prod(R.out_shape(x.shape, O, stride)))
            got = hipops.sconv2d(dev(x), packed, dev(b), dev(s), stride=stride, padding=k // 2)
            assert_same_bits(got, R.sconv_ref(x, w, b, s, stride), (sh, b is not None, s is not None))


# ---- the packed weight, byte for byte ----------------------------------------------------------------------------------
def bf16_terms(v):
    """(hi, mid, lo) of fp32 `v` as bf16 bit patterns: each the upper 16 bits of what is left, remainders in fp32."""
    top = lambda a: a.view(np.uint32) & np.uint32(0xFFFF0000)
    with np.errstate(invalid="ignore"):
        hi = top(v)
        r1 = (v - hi.view(F32)).astype(F32)
        mid = top(r1)
        lo = top((r1 - mid.view(F32)).astype(F32))
    return [(t >> np.uint32(16)).astype(np.uint16) for t in (hi, mid, lo)]


def one_nan(bits16):
    """Every bf16 NaN as 0x7FC0: the layout says WHERE a remainder is NaN, not which payload the subtraction gives it."""
    b = bits16.copy()
    b[((b & 0x7F80) == 0x7F80) & ((b & 0x007F) != 0)] = 0x7FC0
    return b


@pytest.mark.parametrize("O,C,k", [(17, 33, 3), (70, 31, 1)])
def test_packed_real_weight_equals_the_documented_layout_byte_for_byte(O, C, k):
    """The header of csrc/sconv.hip: Wp[cb][tap][os][term][lane][e] = term(W[16 os + (lane & 15)][32 cb + 8 (lane >> 4) + e]
    [tap] * 2^kexp[o]) in hi / mid / lo order, zeros for pad channels, kexp[16 OS] behind the fragments — evaluated
    index by index, on rows below 1 (kexp > 0, one of them deep in the range where an unscaled split loses bits), at and
    above 1, all zero, and with one infinity (hi = the infinity, both remainders NaN, kexp 0)."""
    T, CB, OS = k * k, -(-C // 32), -(-O // 16)
    rng = np.random.default_rng(O * 100 + k)
    w = (rng.standard_normal((O, C, k, k)) * 2.0 ** rng.integers(-20, 3, (O, 1, 1, 1))).astype(F32)
    w[0] = (rng.uniform(-1, 1, (C, k, k)) * 0.99).astype(F32)           # largest magnitude below 1
    w[1] = (rng.standard_normal((C, k, k)) * 2.0 ** -120).astype(F32)   # far below 1
    w[2] = rng.uniform(-3, 3, (C, k, k)).astype(F32)
    w[2, 0, 0, 0] = 1.0                                                  # at 1 and above
    w[3] = 0.0
    w[4] = (rng.uniform(-1, 1, (C, k, k)) * 0.5).astype(F32)
    w[4, C - 1, k - 1, k - 1] = -np.inf                                  # finite part below 1, one infinity
    # kexp: 1 - exponent of the row's largest magnitude when that is in (0, 1), else 0
    m = np.abs(w.reshape(O, -1)).max(1)
    kexp = np.zeros(16 * OS, np.int32)
    kexp[:O] = np.where((m > 0) & (m < 1), 1 - np.frexp(m)[1], 0)
    assert kexp[0] >= 1 and kexp[1] > 100 and kexp[2] == 0 and kexp[3] == 0 and kexp[4] == 0
    # the fragment element at every index
    cb, tap, os_, lane, e = np.meshgrid(np.arange(CB), np.arange(T), np.arange(OS), np.arange(64), np.arange(8), indexing="ij")
    o, c = 16 * os_ + (lane & 15), 32 * cb + 8 * (lane >> 4) + e
    live = (o < O) & (c < C)
    wt = w.reshape(O, C, T)
    v = np.where(live, np.ldexp(wt[np.minimum(o, O - 1), np.minimum(c, C - 1), tap], kexp[o]), 0).astype(F32)
    want = np.stack(bf16_terms(v), axis=3)                               # [cb][tap][os][term][lane][e]
    assert want.shape == (CB, T, OS, 3, 64, 8) and not live.all()
    scaled = v[live].astype(F64)
    fin = np.isfinite(scaled)
    terms = [t[live][fin].astype(np.uint32) << np.uint32(16) for t in bf16_terms(v)]
    assert (sum(t.view(F32).astype(F64) for t in terms) == scaled[fin]).all()    # the split loses nothing here
    got = hipops.sconv_pack_weight(dev(w)).data.cpu().numpy()
    assert got.dtype == np.uint8 and got.size == want.size * 2 + 16 * OS * 4 == R.pack_bytes_ref(O, C, k)
    frag = got[:want.size * 2].view(np.uint16).reshape(want.shape)
    inf_at = (o == 4) & (c == C - 1) & (tap == T - 1)
    assert inf_at.sum() == 1 and (frag[:, :, :, 0][inf_at] == 0xFF80).all()
    for t in (1, 2):
        r = frag[:, :, :, t][inf_at]
        assert ((r & 0x7F80) == 0x7F80).all() and ((r & 0x007F) != 0).all()
    assert np.array_equal(one_nan(frag), one_nan(want))
    assert np.array_equal(got[want.size * 2:].view(np.int32), kexp)


# ---- random data -----------------------------------------------------------------------------------------------------
RANDOM = [(2, 64, 64, 16, 16, 3, 1), (2, 130, 70, 9, 17, 3, 1), (2, 64, 64, 16, 16, 3, 2), (2, 130, 70, 9, 17, 3, 2),
          (2, 64, 64, 16, 16, 1, 1), (2, 130, 70, 9, 17, 1, 1)]


@pytest.mark.parametrize("case", RANDOM, ids=str)
def test_random_cases_stay_inside_the_tolerance_on_every_element(case):
    N, C, O, H, W, k, st = case
    rng = np.random.default_rng(3)
    x = rng.standard_normal((N, C, H, W)).astype(F32)
    w = rng.standard_normal((O, C, k, k)).astype(F32)
    b = rng.standard_normal(O).astype(F32)
    s = (rng.uniform(0.25, 1.0, O) * rng.choice([-1.0, 1.0], O)).astype(F32)
    for bias, scale in ((None, None), (b, s)):
        ref = R.sconv_ref(x, w, bias, scale, st)
        B = R.tolerance(w, ref)
        err = np.abs(run(x, w, bias, scale, st).cpu().numpy().astype(F64) - ref)
        print(case, bias is not None, "max err / B =", float((err / B).max()), "max err =", float(err.max()))
        assert (err <= B).all()


def test_non_finite_weights_reach_every_output_the_reference_marks():
    rng = np.random.default_rng(4)
    x = rng.standard_normal((2, 33, 9, 9)).astype(F32)
    x[0, 5] = 0                                          # 0 * inf: NaN in the reference and on the matrix cores
    w = rng.standard_normal((40, 33, 3, 3)).astype(F32)
    w[3, 5, 1, 1], w[7, 0, 0, 2], w[20, 32, 2, 0], w[21, 1, 1, 1] = np.inf, -np.inf, np.nan, np.inf
    w[21, 2, 1, 1] = -np.inf
    got = run(x, w).cpu().numpy()
    ref = R.sconv_ref(x, w)
    assert (~np.isfinite(ref)).any() and (~np.isfinite(got))[~np.isfinite(ref)].all()
    clean = np.ones(40, bool)
    clean[[3, 7, 20, 21]] = False
    assert np.isfinite(got[:, clean]).all()              # and it does not spread to other output channels


def test_unsupported_geometries_are_refused_by_the_entry_point():
    lib = native.require()
    x = torch.zeros(1 << 16, device=DEV)
    y, packed = torch.zeros(1 << 16, device=DEV), torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    launches = native.launch_count()

    def call(N, O, C, H, W, k, st):
        return lib.bnn_hip_sconv2d_f32(x.data_ptr(), packed.data_ptr(), None, None, y.data_ptr(), N, O, C, H, W, k, st, None)
    for what, args in {"5x5": (1, 8, 8, 8, 8, 5, 1), "strided 1x1": (1, 8, 8, 8, 8, 1, 2), "stride 3": (1, 8, 8, 8, 8, 3, 3),
                       "2x2": (1, 8, 8, 8, 8, 2, 1), "rows of 65": (1, 8, 8, 2, 65, 3, 1)}.items():
        assert call(*args) == native.ERR_UNSUPPORTED, what
    assert lib.bnn_hip_sconv2d_pack_weight_f32(x.data_ptr(), 8, 8, 5, packed.data_ptr(), None) == native.ERR_UNSUPPORTED
    assert native.launch_count() == launches
    pk = hipops.sconv_pack_weight(torch.zeros(8, 8, 3, 3, device=DEV))
    with pytest.raises(NativeError):
        hipops.sconv2d(torch.zeros(1, 8, 8, 65, device=DEV), pk)
    with pytest.raises(NativeError):
        hipops.sconv2d(torch.zeros(1, 8, 8, 8, device=DEV), pk, stride=1, padding=0)
    with pytest.raises(NativeError):
        hipops.sconv_pack_weight(torch.zeros(8, 8, 5, 5, device=DEV))


# ---- the layer -------------------------------------------------------------------------------------------------------
STEP0 = bnn.BConfig(activation_pre_process=BasicInputBinarizer, activation_post_process=BasicScaleBinarizer,
                    weight_pre_process=nn.Identity)


@pytest.fixture
def switch():
    old = fastpath.REAL_WEIGHTS

    def turn(on):
        fastpath.REAL_WEIGHTS = bool(on)
    yield turn
    fastpath.REAL_WEIGHTS = old


def step0_layer(C, O, k, stride, seed):
    torch.manual_seed(seed)
    m = bnn.layers.Conv2d.from_module(nn.Conv2d(C, O, k, stride, k // 2), copy.deepcopy(STEP0)).to(DEV)
    with torch.no_grad():
        m.activation_post_process.alpha.uniform_(0.25, 1.0)
    return m


def composition(m, x):
    out = torch.nn.functional.conv2d(SignActivation.apply(x), m.weight, m.bias, m.stride, m.padding)
    return out * m.activation_post_process.alpha


def layer_ref(m, x):
    return R.sconv_ref(x.detach().cpu().numpy(), m.weight.detach().cpu().numpy(), m.bias.detach().cpu().numpy(),
                       m.activation_post_process.alpha.detach().cpu().numpy().reshape(-1), m.stride[0])


def delta(before, key):
    return fastpath.stats()[key] - before[key]


LAYERS = [(17, 33, 3, 1), (17, 70, 3, 2), (33, 31, 1, 1)]


@pytest.mark.parametrize("C,O,k,stride", LAYERS)
def test_layer_inference_switch_counter_and_cache(C, O, k, stride, switch, monkeypatch):
    m = step0_layer(C, O, k, stride, 0).eval()
    x = torch.randn(3, C, 9, 10, device=DEV)
    with torch.no_grad():
        switch(False)
        before = fastpath.stats()
        off = m(x)
        assert fastpath.stats() == before and torch.equal(off, composition(m, x))
        switch(True)
        on = m(x)
        assert delta(before, "conv2d_real") == 1 and delta(before, "weight_packs") == 1
        ref = layer_ref(m, x)
        assert (np.abs(on.cpu().numpy().astype(F64) - ref) <= R.tolerance(m.weight.detach().cpu().numpy(), ref)).all()
        # the cache: a second call does not re-pack; an in-place optimiser step, invalidate() and train() / eval() do
        assert torch.equal(m(x), on) and delta(before, "weight_packs") == 1 and delta(before, "conv2d_real") == 2
        m.weight.mul_(0.5)                                       # (bumps the version counter, as optimizer.step() does)
        half = m(x)
        assert delta(before, "weight_packs") == 2
        ref = layer_ref(m, x)
        assert (np.abs(half.cpu().numpy().astype(F64) - ref) <= R.tolerance(m.weight.detach().cpu().numpy(), ref)).all()
        m(x)
        assert delta(before, "weight_packs") == 2
        assert fastpath.invalidate(m) == 1
        m(x)
        assert delta(before, "weight_packs") == 3
        m.train().eval()
        m(x)
        assert delta(before, "weight_packs") == 4
        monkeypatch.setenv("BNN_AMD_STRICT_WEIGHTS", "1")        # never trusted
        m(x), m(x)
        assert delta(before, "weight_packs") == 6
        monkeypatch.delenv("BNN_AMD_STRICT_WEIGHTS")
        # declines at run time: autocast, fp16
        before = fastpath.stats()
        with torch.autocast("cuda", dtype=torch.float16):
            m(x)
        m.half()(x.half())
        assert fastpath.stats() == before


@pytest.mark.parametrize("C,O,k,stride", LAYERS)
def test_layer_training_step_gradients(C, O, k, stride, switch):
    m = step0_layer(C, O, k, stride, 1).train()
    torch.manual_seed(2)
    x = (torch.randn(3, C, 9, 10, device=DEV) * 1.2).requires_grad_()
    switch(True)
    before = fastpath.stats()
    out = m(x)
    assert delta(before, "conv2d_real_train") == 1 and delta(before, "conv2d_real") == 0
    g = torch.randn_like(out)
    out.backward(g)
    W64, x64 = m.weight.detach().double().cpu(), x.detach().double().cpu()
    alpha64 = m.activation_post_process.alpha.detach().double().cpu()
    g64 = g.double().cpu()
    gc = (g * m.activation_post_process.alpha).detach()                  # the gradient that reaches the convolution
    gc64 = gc.double().cpu()
    # gW: the weight-gradient kernel's own result, bit for bit
    want_gw = hipops.bconv_grad_weight(gc.contiguous(), x.detach(), k, stride, reduce=True)
    assert torch.equal(m.weight.grad.view(torch.int32), want_gw.view(torch.int32))
    # gx: float64 reference, bound (O k^2 + 1) 2^-23 sum_{o,tap} |g| |W|; exactly 0 where |x| >= 1
    shape = tuple(x.shape)
    gx64 = torch.nn.grad.conv2d_input(shape, W64, gc64, stride, k // 2).masked_fill(x64.abs() >= 1, 0)
    bound = (O * k * k + 1) * 2.0 ** -23 * torch.nn.grad.conv2d_input(shape, W64.abs(), gc.abs().double().cpu(), stride, k // 2)
    gx = x.grad.double().cpu()
    assert ((gx - gx64).abs() <= bound).all(), float(((gx - gx64).abs() / bound.clamp_min(1e-300)).max())
    outside = x64.abs() >= 1
    assert outside.any() and (x.grad.cpu()[outside].view(torch.int32) == 0).all() and (gx[~outside] != 0).any()
    # gb and d scale: fp32 sums of n terms, n 2^-23 sum |terms| (any order, truncating adders allowed for)
    n = g64.numel() // O
    gb64, gb_abs = gc64.sum((0, 2, 3)), gc64.abs().sum((0, 2, 3))
    assert ((m.bias.grad.double().cpu() - gb64).abs() <= n * 2.0 ** -23 * gb_abs).all()
    conv64 = torch.from_numpy(R.sconv_ref(x.detach().cpu().numpy(), W64.numpy(), m.bias.detach().double().cpu().numpy(),
                                          None, stride))
    conv_err = torch.from_numpy(R.tolerance(W64.numpy(), conv64.numpy()))  # of the fp32 forward the product is taken with
    da64 = (g64 * conv64).sum((0, 2, 3))
    da_bound = (g64.abs() * conv_err).sum((0, 2, 3)) + (n + 1) * 2.0 ** -23 * (g64 * conv64).abs().sum((0, 2, 3))
    assert ((m.activation_post_process.alpha.grad.double().cpu().reshape(-1) - da64).abs() <= da_bound).all()
    assert alpha64.numel() == O
    # switch off: the composition, no counter
    switch(False)
    before = fastpath.stats()
    m(x)
    assert fastpath.stats() == before


# ---- the two-step recipe ---------------------------------------------------------------------------------------------
RECIPE = """
step0:
  pre_activation:
    name: "BasicInputBinarizer"
  post_activation:
    name: "BasicScaleBinarizer"
  weight:
    name: "nn.Identity"
  ignore_layer_names:
    - "_last_"
    - "_first_"
step1:
  pre_activation:
    name: "BasicInputBinarizer"
  post_activation:
    name: "BasicScaleBinarizer"
  weight:
    name: "XNORWeightBinarizer"
    args:
      compute_alpha: False
      center_weights: False
  ignore_layer_names:
    - "_last_"
    - "_first_"
"""


class PreBlock(nn.Module):
    """Pre-activation block of examples/imagenet.py in small: BN -> 3x3 conv -> PReLU, twice, shortcut added to each."""

    def __init__(self, cin, cout, stride):
        super().__init__()
        self.bn1, self.conv1, self.act1 = nn.BatchNorm2d(cin), nn.Conv2d(cin, cout, 3, stride, 1, bias=False), nn.PReLU(cout)
        self.bn2, self.conv2, self.act2 = nn.BatchNorm2d(cout), nn.Conv2d(cout, cout, 3, 1, 1, bias=False), nn.PReLU(cout)
        self.down = None
        if stride != 1 or cin != cout:
            self.down = nn.Sequential(nn.AvgPool2d(2, 2), nn.Conv2d(cin, cout, 1, bias=False), nn.BatchNorm2d(cout))

    def forward(self, x):
        y = self.act1(self.conv1(self.bn1(x))) + (x if self.down is None else self.down(x))
        return self.act2(self.conv2(self.bn2(y))) + y


def small_resnet():
    return nn.Sequential(nn.Conv2d(3, 16, 3, 1, 1, bias=False), nn.BatchNorm2d(16), PreBlock(16, 16, 1), PreBlock(16, 32, 2),
                         nn.BatchNorm2d(32), nn.AdaptiveAvgPool2d(1), nn.Flatten(), nn.Linear(32, 10))


def sgd_losses(model, steps=3):
    model = copy.deepcopy(model).train()
    opt = torch.optim.SGD(model.parameters(), lr=0.05, momentum=0.9)
    gen = torch.Generator(device="cpu").manual_seed(7)
    losses = []
    for _ in range(steps):
        x = torch.randn(8, 3, 16, 16, generator=gen).to(DEV)
        t = torch.randint(0, 10, (8,), generator=gen).to(DEV)
        opt.zero_grad(set_to_none=True)
        loss = torch.nn.functional.cross_entropy(model(x), t)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses, model


def test_two_step_recipe_trains_step0_on_the_real_weight_path(tmp_path, switch):
    recipe = tmp_path / "two_steps.yaml"
    recipe.write_text(RECIPE)
    chef = BinaryChef(str(recipe))
    torch.manual_seed(0)
    model = chef.next(small_resnet()).to(DEV)                              # step 0
    converted = [m for m in model.modules() if isinstance(m, bnn.layers.Conv2d)]
    k3 = [m for m in converted if m.kernel_size == (3, 3)]
    assert len(k3) == 4 and len(converted) == 5 and all(isinstance(m.weight_pre_process, nn.Identity) for m in converted)
    switch(False)
    before = fastpath.stats()
    off, _ = sgd_losses(model)
    assert fastpath.stats() == before
    switch(True)
    on, trained = sgd_losses(model)
    assert delta(before, "conv2d_real_train") == 3 * len(converted) and delta(before, "conv2d_train") == 0
    rel = [abs(a - b) / abs(b) for a, b in zip(on, off)]
    print("losses, switch off:", off, "on:", on, "relative difference:", rel)
    assert max(rel) <= 1e-4
    # step 1: XNOR weights take the existing training path, the real-weight counters stand still
    model1 = chef.next(trained)
    before = fastpath.stats()
    sgd_losses(model1, steps=1)
    assert delta(before, "conv2d_train") == len(converted)
    assert delta(before, "conv2d_real_train") == 0 and delta(before, "conv2d_real") == 0

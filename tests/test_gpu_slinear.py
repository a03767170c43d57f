"""The Linear with binary activations and real weights (csrc/slinear.hip) against tests/sconv_ref.py on
``x.reshape(M, F, 1, 1)`` / ``w.reshape(O, F, 1, 1)``: bit for bit where the sums are exact (single-term weights from the
split table; dyadic tables), inside the derived tolerance on random data — its bit planes against ``pack_act_ste``, the
mask kernel, and the layer, the cache, the training function and a two-step recipe on top of it.

Every "bit for bit" comparison is on the int32 view.  The kernel's tiling: 64 rows per workgroup; 64 output channels per
workgroup up to O = 64 and 128 above (``BLOCKINGS``); K blocks of 64 features (one plane word), each two k-steps of 32 of
which the second is missing when ``F % 64`` lies in 1 .. 32; MFMA fragments of 16 rows x 16 channels x 8 features per
lane group.  The shapes are the smallest that reach every one of those paths and their tails, combined."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

import bnn_amd as bnn
from bnn_amd import fastpath, hipops, native, training
from bnn_amd.engine import BinaryChef
from bnn_amd.native import NativeError
from bnn_amd.ops import BasicInputBinarizer, BasicScaleBinarizer, SignActivation
from tests import sconv_ref as R
from tests import test_gpu_sconv as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = np.float32, np.float64
dev, dirty, assert_same_bits = S.dev, S.dirty, S.assert_same_bits


def ref(x, w, bias=None, scale=None):
    """float64 reference [M, O] of the layer."""
    M, F = x.shape
    return R.sconv_ref(x.reshape(M, F, 1, 1), w.reshape(len(w), F, 1, 1), bias, scale)[:, :, 0, 0]


def tol(w, y64):
    return R.tolerance(w.reshape(w.shape[0], w.shape[1], 1, 1), y64[:, :, None, None])[:, :, 0, 0]


def run(x, w, bias=None, scale=None, want_planes=False):
    packed = hipops.slinear_pack_weight(dev(w))
    dirty(4 * x.shape[0] * w.shape[0])
    return hipops.slinear(dev(x), packed, dev(bias), dev(scale), want_planes=want_planes)


# ---- single-term exactness: a dropped or misplaced hi / mid / lo term, a wrong kexp ------------------------------------
def test_one_weight_per_output_channel_comes_out_bit_for_bit():
    table = R.split_table()
    table = table[table != 0]
    F, REP = 70, 7                                       # every value at 7 feature positions: 126 channels, one blocking
    O = len(table) * REP                                 # ... and 140 with the pad below: the other
    w = np.zeros((O + 14, F), F32)
    for o in range(O):
        w[o, (11 * o + 3) % F] = table[o // REP]         # varying f: both k-steps, every lane group, the tail block
    for o in range(O, O + 14):
        w[o, (5 * o) % F] = table[o % len(table)]
    rng = np.random.default_rng(1)
    x = np.array([0.5, -0.5, 2.0, -2.0, 1e-45, -1e-45], F32)[rng.integers(0, 6, (37, F))]
    for rows in (w, w[:60]):                             # O = 140 (128 channels per workgroup) and O = 60 (64)
        got = run(x, rows)
        assert_same_bits(got, ref(x, rows), len(rows))   # one product per output: exact in any arithmetic
        mag = np.abs(got.cpu().numpy())
        wmag = np.abs(rows).max(1)[None, :]
        assert (mag.view(np.uint32) == np.broadcast_to(wmag, mag.shape).view(np.uint32)).all()   # y is +w or -w


# ---- dyadic tables ---------------------------------------------------------------------------------------------------
TABLE = [(1, 1, 1), (15, 7, 15), (16, 8, 16), (17, 9, 17), (63, 31, 64), (64, 32, 65), (65, 33, 70), (130, 63, 130),
         (1, 64, 257), (17, 65, 1), (130, 130, 70), (65, 130, 130), (64, 96, 129)]
BLOCKINGS = {64, 128}                                    # output channels per workgroup the launcher can choose


def block_channels(O):
    return 128 if O > 64 else 64                         # launch_slinear's rule (csrc/slinear.hip)


def test_the_table_covers_every_tail_and_blocking():
    assert {s[0] for s in TABLE} >= {1, 15, 16, 17, 63, 64, 65, 130}
    assert {s[1] for s in TABLE} >= {1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 130}
    assert {s[2] for s in TABLE} >= {1, 15, 16, 17, 64, 65, 70, 130} and max(s[2] for s in TABLE) > max(BLOCKINGS)
    assert {block_channels(s[2]) for s in TABLE} == BLOCKINGS
    assert any(M > 64 and -(-O // block_channels(O)) > 1 for M, F, O in TABLE)         # several tiles on both grid axes
    assert any(-(-O // block_channels(O)) >= 3 for M, F, O in TABLE)
    # K blocks: one and several; a last block with one k-step (F % 64 in 1 .. 32) and with two, full and not
    assert {(F + 63) // 64 for _, F, _ in TABLE} >= {1, 2, 3}
    assert any(0 < F % 64 <= 32 and F > 64 for _, F, _ in TABLE) and any(F % 64 > 32 for _, F, _ in TABLE)
    assert any(F % 64 == 0 for _, F, _ in TABLE) and any(F % 64 == 32 and F > 64 for _, F, _ in TABLE)
    assert any(F % 2 == 1 and M > 1 for M, F, _ in TABLE)                              # rows that are only 4-byte aligned
    # the tails are combined: a case with a tail on all three axes at once, in both blockings
    for bc in BLOCKINGS:
        assert any(M % 64 and F % 32 and O % 16 and block_channels(O) == bc for M, F, O in TABLE)


def dyadic_case(shape):
    M, F, O = shape
    rng = np.random.default_rng(hash(shape) % (1 << 31))
    x = S.X_VALUES[rng.integers(0, len(S.X_VALUES), (M, F))]
    for sh in S.SHIFTS:
        w = rng.integers(-7, 8, (O, F)).astype(F32) * F32(2.0 ** sh)            # (zeros among them)
        if O > 1:
            w[O // 2] = 0                                                        # an all-zero output row
        if F > 1:
            w[:, F // 2] = 0                                                     # an all-zero feature
        bias = rng.integers(-7, 8, O).astype(F32) * F32(2.0 ** sh)
        scale = np.array([1.0, -2.0, 0.5, 4.0, -0.25], F32)[rng.integers(0, 5, O)]
        yield sh, x, w, bias, scale


@pytest.mark.parametrize("shape", TABLE, ids=str)
def test_dyadic_tables_bit_for_bit(shape):
    M, F, O = shape
    for sh, x, w, bias, scale in dyadic_case(shape):
        assert R.assert_exact_inputs(w.reshape(O, F, 1, 1), bias) < 2.0 ** 24
        packed = hipops.slinear_pack_weight(dev(w))
        assert packed.shape == (O, F, 1, 1)
        assert np.array_equal(packed.data.cpu().numpy(), R.sconv_fragments_ref(w.reshape(O, F, 1, 1))), (sh, "fragments")
        for b, s in ((None, None), (bias, None), (None, scale), (bias, scale)):
            dirty(4 * M * O)
            got = hipops.slinear(dev(x), packed, dev(b), dev(s))
            assert_same_bits(got, ref(x, w, b, s), (sh, b is not None, s is not None))


# ---- planes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", TABLE, ids=str)
def test_planes_are_those_of_pack_act_ste_and_leave_the_output_alone(shape):
    M, F, O = shape
    sh, x, w, bias, scale = next(dyadic_case(shape))
    want = hipops.pack_act_ste(dev(x).view(M, F, 1, 1))
    plain = run(x, w, bias, scale)
    dirty(3 * 8 * M * ((F + 63) // 64))
    got, sv = run(x, w, bias, scale, want_planes=True)
    assert torch.equal(got.view(torch.int32), plain.view(torch.int32))
    assert tuple(sv.shape) == (M, F, 1, 1) and sv.nbytes() == 3 * 8 * M * ((F + 63) // 64)
    for name, a, b in (("P", sv.sign.P, want.sign.P), ("Mn", sv.sign.M, want.sign.M), ("T", sv.T, want.T)):
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), name
    live = F - 64 * ((F - 1) // 64)                                            # pad bits of the last word, stated
    if live < 64:
        for t in (sv.sign.P, sv.sign.M, sv.T):
            assert not (t.reshape(M, -1)[:, -1].cpu().numpy().view(np.uint64) >> np.uint64(live)).any()


# ---- random data -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(130, 130, 70), (64, 256, 64)], ids=str)
def test_random_cases_stay_inside_the_tolerance_on_every_element(shape):
    M, F, O = shape
    rng = np.random.default_rng(3)
    x = rng.standard_normal((M, F)).astype(F32)
    w = rng.standard_normal((O, F)).astype(F32)
    b = rng.standard_normal(O).astype(F32)
    s = (rng.uniform(0.25, 1.0, O) * rng.choice([-1.0, 1.0], O)).astype(F32)
    for bias, scale in ((None, None), (b, s)):
        want = ref(x, w, bias, scale)
        B = tol(w, want)
        err = np.abs(run(x, w, bias, scale).cpu().numpy().astype(F64) - want)
        print(shape, bias is not None, "max err / B =", float((err / B).max()), "max err =", float(err.max()))
        assert (err <= B).all()


def test_non_finite_weights_reach_every_output_the_reference_marks():
    rng = np.random.default_rng(4)
    x = rng.standard_normal((70, 33)).astype(F32)
    x[:, 5] = 0                                          # 0 * inf: NaN in the reference and on the matrix cores
    w = rng.standard_normal((40, 33)).astype(F32)
    w[3, 5], w[7, 0], w[20, 32], w[21, 1] = np.inf, -np.inf, np.nan, np.inf
    w[21, 2] = -np.inf
    got = run(x, w).cpu().numpy()
    want = ref(x, w)
    assert (~np.isfinite(want)).any() and (~np.isfinite(got))[~np.isfinite(want)].all()
    clean = np.ones(40, bool)
    clean[[3, 7, 20, 21]] = False
    assert np.isfinite(got[:, clean]).all()              # and it does not spread to other output channels


def test_refusals_launch_nothing():
    lib = native.require()
    x, y = torch.zeros(1 << 12, device=DEV), torch.zeros(1 << 12, device=DEV)
    packed = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    pl = torch.zeros(1 << 10, dtype=torch.int64, device=DEV)
    launches = native.launch_count()

    def call(M, F, O, P=None, Mn=None, T=None):
        return lib.bnn_hip_slinear_f32(M, F, O, x.data_ptr(), packed.data_ptr(), None, None, y.data_ptr(), P, Mn, T, None)
    for M, F, O in ((0, 8, 8), (8, 0, 8), (8, 8, 0), (-1, 8, 8), (8, -8, 8), (8, 8, -8)):
        assert call(M, F, O) == native.ERR_INVALID_ARG, (M, F, O)
    p = pl.data_ptr()
    for planes in ((p, None, None), (p, p, None), (None, p, p), (None, None, p), (p, None, p)):
        assert call(8, 8, 8, *planes) == native.ERR_INVALID_ARG, planes
    assert call(1 << 15, 1 << 15, 8) == native.ERR_TOO_LARGE                     # M * F = 2^30
    assert lib.bnn_hip_ste_mask_f32(y.data_ptr(), p, 0, 8, None) == native.ERR_INVALID_ARG
    assert lib.bnn_hip_ste_mask_f32(y.data_ptr(), p, 1 << 15, 1 << 15, None) == native.ERR_TOO_LARGE
    assert native.launch_count() == launches
    pk = hipops.slinear_pack_weight(torch.zeros(8, 16, device=DEV))
    launches = native.launch_count()
    with pytest.raises(NativeError):
        hipops.slinear(torch.zeros(4, 16, device=DEV).half(), pk)
    with pytest.raises(NativeError):
        hipops.slinear(torch.zeros(4, 16), pk)                                   # not on the device
    with pytest.raises(NativeError):
        hipops.slinear(torch.zeros(4, 8, device=DEV), pk)                        # another F
    with pytest.raises(NativeError):
        hipops.slinear(torch.zeros(4, 16, device=DEV), hipops.sconv_pack_weight(torch.zeros(8, 16, 3, 3, device=DEV)))
    with pytest.raises(NativeError):
        hipops.slinear_pack_weight(torch.zeros(8, 16, 1, 1, device=DEV))
    assert native.launch_count() == launches + 2                                 # (the 3x3 pack's two launches only)


# ---- the mask kernel -------------------------------------------------------------------------------------------------
def test_ste_mask_zeroes_exactly_the_masked_elements():
    M, F = 65, 130
    rng = np.random.default_rng(5)
    x = S.X_VALUES[rng.integers(0, len(S.X_VALUES), (M, F))]
    x[::3] = rng.standard_normal((len(x[::3]), F)).astype(F32)
    g = rng.standard_normal((M, F)).astype(F32)
    g[rng.integers(0, M, 40), rng.integers(0, F, 40)] = np.nan
    g[rng.integers(0, M, 40), rng.integers(0, F, 40)] = np.inf
    g[rng.integers(0, M, 40), rng.integers(0, F, 40)] = -np.inf
    g[0, 0], g[M - 1, F - 1], x[0, 0], x[M - 1, F - 1] = np.nan, -np.inf, 2.0, np.nan   # masked, at both ends
    saved = hipops.pack_act_ste(dev(x).view(M, F, 1, 1))
    gx = dev(g)
    assert hipops.ste_mask_(gx, saved) is gx
    with np.errstate(invalid="ignore"):
        keep = np.abs(x) < 1
    assert keep.any() and (~keep).any() and not np.isfinite(g[~keep]).all() and not np.isfinite(g[keep]).all()
    got = gx.cpu().numpy().view(np.int32)
    assert (got[~keep] == 0).all()                                               # +0.0, whatever was there
    assert (got[keep] == g.view(np.int32)[keep]).all()
    with pytest.raises(NativeError):
        hipops.ste_mask_(torch.zeros(M, F + 1, device=DEV), saved)
    with pytest.raises(NativeError):
        hipops.ste_mask_(torch.zeros(F, M, device=DEV).t(), saved)               # not contiguous


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


def step0_layer(F, O, bias, seed):
    torch.manual_seed(seed)
    m = bnn.layers.Linear.from_module(nn.Linear(F, O, bias), copy.deepcopy(STEP0)).to(DEV)
    with torch.no_grad():
        m.activation_post_process.alpha.uniform_(0.25, 1.0)
    return m


def composition(m, x):
    return torch.nn.functional.linear(SignActivation.apply(x), m.weight, m.bias) * m.activation_post_process.alpha


def np64(t):
    return None if t is None else t.detach().double().cpu().numpy()


def layer_ref(m, x):
    F = m.in_features
    y = ref(x.detach().cpu().numpy().reshape(-1, F), m.weight.detach().cpu().numpy(), np64(m.bias),
            np64(m.activation_post_process.alpha).reshape(-1))
    return y.reshape(*x.shape[:-1], m.out_features)


def layer_tol(m, y64):
    O = m.out_features
    return tol(m.weight.detach().cpu().numpy(), y64.reshape(-1, O)).reshape(y64.shape)


def delta(before, key):
    return fastpath.stats()[key] - before[key]


def inputs(F, seed):
    torch.manual_seed(seed)
    return [torch.randn(3, 5, F, device=DEV), torch.randn(5, F, 3, device=DEV).permute(2, 0, 1)]


LAYERS = [(33, 70, True), (130, 17, False)]


@pytest.mark.parametrize("F,O,bias", LAYERS)
def test_layer_inference_switch_counter_and_cache(F, O, bias, switch, monkeypatch):
    m = step0_layer(F, O, bias, 0).eval()
    x, xt = inputs(F, 1)
    assert not xt.is_contiguous() and xt.shape == x.shape
    with torch.no_grad():
        switch(False)
        before = fastpath.stats()
        off = m(x)
        assert fastpath.stats() == before and torch.equal(off, composition(m, x))
        switch(True)
        on = m(x)
        assert delta(before, "linear_real") == 1 and delta(before, "weight_packs") == 1 and on.shape == (3, 5, O)
        want = layer_ref(m, x)
        assert (np.abs(on.cpu().numpy().astype(F64) - want) <= layer_tol(m, want)).all()
        ont = m(xt)                                              # a non-contiguous view: made contiguous, the same rows
        assert torch.equal(ont, m(xt.contiguous())) and delta(before, "linear_real") == 3
        want = layer_ref(m, xt)
        assert (np.abs(ont.cpu().numpy().astype(F64) - want) <= layer_tol(m, want)).all()
        before = fastpath.stats()
        # the cache: a second call does not re-pack; an in-place optimiser step, invalidate() and train() / eval() do
        assert torch.equal(m(x), on) and delta(before, "weight_packs") == 0 and delta(before, "linear_real") == 1
        m.weight.mul_(0.5)                                       # (bumps the version counter, as optimizer.step() does)
        half = m(x)
        assert delta(before, "weight_packs") == 1
        want = layer_ref(m, x)
        assert (np.abs(half.cpu().numpy().astype(F64) - want) <= layer_tol(m, want)).all()
        m(x)
        assert delta(before, "weight_packs") == 1
        assert fastpath.invalidate(m) == 1
        m(x)
        assert delta(before, "weight_packs") == 2
        m.train().eval()
        m(x)
        assert delta(before, "weight_packs") == 3
        monkeypatch.setenv("BNN_AMD_STRICT_WEIGHTS", "1")        # never trusted
        m(x), m(x)
        assert delta(before, "weight_packs") == 5
        monkeypatch.delenv("BNN_AMD_STRICT_WEIGHTS")
        # declines at run time: autocast, fp16
        before = fastpath.stats()
        with torch.autocast("cuda", dtype=torch.float16):
            m(x)
        m.half()(x.half())
        assert fastpath.stats() == before


@pytest.mark.parametrize("F,O,bias", LAYERS)
def test_layer_training_step_gradients(F, O, bias, switch):
    m = step0_layer(F, O, bias, 1).train()
    torch.manual_seed(2)
    x = (torch.randn(3, 5, F, device=DEV) * 1.2).requires_grad_()
    M = 15
    switch(True)
    before = fastpath.stats()
    training.saved_input_bytes(reset=True)
    out = m(x)
    assert delta(before, "linear_real_train") == 1 and delta(before, "linear_real") == 0
    assert training.saved_input_bytes() == 3 * 8 * M * ((F + 63) // 64)      # 3 bits per input element, no fp32 x
    g = torch.randn_like(out)
    out.backward(g)
    alpha = m.activation_post_process.alpha
    W64, x64 = m.weight.detach().double().cpu(), x.detach().double().cpu().reshape(M, F)
    g64 = g.double().cpu().reshape(M, O)
    gc = (g * alpha).detach().reshape(M, O)                                  # the gradient that reaches the function
    gc64 = gc.double().cpu()
    # gW: the weight-gradient kernel's own result on the planes of x, bit for bit
    planes = hipops.pack_act_ste(x.detach().reshape(M, F, 1, 1))
    want_gw = hipops.blinear_grad_weight(gc.contiguous(), planes, reduce=True)
    assert torch.equal(m.weight.grad.view(torch.int32), want_gw.view(torch.int32))
    # gx: float64 reference, bound (O + 1) 2^-23 sum_o |g alpha| |W|; exactly 0 where |x| >= 1
    outside = x64.abs() >= 1
    gx64 = (gc64 @ W64).masked_fill(outside, 0)
    bound = (O + 1) * 2.0 ** -23 * (gc64.abs() @ W64.abs())
    gx = x.grad.double().cpu().reshape(M, F)
    assert ((gx - gx64).abs() <= bound).all(), float(((gx - gx64).abs() / bound.clamp_min(1e-300)).max())
    assert outside.any() and (x.grad.cpu().reshape(M, F)[outside].view(torch.int32) == 0).all() and (gx[~outside] != 0).any()
    # gb and d scale: fp32 sums of n terms, n 2^-23 sum |terms| (any order, truncating adders allowed for)
    n = M
    if bias:
        gb64, gb_abs = gc64.sum(0), gc64.abs().sum(0)
        assert ((m.bias.grad.double().cpu() - gb64).abs() <= n * 2.0 ** -23 * gb_abs).all()
    lin64 = torch.from_numpy(ref(x.detach().cpu().numpy().reshape(M, F), W64.numpy(), np64(m.bias)))
    lin_err = torch.from_numpy(tol(W64.numpy(), lin64.numpy()))             # of the fp32 forward the product is taken with
    da64 = (g64 * lin64).sum(0)
    da_bound = (g64.abs() * lin_err).sum(0) + (n + 1) * 2.0 ** -23 * (g64 * lin64).abs().sum(0)
    assert alpha.grad.numel() == O
    assert ((alpha.grad.double().cpu().reshape(-1) - da64).abs() <= da_bound).all()
    # switch off: the composition, no counter, the fp32 input kept by autograd (nothing counted here)
    switch(False)
    before = fastpath.stats()
    training.saved_input_bytes(reset=True)
    m(x)
    assert fastpath.stats() == before and training.saved_input_bytes() == 0


# ---- the two-step recipe ---------------------------------------------------------------------------------------------
def small_mlp():
    return nn.Sequential(nn.Linear(32, 64), nn.BatchNorm1d(64), nn.Linear(64, 64), nn.BatchNorm1d(64), nn.Linear(64, 48),
                         nn.BatchNorm1d(48), nn.Linear(48, 10))


def sgd_losses(model, steps=3):
    model = copy.deepcopy(model).train()
    opt = torch.optim.SGD(model.parameters(), lr=0.05, momentum=0.9)
    gen = torch.Generator(device="cpu").manual_seed(7)
    losses = []
    for _ in range(steps):
        x = torch.randn(16, 32, generator=gen).to(DEV)
        t = torch.randint(0, 10, (16,), generator=gen).to(DEV)
        opt.zero_grad(set_to_none=True)
        loss = torch.nn.functional.cross_entropy(model(x), t)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses, model


def test_two_step_recipe_trains_step0_linears_on_the_real_weight_path(tmp_path, switch):
    recipe = tmp_path / "two_steps.yaml"
    recipe.write_text(S.RECIPE)
    chef = BinaryChef(str(recipe))
    torch.manual_seed(0)
    model = chef.next(small_mlp()).to(DEV)                                 # step 0
    converted = [m for m in model.modules() if isinstance(m, bnn.layers.Linear)]
    assert len(converted) == 2 and all(isinstance(m.weight_pre_process, nn.Identity) for m in converted)
    assert type(model[0]) is nn.Linear and type(model[6]) is nn.Linear      # first and last stay real-valued layers
    switch(False)
    before = fastpath.stats()
    off, _ = sgd_losses(model)
    assert fastpath.stats() == before
    switch(True)
    on, trained = sgd_losses(model)
    assert delta(before, "linear_real_train") == 3 * len(converted) and delta(before, "linear_train") == 0
    rel = [abs(a - b) / abs(b) for a, b in zip(on, off)]
    print("losses, switch off:", off, "on:", on, "relative difference:", rel)
    assert max(rel) <= 1e-4
    # step 1: XNOR weights belong to the binary Linear's own paths, the real-weight counters stand still
    model1 = chef.next(trained)
    assert all(not isinstance(m.weight_pre_process, nn.Identity) for m in model1.modules() if isinstance(m, bnn.layers.Linear))
    before = fastpath.stats()
    sgd_losses(model1, steps=1)
    assert delta(before, "linear_real_train") == 0 and delta(before, "linear_real") == 0

"""tests/bn_ref.py against torch's own float64 CPU modules, its emulations against its bounds, its mutants against the
cases designed for them, and the completeness of its case table.  No GPU."""
import functools
import itertools

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from bnn_amd import training
from tests import bn_ref as R

F32, F64 = np.float32, np.float64
EPS, MOM = R.EPS, R.MOMENTUM
SHAPE = {k: v[0] for k, v in R.CASES.items()}


def t64(a, grad=False):
    return torch.from_numpy(np.asarray(a, F64).copy()).requires_grad_(grad)


def close(got, want, what, bound=None):
    """1e-12 relative: to the value itself, or — `bound` given — to the magnitudes of the intermediates that the fp32
    bound of the same element is built from (float64 round-off scales with those too, and a normalised value or a
    gradient near zero has no relative accuracy of its own)."""
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    assert got.shape == want.shape, what
    scale = np.abs(want) if bound is None else bound / (R.MARGIN * R.U)
    assert np.all(np.abs(got - want) <= 1e-12 * scale + 1e-300), (what, float(np.abs(got - want).max()))


def ratio(got, want, bound, what):
    """The largest |got - want| / bound over EVERY element (none is left out: the ratio is finite everywhere)."""
    r = np.abs(np.asarray(got, F64) - np.asarray(want, F64)) / bound
    assert r.shape == np.shape(want) and np.isfinite(r).all(), what
    return float(r.max()) if r.size else 0.0


@functools.lru_cache(maxsize=None)
def bn_in(name):
    return R.backward_inputs(name)


@functools.lru_cache(maxsize=None)
def pool_in(name):
    return R.pool_backward_inputs(name)


def torch_bn(i, C, affine=True, momentum=MOM):
    # (eps and momentum as the fp32 numbers the entry points take: the references are functions of those)
    bn = nn.BatchNorm2d(C, eps=float(F32(EPS)), momentum=None if momentum is None else float(F32(momentum)),
                        affine=affine).double().train()
    with torch.no_grad():
        if affine:
            bn.weight.copy_(t64(i["gamma"]))
            bn.bias.copy_(t64(i["beta"]))
        bn.running_mean.copy_(t64(i["rm"]))
        bn.running_var.copy_(t64(i["rv"]))
    return bn


# ------------------------------------------------------------------------------------------------ references == torch
@pytest.mark.parametrize("name", R.BN_CASES)
def test_references_equal_torch_float64_batchnorm(name):
    i = bn_in(name)
    C = SHAPE[name][1]
    for relu, res, affine in ((True, True, True), (False, False, True), (True, False, False), (False, True, True)):
        bn = torch_bn(i, C, affine)
        x, r = t64(i["x"], True), t64(i["residual"], True)
        y = bn(x) + r if res else bn(x)
        y = torch.relu(y) if relu else y
        gamma, beta = (i["gamma"], i["beta"]) if affine else (None, None)
        a = (i["x"], gamma, beta, i["rm"], i["rv"], MOM, EPS, relu, i["residual"] if res else None)
        (ry, rmean, rinv, rrm, rrv), fb = R.forward_ref(*a), R.forward_bound(*a)
        close(y.detach().numpy(), ry, "y", fb[0])
        close(bn.running_mean.numpy(), rrm, "running_mean", fb[3])
        close(bn.running_var.numpy(), rrv, "running_var", fb[4])
        x64 = np.asarray(i["x"], F64)
        close(x64.mean(axis=(0, 2, 3)), rmean, "save_mean")
        close(1 / np.sqrt(x64.var(axis=(0, 2, 3)) + float(F32(EPS))), rinv, "save_invstd")
        y.backward(t64(i["gy"]))
        # the reference is a function of what the kernel takes: here torch's own y, mean and invstd
        y_np = y.detach().numpy()
        assert not np.any((y_np > 0) & (y_np.astype(F32) == 0))
        a = (i["gy"], y_np if relu else None, i["x"], rmean, rinv, gamma)
        (dx, dgamma, dbeta, dres), bb = R.backward_ref(*a), R.backward_bound(*a)
        close(x.grad.numpy(), dx, "dx", bb[0])
        if affine:
            close(bn.weight.grad.numpy(), dgamma, "dgamma", bb[1])
            close(bn.bias.grad.numpy(), dbeta, "dbeta", bb[2])
        if res:
            assert np.array_equal(r.grad.numpy(), dres.astype(F64))
    # the addend: y = x + bn(x) hands its own gradient in
    bn = torch_bn(i, C)
    x = t64(i["x"], True)
    x2 = t64(i["x"], True)
    (bn(x)).backward(t64(i["gy"]))
    x2.backward(t64(i["addend"]))
    _, mean, invstd, _, _ = R.forward_ref(i["x"], None, None, None, None, MOM, EPS)
    a = (i["gy"], None, i["x"], mean, invstd, i["gamma"], i["addend"])
    close((x.grad + x2.grad).numpy(), R.backward_ref(*a)[0], "dx + addend", R.backward_bound(*a)[0])


def test_momentum_none_and_count_one_in_the_reference():
    """Cumulative average: momentum 1 / (batches seen + 1), three steps chained; and count == 1 keeps the biased value."""
    i = bn_in("bn_odd_channels")
    bn = torch_bn(i, SHAPE["bn_odd_channels"][1], momentum=None)
    rm, rv = i["rm"].astype(F64), i["rv"].astype(F64)
    for step in range(3):
        x = i["x"] * F32(1 + step)
        bn(t64(x))
        prev = np.abs(rm), np.abs(rv)
        _, mean, _, rm, rv = R.forward_ref(x, i["gamma"], i["beta"], rm, rv, 1.0 / (step + 1), EPS)
        # (momentum goes through fp32 in the entry point: 1/3 is within 2^-25 relative there, torch's is the double)
        assert np.all(np.abs(bn.running_mean.numpy() - rm) <= 2.0 ** -24 * (prev[0] + np.abs(mean)))
        assert np.all(np.abs(bn.running_var.numpy() - rv) <= 2.0 ** -24 * (prev[1] + 2 * np.abs(rv)))
    x1 = np.full((1, 2, 1, 1), 3.0, F32)
    y, mean, invstd, rm, rv = R.forward_ref(x1, None, None, np.zeros(2, F32), np.ones(2, F32), 0.5, EPS)
    assert np.array_equal(mean, [3.0, 3.0]) and np.array_equal(rv, [0.5, 0.5]) and np.array_equal(y, np.zeros_like(x1))


@pytest.mark.parametrize("name", R.POOL_CASES)
def test_references_equal_torch_float64_stem_tail(name):
    i = pool_in(name)
    N, C, H, W = SHAPE[name]
    bn = torch_bn(i, C)
    x = t64(i["x"], True)
    p, idx = F.max_pool2d(torch.relu(bn(x)), 3, 2, 1, return_indices=True)
    rp, rcode, bp, _, _ = R.pool_forward_oracle(i)
    close(p.detach().numpy(), rp, "p", bp)
    idx = idx.numpy()
    py, px = np.meshgrid(np.arange(R.half(H)), np.arange(R.half(W)), indexing="ij")
    code = 3 * (idx // W - (2 * py - 1)) + (idx % W - (2 * px - 1))
    assert np.array_equal(code, rcode), "first maximum in raster order"
    p.backward(t64(i["gy"]))
    ref, _ = R._forward(i["x"], i["gamma"], i["beta"], None, None, MOM, EPS, False, None)
    p_np = p.detach().numpy()
    assert not np.any((p_np > 0) & (p_np.astype(F32) == 0))
    a = (i["gy"], p_np, rcode, i["x"], ref["mean"], ref["invstd"], i["gamma"])
    (dx, dgamma, dbeta), bb = R.pool_backward_ref(*a), R.pool_backward_bound(*a)
    close(x.grad.numpy(), dx, "dx", bb[0])
    close(bn.weight.grad.numpy(), dgamma, "dgamma", bb[1])
    close(bn.bias.grad.numpy(), dbeta, "dbeta", bb[2])


def test_first_maximum_rule_with_nan_is_torchs():
    v = np.maximum(np.round(R.gen.normal(R.gen.seed_of("bn_ref", "nanpool"), (2, 3, 9, 11)).astype(F64) * 2) / 2, 0)
    v.reshape(-1)[::7] = np.nan
    p, idx = F.max_pool2d(torch.from_numpy(v), 3, 2, 1, return_indices=True)
    rp, rcode = R._first_max(R._windows(v, -1.0))
    assert np.array_equal(p.numpy(), rp, equal_nan=True)
    py, px = np.meshgrid(np.arange(5), np.arange(6), indexing="ij")
    assert np.array_equal(3 * (idx.numpy() // 11 - (2 * py - 1)) + (idx.numpy() % 11 - (2 * px - 1)), rcode)


def test_avgpool_backward_reference_is_torchs():
    g = R.gen.normal(R.gen.seed_of("bn_ref", "avg"), (2, 3, 3, 5))
    x = torch.zeros(2, 3, 6, 10, dtype=torch.float64, requires_grad=True)
    nn.AvgPool2d(2, 2)(x).backward(t64(g))
    assert np.array_equal(x.grad.numpy(), R.avgpool2x2_backward_ref(g).astype(F64))


# ------------------------------------------------------------------------------------------------ emulations vs bounds
WORST = {}


def note(key, r):
    WORST[key] = max(WORST.get(key, 0.0), r)
    return r


def fwd_args(i, res=True, affine=True, running=True):
    return ((i["x"],) + ((i["gamma"], i["beta"]) if affine else (None, None)) + ((i["rm"], i["rv"]) if running else (None, None))
            + (MOM, EPS))


@pytest.mark.parametrize("name", R.BN_CASES)
def test_emulations_stay_within_half_the_bound_batchnorm(name):
    i = bn_in(name)
    assert R.cancellation_ok(i["x"], EPS)
    for relu, res in itertools.product((False, True), repeat=2):
        a = fwd_args(i) + (relu, i["residual"] if res else None)
        ref, bound, emu = R.forward_ref(*a), R.forward_bound(*a), R.emulate_forward(*a)
        for k, r_, b_, e_ in zip(R.KEYS, ref, bound, emu):
            assert note("forward " + k, ratio(e_, r_, b_, k)) <= 0.5, (k, relu, res)
    for y, addend in ((i["y"], None), (None, None), (None, i["addend"])):
        a = (i["gy"], y, i["x"], i["mean"], i["invstd"], i["gamma"], addend)
        ref, bound, emu = R.backward_ref(*a), R.backward_bound(*a), R.emulate_backward(*a)
        for k, r_, b_, e_ in zip(("dx", "dgamma", "dbeta"), ref, bound, emu):
            assert note("backward " + k, ratio(e_, r_, b_, k)) <= 0.5, (k, y is None, addend is None)
        assert np.array_equal(emu[3].view(np.uint32), ref[3].view(np.uint32))


@pytest.mark.parametrize("name", R.POOL_CASES)
def test_emulations_stay_within_half_the_bound_stem_tail(name):
    i = pool_in(name)
    assert R.cancellation_ok(i["x"], EPS)
    rp, rcode, bp, pre, bpre = R.pool_forward_oracle(i)
    # the grid: equal inputs give equal values, distinct ones lie far more than twice the bound apart, and no value lies
    # within the bound of the ReLU's corner — so the codes are decided
    assert np.array_equal(i["x"] * 8, np.round(i["x"] * 8)) and np.abs(i["gamma"] * i["invstd"]).min() >= 0.5
    assert bpre.max() < 1 / 64 and np.all(np.abs(pre) > 2 * bpre)
    p, code, _, _, _, _ = R.emulate_pool_forward(i["x"], i["gamma"], i["beta"], i["rm"], i["rv"], MOM, EPS)
    assert note("pool forward p", ratio(p, rp, bp, "p")) <= 0.5
    assert np.array_equal(code, rcode)
    for p_, c_ in ((i["p"], i["code"]), (i["hand_p"], i["hand_code"])):
        a = (i["gy"], p_, c_, i["x"], i["mean"], i["invstd"], i["gamma"])
        ref, bound, emu = R.pool_backward_ref(*a), R.pool_backward_bound(*a), R.emulate_pool_backward(*a)
        for k, r_, b_, e_ in zip(("dx", "dgamma", "dbeta"), ref, bound, emu):
            assert note("pool backward " + k, ratio(e_, r_, b_, k)) <= 0.5, k


def test_zz_report_worst_emulation_error(capsys):
    with capsys.disabled():
        for k in sorted(WORST):
            print(f"\n  worst emulation error, {k}: {WORST[k]:.3f} of its bound", end="")


# ------------------------------------------------------------------------------------------------ mutants
@pytest.mark.parametrize("mutant", sorted(R.MUTANTS))
def test_every_mutant_leaves_the_bound_fourfold_on_its_case(mutant):
    name, kind = R.mutant_case(mutant), R.MUTANTS[mutant]
    worst, bits = 0.0, False
    if kind == "forward":
        i = bn_in(name)
        a = fwd_args(i) + (True, i["residual"])
        for k, r_, b_, e_ in zip(R.KEYS, R.forward_ref(*a), R.forward_bound(*a), R.emulate_forward(*a, mutant=mutant)):
            worst = max(worst, ratio(e_, r_, b_, k))
    elif kind == "backward":
        i = bn_in(name)
        y, addend = (None, i["addend"]) if mutant == "addend_dropped" else (i["y"], None)
        a = (i["gy"], y, i["x"], i["mean"], i["invstd"], i["gamma"], addend)
        ref, emu = R.backward_ref(*a), R.emulate_backward(*a, mutant=mutant)
        for k, r_, b_, e_ in zip(("dx", "dgamma", "dbeta"), ref, R.backward_bound(*a), emu):
            worst = max(worst, ratio(e_, r_, b_, k))
        bits = not np.array_equal(emu[3].view(np.uint32), ref[3].view(np.uint32))        # dres is compared bit for bit
    elif kind == "pool_forward":
        i = pool_in(name)
        rp, rcode, bp, _, _ = R.pool_forward_oracle(i)
        p, code, _, _, _, _ = R.emulate_pool_forward(i["x"], i["gamma"], i["beta"], i["rm"], i["rv"], MOM, EPS, mutant=mutant)
        worst, bits = ratio(p, rp, bp, "p"), not np.array_equal(code, rcode)
    else:
        i = pool_in(name)
        a = (i["gy"], i["p"], i["code"], i["x"], i["mean"], i["invstd"], i["gamma"])
        for k, r_, b_, e_ in zip(("dx", "dgamma", "dbeta"), R.pool_backward_ref(*a), R.pool_backward_bound(*a),
                                 R.emulate_pool_backward(*a, mutant=mutant)):
            worst = max(worst, ratio(e_, r_, b_, k))
    exact_only = {"dres_unmasked", "pool_last_max"}          # what these change is compared for equality, not to a bound
    assert bits if mutant in exact_only else worst >= 4.0, (mutant, name, worst, bits)


# ------------------------------------------------------------------------------------------------ the table is complete
def test_the_case_table_reaches_every_form_and_regime():
    assert set(R.MUTANTS) == {m for _, _, ms in R.CASES.values() for m in ms}
    reg = {k: R.split_regimes(s[0], s[1]) for k, s in SHAPE.items()}
    assert R.splits(5, 300) == (3, 2) and "ragged" in reg["bn_ragged"]
    assert R.splits(130, 3) == (44, 3) and {"capped", "ragged"} <= reg["bn_capped"]
    assert R.splits(2, 1024) == (1, 2) and reg["bn_single"] == {"single"}
    assert "per_image" in reg["bn_per_image_odd"] and "per_image" in reg["pool_scalar_ragged"]
    hw = {k: s[2] * s[3] for k, s in SHAPE.items()}
    assert {R.bn_form(v) for v in hw.values()} == {1, 4}
    upb = {k: R.units_per_block(s[0], s[1], hw[k]) for k, s in SHAPE.items()}
    assert upb["bn_long_block"] > 256 and upb["bn_per_image_odd"] < 64 and R.bn_form(hw["bn_per_image_odd"]) == 1
    assert SHAPE["bn_odd_channels"][1] % 64 == 1
    for k, (N, C, H, W) in SHAPE.items():      # the allowance for the double sums rests on this
        assert R.sum_depth(N, C, H * W, R.bn_form(H * W)) <= 256 and R.sum_depth(N, C, R.half(H) * R.half(W), 1) <= 256, k
    fwd = {k: R.pool_fwd_form(*SHAPE[k][2:]) for k in R.POOL_CASES}
    bwd = {k: R.pool_bwd_form(*SHAPE[k][2:]) for k in R.POOL_CASES}
    # both LDS limits, on both sides
    assert hw["pool_both_limits"] == 16384 and fwd["pool_both_limits"] == "lds" and bwd["pool_both_limits"] == ("lds",)
    assert hw["pool_over_plane"] > 16384 and fwd["pool_over_plane"] == "gather" and bwd["pool_over_plane"] == ("gather1", 6, True)
    assert R.half(2) * R.half(8192) == 4096 and bwd["pool_hwp_limit"] == ("lds",)
    assert fwd["pool_hwp_over"] == "lds" and bwd["pool_hwp_over"] == ("gather4", 6, True)
    # the float4 gather: a lane loop that only lane 0 enters twice, and several rows per wave
    assert fwd["pool_v4_loop"] == "gather" and bwd["pool_v4_loop"] == ("gather4", 6, True) and SHAPE["pool_v4_loop"][3] // 4 == 65
    assert bwd["pool_v4_rows"] == ("gather4", 5, False) and SHAPE["pool_v4_rows"][2] % 2 == 0
    assert fwd["pool_scalar_ragged"] == "gather" and bwd["pool_scalar_ragged"] == ("gather1", 6, True)
    assert bwd["pool_scalar_rows"] == ("gather1", 3, False) and SHAPE["pool_scalar_rows"][2] % 2 == 0
    assert bwd["pool_lds_small"] == ("lds",) and SHAPE["pool_lds_small"][3] % 4 != 0
    assert set(fwd.values()) == {"lds", "gather"}
    assert {b[0] for b in bwd.values()} == {"lds", "gather4", "gather1"}
    assert {(b[0], b[2]) for b in bwd.values() if len(b) == 3} == {(f, l) for f in ("gather4", "gather1") for l in (False, True)}
    # a misaligned base pointer turns every float4 form into its scalar one
    assert R.bn_form(16, aligned=False) == 1 and R.pool_fwd_form(8, 8, aligned=False) == "gather"
    assert R.pool_bwd_form(8, 8, aligned=False) == ("gather1", 3, False)


def test_the_inputs_bite():
    i = bn_in("bn_per_image_odd")
    mean, var, _ = R._stats64(i["x"])
    assert np.any(np.abs(mean) > 25) and np.any(var > 400) and np.any(var == 0) and np.any(i["gamma"] < 0)
    gmax = np.abs(i["gy"]).max(axis=(0, 2, 3))
    assert gmax.max() / gmax.min() > 1e9
    y = i["y"].view(np.uint32)
    assert {0, 0x80000000, 1} <= set(y.reshape(-1)[:11].tolist()) and np.any((i["y"] < 0) & (i["gy"] != 0))
    pairs, closed, four = set(), 0, 0
    for name in R.POOL_CASES:
        j = pool_in(name)
        _, code, _, pre, _ = R.pool_forward_oracle(j)
        win = R._windows(np.maximum(pre, 0), -1.0)
        best = win.max(axis=0)
        for b in range(9):      # positive ties: the pair (winner, another position of the same value)
            hit = (win[b] == best) & (best > 0) & (code < b)
            pairs |= {(int(a), b) for a in np.unique(code[hit])}
        closed += int(np.sum(j["p"] == 0))
        four += int(np.sum(R.route(np.ones_like(j["gy"]), j["p"], j["code"], j["x"].shape)[2] == 4))
    assert pairs == {(a, b) for a in range(9) for b in range(a + 1, 9)}
    assert closed > 0 and four > 0
    hp, hc = pool_in("pool_lds_small")["hand_p"], pool_in("pool_lds_small")["hand_code"]
    assert np.sum(R.route(np.ones_like(hp), np.ones_like(hp), hc, SHAPE["pool_lds_small"])[2] == 4) > 0
    assert np.any(hp == 0) and np.any(hp == F32(2.0 ** -149))


# ------------------------------------------------------------------------------------------------ the fix
def test_one_value_per_channel_is_declined_and_raises_as_the_module(monkeypatch):
    monkeypatch.setattr(training, "ENABLED", True)
    monkeypatch.setattr(training, "FUSED_BN", True)
    monkeypatch.setattr(training, "_f32_on_one_device", lambda x, *t: True)      # (no HIP device here)
    bn, act, pool = nn.BatchNorm2d(3).train(), nn.ReLU(), nn.MaxPool2d(3, 2, 1)
    assert training.bn_act_applies(bn, act, torch.zeros(2, 3, 1, 1)) and training.bn_act_applies(bn, None, torch.zeros(1, 3, 1, 2))
    x = torch.zeros(1, 3, 1, 1)
    assert not training.bn_act_applies(bn, act, x) and not training.bn_act_applies(bn, None, x)
    with pytest.raises(ValueError) as lib:
        bn(x)
    for call in (lambda: training.bn_act(x, bn, act), lambda: training.bn_act(x, bn), lambda: training.stem_tail(x, bn, act, pool)):
        with pytest.raises(ValueError) as ours:
            call()
        assert str(ours.value) == str(lib.value) and "Expected more than 1 value per channel" in str(ours.value)

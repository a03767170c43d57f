"""The training BatchNorm kernels and the stem tail (csrc/bn_train.hip) against the float64 oracle of tests/bn_ref.py, at
every kernel form, LDS limit and split regime its case table reaches, each output within its counted per-element bound
(or bit for bit where the result is exact).  tests/test_bn_ref_cpu.py ties the oracle to torch's float64 modules."""
import functools
import itertools

import numpy as np
import pytest
import torch
import torch.nn as nn

from bnn_amd import hipops, training
from tests import bn_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = np.float32, np.float64
EPS, MOM = R.EPS, R.MOMENTUM
SHAPE = {k: v[0] for k, v in R.CASES.items()}
WORST = {}


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def off(t):
    """The same values as a view one element into its storage: 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:].copy_(t.reshape(-1))
    v = buf[1:].view(t.shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == t.element_size()
    return v


def host(t):
    return None if t is None else t.detach().cpu().numpy().copy()


def dirty(*nbytes):
    """The allocator's next blocks of these sizes start as garbage (NaN patterns): an element a kernel leaves out is not a
    lucky 0.  All are held at once, so that two outputs of one size are both dirtied."""
    held = [torch.empty(int(n), dtype=torch.uint8, device=DEV).fill_(0xFF) for n in nbytes if n]
    del held


def dirty_like(x, pooled=False):
    N, C, H, W = x.shape
    n, c = x.numel() * 4, C * 4
    hp = N * C * R.half(H) * R.half(W)
    dirty(n, n, c, c, c, c, *((hp * 4, hp) if pooled else ()))


def within(got, ref, bound, what):
    """Every element within its bound; none is left out (the ratio is finite everywhere)."""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    assert got.shape == ref.shape, what
    r = np.abs(got - ref) / bound
    assert np.isfinite(r).all(), (what, "non-finite")
    worst = float(r.max()) if r.size else 0.0
    key = what.split(":")[0]
    WORST[key] = max(WORST.get(key, 0.0), worst)
    assert worst <= 1.0, (what, worst, int(np.argmax(r)))


def bits(t):
    return host(t).view(np.uint32 if t.dtype == torch.float32 else np.uint8)


def same_bits(a, b, what):
    for u, v in zip(a, b):
        assert (u is None) == (v is None), what
        assert u is None or np.array_equal(bits(u), bits(v)), what


@functools.lru_cache(maxsize=None)
def bn_in(name):
    return R.backward_inputs(name)


@functools.lru_cache(maxsize=None)
def pool_in(name):
    return R.pool_backward_inputs(name)


@functools.lru_cache(maxsize=None)
def on_dev(kind, name):
    return {k: dev(v) for k, v in (bn_in(name) if kind == "bn" else pool_in(name)).items()}


# ------------------------------------------------------------------------------------------------ bn_train_forward
def run_forward(d, relu, res, affine, running, x=None, residual=None):
    rm, rv = (d["rm"].clone(), d["rv"].clone()) if running else (None, None)
    x = d["x"] if x is None else x
    dirty_like(x)
    y, mean, invstd = hipops.bn_train_forward(x, d["gamma"] if affine else None, d["beta"] if affine else None, rm, rv, MOM, EPS,
                                              relu, (d["residual"] if residual is None else residual) if res else None)
    return y, mean, invstd, rm, rv


@pytest.mark.parametrize("name", R.BN_CASES)
def test_forward_every_output_within_its_bound(name):
    i, d = bn_in(name), on_dev("bn", name)
    for relu, res, affine, running in itertools.product((False, True), repeat=4):
        got = run_forward(d, relu, res, affine, running)
        a = (i["x"],) + ((i["gamma"], i["beta"]) if affine else (None, None)) + ((i["rm"], i["rv"]) if running else (None, None)) \
            + (MOM, EPS, relu, i["residual"] if res else None)
        for k, g_, r_, b_ in zip(R.KEYS, got, R.forward_ref(*a), R.forward_bound(*a)):
            assert (g_ is None) == (r_ is None)
            if g_ is not None:
                within(host(g_), r_, b_, f"forward {k}: {name} relu={relu} res={res} affine={affine}")
    same_bits(run_forward(d, True, True, True, True), run_forward(d, True, True, True, True), "the same call twice")


@pytest.mark.parametrize("name", [k for k in R.BN_CASES if SHAPE[k][1] > 1])
def test_forward_nan_poisons_its_channel_only(name):
    i, d = bn_in(name), dict(on_dev("bn", name))
    C = SHAPE[name][1]
    x = i["x"].copy()
    x[-1, C - 1, -1, -1] = np.nan
    d["x"] = dev(x)
    got = run_forward(d, True, True, True, True)
    a = (x, i["gamma"], i["beta"], i["rm"], i["rv"], MOM, EPS, True, i["residual"])
    for k, g_, r_, b_ in zip(R.KEYS, got, R.forward_ref(*a), R.forward_bound(*a)):
        g_ = host(g_)
        sel = (slice(None), slice(0, C - 1)) if g_.ndim == 4 else (slice(0, C - 1),)
        bad = (slice(None), C - 1) if g_.ndim == 4 else (C - 1,)
        within(g_[sel], r_[sel], b_[sel], f"forward {k}: {name} beside a NaN channel")
        assert np.isnan(g_[bad]).all() and np.isnan(r_[bad]).all(), k


# ------------------------------------------------------------------------------------------------ bn_train_backward[_add]
def run_backward(d, relu, affine, want_dres, gy=None, x=None):
    x = d["x"] if x is None else x
    dirty_like(x)
    return hipops.bn_train_backward(d["gy"] if gy is None else gy, d["y"] if relu else None, x, d["mean"], d["invstd"],
                                    d["gamma"] if affine else None, want_dres=want_dres)


def run_backward_add(d, addend, gy=None, x=None):
    x = d["x"] if x is None else x
    dirty_like(x)
    return hipops.bn_train_backward_add(d["gy"] if gy is None else gy, x, d["mean"], d["invstd"], d["gamma"], addend)


@pytest.mark.parametrize("name", R.BN_CASES)
def test_backward_every_output_within_its_bound(name):
    i, d = bn_in(name), on_dev("bn", name)
    for relu, affine, want_dres in itertools.product((False, True), repeat=3):
        dx, dgamma, dbeta, dres = run_backward(d, relu, affine, want_dres)
        a = (i["gy"], i["y"] if relu else None, i["x"], i["mean"], i["invstd"], i["gamma"] if affine else None)
        ref, bound = R.backward_ref(*a), R.backward_bound(*a)
        for k, g_, r_, b_ in zip(("dx", "dgamma", "dbeta"), (dx, dgamma, dbeta), ref, bound):
            within(host(g_), r_, b_, f"backward {k}: {name} relu={relu} affine={affine} dres={want_dres}")
        assert (dres is not None) == want_dres
        if want_dres:       # the masked gy itself: bit for bit (+0 where the mask is closed)
            assert np.array_equal(bits(dres), ref[3].view(np.uint32)), "dres"
    a = (i["gy"], None, i["x"], i["mean"], i["invstd"], i["gamma"], i["addend"])
    got = run_backward_add(d, d["addend"])
    for k, g_, r_, b_ in zip(("dx", "dgamma", "dbeta"), got, R.backward_ref(*a), R.backward_bound(*a)):
        within(host(g_), r_, b_, f"backward_add {k}: {name}")
    same_bits(run_backward_add(d, None), run_backward(d, False, True, False)[:3], "addend=None is bn_train_backward")
    same_bits(run_backward(d, True, True, True), run_backward(d, True, True, True), "the same call twice")
    same_bits(got, run_backward_add(d, d["addend"]), "the same call twice")


# ------------------------------------------------------------------------------------------------ misaligned base pointers
@pytest.mark.parametrize("name", R.BN_CASES)
def test_a_view_one_float_into_its_storage_gives_the_same_bits(name):
    """The scalar forms a misaligned pointer selects do per element what the float4 forms do (the same fmaf, the same
    expression for dx), and the double sums they feed agree to ~2^-50 where the fp32 results are cast from: the same bits."""
    d = on_dev("bn", name)
    want = run_forward(d, True, True, True, True)
    same_bits(run_forward(d, True, True, True, True, x=off(d["x"])), want, "x")
    same_bits(run_forward(d, True, True, True, True, residual=off(d["residual"])), want, "residual")
    want = run_backward(d, True, True, True)
    same_bits(run_backward(d, True, True, True, gy=off(d["gy"])), want, "gy")
    same_bits(run_backward(d, True, True, True, x=off(d["x"])), want, "x (backward)")
    want = run_backward_add(d, d["addend"])
    same_bits(run_backward_add(d, off(d["addend"])), want, "addend")
    same_bits(run_backward_add(d, d["addend"], gy=off(d["gy"])), want, "gy (add)")


# ------------------------------------------------------------------------------------------------ the stem tail
def run_pool_forward(d, affine=True, running=True, x=None):
    rm, rv = (d["rm"].clone(), d["rv"].clone()) if running else (None, None)
    x = d["x"] if x is None else x
    dirty_like(x, pooled=True)
    p, code, mean, invstd = hipops.bn_relu_maxpool_train_forward(x, d["gamma"] if affine else None, d["beta"] if affine else None,
                                                                 rm, rv, MOM, EPS)
    return p, code, mean, invstd, rm, rv


def in_range(code, shape):
    N, C, H, W = shape
    py, px = np.meshgrid(np.arange(R.half(H)), np.arange(R.half(W)), indexing="ij")
    r, q = 2 * py - 1 + code.astype(np.int64) // 3, 2 * px - 1 + code.astype(np.int64) % 3
    return bool(np.all((code < 9) & (r >= 0) & (r < H) & (q >= 0) & (q < W)))


@pytest.mark.parametrize("name", R.POOL_CASES)
def test_pool_forward_values_within_bounds_and_first_maximum_codes(name):
    i, d = pool_in(name), on_dev("pool", name)
    rp, rcode, bp, _, _ = R.pool_forward_oracle(i)
    p, code, mean, invstd, rm, rv = run_pool_forward(d)
    within(host(p), rp, bp, f"pool forward p: {name}")
    assert in_range(host(code), SHAPE[name]) and np.array_equal(host(code), rcode), "first maximum in raster order"
    a = (i["x"], i["gamma"], i["beta"], i["rm"], i["rv"], MOM, EPS)
    for k, g_, r_, b_ in zip(R.KEYS[1:], (mean, invstd, rm, rv), R.forward_ref(*a)[1:], R.forward_bound(*a)[1:]):
        within(host(g_), r_, b_, f"pool forward {k}: {name}")
    same_bits(run_pool_forward(d), (p, code, mean, invstd, rm, rv), "the same call twice")
    # a view one float into its storage takes the gather form: the same nine comparisons in the same order
    same_bits(run_pool_forward(d, x=off(d["x"])), (p, code, mean, invstd, rm, rv), "x")
    # no affine parameters, no running statistics (gamma == 1: the grid's |scale| >= 0.5 needs invstd >= 0.5 — it is ~1)
    j = dict(i, gamma=None, beta=None)
    ref, bound = R._forward(i["x"], None, None, None, None, MOM, EPS, False, None)
    p, code, mean, invstd, rm, rv = run_pool_forward(d, affine=False, running=False)
    rp, rcode = R.pool_forward_ref(i["x"], ref["scale"], ref["shift"])
    assert rm is None and rv is None and np.all(np.abs(ref["y"]) > bound["y"]) and j["gamma"] is None
    within(host(p), rp, R.window_max(bound["y"]), f"pool forward p: {name} plain")
    assert np.array_equal(host(code), rcode)


@pytest.mark.parametrize("name", [k for k in R.POOL_CASES if SHAPE[k][1] > 1])
def test_pool_forward_nan_poisons_its_channel_only(name):
    i, d = pool_in(name), dict(on_dev("pool", name))
    C = SHAPE[name][1]
    x = i["x"].copy()
    x[-1, C - 1, -1, -1] = np.nan
    d["x"] = dev(x)
    p, code, mean, invstd, rm, rv = run_pool_forward(d)
    rp, rcode, bp, _, _ = R.pool_forward_oracle(dict(i, x=x))
    within(host(p)[:, :C - 1], rp[:, :C - 1], bp[:, :C - 1], f"pool forward p: {name} beside a NaN channel")
    assert np.isnan(host(p)[:, C - 1]).all() and np.isnan(rp[:, C - 1]).all()
    assert in_range(host(code), SHAPE[name]) and np.array_equal(host(code), rcode), "the last NaN of a window wins it"
    assert np.isnan(host(mean)[C - 1]) and np.isnan(host(rv)[C - 1]) and np.isfinite(host(mean)[:C - 1]).all()


def with_tail(gy, p, code):
    """The pooled tensors as views of storages that go on for one more pooled row of R's tail: open windows with a large
    gradient whose codes name window row 0.  Nothing may read it."""
    Wp = p.shape[-1]
    n = p.numel()
    out = []
    for t, tail in ((gy, np.full(Wp, R.TAIL_GY, F32)), (p, np.full(Wp, R.TAIL_P, F32)), (code, (np.arange(Wp) % 3).astype(np.uint8))):
        buf = torch.cat([t.reshape(-1), dev(tail)])
        out.append(buf[:n].view(t.shape))
    return out


def run_pool_backward(gy, p, code, x, mean, invstd, gamma):
    dirty_like(x)
    return hipops.bn_relu_maxpool_train_backward(gy, p, code, x, mean, invstd, gamma)


@pytest.mark.parametrize("name", R.POOL_CASES)
def test_pool_backward_every_output_within_its_bound(name):
    i, d = pool_in(name), on_dev("pool", name)
    fp, fcode, fmean, finvstd, _, _ = run_pool_forward(d)
    for what, p, code, mean, invstd in (("hand-made", d["hand_p"], d["hand_code"], d["mean"], d["invstd"]),
                                        ("forward's own", fp, fcode, fmean, finvstd)):
        gy, p, code = with_tail(d["gy"], p, code)
        a = (i["gy"], host(p), host(code), i["x"], host(mean), host(invstd), i["gamma"])
        ref, bound = R.pool_backward_ref(*a), R.pool_backward_bound(*a)
        got = run_pool_backward(gy, p, code, d["x"], mean, invstd, d["gamma"])
        for k, g_, r_, b_ in zip(("dx", "dgamma", "dbeta"), got, ref, bound):
            within(host(g_), r_, b_, f"pool backward {k}: {name} {what}")
        same_bits(run_pool_backward(gy, p, code, d["x"], mean, invstd, d["gamma"]), got, "the same call twice")
        same_bits(run_pool_backward(off(d["gy"]), p, code, d["x"], mean, invstd, d["gamma"]), got, "gy one float in")
        # x one float in: the gather form instead of the LDS one adds a pixel's (up to four) window gradients in another
        # order, so dx agrees within the bound, not in its bits; the reductions never see those fp32 sums
        mis = run_pool_backward(gy, p, code, off(d["x"]), mean, invstd, d["gamma"])
        within(host(mis[0]), ref[0], bound[0], f"pool backward dx: {name} {what}, x one float in")
        same_bits(mis[1:], got[1:], "dgamma, dbeta with x one float in")


# ------------------------------------------------------------------------------------------------ avgpool2x2_backward
@pytest.mark.parametrize("shape", [(2, 3, 3, 4), (2, 3, 3, 5), (1, 1, 1, 1), (3, 5, 9, 130)])
def test_avgpool_backward_is_exact_in_both_forms(shape):
    g = (R.gen.normal(R.gen.seed_of("bn_ref", "avg", shape), shape) * 10.0 ** (np.arange(shape[1]) % 7 - 3)[None, :, None, None]).astype(F32)
    want = R.avgpool2x2_backward_ref(g).view(np.uint32)
    n = int(np.prod(shape)) * 16
    for t in (dev(g), off(dev(g))):         # the float2 form where Wo is even, and the scalar form of a misaligned gy
        dirty(n)
        assert np.array_equal(bits(hipops.avgpool2x2_backward(t)), want)


# ------------------------------------------------------------------------------------------------ through the modules
def module_for(i, C, momentum, affine=True):
    bn = nn.BatchNorm2d(C, eps=EPS, momentum=momentum, affine=affine).to(DEV).train()
    with torch.no_grad():
        if affine:
            bn.weight.copy_(dev(i["gamma"]))
            bn.bias.copy_(dev(i["beta"]))
        bn.running_mean.copy_(dev(i["rm"]))
        bn.running_var.copy_(dev(i["rv"]))
    return bn


@pytest.mark.parametrize("affine,offset", [(True, False), (False, False), (True, True)])
def test_bn_act_three_steps_of_cumulative_average(affine, offset):
    name = "bn_odd_channels"
    i, C = bn_in(name), SHAPE[name][1]
    bn, act = module_for(i, C, None, affine), nn.ReLU()
    gamma, beta = (i["gamma"], i["beta"]) if affine else (None, None)
    for step in range(3):
        x_np = (i["x"] * F32(1 + step)).astype(F32)
        leaf = (off(dev(x_np)) if offset else dev(x_np)).requires_grad_(True)
        res = dev(i["residual"]).requires_grad_(True)
        assert training.bn_act_applies(bn, act, leaf)
        rm0, rv0 = host(bn.running_mean), host(bn.running_var)
        y = training.bn_act(leaf, bn, act, res)
        assert type(y.grad_fn).__name__.startswith("BNActFn") and int(bn.num_batches_tracked) == step + 1
        a = (x_np, gamma, beta, rm0, rv0, 1.0 / (step + 1), EPS, True, i["residual"])
        ref, bound = R.forward_ref(*a), R.forward_bound(*a)
        within(host(y), ref[0], bound[0], f"bn_act y: step {step}")
        within(host(bn.running_mean), ref[3], bound[3], f"bn_act rm: step {step}")
        within(host(bn.running_var), ref[4], bound[4], f"bn_act rv: step {step}")
        xs, ys, mean, invstd, _ = y.grad_fn.saved_tensors
        assert xs.data_ptr() == leaf.data_ptr()          # (.contiguous() keeps the offset view: the scalar forms run)
        within(host(mean), ref[1], bound[1], "bn_act mean")
        within(host(invstd), ref[2], bound[2], "bn_act invstd")
        y.backward(dev(i["gy"]))
        b = (i["gy"], host(y), x_np, host(mean), host(invstd), gamma)
        bref, bb = R.backward_ref(*b), R.backward_bound(*b)
        within(host(leaf.grad), bref[0], bb[0], "bn_act dx")
        if affine:
            within(host(bn.weight.grad), bref[1], bb[1], "bn_act dgamma")
            within(host(bn.bias.grad), bref[2], bb[2], "bn_act dbeta")
            bn.weight.grad = bn.bias.grad = None
        assert np.array_equal(bits(res.grad), bref[3].view(np.uint32))


@pytest.mark.parametrize("offset", [False, True])
def test_stem_tail_three_steps_of_cumulative_average(offset):
    name = "pool_lds_small"
    i, C = pool_in(name), SHAPE[name][1]
    bn, act, pool = module_for(i, C, None), nn.ReLU(), nn.MaxPool2d(3, 2, 1)
    for step in range(3):
        x_np = i["x"] if step == 0 else (i["x"] + F32(step)).astype(F32)          # (still on the grid)
        leaf = (off(dev(x_np)) if offset else dev(x_np)).requires_grad_(True)
        rm0, rv0 = host(bn.running_mean), host(bn.running_var)
        p = training.stem_tail(leaf, bn, act, pool)
        assert type(p.grad_fn).__name__.startswith("StemTailFn") and int(bn.num_batches_tracked) == step + 1
        a = (x_np, i["gamma"], i["beta"], rm0, rv0, 1.0 / (step + 1), EPS)
        ref, bound = R.forward_ref(*a), R.forward_bound(*a)
        rp, rcode, bp, pre, bpre = R.pool_forward_oracle(dict(i, x=x_np))
        assert np.all(np.abs(pre) > bpre)
        within(host(p), rp, bp, f"stem_tail p: step {step}")
        within(host(bn.running_mean), ref[3], bound[3], f"stem_tail rm: step {step}")
        within(host(bn.running_var), ref[4], bound[4], f"stem_tail rv: step {step}")
        xs, ps, code, mean, invstd, _ = p.grad_fn.saved_tensors
        assert np.array_equal(host(code), rcode)
        p.backward(dev(i["gy"]))
        b = (i["gy"], host(ps), host(code), x_np, host(mean), host(invstd), i["gamma"])
        bref, bb = R.pool_backward_ref(*b), R.pool_backward_bound(*b)
        for k, g_, r_, b_ in zip(("dx", "dgamma", "dbeta"), (leaf.grad, bn.weight.grad, bn.bias.grad), bref, bb):
            within(host(g_), r_, b_, f"stem_tail {k}")
        bn.weight.grad = bn.bias.grad = None


def test_one_value_per_channel_raises_as_the_module_does():
    bn, act, pool = nn.BatchNorm2d(3).to(DEV).train(), nn.ReLU(), nn.MaxPool2d(3, 2, 1)
    x = torch.zeros(1, 3, 1, 1, device=DEV, requires_grad=True)
    assert training.bn_act_applies(bn, act, torch.zeros(2, 3, 1, 1, device=DEV)) and not training.bn_act_applies(bn, act, x)
    with pytest.raises(ValueError) as lib:
        bn(x)
    for call in (lambda: training.bn_act(x, bn, act), lambda: training.bn_act(x, bn), lambda: training.stem_tail(x, bn, act, pool)):
        with pytest.raises(ValueError) as ours:
            call()
        assert str(ours.value) == str(lib.value)


def test_zz_report_worst_error(capsys):
    with capsys.disabled():
        for k in sorted(WORST):
            print(f"\n  worst error on the device, {k}: {WORST[k]:.3f} of its bound", end="")

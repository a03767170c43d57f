"""The one-launch hierarchical block (csrc/hblock.hip pixel lanes, csrc/hblock_cl.hip channel lanes) against the CPU
oracle (tests/hblock_oracle.py), bit for bit: the plain form (bnn_hip_hblock_forward), the pool form
(bnn_hip_hblock_pool_forward) and the shortcut form (bnn_hip_hblock_shortcut_forward), on every shape of
test_gpu_hblock.py plus one-pixel rows, ragged bands, N = 1 and N = 130, over swept plans and the data kinds of
hblock_oracle.KINDS (negative BatchNorm scales, exact ties, saturated packs, a cancelling residual).  Nothing on the
reference side is a HIP launch: the weights, constants and planes come from numpy, the expected bits from the oracle."""
import ctypes
import dataclasses
import functools
import zlib

import numpy as np
import pytest
import torch

from bnn_amd import hipops, native
from tests import hblock_oracle as hbo
from tests.test_gpu_hblock import PLANS, POOL_PLANS, POOL_SHAPES, SC_SHAPES, SHAPES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

PLAIN_EDGES = [(64, 64, 2, 1, 19), (64, 64, 2, 23, 1), (64, 64, 1, 9, 9), (128, 128, 7, 6, 5), (64, 64, 130, 5, 5)]
POOL_EDGES = [(64, 2, 2, 2), (128, 3, 4, 2), (64, 1, 6, 6), (64, 7, 4, 6)]          # planes, N, H, W
SC_EDGES = [(64, 2, 1, 19), (64, 7, 6, 5), (128, 1, 3, 3)]                           # C_in, N, H, W
SWEEP_MAX_PIXELS = 150     # images up to this size sweep the plans instead of taking the fixed lists


def _plans(N, H, W, fixed):
    """Every plan of the sweep (rows_per_band 0..H, images_per_band {0, 1, 2, 3, N}, waves, throughput) for small images,
    else the fixed list of test_gpu_hblock.py."""
    if H * W > SWEEP_MAX_PIXELS:
        return [p for p in fixed if p.get("rows_per_band", 0) <= H and p.get("images_per_band", 0) <= N]
    return [dict(rows_per_band=r, images_per_band=i, waves=w, throughput=t)
            for r in range(H + 1) for i in sorted({0, 1, 2, 3, N}) for w in (0, 1, 2, 3, 4, 8, 16) for t in (False, True)]


def _min_ran(N, H, W):
    return 40 if H * W <= SWEEP_MAX_PIXELS else 4


def _dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(DEV)


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _bn(bn):
    return _dev(bn[0]), _dev(bn[1])


@functools.lru_cache(maxsize=16)
def _case(form, shape, kind):
    """Block data, its oracle route and the device-side inputs, once per form, shape and data kind."""
    if form == "plain":
        c_in, planes, N, H, W = shape
    elif form == "pool":
        planes, N, H, W = shape
        c_in = planes
    else:
        c_in, N, H, W = shape
        planes = 2 * c_in
    d = hbo.draw(zlib.crc32(repr((form, shape, kind)).encode()) % 10007, c_in, planes, N, H, W, kind, form)
    want = hbo.run(d, form)
    p_in = hipops.PackedAct(_dev(d["P_in"]), torch.zeros_like(_dev(d["P_in"])), (N, c_in, H, W), nonneg=True)
    pws = [hipops.pack_weight(_dev(w)) for w in d["ws"]]
    ins = dict(p_in=p_in, pws=pws, geom=(N, c_in, H, W, planes))
    if form == "pool":
        ins["pack"] = hipops.hblock_pack(*pws, _bn(d["bn2"]), _bn(d["bn3"]), None)
        ins["kp"] = hipops.hblock_pool_consts(_bn(d["bn1"]), _bn(d["bn_ds"]), planes)
        ins["res"] = _dev(d["res"])
    else:
        ins["pack"] = hipops.hblock_pack(*pws, _bn(d["bn2"]), _bn(d["bn3"]), _bn(d["nbn"]))
    if form == "plain":
        ins["pack_last"] = hipops.hblock_pack(*pws, _bn(d["bn2"]), _bn(d["bn3"]), None)
        ins["res"] = _dev(d["res"])
    if form == "shortcut":
        ins["p_sc"] = hipops.PackedAct(_dev(d["P_sc"]), _dev(d["M_sc"]), (N, c_in, H, W), nonneg=False)
        ins["sc_pack"] = hipops.hblock_shortcut_pack(hipops.pack_weight(_dev(d["w_sc"])))
    return d, want, ins


def _check_next(y, p, want, what):
    assert torch.equal(y.cpu(), torch.from_numpy(want["y"])), what
    assert np.array_equal(_u64(p.P), want["P"]), what
    assert p.nonneg and not bool(p.M.any()) and not want["M"].any(), what


def _ids(s):
    return "x".join(map(str, s))


@pytest.mark.parametrize("kind", hbo.KINDS)
@pytest.mark.parametrize("shape", SHAPES + PLAIN_EDGES, ids=_ids)
def test_plain_form_against_the_oracle(shape, kind):
    d, want, ins = _case("plain", shape, kind)
    N, c_in, H, W, planes = ins["geom"]
    ran = 0
    for plan in _plans(N, H, W, PLANS):
        if not hipops.hblock_supported(N, c_in, H, W, planes, **plan):
            continue
        y, p = hipops.hblock_forward(ins["p_in"], ins["pack"], ins["res"], **plan)
        _check_next(y, p, want, plan)
        y2, p2 = hipops.hblock_forward(ins["p_in"], ins["pack_last"], ins["res"], out_packed=False, **plan)
        assert p2 is None and torch.equal(y2.cpu(), torch.from_numpy(want["y"])), plan
        ran += 1
    assert ran >= _min_ran(N, H, W), ran
    if hipops.hblock_supported(N, c_in, H, W, planes, channel_lanes=True):
        for waves in (0, 3, 4):
            y, p = hipops.hblock_forward(ins["p_in"], ins["pack"], ins["res"], channel_lanes=True, waves=waves)
            _check_next(y, p, want, ("channel lanes", waves))
            y2, _ = hipops.hblock_forward(ins["p_in"], ins["pack_last"], ins["res"], out_packed=False, channel_lanes=True,
                                          waves=waves)
            assert torch.equal(y2.cpu(), torch.from_numpy(want["y"])), waves
    if kind == "cancel":
        assert (want["y"] == 0).mean() > 0.1


@pytest.mark.parametrize("kind", hbo.KINDS)
@pytest.mark.parametrize("shape", POOL_SHAPES + POOL_EDGES, ids=_ids)
def test_pool_form_against_the_oracle(shape, kind):
    d, want, ins = _case("pool", shape, kind)
    N, c_in, H, W, planes = ins["geom"]
    ran = 0
    for plan in _plans(N, H, W, POOL_PLANS):
        if not hipops.hblock_pool_supported(N, c_in, H, W, planes, **plan):
            continue
        p1, p2 = hipops.hblock_pool_forward(ins["p_in"], ins["pack"], ins["res"], ins["kp"], **plan)
        assert np.array_equal(_u64(p1.P), want["P1"]) and p1.nonneg and not bool(p1.M.any()), plan
        assert np.array_equal(_u64(p2.P), want["P2"]) and np.array_equal(_u64(p2.M), want["M2"]), plan
        assert not p2.nonneg
        ran += 1
    # (the pool form takes bands of whole windows: half the swept row counts are refused)
    assert ran >= _min_ran(N, H, W) // 2, ran
    if kind == "ties":
        assert bool((hbo.signs_of(want["P2"], want["M2"], planes) == 0).any())     # sign(0) == 0 did occur


@pytest.mark.parametrize("kind", hbo.KINDS)
@pytest.mark.parametrize("shape", SC_SHAPES + SC_EDGES, ids=_ids)
def test_shortcut_form_against_the_oracle(shape, kind):
    d, want, ins = _case("shortcut", shape, kind)
    N, c_in, H, W, planes = ins["geom"]
    ran = 0
    pixel_lanes = hipops.hblock_shortcut_supported(N, c_in, H, W, planes)
    for plan in _plans(N, H, W, PLANS) if pixel_lanes else ():
        if not hipops.hblock_shortcut_supported(N, c_in, H, W, planes, **plan):
            continue
        y, p = hipops.hblock_shortcut_forward(ins["p_in"], ins["pack"], ins["p_sc"], ins["sc_pack"], **plan)
        _check_next(y, p, want, plan)
        ran += 1
    assert ran >= _min_ran(N, H, W) or not pixel_lanes, ran
    cl = hipops.hblock_shortcut_supported(N, c_in, H, W, planes, channel_lanes=True)
    assert pixel_lanes or cl
    if cl:
        for waves in (0, 3, 4):
            y, p = hipops.hblock_shortcut_forward(ins["p_in"], ins["pack"], ins["p_sc"], ins["sc_pack"], channel_lanes=True,
                                                  waves=waves)
            _check_next(y, p, want, ("channel lanes", waves))


def test_pool_consts_refuse_a_scale_that_does_not_divide_by_four():
    planes = 64
    ok = (torch.ones(planes, device=DEV), torch.zeros(planes, device=DEV))
    hipops.hblock_pool_consts(ok, ok, planes)
    for tiny in (np.nextafter(np.float32(2.0 ** -126), np.float32(1)), np.float32(2.0 ** -149)):
        for which in (0, 1):
            a = torch.ones(planes, device=DEV)
            a[5] = float(tiny) * (-1.0 if which else 1.0)
            bns = [ok, ok]
            bns[which] = (a, ok[1])
            with pytest.raises(native.NativeError):
                hipops.hblock_pool_consts(bns[0], bns[1], planes)


def _offset_view(t, nbytes):
    """A copy of ``t`` that starts ``nbytes`` past a fresh allocation (a misaligned, contiguous view)."""
    k = nbytes // t.element_size()
    buf = torch.zeros(t.numel() + 16, dtype=t.dtype, device=t.device)
    v = buf[k:k + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def test_misaligned_constants_and_channel_lane_tensors_are_refused():
    """include/bnn_hip.h, next to bnn_hip_hblock_layout: consts 32-byte aligned in all three entry points (the kernels read
    it eight floats at a time); residual and out 8-byte aligned for the channel-lane form on 14 x 14 images.  Refused by
    the host-side check before any launch; a 32-byte offset is accepted and computes the same bits."""
    _, want, ins = _case("plain", (256, 256, 5, 14, 14), "neg_scales")
    N, c_in, H, W, planes = ins["geom"]
    pack, res, p_in = ins["pack"], ins["res"], ins["p_in"]
    bad = dataclasses.replace(pack, consts=_offset_view(pack.consts, 8))
    assert bad.consts.data_ptr() % 32 == 8
    for cl in (False, True):
        with pytest.raises(native.NativeError):
            hipops.hblock_forward(p_in, bad, res, channel_lanes=cl)
    good = dataclasses.replace(pack, consts=_offset_view(pack.consts, 32))
    _check_next(*hipops.hblock_forward(p_in, good, res), want, "consts at a 32-byte offset")
    # the channel-lane form on 14 x 14: two pixels per access of residual and out
    assert hipops.hblock_supported(N, c_in, H, W, planes, channel_lanes=True)
    res4 = _offset_view(res, 4)
    assert res4.data_ptr() % 8 == 4
    with pytest.raises(native.NativeError):
        hipops.hblock_forward(p_in, pack, res4, channel_lanes=True)
    lib = native.require()
    d = hipops._hblock_desc(N, c_in, H, W, planes, channel_lanes=True)
    out4 = _offset_view(torch.empty_like(res), 4)
    outP = torch.empty((N, planes // 64, H, W), dtype=torch.int64, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    st = lib.bnn_hip_hblock_forward(ctypes.byref(d), p_in.P.data_ptr(), pack.channel_lane_weights().data_ptr(),
                                    pack.consts.data_ptr(), res.data_ptr(), out4.data_ptr(), outP.data_ptr(), stream)
    assert st == -1                                                   # BNN_HIP_ERR_INVALID_ARG
    # the pool form and the shortcut form
    _, _, ip = _case("pool", (256, 5, 14, 14), "neg_scales")
    bad = dataclasses.replace(ip["pack"], consts=_offset_view(ip["pack"].consts, 8))
    with pytest.raises(native.NativeError):
        hipops.hblock_pool_forward(ip["p_in"], bad, ip["res"], ip["kp"])
    _, _, isc = _case("shortcut", (128, 5, 14, 14), "neg_scales")
    bad = dataclasses.replace(isc["pack"], consts=_offset_view(isc["pack"].consts, 8))
    for cl in (False, True):
        with pytest.raises(native.NativeError):
            hipops.hblock_shortcut_forward(isc["p_in"], bad, isc["p_sc"], isc["sc_pack"], channel_lanes=cl)
    N, c_in, H, W, planes = isc["geom"]
    d = hipops._hblock_desc(N, c_in, H, W, planes, channel_lanes=True)
    assert lib.bnn_hip_hblock_shortcut_supported(ctypes.byref(d))
    wsc, asc = isc["sc_pack"]
    out4 = _offset_view(torch.empty((N, planes, H, W), device=DEV), 4)
    outP = torch.empty((N, planes // 64, H, W), dtype=torch.int64, device=DEV)
    st = lib.bnn_hip_hblock_shortcut_forward(ctypes.byref(d), isc["p_in"].P.data_ptr(),
                                             isc["pack"].channel_lane_weights().data_ptr(), isc["pack"].consts.data_ptr(),
                                             isc["p_sc"].P.data_ptr(), isc["p_sc"].M.data_ptr(), wsc.data_ptr(),
                                             asc.data_ptr(), out4.data_ptr(), outP.data_ptr(), stream)
    assert st == -1

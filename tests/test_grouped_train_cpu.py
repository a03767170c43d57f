"""Grouped binary convolutions in a training step, the parts that need no GPU: the host functions that state what the
gradient kernels of csrc/grad_grouped.hip cover, the argument validation of their entry points (no launch), and the
training.GROUPED switch leaving CPU tensors on the torch composition."""
import copy
import ctypes
import os

import numpy as np
import torch
import torch.nn as nn

import bnn_amd as bnn
from bnn_amd import fastpath, native, training
from bnn_amd.ops import BasicInputBinarizer, BasicScaleBinarizer, XNORWeightBinarizer
from tests.golden import gen
from tests.golden.grouped_cases import GROUPED_CASES


def desc(N, C, H, W, O, k, stride=1, pad=1, dil=1):
    return native.ConvDesc(N, C, H, W, O, k, k, stride, stride, pad, pad, dil, dil, 0)


def test_the_host_functions_state_what_the_kernels_cover():
    lib = native.require()
    ok, splits = lib.bnn_hip_bconv_grouped_grad_supported, lib.bnn_hip_bconv_grouped_grad_weight_splits
    # every BATS operation: 3x3, pad = dil in {1, 2}, stride 1 or 2, G = 12, Cg in {4, 8, 16, 32}
    for C in (48, 96, 192, 384):
        for dil in (1, 2):
            for stride in (1, 2):
                for N in (1, 5, 256):
                    d = desc(N, C, 32, 32, C, 3, stride, dil, dil)
                    assert ok(ctypes.byref(d), 12) == 1, (C, dil, stride, N)
                    assert 1 <= splits(ctypes.byref(d), 12) <= N
    dw = desc(2, 130, 9, 9, 130, 3, 2, 1)
    assert ok(ctypes.byref(dw), 130) == 1 and 1 <= splits(ctypes.byref(dw), 130) <= 2      # depthwise 3x3 stride 2
    wide = desc(1, 8, 3, 70, 8, 3)
    assert ok(ctypes.byref(wide), 2) == 1 and splits(ctypes.byref(wide), 2) == 1           # wider than a wave; one image
    d = desc(4, 96, 16, 16, 96, 3)
    for groups, why in ((1, "dense"), (7, "C % groups"), (0, "groups"), (-3, "groups")):
        assert ok(ctypes.byref(d), groups) == 0 and splits(ctypes.byref(d), groups) == 0, why
    s3 = desc(4, 96, 16, 16, 96, 3, 3)
    assert ok(ctypes.byref(s3), 12) == 0 and splits(ctypes.byref(s3), 12) == 0             # stride 3
    cg128 = desc(1, 256, 9, 9, 64, 3, 1, 2, 2)
    assert ok(ctypes.byref(cg128), 2) == 0 and splits(ctypes.byref(cg128), 2) == 0         # 128 channels per group
    mixed = native.ConvDesc(4, 96, 16, 16, 96, 3, 3, 1, 2, 1, 1, 1, 1, 0)
    assert ok(ctypes.byref(mixed), 12) == 0                                                # stride_h != stride_w
    k9 = desc(1, 24, 20, 20, 24, 9, 1, 4)
    assert ok(ctypes.byref(k9), 12) == 0                                                   # 9x9 kernel
    assert ok(None, 12) == 0 and splits(None, 12) == 0


def test_argument_validation_without_a_launch():
    lib = native.require()
    gin, gw = lib.bnn_hip_bconv_grouped_grad_input_f32, lib.bnn_hip_bconv_grouped_grad_weight_f32
    d = desc(4, 96, 16, 16, 96, 3)
    r = ctypes.byref(d)
    before = native.launch_count()
    # null and misaligned pointers (fp32 tensors 4 bytes, planes 8 bytes)
    assert gin(r, 12, None, 16, 16, 16, None) == -1 and gin(r, 12, 16, None, 16, 16, None) == -1
    assert gin(r, 12, 16, 16, None, 16, None) == -1 and gin(r, 12, 16, 16, 16, None, None) == -1
    assert gin(r, 12, 18, 16, 16, 16, None) == -1 and gin(r, 12, 16, 16, 20, 16, None) == -1
    assert gw(r, 12, None, 16, 16, 16, 1, None) == -1 and gw(r, 12, 16, None, 16, 16, 1, None) == -1
    assert gw(r, 12, 16, 16, None, 16, 1, None) == -1 and gw(r, 12, 16, 16, 16, None, 1, None) == -1
    assert gw(r, 12, 16, 20, 16, 16, 1, None) == -1 and gw(r, 12, 16, 16, 16, 18, 1, None) == -1
    assert gin(None, 12, 16, 16, 16, 16, None) == -1 and gw(None, 12, 16, 16, 16, 16, 1, None) == -1
    # groups that do not divide C and O, or are not positive: invalid; groups == 1: the dense kernels' business
    for groups, st in ((7, -1), (0, -1), (-12, -1), (1, -2)):
        assert gin(r, groups, 16, 16, 16, 16, None) == st and gw(r, groups, 16, 16, 16, 16, 1, None) == st, groups
    # splits outside 1 .. N
    for s in (0, -1, 5, 1 << 20):
        assert gw(r, 12, 16, 16, 16, 16, s, None) == -1, s
    # valid but not covered: stride 3, 128 channels per group, a 9x9 kernel
    for dd, groups in ((desc(4, 96, 16, 16, 96, 3, 3), 12), (desc(1, 256, 9, 9, 64, 3, 1, 2, 2), 2),
                       (desc(1, 24, 20, 20, 24, 9, 1, 4), 12)):
        assert gin(ctypes.byref(dd), groups, 16, 16, 16, 16, None) == -2
        assert gw(ctypes.byref(dd), groups, 16, 16, 16, 16, 1, None) == -2
    # beyond the 2^30-element addressing of a launch: the status of the other entry points
    big = desc(1 << 15, 384, 32, 32, 384, 3)
    assert gin(ctypes.byref(big), 12, 16, 16, 16, 16, None) == -4 and gw(ctypes.byref(big), 12, 16, 16, 16, 16, 1, None) == -4
    assert lib.bnn_hip_bconv_grouped_grad_supported(ctypes.byref(big), 12) == 0
    assert native.launch_count() == before


def _layer(case, w, b, sc):
    conv = nn.Conv2d(case.C, case.O, (case.kh, case.kw), stride=case.stride, padding=case.pad, dilation=case.dilation,
                     groups=case.groups, bias=case.bias)
    conv.weight.data.copy_(torch.from_numpy(w))
    if b is not None:
        conv.bias.data.copy_(torch.from_numpy(b))
    cfg = bnn.BConfig(activation_pre_process=BasicInputBinarizer,
                      activation_post_process=BasicScaleBinarizer if case.post == "scale" else bnn.Identity,
                      weight_pre_process=XNORWeightBinarizer.with_args(compute_alpha=case.compute_alpha,
                                                                       center_weights=case.center))
    layer = bnn.prepare_binary_model(conv, cfg)
    if sc is not None:
        layer.activation_post_process.alpha.data.copy_(torch.from_numpy(sc).view(1, -1, 1, 1))
    return layer.train()


def test_the_switch_leaves_cpu_tensors_on_the_composition_bit_for_bit():
    assert training.GROUPED is (os.environ.get("BNN_AMD_TRAIN_GROUPED", "0") == "1")      # off unless the environment asks
    previous = training.GROUPED
    for case in (GROUPED_CASES[1], GROUPED_CASES[9]):      # bias; depthwise with BasicScaleBinarizer
        x, w, b, sc = case.tensors()
        off = _layer(case, w, b, sc)
        on = copy.deepcopy(off)
        g = None
        res = []
        launches, stats = native.launch_count(), fastpath.stats()
        for layer, flag in ((off, False), (on, True)):
            training.GROUPED = flag
            try:
                xa = torch.from_numpy(x).requires_grad_()
                y = layer(xa)
                g = torch.from_numpy(gen.normal(3, tuple(y.shape))) if g is None else g
                y.backward(g)
                res.append((y.detach(), xa.grad, [q.grad for q in layer.parameters()]))
            finally:
                training.GROUPED = previous
        assert native.launch_count() == launches and fastpath.stats() == stats      # no native call, no counter moved
        (y0, gx0, p0), (y1, gx1, p1) = res
        assert torch.equal(y0, y1) and torch.equal(gx0, gx1) and len(p0) == len(p1) >= 2
        for a, r in zip(p1, p0):
            assert a is not None and torch.equal(a, r)

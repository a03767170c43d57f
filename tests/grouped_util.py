"""Shared pieces of the grouped-convolution tests: the window layout restated in Python, and the per-group
decomposition of a grouped convolution into dense ones (what the CPU oracle evaluates)."""
from __future__ import annotations

import numpy as np

import oracle


def layout(O, C, G, KH, KW):
    """include/bnn_hip.h, bnn_hip_grouped_weight_layout, by brute force over every 32-channel output block."""
    Cg, Og = C // G, O // G
    nb = (O + 31) // 32
    S = 0
    for ob in range(nb):
        o0, o1 = 32 * ob, min(O, 32 * ob + 32) - 1
        g_lo, g_hi = o0 // Og, o1 // Og
        S = max(S, ((g_hi + 1) * Cg - 1) // 32 - (g_lo * Cg) // 32 + 1)
    return dict(S=S, o_pad=nb * 32, n_words=nb * 32 * KH * KW * S)


def window_pack(w, groups, center=False):
    """The windowed weight words built from oracle.pack_weight of the [O, Cg, KH, KW] weight: (wbits, wnz)."""
    w = np.ascontiguousarray(w, np.float32)
    O, Cg, KH, KW = w.shape
    taps, Og = KH * KW, O // groups
    wb_d, wz_d, _, _ = oracle.pack_weight(w, center, True)
    D = oracle.weight_layout(O, Cg, KH, KW)
    L = layout(O, Cg * groups, groups, KH, KW)
    S = L["S"]
    o = np.arange(O)[:, None, None]
    c = np.arange(Cg)[None, :, None]
    t = np.arange(taps)[None, None, :]
    cw = c // 32
    addr = (((o // 32) * D["nchunk"] + cw // D["cwc"]) * 32 + o % 32) * taps * D["cwc"] + t * D["cwc"] + cw % D["cwc"]
    sh = (c % 32).astype(np.uint32)
    bit = (wb_d[addr] >> sh) & np.uint32(1)
    nzb = (wz_d[addr] >> sh) & np.uint32(1)
    ob = o // 32
    w_lo = ((ob * 32) // Og) * Cg // 32
    cabs = (o // Og) * Cg + c
    s = cabs // 32 - w_lo
    assert (s >= 0).all() and (s < S).all()
    idx = ((ob * taps + t) * S + s) * 32 + o % 32
    shape = np.broadcast(idx, sh).shape
    idx = np.broadcast_to(idx, shape).ravel()
    b = np.broadcast_to((cabs % 32).astype(np.uint32), shape).ravel()
    wb = np.zeros(L["n_words"], np.uint32)
    wz = np.zeros(L["n_words"], np.uint32)
    np.bitwise_or.at(wb, idx, np.broadcast_to(bit, shape).ravel() << b)
    np.bitwise_or.at(wz, idx, np.broadcast_to(nzb, shape).ravel() << b)
    return wb, wz


def per_group(fn, x, w, groups, bias=None, scale=None, **kw):
    """fn(x_g, w_g, bias_g, scale_g, **kw) on each group's channel slices, concatenated along channels."""
    C, O = x.shape[1], w.shape[0]
    Cg, Og = C // groups, O // groups
    outs = []
    for g in range(groups):
        bg = None if bias is None else bias[g * Og:(g + 1) * Og]
        sg = None if scale is None else scale[g * Og:(g + 1) * Og]
        outs.append(fn(x[:, g * Cg:(g + 1) * Cg], w[g * Og:(g + 1) * Og], bg, sg, **kw))
    return np.concatenate(outs, axis=1)


def oracle_dot(x, w, groups, stride, pad, dilation, center):
    """Integer dot of a grouped convolution: oracle.ternary_dot per group on sign(W - mean) (4-D tensors)."""
    def one(xg, wg, _b, _s):
        wsign = oracle.xnor_weight(wg, center, False)[1]
        return oracle.ternary_dot(xg, wsign, stride, pad, dilation)
    return per_group(one, x, w, groups)


def oracle_float(x, w, groups, bias, scale, stride, pad, dilation, center, compute_alpha):
    """Route F of the oracle (the reference forward restated, double accumulation) per group."""
    def one(xg, wg, bg, sg):
        return oracle.binary_conv2d_float(xg, wg, bg, sg, stride, pad, dilation, center, compute_alpha)
    return per_group(one, x, w, groups, bias, scale)


def as_2d(case, x, w):
    """A Conv1d case as its H == 1 two-dimensional convolution: (x, w, stride, pad, dilation)."""
    if case.conv1d:
        return x[:, :, None, :], w[:, :, None, :], (1, case.stride), (0, case.pad[1]), (1, case.dilation)
    return x, w, case.stride, case.pad, case.dilation

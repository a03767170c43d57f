"""The one-launch hierarchical block (csrc/hblock.hip, csrc/hblock_cl.hip) restated from the CPU oracle alone: what
bnn_hip_hblock_forward, _pool_forward and _shortcut_forward write, out of oracle.pack_weight / bconv_dot / epilogue /
fused_epilogue2 / pack_act / avgpool_ceil and no HIP op.  The specification is the launch-by-launch chain of
tests/test_gpu_hblock.py (_launch_by_launch): three slice-writing convolutions with the residual added after the
activation and the pack taken before it, then the next block's packing pass.  Every sign() decision of a BatchNorm in
front of a pack is taken on the affine evaluated in float64 (exact for a float32 value, scale and shift: the sign of
the kernel's fmaf).

Also the block data the tests draw (`draw`): ordinary values with negative BatchNorm scales, exact ties (sign(0) == 0),
saturated packs (every bit set / none) and a residual that cancels the block output exactly."""
from __future__ import annotations

import numpy as np

import oracle

KINDS = ("neg_scales", "ties", "all_set", "none_set", "cancel")


def _col(v):
    return np.asarray(v, np.float64).reshape(1, -1, 1, 1)


def sign_affine(v, a, b, relu):
    """sign(act(v * a + b)) per channel of an [N, C, H, W] float32 tensor, the affine in float64: int8 in {-1, 0, 1}."""
    t = np.asarray(v, np.float32).astype(np.float64) * _col(a) + _col(b)
    if relu:
        t = np.maximum(t, 0.0)
    return np.sign(t).astype(np.int8)


def planes_of(s):
    """(P, M) uint64 planes of a sign tensor."""
    return oracle.pack_act(np.asarray(s, np.float32))


def signs_of(P, M, C):
    """The inverse of planes_of: int8 [N, C, H, W]."""
    c = np.arange(C)
    sh = (c % 64).astype(np.uint64).reshape(1, -1, 1, 1)
    p = (P[:, c // 64] >> sh) & np.uint64(1)
    m = (M[:, c // 64] >> sh) & np.uint64(1)
    return p.astype(np.int8) - m.astype(np.int8)


def _conv(P, M, c_in, w, res, y, c_off):
    """One 3x3 / padding 1 binary convolution into channels c_off.. of y (+ residual after the activation): returns its
    value before the residual, the one the next pack binarises."""
    N, _, H, W = P.shape
    wb, wz, alpha, anyz = oracle.pack_weight(w)
    assert not anyz, "the one-launch block takes no zero weights"
    O = w.shape[0]
    dot = oracle.bconv_dot(P, M, wb, wz, (N, c_in, H, W), w.shape, padding=1)
    _, pre = oracle.fused_epilogue2(dot, alpha[:O], res=res, res_late=True, pack_pre=True, out=y, c_off=c_off)
    return pre


def plain(P_in, ws, bn2, bn3, res, nbn=None):
    """bnn_hip_hblock_forward: ``P_in`` the block's (non-negative) input planes [N, ceil(C_in / 64), H, W] uint64, ``ws``
    the three fp32 weights, ``bn2`` / ``bn3`` / ``nbn`` (scale, shift) of the BatchNorms in front of conv2 / conv3 / the
    next block, ``res`` the fp32 residual.  Returns dict(y, P, M (the next planes, or None), pre (the three values each
    pack binarises: conv1's and conv2's before the residual, y))."""
    P_in = np.ascontiguousarray(P_in, np.uint64)
    res = np.ascontiguousarray(res, np.float32)
    N, planes, H, W = res.shape
    half, quarter = planes // 2, planes // 4
    c_in = ws[0].shape[1]
    y = np.zeros(res.shape, np.float32)
    p1 = _conv(P_in, np.zeros_like(P_in), c_in, ws[0], res, y, 0)
    P1, M1 = planes_of(sign_affine(p1, *bn2, relu=True))
    p2 = _conv(P1, M1, half, ws[1], res, y, half)
    P2, M2 = planes_of(sign_affine(p2, *bn3, relu=True))
    _conv(P2, M2, quarter, ws[2], res, y, half + quarter)
    out = dict(y=y, P=None, M=None, pre=(p1, p2, y))
    if nbn is not None:
        out["P"], out["M"] = planes_of(sign_affine(y, *nbn, relu=True))
    return out


def pool(P_in, ws, bn2, bn3, res, bn1, bn_ds):
    """bnn_hip_hblock_pool_forward: the plain form's y -> AvgPool2d(2, 2) -> (sign(relu(bn1(t))), sign(bn_ds(t))).
    Returns dict(t, P1, M1, P2, M2, y)."""
    y = plain(P_in, ws, bn2, bn3, res)["y"]
    t = oracle.avgpool_ceil(y, 2)
    P1, M1 = planes_of(sign_affine(t, *bn1, relu=True))
    P2, M2 = planes_of(sign_affine(t, *bn_ds, relu=False))
    return dict(t=t, P1=P1, M1=M1, P2=P2, M2=M2, y=y)


def shortcut_residual(P_sc, M_sc, w_sc):
    """The shortcut of a width-changing block: binary conv1x1 of the planes of its BatchNorm -> sign, fp32."""
    N, _, H, W = P_sc.shape
    wb, wz, alpha, anyz = oracle.pack_weight(w_sc)
    assert not anyz
    O, C = w_sc.shape[:2]
    dot = oracle.bconv_dot(np.ascontiguousarray(P_sc, np.uint64), np.ascontiguousarray(M_sc, np.uint64), wb, wz,
                           (N, C, H, W), w_sc.shape)
    return oracle.epilogue(dot, alpha[:O])


def shortcut(P_in, ws, bn2, bn3, P_sc, M_sc, w_sc, nbn):
    """bnn_hip_hblock_shortcut_forward: the plain form on top of the shortcut convolution's output."""
    out = plain(P_in, ws, bn2, bn3, shortcut_residual(P_sc, M_sc, w_sc), nbn)
    return out


# ----------------------------------------------------------------------------------------------------- block data
def _mode(v):
    """Per channel, the value of an [N, C, H, W] tensor that occurs most often in its first image."""
    out = np.empty(v.shape[1], np.float32)
    for c in range(v.shape[1]):
        u, n = np.unique(v[0, c], return_counts=True)
        out[c] = u[np.argmax(n)]
    return out


def draw(seed, c_in, planes, N, H, W, kind, form="plain"):
    """Block data (numpy, fp32) of one of KINDS for the plain, pool or shortcut form: dict(s_in (0 / 1 signs of the
    input), P_in, ws, bn2, bn3, nbn, res | (s_sc, P_sc, M_sc, w_sc) | (bn1, bn_ds)).

    neg_scales: about a third of the channels of every BatchNorm in front of a pack have a negative scale.
    ties:       every weight of a convolution has the magnitude 2^-6 (alpha and alpha * dot exact), power-of-two scales,
                and shifts of -scale * (the most frequent value of that channel): those pixels are exactly 0 in front of
                the sign, which must set neither plane.  The residual is a multiple of 2^-6 (y exact).
    all_set / none_set: shifts of +-1e4 in front of every pack: every bit of every packed word set, or none.
    cancel:     the residual is minus the block output on whole 2 x 2 windows of a quarter of the pixels (y == 0 there),
                and the next BatchNorms shift every other channel by 0: sign(relu(0)) == 0."""
    assert kind in KINDS and form in ("plain", "pool", "shortcut")
    rng = np.random.default_rng(seed)
    half, quarter = planes // 2, planes // 4
    f32 = np.float32
    ties = kind == "ties"

    def weight(o, c, k):
        if ties:
            return (np.where(rng.random((o, c, k, k)) < 0.5, -1.0, 1.0) * 2.0 ** -6).astype(f32)
        w = rng.standard_normal((o, c, k, k)).astype(f32) * f32(0.05)
        w[w == 0] = f32(0.01)
        return w

    def scale(c):
        neg = np.where(np.arange(c) % 3 == 0, -1.0, 1.0)
        if ties:
            return (neg * 2.0 ** rng.integers(-1, 2, c)).astype(f32)
        return (neg * (rng.random(c) + 0.5)).astype(f32)

    def shift(c):
        if kind == "all_set":
            return np.full(c, 1e4, f32)
        if kind == "none_set":
            return np.full(c, -1e4, f32)
        b = (rng.standard_normal(c) * 0.3).astype(f32)
        if kind == "cancel":
            b[::2] = 0.0
        return b

    s_in = (rng.random((N, c_in, H, W)) < 0.5).astype(f32)
    P_in, _ = planes_of(s_in)
    ws = [weight(half, c_in, 3), weight(quarter, half, 3), weight(quarter, quarter, 3)]
    bn2, bn3, nbn = (scale(half), shift(half)), (scale(quarter), shift(quarter)), (scale(planes), shift(planes))
    d = dict(s_in=s_in, P_in=P_in, ws=ws, bn2=bn2, bn3=bn3, nbn=nbn)
    if form == "shortcut":
        s_sc = rng.integers(-1, 2, (N, c_in, H, W)).astype(f32)
        d["s_sc"] = s_sc
        d["P_sc"], d["M_sc"] = planes_of(s_sc)
        d["w_sc"] = weight(planes, c_in, 1)
        res = shortcut_residual(d["P_sc"], d["M_sc"], d["w_sc"])
    elif ties:
        res = (rng.integers(-3, 4, (N, planes, H, W)) * 2.0 ** -6).astype(f32)
    else:
        res = rng.standard_normal((N, planes, H, W)).astype(f32)
    if form == "pool":
        d["bn1"], d["bn_ds"] = (scale(planes), shift(planes)), (scale(planes), shift(planes))
    if ties:   # one stage after the other: each tie is chosen on the values the previous choices produce
        p1 = plain(P_in, ws, bn2, bn3, res)["pre"][0]
        bn2 = d["bn2"] = (bn2[0], -bn2[0] * _mode(p1))
        p2 = plain(P_in, ws, bn2, bn3, res)["pre"][1]
        bn3 = d["bn3"] = (bn3[0], -bn3[0] * _mode(p2))
        y = plain(P_in, ws, bn2, bn3, res)["y"]
        d["nbn"] = (nbn[0], -nbn[0] * _mode(y))
        if form == "pool":
            t = oracle.avgpool_ceil(y, 2)
            d["bn1"] = (d["bn1"][0], -d["bn1"][0] * _mode(t))
            d["bn_ds"] = (d["bn_ds"][0], -d["bn_ds"][0] * _mode(t))
    if kind == "cancel" and form != "shortcut":
        o = plain(P_in, ws, bn2, bn3, np.zeros_like(res))["y"]      # cat(o1, o2, o3): independent of the residual
        win = rng.random((N, 1, (H + 1) // 2, (W + 1) // 2)) < 0.25
        win[0, 0, 0, 0] = True
        mask = np.repeat(np.repeat(win, 2, 2), 2, 3)[:, :, :H, :W] & np.ones((1, planes, 1, 1), bool)
        res = np.where(mask, -o, res).astype(f32)
    if form != "shortcut":
        d["res"] = np.ascontiguousarray(res)
    return d


def run(d, form="plain"):
    """The oracle route of `draw`'s data for one form."""
    if form == "plain":
        return plain(d["P_in"], d["ws"], d["bn2"], d["bn3"], d["res"], d["nbn"])
    if form == "pool":
        return pool(d["P_in"], d["ws"], d["bn2"], d["bn3"], d["res"], d["bn1"], d["bn_ds"])
    return shortcut(d["P_in"], d["ws"], d["bn2"], d["bn3"], d["P_sc"], d["M_sc"], d["w_sc"], d["nbn"])

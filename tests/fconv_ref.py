"""The arithmetic of ``bnn_hip_fconv_fused`` (include/bnn_hip.h) restated in NumPy float32 on the CPU oracle's integer
dot: what the one-launch FactorizedConv kernel has to give bit for bit.  Every float operation is rounded on its own
(``oracle.epilogue`` and ``oracle.bn_act`` are the C restatements of ``fmaf(alpha, dot, bias) [* scale]`` and
``fmaf(v, a, b)``)."""
from __future__ import annotations

import numpy as np

import oracle
from tests.grouped_util import oracle_dot


def prelu(v: np.ndarray, slope) -> np.ndarray:
    """``v >= 0 ? v : slope[c] * v`` in float32 (NaN takes the product, like the kernels' select)."""
    v = v.astype(np.float32)
    if slope is None:
        return v
    with np.errstate(invalid="ignore"):
        return np.where(v >= 0, v, np.asarray(slope, np.float32)[None, :, None, None] * v).astype(np.float32)


def shuffle_add(v: np.ndarray, sg: int, res) -> np.ndarray:
    """``out[:, (o % (C/sg)) sg + o // (C/sg)] = v[:, o]``, then ``res + out``."""
    C = v.shape[1]
    o = np.arange(C)
    dst = (o % (C // sg)) * sg + o // (C // sg) if sg > 1 else o
    out = np.empty_like(v)
    out[:, dst] = v
    return (res.astype(np.float32) + out).astype(np.float32) if res is not None else out


def stage(x: np.ndarray, w: np.ndarray, alpha, bias, scale, slope, stride, pad) -> np.ndarray:
    """One binary convolution on values whose sign is taken: the zero-aware integer dot (``groups = 1``), then
    ``fmaf(alpha, dot, bias) [* scale]`` and the PReLU."""
    dot = oracle_dot(x, w, 1, stride, pad, (1, 1), False)
    return prelu(oracle.epilogue(dot, alpha, bias, scale), slope)


def mid_sign(v: np.ndarray, mid_a, mid_b) -> np.ndarray:
    """``p = fmaf(v, mid_a[c], mid_b[c])``; ``(p > 0) - (p < 0)``: NaN and +-0 give 0, denormals keep their sign."""
    p = oracle.bn_act(v, mid_a, mid_b)
    with np.errstate(invalid="ignore"):
        return ((p > 0).astype(np.float32) - (p < 0).astype(np.float32)).astype(np.float32)


def fconv(xb: np.ndarray, w1: np.ndarray, w2: np.ndarray, alpha1, alpha2, mid_a, mid_b, stride: int, *, bias1=None,
          scale1=None, prelu1=None, bias2=None, scale2=None, prelu2=None, shuffle_groups: int = 1, residual=None):
    """``xb``: the values whose sign the input planes hold (``oracle.bn_act(x, bn1)``); ``w1`` ``[C, C, 1, K]``, ``w2``
    ``[C, C, K, 1]``; ``alpha``: the packs' scales (``[>= C]``).  Returns ``(out, t)``: the launch's result and the
    ternary tensor between the two convolutions."""
    C, K = w1.shape[0], w1.shape[3]
    assert w1.shape == (C, C, 1, K) and w2.shape == (C, C, K, 1)
    v = stage(xb, w1, np.asarray(alpha1, np.float32)[:C], bias1, scale1, prelu1, (1, stride), (0, K // 2))
    t = mid_sign(v, mid_a, mid_b)
    v = stage(t, w2, np.asarray(alpha2, np.float32)[:C], bias2, scale2, prelu2, (stride, 1), (K // 2, 0))
    return shuffle_add(v, shuffle_groups, residual), t

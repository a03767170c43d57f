"""Golden cases of the grouped / depthwise binary convolutions (used by make_golden_grouped.py and the tests)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Tuple

import numpy as np

from . import gen


@dataclass(frozen=True)
class GroupedCase:
    name: str
    N: int
    C: int
    H: int
    W: int
    O: int
    groups: int
    kh: int
    kw: int
    stride: int = 1
    pad: Tuple[int, int] = (0, 0)
    dilation: int = 1
    act: str = "normal"        # gen.activation kind
    winit: str = "kaiming"     # gen.conv_weight kind
    center: bool = False
    compute_alpha: bool = True
    bias: bool = False
    post: str = "identity"     # identity | scale
    conv1d: bool = False       # a Conv1d (H == 1, input [N, C, W])

    @property
    def Cg(self) -> int:
        return self.C // self.groups

    @property
    def xshape(self):
        return (self.N, self.C, self.W) if self.conv1d else (self.N, self.C, self.H, self.W)

    @property
    def wshape(self):
        return (self.O, self.Cg, self.kw) if self.conv1d else (self.O, self.Cg, self.kh, self.kw)

    def tensors(self):
        s = gen.seed_of("grouped", self.name)
        x = gen.activation(self.act, s, self.xshape)
        w = gen.conv_weight(self.winit, s + 11, self.wshape)
        b = (0.1 * gen.normal(s + 12, (self.O,))).astype(np.float32) if self.bias else None
        sc = (0.5 + gen.uniform(s + 13, (self.O,))).astype(np.float32) if self.post == "scale" else None
        return x, w, b, sc


# Cg in {1, 3, 8, 12, 16, 32, 128}; O not a multiple of 32; windows across a 32- and a 64-bit word boundary (C = 144,
# G = 12: groups 24..35 and 60..71; depthwise C = 130); Og = 2 Cg; kernels 1, 3, 5, 7 and 1 x 7; dilation 2, stride 2,
# asymmetric padding; bias, BasicScaleBinarizer, centring, compute_alpha = False, exact-zero weights, inputs with zeros
# and negatives.
GROUPED_CASES = [
    GroupedCase("g2_cg16", 2, 32, 9, 9, 32, 2, 3, 3, pad=(1, 1), act="relu"),
    GroupedCase("g4_cg8_bias", 2, 32, 8, 8, 32, 4, 3, 3, pad=(1, 1), bias=True),
    GroupedCase("g12_cg3_o36", 2, 36, 7, 9, 36, 12, 3, 3, pad=(1, 1), act="sparse"),
    GroupedCase("g12_cg12_k5_c144", 1, 144, 8, 8, 144, 12, 5, 5, pad=(2, 2), center=True),
    GroupedCase("dw130_s2", 2, 130, 9, 9, 130, 130, 3, 3, stride=2, pad=(1, 1), act="negrelu"),
    GroupedCase("g4_cg32_og64_1x1", 2, 128, 5, 5, 256, 4, 1, 1),
    GroupedCase("g2_cg128_dil2", 1, 256, 9, 9, 64, 2, 3, 3, pad=(2, 2), dilation=2, act="relu"),
    GroupedCase("g4_og2cg_1x7", 2, 32, 6, 11, 64, 4, 1, 7, pad=(0, 3)),
    GroupedCase("g12_cg2_k7_zeros", 1, 24, 9, 9, 24, 12, 7, 7, pad=(3, 3), winit="withzeros", center=True),
    GroupedCase("dw48_scale_noalpha", 2, 48, 7, 7, 48, 48, 3, 3, pad=(1, 1), post="scale", compute_alpha=False),
    GroupedCase("g4_stem_like_s2", 2, 40, 12, 12, 80, 4, 3, 3, stride=2, pad=(1, 1), act="special"),
    GroupedCase("g12_conv1d", 2, 24, 1, 20, 48, 12, 1, 3, pad=(0, 1), bias=True, conv1d=True),
]

# The reference's own BATS ops (bnn/models/layers/bats_ops.py): SepConv(C, C, 3, 1, 1, groups=12) and
# DilConv(C, C, 3, 1, 2, 2, groups=12), binarised with prepare_binary_model, eval mode.
OP_C, OP_SHAPE = 48, (2, 48, 10, 10)
OP_CASES = {"sepconv": dict(kernel_size=3, padding=1, dilation=1), "dilconv": dict(kernel_size=3, padding=2, dilation=2)}


def op_input(name: str) -> np.ndarray:
    return gen.activation("normal", gen.seed_of("grouped-op", name), OP_SHAPE)

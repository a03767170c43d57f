"""Golden cases of the two primitives the reference's OPS table has beyond PRIMITIVES (used by make_golden_fconv.py and
the tests): FactorizedConv ('conv_7x1_1x7', bnn/models/layers/bats_ops.py:55-75) and OPS['sep_conv_7x7'], binarised
with prepare_binary_model, eval mode."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import gen


@dataclass(frozen=True)
class FconvCase:
    name: str
    kind: str                  # conv_7x1_1x7 | sep_conv_7x7
    C: int
    stride: int
    N: int
    H: int
    W: int
    affine: bool = True
    salt: int = 0              # changes the seed (a case whose BatchNorm margin came out too small)

    @property
    def xshape(self):
        return (self.N, self.C, self.H, self.W)

    def build(self, ns):
        """The float module from the op table of ``ns`` (the reference's bats_ops module, or bnn_amd.models)."""
        table = getattr(ns, "ALL_OPS", None) or ns.OPS
        return table[self.kind](self.C, self.stride, self.affine, True, 12)

    @property
    def seed(self) -> int:
        return gen.seed_of("fconv", self.name, self.salt)

    def input(self) -> np.ndarray:
        return gen.activation("normal", self.seed, self.xshape)

    def state(self, shapes: dict) -> dict:
        return gen.model_state(shapes, self.seed)


# FactorizedConv at C 48 / 80 / 96, stride 1 (skip) and 2, odd sizes, an image smaller than the kernel both ways,
# affine=False; sep_conv_7x7 at both strides.
FCONV_CASES = [
    FconvCase("f7_c48", "conv_7x1_1x7", 48, 1, 2, 9, 10),
    FconvCase("f7_c96_s2", "conv_7x1_1x7", 96, 2, 2, 10, 9),
    FconvCase("f7_c48_s2", "conv_7x1_1x7", 48, 2, 2, 7, 8),
    FconvCase("f7_c80", "conv_7x1_1x7", 80, 1, 2, 7, 7),
    FconvCase("f7_c48_small", "conv_7x1_1x7", 48, 1, 3, 3, 5),
    FconvCase("f7_c96_noaffine", "conv_7x1_1x7", 96, 1, 2, 8, 8, affine=False),
    FconvCase("sep7_c48", "sep_conv_7x7", 48, 1, 2, 8, 8),
    FconvCase("sep7_c48_s2", "sep_conv_7x7", 48, 2, 2, 8, 8),
]
FACTORIZED = [c for c in FCONV_CASES if c.kind == "conv_7x1_1x7"]
SEP7 = [c for c in FCONV_CASES if c.kind == "sep_conv_7x7"]

MIN_BN_MARGIN = 1e-5       # min |bn(.)| in front of every sign(): no sign() depends on how BatchNorm is rounded


def folded_bn64(state: dict, prefix: str, eps: float = 1e-5):
    """(scale, shift) of an eval-mode BatchNorm of the state dict in float64."""
    var, mean = state[prefix + "running_var"].astype(np.float64), state[prefix + "running_mean"].astype(np.float64)
    gamma = state.get(prefix + "weight", np.ones_like(var)).astype(np.float64)
    beta = state.get(prefix + "bias", np.zeros_like(var)).astype(np.float64)
    scale = gamma / np.sqrt(var + eps)
    return scale, beta - mean * scale


def bn_margin(v: np.ndarray, state: dict, prefix: str) -> float:
    """min |scale v + shift| in float64."""
    a, b = folded_bn64(state, prefix)
    return float(np.abs(v.astype(np.float64) * a[None, :, None, None] + b[None, :, None, None]).min())

"""Golden cases of the BATS cell operations (used by make_golden_cellops.py and the tests): the reference's SepConv /
DilConv / ReLUConvBN (bnn/models/layers/bats_ops.py:78-173), binarised with prepare_binary_model, eval mode."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import gen


@dataclass(frozen=True)
class CellCase:
    name: str
    kind: str                  # SepConv | DilConv | ReLUConvBN
    C_in: int
    C_out: int
    k: int
    stride: int
    pad: int
    dilation: int = 1
    affine: bool = True
    H: int = 8
    W: int = 8
    N: int = 2

    @property
    def xshape(self):
        return (self.N, self.C_in, self.H, self.W)

    def build(self, ns):
        """The float module from the classes of ``ns`` (the reference's bats_ops module, or bnn_amd.models)."""
        if self.kind == "SepConv":
            return ns.SepConv(self.C_in, self.C_out, self.k, self.stride, self.pad, affine=self.affine, groups=12)
        if self.kind == "DilConv":
            return ns.DilConv(self.C_in, self.C_out, self.k, self.stride, self.pad, self.dilation, affine=self.affine,
                              groups=12)
        return ns.ReLUConvBN(self.C_in, self.C_out, self.k, self.stride, self.pad, affine=self.affine)

    @property
    def seed(self) -> int:
        return gen.seed_of("cellops", self.name)

    def input(self) -> np.ndarray:
        return gen.activation("normal", self.seed, self.xshape)

    def state(self, shapes: dict) -> dict:
        return gen.model_state(shapes, self.seed)


# 3x3 and 5x5 SepConv, 3x3 (d2, p2) and 5x5 (d2, p4) DilConv at stride 1 (skip); one of each at stride 2 (no skip, odd H
# or W); ReLUConvBN 1x1 with C_in == C_out (skip) and 3x3 with C_in != C_out (no skip); affine=False; C in {48, 96}.
CELL_CASES = [
    CellCase("sep3_c48", "SepConv", 48, 48, 3, 1, 1, H=10, W=10),
    CellCase("sep5_c96", "SepConv", 96, 96, 5, 1, 2, H=8, W=9),
    CellCase("dil3_c48", "DilConv", 48, 48, 3, 1, 2, 2, H=10, W=10),
    CellCase("dil5_c96", "DilConv", 96, 96, 5, 1, 4, 2, H=9, W=8),
    CellCase("sep3_s2_c48", "SepConv", 48, 48, 3, 2, 1, H=9, W=10),
    CellCase("dil3_s2_c96", "DilConv", 96, 96, 3, 2, 2, 2, H=10, W=9),
    CellCase("rcb1_c48_keep", "ReLUConvBN", 48, 48, 1, 1, 0, H=9, W=9),
    CellCase("rcb3_c48_c96", "ReLUConvBN", 48, 96, 3, 1, 1, H=8, W=8),
    CellCase("sep3_c96_noaffine", "SepConv", 96, 96, 3, 1, 1, affine=False, H=7, W=9),
]

MIN_BN_MARGIN = 1e-5       # min |bn(x)| over a case's input: no sign() depends on how BatchNorm is rounded


def folded_bn(state: dict, eps: float = 1e-5):
    """(scale, shift) of the operation's eval-mode BatchNorm as fp32 vectors, rounded as the reference's forward rounds
    them: scale = gamma / sqrt(var + eps), shift = fma(-mean, scale, beta)."""
    var, mean = state["op.0.running_var"], state["op.0.running_mean"]
    gamma = state.get("op.0.weight", np.ones_like(var))
    beta = state.get("op.0.bias", np.zeros_like(var))
    scale = (gamma * (np.float32(1.0) / np.sqrt(var + np.float32(eps), dtype=np.float32))).astype(np.float32)
    shift = (beta.astype(np.float64) - mean.astype(np.float64) * scale.astype(np.float64)).astype(np.float32)
    return scale, shift


def bn_margin(x: np.ndarray, state: dict) -> float:
    """min |scale x + shift| in float64."""
    a, b = folded_bn(state)
    return float(np.abs(x.astype(np.float64) * a.astype(np.float64)[None, :, None, None]
                        + b.astype(np.float64)[None, :, None, None]).min())

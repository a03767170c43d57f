"""The BATS cell operations in two launches (reference: ``bnn/models/layers/bats_ops.py:78-173``).

``SepConv`` / ``DilConv`` / ``ReLUConvBN`` all have the form

    y = [x +] channel_shuffle(PReLU(conv(sign(BatchNorm(x)))), 4)        # skip only at stride 1; ReLUConvBN: no shuffle

``FusedCellOp(module)`` evaluates one of them as ``bn_act_pack`` (BatchNorm + sign -> bit planes, one pass over x) and ONE
convolution launch whose epilogue applies the PReLU, stores through the shuffle permutation and adds the skip
(``bnn_hip_bconv2d_grouped_fused``, csrc/bconv_grouped.hip; the dense ``ReLUConvBN`` takes ``bnn_hip_bconv2d_fused``):
three fp32 passes over HBM (x read by the pack, x read as the skip, y written) instead of about eleven.  The per-layer
path — torch BatchNorm, ``pack_act``, the grouped kernel, torch PReLU, the ``.contiguous()`` shuffle copy, torch add —
stays what every call outside ``eval()`` / ``no_grad()`` runs.
"""
from __future__ import annotations

import itertools
from typing import Optional

import torch
import torch.nn as nn

from . import fastpath, hipops, native
from .executor import FusionError, fold_bn

CELL_OP_NAMES = ("SepConv", "DilConv", "ReLUConvBN")
SHUFFLE_GROUPS = 4      # channel_shuffle(., 4) in SepConv.forward / DilConv.forward


def _pair_of(v, what: str):
    if isinstance(v, int):
        return (v, v)
    if isinstance(v, (tuple, list)) and len(v) == 2 and all(isinstance(e, int) for e in v):
        return tuple(v)
    raise FusionError(f"cell op: {what}={v!r} is not numeric")


class FusedCellOp(nn.Module):
    """Inference executor of one BATS cell operation.  Recognition is by structure — the class NAME must be one of
    ``SepConv`` / ``DilConv`` / ``ReLUConvBN`` and ``module.op`` must be ``Sequential(BatchNorm2d, binary Conv2d,
    PReLU)`` with ``stride`` / ``skip`` as those classes define them — so an instance of the reference's own classes,
    handed over explicitly, works as well as one of ``bnn_amd.models``.  Anything else raises ``FusionError``.

    Derived data (folded BatchNorm, the PReLU slopes as a vector of ``O``, the packed weight) is keyed on the identity,
    storage and version of every parameter and buffer and re-derived when one changes; writes through ``.data`` need
    ``refresh()`` (or ``fastpath.invalidate(module)`` for the executor ``module(x)`` dispatches to)."""

    def __init__(self, module: nn.Module) -> None:
        super().__init__()
        self.model = module
        self._sig = None
        self.refresh()

    # ---- recognition ------------------------------------------------------------------------------------------------
    def _recognise(self) -> None:
        m = self.model
        kind = type(m).__name__
        if kind not in CELL_OP_NAMES:
            raise FusionError(f"{kind} is not a BATS cell operation ({', '.join(CELL_OP_NAMES)})")
        op = getattr(m, "op", None)
        if not (isinstance(op, nn.Sequential) and len(op) == 3 and isinstance(op[0], nn.BatchNorm2d)
                and isinstance(op[1], nn.Conv2d) and hasattr(op[1], "activation_pre_process")
                and isinstance(op[2], nn.PReLU)):
            raise FusionError(f"{kind}.op is not Sequential(BatchNorm2d, binary Conv2d, PReLU) "
                              "(run prepare_binary_model first)")
        bn, conv, act = op
        if m.training:
            raise FusionError("FusedCellOp is inference-only: call .eval() first")
        if bn.running_mean is None or bn.running_var is None:
            raise FusionError("cell op: BatchNorm2d without running statistics normalises with batch statistics")
        plan = fastpath._recognise(conv, conv.out_channels)
        if plan is None:
            raise FusionError("cell op: layer recipe is not BasicInputBinarizer + XNORWeightBinarizer "
                              "(+ Identity | BasicScaleBinarizer)")
        if isinstance(conv.padding, str) or conv.padding_mode != "zeros":
            raise FusionError(f"cell op: padding={conv.padding!r}, padding_mode={conv.padding_mode!r} is not covered")
        if conv.weight.dtype != torch.float32 or bn.running_var.dtype != torch.float32:
            raise FusionError("cell op: only float32 modules are covered")
        stride = _pair_of(getattr(m, "stride", None), "stride")
        if stride != tuple(conv.stride) or stride[0] != stride[1]:
            raise FusionError(f"cell op: {kind}.stride={m.stride!r} is not the convolution's {tuple(conv.stride)}")
        if not isinstance(getattr(m, "skip", None), bool):
            raise FusionError(f"cell op: {kind}.skip is not a bool")
        C, O = conv.in_channels, conv.out_channels
        if bn.num_features != C or act.weight.numel() not in (1, O):
            raise FusionError("cell op: BatchNorm2d / PReLU widths do not fit the convolution")
        if kind == "ReLUConvBN":
            if conv.groups != 1 or getattr(m, "C_in", None) != C or getattr(m, "C_out", None) != O:
                raise FusionError("cell op: ReLUConvBN with groups != 1 or C_in / C_out unlike its convolution")
            self._add_skip = m.skip and stride[0] == 1 and C == O
            self._shuffle = 1
        else:
            if C != O or O % SHUFFLE_GROUPS or conv.groups < 2:
                raise FusionError(f"cell op: {kind} needs C_in == C_out, a multiple of {SHUFFLE_GROUPS}, and groups > 1")
            self._add_skip = m.skip and stride[0] == 1
            self._shuffle = SHUFFLE_GROUPS
        self._plan = plan
        self._grouped = conv.groups != 1

    # ---- derived data -----------------------------------------------------------------------------------------------
    def _signature(self):
        return tuple((id(t), t.data_ptr(), t._version)
                     for t in itertools.chain(self.model.parameters(), self.model.buffers()))

    def _unchanged(self) -> bool:
        return self._sig is not None and not self.model.training and self._signature() == self._sig

    def refresh(self) -> None:
        """Re-derive everything from the module's current parameters and buffers."""
        self._sig = None
        self._recognise()
        bn, conv, act = self.model.op
        fastpath.invalidate(self.model, executors=False)
        self._bn_a, self._bn_b = fold_bn(bn)
        O = conv.out_channels
        slope = act.weight.detach().float().reshape(-1)
        self._prelu = (slope.expand(O) if slope.numel() == 1 else slope).clone()     # a snapshot, like the other two
        self._weight: Optional[hipops.PackedWeight] = None
        if conv.weight.is_cuda:
            native.require()
            self._weight = fastpath.packed_weight(conv, self._plan)
        self._sig = self._signature()

    # ---- forward ----------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4):
            raise FusionError("cell op: the input must be a float32 NCHW tensor on a HIP device")
        if not self._unchanged():
            self.refresh()
        conv = self.model.op[1]
        if self._weight is None or conv.weight.device != x.device:
            raise FusionError("cell op: module and input live on different devices")
        act = hipops.bn_act_pack(x, self._bn_a, self._bn_b, relu=False)
        res = x if self._add_skip else None
        if self._grouped:
            y = hipops.bconv2d_grouped_fused(act, self._weight, fastpath._f32(conv.bias), fastpath._f32(self._plan.scale),
                                             conv.stride, conv.padding, conv.dilation, prelu=self._prelu,
                                             shuffle_groups=self._shuffle, residual=res)
        else:       # ReLUConvBN: the dense convolution's own epilogue has PReLU and the late residual
            y, _ = hipops.bconv2d_fused(act, self._weight, bias=conv.bias, post_scale=self._plan.scale,
                                        prelu=self._prelu, residual=res, residual_after_act=True, stride=conv.stride,
                                        padding=conv.padding, dilation=conv.dilation)
        fastpath._bump("cell_op")
        return y

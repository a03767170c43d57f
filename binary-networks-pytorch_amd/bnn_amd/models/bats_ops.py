"""The BATS cell operations built on grouped binary convolutions (``bnn/models/layers/bats_ops.py``):
``SepConv``, ``DilConv`` and ``ReLUConvBN``, the dense ``FactorizedConv``, and what a cell needs around them —
``FactorizedReduce``, ``Zero``, ``drop_path``, ``Genotype`` / ``PRIMITIVES`` / ``OPS`` / ``EXTENDED_OPS`` / ``ALL_OPS``.

Plain float ``nn.Module`` graphs, like ``blocks.py``: the ``nn.Conv2d`` inside becomes a binary layer only after
``prepare_binary_model``.  Constructor signatures, attribute names and forward order equal the reference's, so
``state_dict`` keys (``op.0.*``, ``op.1.weight``, ``op.2.weight``) are interchangeable and outputs can be pinned against
fixtures generated from the reference.  Every operation has the form

    y = [x +] channel_shuffle(PReLU(conv(BatchNorm(x))), 4)          # skip only at stride 1; ReLUConvBN: no shuffle

and, evaluated for inference on a HIP device, first offers itself to the cell-operation executor
(``bnn_amd/dispatch.py: OpFusion`` -> ``bnn_amd/cellops.py: FusedCellOp``); in ``train()`` mode under autograd, with
``training.CELL_OPS`` on, to the training executor (``bnn_amd/training.py: cell_op_train`` -> ``CellOpTrainFn``;
``FactorizedReduce``: ``reduce_train`` -> ``ReduceTrainFn``).
"""
from __future__ import annotations

from collections import namedtuple

import torch
import torch.nn as nn

Genotype = namedtuple("Genotype", "normal normal_concat reduce reduce_concat")

PRIMITIVES = ["none", "max_pool_3x3", "avg_pool_3x3", "skip_connect", "sep_conv_3x3", "sep_conv_5x5", "dil_conv_3x3",
              "dil_conv_5x5"]


def channel_shuffle(x: torch.Tensor, groups: int) -> torch.Tensor:
    """Output channel ``(o % (C / groups)) * groups + o // (C / groups)`` is input channel ``o``: the ``groups`` runs of
    ``C / groups`` channels interleaved."""
    n, c, h, w = x.shape
    return x.reshape(n, groups, c // groups, h, w).transpose(1, 2).reshape(n, c, h, w)


def _fused(op, x):
    from ..inference import auto_op_forward         # (inference imports this package)
    return auto_op_forward(op, x)


class _CellOp(nn.Module):
    """``BatchNorm2d -> Conv2d -> PReLU`` as ``self.op``; the subclasses say what happens around it (``_forward``)."""

    def __init__(self, C_in: int, C_out: int, kernel_size: int, stride: int, padding: int, dilation: int, affine: bool,
                 skip: bool, groups: int) -> None:
        super().__init__()
        self.skip = skip or True        # (the reference's expression: every operation has its skip connection)
        self.stride = stride
        self.op = nn.Sequential(
            nn.BatchNorm2d(C_in, affine=affine),
            nn.Conv2d(C_in, C_out, kernel_size, stride=stride, padding=padding, dilation=dilation, groups=groups,
                      bias=False),
            nn.PReLU(num_parameters=C_out))

    def train(self, mode: bool = True):
        # train() <-> eval(): the executor's derived data goes with the mode (models/blocks.py: _Residual.train)
        if bool(mode) != self.training:
            from ..fastpath import drop_executor
            drop_executor(self)
        return super().train(mode)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if not self.training and x.is_cuda and not torch.is_grad_enabled():
            y = _fused(self, x)
            if y is not None:
                return y
        if self.training and torch.is_grad_enabled():
            from .. import training                 # (training imports hipops; this package stays importable alone)
            if training.CELL_OPS:       # read at every call; None: the rule of training.cell_op_train declined
                y = training.cell_op_train(self, x)
                if y is not None:
                    return y
        return self._forward(x)

    def _forward(self, x: torch.Tensor) -> torch.Tensor:
        y = channel_shuffle(self.op(x), 4)
        return x + y if self.skip and self.stride == 1 else y


class SepConv(_CellOp):
    """BN - grouped conv - PReLU, channel shuffle, skip at stride 1   (reference: ``bats_ops.py:148-173``)."""

    def __init__(self, C_in: int, C_out: int, kernel_size: int, stride: int, padding: int, affine: bool = True,
                 skip: bool = False, groups: int = 12) -> None:
        super().__init__(C_in, C_in, kernel_size, stride, padding, 1, affine, skip, groups)   # (C_out unused there too)


class DilConv(_CellOp):
    """The same with a dilated convolution   (reference: ``bats_ops.py:108-145``)."""

    def __init__(self, C_in: int, C_out: int, kernel_size: int, stride: int, padding: int, dilation: int,
                 affine: bool = True, skip: bool = False, groups: int = 12) -> None:
        super().__init__(C_in, C_in, kernel_size, stride, padding, dilation, affine, skip, groups)


class ReLUConvBN(_CellOp):
    """BN - dense conv - PReLU, skip when the shape is kept, no shuffle   (reference: ``bats_ops.py:78-105``)."""

    def __init__(self, C_in: int, C_out: int, kernel_size: int, stride: int, padding: int, affine: bool = True,
                 skip: bool = False) -> None:
        super().__init__(C_in, C_out, kernel_size, stride, padding, 1, affine, skip, 1)
        self.C_in = C_in
        self.C_out = C_out

    def _forward(self, x: torch.Tensor) -> torch.Tensor:
        y = self.op(x)
        return x + y if self.skip and self.stride == 1 and self.C_in == self.C_out else y


class FactorizedConv(nn.Module):
    """BN - dense 1 x K conv, stride (1, s) - PReLU - BN - dense K x 1 conv, stride (s, 1) - PReLU, channel shuffle, skip
    at stride 1   (reference: ``bats_ops.py:55-75``, the ``'conv_7x1_1x7'`` primitive).  Evaluated for inference on a HIP
    device it first offers itself to its executor (``bnn_amd/dispatch.py: FactorizedFusion`` ->
    ``bnn_amd/cellops.py: FusedFactorizedConv``: both convolutions in one launch, the sign between them in LDS); in
    training mode and under autograd its two layers take their per-layer paths."""

    def __init__(self, C: int, kernel_size: int, stride: int, affine: bool = True, skip: bool = False) -> None:
        super().__init__()
        self.skip = skip or True        # (the reference's expression, as in _CellOp)
        self.stride = stride
        self.op = nn.Sequential(
            nn.BatchNorm2d(C, affine=affine),
            nn.Conv2d(C, C, (1, kernel_size), stride=(1, stride), padding=(0, kernel_size // 2), bias=False),
            nn.PReLU(num_parameters=C),
            nn.BatchNorm2d(C, affine=affine),
            nn.Conv2d(C, C, (kernel_size, 1), stride=(stride, 1), padding=(kernel_size // 2, 0), bias=False),
            nn.PReLU(num_parameters=C))

    def train(self, mode: bool = True):
        # train() <-> eval(): the executor's derived data goes with the mode (_CellOp.train)
        if bool(mode) != self.training:
            from ..fastpath import drop_executor
            drop_executor(self)
        return super().train(mode)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if not self.training and x.is_cuda and not torch.is_grad_enabled():
            from ..inference import auto_fconv_forward      # (inference imports this package)
            y = auto_fconv_forward(self, x)
            if y is not None:
                return y
        y = channel_shuffle(self.op(x), 4)
        return x + y if self.skip and self.stride == 1 else y


class Zero(nn.Module):
    """The ``none`` primitive: zeros of the input's shape, ``H`` and ``W`` floor-divided by the stride   (reference:
    ``bats_ops.py:176-187``; fp32 there whatever the input's dtype, the same here)."""

    def __init__(self, stride: int) -> None:
        super().__init__()
        self.stride = stride

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        n, c, h, w = x.size()
        return torch.zeros(n, c, h // self.stride, w // self.stride, dtype=torch.float32, device=x.device)


class FactorizedReduce(nn.Module):
    """BN - two 1x1 stride-2 convolutions, on the pixels ``(2i, 2j)`` and ``(2i+1, 2j+1)`` - concat - PReLU   (reference:
    ``bats_ops.py:190-209``).  ``H`` and ``W`` must be even for the two halves to have one shape."""

    def __init__(self, C_in: int, C_out: int, affine: bool = True) -> None:
        super().__init__()
        assert C_out % 2 == 0
        self.activation = nn.PReLU(num_parameters=C_out)
        self.conv_1 = nn.Sequential(nn.Conv2d(C_in, C_out // 2, 1, stride=2, padding=0, bias=False))
        self.conv_2 = nn.Sequential(nn.Conv2d(C_in, C_out // 2, 1, stride=2, padding=0, bias=False))
        self.bn = nn.BatchNorm2d(C_in, affine=affine)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.training and torch.is_grad_enabled():
            from .. import training                 # (see _CellOp.forward)
            if training.CELL_OPS:       # read at every call; None: the rule of training.reduce_train declined
                y = training.reduce_train(self, x)
                if y is not None:
                    return y
        x = self.bn(x)
        out = torch.cat([self.conv_1(x), self.conv_2(x[:, :, 1:, 1:])], dim=1)
        return self.activation(out)


def drop_path(x: torch.Tensor, drop_prob: float) -> torch.Tensor:
    """Drop whole samples of a branch with probability ``drop_prob`` and rescale the kept ones, in place: a Bernoulli
    mask of shape ``[N, 1, 1, 1]``.  The reference's version (``bats_ops.py:33-39``) builds the mask with
    ``torch.tensor(x.size(0), 1, 1, 1)``, which raises a ``TypeError``; this one does what that line means.  Only
    ``Cell.forward`` in training mode calls it."""
    if drop_prob > 0.:
        keep_prob = 1. - drop_prob
        mask = torch.empty(x.size(0), 1, 1, 1, dtype=x.dtype, device=x.device).bernoulli_(keep_prob)
        x.div_(keep_prob)
        x.mul_(mask)
    return x


# primitive name -> constructor(C, stride, affine, skip, groups)   (reference: ``bats_ops.py:41-52``).  OPS holds the
# eight names of PRIMITIVES, the search space; the reference's table has two more that no entry of PRIMITIVES names,
# 'sep_conv_7x7' and 'conv_7x1_1x7': EXTENDED_OPS.  A genotype may name any of the ten: Cell._compile reads ALL_OPS.
OPS = {
    "none": lambda C, stride, affine, skip, groups: Zero(stride),
    "avg_pool_3x3": lambda C, stride, affine, skip, groups: nn.AvgPool2d(3, stride=stride, padding=1,
                                                                           count_include_pad=False),
    "max_pool_3x3": lambda C, stride, affine, skip, groups: nn.MaxPool2d(3, stride=stride, padding=1),
    "skip_connect": lambda C, stride, affine, skip, groups: (nn.Identity() if stride == 1
                                                             else FactorizedReduce(C, C, affine=affine)),
    "sep_conv_3x3": lambda C, stride, affine, skip, groups: SepConv(C, C, 3, stride, 1, affine=affine, skip=skip,
                                                                    groups=groups),
    "sep_conv_5x5": lambda C, stride, affine, skip, groups: SepConv(C, C, 5, stride, 2, affine=affine, skip=skip,
                                                                    groups=groups),
    "dil_conv_3x3": lambda C, stride, affine, skip, groups: DilConv(C, C, 3, stride, 2, 2, affine=affine, skip=skip,
                                                                    groups=groups),
    "dil_conv_5x5": lambda C, stride, affine, skip, groups: DilConv(C, C, 5, stride, 4, 2, affine=affine, skip=skip,
                                                                    groups=groups),
}

EXTENDED_OPS = {
    "sep_conv_7x7": lambda C, stride, affine, skip, groups: SepConv(C, C, 7, stride, 3, affine=affine, skip=skip,
                                                                    groups=groups),
    "conv_7x1_1x7": lambda C, stride, affine, skip, groups: FactorizedConv(C, 7, stride, affine=affine, skip=skip),
}

ALL_OPS = {**OPS, **EXTENDED_OPS}

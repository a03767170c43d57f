"""The BATS cell operations built on grouped binary convolutions (``bnn/models/layers/bats_ops.py:20-30,
78-173``): ``SepConv``, ``DilConv`` and ``ReLUConvBN``.

Plain float ``nn.Module`` graphs, like ``blocks.py``: the ``nn.Conv2d`` inside becomes a binary layer only after
``prepare_binary_model``.  Constructor signatures, attribute names and forward order equal the reference's, so
``state_dict`` keys (``op.0.*``, ``op.1.weight``, ``op.2.weight``) are interchangeable and outputs can be pinned against
fixtures generated from the reference.  Every operation has the form

    y = [x +] channel_shuffle(PReLU(conv(BatchNorm(x))), 4)          # skip only at stride 1; ReLUConvBN: no shuffle

and, evaluated for inference on a HIP device, first offers itself to the cell-operation executor
(``bnn_amd/dispatch.py: OpFusion`` -> ``bnn_amd/cellops.py: FusedCellOp``).
"""
from __future__ import annotations

import torch
import torch.nn as nn


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
            self.__dict__.pop("_bnn_auto_op", None)
        return super().train(mode)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if not self.training and x.is_cuda and not torch.is_grad_enabled():
            y = _fused(self, x)
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

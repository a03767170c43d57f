"""The BATS networks (``bnn/models/bats.py``): ``Cell``, ``AuxiliaryHead``, ``BATSNetworkCIFAR`` and
``BATSNetworkImageNet``.

Plain float ``nn.Module`` graphs like ``bats_ops.py`` / ``blocks.py``: constructor signatures, attribute names, forward
order and ``state_dict`` keys equal the reference's, and the convolutions become binary layers through
``prepare_binary_model``.  A ``Cell`` evaluated for inference on a HIP device first offers itself to the cell executor
(``bnn_amd/dispatch.py: CellFusion`` -> ``bnn_amd/cellops.py: FusedCell``), which runs the whole cell — preprocessing,
every node's two operations and their sum, the concatenation — as fused launches.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch
import torch.nn as nn

from .bats_ops import ALL_OPS, FactorizedReduce, Genotype, ReLUConvBN, drop_path


def _fused(cell, s0, s1):
    from ..inference import auto_cell_forward       # (inference imports this package)
    return auto_cell_forward(cell, s0, s1)


class Cell(nn.Module):
    """Two preprocessed input states, ``len(ops) / 2`` nodes ``s = op1(states[i]) + op2(states[j])``, the states named by
    the genotype's concat list joined along the channels   (reference: ``bats.py:9-83``)."""

    def __init__(self, genotype: Genotype, C_prev_prev: int, C_prev: int, C: int, reduction: bool, reduction_prev: bool,
                 groups: int = 12, use_shake_shake: bool = False) -> None:
        super().__init__()
        self.use_shake_shake = use_shake_shake
        if reduction_prev:
            self.preprocess0 = FactorizedReduce(C_prev_prev, C)
        else:
            self.preprocess0 = ReLUConvBN(C_prev_prev, C, 1, 1, 0)
        self.preprocess1 = ReLUConvBN(C_prev, C, 1, 1, 0)
        if reduction:
            op_names, indices = zip(*genotype.reduce)
            concat = genotype.reduce_concat
        else:
            op_names, indices = zip(*genotype.normal)
            concat = genotype.normal_concat
        self._compile(C, op_names, indices, concat, reduction, groups)

    def _compile(self, C: int, op_names: List[str], indices: List[int], concat: List[int], reduction: bool,
                 groups: int) -> None:
        assert len(op_names) == len(indices)
        self._steps = len(op_names) // 2
        self._concat = concat
        self.multiplier = len(concat)
        self._ops = nn.ModuleList()
        for name, index in zip(op_names, indices):
            stride = 2 if reduction and index < 2 else 1
            self._ops += [ALL_OPS[name](C, stride, True, True, groups)]
        self._indices = indices

    def train(self, mode: bool = True):
        # train() <-> eval(): the executor's derived data goes with the mode (bats_ops.py: _CellOp.train)
        if bool(mode) != self.training:
            from ..fastpath import drop_executor
            drop_executor(self)
        return super().train(mode)

    def forward(self, s0: torch.Tensor, s1: torch.Tensor, drop_prob: float = 0.0) -> torch.Tensor:
        if not self.training and s0.is_cuda and not torch.is_grad_enabled():
            y = _fused(self, s0, s1)
            if y is not None:
                return y
        s0 = self.preprocess0(s0)
        s1 = self.preprocess1(s1)
        states = [s0, s1]
        for i in range(self._steps):
            op1, op2 = self._ops[2 * i], self._ops[2 * i + 1]
            h1 = op1(states[self._indices[2 * i]])
            h2 = op2(states[self._indices[2 * i + 1]])
            if self.training and drop_prob > 0.:
                if not isinstance(op1, nn.Identity):
                    h1 = drop_path(h1, drop_prob)
                if not isinstance(op2, nn.Identity):
                    h2 = drop_path(h2, drop_prob)
            states += [h1 + h2]
        if self.use_shake_shake:
            if self.training:
                shake = torch.softmax(torch.zeros(len(self._concat)).uniform_(), dim=0)
                return torch.cat([states[i] * shake[j].item() for j, i in enumerate(self._concat)], dim=1)
            return torch.cat([states[i] * (1 / len(self._concat)) for i in self._concat], dim=1)
        return torch.cat([states[i] for i in self._concat], dim=1)


class AuxiliaryHead(nn.Module):
    """The training-time auxiliary classifier   (reference: ``bats.py:86-105``)."""

    def __init__(self, C: int, num_classes: int, stride: int) -> None:
        super().__init__()
        self.features = nn.Sequential(
            nn.AvgPool2d(5, stride=stride, padding=0, count_include_pad=False),
            nn.BatchNorm2d(C),
            nn.Conv2d(C, 128, 1, bias=False),
            nn.PReLU(num_parameters=128),
            nn.BatchNorm2d(128),
            nn.Conv2d(128, 768, 2, bias=False),
            nn.PReLU(num_parameters=768),
        )
        self.classifier = nn.Linear(768, num_classes)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = self.features(x)
        return self.classifier(x.view(x.size(0), -1))


class _BATSNetwork(nn.Module):
    """The cell stack and the head both networks share; ``drop_path_prob`` is set by the training script, as in the
    reference (its forward reads the attribute and the constructor does not create it)."""

    def _build_cells(self, C_prev_prev: int, C_prev: int, C_curr: int, layers: int, genotype, groups: int,
                     reduction_prev: bool) -> Tuple[int, int]:
        self.cells = nn.ModuleList()
        C_to_auxiliary = C_prev
        for i in range(layers):
            reduction = i in [layers // 3, 2 * layers // 3]
            if reduction:
                C_curr *= 2
            cell = Cell(genotype, C_prev_prev, C_prev, C_curr, reduction, reduction_prev, groups)
            reduction_prev = reduction
            self.cells += [cell]
            C_prev_prev, C_prev = C_prev, cell.multiplier * C_curr
            if i == 2 * layers // 3:
                C_to_auxiliary = C_prev
        return C_prev, C_to_auxiliary

    def _run_cells(self, s0: torch.Tensor, s1: torch.Tensor) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        logits_aux = None
        for i, cell in enumerate(self.cells):
            s0, s1 = s1, cell(s0, s1, self.drop_path_prob)
            if i == 2 * self._layers // 3 and self._auxiliary and self.training:
                logits_aux = self.auxiliary_head(s1)
        out = self.global_pooling(s1)
        return self.classifier(out.view(out.size(0), -1)), logits_aux


class BATSNetworkCIFAR(_BATSNetwork):
    """Reference: ``bats.py:108-151``.  ``forward`` returns ``(logits, logits_aux)``."""

    def __init__(self, C: int, num_classes: int, layers: int, auxiliary: bool, genotype, groups: int) -> None:
        super().__init__()
        self._layers = layers
        self._auxiliary = auxiliary
        C_curr = 3 * C      # (stem_multiplier)
        self.stem = nn.Sequential(
            nn.Conv2d(3, C_curr, 3, padding=1, bias=False),
            nn.BatchNorm2d(C_curr),
            nn.ReLU(inplace=True),
        )
        C_prev, C_to_auxiliary = self._build_cells(C_curr, C_curr, C, layers, genotype, groups, False)
        if auxiliary:
            self.auxiliary_head = AuxiliaryHead(C_to_auxiliary, num_classes, 3)
        self.global_pooling = nn.AdaptiveAvgPool2d(1)
        self.classifier = nn.Linear(C_prev, num_classes)

    def forward(self, input: torch.Tensor) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        s0 = s1 = self.stem(input)
        return self._run_cells(s0, s1)


class BATSNetworkImageNet(_BATSNetwork):
    """Reference: ``bats.py:154-206``."""

    def __init__(self, C: int, num_classes: int, layers: int, auxiliary: bool, genotype, groups: int) -> None:
        super().__init__()
        self._layers = layers
        self._auxiliary = auxiliary
        self.stem0 = nn.Sequential(
            nn.Conv2d(3, C // 2, kernel_size=3, stride=2, padding=1, bias=False),
            nn.BatchNorm2d(C // 2),
            nn.ReLU(inplace=True),
            nn.Conv2d(C // 2, C, 3, stride=2, padding=1, bias=False, groups=C // 20),
            nn.BatchNorm2d(C),
        )
        self.stem1 = nn.Sequential(
            nn.ReLU(inplace=True),
            nn.Conv2d(C, C, 3, stride=2, padding=1, bias=False, groups=C // 20),
            nn.BatchNorm2d(C),
        )
        C_prev, C_to_auxiliary = self._build_cells(C, C, C, layers, genotype, groups, True)
        if auxiliary:
            self.auxiliary_head = AuxiliaryHead(C_to_auxiliary, num_classes, 2)
        self.global_pooling = nn.AvgPool2d(7)
        self.classifier = nn.Linear(C_prev, num_classes)

    def forward(self, input: torch.Tensor) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        s0 = self.stem0(input)
        s1 = self.stem1(s0)
        return self._run_cells(s0, s1)

"""The BATS cell operations in two launches (reference: ``bnn/models/layers/bats_ops.py:78-173``).

``SepConv`` / ``DilConv`` / ``ReLUConvBN`` all have the form

    y = [x +] channel_shuffle(PReLU(conv(sign(BatchNorm(x)))), 4)        # skip only at stride 1; ReLUConvBN: no shuffle

``FusedCellOp(module)`` evaluates one of them as ``bn_act_pack`` (BatchNorm + sign -> bit planes, one pass over x) and ONE
convolution launch whose epilogue applies the PReLU, stores through the shuffle permutation and adds the skip
(``bnn_hip_bconv2d_grouped_fused``, csrc/bconv_grouped.hip; the dense ``ReLUConvBN`` takes ``bnn_hip_bconv2d_fused``):
three fp32 passes over HBM (x read by the pack, x read as the skip, y written) instead of about eleven.  The per-layer
path — torch BatchNorm, ``pack_act``, the grouped kernel, torch PReLU, the ``.contiguous()`` shuffle copy, torch add —
stays what every call outside ``eval()`` / ``no_grad()`` runs.

``FusedFactorizedConv(module)`` does the same for ``FactorizedConv`` (``'conv_7x1_1x7'``): two dense binary convolutions
with only a sign between them, run as ``bn_act_pack`` and one launch that keeps that sign in LDS (csrc/fconv.hip).

``FusedCell(cell)`` evaluates a whole ``Cell`` (reference: ``bnn/models/bats.py:9-83``) the same way: every state is
binarised once for all the operations that read it (``bn_act_pack_multi``), a node ``s = op1(h1) + op2(h2)`` is the
second operation's launch adding the first one's result in its epilogue (``bnn_hip_bconv2d_grouped_node``), and that
launch stores into the node's channel slice of the cell output, so neither the add nor ``torch.cat`` runs.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch
import torch.nn as nn

from . import fastpath, hipops, native
from .executor import FusionError, fold_bn, param_signature

CELL_OP_NAMES = ("SepConv", "DilConv", "ReLUConvBN")
MAX_PACK_SETS = 4       # plane sets one bn_act_pack_multi launch writes (include/bnn_hip.h)
SHUFFLE_GROUPS = 4      # channel_shuffle(., 4) in SepConv.forward / DilConv.forward


def _pair_of(v, what: str):
    if isinstance(v, int):
        return (v, v)
    if isinstance(v, (tuple, list)) and len(v) == 2 and all(isinstance(e, int) for e in v):
        return tuple(v)
    raise FusionError(f"cell op: {what}={v!r} is not numeric")


def _binary_plan(conv, what: str):
    """The recipe of a binary convolution the HIP kernels cover, or ``FusionError`` (messages start with ``what``)."""
    if not (isinstance(conv, nn.Conv2d) and hasattr(conv, "activation_pre_process")):
        raise FusionError(f"{what} is not a binary Conv2d (run prepare_binary_model first)")
    plan = fastpath._recognise(conv, conv.out_channels)
    if plan is None:
        raise FusionError(f"{what}: layer recipe is not BasicInputBinarizer + XNORWeightBinarizer "
                          "(+ Identity | BasicScaleBinarizer)")
    if conv.weight.dtype != torch.float32:
        raise FusionError(f"{what}: only float32 modules are covered")
    return plan


def _prelu_slopes(act: nn.PReLU, channels: int) -> torch.Tensor:
    """The PReLU slopes as a vector of ``channels``: a snapshot, like the folded BatchNorm and the packed weight."""
    slope = act.weight.detach().float().reshape(-1)
    return (slope.expand(channels) if slope.numel() == 1 else slope).clone()


class Preprocessor(NamedTuple):
    """What ``FusedCell.preprocessor(i)`` tells about ``preprocess{i}``: ``kind`` is ``ReLUConvBN`` or
    ``FactorizedReduce``; ``bn_a`` / ``bn_b`` the folded BatchNorm in front of its sign(); ``add_skip`` whether it adds its
    fp32 input (a ``FactorizedReduce`` always reads it: it packs for itself)."""
    kind: str
    bn_a: torch.Tensor
    bn_b: torch.Tensor
    add_skip: bool
    C_in: int


class _Executor(nn.Module):
    """What ``FusedCellOp`` and ``FusedCell`` share: derived data keyed on the identity, storage and version of every
    parameter and buffer of ``model`` (``refresh()`` derives it and sets ``_sig``), and the test of an input."""
    takes: str      # what the inputs must be, for the error message

    def __init__(self, module: nn.Module) -> None:
        super().__init__()
        self.model = module
        self._sig = None
        self.refresh()

    def _unchanged(self) -> bool:
        return self._sig is not None and not self.model.training and param_signature(self.model) == self._sig

    def _check_inputs(self, *inputs) -> None:
        for x in inputs:
            if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4):
                raise FusionError(f"{self.takes} on a HIP device")


class FusedCellOp(_Executor):
    """Inference executor of one BATS cell operation.  Recognition is by structure — the class NAME must be one of
    ``SepConv`` / ``DilConv`` / ``ReLUConvBN`` and ``module.op`` must be ``Sequential(BatchNorm2d, binary Conv2d,
    PReLU)`` with ``stride`` / ``skip`` as those classes define them — so an instance of the reference's own classes,
    handed over explicitly, works as well as one of ``bnn_amd.models``.  Anything else raises ``FusionError``.

    Derived data (folded BatchNorm, the launch arguments with the PReLU slopes as a vector of ``O``, the packed weight)
    is keyed on the identity, storage and version of every parameter and buffer and re-derived when one changes; writes
    through ``.data`` need ``refresh()`` (or ``fastpath.invalidate(module)`` for the executor ``module(x)`` dispatches to).

    ``forward`` is ``conv(pack(x), x)``; a ``FusedCell`` runs the two steps apart (one pack for several operations) and
    takes the convolution in its node form, ``conv_node``.  ``bn_a`` / ``bn_b`` are the folded BatchNorm constants the
    pack applies, ``add_skip`` says whether the convolution launch adds ``x``."""
    takes = "cell op: the input must be a float32 NCHW tensor"

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
        plan = _binary_plan(conv, "cell op")
        if isinstance(conv.padding, str) or conv.padding_mode != "zeros":
            raise FusionError(f"cell op: padding={conv.padding!r}, padding_mode={conv.padding_mode!r} is not covered")
        if bn.running_var.dtype != torch.float32:
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
            self.add_skip = m.skip and stride[0] == 1 and C == O
            self._shuffle = 1
        else:
            if C != O or O % SHUFFLE_GROUPS or conv.groups < 2:
                raise FusionError(f"cell op: {kind} needs C_in == C_out, a multiple of {SHUFFLE_GROUPS}, and groups > 1")
            self.add_skip = m.skip and stride[0] == 1
            self._shuffle = SHUFFLE_GROUPS
        self._plan = plan
        self._grouped = conv.groups != 1

    # ---- derived data -----------------------------------------------------------------------------------------------
    def refresh(self) -> None:
        """Re-derive everything from the module's current parameters and buffers."""
        self._sig = None
        self._recognise()
        bn, conv, act = self.model.op
        fastpath.invalidate(self.model, executors=False)
        self.bn_a, self.bn_b = fold_bn(bn)
        # what every form of the convolution launch takes besides planes, weight and skip: bias, post scale, geometry,
        # PReLU slopes, and the shuffle groups or (ReLUConvBN: the dense convolution's own epilogue) the late residual
        self._launch = dict(bias=fastpath._f32(conv.bias), post_scale=fastpath._f32(self._plan.scale), stride=conv.stride,
                            padding=conv.padding, dilation=conv.dilation, prelu=_prelu_slopes(act, conv.out_channels),
                            **({"shuffle_groups": self._shuffle} if self._grouped else {"residual_after_act": True}))
        self._weight: Optional[hipops.PackedWeight] = None
        if conv.weight.is_cuda:
            native.require()
            self._weight = fastpath.packed_weight(conv, self._plan)
        self._sig = param_signature(self.model)

    # ---- the two launches -------------------------------------------------------------------------------------------
    def pack(self, x: torch.Tensor) -> hipops.PackedAct:
        """``sign(BatchNorm(x))`` as bit planes (``bn_act_pack``)."""
        return hipops.bn_act_pack(x, self.bn_a, self.bn_b, relu=False)

    def conv(self, planes: hipops.PackedAct, x: torch.Tensor) -> torch.Tensor:
        """The convolution launch on ``planes`` (of ``x``: ``pack(x)``, or its set of a ``bn_act_pack_multi``) with
        PReLU, shuffle and skip in its epilogue: ``bconv2d_grouped_fused``, or ``bconv2d_fused`` for ``ReLUConvBN``."""
        res = x if self.add_skip else None
        if self._grouped:
            return hipops.bconv2d_grouped_fused(planes, self._weight, residual=res, **self._launch)
        return hipops.bconv2d_fused(planes, self._weight, residual=res, **self._launch)[0]

    def conv_node(self, planes: hipops.PackedAct, x: torch.Tensor, addend: Optional[torch.Tensor] = None,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``conv`` of a ``SepConv`` / ``DilConv`` as one term of a cell node (``bconv2d_grouped_node``): ``addend`` is
        added in the epilogue and the result stored into ``out``; each may be missing."""
        return hipops.bconv2d_grouped_node(planes, self._weight, residual=x if self.add_skip else None, addend=addend,
                                           out=out, **self._launch)

    @torch.no_grad()
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        self._check_inputs(x)
        if not self._unchanged():
            self.refresh()
        if self._weight is None or self._weight.alpha.device != x.device:     # (packed from the current weight)
            raise FusionError("cell op: module and input live on different devices")
        y = self.conv(self.pack(x), x)
        fastpath._bump("cell_op")
        return y


class FusedFactorizedConv(_Executor):
    """Inference executor of a BATS ``FactorizedConv`` (reference: ``bats_ops.py:55-75``, ``'conv_7x1_1x7'``)

        y = [x +] channel_shuffle(PReLU(conv_Kx1(sign(BN(PReLU(conv_1xK(sign(BN(x)))))))), 4)     # skip at stride 1

    as ``bn_act_pack`` and ONE launch (``hipops.fconv_fused``, csrc/fconv.hip) that keeps the tensor between the two
    convolutions in LDS as bit planes: two launches and three fp32 passes over HBM (x read by the pack, x read as the
    skip, y written).  Where ``hipops.fconv_supported`` or ``fastpath.fconv_admitted`` says no, the same bits come from
    the launches the library had before: ``bconv2d_fused`` of the 1 x K layer (planes only), ``bconv2d_fused`` of the
    K x 1 layer, torch's shuffle and add.

    Recognition is by structure, like ``FusedCellOp``: the class NAME must be ``FactorizedConv`` and ``module.op`` the
    six modules of the reference with both convolutions binary, dense and of exactly the constructor's geometry, so an
    instance of the reference's own class, handed over explicitly, works.  Derived data (the two folded BatchNorms, the
    two packed weights, the slope vectors) is keyed on the identity, storage and version of every parameter and buffer;
    writes through ``.data`` need ``refresh()`` (or ``fastpath.invalidate(module)``)."""
    takes = "factorized conv: the input must be a float32 NCHW tensor"

    def _recognise(self) -> None:
        m = self.model
        kind = type(m).__name__
        if kind != "FactorizedConv":
            raise FusionError(f"{kind} is not a BATS FactorizedConv")
        op = getattr(m, "op", None)
        kinds = (nn.BatchNorm2d, nn.Conv2d, nn.PReLU, nn.BatchNorm2d, nn.Conv2d, nn.PReLU)
        if not (isinstance(op, nn.Sequential) and len(op) == 6 and all(isinstance(a, b) for a, b in zip(op, kinds))):
            raise FusionError("FactorizedConv.op is not Sequential(BatchNorm2d, Conv2d, PReLU, BatchNorm2d, Conv2d, PReLU)")
        bn1, c1, a1, bn2, c2, a2 = op
        if m.training:
            raise FusionError("FusedFactorizedConv is inference-only: call .eval() first")
        self._plans = [_binary_plan(c, "factorized conv") for c in (c1, c2)]
        for bn in (bn1, bn2):
            if bn.running_mean is None or bn.running_var is None:
                raise FusionError("factorized conv: BatchNorm2d without running statistics normalises with batch statistics")
            if bn.running_var.dtype != torch.float32:
                raise FusionError("factorized conv: only float32 modules are covered")
        stride = getattr(m, "stride", None)
        if not isinstance(stride, int) or isinstance(stride, bool) or stride < 1:
            raise FusionError(f"factorized conv: stride={stride!r} is not a positive int")
        if not isinstance(getattr(m, "skip", None), bool):
            raise FusionError("factorized conv: FactorizedConv.skip is not a bool")
        C, K = c1.in_channels, c1.kernel_size[1]
        want = [((1, K), (1, stride), (0, K // 2)), ((K, 1), (stride, 1), (K // 2, 0))]
        for c, (ks, st, pd) in zip((c1, c2), want):
            if (isinstance(c.padding, str) or c.padding_mode != "zeros" or c.groups != 1 or tuple(c.dilation) != (1, 1)
                    or c.in_channels != C or c.out_channels != C or K % 2 == 0
                    or (tuple(c.kernel_size), tuple(c.stride), tuple(c.padding)) != (ks, st, pd)):
                raise FusionError("factorized conv: the convolutions are not dense C -> C, (1, K) / (1, s) / (0, K//2) then "
                                  "(K, 1) / (s, 1) / (K//2, 0)")
        if C % SHUFFLE_GROUPS or any(bn.num_features != C for bn in (bn1, bn2)) \
                or any(a.weight.numel() not in (1, C) for a in (a1, a2)):
            raise FusionError(f"factorized conv: widths do not fit ({C} channels, a multiple of {SHUFFLE_GROUPS})")
        self.C, self.K, self.stride = C, K, stride
        self.add_skip = m.skip and stride == 1

    def refresh(self) -> None:
        """Re-derive everything from the module's current parameters and buffers."""
        self._sig = None
        self._recognise()
        bn1, c1, a1, bn2, c2, a2 = self.model.op
        fastpath.invalidate(self.model, executors=False)
        self.bn_a, self.bn_b = fold_bn(bn1)
        self.mid_a, self.mid_b = fold_bn(bn2)
        self._stage = [dict(bias=fastpath._f32(c.bias), post_scale=fastpath._f32(p.scale), prelu=_prelu_slopes(a, self.C))
                       for c, p, a in ((c1, self._plans[0], a1), (c2, self._plans[1], a2))]
        self._weights = None
        self._fused = {}        # input shape -> whether the one-launch kernel takes it
        if c1.weight.is_cuda:
            native.require()
            self._weights = [fastpath.packed_weight(c, p) for c, p in zip((c1, c2), self._plans)]
        self._sig = param_signature(self.model)

    def pack(self, x: torch.Tensor) -> hipops.PackedAct:
        """``sign(BatchNorm(x))`` as bit planes (``bn_act_pack``)."""
        return hipops.bn_act_pack(x, self.bn_a, self.bn_b, relu=False)

    def takes_fused(self, shape) -> bool:
        """Whether an input of this shape runs the one-launch kernel: it exists for the geometry
        (``hipops.fconv_supported``) and did not measure slower than the per-layer launches
        (``fastpath.fconv_admitted``)."""
        shape = tuple(shape)
        ok = self._fused.get(shape)
        if ok is None:
            N, C, H, W = shape
            ok = self._fused[shape] = bool(fastpath.fconv_admitted(C, H, W, self.stride)
                                           and hipops.fconv_supported(N, C, H, W, self.K, self.stride))
        return ok

    def conv(self, planes: hipops.PackedAct, x: torch.Tensor) -> torch.Tensor:
        """Everything behind the first BatchNorm in one launch (``hipops.fconv_fused``)."""
        s1, s2 = self._stage
        return hipops.fconv_fused(planes, self._weights[0], self._weights[1], self.mid_a, self.mid_b, stride=self.stride,
                                  bias1=s1["bias"], post_scale1=s1["post_scale"], prelu1=s1["prelu"], bias2=s2["bias"],
                                  post_scale2=s2["post_scale"], prelu2=s2["prelu"], shuffle_groups=SHUFFLE_GROUPS,
                                  residual=x if self.add_skip else None)

    def composition(self, planes: hipops.PackedAct, x: torch.Tensor) -> torch.Tensor:
        """The same bits from two ``bconv2d_fused`` launches (the tensor between them as bit planes in global memory),
        torch's shuffle copy and torch's add: what runs where the one-launch kernel does not."""
        s, K = self.stride, self.K
        _, t = hipops.bconv2d_fused(planes, self._weights[0], stride=(1, s), padding=(0, K // 2), pack_scale=self.mid_a,
                                    pack_shift=self.mid_b, out_f32=False, out_packed=True, **self._stage[0])
        y, _ = hipops.bconv2d_fused(t, self._weights[1], stride=(s, 1), padding=(K // 2, 0), **self._stage[1])
        n, c, h, w = y.shape
        y = y.reshape(n, SHUFFLE_GROUPS, c // SHUFFLE_GROUPS, h, w).transpose(1, 2).reshape(n, c, h, w)
        return x + y if self.add_skip else y.contiguous()

    @torch.no_grad()
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        self._check_inputs(x)
        if not self._unchanged():
            self.refresh()
        if self._weights is None or self._weights[0].alpha.device != x.device:
            raise FusionError("factorized conv: module and input live on different devices")
        if x.shape[1] != self.C:
            raise FusionError(f"factorized conv: the input has {x.shape[1]} channels, the module {self.C}")
        planes = self.pack(x)
        if self.takes_fused(x.shape):
            y = self.conv(planes, x)
            fastpath._bump("fconv")
            return y
        return self.composition(planes, x)


def _stride_of(op: nn.Module) -> int:
    s = getattr(op, "stride", 1)
    return s[0] if isinstance(s, (tuple, list)) else s


class _Reduce:
    """Recognition and derived data of one ``FactorizedReduce``: BatchNorm folded for ``bn_act_pack_s2``, the two 1x1
    stride-2 convolutions as dense launches on the two phases, the PReLU slopes split like the output channels."""

    def __init__(self, m: nn.Module) -> None:
        bn, act = getattr(m, "bn", None), getattr(m, "activation", None)
        convs = [getattr(m, n, None) for n in ("conv_1", "conv_2")]
        if not (isinstance(bn, nn.BatchNorm2d) and isinstance(act, nn.PReLU)
                and all(isinstance(c, nn.Sequential) and len(c) == 1 for c in convs)):
            raise FusionError("FactorizedReduce is not bn / conv_1 / conv_2 / activation as the reference defines it")
        if bn.running_mean is None or bn.running_var is None or bn.running_var.dtype != torch.float32:
            raise FusionError("FactorizedReduce: BatchNorm2d without float32 running statistics")
        self.convs = [c[0] for c in convs]
        self.plans = [_binary_plan(c, "FactorizedReduce convolution") for c in self.convs]
        half = self.convs[0].out_channels
        for c in self.convs:
            if (c.in_channels != bn.num_features or c.out_channels != half or c.groups != 1
                    or tuple(c.kernel_size) != (1, 1) or tuple(c.stride) != (2, 2) or tuple(c.padding) != (0, 0)
                    or isinstance(c.padding, str) or c.padding_mode != "zeros"):
                raise FusionError("FactorizedReduce: the convolutions are not 1x1 / stride 2 / no padding over the "
                                  "BatchNorm's channels")
        if act.weight.numel() not in (1, 2 * half):
            raise FusionError("FactorizedReduce: PReLU width does not fit the concatenated output")
        self.C_in, self.C_out = bn.num_features, 2 * half
        self.bn_a, self.bn_b = fold_bn(bn)
        slope = _prelu_slopes(act, self.C_out)
        self.prelu = [slope[:half].contiguous(), slope[half:].contiguous()]
        self.weights = None
        if self.convs[0].weight.is_cuda:
            native.require()
            self.weights = [fastpath.packed_weight(c, p) for c, p in zip(self.convs, self.plans)]

    def pack(self, x: torch.Tensor):
        if x.shape[2] % 2 or x.shape[3] % 2:
            raise FusionError(f"FactorizedReduce needs even H and W, got {tuple(x.shape[2:])}")
        return hipops.bn_act_pack_s2(x, self.bn_a, self.bn_b, relu=False)

    def conv(self, planes, k: int, out: torch.Tensor) -> None:
        half = self.C_out // 2
        hipops.bconv2d_fused(planes[k], self.weights[k], bias=self.convs[k].bias, post_scale=self.plans[k].scale,
                             prelu=self.prelu[k], out=out, out_c_offset=k * half)


class FusedCell(_Executor):
    """Inference executor of one BATS ``Cell`` at ``drop_prob = 0``: ``FusedCell(cell)(s0, s1)``.

    Recognition follows ``FusedCellOp`` — class names plus structure (``Cell`` with ``preprocess0`` / ``preprocess1`` /
    ``_ops`` / ``_indices`` / ``_concat``; operations named ``SepConv``, ``DilConv``, ``FactorizedReduce``, ``Zero`` or
    torch's ``Identity`` / ``AvgPool2d`` / ``MaxPool2d``), so a cell of the reference's own classes works when handed over
    explicitly.  ``use_shake_shake``, training mode, an odd ``H`` or ``W`` in front of a ``FactorizedReduce`` and
    anything unrecognised raise ``FusionError``.

    ``steps`` lists the planned launches and torch calls as ``(kind, detail)`` with kinds ``pack``, ``pack_s2``,
    ``pack_multi``, ``dense``, ``grouped_node``, ``torch_pool``, ``torch_add``, ``copy``, ``zero``.  A ``Zero`` term is
    dropped from its node: equal as numbers, only ``-0.0 + 0.0`` would have been ``+0.0``.

    Derived data is keyed on the identity, storage and version of every parameter and buffer of the cell, like
    ``FusedCellOp``; writes through ``.data`` need ``refresh()`` (or ``fastpath.invalidate(cell)``)."""
    takes = "cell: the inputs must be float32 NCHW tensors"

    # ---- recognition and planning ---------------------------------------------------------------------------------
    def _kind(self, op: nn.Module) -> str:
        name = type(op).__name__
        if name in ("SepConv", "DilConv"):
            return "conv"
        if name == "FactorizedReduce":
            return "reduce"
        if name == "Zero" and isinstance(getattr(op, "stride", None), int):
            return "zero"
        if type(op) is nn.Identity:
            return "identity"
        if type(op) in (nn.AvgPool2d, nn.MaxPool2d):
            return "pool"
        raise FusionError(f"cell: operation {name} is not covered")

    def refresh(self) -> None:
        """Re-derive everything from the cell's current parameters and buffers."""
        self._sig = None
        cell = self.model
        if type(cell).__name__ != "Cell":
            raise FusionError(f"{type(cell).__name__} is not a BATS Cell")
        if cell.training:
            raise FusionError("FusedCell is inference-only: call .eval() first")
        if getattr(cell, "use_shake_shake", False):
            raise FusionError("cell: use_shake_shake is not covered")
        ops, idx, concat = getattr(cell, "_ops", None), getattr(cell, "_indices", None), getattr(cell, "_concat", None)
        if not (isinstance(ops, nn.ModuleList) and idx is not None and concat is not None and len(ops) == len(idx)
                and len(ops) % 2 == 0 and len(ops) == 2 * getattr(cell, "_steps", -1) and len(concat) > 0):
            raise FusionError("cell: _ops / _indices / _concat / _steps are not as Cell._compile leaves them")
        n_states = 2 + len(ops) // 2
        idx, concat = [int(i) for i in idx], [int(c) for c in concat]
        if any(not 0 <= j < 2 + k // 2 for k, j in enumerate(idx)) or any(not 0 <= c < n_states for c in concat) \
                or len(set(concat)) != len(concat):
            raise FusionError("cell: an operation reads a later state, or the concat list repeats or exceeds the states")
        fastpath.invalidate(cell, executors=False)
        self._pre = []
        for name in ("preprocess0", "preprocess1"):
            m = getattr(cell, name, None)
            if type(m).__name__ == "ReLUConvBN":
                self._pre.append(FusedCellOp(m))
            elif type(m).__name__ == "FactorizedReduce":
                self._pre.append(_Reduce(m))
            else:
                raise FusionError(f"cell: {name} is {type(m).__name__}, not ReLUConvBN / FactorizedReduce")
        self._kinds = [self._kind(op) for op in ops]
        self._conv = {k: FusedCellOp(op) for k, op in enumerate(ops) if self._kinds[k] == "conv"}
        self._red = {k: _Reduce(op) for k, op in enumerate(ops) if self._kinds[k] == "reduce"}
        widths = {p.C_out if isinstance(p, _Reduce) else p.model.op[1].out_channels for p in self._pre}
        widths |= {e.model.op[1].in_channels for e in self._conv.values()} | {r.C_in for r in self._red.values()}
        widths |= {r.C_out for r in self._red.values()}
        if len(widths) != 1:
            raise FusionError(f"cell: preprocessing and operations do not share one width ({sorted(widths)})")
        C = widths.pop()
        # a reduction cell: every operation on s0 / s1 has stride 2, and the nodes live at half the resolution
        self._reduction = any(self._kinds[k] == "reduce" or _stride_of(op) == 2 for k, op in enumerate(ops))
        self._C, self._idx, self._concat, self._n_states = C, idx, concat, n_states
        # per state: its SepConv / DilConv consumers in chunks of MAX_PACK_SETS, their folded BatchNorms stacked
        self._packs = {}
        for j in range(n_states):
            users = [k for k in self._conv if idx[k] == j]
            chunks = [users[i:i + MAX_PACK_SETS] for i in range(0, len(users), MAX_PACK_SETS)]
            self._packs[j] = [(ch, torch.stack([self._conv[k].bn_a for k in ch]),
                               torch.stack([self._conv[k].bn_b for k in ch])) for ch in chunks]
        self._plan = self._make_plan()
        self._sig = param_signature(self.model)

    def _make_plan(self):
        """The steps of one forward as ``(kind, detail, run)``; ``run(env)`` works on ``env``: ``in`` (s0, s1), ``state``
        (list), ``planes`` (operation -> PackedAct), ``out`` (the cell output)."""
        plan = []
        C, idx, kinds = self._C, self._idx, self._kinds

        def add(kind, detail, run):
            plan.append((kind, detail, run))

        # -- the two input states
        for i, pre in enumerate(self._pre):
            if isinstance(pre, FusedCellOp):
                add("pack", {"op": f"preprocess{i}", "sets": 1}, lambda env, i=i, pre=pre: self._pre_pack(env, i, pre))
                add("dense", {"op": f"preprocess{i}"}, lambda env, i=i, pre=pre: env["state"].__setitem__(
                    i, pre.conv(env["planes"][("pre", i)], env["in"][i])))
            else:
                self._plan_reduce(add, f"preprocess{i}", pre, lambda env, i=i: env["in"][i],
                                  lambda env, y, i=i: env["state"].__setitem__(i, y))
        add("alloc", None, self._alloc)     # (not a step: the cell output, once the states' shape is known)

        packed = set()

        def need_planes(j):
            if j in packed:
                return
            packed.add(j)
            for ch, a, b in self._packs[j]:
                add("pack_multi", {"state": j, "ops": list(ch), "sets": len(ch)},
                    lambda env, j=j, ch=ch, a=a, b=b: env["planes"].update(
                        zip(ch, hipops.bn_act_pack_multi(env["state"][j], a, b, relu=False))))

        def other_term(k, tmp):
            """Plan the non-convolution operation k; returns how to fetch its value from env."""
            j = idx[k]
            if kinds[k] == "identity":
                return lambda env: env["state"][j]
            if kinds[k] == "pool":
                op = self.model._ops[k]
                add("torch_pool", {"op": k, "state": j}, lambda env: env["tmp"].__setitem__(tmp, op(env["state"][j])))
            else:
                self._plan_reduce(add, k, self._red[k], lambda env: env["state"][j],
                                  lambda env, y: env["tmp"].__setitem__(tmp, y))
            return lambda env: env["tmp"][tmp]

        # -- the nodes
        for n in range(len(kinds) // 2):
            s = n + 2
            terms = [k for k in (2 * n, 2 * n + 1) if kinds[k] != "zero"]
            convs = [k for k in terms if kinds[k] == "conv"]
            others = [k for k in terms if kinds[k] != "conv"]
            dest = lambda env, s=s: self._dest(env, s)      # noqa: E731
            for k in convs:
                need_planes(idx[k])
            if len(convs) == 2:
                k1, k2 = convs
                add("grouped_node", {"op": k1, "state": idx[k1], "addend": False, "to": "temporary"},
                    lambda env, k1=k1, s=s: env["tmp"].__setitem__((s, "h1"), self._run_node(env, k1, None, None)))
                add("grouped_node", {"op": k2, "state": idx[k2], "addend": True, "to": s},
                    lambda env, k2=k2, s=s, dest=dest: self._run_node(env, k2, env["tmp"][(s, "h1")], dest(env)))
            elif len(convs) == 1:
                get = other_term(others[0], (s, "other")) if others else None
                add("grouped_node", {"op": convs[0], "state": idx[convs[0]], "addend": get is not None, "to": s},
                    lambda env, k=convs[0], get=get, dest=dest: self._run_node(
                        env, k, None if get is None else get(env), dest(env)))
            elif len(others) == 2:
                ga, gb = other_term(others[0], (s, "a")), other_term(others[1], (s, "b"))
                add("torch_add", {"ops": list(others), "to": s},
                    lambda env, ga=ga, gb=gb, dest=dest: torch.add(self._same(ga(env), gb(env)), gb(env), out=dest(env)))
            elif len(others) == 1:
                ga = other_term(others[0], (s, "a"))
                add("copy", {"op": others[0], "to": s}, lambda env, ga=ga, dest=dest: dest(env).copy_(ga(env)))
            else:
                add("zero", {"to": s}, lambda env, dest=dest: dest(env).zero_())
        # -- input states named in the concat list are copied into their slices
        for c in self._concat:
            if c < 2:
                add("copy", {"state": c, "to": "concat"},
                    lambda env, c=c: self._slice(env, c).copy_(self._same(env["state"][c], self._slice(env, c))))
        return plan

    def _plan_reduce(self, add, name, red, src, put) -> None:
        key = ("reduce", name)
        add("pack_s2", {"op": name}, lambda env: env["planes"].__setitem__(key, red.pack(src(env))))

        def first(env):
            p = env["planes"][key]
            N, _, H, W = p[0].shape
            y = torch.empty((N, red.C_out, H, W), dtype=torch.float32, device=p[0].P.device)
            red.conv(p, 0, y)
            put(env, y)
            env["tmp"][key] = y
        add("dense", {"op": name, "half": 0}, first)
        add("dense", {"op": name, "half": 1}, lambda env: red.conv(env["planes"][key], 1, env["tmp"][key]))

    @property
    def steps(self):
        """The planned steps as ``(kind, detail)``, in execution order."""
        return [(kind, dict(detail)) for kind, detail, _ in self._plan if detail is not None]

    # ---- the steps ------------------------------------------------------------------------------------------------
    @staticmethod
    def _pre_pack(env, i: int, pre: FusedCellOp) -> None:
        """The ``pack`` step of preprocessor ``i``; nothing to do when the caller handed its planes over."""
        if ("pre", i) not in env["planes"]:
            env["planes"][("pre", i)] = pre.pack(env["in"][i])

    @staticmethod
    def _same(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
        if a.shape != b.shape:
            raise FusionError(f"cell: the two terms of a node have shapes {tuple(a.shape)} and {tuple(b.shape)}")
        return a

    def _alloc(self, env) -> None:
        """The cell output ``[N, len(concat) * C, H, W]`` at the nodes' resolution: every node state named in the concat
        list IS its channel slice."""
        s0, s1 = env["state"][0], env["state"][1]
        self._same(s0, s1)
        N, C, H, W = s1.shape
        if self._reduction:
            H, W = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        env["out"] = torch.empty((N, len(self._concat) * C, H, W), dtype=torch.float32, device=s1.device)
        env["node_shape"] = (N, C, H, W)

    def _slice(self, env, s: int) -> torch.Tensor:
        p = self._concat.index(s)
        return env["out"][:, p * self._C:(p + 1) * self._C]

    def _dest(self, env, s: int) -> torch.Tensor:
        """Where node state ``s`` is stored: its slice of the cell output, or a tensor of its own."""
        if env["state"][s] is None:
            env["state"][s] = self._slice(env, s) if s in self._concat else torch.empty(
                env["node_shape"], dtype=torch.float32, device=env["out"].device)
        return env["state"][s]

    def _run_node(self, env, k: int, addend: Optional[torch.Tensor], out: Optional[torch.Tensor]) -> torch.Tensor:
        e = self._conv[k]
        conv = e.model.op[1]
        x = env["state"][self._idx[k]]
        planes = env["planes"][k]
        N, _, H, W = planes.shape
        shape = (N, self._C) + hipops.conv_out_hw(H, W, conv.kernel_size[0], conv.kernel_size[1], conv.stride,
                                                  conv.padding, conv.dilation)
        for t in (addend, out):
            if t is not None and tuple(t.shape) != shape:
                raise FusionError(f"cell: operation {k} gives {shape}, its node holds {tuple(t.shape)}")
        return e.conv_node(planes, x, addend, out)

    # ---- what a caller that packs for the cell needs to know ------------------------------------------------------
    def preprocessor(self, i: int) -> "Preprocessor":
        """Kind, folded BatchNorm and skip of ``preprocess{i}`` (current as of the last ``refresh()``)."""
        pre = self._pre[i]
        if isinstance(pre, FusedCellOp):
            return Preprocessor("ReLUConvBN", pre.bn_a, pre.bn_b, pre.add_skip, pre.model.op[1].in_channels)
        return Preprocessor("FactorizedReduce", pre.bn_a, pre.bn_b, False, pre.C_in)

    def _handed(self, i: int, s: Optional[torch.Tensor], p) -> tuple:
        """Checks input ``i`` and the planes handed over for it; returns its (device, batch size)."""
        pre = self.preprocessor(i)
        if p is None:
            if s is None:
                raise FusionError(f"cell: input {i} is missing and no planes were handed over for it")
            self._check_inputs(s)
            return s.device, s.shape[0]
        if pre.kind != "ReLUConvBN":
            raise FusionError(f"cell: preprocess{i} is a FactorizedReduce, which packs for itself")
        if not isinstance(p, hipops.PackedAct) or p.shape[1] != pre.C_in or not p.P.is_cuda:
            raise FusionError(f"cell: planes[{i}] must be a PackedAct of {pre.C_in} channels on a HIP device")
        if s is None:
            if pre.add_skip:
                raise FusionError(f"cell: preprocess{i} adds its input, so input {i} is needed next to its planes")
        else:
            self._check_inputs(s)
            if tuple(s.shape) != tuple(p.shape) or s.device != p.P.device:
                raise FusionError(f"cell: planes[{i}] are not those of input {i}")
        return p.P.device, p.shape[0]

    # ---- forward --------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def forward(self, s0: Optional[torch.Tensor], s1: Optional[torch.Tensor], planes=None) -> torch.Tensor:
        """``cell(s0, s1, 0.0)``.  ``planes``: a pair with, per input, ``None`` or the ``PackedAct`` of
        ``sign(BatchNorm(s_i))`` made with ``preprocessor(i)``'s ``bn_a`` / ``bn_b`` by somebody who packs one tensor for
        several cells; that ``ReLUConvBN`` then skips its own pack, and ``s_i`` may be ``None`` unless it adds a skip."""
        if not self._unchanged():
            self.refresh()
        planes = (None, None) if planes is None else tuple(planes)
        if len(planes) != 2:
            raise FusionError("cell: planes is a pair, one entry per input")
        (d0, n0), (d1, n1) = self._handed(0, s0, planes[0]), self._handed(1, s1, planes[1])
        if d0 != d1 or n0 != n1:
            raise FusionError("cell: the two inputs differ in device or batch size")
        if next(self.model.parameters()).device != d0:
            raise FusionError("cell: module and input live on different devices")
        env = {"in": (s0, s1), "state": [None] * self._n_states,
               "planes": {("pre", i): p for i, p in enumerate(planes) if p is not None}, "tmp": {}, "out": None}
        for _, _, run in self._plan:
            run(env)
        fastpath._bump("cell")
        return env["out"]

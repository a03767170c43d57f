"""Training step of a binary ``Conv2d`` with the forward on the HIP XNOR/popcount path
(reference: ``bnn/ops.py:63-73`` straight-through estimator,
``bnn/layers/conv.py:90-97`` forward, ``examples/imagenet.py:337-384`` training loop).

    forward :  y = bconv2d( pack(sign(x)), pack(sign(Wc)), alpha ) [+ bias]        HIP XNOR/popcount kernels
    backward:  g_xhat[n,c] = sum_o,k g_y * W_hat      g_x = g_xhat * 1[|x| < 1]       STE of ops.py:68-73
               g_what[o,c] = sum_n,p g_y * sign(x)
               g_W through the weight hook's own autograd graph (sign STE + alpha = mean|W|)

Each gradient GEMM has ONE real operand (``g_y``) and one that is exactly ternary (``sign(Wc)``, ``sign(x)``).
For the 3x3 / padding 1 layers of stride 1 or 2 and the 1x1 / stride 1 (shortcut) layers — all 19 binary convs of a
ResNet-18 — both run on hand-written MFMA kernels (``csrc/grad.hip``: g split into THREE bf16 terms hi + mid + lo — 24
mantissa bits and the exponent range of fp32, so gradients of a mean-reduced loss at batch 256 (1e-5 .. 1e-9) keep
fp32 accuracy — the ternary side exact in bf16, three ``v_mfma_f32_16x16x32_bf16`` per product, fp32 accumulation), with
the STE mask fused into the input-gradient store; any other geometry uses ``aten::convolution_backward``.
``W_hat = weight_pre_process(W)`` is computed by the hook under autograd, which makes the weight gradient flow exactly
as in the reference composition; the forward kernel re-derives the packed form of the same weights on every training
forward (``fastpath.packed_weight(..., fresh=True)``).  The forward is ONE launch (``bnn_hip_bconv2d_direct``:
``sign(x)`` on the fly in LDS, no packed copy of the activations in HBM).  What it keeps for the backward is the fp32
``x`` by default, or — ``PACKED_STATE`` — THREE BITS per input element: the sign planes and the mask ``|x| < 1``
(``bnn_hip_pack_act_ste_f32``, one extra pass over x) instead of the fp32 ``x`` and fp32 ``sign(x)`` the reference's
autograd keeps alive; the gradient kernels read the planes (``bnn_hip_bconv_grad_*_packed_f32``) and return the same
bits as from the fp32 tensor.

Grouped and depthwise layers (``groups > 1``: the BATS cells' ``SepConv`` / ``DilConv``) take the same autograd
function under ``GROUPED``: ``pack_act_ste`` + ``bnn_hip_bconv2d_grouped`` forward, and — where
``hipops.grouped_grad_supported`` says so — the fp32 VALU gradient kernels of ``csrc/grad_grouped.hip`` on the three bit
planes, which are then ALL that is kept of the input; other grouped geometries keep the fp32 ``x`` for
``aten::convolution_backward`` with ``groups``.

The backward of a binary layer is written ONCE and every autograd function of this module calls it
(``BinaryConv2dTrainFn``, ``CellOpTrainFn``, both phases of ``ReduceTrainFn``; ``BinaryLinearTrainFn`` and the operator
``torch.ops.bnn_amd.binary_linear`` for a ``Linear``):

    _bconv_backward / blinear_backward(g, kept input, weight, ..., wconf) -> (gx, gw)
        sign fragments of the weight (dense) or the fp32 What (grouped; a Linear reads the forward's pack)
        -> the input-gradient kernel, STE mask fused
        -> the weight-gradient kernel's split-K slabs
        -> ``_weight_grad_from_slabs``: more than 16 slabs added first, then ``xnor_weight_backward``

``wconf = (center, compute_alpha)``: the weight is the LATENT one and the XNORWeightBinarizer is inside (the fused weight
hook, ``FUSED_WEIGHT_HOOK``); ``wconf = None``: the weight is ``What = weight_pre_process(W)``, made under autograd by the
caller, and the slabs are summed into dL/dWhat.  What a forward keeps of its input as bit planes goes through ``_keep`` /
``_kept`` (which also counts ``saved_input_bytes``), and the rules by which ``cell_op_train`` / ``reduce_train`` /
``conv2d_train`` / ``linear_train`` / ``bn_act_applies`` admit a module are the named predicates ``_batch_stat_bn``,
``_fusable_binary_conv``, ``_fused_weight_hook``, ``_f32_on_one_device`` and ``_no_hooks``.

Data-parallel training is ordinary ``DistributedDataParallel`` over RCCL (backend ``"nccl"``), one
process per GPU: the binary layers are ``nn.Module``s with ordinary fp32 Parameters, so gradient
bucketing / all-reduce needs nothing special (``make_ddp``).
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn

from . import hipops

ENABLED = True  # set False to force the torch composition in training (tests compare the two)
BINARY_GRADS = True  # False: library fp32 gradient convolutions for every layer (tests / A-B timing)
# Keep 3 bits per input element for the backward (sign planes + STE mask) instead of the fp32 input: 10.7x less saved
# state per binary convolution, same gradients bit for bit, +8 % step time on ResNet-18 at batch 256 (32.0 vs 29.5 ms:
# the weight-gradient kernel's fill extracts bits and issues two plane loads per element).  Off by default (speed);
# BNN_AMD_TRAIN_PACKED_STATE=1 or `training.PACKED_STATE = True` turns it on (memory).
PACKED_STATE = os.environ.get("BNN_AMD_TRAIN_PACKED_STATE", "0") == "1"


_saved_bytes = 0     # bytes of layer INPUT state the binary convolutions have kept for their backward since the last reset


def saved_input_bytes(reset: bool = False) -> int:
    """Bytes of input state (fp32 ``x``, or its three bit planes) the training forwards of the binary convolutions have
    saved for the backward since the last reset — what ``PACKED_STATE`` shrinks (tests, tools/bench_train.py)."""
    global _saved_bytes
    n = _saved_bytes
    if reset:
        _saved_bytes = 0
    return n


# Grouped / depthwise layers (the BATS cells' SepConv / DilConv) on the HIP path in a training step: pack_act_ste +
# bnn_hip_bconv2d_grouped forward, the gradient kernels of csrc/grad_grouped.hip backward, the three bit planes as all
# that is kept of the input.  Off by default (its speed against the library's grouped convolutions is recorded in
# profiles/grouped_train_bench.jsonl; the default is a later decision); BNN_AMD_TRAIN_GROUPED=1 or
# `training.GROUPED = True` turns it on — read at every call (fastpath.plan_conv2d_train).
GROUPED = os.environ.get("BNN_AMD_TRAIN_GROUPED", "0") == "1"


def _keep(ctx, acts, *tensors, nbytes: int = 0) -> None:
    """Save the bit planes of the ``SavedAct``s ``acts`` and then ``tensors`` on ``ctx`` for ``_kept``, and count the
    planes' bytes (plus ``nbytes``: an fp32 input kept in their place) into ``saved_input_bytes``."""
    global _saved_bytes
    ctx.save_for_backward(*[t for sv in acts for t in (sv.sign.P, sv.sign.M, sv.T)], *tensors)
    ctx.act_shapes = [tuple(sv.shape) for sv in acts]
    _saved_bytes += nbytes + sum(sv.nbytes() for sv in acts)


def _kept(ctx):
    """``(acts, tensors)`` as ``_keep`` was given them."""
    ts, shapes = ctx.saved_tensors, ctx.act_shapes
    acts = [hipops.SavedAct(hipops.PackedAct(ts[3 * i], ts[3 * i + 1], shape), ts[3 * i + 2], shape)
            for i, shape in enumerate(shapes)]
    return acts, ts[3 * len(shapes):]


def _weight_grad_from_slabs(w, slabs, wconf):
    """dL/dW of the latent weight ``w`` from the split-K slabs ``[splits, *w.shape]`` of dL/dWhat, through the fused
    weight hook."""
    # up to 16 slabs are added inside the hook's kernel (one workgroup per output channel walks them), the hundreds of a
    # 64-channel layer by the library's parallel reduction
    if slabs.shape[0] > 16:
        slabs = slabs.sum(0)
    return hipops.xnor_weight_backward(w, slabs, *wconf)


def _bconv_backward(g, x, w, geom, need_x, need_w, wconf):
    """``(gx, gw)`` of one binary convolution on the binary-aware kernels.  ``x``: the kept input (fp32, or its
    ``SavedAct``; a grouped layer keeps planes only); ``geom = (groups, stride, padding, dilation)`` picks the dense or the
    grouped kernels; ``wconf``: module docstring (``gw`` is dL/dW with it, dL/dWhat without)."""
    groups, stride = geom[0], geom[1]
    latent = wconf is not None
    gx = gw = None
    if groups != 1:
        if need_x:      # the grouped kernel reads the fp32 What (wave-uniform per group), not sign fragments
            gx = hipops.bconv_grouped_grad_input(g, x, hipops.xnor_what(w, *wconf) if latent else w, *geom)  # STE mask fused
        if need_w:
            gw = hipops.bconv_grouped_grad_weight(g, x, w.shape, *geom, reduce=not latent)
    else:
        if need_x:      # (latent: one launch, the same bytes)
            packed, alpha = hipops.xnor_grad_pack_weight(w, *wconf) if latent else hipops.grad_pack_weight(w)
            gx = hipops.bconv_grad_input(g, x, packed, alpha, w.shape[2], stride[0])               # STE mask fused
        if need_w:
            gw = hipops.bconv_grad_weight(g, x, w.shape[2], stride[0], reduce=not latent)
    if need_w and latent:
        gw = _weight_grad_from_slabs(w, gw, wconf)
    return gx, gw


def blinear_backward(g, saved, packed, w, wconf, need_x, need_w):
    """``(gx, gw)`` of one binary ``Linear``: ``g`` as ``[M, O]``, ``saved`` the planes of the ``[M, F]`` input, ``packed``
    the forward's weight pack; ``gx`` is ``[M, F]``.  ``wconf``: module docstring."""
    gx = gw = None
    if need_x:
        gx = hipops.blinear_grad_input(g, saved, packed)                                           # STE mask fused
    if need_w:
        gw = hipops.blinear_grad_weight(g, saved, reduce=wconf is None)
        if wconf is not None:
            gw = _weight_grad_from_slabs(w, gw, wconf)
    return gx, gw


def _forward_and_keep(ctx, x, w, bias, layer, packed):
    """Forward of ``BinaryConv2dTrainFn``, and what it keeps of ``x`` for the backward (``w``: the tensor saved next to
    it).  Dense layer: ONE launch, the fp32 ``x`` kept — or, ``PACKED_STATE``, its three bit planes where the gradient
    kernels cover the geometry.  Grouped layer: the planes are made first (the forward reads the sign planes) and are
    ALL that is kept where the grouped gradient kernels cover the geometry; otherwise the fp32 ``x`` for the library's
    backward.  Returns ``(out, (stride, padding, dilation))``."""
    stride, padding, dilation = tuple(layer.stride), tuple(layer.padding), tuple(layer.dilation)
    groups = int(layer.groups)
    sv = None
    if groups != 1:
        sv = hipops.pack_act_ste(x)
        out = hipops.bconv2d_grouped(sv.sign, packed, bias, None, stride, padding, dilation)
        planes = BINARY_GRADS and hipops.grouped_grad_supported(x.shape, w.shape, groups, stride, padding, dilation)
    else:
        out = hipops.bconv2d_direct(x, packed, bias, None, stride, padding, dilation)   # one launch
        planes = PACKED_STATE and BINARY_GRADS and hipops.grad_supported(x.shape, w.shape, stride, padding, dilation)
        if planes:
            # the gradient kernels need sign(x) and the mask |x| < 1: three bit planes (3/32 of the fp32 tensor the
            # reference's autograd keeps alive until the backward)
            sv = hipops.pack_act_ste(x)
    if planes:
        _keep(ctx, [sv], w)
    else:
        _keep(ctx, [], x, w, nbytes=x.numel() * x.element_size())
    ctx.groups = groups
    return out, (stride, padding, dilation)


def _library_backward(ctx, g, x, w_hat, conf, need):
    """``aten::convolution_backward`` on ``sign(x)`` and the hard-tanh STE mask (bnn/ops.py:68-73)."""
    stride, padding, dilation, has_bias, bias_shape = conf
    gx, gw, gb = torch.ops.aten.convolution_backward(
        g, torch.sign(x), w_hat, list(bias_shape) if has_bias else None, list(stride), list(padding), list(dilation),
        False, [0, 0], ctx.groups, [bool(v) for v in need])
    if need[0]:
        gx = gx.masked_fill(x.abs() >= 1, 0)
    return gx, gw, gb


class BinaryConv2dTrainFn(torch.autograd.Function):
    """``wconf``: module docstring (``w`` is the latent weight with it, ``What`` without)."""

    @staticmethod
    def forward(ctx, x, w, bias, layer, packed, wconf):
        out, (stride, padding, dilation) = _forward_and_keep(ctx, x, w, bias, layer, packed)
        ctx.conf = (stride, padding, dilation, bias is not None, None if bias is None else tuple(bias.shape))
        ctx.wconf = wconf
        return out

    @staticmethod
    def backward(ctx, g):
        stride, padding, dilation, has_bias, bias_shape = ctx.conf
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], has_bias and ctx.needs_input_grad[2]
        acts, rest = _kept(ctx)
        x, w = (acts[0], rest[0]) if acts else rest     # x: the fp32 input, or the SavedAct of its planes
        wconf = ctx.wconf
        g = g.contiguous()
        # the binary-aware kernels: always when only the planes were kept, else for a dense layer they cover (a grouped
        # layer that kept its fp32 input takes the library's backward)
        if acts or (ctx.groups == 1 and BINARY_GRADS and hipops.grad_supported(x.shape, w.shape, stride, padding, dilation)):
            gx, gw = _bconv_backward(g, x, w, (ctx.groups, stride, padding, dilation), need_x, need_w, wconf)
            gb = g.sum(dim=(0, 2, 3)) if need_b else None
        else:
            what = w if wconf is None else hipops.xnor_what(w, *wconf)
            gx, gw, gb = _library_backward(ctx, g, x, what, ctx.conf, (need_x, need_w, need_b))
            if need_w and wconf is not None:
                gw = _weight_grad_from_slabs(w, gw[None], wconf)        # (one slab)
        return (gx if need_x else None, gw if need_w else None, gb if need_b else None, None, None, None)


# ---- training-mode BatchNorm (+ residual) (+ ReLU) as one fused op ---------------------------------------------------
# Of the 29.5 ms ResNet-18 step at batch 256, 9.1 ms were the library's BatchNorm kernels and 6 ms its ReLU / add /
# their backward passes over the same fp32 tensors.  `bn_act` evaluates  act(bn(x) (+ identity))  of the reference's
# blocks (bnn/models/layers/res_block.py:40-56) in three launches forward and three backward (csrc/bn_train.hip).
FUSED_BN = os.environ.get("BNN_AMD_TRAIN_FUSED_BN", "1") == "1"


class BNActFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, residual, bn, relu):
        # the kernels address NCHW: what is SAVED must be the contiguous tensor they ran on (a channels_last / strided
        # input would otherwise reach the backward kernels with its own strides: wrong dx, dgamma, dbeta)
        x = x.contiguous()
        if residual is not None:
            residual = residual.contiguous()
        y, mean, invstd = hipops.bn_train_forward(x, weight, bias, bn.running_mean, bn.running_var,
                                                  _momentum(bn), bn.eps, relu, residual)
        _stats_written(bn)
        ctx.relu, ctx.has_res = relu, residual is not None
        ctx.save_for_backward(x, y if relu else None, mean, invstd, weight)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, y, mean, invstd, weight = ctx.saved_tensors
        dx, dgamma, dbeta, dres = hipops.bn_train_backward(gy.contiguous(), y, x, mean, invstd, weight,
                                                           want_dres=ctx.has_res and ctx.relu and ctx.needs_input_grad[3])
        if ctx.has_res and ctx.needs_input_grad[3] and dres is None:
            dres = gy            # no ReLU in between: the residual's gradient IS the incoming one
        return (dx if ctx.needs_input_grad[0] else None, dgamma if ctx.needs_input_grad[1] else None,
                dbeta if ctx.needs_input_grad[2] else None, dres, None, None)


def _stats_written(bn: nn.BatchNorm2d) -> None:
    """The kernel has updated ``running_mean`` / ``running_var`` through raw pointers: bump their version counters (what an
    in-place torch op would have done — caches keyed on ``_version``, e.g. ``tails.cached_fold``, must see the
    change) and count the batch."""
    for t in (bn.running_mean, bn.running_var):
        if t is not None:
            torch.autograd.graph.increment_version(t)
    if bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)


def _momentum(bn: nn.BatchNorm2d) -> float:
    if bn.momentum is None:     # cumulative moving average (torch: 1 / num_batches_tracked, counted before the update)
        return 1.0 / float(int(bn.num_batches_tracked) + 1)
    return float(bn.momentum)


def _no_hooks(*modules, backward: bool = True) -> bool:
    """None of ``modules`` (``None`` entries skipped) carries a forward or forward-pre hook — nor, ``backward``, a
    backward or backward-pre hook: a fused op that stands in for the modules would not fire them."""
    return not any(m._forward_hooks or m._forward_pre_hooks or (backward and (m._backward_hooks or m._backward_pre_hooks))
                   for m in modules if m is not None)


def _f32_on_one_device(x: torch.Tensor, *tensors) -> bool:
    """``x`` and ``tensors`` are fp32 on the HIP device of ``x``."""
    return all(t.is_cuda and t.device == x.device and t.dtype == torch.float32 for t in (x, *tensors))


def _batch_stat_bn(bn) -> bool:
    """A stock ``nn.BatchNorm2d`` (no subclass) in training mode that normalises with batch statistics and has both
    running statistics for the kernels to update."""
    return (type(bn) is nn.BatchNorm2d and bn.training and bn.track_running_stats and bn.running_mean is not None
            and bn.running_var is not None)


def bn_act_applies(bn: nn.Module, act, x: torch.Tensor) -> bool:
    """The fused op stands in for ``act(bn(x) [+ identity])`` iff: ``_batch_stat_bn``, ``act`` None or a stock
    ``nn.ReLU``, fp32 NCHW on a HIP device with more than one value per channel (with one, the module raises "Expected
    more than 1 value per channel": it must get to), autograd recording, and no forward hooks on either module."""
    return (FUSED_BN and ENABLED and _batch_stat_bn(bn) and (act is None or type(act) is nn.ReLU)
            and _f32_on_one_device(x) and x.dim() == 4 and x.numel() > x.shape[1] and torch.is_grad_enabled()
            and (bn.weight is None or bn.weight.dtype == torch.float32) and _no_hooks(bn, act, backward=False))


def bn_act(x: torch.Tensor, bn: nn.BatchNorm2d, act=None, residual=None) -> torch.Tensor:
    """``act(bn(x) (+ residual))`` — fused when ``bn_act_applies``, else the modules themselves."""
    if bn_act_applies(bn, act, x):
        return BNActFn.apply(x, bn.weight, bn.bias, residual, bn, act is not None)
    y = bn(x)
    if residual is not None:
        y = y + residual
    return y if act is None else act(y)


class StemTailFn(torch.autograd.Function):
    """``maxpool(relu(bn1(x)))`` of the stem (bnn/models/resnet.py:150-153), training mode: the normalised tensor is
    never written; one byte per pooled output routes the gradient back (csrc/bn_train.hip, "stem tail")."""

    @staticmethod
    def forward(ctx, x, weight, bias, bn):
        x = x.contiguous()   # (see BNActFn.forward)
        p, code, mean, invstd = hipops.bn_relu_maxpool_train_forward(x, weight, bias, bn.running_mean, bn.running_var,
                                                                    _momentum(bn), bn.eps)
        _stats_written(bn)
        ctx.save_for_backward(x, p, code, mean, invstd, weight)
        ctx.mark_non_differentiable(code)
        return p, code

    @staticmethod
    def backward(ctx, gp, _gcode):
        x, p, code, mean, invstd, weight = ctx.saved_tensors
        dx, dgamma, dbeta = hipops.bn_relu_maxpool_train_backward(gp.contiguous(), p, code, x, mean, invstd, weight)
        return (dx if ctx.needs_input_grad[0] else None, dgamma if ctx.needs_input_grad[1] else None,
                dbeta if ctx.needs_input_grad[2] else None, None)


# The stem's convolution in a training step (bnn/models/resnet.py:150): the library's 7x7 forward is 1.2 ms of a 19.6 ms
# step at batch 256; the inference stem's MFMA core with a raw-conv epilogue (csrc/stem_rows.hip, RAW) is ~0.4 ms.  The
# weight gradient stays the library's (the input is data: no input gradient).
FUSED_STEM_CONV = os.environ.get("BNN_AMD_TRAIN_STEM_CONV", "1") == "1"
FUSED_STEM_WGRAD = os.environ.get("BNN_AMD_TRAIN_STEM_WGRAD", "1") == "1"


class StemConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x, w)
        return hipops.stem7x7_conv(x, w)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        if not ctx.needs_input_grad[0] and FUSED_STEM_WGRAD and hipops.stem7x7_wgrad_supported(x):
            # the input is data: the weight gradient is the whole backward (csrc/stem_wgrad.hip: fp32 MFMA, 0.6 ms
            # where the library's implicit GEMM with its two NHWC transposes of the 822 MB gradient takes 1.46)
            return None, (hipops.stem7x7_wgrad(x, g.contiguous()) if ctx.needs_input_grad[1] else None)
        gx, gw, _ = torch.ops.aten.convolution_backward(
            g.contiguous(), x, w, None, [2, 2], [3, 3], [1, 1], False, [0, 0], 1,
            [bool(ctx.needs_input_grad[0]), bool(ctx.needs_input_grad[1]), False])
        return (gx if ctx.needs_input_grad[0] else None, gw if ctx.needs_input_grad[1] else None)


def stem_conv_applies(conv: nn.Module, x: torch.Tensor) -> bool:
    """``conv(x)`` is the canonical real-valued stem convolution in a training step on a HIP device: a stock
    ``nn.Conv2d`` (or a binary-class layer whose recipe is all-Identity, examples/cifar10.py:71) 3 -> 64, 7x7, stride 2,
    padding 3, no bias, fp32 NCHW, no hooks."""
    from .executor import _is_float_layer
    return (FUSED_STEM_CONV and ENABLED and isinstance(conv, nn.Conv2d) and _is_float_layer(conv)
            and conv.in_channels == 3 and conv.out_channels == 64 and tuple(conv.kernel_size) == (7, 7)
            and tuple(conv.stride) == (2, 2) and tuple(conv.padding) == (3, 3) and tuple(conv.dilation) == (1, 1)
            and conv.groups == 1 and conv.bias is None and conv.padding_mode == "zeros"
            and _f32_on_one_device(x) and x.dim() == 4 and x.is_contiguous()
            and conv.weight.dtype == torch.float32 and torch.is_grad_enabled() and _no_hooks(conv)
            and not torch.is_autocast_enabled())      # (under AMP the reference's conv returns fp16: the module itself)


def stem_conv(x: torch.Tensor, conv: nn.Module) -> torch.Tensor:
    """``conv(x)`` — the MFMA kernel when ``stem_conv_applies``, else the module itself."""
    if stem_conv_applies(conv, x):
        return StemConvFn.apply(x, conv.weight)
    return conv(x)


def stem_tail(x: torch.Tensor, bn: nn.Module, act: nn.Module, pool: nn.Module) -> torch.Tensor:
    """``pool(act(bn(x)))`` — one fused op when it is BatchNorm2d (training) -> ReLU -> MaxPool2d(3, 2, 1) on a HIP
    device, else the modules themselves."""
    if (bn_act_applies(bn, act, x) and act is not None and type(pool) is nn.MaxPool2d
            and pool.kernel_size in (3, (3, 3)) and pool.stride in (2, (2, 2)) and pool.padding in (1, (1, 1))
            and pool.dilation in (1, (1, 1)) and not pool.ceil_mode and not pool.return_indices
            and _no_hooks(pool, backward=False)):
        return StemTailFn.apply(x, bn.weight, bn.bias, bn)[0]
    return pool(bn_act(x, bn, act))


# The shortcut's AvgPool2d(2, 2) in a training step (bnn/models/resnet.py:128-133): the library's forward, and a streaming
# kernel for its backward (the library's generic avg_pool2d backward: 0.53 ms per ResNet-18 step at batch 256, this 0.09).
FUSED_SHORTCUT_POOL = os.environ.get("BNN_AMD_TRAIN_SHORTCUT_POOL", "1") == "1"


class AvgPool2x2Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return torch.nn.functional.avg_pool2d(x, 2)

    @staticmethod
    def backward(ctx, g):
        return hipops.avgpool2x2_backward(g.contiguous())


def shortcut_pool(x: torch.Tensor, pool: nn.Module) -> torch.Tensor:
    """``pool(x)`` — with the streaming backward when it is ``AvgPool2d(2, 2)`` without padding on an even-sized fp32 map of
    a HIP device under autograd, else the module itself."""
    if (FUSED_SHORTCUT_POOL and ENABLED and type(pool) is nn.AvgPool2d and pool.kernel_size in (2, (2, 2))
            and pool.stride in (2, (2, 2)) and pool.padding in (0, (0, 0)) and pool.divisor_override is None
            and _f32_on_one_device(x) and x.dim() == 4 and x.shape[2] % 2 == 0 and x.shape[3] % 2 == 0
            and torch.is_grad_enabled() and x.requires_grad
            and _no_hooks(pool, backward=False) and not pool._backward_hooks):   # (backward-pre hooks were never asked)
        return AvgPool2x2Fn.apply(x)
    return pool(x)


# The weight hook of a training step as two kernels instead of torch's ~14 per layer (csrc/xnor_train.hip): the forward
# needs no fp32 What at all (the conv reads the packed weights), the backward derives What for the input-gradient
# kernel and maps dL/dWhat to dL/dW (sign STE, alpha = mean|Wc|, centring) in one kernel each.
FUSED_WEIGHT_HOOK = os.environ.get("BNN_AMD_TRAIN_FUSED_WEIGHT_HOOK", "1") == "1"


def _fused_weight_hook(layer: nn.Module, rank: int, backward_hooks: bool) -> bool:
    """The two kernels can stand in for ``layer.weight_pre_process`` (an XNORWeightBinarizer, by the layer's plan): the
    switch is on, the weight is contiguous of ``rank`` 4 (``Conv2d``; at most 1024 taps) or 2 (``Linear``), and the
    binarizer carries no forward hook — ``backward_hooks``: nor a backward hook (the per-layer functions never asked)."""
    w = layer.weight
    return (FUSED_WEIGHT_HOOK and w.dim() == rank and w.is_contiguous() and (rank == 2 or w.shape[2] * w.shape[3] <= 1024)
            and _no_hooks(layer.weight_pre_process, backward=backward_hooks))


def conv2d_train(layer: nn.Module, x: torch.Tensor, plan, packed) -> torch.Tensor:
    """``bnn.layers.Conv2d.forward`` with autograd recording: HIP forward; binary-aware HIP backward where the gradient
    kernels cover the layer (dense or — ``GROUPED`` — grouped), the library's otherwise."""
    if _fused_weight_hook(layer, 4, backward_hooks=False):
        w, wconf = layer.weight, (bool(plan.center), bool(plan.compute_alpha))
    else:
        w, wconf = layer.weight_pre_process(layer.weight), None     # autograd edge to W (sign STE, alpha)
    out = BinaryConv2dTrainFn.apply(x, w, layer.bias, layer, packed, wconf)
    if plan.scale is not None:                                      # BasicScaleBinarizer (bnn/ops.py:200-202)
        out = out * plan.scale
    return out


# ---- binary activations, real weights, in a training step ------------------------------------------------------------
# Step 0 of the reference's two-stage recipe (``weight: nn.Identity``): ``conv2d(sign(x), W, b)`` under autograd is sign(x)
# materialised in fp32, the library's fp32 convolution, and the fp32 x and fp32 sign(x) kept alive.  ``SignConvTrainFn`` is
# the layer as one autograd function (``fastpath.REAL_WEIGHTS``):
#   forward :  the weight fragments (re-packed on every forward) and ONE launch of csrc/sconv.hip; keeps x and W
#   backward:  gW = sum g sign(x): the weight-gradient kernel of csrc/grad.hip, which is the layer's whole dL/dW (the
#              weight hook is the identity); gx = the library's input gradient + the hard-tanh STE mask (g W has two real
#              operands and no ternary one: the three-term trick does not apply); gb = the sum of g.
class SignConvTrainFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias, stride):
        out = hipops.sconv2d(x, hipops.sconv_pack_weight(w), bias, None, stride)
        ctx.save_for_backward(x, w)
        ctx.stride, ctx.has_bias = int(stride), bias is not None
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        k, st = w.shape[2], ctx.stride
        g = g.contiguous()
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = torch.ops.aten.convolution_backward(g, x, w, None, [st, st], [k // 2, k // 2], [1, 1], False, [0, 0], 1,
                                                     [True, False, False])[0]
            gx = gx.masked_fill(x.abs() >= 1, 0)                    # hard-tanh STE (bnn/ops.py:68-73)
        if ctx.needs_input_grad[1]:
            gw = hipops.bconv_grad_weight(g, x, k, st, reduce=True)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            gb = g.sum((0, 2, 3))
        return gx, gw, gb, None


def sconv2d_train(layer: nn.Module, x: torch.Tensor, plan) -> torch.Tensor:
    """``bnn.layers.Conv2d.forward`` of a layer with an identity weight hook, autograd recording (``fastpath.
    plan_conv2d_real_train`` admitted it: dense, fp32, a geometry of ``hipops.sconv_supported``)."""
    out = SignConvTrainFn.apply(x, layer.weight, layer.bias, layer.stride[0])
    if plan.scale is not None:                                      # BasicScaleBinarizer (bnn/ops.py:200-202)
        out = out * plan.scale
    return out


# The ``Linear`` twin (csrc/slinear.hip), under the same switch:
#   forward :  the weight fragments (re-packed on every forward) and ONE launch that also writes the three bit planes of
#              x — all that is kept of it, with W
#   backward:  gx = the library's g W, then the hard-tanh STE mask in place from the T plane (bnn_hip_ste_mask_f32);
#              gW = sum_m g sign(x) from the sign planes (the weight-gradient kernel of csrc/blinear.hip), the layer's
#              whole dL/dW; gb = the sum of g.
class SignLinearTrainFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias):
        out, sv = hipops.slinear(x, hipops.slinear_pack_weight(w), bias, None, want_planes=True)
        _keep(ctx, [sv], w)
        ctx.x_shape, ctx.has_bias = tuple(x.shape), bias is not None
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (saved,), (w,) = _kept(ctx)
        g = g.reshape(-1, g.shape[-1]).contiguous()
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = hipops.ste_mask_(torch.mm(g, w), saved).reshape(ctx.x_shape)   # hard-tanh STE (bnn/ops.py:68-73)
        if ctx.needs_input_grad[1]:
            gw = hipops.blinear_grad_weight(g, saved, reduce=True)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            gb = g.sum(0)
        return gx, gw, gb


def slinear_train(layer: nn.Module, x: torch.Tensor, plan) -> torch.Tensor:
    """``bnn.layers.Linear.forward`` of a layer with an identity weight hook, autograd recording (``fastpath.
    plan_linear_real_train`` admitted it: fp32 on one HIP device, recognised hooks)."""
    out = SignLinearTrainFn.apply(x, layer.weight, layer.bias)
    if plan.scale is not None:                                      # BasicScaleBinarizer (bnn/ops.py:200-202)
        out = out * plan.scale
    return out


# ---- a binary Linear in a training step -----------------------------------------------------------------------------
# `F.linear(sign(x), What)` under autograd is sign(x) materialised in fp32, a library fp32 GEMM, and the fp32 x and fp32
# sign(x) kept alive.  `BinaryLinearTrainFn` is the layer as one autograd function on the kernels of csrc/blinear.hip:
#   forward :  ONE launch (bnn_hip_blinear_direct) that also writes the three bit planes of x — all that is kept of it
#   backward:  input gradient from the forward's weight pack and the mask plane, weight gradient from the sign planes as
#              partial slabs (both bf16 x 3 on the matrix cores), the slabs through the fused weight hook
# Off by default (its speed against the library's GEMMs is recorded in profiles/linear_bench.jsonl; the default is a later
# decision); BNN_AMD_TRAIN_LINEAR=1 or `training.LINEAR = True` turns it on — read at every call
# (fastpath.plan_linear_train).
LINEAR = os.environ.get("BNN_AMD_TRAIN_LINEAR", "0") == "1"


class BinaryLinearTrainFn(torch.autograd.Function):
    """``wconf``: module docstring (``w`` is the latent weight with it, ``What`` without)."""

    @staticmethod
    def forward(ctx, x, w, bias, packed, wconf):
        out, sv = hipops.blinear_direct(x, packed, bias, None, want_planes=True)
        _keep(ctx, [sv], w)
        ctx.packed, ctx.wconf, ctx.x_shape, ctx.has_bias = packed, wconf, tuple(x.shape), bias is not None
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (saved,), (w,) = _kept(ctx)
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        g = g.reshape(-1, g.shape[-1]).contiguous()
        gx, gw = blinear_backward(g, saved, ctx.packed, w, ctx.wconf, need_x, need_w)
        return (gx.reshape(ctx.x_shape) if need_x else None, gw, g.sum(0) if need_b else None, None, None)


def linear_train(layer: nn.Module, x: torch.Tensor, plan, packed) -> torch.Tensor:
    """``bnn.layers.Linear.forward`` with autograd recording (``fastpath.plan_linear_train`` admitted the layer, and
    with it ``weight_pre_process`` as one without forward hooks)."""
    if _fused_weight_hook(layer, 2, backward_hooks=False):
        w, wconf = layer.weight, (bool(plan.center), bool(plan.compute_alpha))
    else:
        w, wconf = layer.weight_pre_process(layer.weight), None     # autograd edge to W (sign STE, alpha)
    out = BinaryLinearTrainFn.apply(x, w, layer.bias, packed, wconf)
    if plan.scale is not None:                                      # BasicScaleBinarizer (bnn/ops.py:200-202)
        out = out * plan.scale
    return out


# ---- a whole BATS cell operation in a training step -----------------------------------------------------------------
# SepConv / DilConv / ReLUConvBN (bnn_amd/models/bats_ops.py) evaluate  y = [x +] channel_shuffle(PReLU(conv(sign(bn(x)))), 4)
# in train() mode as six steps (the library's BatchNorm, pack_act_ste, the convolution, torch PReLU, the shuffle's
# .contiguous() copy, torch add), and autograd keeps the BatchNorm output u and the convolution output z alive, each as
# large as the activation.  `CellOpTrainFn` is the whole operation as one autograd function:
#   forward :  batch statistics (csrc/bn_train.hip)  ->  BatchNorm + sign + STE mask as three bit planes, u never written
#              (csrc/pack_ste.hip)  ->  the fused convolution launch of the inference path (PReLU, shuffle, skip in its
#              epilogue)
#   kept    :  x (an input of the graph anyway), the three planes, mean / invstd, and the parameters — not u, z or y
#   backward:  z recomputed by the un-fused convolution launch on the kept planes and packed weight (the same bits the
#              epilogue saw)  ->  PReLU + shuffle backward (csrc/prelu_bwd.hip)  ->  the gradient kernels of the binary
#              convolution (_bconv_backward)  ->  BatchNorm backward with the skip's gradient added
#              in its dx kernel.
# Off by default (its speed against the per-layer path is recorded in profiles/cellops_train_bench.jsonl; the default is
# a later decision); BNN_AMD_TRAIN_CELL_OPS=1 or `training.CELL_OPS = True` turns it on — read at every call.
CELL_OPS = os.environ.get("BNN_AMD_TRAIN_CELL_OPS", "0") == "1"

CELL_OP_SHUFFLE = {"SepConv": 4, "DilConv": 4, "ReLUConvBN": 1}    # channel_shuffle(., 4) in SepConv / DilConv.forward


def _cell_conv(planes, packed, conf, prelu=None, residual=None):
    """The convolution launch of a cell operation on bit planes: with ``prelu`` / ``residual`` the fused forward, with
    neither the pre-activation value ``z`` its epilogue starts from."""
    groups, stride, padding, dilation, shuffle = conf
    if groups != 1:
        if prelu is None and residual is None:
            return hipops.bconv2d_grouped(planes, packed, None, None, stride, padding, dilation)
        return hipops.bconv2d_grouped_fused(planes, packed, None, None, stride, padding, dilation, prelu=prelu,
                                            shuffle_groups=shuffle, residual=residual)
    return hipops.bconv2d_fused(planes, packed, stride=stride, padding=padding, dilation=dilation, prelu=prelu,
                                residual=residual, residual_after_act=True)[0]


class CellOpTrainFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, gamma, beta, slope, bn, conf, packed, add_skip, wconf):
        x = x.contiguous()      # (see BNActFn.forward: what is saved is what the kernels ran on)
        sv, mean, invstd, _, _ = hipops.bn_train_pack_ste(x, gamma, beta, bn.running_mean, bn.running_var, _momentum(bn),
                                                          bn.eps)
        _stats_written(bn)
        O = w.shape[0]
        slopes = slope.detach().reshape(-1)
        y = _cell_conv(sv.sign, packed, conf, prelu=slopes.expand(O) if slopes.numel() == 1 else slopes,
                       residual=x if add_skip else None)
        # (the output is NOT saved: Cell.forward applies drop_path to it in place)
        _keep(ctx, [sv], x, mean, invstd, w, gamma, slope)
        ctx.packed, ctx.conf, ctx.add_skip, ctx.wconf = packed, conf, add_skip, wconf
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (saved,), (x, mean, invstd, w, gamma, slope) = _kept(ctx)
        shuffle = ctx.conf[4]
        need_x, need_w, need_gamma, need_beta, need_slope = ctx.needs_input_grad[:5]
        g = g.contiguous()
        z = _cell_conv(saved.sign, ctx.packed, ctx.conf)           # scratch: overwritten by gz, dies in here
        gz, gslope = hipops.prelu_shuffle_backward(g, z, slope, shuffle, inplace=True)
        need_u = need_x or need_gamma or need_beta
        gu, gw = _bconv_backward(gz, saved, w, ctx.conf[:4], need_u, need_w, ctx.wconf)
        dx = dgamma = dbeta = None
        if need_u:
            dx, dgamma, dbeta = hipops.bn_train_backward_add(gu, x, mean, invstd, gamma, g if ctx.add_skip else None)
        return (dx if need_x else None, gw, dgamma if need_gamma else None, dbeta if need_beta else None,
                gslope.reshape(slope.shape) if need_slope else None, None, None, None, None, None)


def _fusable_binary_conv(conv: nn.Module, plan) -> bool:
    """``conv`` with its ``fastpath._recognise`` ``plan`` can sit inside a fused training op: recognised hooks whose input
    binarizer has the hard-tanh STE (``plan.ste``: BasicInputBinarizer), no post scale, no bias, zero padding given as
    numbers."""
    return (plan is not None and plan.ste and plan.scale is None and conv.bias is None
            and not isinstance(conv.padding, str) and conv.padding_mode == "zeros")


def _binary_conv_plan(conv):
    """The plan of ``conv`` when it is a binary ``Conv2d`` under ``_fusable_binary_conv`` and ``_fused_weight_hook``
    (backward hooks included: nothing of a fused op fires), else None."""
    if not (isinstance(conv, nn.Conv2d) and hasattr(conv, "activation_pre_process")):
        return None
    from . import fastpath
    plan = fastpath._recognise(conv, conv.out_channels)
    return plan if _fusable_binary_conv(conv, plan) and _fused_weight_hook(conv, 4, backward_hooks=True) else None


def cell_op_train(op: nn.Module, x: torch.Tensor):
    """``op(x)`` of a ``SepConv`` / ``DilConv`` / ``ReLUConvBN`` in train() mode as ``CellOpTrainFn``, or None — the
    caller then runs the per-layer path — unless: the switches are on and autograd is recording without autocast; ``op.op``
    is ``Sequential(BatchNorm2d, binary Conv2d, PReLU)`` with ``_batch_stat_bn`` and ``_binary_conv_plan``; ``_no_hooks``
    on everything; the geometry is the operation's own and the gradient kernels cover it; ``_f32_on_one_device``, NCHW
    with more than one value per channel."""
    from . import fastpath
    shuffle = CELL_OP_SHUFFLE.get(type(op).__name__)
    seq = getattr(op, "op", None)
    if not (CELL_OPS and ENABLED and BINARY_GRADS and shuffle is not None and op.training
            and torch.is_grad_enabled() and not torch.is_autocast_enabled()
            and isinstance(seq, nn.Sequential) and len(seq) == 3):
        return None
    bn, conv, act = seq
    plan = _binary_conv_plan(conv) if _batch_stat_bn(bn) and type(act) is nn.PReLU else None
    if plan is None or not _no_hooks(op, seq, bn, conv, act, conv.activation_pre_process, conv.activation_post_process):
        return None
    w, C, O, groups = conv.weight, conv.in_channels, conv.out_channels, int(conv.groups)
    stride, padding, dilation = tuple(conv.stride), tuple(conv.padding), tuple(conv.dilation)
    grouped = shuffle != 1
    if grouped != (groups != 1) or O % shuffle or bn.num_features != C or act.weight.numel() not in (1, O) \
            or getattr(op, "stride", None) != stride[0] or stride[0] != stride[1] \
            or not isinstance(getattr(op, "skip", None), bool):
        return None
    if not grouped and (getattr(op, "C_in", None) != C or getattr(op, "C_out", None) != O):
        return None
    affine = [t for t in (bn.weight, bn.bias) if t is not None]
    if not (x.dim() == 4 and x.shape[1] == C and x.numel() > C
            and _f32_on_one_device(x, w, act.weight, bn.running_mean, bn.running_var, *affine)):
        return None
    supported = hipops.grouped_grad_supported(x.shape, w.shape, groups, stride, padding, dilation) if grouped \
        else hipops.grad_supported(x.shape, w.shape, stride, padding, dilation)
    if not supported:
        return None
    add_skip = op.skip and stride[0] == 1 and (grouped or C == O)
    packed = fastpath.packed_weight(conv, plan, sync=False, fresh=True)
    y = CellOpTrainFn.apply(x, w, bn.weight, bn.bias, act.weight, bn, (groups, stride, padding, dilation, shuffle), packed,
                            add_skip, (bool(plan.center), bool(plan.compute_alpha)))
    fastpath._bump("cell_op_train")
    return y


# ---- FactorizedReduce in a training step -----------------------------------------------------------------------------
# y = PReLU(cat(conv_1(sign(bn(x))), conv_2(sign(bn(x)[:, :, 1:, 1:]))))  with two 1x1 / stride-2 convolutions reads
# bn(x) at the pixels (2i, 2j) and (2i+1, 2j+1) only.  `ReduceTrainFn` is the module as one autograd function, behind the
# same switch as the cell operations (CELL_OPS):
#   forward :  batch statistics over all of x  ->  BatchNorm + sign + STE mask of the two lattices as bit planes at half
#              resolution (csrc/pack_ste.hip: bn_pack_ste_s2_kernel), u never written  ->  two dense 1x1 STRIDE-1
#              launches on the phase planes, each with its half of the PReLU slopes, stored into its half of y
#   kept    :  x, the two triples of planes, mean / invstd, the parameters — not u, the convolution outputs or y
#   backward:  z recomputed by the un-fused launches  ->  PReLU backward on the whole of g  ->  ONE copy of gz that makes
#              its two channel halves contiguous (the gradient kernels take contiguous tensors)  ->  per phase the 1x1
#              stride-1 gradient kernels of csrc/grad.hip (_bconv_backward)  ->  BatchNorm backward from the two
#              lattice gradients (csrc/bn_train.hip: bn_bwd_s2_reduce_kernel, bn_bwd_dx_s2_kernel), dx written once.
class ReduceTrainFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w1, w2, gamma, beta, slope, bn, packed, wconf):
        x = x.contiguous()      # (see BNActFn.forward: what is saved is what the kernels ran on)
        phases, mean, invstd, _, _ = hipops.bn_train_pack_ste_s2(x, gamma, beta, bn.running_mean, bn.running_var,
                                                                 _momentum(bn), bn.eps)
        _stats_written(bn)
        N, _, H, W = x.shape
        half = w1.shape[0]
        slopes = slope.detach().reshape(-1)
        if slopes.numel() == 1:
            slopes = slopes.expand(2 * half)
        y = torch.empty((N, 2 * half, H // 2, W // 2), dtype=torch.float32, device=x.device)
        for k in range(2):      # torch.cat in place, as cellops._Reduce.conv
            hipops.bconv2d_fused(phases[k].sign, packed[k], prelu=slopes[k * half:(k + 1) * half], out=y,
                                 out_c_offset=k * half)
        # (the output is NOT saved: Cell.forward applies drop_path to it in place)
        _keep(ctx, phases, x, mean, invstd, w1, w2, gamma, slope)
        ctx.packed, ctx.wconf = packed, wconf
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        saved, (x, mean, invstd, w1, w2, gamma, slope) = _kept(ctx)
        need_x, need_w1, need_w2, need_gamma, need_beta, need_slope = ctx.needs_input_grad[:6]
        g = g.contiguous()
        N, half = x.shape[0], w1.shape[0]
        z = torch.empty_like(g)                                    # scratch: overwritten by gz, dies in here
        for k in range(2):
            hipops.bconv2d_fused(saved[k].sign, ctx.packed[k], out=z, out_c_offset=k * half)
        gz, gslope = hipops.prelu_shuffle_backward(g, z, slope, 1, inplace=True)
        # the one extra pass over g: [N, 2, half, Ho, Wo] -> [2, N, half, Ho, Wo], each half contiguous
        gzk = gz.view(N, 2, half, *gz.shape[2:]).transpose(0, 1).contiguous()
        need_u = need_x or need_gamma or need_beta
        geom = (1, (1, 1), (0, 0), (1, 1))                         # the phases are dense 1x1 stride-1 convolutions
        (gu0, gw0), (gu1, gw1) = (_bconv_backward(gzk[k], saved[k], w, geom, need_u, need_w, ctx.wconf[k])
                                  for k, (w, need_w) in enumerate(((w1, need_w1), (w2, need_w2))))
        dx = dgamma = dbeta = None
        if need_u:
            dx, dgamma, dbeta = hipops.bn_train_backward_s2(gu0, gu1, x, mean, invstd, gamma)
        return (dx if need_x else None, gw0, gw1, dgamma if need_gamma else None, dbeta if need_beta else None,
                gslope.reshape(slope.shape) if need_slope else None, None, None, None)


def reduce_train(m: nn.Module, x: torch.Tensor):
    """``m(x)`` of a ``FactorizedReduce`` in train() mode as ``ReduceTrainFn``, or None — the caller then runs the module's
    own forward — unless: the switches are on and autograd is recording without autocast; the module is ``bn`` /
    ``conv_1`` / ``conv_2`` / ``activation`` as ``cellops._Reduce`` recognises it, with ``_batch_stat_bn`` and, for both
    convolutions, ``_binary_conv_plan``; both are 1x1 / stride 2 / padding 0 / ``groups == 1`` over the BatchNorm's
    channels; ``_no_hooks`` on everything; ``_f32_on_one_device``, NCHW with even ``H`` and ``W`` and
    more than one value per channel; the 1x1 stride-1 gradient kernels cover the half-resolution geometry; and a phase
    holds an even number of plane words (the second phase's planes are then 16-byte aligned, as the convolution launch
    requires)."""
    from . import fastpath
    if not (CELL_OPS and ENABLED and BINARY_GRADS and type(m).__name__ == "FactorizedReduce"
            and m.training and torch.is_grad_enabled() and not torch.is_autocast_enabled()):
        return None
    bn, act = getattr(m, "bn", None), getattr(m, "activation", None)
    seqs = [getattr(m, n, None) for n in ("conv_1", "conv_2")]
    if not (_batch_stat_bn(bn) and type(act) is nn.PReLU
            and all(isinstance(s, nn.Sequential) and len(s) == 1 for s in seqs)):
        return None
    convs = [s[0] for s in seqs]
    C, half = bn.num_features, getattr(convs[0], "out_channels", None)
    plans = [_binary_conv_plan(conv) for conv in convs]
    if any(p is None for p in plans):
        return None
    for conv in convs:
        if (conv.in_channels != C or conv.out_channels != half or conv.groups != 1 or tuple(conv.kernel_size) != (1, 1)
                or tuple(conv.stride) != (2, 2) or tuple(conv.padding) != (0, 0) or tuple(conv.dilation) != (1, 1)):
            return None
    if act.weight.numel() not in (1, 2 * half):
        return None
    if not _no_hooks(m, bn, act, *seqs, *convs, *[h for c in convs for h in (c.activation_pre_process,
                                                                             c.activation_post_process)]):
        return None
    affine = [t for t in (bn.weight, bn.bias) if t is not None]
    if not (x.dim() == 4 and x.shape[1] == C and x.numel() > C and x.shape[2] % 2 == 0 and x.shape[3] % 2 == 0
            and _f32_on_one_device(x, convs[0].weight, convs[1].weight, act.weight, bn.running_mean, bn.running_var,
                                   *affine)):
        return None
    N, _, H, W = x.shape
    if not hipops.grad_supported((N, C, H // 2, W // 2), (half, C, 1, 1), (1, 1), (0, 0), (1, 1)):
        return None
    # the planes of both phases are ONE phase-major allocation (what the pack launch writes) and the convolution launch
    # takes 16-byte aligned planes: phase 1 starts N * cw64 * H/2 * W/2 words of 8 bytes behind phase 0
    if (N * ((C + 63) // 64) * (H // 2) * (W // 2)) % 2:
        return None
    packed = tuple(fastpath.packed_weight(c, p, sync=False, fresh=True) for c, p in zip(convs, plans))
    y = ReduceTrainFn.apply(x, convs[0].weight, convs[1].weight, bn.weight, bn.bias, act.weight, bn, packed,
                            tuple((bool(p.center), bool(p.compute_alpha)) for p in plans))
    fastpath._bump("reduce_train")
    return y


def make_ddp(model: nn.Module, device: torch.device | None = None, **kw) -> nn.Module:
    """Wrap ``model`` for one-process-per-GPU data-parallel training (RCCL when on GPU, gloo on CPU).
    ``torch.distributed`` must be initialised.  Gradient buckets default to 64 MB: xGMI rings are
    per-link bound, so fewer, larger all-reduces beat the 25 MB default tuned for NVSwitch."""
    from torch.nn.parallel import DistributedDataParallel as DDP
    kw.setdefault("bucket_cap_mb", 64)
    if device is not None and device.type == "cuda":
        return DDP(model.to(device), device_ids=[device.index], output_device=device.index, **kw)
    return DDP(model, **kw)

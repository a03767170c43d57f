"""The fused executors: ``FusedResNet`` / ``FusedBlocks``.

The drop-in path (``prepare_binary_model`` + ``model(x)`` layer by layer) evaluates every binary conv as
pack -> XNOR/popcount -> fp32 NCHW and leaves BatchNorm / ReLU / residual adds to torch: each of
those is a full fp32 round trip through HBM.  For the block structure of the reference's ResNets
(``bnn/models/layers/res_block.py:40-56``: conv-BN-ReLU-conv-BN-(+identity)-ReLU) all of that
folds into the conv kernel's epilogue (``bnn_hip_epilogue``), so activations travel between
binary layers as bit planes and only the residual stream is ever written in fp32:

    conv1 -> BN1 -> ReLU            -> packed only                (no fp32 tensor at all)
    conv2 -> BN2 -> +identity -> ReLU -> fp32 (next identity) + packed (next conv1 input)
    shortcut: AvgPool(ceil) -> sign -> 1x1 binary conv -> BN, computed inside the block's conv2 launch

``FusedResNet`` shares the weights of the model it wraps; packed weights and folded BN constants
are derived once (call ``refresh()`` after changing parameters).  Eval mode only.  19 launches per ResNet-18
forward, eager or as HIP graphs (``capture``: whole forward over a static input; ``forward_fresh``: stem launch on the
caller's tensor + graph of the rest).

Part of what used to be one module, ``bnn_amd/inference.py`` (now a facade): executor.py (this file), pipeline.py
(several batches in flight), tails.py (the per-layer path's one-launch tails), dispatch.py (what ``model(x)`` /
``block(x)`` pick by themselves).
"""
from __future__ import annotations

import collections
import contextlib
import enum
import itertools
import os
from dataclasses import dataclass, field
from typing import Dict, List, NamedTuple, Optional, Tuple, Union

import torch
import torch.nn as nn
import torch.nn.modules.module as _mm

from . import fastpath, hipops, native
from .fastpath import Form
from .layers import Conv2d as BinaryConv2d
from .models.blocks import BasicBlock, Bottleneck, HBlock, PreBasicBlock, PreBottleneck
from .models.resnet import ResNet


class FusionError(RuntimeError):
    """The model (or a layer's recipe) is outside what the fused executor covers."""


def fold_bn(bn: nn.BatchNorm2d):
    """Eval-mode BatchNorm as one fused multiply-add per channel, ``y = fma(x, scale, shift)``, with the
    constants rounded exactly as the reference's forward rounds them.

    The reference evaluates ``bnN(...)`` with ATen's CPU kernel, which computes (all fp32)
    ``scale = weight * (1 / sqrt(var + eps))``, ``shift = fma(-mean, scale, bias)`` and
    ``out = fma(x, scale, shift)`` — measured: bit-identical on 1.6 M elements, whereas constants folded
    in double precision differ in the last bit for 34 % of the elements.  A last-bit difference in front
    of a ``sign()`` is a flipped activation, so the fold follows the reference's rounding, not the
    "more accurate" one.  Done on the host in numpy (IEEE-correct fp32 sqrt / divide), 64..512 values."""
    if not isinstance(bn, nn.BatchNorm2d) or bn.running_mean is None:
        raise FusionError(f"cannot fold {type(bn).__name__} (needs BatchNorm2d with running stats)")
    import numpy as np
    dev = bn.running_var.device
    var = bn.running_var.detach().float().cpu().numpy()
    mean = bn.running_mean.detach().float().cpu().numpy()
    gamma = bn.weight.detach().float().cpu().numpy() if bn.weight is not None else np.ones_like(var)
    beta = bn.bias.detach().float().cpu().numpy() if bn.bias is not None else np.zeros_like(var)
    inv = np.float32(1.0) / np.sqrt(var + np.float32(bn.eps), dtype=np.float32)
    scale = (gamma * inv).astype(np.float32)
    # fma(-mean, scale, bias): the product of two fp32 values is exact in fp64, one rounding to fp32 after the add
    shift = (beta.astype(np.float64) - mean.astype(np.float64) * scale.astype(np.float64)).astype(np.float32)
    return torch.from_numpy(scale).to(dev), torch.from_numpy(shift).to(dev)


def param_signature(module: nn.Module):
    """Changes whenever a parameter or buffer of ``module`` is replaced or written in place (optimizer step,
    ``load_state_dict``, ``.to()``): what was derived from them must then be rebuilt."""
    # a fresh walk every time: a Parameter that was REPLACED (setattr, a swapped sub-module) is a new object with
    # its own storage, which a list captured at refresh() time would never see
    return tuple((id(t), t.data_ptr(), t._version) for t in itertools.chain(module.parameters(), module.buffers()))


def inner_hooks(module: nn.Module, mods=None) -> bool:
    """Forward (pre-)hooks, global or on inner modules of ``module`` (``mods``: its ``modules()``, when the caller has
    them collected): they would not fire in a fused executor."""
    if _mm._global_forward_hooks or _mm._global_forward_pre_hooks:
        return True
    return any(m._forward_hooks or m._forward_pre_hooks
               for m in (module.modules() if mods is None else mods) if m is not module)


_TAP = None


@contextlib.contextmanager
def tap_binary_inputs(fn):
    """Debug/test hook: while active, ``fn(layer_name, PackedAct)`` is called with the bit planes every
    binary convolution of a ``FusedResNet`` reads (eager launches only — not during graph replay)."""
    global _TAP
    prev, _TAP = _TAP, fn
    try:
        yield
    finally:
        _TAP = prev


class RouteKey(NamedTuple):
    """One launch of a ``_Conv`` as ``_Conv.route`` sees it: all it asks about beyond the layer's own constants."""
    shape: Tuple[int, ...]                 # of the input planes
    nonneg: bool                           # the planes are non-negative (M is not read)
    residual: bool                         # an fp32 residual is added
    out_f32: bool
    out_packed: bool
    thr: bool                              # the sign bit comes from integer thresholds
    epi: Tuple[str, ...]                   # the ``epi`` switches that are on, sorted
    epi_off: Tuple[str, ...]               # those given as ``None`` / ``False``, sorted: present all the same
    shortcut: Optional[Tuple[int, ...]]    # shape of the folded shortcut's planes
    shortcut_w8: bool                      # the shortcut's weight has an int8 pack
    throughput: bool


# the ``epi`` switches a 1x1 launch on the FP4 kernel may carry -> their BNN_HIP_EPI_* flag (None: a tensor, no flag)
_EPI_1X1 = {"residual_after_act": native.EPI_RES_AFTER_ACT, "pack_before_residual": native.EPI_PACK_BEFORE_RES,
            "pack_relu": native.EPI_PACK_RELU, "pack_scale": None, "pack_shift": None}

# form -> (the ``hipops`` launch, the form under which ``_Conv.packs`` holds its weight pack, takes the shortcut's int8 pack)
_LAUNCH = {Form.POPCOUNT: ("bconv2d_fused", None, False),
           Form.I8_3X3: ("bconv2d_mfma_fused", Form.I8_3X3, False),
           Form.F4_3X3: ("bconv2d_mfma4_fused", Form.F4_3X3, False),
           Form.I8_FOLD: ("bconv2d_mfma_fold_fused", Form.I8_3X3, True),
           Form.F4_FOLD: ("bconv2d_mfma4_fold_fused", Form.F4_3X3, True),
           Form.F4_1X1: ("bconv1x1_mfma4_fused", Form.F4_1X1, False)}


@dataclass
class _Conv:
    layer: BinaryConv2d
    plan: fastpath.Plan
    weight: hipops.PackedWeight
    bn_scale: Optional[torch.Tensor]
    bn_shift: Optional[torch.Tensor]
    relu: bool
    prelu: Optional[torch.Tensor]
    name: str = ""
    throughput: bool = False   # BNN_HIP_FLAG_THROUGHPUT: several batches in flight (PipelinedInference)
    thr: Optional[torch.Tensor] = None   # integer sign thresholds of a BN + ReLU -> planes-only epilogue
    # the matrix-core packs of the weight, built with the plan: I8_3X3 / F4_3X3 (csrc/bconv_mfma.hip; the fold forms read
    # them too) and F4_1X1 (csrc/bconv1x1_mfma.hip).  A form without an entry has no pack for this weight
    packs: Dict[Form, torch.Tensor] = field(default_factory=dict)
    sc_w8: Optional[torch.Tensor] = None  # a block's shortcut convolution: int8 pack of its 1x1 weight (built with the plan)
    routes: Dict[RouteKey, Form] = field(default_factory=dict)   # the form of each launch seen so far, decided once

    def route(self, act: hipops.PackedAct, residual, out_f32: bool, out_packed: bool, thr, epi, shortcut_w8) -> Form:
        """The kernel form of one launch, decided once per ``RouteKey``: the switches and tables of ``fastpath`` (shapes
        that measured faster) and the kernels' own queries.  Each form needs all of its line:

        * ``F4_1X1``: the 1x1 FP4 pack exists; every key of ``epi`` is one of ``_EPI_1X1`` (so not a channel window, a
          caller's ``out`` or the folded shortcut); ``pack_scale`` and ``pack_shift`` are both on or both off;
          ``fastpath.mfma_1x1_admitted``; ``bconv1x1_mfma4_supported`` for this epilogue, flags and pack affine included.
        * ``I8_3X3`` / ``F4_3X3``: the int8 pack exists; ``epi`` has no key at all, on or off;
          ``fastpath.mfma_conv_admitted``; ``bconv2d_mfma_supported``.
        * ``I8_FOLD`` / ``F4_FOLD``: no residual; the int8 pack and ``shortcut_w8`` exist; ``epi`` is exactly the shortcut;
          fp32 and planes are both written; the layer has no bias and no post-scale, a BatchNorm, ReLU, no PReLU and a 3x3
          kernel; ``fastpath.mfma_fold_admitted``; ``bconv2d_mfma_fold_supported``.
        * ``POPCOUNT`` otherwise.

        A 3x3 or fold launch so admitted takes the FP4 form where the FP4 pack exists too and ``fastpath.mfma_f4_admitted``
        (its dense or fold key) and the form's ``mfma4`` query say yes.  No launch meets two of the lines — a weight has
        a 1x1 pack or 3x3 packs, never both, and the 3x3 and fold lines want a different ``epi`` — so their order is moot."""
        on, off, sc = (), (), None
        if epi:
            on = tuple(sorted([name for name, v in epi.items() if v is not None and v is not False]))
            off = tuple(sorted(set(epi).difference(on))) if len(on) != len(epi) else ()
            sc = tuple(epi["shortcut"][0].shape) if "shortcut" in on else None
        k = RouteKey(tuple(act.shape), act.nonneg, residual is not None, out_f32, out_packed, thr is not None, on, off, sc,
                     shortcut_w8 is not None, self.throughput)
        form = self.routes.get(k)
        if form is None:
            form = self.routes[k] = self._decide(k)
        return form

    def _decide(self, k: RouteKey) -> Form:
        lay, packs, w = self.layer, self.packs, self.weight
        C, O, H = k.shape[1], lay.out_channels, k.shape[2]
        names = set(k.epi + k.epi_off)
        f4 = Form.F4_3X3 in packs
        if Form.F4_1X1 in packs and names <= set(_EPI_1X1):
            flags = sum(_EPI_1X1[name] or 0 for name in k.epi)      # one bit each
            affine = "pack_scale" in k.epi
            if (affine == ("pack_shift" in k.epi) and fastpath.mfma_1x1_admitted(C, O, H, k.out_f32, k.nonneg)
                    and hipops.bconv1x1_mfma4_supported(k.shape, w, **self._epilogue(k), epi_flags=flags, pack_affine=affine)):
                return Form.F4_1X1
        if Form.I8_3X3 in packs and not names:
            stride = lay.stride[0] if isinstance(lay.stride, (tuple, list)) else lay.stride
            key, desc = (C, O, H, stride, False), self._epilogue(k)
            if fastpath.mfma_conv_admitted(*key) and hipops.bconv2d_mfma_supported(k.shape, w, **desc):
                f4 = f4 and fastpath.mfma_f4_admitted(key) and hipops.bconv2d_mfma4_supported(k.shape, w, **desc)
                return Form.F4_3X3 if f4 else Form.I8_3X3
        if (Form.I8_3X3 in packs and names == {"shortcut"} and k.shortcut is not None and k.shortcut_w8 and not k.residual
                and k.out_f32 and k.out_packed and lay.bias is None and self.plan.scale is None and self.bn_scale is not None
                and self.relu and self.prelu is None and tuple(lay.kernel_size) == (3, 3)):
            sc_C, sc_hw = k.shortcut[1], k.shortcut[2:]
            pooled = sc_hw == tuple(hipops.conv_out_hw(H, k.shape[3], 3, 3, lay.stride, lay.padding, lay.dilation))
            key, desc = (C, O, H, sc_C), dict(nonneg=k.nonneg, stride=lay.stride, padding=lay.padding, dilation=lay.dilation,
                                              unpooled_hw=None if pooled else sc_hw, throughput=k.throughput)
            if fastpath.mfma_fold_admitted(*key) and hipops.bconv2d_mfma_fold_supported(k.shape, w, sc_C, **desc):
                f4 = f4 and fastpath.mfma_f4_admitted(key) and hipops.bconv2d_mfma4_fold_supported(k.shape, w, sc_C, **desc)
                return Form.F4_FOLD if f4 else Form.I8_FOLD
        return Form.POPCOUNT

    def plain(self, **geometry) -> bool:
        """A plain binary convolution (no bias, post-scale, zero weight, PReLU or ReLU) whose layer has this ``geometry``:
        ``kernel_size`` / ``stride`` / ``padding`` / ``dilation``, whichever are given."""
        return (self.layer.bias is None and self.plan.scale is None and not self.weight.has_zero and self.prelu is None
                and not self.relu and all(tuple(getattr(self.layer, k)) == v for k, v in geometry.items()))

    def _epilogue(self, k: RouteKey) -> dict:
        """The launch ``k`` of this layer as the ``*_supported`` queries of ``hipops`` take it: what its epilogue contains."""
        lay = self.layer
        return dict(nonneg=k.nonneg, bias=lay.bias is not None, post_scale=self.plan.scale is not None,
                    bn=self.bn_scale is not None, residual=k.residual, prelu=self.prelu is not None, relu=self.relu,
                    out_f32=k.out_f32, out_packed=k.out_packed, stride=lay.stride, padding=lay.padding,
                    dilation=lay.dilation, sign_thresholds=k.thr)

    def run(self, act: hipops.PackedAct, *, residual=None, out_f32: bool, out_packed: bool, shortcut_w8=None, **epi):
        """``epi``: the pre-activation switches of ``hipops.bconv2d_fused`` (late residual, pack affine, ...);
        ``shortcut_w8``: the int8 pack of the weight in ``epi["shortcut"]``, where there is one."""
        lay = self.layer
        if _TAP is not None:
            _TAP(self.name, act)
        # BN + ReLU -> planes only (conv1 of a BasicBlock): the sign bit is an integer compare of the dot
        thr = self.thr if (out_packed and not out_f32 and residual is None and not epi) else None
        args = dict(bias=lay.bias, post_scale=self.plan.scale, bn_scale=self.bn_scale,
                    bn_shift=self.bn_shift, residual=residual, prelu=self.prelu, relu=self.relu,
                    out_f32=out_f32, out_packed=out_packed, stride=lay.stride, padding=lay.padding,
                    dilation=lay.dilation, throughput=self.throughput, sign_thresholds=thr, **epi)
        launch, pack, fold = _LAUNCH[self.route(act, residual, out_f32, out_packed, thr, epi, shortcut_w8)]
        packs = (() if pack is None else (self.packs[pack],)) + ((shortcut_w8,) if fold else ())
        return getattr(hipops, launch)(act, self.weight, *packs, **args)


def _plan_of(conv: nn.Module) -> fastpath.Plan:
    if not isinstance(conv, BinaryConv2d):
        raise FusionError(f"{type(conv).__name__} is not a binary Conv2d (run prepare_binary_model first)")
    plan = fastpath._recognise(conv, conv.out_channels)
    if plan is None or not fastpath._numeric_padding(conv):
        raise FusionError("layer recipe is not BasicInputBinarizer + XNORWeightBinarizer "
                          "(+ Identity | BasicScaleBinarizer)")
    return plan


def _is_float_layer(conv: nn.Module) -> bool:
    """True for a stock conv or a binary-class conv whose recipe is all-Identity (kept real-valued
    the way examples/cifar10.py:71 does it: custom_config_layers_name={'conv1': BConfig()})."""
    if not isinstance(conv, BinaryConv2d):
        return type(conv) is nn.Conv2d
    return (type(conv.activation_pre_process) is nn.Identity and type(conv.weight_pre_process) is nn.Identity
            and type(conv.activation_post_process).__name__ == "Identity")


# ---- one record per entry of ``FusedResNet._blocks``; ``kind`` is what ``_run_blocks`` branches on.  (eq=False: blocks
# are compared by identity.)  Fields behind "derived lazily" are caches: decided once, on first use ----------------------
@dataclass(eq=False)
class _Post:
    """BasicBlock / Bottleneck: conv-BN-act ... conv-BN-(+id)-act."""
    kind = "post"
    convs: List[_Conv]
    ds: Optional[_Conv] = None              # the binary shortcut convolution with its BatchNorm folded (_shortcut)
    pool: int = 0                           # kernel of the AvgPool2d(ceil) in front of ``ds``
    ds_float: Optional[nn.Module] = None    # a real-valued shortcut branch: runs as the torch modules it is
    # derived lazily (_fold_applies)
    fold_recipe: Optional[bool] = None      # the layers' recipes allow the shortcut inside the last convolution
    fold_geo: Dict[Tuple[int, int, int], bool] = field(default_factory=dict)   # (images per launch, H, W) -> the kernel does


@dataclass(eq=False)
class _Pre:
    """PreBasicBlock (K = 2) / PreBottleneck (K = 3): K times BN-conv-act, (+id)."""
    kind = "pre"
    bn: List[Tuple[torch.Tensor, torch.Tensor]]     # (scale, shift) of fold_bn: the BatchNorm in front of each convolution
    convs: List[_Conv]
    ds: Optional[_Conv] = None              # as in _Post
    pool: int = 0
    ds_float: Optional[nn.Module] = None


class HForm(enum.Enum):
    """How one hierarchical block runs at one geometry (``_H.route``)."""
    STEPS = "launch by launch"
    ONE = "hblock_forward"
    SHORTCUT = "hblock_shortcut_forward"        # the shortcut convolution inside the launch
    POOLED = "hblock_pool_forward"              # the stage's pool and both binarisations behind it inside the launch


class _HRoute(NamedTuple):
    form: HForm
    channel_lanes: bool = False                 # ONE / SHORTCUT in the small-image form (lanes = output channels, csrc/hblock_cl.hip)
    pool_consts: Optional[torch.Tensor] = None  # POOLED: ``hipops.hblock_pool_consts`` of the block behind the pool


def _hblock_env(name: str, default: str = "1") -> str:
    """``BNN_AMD_<name>``: FUSE_HBLOCK, read when an executor is built; HBLOCK_SHORTCUT, at ``refresh``;
    HBLOCK_CL, HBLOCK_POOL and HBLOCK_POOL_MIN (pixels), when ``_H.route`` first decides a geometry.  "0" switches off."""
    return os.environ.get("BNN_AMD_" + name, default)


def _is_pool2x2(m: nn.Module) -> bool:
    return isinstance(m, nn.AvgPool2d) and m.kernel_size in (2, (2, 2)) and m.stride in (2, (2, 2)) and m.padding in (0, (0, 0))


@dataclass(eq=False)
class _H:
    """HBlock: three BN-act-conv stages, cat, (+id)."""
    kind = "h"
    planes: int
    bn: List[Tuple[torch.Tensor, torch.Tensor]]     # bn1, bn2, bn3 folded
    relu: List[bool]                        # _sign_through of act1, act2, act3
    convs: List[_Conv]
    ds_bn: Optional[Tuple[torch.Tensor, torch.Tensor]] = None   # shortcut: BatchNorm -> binary 1x1 (no BN behind it)
    ds: Optional[_Conv] = None
    throughput: bool = False                # as ``_Conv.throughput``
    # filled by _link_hblocks
    next: Optional[object] = None           # the next block of the stage
    end_pool: Optional[nn.Module] = None    # the ``AvgPool2d(2, 2)`` that ends the stage behind this block ...
    behind: Optional[object] = None         # ... and the block behind that pool
    hpack: Optional[hipops.HBlockPack] = None       # constants of the one-launch forms; None: the block does not qualify
    hsc: Optional[Tuple[torch.Tensor, torch.Tensor]] = None     # hblock_shortcut_pack of ``ds``: it runs inside the launch
    routes: Dict[Tuple[int, int, int], _HRoute] = field(default_factory=dict)   # (N, H, W) -> how it runs, decided once

    def route(self, N: int, H: int, W: int) -> _HRoute:
        """How the block runs on ``N`` images of ``H`` x ``W``, decided once per geometry.  A lane form covers the geometry:
        channel lanes iff ``BNN_AMD_HBLOCK_CL`` is not "0", ``H == 7`` or several batches are in flight (``throughput``), and
        ``hblock_supported(..., channel_lanes=True)``; else pixel lanes iff ``hblock_supported``.  (Alone, the pixel-lane
        kernel splits a 14 x 14 image over two workgroups and fills the chip; measured at batch 128, us per block: 7 x 7 53.6
        vs 67.1; 14 x 14 shared 60.4 vs 72.0, alone 60.4 vs 44.8.)  Each form needs all of its line; the first that holds wins:

        * ``SHORTCUT``: ``hpack``, a lane form and ``hsc`` exist; ``hblock_shortcut_supported`` in that lane form.
        * ``POOLED``: ``hpack`` and a lane form exist; ``BNN_AMD_HBLOCK_POOL`` is not "0"; the stage ends behind the block in
          an ``AvgPool2d(2, 2)`` and the block ``behind`` that ``_takes_planes`` of this width and has a shortcut convolution
          (so nobody reads this block's fp32 output); ``H`` and ``W`` are even; the block keeps its width; ``H * W`` is at
          least ``BNN_AMD_HBLOCK_POOL_MIN`` (784); the block behind does not run ``STEPS`` at the halved geometry
          (``one_launch``); ``hblock_pool_supported``; ``hblock_pool_consts`` raises no ``NativeError`` (a scale that cannot
          take the average's 1 / 4 exactly).  Pixel lanes only.
        * ``ONE``: ``hpack`` and a lane form exist.
        * ``STEPS`` otherwise.  A run under ``tap_binary_inputs`` is ``STEPS`` too and never comes here (``_run_h``)."""
        r = self.routes.get((N, H, W))
        if r is None:
            r = self.routes[(N, H, W)] = self._decide(N, H, W)
        return r

    def _decide(self, N: int, H: int, W: int) -> _HRoute:
        hp, nb = self.hpack, self.behind
        if hp is None:
            return _HRoute(HForm.STEPS)
        geo = (N, hp.c_in, H, W, hp.planes, self.throughput)
        cl = _hblock_env("HBLOCK_CL") != "0" and (H == 7 or self.throughput) and hipops.hblock_supported(*geo, channel_lanes=True)
        if not (cl or hipops.hblock_supported(*geo)):
            return _HRoute(HForm.STEPS)
        if self.hsc is not None and hipops.hblock_shortcut_supported(*geo, channel_lanes=cl):
            return _HRoute(HForm.SHORTCUT, cl)
        if (_hblock_env("HBLOCK_POOL") != "0" and self.end_pool is not None and _takes_planes(nb, hp.planes)
                and nb.ds is not None and H % 2 == 0 and W % 2 == 0 and hp.c_in == hp.planes
                and H * W >= int(_hblock_env("HBLOCK_POOL_MIN", "784")) and nb.one_launch(N, H // 2, W // 2)
                and hipops.hblock_pool_supported(*geo)):
            with contextlib.suppress(native.NativeError):
                return _HRoute(HForm.POOLED, False, hipops.hblock_pool_consts(nb.bn[0], nb.ds_bn, hp.planes))
        return _HRoute(HForm.ONE, cl)

    def one_launch(self, N: int, H: int, W: int) -> bool:
        """What a producer asks before it writes this block's input planes and NO fp32 tensor (``_pool_into_hblock`` in front
        of a shortcut BatchNorm; ``POOLED``): ``t is None`` may reach a block only where it does not run launch by launch —
        ``STEPS`` binarises the fp32 tensor itself.  ``_run_h`` asserts it on the consumer's side."""
        return self.route(N, H, W).form is not HForm.STEPS


def _takes_planes(b, channels: int) -> bool:
    """A producer of ``channels`` channels may write block ``b``'s input planes, ``sign(relu(bn1(.)))``, itself."""
    return b is not None and b.kind == "h" and b.hpack is not None and b.relu[0] and b.hpack.c_in == channels


def _link_hblocks(blocks: list, fuse: bool, shortcut: bool) -> None:
    """Links every hierarchical block to its neighbours and, with ``fuse``, builds the one-launch pack of each that qualifies
    (csrc/hblock.hip): ReLU activations (all sign planes non-negative), plain 3x3 / stride 1 / padding 1 convolutions of
    a half, a quarter and a quarter of the block's width, a multiple of 64.  The launch also writes the NEXT block's input
    planes when that block is a hierarchical block behind a ReLU."""
    for b, nxt, nxt2 in zip(blocks, blocks[1:] + [None], blocks[2:] + [None, None]):
        if b.kind != "h":
            continue
        if nxt is not None and nxt.kind == "pool":
            if _is_pool2x2(nxt.mod) and nxt2 is not None:
                b.end_pool, b.behind = nxt.mod, nxt2
            nxt = None
        b.next = nxt
        convs, planes = b.convs, b.planes
        if not (fuse and all(b.relu)
                and all(c.plain(kernel_size=(3, 3), stride=(1, 1), padding=(1, 1), dilation=(1, 1)) for c in convs)
                and [c.layer.out_channels * k for c, k in zip(convs, (2, 4, 4))] == [planes] * 3 and planes % 64 == 0):
            continue
        nbn = nxt.bn[0] if (nxt is not None and nxt.kind == "h" and nxt.relu[0]
                            and nxt.convs[0].layer.in_channels == planes) else None
        try:
            b.hpack = hipops.hblock_pack(convs[0].weight, convs[1].weight, convs[2].weight, b.bn[1], b.bn[2], nbn)
        except native.NativeError:      # a width the one-launch kernel has no instance for
            continue
        # a stage's first block takes its shortcut convolution into the launch (bnn_hip_hblock_shortcut_forward): a plain
        # binary 1x1 behind its own BatchNorm (none behind it), and a next block in the stage
        sc = b.ds
        if (sc is not None and nbn is not None and sc.plain(kernel_size=(1, 1), stride=(1, 1), padding=(0, 0))
                and sc.bn_scale is None and sc.layer.in_channels * 2 == planes and shortcut):
            with contextlib.suppress(native.NativeError):
                b.hsc = hipops.hblock_shortcut_pack(sc.weight)


@dataclass(eq=False)
class _Pool:
    """``nn.AvgPool2d`` in front of a stage of hierarchical blocks."""
    kind = "pool"
    mod: nn.Module


@dataclass
class _Handoff:
    """Travels next to ``(t, packed)`` when ``packed`` is NOT ``sign(t)``: a launch wrote the input planes of ``owner``'s
    first binary convolution — ``owner``'s bn1 (and ReLU) already applied — and, in ``ds``, the planes of ``owner``'s
    shortcut BatchNorm when it wrote those too.  Only ``owner`` may read them (``_run_h`` / ``_run_pre`` test for it and
    pack again otherwise; every other reader of ``packed`` asserts that there is no hand-off)."""
    owner: Union[_Pre, _H]
    ds: Optional[hipops.PackedAct] = None


_BLOCK_KINDS = {"BasicBlock": BasicBlock, "PreBasicBlock": PreBasicBlock, "Bottleneck": Bottleneck,
                "PreBottleneck": PreBottleneck, "HBlock": HBlock}
_BLOCK_ATTRS = {BasicBlock: ("conv1", "bn1", "act1", "conv2", "bn2", "act2", "downsample"),
                PreBasicBlock: ("conv1", "bn1", "act1", "conv2", "bn2", "act2", "downsample"),
                Bottleneck: ("conv1", "bn1", "act1", "conv2", "bn2", "act2", "conv3", "bn3", "act3", "downsample"),
                PreBottleneck: ("conv1", "bn1", "act1", "conv2", "bn2", "act2", "conv3", "bn3", "act3", "downsample"),
                HBlock: ("conv1", "bn1", "act1", "conv2", "bn2", "act2", "conv3", "bn3", "act3", "downsample")}


def _block_kind(blk: nn.Module):
    """The block family ``blk`` belongs to: one of this package's classes (exact type), or a class of the same NAME
    and attribute layout from another package — the reference's own ``bnn.models.layers`` blocks, which these mirror
    attribute for attribute (res_block.py:8-56,59-118,121-167,170-229, hierarchical_block.py:8-60).  Foreign classes are
    only ever fused after ``AutoFusion`` has checked the fused result against the model's own forward."""
    t = type(blk)
    if t in _BLOCK_ATTRS:
        return t
    kind = _BLOCK_KINDS.get(t.__name__)
    if kind is not None and all(hasattr(blk, a) for a in _BLOCK_ATTRS[kind]):
        return kind
    return None


def is_native_model(model: nn.Module) -> bool:
    """True when ``model`` and all its residual blocks are this package's classes (their forward is known)."""
    return isinstance(model, ResNet) and all(
        type(b) in _BLOCK_ATTRS or isinstance(b, nn.AvgPool2d)
        for stage in (model.layer1, model.layer2, model.layer3, model.layer4) for b in stage)


def resnet_shaped(model: nn.Module) -> bool:
    """The module layout of the reference's ``bnn.models.resnet.ResNet`` (resnet.py:93-101,147-164)."""
    stem = getattr(model, "stem_type", "basic")
    need = ("conv1", "maxpool", "layer1", "layer2", "layer3", "layer4", "avgpool", "fc") + (("bn1",) if stem == "basic" else ())
    return stem in ("basic", "dabnn") and all(isinstance(getattr(model, a, None), nn.Module) for a in need) and \
        all(isinstance(getattr(model, a), nn.Sequential) for a in ("layer1", "layer2", "layer3", "layer4"))


def _activation(act: nn.Module):
    if isinstance(act, nn.ReLU):
        return True, None
    if isinstance(act, nn.PReLU):
        return False, act.weight.detach().float().contiguous()
    raise FusionError(f"unsupported activation {type(act).__name__}")


# HIP graphs (and side streams / events) of executors that were garbage-collected while the calling thread was capturing
# a HIP graph of its own: kept alive until the next executor is built outside a capture (``FusedResNet.__del__``)
_PARKED: list = []


class FusedResNet(nn.Module):
    """Inference executor for ``bnn_amd.models.ResNet`` built from ``BasicBlock`` (ResNet-18/34),
    ``Bottleneck`` (ResNet-50/101/152: mixed 1x1 / 3x3 binary convolutions), ``PreBasicBlock`` (the
    pre-activation dataflow of examples/imagenet.py), ``PreBottleneck`` (that dataflow with the 1x1 / 3x3 / 1x1
    convolutions of a Bottleneck) or ``HBlock`` (hierarchical blocks)."""

    def __init__(self, model: ResNet, use_mfma_stem: bool = True, overlap_shortcut: bool = True,
                 stem_fp16: bool = False, stem_exact_fp32: bool = False, throughput_mode: bool = False,
                 int_thresholds: bool = True, skip_dead_f32: bool = True, fold_shortcut: bool = True,
                 fuse_hblock: bool = True) -> None:
        super().__init__()
        if _PARKED and not torch.cuda.is_current_stream_capturing():
            _PARKED.clear()
        # a hierarchical block as ONE launch (bnn_hip_hblock_forward) instead of a packing pass + three convolutions
        self.fuse_hblock = fuse_hblock and _hblock_env("FUSE_HBLOCK") != "0"   # ("0": launch by launch, for A/B profiles)
        # the last conv of a block writes no fp32 tensor when the next block consumes sign planes only
        self.skip_dead_f32 = skip_dead_f32
        # BN + ReLU + sign of the conv1-type layers as an integer compare of the dot (same bits, fewer instructions)
        self.int_thresholds = int_thresholds
        # several batches in flight on other streams: kernels prefer fewer, longer waves (BNN_HIP_FLAG_THROUGHPUT)
        self.throughput_mode = throughput_mode
        self.stem_fp16 = stem_fp16           # opt-in: plain fp16 stem operands (~5e-4 relative error)
        self.use_mfma_stem = use_mfma_stem
        self.stem_exact_fp32 = stem_exact_fp32   # v_mfma_f32_16x16x4_f32: bit-for-bit an fp32 fmaf chain (slower)
        self.overlap_shortcut = overlap_shortcut
        # a down-sampling block's shortcut conv (AvgPool -> binary 1x1 -> BN) computed inside its last conv
        self.fold_shortcut = fold_shortcut
        self._side = {}
        self.model = model
        self._blocks: List[Union[_Post, _Pre, _H, _Pool]] = []
        self._graph = None
        self._split = collections.OrderedDict()   # (input shape, stream) -> _Split (forward_fresh)
        self.refresh()

    def __del__(self):
        # The executor is in a reference cycle with the model it wraps (the model's dispatch state holds the executor), so
        # it dies in whichever garbage collection finds it — possibly one that runs while the CALLER captures a HIP graph of
        # its own around a later ``net(x)``.  Destroying a graph is not an operation a capture admits (the HIP runtime
        # aborted the process there), so inside a capture the HIP objects are handed to ``_PARKED`` instead.
        try:
            held = [self.__dict__.get("_graph")] + [sp.graph for sp in self.__dict__.get("_split", {}).values()]
            held = [g for g in held if g is not None]
            if held and torch.cuda.is_current_stream_capturing():
                _PARKED.append((held, dict(self.__dict__.get("_side", {}))))
        except Exception:       # interpreter shutdown: nothing to protect any more
            pass

    def _conv(self, conv, bn, act) -> _Conv:
        plan = _plan_of(conv)
        relu, prelu = (False, None) if act is None else _activation(act)
        if prelu is not None and prelu.numel() != conv.out_channels:
            prelu = prelu.expand(conv.out_channels).contiguous()
        scale, shift = (None, None) if bn is None else fold_bn(bn)
        pw = fastpath.packed_weight(conv, plan)
        thr = None
        if (self.int_thresholds and scale is not None and relu and prelu is None and conv.bias is None
                and plan.scale is None and not pw.has_zero):
            thr = hipops.sign_thresholds(pw, scale, shift)
        # the matrix-core packs the switches make worth building (FP4 of a 3x3 only beside its int8 form)
        wanted, ksize, packs = fastpath.mfma_packs(), tuple(pw.shape[2:]), {}
        if Form.I8_3X3 in wanted and ksize == (3, 3):
            packs[Form.I8_3X3] = hipops.pack_weight_i8(pw)
            if Form.F4_3X3 in wanted and packs[Form.I8_3X3] is not None:
                packs[Form.F4_3X3] = hipops.pack_weight_f4(pw)
        if Form.F4_1X1 in wanted and ksize == (1, 1):
            packs[Form.F4_1X1] = hipops.pack_weight1x1_f4(pw)
        packs = {form: pack for form, pack in packs.items() if pack is not None}     # None: no such form for this weight
        return _Conv(conv, plan, pw, scale, shift, relu, prelu, self._names.get(id(conv), ""), self.throughput_mode, thr,
                     packs)

    @staticmethod
    def _sign_through(act: nn.Module):
        """How ``sign(act(v))`` is produced from ``v``: (relu_planes, ok).  ReLU: P = v > 0, M = 0.
        PReLU with positive slopes: sign(prelu(v)) == sign(v).  Anything else is not fused."""
        if isinstance(act, nn.ReLU):
            return True
        if isinstance(act, nn.PReLU) and bool((act.weight.detach() > 0).all()):
            return False
        raise FusionError(f"cannot binarise through {type(act).__name__} in a fused epilogue")

    def refresh(self) -> None:
        """(Re)derive packed weights and folded BN constants from the wrapped model.  Runs by itself when a
        parameter/buffer was replaced or written in place (version counters); call it by hand after writes
        through ``.data`` (they bypass the counters), then ``capture`` again if a graph was captured."""
        m = self.model
        if not resnet_shaped(m):
            raise FusionError("FusedResNet covers ResNets laid out like bnn.models.resnet.ResNet")
        native.require()
        fastpath.invalidate(m, executors=False)
        if m.training:
            raise FusionError("FusedResNet is inference-only: call model.eval() first")
        if m.fc.weight.device.type != "cuda":
            raise FusionError("FusedResNet needs the model on a HIP device")
        self._split.clear()     # graphs behind the stem hold pointers to the derived data rebuilt below
        self._stem = None
        mp = m.maxpool
        self._stem_module = getattr(m, "stem_type", "basic") != "basic"   # daBNN stem (resnet.py:10-47): m.conv1 is all of it
        if not self._stem_module and isinstance(mp, nn.MaxPool2d) and isinstance(m.bn1, nn.BatchNorm2d) \
                and mp.dilation in (1, (1, 1)) \
                and not mp.ceil_mode and isinstance(mp.kernel_size, int) and isinstance(mp.stride, int) \
                and isinstance(mp.padding, int):
            self._stem = (*fold_bn(m.bn1), (mp.kernel_size, mp.stride, mp.padding))
        c1 = m.conv1
        # the whole stem as one fp32-MFMA kernel when it is the canonical 7x7/2/3 conv + 3/2/1 pool
        self._stem_mfma = (self.use_mfma_stem and self._stem is not None and self._stem[2] == (3, 2, 1)
                           and isinstance(c1, nn.Conv2d) and c1.weight.shape == (64, 3, 7, 7)
                           and c1.stride == (2, 2) and c1.padding == (3, 3) and c1.dilation == (1, 1)
                           and c1.groups == 1 and c1.bias is None and c1.weight.dtype == torch.float32
                           and _is_float_layer(c1))
        # real-valued head (avgpool -> flatten -> fc, resnet.py:160-164) as one kernel when it is the canonical one
        fc, ap = m.fc, m.avgpool
        fc_float = _is_float_layer_linear(fc)
        self._head = None
        if fc_float and isinstance(ap, nn.AdaptiveAvgPool2d) and ap.output_size in (1, (1, 1)) \
                and fc.weight.dtype == torch.float32 and fc.in_features * 16 <= 160 * 1024:
            self._head = (fc.weight.detach().t().contiguous(), None if fc.bias is None else fc.bias.detach())
        self._plan(itertools.chain(m.layer1, m.layer2, m.layer3, m.layer4))

    def _plan(self, blocks) -> None:
        """The end of every ``refresh``: one record per block of ``blocks``, the hierarchical blocks linked."""
        self._blocks = []
        self._names = {id(mod): name for name, mod in self.model.named_modules()}
        for blk in blocks:
            self._add_block(blk)
        _link_hblocks(self._blocks, self.fuse_hblock, _hblock_env("HBLOCK_SHORTCUT") != "0")
        self._graph = None
        self._sig = param_signature(self.model)

    def _add_block(self, blk) -> None:
        """Derive the fused form of one residual block (appends to ``self._blocks``)."""
        if isinstance(blk, nn.AvgPool2d):   # HBlock stages pool in front (bnn_amd/models/resnet.py)
            self._blocks.append(_Pool(blk))
            return
        kind = _block_kind(blk)
        if kind is PreBasicBlock or kind is PreBottleneck:   # K times BN-conv-act, (+id)   (res_block.py:147-152,205-210)
            ks = (1, 2) if kind is PreBasicBlock else (1, 2, 3)
            entry = _Pre(bn=[fold_bn(getattr(blk, f"bn{i}")) for i in ks],
                         convs=[self._conv(getattr(blk, f"conv{i}"), None, getattr(blk, f"act{i}")) for i in ks])
            self._shortcut(blk, entry)
            self._blocks.append(entry)
            return
        if kind is HBlock:                  # three BN-act-conv stages, cat, (+id)  (hierarchical_block.py:38-60)
            entry = _H(planes=blk.conv1.out_channels * 2,
                       bn=[fold_bn(blk.bn1), fold_bn(blk.bn2), fold_bn(blk.bn3)],
                       relu=[self._sign_through(a) for a in (blk.act1, blk.act2, blk.act3)],
                       convs=[self._conv(c, None, None) for c in (blk.conv1, blk.conv2, blk.conv3)],
                       throughput=self.throughput_mode)
            if blk.downsample is not None:  # BN -> binary 1x1 (no BN behind it)
                bn, conv = blk.downsample[0], blk.downsample[1]
                entry.ds_bn, entry.ds = fold_bn(bn), self._conv(conv, None, None)
            self._blocks.append(entry)
            return
        if kind is BasicBlock:           # conv-BN-act, conv-BN-(+id)-act
            convs = [self._conv(blk.conv1, blk.bn1, blk.act1), self._conv(blk.conv2, blk.bn2, blk.act2)]
        elif kind is Bottleneck:         # 1x1-BN-act, 3x3-BN-act, 1x1-BN-(+id)-act  (res_block.py:98-118)
            convs = [self._conv(blk.conv1, blk.bn1, blk.act1), self._conv(blk.conv2, blk.bn2, blk.act2),
                     self._conv(blk.conv3, blk.bn3, blk.act3)]
        else:
            raise FusionError(f"unsupported block {type(blk).__name__}")
        entry = _Post(convs)
        self._shortcut(blk, entry)
        self._blocks.append(entry)

    def _shortcut(self, blk, entry) -> None:
        """AvgPool(ceil) -> binary 1x1 -> BN shortcut of bnn/models/resnet.py:128-133."""
        if blk.downsample is None:
            return
        pool, conv, bn = blk.downsample[0], blk.downsample[1], blk.downsample[2]
        if _is_float_layer(conv):
            # a real-valued shortcut convolution (examples/recepies/imagenet-baseline.yaml keeps
            # layerN.0.downsample.1 out of the binarisation): the branch runs as the torch modules it is
            entry.ds_float = blk.downsample
            return
        k = pool.kernel_size if isinstance(pool.kernel_size, int) else pool.kernel_size[0]
        if not (isinstance(pool, nn.AvgPool2d) and pool.ceil_mode and not pool.count_include_pad
                and pool.padding in (0, (0, 0))):
            raise FusionError("shortcut pooling must be AvgPool2d(k, k, ceil_mode=True, "
                              "count_include_pad=False)")
        entry.ds = self._conv(conv, bn, None)
        entry.pool = k
        # the int8 form of the shortcut weight, for the fold on the matrix cores (None: no such form, or switched off)
        if Form.I8_FOLD in fastpath.mfma_packs():
            entry.ds.sc_w8 = hipops.pack_shortcut_weight_i8(entry.ds.weight)

    @torch.no_grad()
    def _forward_impl(self, x: torch.Tensor) -> torch.Tensor:
        return self._back(*self._front(x))

    def _front(self, x: torch.Tensor, out=None):
        """The part that reads the input tensor: the real-valued stem (first layer stays float: examples/cifar10.py:71)
        -> (fp32 NCHW, sign planes, _Handoff | None).  ``out``: the ``(fp32, planes)`` of an earlier call to overwrite
        (one-kernel stem only)."""
        m = self.model
        if self._stem_mfma:
            # a hierarchical block behind the stem reads sign(relu(bn1(t))): the stem kernel writes THOSE planes (its own
            # packing pass over the fp32 tensor disappears); the hand-off tells _run_h whose planes they are
            b0 = self._blocks[0] if self._blocks else None
            aff = b0.bn[0] if (_takes_planes(b0, 64) and b0.ds is None and not self.stem_exact_fp32 and _TAP is None) else None
            t, pk = hipops.stem7x7(x, m.conv1.weight, self._stem[0], self._stem[1], exact_fp32=self.stem_exact_fp32,
                                   fp16=self.stem_fp16, out=out, pack_affine=aff)
            return t, pk, (_Handoff(b0) if aff is not None else None)
        if out is not None:
            raise FusionError("only the one-kernel stem writes into preallocated buffers")
        if self._stem is not None:   # the conv runs in the vendor library, its BN -> ReLU -> MaxPool -> sign tail in one pass
            t = m.conv1(x)
            return (*hipops.bn_relu_maxpool_pack(t, self._stem[0], self._stem[1], True, *self._stem[2]), None)
        # any other stem runs as the torch modules it is (binary layers inside it one launch each); the residual blocks
        # behind it are fused all the same
        t = m.conv1(x) if self._stem_module else m.maxpool(m.relu(m.bn1(m.conv1(x))))
        return t, hipops.pack_act(t), None

    def _back(self, t, packed, left) -> torch.Tensor:
        """Everything behind the stem: residual blocks + real-valued head (last layer stays float)."""
        m = self.model
        t = self._run_blocks(t, packed, left)
        if self._head is not None:
            return hipops.avgpool_fc(t, *self._head)
        return m.fc(torch.flatten(m.avgpool(t), 1))

    def _run_blocks(self, t, packed, left):
        """The residual blocks: ``t`` fp32 NCHW (may be None when only planes exist), ``packed`` its sign planes
        or None — or, with a hand-off ``left``, the planes ``left.owner`` reads.  Returns the fp32 output of the last block."""
        last = len(self._blocks) - 1
        for i, b in enumerate(self._blocks):
            nxt = self._blocks[i + 1] if i < last else None
            if b.kind == "pool":
                if t is None:               # the previous block's launch pooled and binarised its own output (POOLED)
                    assert left is not None and left.owner is nxt and nxt.one_launch(packed.shape[0], *packed.shape[2:])
                    continue
                # the pool + both sign planes the next stage's first block reads in one pass, where that applies
                t, packed, left = self._pool_into_hblock(b.mod, nxt, t) or (b.mod(t), None, None)
                continue
            if b.kind == "pre":
                t, packed, left = self._run_pre(b, nxt, t, packed, left)
                continue
            if b.kind == "h":
                t, packed, left = self._run_h(b, t, packed, left)
                continue
            assert left is None, "sign planes written for another block's first convolution"
            if packed is None:
                packed = hipops.pack_act(t)
            side = None
            fold = None   # (PackedAct, PackedWeight, bn_scale, bn_shift) of a shortcut conv folded into the last conv
            if b.ds is not None and self._fold_applies(b, packed):
                # the shortcut conv (1x1 over the OR-pooled sign planes) is computed inside the block's last conv: no
                # fp32 shortcut tensor, no 1x1 launch (bnn_hip_epilogue.sc_*)
                # (pool 2: the kernel ORs the 2 x 2 windows of the block's input planes itself — no OR-pool launch)
                sc_in = packed if b.pool in (0, 1, 2) else hipops.orpool_packed(packed, b.pool)
                if _TAP is not None:
                    _TAP(b.ds.name, hipops.orpool_packed(packed, b.pool) if b.pool > 1 else packed)
                fold = (sc_in, b.ds.weight, b.ds.bn_scale, b.ds.bn_shift)
                idn = None
            elif b.ds is not None:
                # the shortcut branch (HBM-bound avg-pool + a small 1x1 conv) is independent of the block's
                # first convs (ALU-bound): run it on a second stream and join before the residual is needed
                dev_ = packed.P.device      # (t is None when the previous block skipped its dead fp32 output)
                cur = torch.cuda.current_stream(dev_)
                side = self._side_stream(dev_) if self.overlap_shortcut else None
                if side is not None:
                    side.wait_stream(cur)
                with torch.cuda.stream(side) if side is not None else contextlib.nullcontext():
                    if b.pool > 1 and packed.nonneg:   # sign(avg of non-negative values) = OR of the sign bits
                        sc_in = hipops.orpool_packed(packed, b.pool)
                    elif b.pool > 1:
                        sc_in = hipops.avgpool_pack(t, b.pool)
                    else:
                        sc_in = packed
                    idn, _ = b.ds.run(sc_in, out_f32=True, out_packed=False)
                if side is not None:
                    if t is not None:
                        t.record_stream(side)
                    packed.P.record_stream(side)
                    sc_in.P.record_stream(side)
                    sc_in.M.record_stream(side)
            elif b.ds_float is not None:
                idn = b.ds_float(t)
            else:
                idn = t
            for c in b.convs[:-1]:              # activations travel between binary layers as bit planes
                _, packed = c.run(packed, out_f32=False, out_packed=True)
            if side is not None:
                cur.wait_stream(side)
                idn.record_stream(cur)
            # the fp32 output is dead when the next block reads sign planes only: its convs always do, its shortcut
            # does when it is AvgPool -> binary 1x1 (-> OR-pool of the planes of a non-negative tensor, or no pooling)
            c2 = b.convs[-1]
            dead_f32 = (self.skip_dead_f32 and nxt is not None and nxt.kind == "post" and nxt.ds is not None
                        and (nxt.pool <= 1 or (c2.relu and c2.prelu is None)))
            if fold is not None:
                t, packed = c2.run(packed, out_f32=True, out_packed=True, shortcut=fold, shortcut_w8=b.ds.sc_w8)
            else:
                t, packed = c2.run(packed, residual=idn, out_f32=not dead_f32, out_packed=i != last)
        return t

    def _fold_applies(self, b, packed) -> bool:
        """Whether the block's shortcut convolution can be computed inside its last convolution.  The recipe part is
        decided once per block; the kernel part (``hipops.shortcut_fold_supported``) depends on the geometry — image
        size and the images one launch covers (large batches are split) — and is cached per geometry.  Needs:
        non-negative sign planes in front of the block (an OR-pool then IS the avg-pool's sign), a bias-free 1x1 /
        stride-1 shortcut conv without post scale or zero weights, a last conv whose kernel takes the fold and whose
        fp32 output and sign planes are both wanted (a block in the middle of the net)."""
        if not self.fold_shortcut or not packed.nonneg:
            return False
        ds, c2 = b.ds, b.convs[-1]
        lay, c2l = ds.layer, c2.layer
        if b.fold_recipe is None:
            b.fold_recipe = bool(
                ds.plain(kernel_size=(1, 1), stride=(1, 1), padding=(0, 0)) and b is not self._blocks[-1] and len(b.convs) >= 2
                and all(c.relu and c.prelu is None for c in b.convs[:-1])
                and c2.relu and c2.prelu is None and c2.layer.bias is None and c2.plan.scale is None)
        if not b.fold_recipe:
            return False
        N, _, H, W = packed.shape
        k = max(b.pool, 1)
        ho, wo = -(-H // k), -(-W // k)
        n_launch = hipops.fused_launch_images(N, c2l.in_channels, ho, wo, c2l.out_channels, c2l.kernel_size,
                                              c2l.stride, c2l.padding, c2l.dilation)
        key = (n_launch, ho, wo)
        ok = b.fold_geo.get(key)
        if ok is None:
            probe = hipops.PackedAct(packed.P, packed.M, (n_launch, c2l.in_channels, ho, wo), nonneg=True)
            ok = b.fold_geo[key] = bool(hipops.shortcut_fold_supported(
                probe, c2.weight, lay.in_channels, c2l.stride, c2l.padding, c2l.dilation, throughput=c2.throughput))
        return ok

    def _side_stream(self, device) -> torch.cuda.Stream:
        key = (device.index, torch.cuda.current_stream(device).cuda_stream)
        if key not in self._side:
            self._side[key] = torch.cuda.Stream(device=device)
        return self._side[key]

    def _run_pre(self, b, nxt, t, packed, left):
        """PreBasicBlock / PreBottleneck: the block input travels as fp32 ``t`` (shortcut) and as ``sign(bn1(t))``; the
        latter comes out of the previous block's last epilogue (its ``pack_scale`` = this ``bn1``).  Every convolution but
        the last hands ``sign(bn_next(act(conv)))`` on as planes; the last adds the shortcut behind its activation."""
        if left is None or left.owner is not b:
            packed = hipops.bn_act_pack(t, *b.bn[0], relu=False)
        if b.ds is not None:
            sc_in = hipops.avgpool_pack(t, b.pool) if b.pool > 1 else hipops.pack_act(t)
            idn, _ = b.ds.run(sc_in, out_f32=True, out_packed=False)
        elif b.ds_float is not None:
            idn = b.ds_float(t)
        else:
            idn = t
        p1 = packed
        for c, bn in zip(b.convs[:-1], b.bn[1:]):
            _, p1 = c.run(p1, out_f32=False, out_packed=True, pack_scale=bn[0], pack_shift=bn[1])
        c2 = b.convs[-1]
        if nxt is not None and nxt.kind == "pre":   # binarise for the next block's conv1 right here
            t, pk = c2.run(p1, residual=idn, out_f32=True, out_packed=True, residual_after_act=True,
                           pack_scale=nxt.bn[0][0], pack_shift=nxt.bn[0][1])
            return t, pk, _Handoff(nxt)
        t, _ = c2.run(p1, residual=idn, out_f32=True, out_packed=False, residual_after_act=True)
        return t, None, None

    def _pool_into_hblock(self, pool, nxt, t):
        """``AvgPool2d(2, 2)`` in front of a hierarchical block that runs as one launch: the pooled tensor is only ever
        binarised — by the block's bn1 -> ReLU and by its shortcut's BatchNorm — so one pass writes both sets of planes
        and (when the block has a shortcut convolution) no fp32 tensor at all.  None: not that case."""
        N, C, H, W = t.shape
        if (_TAP is not None or not _is_pool2x2(pool) or H % 2 or W % 2 or not _takes_planes(nxt, C)
                or not nxt.one_launch(N, H // 2, W // 2)):
            return None
        p1, p2, tp = hipops.avgpool2_bn_pack2(t, nxt.bn[0], True, nxt.ds_bn, False, out_f32=nxt.ds_bn is None)
        return tp, p1, _Handoff(nxt, p2)

    def _run_h(self, b, t, packed=None, left=None):
        """HBlock: three BN-act-conv stages write their slice of the concatenated output in place, each adds its slice of
        the shortcut and hands ``sign(act(bn_next(o_k)))`` to the next stage.  Returns ``(y, planes of the next block's input
        | None, their _Handoff | None)``; ``packed`` / ``left``: what the previous block's launch left, for this block when
        ``left.owner is b``.  ``POOLED`` returns ``(None, planes of the next stage's first block, ...)``: its own output pooled."""
        mine = left is not None and left.owner is b     # planes the previous launch left for this block
        sp = left.ds if mine else None                  # planes of the shortcut's BatchNorm
        if b.ds is not None and sp is None:
            sp = hipops.bn_act_pack(t, *b.ds_bn, relu=False)
        N, _, H, W = (t if sp is None else sp).shape
        # a tap wants the planes in front of every convolution: launch by launch, and no route is asked for or kept
        r = _HRoute(HForm.STEPS) if _TAP is not None else b.route(N, H, W)
        assert t is not None or (mine and r.form is not HForm.STEPS), "no fp32 tensor in front of a launch-by-launch block"
        hp, thr = b.hpack, b.throughput
        if r.form is HForm.SHORTCUT:
            if not mine:
                packed = hipops.bn_act_pack(t, *b.bn[0], relu=True)
            y, pk = hipops.hblock_shortcut_forward(packed, hp, sp, b.hsc, throughput=thr, channel_lanes=r.channel_lanes)
            return y, pk, _Handoff(b.next)
        idn = t if sp is None else b.ds.run(sp, out_f32=True, out_packed=False)[0]
        if r.form is not HForm.STEPS:
            if not mine:
                packed = hipops.bn_act_pack(t, *b.bn[0], relu=True)
            if r.form is HForm.POOLED:
                p1, p2 = hipops.hblock_pool_forward(packed, hp, idn, r.pool_consts, throughput=thr)
                return None, p1, _Handoff(b.behind, p2)
            y, pk = hipops.hblock_forward(packed, hp, idn, out_packed=hp.has_next, throughput=thr, channel_lanes=r.channel_lanes)
            return y, pk, (_Handoff(b.next) if pk is not None else None)
        (c1, c2, c3), half, quarter = b.convs, b.planes // 2, b.convs[1].layer.out_channels
        p = hipops.bn_act_pack(t, *b.bn[0], relu=b.relu[0])
        y = torch.empty((t.shape[0], b.planes, t.shape[2], t.shape[3]), dtype=torch.float32, device=t.device)
        late = dict(residual=idn, residual_after_act=True, pack_before_residual=True, out=y, out_f32=True)
        for c, bn, relu, offset in zip((c1, c2), b.bn[1:], b.relu[1:], (0, half)):
            _, p = c.run(p, out_packed=True, out_c_offset=offset, pack_scale=bn[0], pack_shift=bn[1], pack_relu=relu, **late)
        c3.run(p, out_packed=False, out_c_offset=half + quarter, **late)
        return y, None, None

    def _slots(self):
        """(module dict, name) of every parameter / buffer slot of the wrapped model in the order of ``param_signature``
        (all parameters in module order, then all buffers; shared tensors once), collected once per refresh: the
        per-call staleness check reads the slots directly instead of walking the module tree (a ``net(x)`` call at
        batch 32 is host-bound: the tree walks were most of its 0.27 ms)."""
        mods = list(self.model.modules())
        slots, seen = [], set()
        for kind in ("_parameters", "_buffers"):
            for m in mods:
                d = getattr(m, kind)
                for k, t in d.items():
                    if t is not None and id(t) not in seen:
                        seen.add(id(t))
                        slots.append((d, k))
        return mods, slots

    def _unchanged(self) -> bool:
        """Cheap form of ``param_signature(self.model) == self._sig``: same triples read through the cached slots (no
        tree walk, early exit), plus the identity of every module's children (a swapped sub-module has other slots)."""
        cache = self.__dict__.get("_fast")
        if cache is None or cache[0] is not self._sig:
            if param_signature(self.model) != self._sig:
                return False
            mods, slots = self._slots()
            aligned = tuple((id(d[k]), d[k].data_ptr(), d[k]._version) for d, k in slots) == self._sig
            cache = self.__dict__["_fast"] = (self._sig, mods, slots if aligned else None,
                                              [(m._modules, tuple(m._modules.values())) for m in mods])
            return True
        _, mods, slots, children = cache
        if slots is None:                                   # (an unusual module tree: keep the plain comparison)
            return param_signature(self.model) == self._sig
        for (d, k), want in zip(slots, self._sig):
            t = d.get(k)
            if t is None or id(t) != want[0] or t._version != want[2] or t.data_ptr() != want[1]:
                return False
        for ch, snap in children:                           # a replaced / added / removed sub-module
            if len(ch) != len(snap) or any(a is not b for a, b in zip(ch.values(), snap)):
                return False
        return True

    def hooked(self) -> bool:
        """``inner_hooks`` of the wrapped model, over the module list cached by ``_unchanged``."""
        cache = self.__dict__.get("_fast")
        return inner_hooks(self.model, cache[1] if cache is not None and cache[0] is self._sig else None)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        self._check_current()
        if self._graph is not None and x.shape == self._gx.shape:
            if x.data_ptr() != self._gx.data_ptr():   # callers that fill `static_input` in place skip the copy
                self._gx.copy_(x, non_blocking=True)
            self._graph.replay()
            return self._gy
        return self._forward_impl(x)

    @property
    def static_input(self):
        """The graph's input buffer (None before ``capture``).  Writing the batch into it in place
        (e.g. as the destination of the host-to-device copy) and passing it to ``forward`` replays
        the graph without the extra device-to-device copy of the input (154 MB at batch 256)."""
        return getattr(self, "_gx", None) if self._graph is not None else None

    def capture(self, example: torch.Tensor) -> "FusedResNet":
        """Record the whole forward (for this input shape) into a HIP graph; later calls with the
        same shape replay it — no per-kernel launch cost on the host."""
        self._graph = None
        self._gx = example.clone()
        side = torch.cuda.Stream(device=example.device)
        side.wait_stream(torch.cuda.current_stream(example.device))
        with torch.cuda.stream(side):
            for _ in range(2):
                self._forward_impl(self._gx)
        torch.cuda.current_stream(example.device).wait_stream(side)
        g = torch.cuda.CUDAGraph()
        # thread_local: HIP calls of OTHER threads (the RCCL watchdog of an initialised process group, data-loader
        # pinning threads) must not invalidate the capture
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            self._gy = self._forward_impl(self._gx)
        self._graph = g
        return self

    # ---- fresh input every call: the stem reads the CALLER's tensor, a HIP graph replays the rest ------------------
    MAX_SPLIT_GRAPHS = 4

    @property
    def reads_caller_tensor(self) -> bool:
        """True when ``forward_fresh`` applies (the stem is the one-kernel MFMA stem)."""
        return bool(self._stem_mfma)

    def _check_current(self) -> None:
        if not self._unchanged():                 # weights changed since the packed forms were derived
            recapture = self._graph is not None
            self.refresh()
            if recapture:
                self.capture(self._gx)

    @torch.no_grad()
    def capture_fresh(self, example: torch.Tensor) -> "_Split":
        """HIP graph of everything BEHIND the stem for inputs shaped like ``example``.  The stem stays an ordinary
        launch that reads whatever tensor the caller passes and writes the graph's two static inputs (its fp32 output
        and sign planes) — so a new input tensor per call costs no staging copy (154 MB at batch 256) and no
        re-capture, and the host issues two calls per forward instead of 21."""
        if not self._stem_mfma:
            raise FusionError("forward_fresh needs the one-kernel stem (7x7/2/3 conv + BN + ReLU + 3/2/1 max-pool)")
        dev = example.device
        with torch.cuda.device(dev):
            cur = torch.cuda.current_stream(dev)
            t0, pk0, left0 = self._front(example)   # allocated on the stream that will replay (the key holds it)
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                for _ in range(2):
                    self._back(t0, pk0, left0)
            cur.wait_stream(side)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                gy = self._back(t0, pk0, left0)
        return _Split(g, t0, pk0, left0, gy)

    @torch.no_grad()
    def forward_fresh(self, x: torch.Tensor, clone: bool = True) -> torch.Tensor:
        """``forward`` for a caller that brings a NEW tensor every call (the reference's eval loop,
        examples/cifar10.py:147-149): stem launch on ``x`` + graph replay of the rest.  The graph for an input shape is
        captured on its first use (per stream; at most ``MAX_SPLIT_GRAPHS`` are kept).  Returns a fresh tensor unless
        ``clone=False`` (then: the graph's output buffer, overwritten by the next call with this shape)."""
        self._check_current()
        x = hipops._require_cuda_f32(x, "stem input")
        dev = x.device
        with torch.cuda.device(dev):
            key = (tuple(x.shape), torch.cuda.current_stream(dev).cuda_stream)
            sp = self._split.get(key)
            if sp is None:
                sp = self._split[key] = self.capture_fresh(x)
                while len(self._split) > self.MAX_SPLIT_GRAPHS:
                    self._split.popitem(last=False)
            else:
                self._split.move_to_end(key)
            _, _, left = self._front(x, out=(sp.t0, sp.pk0))
            # the graph reads pk0 as it was captured: as the planes of left0's owner, or as sign(t0)
            assert (left is None) == (sp.left0 is None), "the stem wrote other sign planes than the captured graph reads"
            sp.graph.replay()
            return sp.gy.clone() if clone else sp.gy


@dataclass
class _Split:
    graph: "torch.cuda.CUDAGraph"
    t0: torch.Tensor            # static fp32 output of the stem
    pk0: hipops.PackedAct       # static sign planes of the stem
    left0: Optional[_Handoff]   # whose planes pk0 holds when they are not sign(t0): the graph was captured reading them so
    gy: torch.Tensor            # static logits


class FusedBlocks(FusedResNet):
    """The fused executor for a bare ``nn.Sequential`` of residual blocks (``BasicBlock`` / ``Bottleneck`` /
    ``PreBasicBlock`` / ``PreBottleneck`` / ``HBlock``, optionally ``nn.AvgPool2d`` between them): fp32 NCHW in, fp32 NCHW
    out, the activations between the binary layers travel as bit planes exactly as inside ``FusedResNet``.  For custom
    networks that keep their own stem / head, and for testing the cross-block dataflow on its own."""

    _stem_mfma = False      # no stem: ``forward_fresh`` does not apply

    def __init__(self, blocks: nn.Sequential, throughput_mode: bool = False, int_thresholds: bool = True) -> None:
        # every other option: FusedResNet's default
        super().__init__(blocks, throughput_mode=throughput_mode, int_thresholds=int_thresholds)

    def refresh(self) -> None:
        native.require()
        fastpath.invalidate(self.model, executors=False)
        if self.model.training:
            raise FusionError("FusedBlocks is inference-only: call .eval() first")
        self._plan(self.model)

    @torch.no_grad()
    def _forward_impl(self, x: torch.Tensor) -> torch.Tensor:
        return self._run_blocks(hipops._require_cuda_f32(x, "activation"), None, None)


def _is_float_layer_linear(fc: nn.Module) -> bool:
    """A stock ``nn.Linear``, or a binary-class Linear whose recipe is all-Identity (examples/cifar10.py:71 keeps ``fc``
    real-valued that way)."""
    return type(fc) is nn.Linear or (
        isinstance(fc, nn.Linear) and type(getattr(fc, "activation_pre_process", None)) is nn.Identity
        and type(getattr(fc, "weight_pre_process", None)) is nn.Identity
        and type(getattr(fc, "activation_post_process", None)).__name__ == "Identity")

"""Dispatch of binary layers onto the HIP XNOR/popcount path.

A layer takes the HIP path when ALL of the following hold (otherwise the torch composition in
``layers/*.py`` — the reference's own formulation — runs):

* hooks are exactly ``BasicInputBinarizer`` (or, for inference, ``AdvancedInputBinarizer`` with its default
  ``tanh``, whose value is also ``sign(x)``) / ``XNORWeightBinarizer`` / (``Identity`` or a
  per-output-channel ``BasicScaleBinarizer``)      (reference: ``examples/cifar10.py:65-69``,
  ``test/test_layers.py:17-21``)
* on the same HIP device, input and weight are
  - both float32, or
  - both float16 (a ``.half()`` model: bit planes straight from the fp16 tensor, fp32 arithmetic inside, output rounded
    to fp16 once), or — inference only, ``lowp_dtype`` —
  - both bfloat16 (a ``.bfloat16()`` model), or
  - a 16-bit input of the autocast dtype with a float32 weight under ``torch.autocast("cuda", dtype=float16 | bfloat16)``
    (what every binary layer behind the first one sees there).  These two return a tensor of that 16-bit dtype ``D`` with
    the reference's own rounding points: the weight is ``weight_pre_process(weight).to(D)`` (its sign bits, its zeros and
    ``alpha[o] = max |What_D[o]|``: ``lowp_packed_weight``), the bias is rounded to ``D``, the result
    ``fmaf(alpha, dot, bias)`` is rounded to ``D`` and, with a ``BasicScaleBinarizer``, multiplied and rounded again
    (``hipops.round_lowp``; the one-launch kernel stores the 16 bits itself: ``LOWP_STORE_DECLINED_SHAPES``).  A float32
    input under autocast still returns float32; a 16-bit input with a float32 weight and no autocast reaches the
    composition; the fused executors and the real-weight path keep declining 16 bits
* autograd is not recording (``torch.no_grad()`` / inference); when it IS recording, ``Conv2d`` takes the
  training variant (HIP forward, binary-aware HIP gradient kernels or the library's fp32 backward with the
  straight-through estimator: ``bnn_amd/training.py``); ``Linear`` takes its own training variant under
  ``training.LINEAR`` (``BNN_AMD_TRAIN_LINEAR=1``, off by default: one HIP launch forward that keeps three bit planes
  of the input, bf16 x 3 matrix-core gradients from the weight pack and the planes: ``csrc/blinear.hip``) and the
  composition otherwise; ``Conv1d`` under autograd stays on the composition
* a ``Conv2d`` whose weight hook is the identity (binary activations, real weights: step 0 of the two-stage recipe) takes
  a path of its own under ``REAL_WEIGHTS`` (``BNN_AMD_REAL_WEIGHTS=1``, off by default): ``csrc/sconv.hip`` forward, in a
  training step ``training.SignConvTrainFn``; a ``Linear`` with these hooks takes ``csrc/slinear.hip`` under the same
  switch (one launch on the row-major input at every ``M``; ``training.SignLinearTrainFn`` in a training step, which
  keeps three bit planes of the input); ``Conv1d``, grouped layers and fp16 keep the composition
* ``padding_mode == 'zeros'``, numeric padding, and either ``groups == 1`` or — ``Conv2d`` / ``Conv1d`` under inference,
  ``Conv2d`` under autograd only with ``training.GROUPED`` — ``groups > 1`` (grouped and depthwise layers: ``pack_act``
  + ``bnn_hip_bconv2d_grouped``, two launches; the ResNet executors keep declining them, and so does the training
  forward by default; inside a BATS cell operation of ``bnn_amd.models`` the layer runs as part of
  ``cellops.FusedCellOp``)

When those hold and ``libbnn_hip.so`` cannot be loaded the call raises ``NativeError``: there is
no CPU or eager stand-in for the GPU path.

Packed weights (1 bit + 1 mask bit per weight, alpha per channel) are derived data: they are
cached on the layer, keyed on the weight's storage pointer and version counter, and rebuilt after
``load_state_dict`` / ``.to()`` / optimiser steps.  The fp32 ``weight`` Parameter stays the source
of truth (reference: ``bnn/layers/conv.py:111-112`` shares it with the float module).
"""
from __future__ import annotations

import enum
import os
import threading
import warnings
import weakref
from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn as nn

from . import hipops, native

_stats_lock = threading.Lock()
_stats = {"conv2d": 0, "conv1d": 0, "linear": 0, "weight_packs": 0, "conv2d_train": 0, "cell_op": 0, "cell": 0,
          "cell_op_train": 0, "reduce_train": 0, "linear_train": 0, "conv2d_real": 0, "conv2d_real_train": 0,
          "linear_real": 0, "linear_real_train": 0, "fconv": 0}

# Binary activations with REAL weights (step 0 of the reference's two-stage recipe, examples/recepies/imagenet-baseline.yaml:
# ``weight: nn.Identity``) on the HIP path: ``Conv2d`` layers whose weight hook is the identity take csrc/sconv.hip (one
# launch from the fp32 input, three bf16 matrix-core products per weight) instead of the torch composition, in ``eval()``
# and in a training step.  Off by default (its speed against the composition is recorded in profiles/sconv_bench.jsonl;
# the default is a later decision); BNN_AMD_REAL_WEIGHTS=1 or ``fastpath.REAL_WEIGHTS = True`` turns it on — read at
# every call (``plan_conv2d_real`` / ``plan_conv2d_real_train``).  With it off nothing here runs.
REAL_WEIGHTS = os.environ.get("BNN_AMD_REAL_WEIGHTS", "0") == "1"


class Form(str, enum.Enum):
    """The kernel form one binary-convolution launch of the fused ResNet executor takes (``executor._Conv.route``).  A
    ``str`` too, so that a member hashes in C, as its value does: it is a dict key on every eager launch."""
    POPCOUNT = "popcount"      # bnn_hip_bconv2d_fused: the XNOR-popcount kernels, every launch no other form admits
    I8_3X3 = "int8-3x3"        # bnn_hip_bconv2d_mfma_fused
    F4_3X3 = "fp4-3x3"         # bnn_hip_bconv2d_mfma4_fused
    I8_FOLD = "int8-fold"      # bnn_hip_bconv2d_mfma_fold_fused: a 3x3 launch with the block's shortcut folded in
    F4_FOLD = "fp4-fold"       # bnn_hip_bconv2d_mfma4_fold_fused
    F4_1X1 = "fp4-1x1"         # bnn_hip_bconv1x1_mfma4_fused


def _admitted(own: str, key: tuple, table: dict, parents: tuple = ()) -> bool:
    """The switch rule of every matrix-core form, in one place.  ``own``: the form's switch; ``parents``: the switches
    that turn it off too.  "0" in any of them -> no; else ``own == "all"`` -> yes; else ("1") -> ``key`` is in ``table``."""
    return "0" not in (own, *parents) and (own == "all" or key in table)


def mfma_packs() -> frozenset:
    """The forms whose weight pack is worth building under the current switches, asked when an executor plans its layers:
    ``I8_3X3`` / ``F4_3X3`` — the int8 / FP4 pack of a 3x3 weight; ``I8_FOLD`` — the int8 pack of a shortcut's 1x1 weight;
    ``F4_1X1`` — the FP4 pack of a 1x1 weight."""
    own = {Form.I8_3X3: MFMA_CONV, Form.F4_3X3: MFMA_F4, Form.I8_FOLD: MFMA_FOLD, Form.F4_1X1: MFMA_1X1}
    return frozenset(form for form, switch in own.items() if "0" not in (switch, MFMA_CONV))


# The dense 3x3 convolutions of the fused ResNet executor on the int8 matrix cores (csrc/bconv_mfma.hip: the same integer
# dot from v_mfma_i32_16x16x64_i8, the same float epilogue, the same bits) instead of the XNOR-popcount kernels.
# BNN_AMD_MFMA_CONV: "1" (default) — the launches listed in MFMA_CONV_SHAPES; "0" — none, the popcount launches as
# before; "all" — every launch bnn_hip_bconv2d_mfma_supported takes (for measuring a new shape).  Read when an executor
# plans its layers (``FusedResNet.refresh``), never during a graph capture.
MFMA_CONV = os.environ.get("BNN_AMD_MFMA_CONV", "1")
# The admission rule, in one place: (C, O, H of the input, stride, folded shortcut) -> (popcount us, MFMA us) of that
# launch in a kernel trace of one ResNet-18 forward at batch 256 on MI355X, one batch in flight
# (profiles/mfma_conv_kernel_roofline.md).  A shape is listed only where the MFMA launch measured faster.
MFMA_CONV_SHAPES = {
    (128, 128, 28, 1, False): ((51.9, 37.8), (58.6, 45.2)),   # layer2.1.conv1, layer2.1.conv2
    (128, 256, 28, 2, False): ((30.3, 26.2),),                # layer3.0.conv1
    (256, 256, 14, 1, False): ((54.9, 33.4), (56.9, 38.9)),   # layer3.1.conv1, layer3.1.conv2
    (256, 512, 14, 2, False): ((33.6, 23.8),),                # layer4.0.conv1
    (512, 512, 7, 1, False): ((60.6, 32.0), (63.3, 39.2)),    # layer4.1.conv1, layer4.1.conv2
    # measured slower or level, left on the popcount kernels:
    #   (64, 64, 56, 1, False)   layer1.*.conv1 51.6 -> 49.2, 51.2 -> 48.0 but layer1.*.conv2 81.2 -> 86.2, 63.3 -> 69.6
    #                            (the fp32 residual and output streams: 54 us of HBM time, not hidden behind the MFMAs)
    #   (64, 128, 56, 2, False)  layer2.0.conv1 28.9 -> 30.0
    # the folded shortcut (layer2.0 / 3.0 / 4.0 conv2) has a launch and a table of its own: MFMA_FOLD_SHAPES below
    # (bnn_hip_bconv2d_mfma_supported keeps saying no to it)
}


def mfma_conv_admitted(C: int, O: int, H: int, stride: int, fold: bool) -> bool:
    return _admitted(MFMA_CONV, (C, O, H, stride, fold), MFMA_CONV_SHAPES)


# The same for the last convolution of a down-sampling block with its shortcut folded in (csrc/bconv_mfma.hip, the DS form:
# both dots on the matrix cores, bnn_hip_bconv2d_mfma_fold_fused) instead of the popcount fold.
# BNN_AMD_MFMA_FOLD: "1" (default) — the launches listed in MFMA_FOLD_SHAPES; "0" — none: exactly the launches of before;
# "all" — every launch bnn_hip_bconv2d_mfma_fold_supported takes.  BNN_AMD_MFMA_CONV=0 turns this off too.
MFMA_FOLD = os.environ.get("BNN_AMD_MFMA_FOLD", "1")
# (C, O, H of the input, channels of the shortcut input) -> (popcount us, MFMA us) in the same kind of trace
# (profiles/mfma_fold_kernel_roofline.md).  A shape is listed only where the fold launch measured faster.
MFMA_FOLD_SHAPES = {           # (means of two traces each; both MFMA values lie below both popcount values)
    (128, 128, 28, 64): (71.0, 61.2),     # layer2.0.conv2 + shortcut
    (256, 256, 14, 128): (66.0, 50.3),    # layer3.0.conv2 + shortcut
    (512, 512, 7, 256): (71.8, 45.3),     # layer4.0.conv2 + shortcut
}


def mfma_fold_admitted(C: int, O: int, H: int, sc_C: int) -> bool:
    return _admitted(MFMA_FOLD, (C, O, H, sc_C), MFMA_FOLD_SHAPES, parents=(MFMA_CONV,))


# A launch already on the matrix cores (admitted above) on the FP4 form of the same kernel (csrc/bconv_mfma.hip, F4:
# v_mfma_f32_16x16x128_f8f6f4 with E2M1 operands — half the matrix cycles, operand bytes and k-steps, the same bits;
# bnn_hip_bconv2d_mfma4_fused / _fold_fused) instead of the int8 form.
# BNN_AMD_MFMA_F4: "1" (default) — the launches listed in MFMA_F4_SHAPES; "0" — none: exactly the launches of before;
# "all" — every matrix-core launch bnn_hip_bconv2d_mfma4_supported / _fold_supported takes (C % 128 == 0).
MFMA_F4 = os.environ.get("BNN_AMD_MFMA_F4", "1")
# The dense key (C, O, H of the input, stride, False) or the fold key (C, O, H of the input, channels of the shortcut
# input) -> (int8 MFMA us, FP4 us) in the same kind of trace (profiles/mfma_f4_kernel_roofline.md).  A shape is listed
# only where both FP4 traces lie below both int8 traces by more than the launch's trace-to-trace gap.  (Means of two
# traces each; a dense key that two launches share holds their sums.)
MFMA_F4_SHAPES = {
    (128, 128, 28, 64): (61.6, 53.1),             # layer2.0.conv2 + shortcut
    (128, 128, 28, 1, False): (86.6, 71.9),       # layer2.1.conv1 39.1 -> 31.1, layer2.1.conv2 47.4 -> 40.8
    (128, 256, 28, 2, False): (26.8, 21.4),       # layer3.0.conv1
    (256, 256, 14, 128): (48.8, 39.1),            # layer3.0.conv2 + shortcut
    (256, 256, 14, 1, False): (73.7, 52.5),       # layer3.1.conv1 34.3 -> 23.9, layer3.1.conv2 39.4 -> 28.7
    (256, 512, 14, 2, False): (24.4, 17.2),       # layer4.0.conv1
    (512, 512, 7, 256): (44.5, 32.7),             # layer4.0.conv2 + shortcut
    (512, 512, 7, 1, False): (74.1, 50.6),        # layer4.1.conv1 32.7 -> 21.3, layer4.1.conv2 41.4 -> 29.3
}


def mfma_f4_admitted(key: tuple) -> bool:
    return _admitted(MFMA_F4, tuple(key), MFMA_F4_SHAPES)    # (not MFMA_CONV: asked only for a launch the int8 form took)


# The 1x1 convolutions of the fused ResNet executor (Bottleneck and PreBottleneck: conv1, conv3 and the shortcut) on the FP4
# matrix-core kernel of csrc/bconv1x1_mfma.hip (a plain GEMM on v_mfma_f32_16x16x128_f8f6f4, every epilogue of
# bnn_hip_bconv2d_fused, the same bits; bnn_hip_bconv1x1_mfma4_fused) instead of the XNOR-popcount kernels.
# BNN_AMD_MFMA_1X1: "1" (default) — the launches listed in MFMA_1X1_SHAPES; "0" — none: exactly the launches of before;
# "all" — every launch bnn_hip_bconv1x1_mfma4_supported takes (C % 128 == 0, O % 64 == 0).  BNN_AMD_MFMA_CONV=0 turns
# this off too.  Read when an executor plans its layers.
MFMA_1X1 = os.environ.get("BNN_AMD_MFMA_1X1", "1")
# (C, O, H of the input, writes fp32) -> (popcount us, FP4 us) of that launch in kernel traces of resnet50() at batch 128,
# one batch in flight (tools/bench_conv1x1.py, profiles/conv1x1_mfma_bench.jsonl; means of two traces each, per launch
# where several share a key).  A shape is listed only where both FP4 traces lie below both popcount traces by more than
# the launch's trace-to-trace gap — the rule of MFMA_F4_SHAPES.  These are launches on NON-NEGATIVE planes (a Bottleneck
# behind ReLU: M is not read, one expansion per half-word) with an epilogue the kernel has compiled in.
MFMA_1X1_SHAPES = {
    (256, 64, 56, False): (44.2, 19.5),       # layer1.1 / 1.2 conv1
    (256, 128, 56, False): (75.4, 28.9),      # layer2.0.conv1
    (128, 512, 28, True): (104.2, 85.2),      # layer2.0 / 2.1 / 2.2 conv3
    (128, 512, 28, False): (86.5, 61.4),      # layer2.3.conv3 (planes only: layer3.0 reads nothing else)
    (512, 128, 28, False): (35.0, 17.4),      # layer2.1 / 2.2 / 2.3 conv1
    (512, 256, 28, False): (57.9, 26.1),      # layer3.0.conv1
    (512, 1024, 14, True): (39.5, 35.1),      # layer3.0 shortcut
    (256, 1024, 14, True): (61.6, 50.1),      # layer3.0 .. 3.4 conv3
    (256, 1024, 14, False): (49.7, 34.4),     # layer3.5.conv3 (planes only)
    (1024, 256, 14, False): (29.6, 14.0),     # layer3.1 .. 3.5 conv1
    (1024, 512, 14, False): (49.8, 24.5),     # layer4.0.conv1
    (1024, 2048, 7, True): (35.2, 30.9),      # layer4.0 shortcut
    (512, 2048, 7, True): (41.7, 35.3),       # layer4.0 / 4.1 / 4.2 conv3
    (2048, 512, 7, False): (32.7, 19.6),      # layer4.1 / 4.2 conv1
    # not listed: (256, 512, 28, True), the layer2.0 shortcut: 51.7 -> 59.3 us (its fp32 stores bind either way)
}
# The same for launches on TERNARY planes (both planes live: the pre-activation blocks binarise behind a BatchNorm: two
# expansions per half-word, twice the plane loads), traced in resnet50(block_type=PreBottleneck, activation=nn.PReLU); the
# epilogues are the kernel's compiled pre-activation profiles (PReLU -> next BatchNorm -> planes; PReLU -> + shortcut ->
# fp32 and planes).
MFMA_1X1_TERNARY_SHAPES = {
    (256, 64, 56, False): (50.4, 34.3),       # layer1.1 / 1.2 conv1
    (256, 128, 56, False): (89.1, 52.9),      # layer2.0.conv1
    (128, 512, 28, True): (117.8, 98.8),      # layer2.0 .. 2.3 conv3
    (512, 128, 28, False): (38.9, 27.3),      # layer2.1 / 2.2 / 2.3 conv1
    (512, 256, 28, False): (65.7, 41.9),      # layer3.0.conv1
    (256, 1024, 14, True): (72.8, 62.2),      # layer3.0 .. 3.5 conv3
    (1024, 256, 14, False): (32.6, 20.1),     # layer3.1 .. 3.5 conv1
    (1024, 512, 14, False): (51.9, 36.4),     # layer4.0.conv1
    (512, 2048, 7, True): (45.0, 40.8),       # layer4.0 / 4.1 / 4.2 conv3
    (2048, 512, 7, False): (33.4, 28.0),      # layer4.1 / 4.2 conv1
    # not listed, the three shortcuts (BN -> fp32 on the pooled ternary planes): (256, 512, 28, True) 49.8 -> 62.5 us,
    # (512, 1024, 14, True) 40.8 -> 41.1, (1024, 2048, 7, True) 37.3 -> 37.9
}


def mfma_1x1_admitted(C: int, O: int, H: int, out_f32: bool, nonneg: bool = True) -> bool:
    table = MFMA_1X1_SHAPES if nonneg else MFMA_1X1_TERNARY_SHAPES
    return _admitted(MFMA_1X1, (C, O, H, bool(out_f32)), table, parents=(MFMA_CONV,))


# The one-launch FactorizedConv kernel (csrc/fconv.hip) against the per-layer path of the same module, batch 256 on
# MI355X (tools/bench_fconv.py -> profiles/fconv_bench.jsonl).  The admission rule, in one place: a shape (C, H, W,
# stride) whose fused executor measured SLOWER than the per-layer path is listed here with its (per-layer us, fused us)
# and takes the launches the library had before (``cellops.FusedFactorizedConv.composition``: the same bits).
FCONV_DECLINED_SHAPES = {
    # none: per-layer -> fused us at batch 256 was 460 -> 104 (48, 32, 32, 1), 427 -> 91 (96, 16, 16, 1), 479 -> 91
    # (192, 8, 8, 1), 513 -> 95 (96, 32, 32, 2), 488 -> 87 (192, 16, 16, 2), 648 -> 166 (80, 28, 28, 1)
}


def fconv_admitted(C: int, H: int, W: int, stride: int) -> bool:
    return (C, H, W, stride) not in FCONV_DECLINED_SHAPES


# The 16-bit store inside the one-launch layer kernel (``hipops.bconv2d_direct(out_dtype=D)``: 2 bytes of traffic per output
# element) against the same kernel's fp32 store followed by ``hipops.round_lowp`` (10 bytes), batch 256 on MI355X
# (tools/bench_lowp.py -> profiles/lowp_bench.jsonl).  The admission rule, in one place: a shape (D, C, O, H, W, kernel,
# stride) where the 16-bit store measured SLOWER is listed here with its (fp32 store + round_lowp us, 16-bit store us) and
# takes the former: the same bits.
LOWP_STORE_DECLINED_SHAPES = {
    # none: fp32 store + round_lowp -> 16-bit store, us at batch 256, bf16 / fp16: 187.6 -> 88.4 / 185.8 -> 87.0 (64, 64, 56, 56,
    # 3, 1), 130.2 -> 78.5 / 130.4 -> 81.2 (128, 128, 28, 28, 3, 1), 112.9 -> 84.5 / 111.4 -> 82.4 (256, 256, 14, 14, 3, 1),
    # 102.1 -> 75.2 / 101.4 -> 75.8 (512, 512, 7, 7, 3, 1), 110.5 -> 60.5 / 108.3 -> 60.1 (64, 128, 56, 56, 3, 2)
}


def lowp_store_admitted(D: torch.dtype, C: int, O: int, H: int, W: int, kernel: int, stride: int) -> bool:
    return (D, C, O, H, W, kernel, stride) not in LOWP_STORE_DECLINED_SHAPES


def stats() -> dict:
    """Counters of HIP-path invocations (tests use them to prove which path ran)."""
    with _stats_lock:
        return dict(_stats)


def _bump(key: str) -> None:
    with _stats_lock:
        _stats[key] += 1


def strict_weights() -> bool:
    """``BNN_AMD_STRICT_WEIGHTS=1``: derived weight data is never cached — every forward of every binary layer re-derives
    sign bits, zero mask and alpha from the CURRENT values of ``weight`` and reads the zero-weight flag before it
    launches, exactly as the reference re-binarises on every forward (bnn/layers/conv.py:92, bnn/ops.py:129-140).
    Writes through ``.data`` need no ``invalidate()`` then, and a training step never runs on an unverified "no exact
    zero" assumption.  The price is one packing launch and one host round trip per layer and call, and ``model(x)``
    stays on the per-layer tier (the fused executors and their HIP graphs hold derived data by construction):
    README.md has the measured cost.  Read at every call, so tests can flip it."""
    return os.environ.get("BNN_AMD_STRICT_WEIGHTS", "0") == "1"


@dataclass
class Plan:
    center: bool
    compute_alpha: bool
    scale: Optional[torch.Tensor]  # BasicScaleBinarizer.alpha or None
    ste: bool = True               # the input hook's backward is the hard-tanh STE (training fast path allowed)


@dataclass
class RealPlan:
    """Plan of a layer with binary activations and a real-valued weight (``_recognise_real``)."""
    scale: Optional[torch.Tensor]  # BasicScaleBinarizer.alpha or None
    ste: bool = True               # the input hook's backward is the hard-tanh STE (training fast path allowed)


_HOOK_MODULES = ("bnn_amd.ops", "bnn_amd.bconfig", "bnn.ops", "bnn.bconfig")


def _is(obj, name: str) -> bool:
    """Exact hook class, by name, from this package or from the reference package (so that a
    model converted with the reference's own `bnn.ops` classes is accelerated as well)."""
    t = type(obj)
    return t.__name__ == name and t.__module__ in _HOOK_MODULES


def _input_hook(pre) -> Optional[bool]:
    """``True``: ``BasicInputBinarizer``; ``False``: an input hook whose VALUE is ``sign(x)`` too (inference only);
    ``None``: anything else."""
    if _is(pre, "BasicInputBinarizer"):
        return True
    # AdvancedInputBinarizer (bnn/ops.py:167-177) returns sign(f(t*x)); with the default f = tanh and t > 0
    # that IS sign(x), only its gradient differs — so inference may take the same kernels, training may not
    advanced = (_is(pre, "AdvancedInputBinarizer") and getattr(pre, "derivative_funct", None) is torch.tanh
                and isinstance(getattr(pre, "t", None), (int, float)) and pre.t > 0)
    return False if advanced else None


def _post_scale(post, out_channels: int):
    """``(recognised, scale)`` of the post hook: ``Identity``, or a per-output-channel ``BasicScaleBinarizer``."""
    if _is(post, "Identity"):
        return True, None
    if _is(post, "BasicScaleBinarizer") and post.alpha.numel() == out_channels \
            and post.alpha.dim() >= 2 and post.alpha.shape[1] == out_channels:
        return True, post.alpha
    return False, None


def _recognise(layer: nn.Module, out_channels: int) -> Optional[Plan]:
    wpre = layer.weight_pre_process
    basic = _input_hook(layer.activation_pre_process)
    if basic is None or not _is(wpre, "XNORWeightBinarizer"):
        return None
    ok, scale = _post_scale(layer.activation_post_process, out_channels)
    if not ok:
        return None
    return Plan(bool(wpre.center_weights), bool(wpre.compute_alpha), scale, ste=basic)


def _recognise_real(layer: nn.Module, out_channels: int) -> Optional[RealPlan]:
    """The hooks of a layer that binarises its activations only: the input hooks of ``_recognise``, a weight hook that is
    exactly ``torch.nn.Identity`` or this package's / the reference's ``Identity`` with no forward hooks on it (a fused
    launch would not fire them), and the post hooks of ``_recognise``.  ``_recognise`` returns ``None`` for these layers,
    so the fused executors keep declining them."""
    wpre = layer.weight_pre_process
    basic = _input_hook(layer.activation_pre_process)
    if basic is None:
        return None
    if not (type(wpre) is nn.Identity or _is(wpre, "Identity")) or wpre._forward_hooks or wpre._forward_pre_hooks:
        return None
    ok, scale = _post_scale(layer.activation_post_process, out_channels)
    if not ok:
        return None
    return RealPlan(scale, ste=basic)


_LOWP = (torch.float16, torch.bfloat16)


def lowp_dtype(layer: nn.Module, x: torch.Tensor) -> Optional[torch.dtype]:
    """The 16-bit dtype ``D`` a layer computes in on the HIP path, or ``None``: the two admission cases beyond fp32 and
    ``.half()`` (module docstring).  (1) a bf16 model: input and weight both bfloat16 — under autocast only if its dtype is
    bfloat16 too, where the casts are no-ops; (2) autocast: a float32 weight and an input of the autocast dtype, float16 or
    bfloat16.  Looks at devices and dtypes only; ``_eligible`` adds "autograd is not recording"."""
    w = layer.weight
    if not (x.is_cuda and w.is_cuda and x.device == w.device) or x.dtype not in _LOWP:
        return None
    cast = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled("cuda") else None
    if w.dtype == torch.bfloat16:
        return torch.bfloat16 if x.dtype == torch.bfloat16 and cast in (None, torch.bfloat16) else None
    if w.dtype == torch.float32:
        return x.dtype if cast == x.dtype else None
    return None


def _eligible(layer: nn.Module, x: torch.Tensor, plan: Plan) -> bool:
    w = layer.weight
    if not (x.is_cuda and w.is_cuda and x.device == w.device):
        return False
    if (x.dtype != w.dtype or x.dtype not in (torch.float32, torch.float16)) and lowp_dtype(layer, x) is None:
        return False
    if torch.is_grad_enabled():
        needs = x.requires_grad or w.requires_grad
        needs = needs or (layer.bias is not None and layer.bias.requires_grad)
        needs = needs or (plan.scale is not None and plan.scale.requires_grad)
        if needs:
            return False
    return True


def _eligible_train(layer: nn.Module, x: torch.Tensor) -> bool:
    """Autograd is recording and something on the path needs a gradient: HIP forward + library
    backward (``bnn_amd/training.py``) instead of the pure torch composition."""
    from . import training
    w = layer.weight
    return (training.ENABLED and torch.is_grad_enabled() and x.is_cuda and w.is_cuda and x.device == w.device
            and x.dtype == torch.float32 and w.dtype == torch.float32)


def _numeric_padding(layer) -> bool:
    return not isinstance(layer.padding, str) and layer.padding_mode == "zeros" and layer.groups == 1


def _grouped_numeric_padding(layer) -> bool:
    """A grouped / depthwise layer the inference path takes (``bnn_hip_bconv2d_grouped``), and — ``training.GROUPED`` —
    the training forward.  ``_numeric_padding`` keeps rejecting these: the fused executors rely on it."""
    return not isinstance(layer.padding, str) and layer.padding_mode == "zeros" and layer.groups > 1


def plan_conv2d(layer, x: torch.Tensor) -> Optional[Plan]:
    if x.dim() != 4 or not (_numeric_padding(layer) or _grouped_numeric_padding(layer)):
        return None
    plan = _recognise(layer, layer.out_channels)
    return plan if plan is not None and _eligible(layer, x, plan) else None


def plan_conv2d_train(layer, x: torch.Tensor) -> Optional[Plan]:
    """Plan for a training-mode forward (only consulted when ``plan_conv2d`` declined).  Grouped / depthwise layers
    take it under ``training.GROUPED`` (read at every call; off by default)."""
    from . import training
    if x.dim() != 4 or not (_numeric_padding(layer) or (training.GROUPED and _grouped_numeric_padding(layer))):
        return None
    plan = _recognise(layer, layer.out_channels)
    return plan if plan is not None and plan.ste and _eligible_train(layer, x) else None


def _real_applies(layer, x: torch.Tensor) -> Optional[RealPlan]:
    """What both real-weight plans ask: the switch, a dense zero-padded ``Conv2d`` with the recognised hooks, fp32 without
    autocast, a geometry of ``hipops.sconv_supported``."""
    if not REAL_WEIGHTS or x.dim() != 4 or not _numeric_padding(layer) or torch.is_autocast_enabled():
        return None
    if x.dtype != torch.float32 or layer.weight.dtype != torch.float32:
        return None
    plan = _recognise_real(layer, layer.out_channels)
    if plan is None or not hipops.sconv_supported(x.shape, layer.weight.shape, layer.stride, layer.padding, layer.dilation):
        return None
    return plan


def plan_conv2d_real(layer, x: torch.Tensor) -> Optional[RealPlan]:
    """Plan for the inference forward of a layer with binary activations and real weights (consulted when both XNOR plans
    declined; ``REAL_WEIGHTS``, read at every call)."""
    plan = _real_applies(layer, x)
    return plan if plan is not None and _eligible(layer, x, plan) else None


def plan_conv2d_real_train(layer, x: torch.Tensor) -> Optional[RealPlan]:
    """The same for a training-mode forward (only consulted when ``plan_conv2d_real`` declined): the input hook's
    backward must be the hard-tanh STE."""
    plan = _real_applies(layer, x)
    return plan if plan is not None and plan.ste and _eligible_train(layer, x) else None


def _real_linear_applies(layer, x: torch.Tensor) -> Optional[RealPlan]:
    """What both real-weight plans of a ``Linear`` ask: the switch, the recognised hooks, fp32 without autocast."""
    if not REAL_WEIGHTS or x.dim() < 1 or torch.is_autocast_enabled():
        return None
    if x.dtype != torch.float32 or layer.weight.dtype != torch.float32:
        return None
    return _recognise_real(layer, layer.out_features)


def plan_linear_real(layer, x: torch.Tensor) -> Optional[RealPlan]:
    """Plan for the inference forward of a ``Linear`` with binary activations and real weights (consulted when both XNOR
    plans declined; ``REAL_WEIGHTS``, read at every call)."""
    plan = _real_linear_applies(layer, x)
    return plan if plan is not None and _eligible(layer, x, plan) else None


def plan_linear_real_train(layer, x: torch.Tensor) -> Optional[RealPlan]:
    """The same for a training-mode forward (only consulted when ``plan_linear_real`` declined): the input hook's
    backward must be the hard-tanh STE."""
    plan = _real_linear_applies(layer, x)
    return plan if plan is not None and plan.ste and _eligible_train(layer, x) else None


def plan_conv1d(layer, x: torch.Tensor) -> Optional[Plan]:
    if x.dim() != 3 or not (_numeric_padding(layer) or _grouped_numeric_padding(layer)):
        return None
    plan = _recognise(layer, layer.out_channels)
    return plan if plan is not None and _eligible(layer, x, plan) else None


def plan_linear(layer, x: torch.Tensor) -> Optional[Plan]:
    if x.dim() < 1:
        return None
    plan = _recognise(layer, layer.out_features)
    return plan if plan is not None and _eligible(layer, x, plan) else None


def plan_linear_train(layer, x: torch.Tensor) -> Optional[Plan]:
    """Plan for a training-mode forward of a ``Linear`` (only consulted when ``plan_linear`` declined), under
    ``training.LINEAR`` (read at every call; off by default): recognised hooks with the hard-tanh STE, fp32 weight and
    input on one HIP device, autograd recording without autocast, no hooks on ``weight_pre_process`` (they would not
    fire)."""
    from . import training
    if not training.LINEAR or x.dim() < 1 or torch.is_autocast_enabled():
        return None
    plan = _recognise(layer, layer.out_features)
    if plan is None or not plan.ste or not _eligible_train(layer, x):
        return None
    return plan if training._no_hooks(layer.weight_pre_process, backward=False) else None


def packed_weight(layer, plan: Plan, sync: bool = True, fresh: bool = False) -> hipops.PackedWeight:
    """Cached ``XNORWeightBinarizer`` output for ``layer.weight`` (rebuilt when it changes).

    The cache key is the weight's storage pointer + version counter (+ recipe).  Autograd's version counter
    does NOT see writes through ``weight.data`` (``p.data.clamp_()``, ``p.data.copy_(ema)``): after such a write
    call ``invalidate(model)`` (inference) — the training forward never trusts the cache (``fresh=True``: it
    re-derives sign bits and alpha from the current values on every call, like the reference does,
    bnn/ops.py:129-140).

    ``sync=False`` (training step: the weight changed, and will change again) skips the host round trip that
    reads the zero-weight flag: the pack is made under the assumption "no weight is exactly 0" and the flag
    travels to pinned host memory asynchronously.  It is resolved by the NEXT call for this layer — a training
    call checks the previous step's flag (long since on the host), an inference call (``sync=True``) waits for
    it — and a layer that ever showed a zero is packed synchronously (mask-aware kernel) from then on.  The FIRST
    pack of a layer is always synchronous: zeros that are there from the start (pruned or zero-initialised weights, a
    loaded sparse checkpoint) take the zero-aware kernels from the first step on; what the optimistic path can still
    meet is a weight that an update lands on exactly 0.0 — one forward treats it as -1, the next call warns."""
    if strict_weights():
        sync, fresh = True, True
    master = layer.__dict__.get("_bnn_master")
    if master is not None:          # a DataParallel replica: cached on the layer it was replicated from
        return _replica_packed_weight(layer, master, plan, fresh)
    w = layer.weight
    groups = getattr(layer, "groups", 1)
    key = (w.data_ptr(), w._version, str(w.device), tuple(w.shape), plan.center, plan.compute_alpha, groups)
    cached = layer.__dict__.get("_bnn_packed")
    sync = sync or cached is None
    if cached is not None and cached[1].zero_probe is not None and (sync or fresh or cached[0] != key):
        # a pack made without reading its zero flag: resolve it before it is trusted / replaced
        pw = cached[1]
        if pw.zero_found_later():
            layer.__dict__["_bnn_zero_seen"] = True
            warnings.warn("bnn_amd: a binary weight is exactly 0 (sign(0) == 0); a forward that ran before this "
                          "was known treated it as -1.  This layer now takes the zero-aware kernels.",
                          RuntimeWarning)
            cached = None      # the unmasked pack is wrong for this weight: rebuild below
        else:
            pw.zero_probe = None
    if cached is not None and cached[0] == key and not fresh:
        return cached[1]
    sync = sync or layer.__dict__.get("_bnn_zero_seen", False)
    pw = _pack(w, plan, groups, sync)
    if pw.has_zero:  # once a layer has shown an exact zero it is always packed synchronously (mask-aware)
        layer.__dict__["_bnn_zero_seen"] = True
    layer.__dict__["_bnn_packed"] = (key, pw)
    _bump("weight_packs")
    return pw


def _pack(w: torch.Tensor, plan: Plan, groups: int, sync: bool) -> hipops.PackedWeight:
    if groups != 1:   # the windowed layout of bnn_hip_bconv2d_grouped
        return hipops.pack_weight_grouped(w, groups, plan.center, plan.compute_alpha, sync=sync)
    return hipops.pack_weight(w, plan.center, plan.compute_alpha, sync=sync)


def _replica_packed_weight(layer, master, plan: Plan, fresh: bool = False) -> hipops.PackedWeight:
    """Packed weights of a ``DataParallel`` replica.  Its ``weight`` is a broadcast copy that is new on every forward
    (new storage, version 0), so the replica's own pointer / version say nothing; the values are those of the layer it
    was replicated from.  The pack is therefore keyed on the MASTER's weight (pointer, version, recipe) and kept on the
    master per replica device: one pack — and one host round trip for the zero-weight flag — per device and weight
    version instead of one per forward."""
    mw = master.weight
    w = layer.weight
    groups = getattr(layer, "groups", 1)
    key = (mw.data_ptr(), mw._version, tuple(mw.shape), plan.center, plan.compute_alpha, groups)
    cache = master.__dict__.setdefault("_bnn_packed_replicas", {})
    dev = str(w.device)
    hit = cache.get(dev)
    if hit is not None and hit[0] == key and not fresh:
        return hit[1]
    # ``fresh`` (the training forward): never trust the cache — a ``.data`` write on the master does not move its
    # version counter, and the fused backward re-derives What from the current values (forward and backward must agree)
    pw = _pack(w, plan, groups, sync=True)
    cache[dev] = (key, pw)
    _bump("weight_packs")
    return pw


# ``module.__dict__`` keys under which a residual block, a cell operation and a cell keep the state of their own fused
# executor (dispatch.BlockFusion / OpFusion / CellFusion)
BLOCK_KEY, OP_KEY, CELL_KEY = TIER_KEYS = ("_bnn_auto_block", "_bnn_auto_op", "_bnn_auto_cell")


# ``model.__dict__`` key under which the explicit whole-network executors built for a model (batsnet.FusedBATSNetwork) are
# remembered, weakly, so that ``invalidate(model)`` reaches them
WATCH_KEY = "_bnn_watchers"


class _Watchers:
    """Weak set of the executors to mark stale; a copied or pickled model starts with none."""

    def __init__(self) -> None:
        self.refs = weakref.WeakSet()

    def __deepcopy__(self, memo) -> "_Watchers":
        return _Watchers()

    def __reduce__(self):
        return (_Watchers, ())


def watch(model: nn.Module, executor) -> None:
    """``invalidate(model)`` (or of a module that contains it) will call ``executor.mark_stale()``."""
    model.__dict__.setdefault(WATCH_KEY, _Watchers()).refs.add(executor)


def drop_executor(m: nn.Module) -> None:
    """Drop the fused executor ``m`` itself dispatches to (not those of its sub-modules): derived data goes with a
    ``train()`` <-> ``eval()`` switch."""
    for key in TIER_KEYS:
        m.__dict__.pop(key, None)


def invalidate(module: nn.Module, executors: bool = True) -> int:
    """Drop every cached packed weight under ``module`` (returns how many).  Needed after writing weights
    through ``.data`` (weight clipping ``p.data.clamp_(-1, 1)``, EMA swaps ``p.data.copy_(ema)``, hand-written
    SGD on ``.data``): those writes do not bump the Parameter's version counter, so nothing else can notice
    them.  ``FusedResNet.refresh()`` calls this for the model it wraps."""
    n = 0
    for m in module.modules():
        if m.__dict__.pop("_bnn_packed", None) is not None:
            n += 1
        n += len(m.__dict__.pop(LOWP_KEY, ()))
        if m.__dict__.pop(REAL_KEY, None) is not None:
            n += 1
        m.__dict__.pop("_bnn_packed_replicas", None)
        if executors:       # (an executor that re-derives ITSELF (refresh) passes False: it may be that very object)
            drop_executor(m)
            for ex in tuple(getattr(m.__dict__.get(WATCH_KEY), "refs", ())):
                ex.mark_stale()
    from .tails import drop_derived                 # folded BatchNorms / transposed head weights of the per-layer tails
    drop_derived(module)
    return n


# ``layer.__dict__`` key of the packs of the 16-bit cases: {(D, weight dtype): (key, pack, bias)} (``lowp_packed_weight``)
LOWP_KEY = "_bnn_packed_lowp"


def lowp_packed_weight(layer, plan: Plan, D: torch.dtype):
    """``(pack, bias)`` of a layer that computes in the 16-bit dtype ``D`` (``lowp_dtype``), cached beside the fp32 pack
    (one entry per ``D`` and case, so a layer called plainly, under autocast and plainly again keeps all its packs):

    * ``What_D = weight_pre_process(weight).to(D)``, by the layer's own hook, in torch on the device — what the reference
      hands to the convolution: under autocast the fp32 ``alpha * sign(w)`` rounded by the cast, in a 16-bit model the
      hook's own ``D`` arithmetic.  The pack holds its sign bits and zero mask (``pack_weight`` of the widened tensor
      without centring) and ``alpha[o] = max |What_D[o]|`` — exact: every non-zero entry of row ``o`` is +-alpha;
    * the bias rounded to ``D`` as autocast's cast does (a 16-bit model's already is), widened for the fp32 epilogue.

    Keyed like ``packed_weight`` (storage pointer, version, device, shape, recipe, groups) plus the bias's pointer and
    version; never trusted under ``BNN_AMD_STRICT_WEIGHTS=1``; dropped by ``invalidate()``.  A ``DataParallel`` replica
    (new storage every forward) packs on every call."""
    w, b = layer.weight, layer.bias
    groups = getattr(layer, "groups", 1)
    case = (D, w.dtype)
    key = (w.data_ptr(), w._version, str(w.device), tuple(w.shape), plan.center, plan.compute_alpha, groups,
           None if b is None else (b.data_ptr(), b._version))
    cache = layer.__dict__.setdefault(LOWP_KEY, {})
    hit = cache.get(case)
    if hit is not None and hit[0] == key and not strict_weights():
        return hit[1], hit[2]
    with torch.no_grad(), torch.autocast("cuda", enabled=False):
        what = layer.weight_pre_process(w).detach().to(D)
        wf = what.float()
        pw = hipops.pack_weight_grouped(wf, groups, center=False) if groups != 1 else hipops.pack_weight(wf, center=False)
        pw.alpha[:wf.shape[0]] = wf.abs().flatten(1).amax(1)
        bias = None if b is None else b.detach().to(D).float()
    cache[case] = (key, pw, bias)
    _bump("weight_packs")
    return pw, bias


def _f32(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """Per-channel constants of a ``.half()`` model, widened (exactly) for the fp32 epilogue."""
    return t if t is None or t.dtype == torch.float32 else t.detach().float()


def conv2d(layer, x: torch.Tensor, plan: Plan) -> torch.Tensor:
    """HIP evaluation of ``bnn.layers.Conv2d.forward`` (bnn/layers/conv.py:90-97)."""
    native.require()
    D = lowp_dtype(layer, x)
    if D is not None:
        return _conv2d_lowp(layer, x, plan, D)
    pw = packed_weight(layer, plan)
    if layer.groups != 1:   # grouped / depthwise: the sign planes, then the grouped kernel (csrc/bconv_grouped.hip)
        out = hipops.bconv2d_grouped(hipops.pack_act(x), pw, _f32(layer.bias), _f32(plan.scale), layer.stride,
                                     layer.padding, layer.dilation)
        _bump("conv2d")
        return out.to(x.dtype)
    # one launch: sign(x) is computed inside the convolution kernel (csrc/bconv_fly.hip)
    out = hipops.bconv2d_direct(x, pw, _f32(layer.bias), _f32(plan.scale), layer.stride, layer.padding,
                                layer.dilation)
    _bump("conv2d")
    return out.to(x.dtype)


def _conv2d_lowp(layer, x: torch.Tensor, plan: Plan, D: torch.dtype) -> torch.Tensor:
    """``conv2d`` of a layer that computes in the 16-bit dtype ``D``: the same launches on ``lowp_packed_weight``, the
    result rounded where the reference rounds — by the one-launch kernel's own 16-bit store where it was measured not
    slower (``lowp_store_admitted``), else and on the grouped kernel by ``hipops.round_lowp`` on the fp32 result."""
    pw, bias = lowp_packed_weight(layer, plan, D)
    scale = _f32(plan.scale)
    geometry = (layer.stride, layer.padding, layer.dilation)
    if layer.groups != 1:
        out = hipops.round_lowp(hipops.bconv2d_grouped(hipops.pack_act(x), pw, bias, None, *geometry), scale, D)
    elif (layer.kernel_size[0] == layer.kernel_size[1] and layer.stride[0] == layer.stride[1] and
          not lowp_store_admitted(D, x.shape[1], layer.out_channels, x.shape[2], x.shape[3], layer.kernel_size[0],
                                  layer.stride[0])):
        out = hipops.round_lowp(hipops.bconv2d_direct(x, pw, bias, None, *geometry), scale, D)
    else:
        out = hipops.bconv2d_direct(x, pw, bias, scale, *geometry, out_dtype=D)
    _bump("conv2d")
    return out


def conv2d_train(layer, x: torch.Tensor, plan: Plan) -> torch.Tensor:
    """Same forward under autograd (``training.conv2d_train``): HIP kernels forward, binary-aware HIP gradient kernels
    or the library's fp32 convolutions backward."""
    from . import training
    native.require()
    out = training.conv2d_train(layer, x, plan, packed_weight(layer, plan, sync=False, fresh=True))
    _bump("conv2d_train")
    return out


# ``layer.__dict__`` key of the cached weight fragments of a real-weight layer (``real_packed_weight``)
REAL_KEY = "_bnn_packed_real"


def real_packed_weight(layer) -> hipops.SconvWeight:
    """Cached ``hipops.sconv_pack_weight(layer.weight)`` (``slinear_pack_weight`` for the 2-D weight of a ``Linear``: the
    ``ksize = 1`` pack), the way ``packed_weight`` caches: keyed on the weight's storage
    pointer, version counter and a recipe tag of its own; dropped by ``invalidate()`` and by ``train()`` / ``eval()``;
    never trusted under ``BNN_AMD_STRICT_WEIGHTS=1``."""
    w = layer.weight
    key = (w.data_ptr(), w._version, str(w.device), tuple(w.shape), "sconv")
    cached = layer.__dict__.get(REAL_KEY)
    if cached is not None and cached[0] == key and not strict_weights():
        return cached[1]
    pw = hipops.slinear_pack_weight(w) if w.dim() == 2 else hipops.sconv_pack_weight(w)
    layer.__dict__[REAL_KEY] = (key, pw)
    _bump("weight_packs")
    return pw


def conv2d_real(layer, x: torch.Tensor, plan: RealPlan) -> torch.Tensor:
    """HIP evaluation of ``bnn.layers.Conv2d.forward`` for a layer with an identity weight hook: one launch, bias and
    scale in its epilogue (csrc/sconv.hip)."""
    native.require()
    out = hipops.sconv2d(x, real_packed_weight(layer), layer.bias, plan.scale, layer.stride, layer.padding)
    _bump("conv2d_real")
    return out


def conv2d_real_train(layer, x: torch.Tensor, plan: RealPlan) -> torch.Tensor:
    """Same forward under autograd (``training.sconv2d_train``); the weight is re-packed on every forward."""
    from . import training
    native.require()
    out = training.sconv2d_train(layer, x, plan)
    _bump("conv2d_real_train")
    return out


def linear_real(layer, x: torch.Tensor, plan: RealPlan) -> torch.Tensor:
    """HIP evaluation of ``bnn.layers.Linear.forward`` for a layer with an identity weight hook: one launch on the
    row-major input, bias and scale in its epilogue (csrc/slinear.hip)."""
    native.require()
    scale = None if plan.scale is None else plan.scale.reshape(-1)
    out = hipops.slinear(x, real_packed_weight(layer), layer.bias, scale)
    _bump("linear_real")
    return out


def linear_real_train(layer, x: torch.Tensor, plan: RealPlan) -> torch.Tensor:
    """Same forward under autograd (``training.slinear_train``); the weight is re-packed on every forward."""
    from . import training
    native.require()
    out = training.slinear_train(layer, x, plan)
    _bump("linear_real_train")
    return out


def conv1d(layer, x: torch.Tensor, plan: Plan) -> torch.Tensor:
    """``Conv1d`` as an ``H == 1`` 2-D convolution (bnn/layers/conv.py:36-43)."""
    native.require()
    D = lowp_dtype(layer, x)
    if D is not None:   # a 16-bit layer: the fp32 launches on its own pack, then the reference's two roundings
        pw, bias = lowp_packed_weight(layer, plan, D)
        geometry = ((1, layer.stride[0]), (0, layer.padding[0]), (1, layer.dilation[0]))
        if layer.groups != 1:
            out = hipops.bconv2d_grouped(hipops.pack_act(x.unsqueeze(2)), pw, bias, None, *geometry)
        else:
            out = hipops.bconv2d_direct(x.unsqueeze(2), pw, bias, None, *geometry)
        _bump("conv1d")
        return hipops.round_lowp(out.squeeze(2), _f32(plan.scale), D)
    pw = packed_weight(layer, plan)
    if layer.groups != 1:
        out = hipops.bconv2d_grouped(hipops.pack_act(x.unsqueeze(2)), pw, _f32(layer.bias), _f32(plan.scale),
                                     (1, layer.stride[0]), (0, layer.padding[0]), (1, layer.dilation[0]))
        _bump("conv1d")
        return out.squeeze(2).to(x.dtype)
    out = hipops.bconv2d_direct(x.unsqueeze(2), pw, _f32(layer.bias), _f32(plan.scale), (1, layer.stride[0]),
                                (0, layer.padding[0]), (1, layer.dilation[0]))
    _bump("conv1d")
    return out.squeeze(2).to(x.dtype)


def linear(layer, x: torch.Tensor, plan: Plan) -> torch.Tensor:
    """``Linear`` (bnn/layers/linear.py:22-27): the row-major XNOR GEMM kernel where it was measured not slower, else a
    1x1 convolution over 1x1 images (``hipops.linear``) — the same bits."""
    native.require()
    D = lowp_dtype(layer, x)
    if D is not None:   # a 16-bit layer: the fp32 launch on its own pack, then the reference's two roundings
        pw, bias = lowp_packed_weight(layer, plan, D)
        out = hipops.round_lowp(hipops.linear(x, pw, bias, None), _f32(plan.scale), D, channel_dim=-1)
        _bump("linear")
        return out
    pw = packed_weight(layer, plan)
    out = hipops.linear(x, pw, _f32(layer.bias), _f32(plan.scale))
    _bump("linear")
    return out.to(x.dtype)


def linear_train(layer, x: torch.Tensor, plan: Plan) -> torch.Tensor:
    """Same forward under autograd (``training.linear_train``): one HIP launch forward that keeps three bit planes of the
    input, the binary-aware HIP gradient kernels backward."""
    from . import training
    native.require()
    out = training.linear_train(layer, x, plan, packed_weight(layer, plan, sync=False, fresh=True))
    _bump("linear_train")
    return out

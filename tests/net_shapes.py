"""Whole networks at odd, non-square and small resolutions: the table, the float64 reference and the judge that
tests/test_net_shapes_cpu.py and tests/test_gpu_net_shapes.py share.  Imports without a GPU.

The kernels are pinned one by one against the CPU oracle; what chooses among them for a whole network
(``bnn_amd/executor.py``: ``_pool_into_hblock``, ``_pooled_form``, ``_hblock_ok``, ``_fold_applies``, ``_Conv.route`` and the
tables of ``fastpath``) is keyed on the stage's ``N, H, W``.  The table below walks five shallow networks through inputs
whose stages are odd, non-square, smaller than a halo and 1 x 1 (five rows), and square behind odd ones (a sixth row).

THE REFERENCE is independent of every HIP path: the model's own torch composition on the CPU in float64
(``reference``, "R64"), with the input tensor of every binary convolution kept.  R32 is the same run in float32.

THE JUDGE.  A binary network cannot be compared with a tolerance alone: one value within rounding distance of 0 in front
of a sign(), decided the other way, changes thousands of signs behind it.  So every image is walked through the binary
layers in execution order:

  1. an image whose signs in {-1, 0, +1} equal R64's at every binary layer has logits within ``LOGIT_TOL * max|R64 logits|``;
  2. at the FIRST layer where an image's signs differ from R64's, every differing element is a knife edge of the
     reference, ``|v64| <= B * max|v64|`` over that image's tensor at that layer; layers behind it are not judged;
  3. at most ``MAX_ELEMS`` elements differ at an image's first diverging layer (a wrong tap, row or tile differs in far
     more; ONE stem value that is the maximum of four overlapping 3x3/2 max-pool windows is four elements — the table has
     such an image: PreBottleneck, 210 x 224, image 1, 1.1e-7 of the maximum at ``layer1.0.downsample.1``), and at most one
     image in four of the whole table diverges at all (``MAX_DIVERGED``).

THE BOUND.  ``D`` is the largest ``|R32 - R64| / max|R64|`` over every binary-layer input of every case of the table (per
image, layers behind a diverging one left out), measured on the CPU: between 3.0e-7 and 8.6e-7 per case (30 pairs, 75
images, none of which diverges); tests/test_net_shapes_cpu.py asserts the value below as an upper bound.  ``B = 8 D``:
the HIP paths evaluate the same values in another operation order (BatchNorm folded into one fmaf, sums in tile order);
each reordering is worth a few units in the last place of the operands, like float32 against float64, and 8 leaves three
bits over that.  B stays four orders of magnitude below an ordinary value.

    D = 1.0e-6        B = 8.0e-6

THE STEM of the judged fused runs is the default one, the split-fp16 stem (``JUDGED_STEM_EXACT = False``): its differences
against float64 (its own test allows 2e-6 of the maximum) put no other than knife-edge differences into the first block
— measured on MI355X: no image of the table diverges, with this stem or with ``stem_exact_fp32=True``.  The bit-equality
checks use the default stem too.
"""
from __future__ import annotations

import copy
import functools
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

import bnn_amd as bnn
from bnn_amd.models import Bottleneck, HBlock, PreBasicBlock, PreBottleneck, ResNet, resnet18
from bnn_amd.ops import BasicInputBinarizer, BasicScaleBinarizer, XNORWeightBinarizer
from tests.golden import gen

D = 1.0e-6
B = 8 * D
JUDGED_STEM_EXACT = False
LOGIT_TOL = 1e-4            # of max|R64 logits|: the bound tests/test_gpu_c3_full.py asserts for images without a flip
MAX_ELEMS = 4               # differing elements at an image's first diverging layer
MAX_DIVERGED = 0.25         # of the images of the whole table


# ------------------------------------------------------------------------------------------------------------ the table
def _cfg(post=bnn.Identity):
    return bnn.BConfig(activation_pre_process=BasicInputBinarizer, activation_post_process=post,
                       weight_pre_process=XNORWeightBinarizer)


# family -> (constructor, configuration of the binary layers, state seed of gen.model_state)
# (PreBasicBlock with ReLU stays out: the exact integer zero of the HIP path is not reproducible by a float composition,
#  tests/test_gpu_fused.py: test_fused_preactivation_and_hierarchical_nets)
FAMILIES = {
    "basic_relu": (lambda: resnet18(num_classes=1000), _cfg, 11),
    "bottleneck_relu": (lambda: ResNet(Bottleneck, [1, 1, 1, 1], num_classes=1000), _cfg, 11),
    "prebasic_prelu": (lambda: resnet18(block_type=PreBasicBlock, activation=nn.PReLU, num_classes=1000),
                       lambda: _cfg(BasicScaleBinarizer), 4),
    "prebottleneck_prelu": (lambda: ResNet(PreBottleneck, [1, 1, 1, 1], activation=nn.PReLU, num_classes=1000), _cfg, 4),
    "hblock_relu": (lambda: ResNet(HBlock, [2, 2, 1, 1], num_classes=1000), _cfg, 4),
}

# input (N, 3, H, W) -> the stage sizes it gives and what they reach
INPUTS = [
    (2, 3, 224, 160),   # 56x40, 28x20, 14x10, 7x5: every route-table key at a foreign width; _pooled_form hit at the first
                        # stage end, decline (size) at the second; 7 x 5: channel lanes asked for (H == 7), refused by the
                        # kernel's own query (built for 7 x 7 and 14 x 14), pixel lanes taken
    (2, 3, 200, 216),   # 50x54, 25x27, 13x14, 7x7: odd stages; clipped shortcut windows at two stage ends;
                        # _pool_into_hblock and _pooled_form declining on oddness
    (3, 3, 75, 61),     # 19x16, 10x8, 5x4, 3x2: ragged tiles spanning images; odd then even
    (5, 3, 33, 47),     # 9x12, 5x6, 3x3, 2x2: images smaller than a halo; head over 4 pixels
    (1, 3, 32, 32),     # 8, 4, 2, 1: one image; a 1 x 1 last stage
    (2, 3, 210, 224),   # 53x56, 27x28, 14x14, 7x7: square late stages behind odd, non-square ones — the two sizes the
                        # channel-lane hierarchical-block kernel is built for (14 x 14: with several batches in flight)
]
STAGES = {
    (2, 3, 224, 160): [(56, 40), (28, 20), (14, 10), (7, 5)],
    (2, 3, 200, 216): [(50, 54), (25, 27), (13, 14), (7, 7)],
    (3, 3, 75, 61): [(19, 16), (10, 8), (5, 4), (3, 2)],
    (5, 3, 33, 47): [(9, 12), (5, 6), (3, 3), (2, 2)],
    (1, 3, 32, 32): [(8, 8), (4, 4), (2, 2), (1, 1)],
    (2, 3, 210, 224): [(53, 56), (27, 28), (14, 14), (7, 7)],
}
CASES = [(family, shape) for family in FAMILIES for shape in INPUTS]


def case_id(case) -> str:
    family, shape = case
    return f"{family}-{shape[0]}x{shape[2]}x{shape[3]}"


def build(family: str) -> nn.Module:
    """The network of ``family`` on the CPU in float32, eval mode: ``conv1`` and ``fc`` real, state from ``gen.model_state``."""
    make, cfg, seed = FAMILIES[family]
    net = bnn.prepare_binary_model(make(), cfg(), custom_config_layers_name={"conv1": bnn.BConfig(), "fc": bnn.BConfig()})
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict({k: torch.from_numpy(v) for k, v in gen.model_state(shapes, seed).items()})
    return net.eval()


def input_of(shape) -> torch.Tensor:
    return torch.from_numpy(gen.normal(gen.seed_of("net-shapes", *shape), tuple(shape)))


def binary_names(net: nn.Module) -> List[str]:
    return [n for n, m in net.named_modules()
            if isinstance(m, bnn.layers.Conv2d) and isinstance(m.activation_pre_process, BasicInputBinarizer)]


# -------------------------------------------------------------------------------------------------------- the reference
@dataclass
class Reference:
    names: List[str]                        # the binary convolutions in execution order
    values: Dict[str, np.ndarray]           # name -> the layer's input tensor [N, C, H, W]
    logits: np.ndarray                      # [N, classes]
    _signs: Dict[str, np.ndarray] = field(default_factory=dict, repr=False)

    def signs(self, name: str) -> np.ndarray:
        s = self._signs.get(name)
        if s is None:
            s = self._signs[name] = np.sign(self.values[name]).astype(np.int8)
        return s

    def all_signs(self) -> Dict[str, np.ndarray]:
        return {name: self.signs(name).copy() for name in self.names}


def tap_inputs(net: nn.Module, run, keep=lambda t: t.detach().cpu().numpy()):
    """``run()`` with a forward pre-hook on every binary convolution of ``net``: (its result, names in execution order,
    {name: keep(input tensor)})."""
    order, values, hooks, mods = [], {}, [], dict(net.named_modules())
    for name in binary_names(net):
        def pre(m, inp, name=name):
            assert name not in values, f"{name} ran twice"
            order.append(name)
            values[name] = keep(inp[0])
        hooks.append(mods[name].register_forward_pre_hook(pre))
    try:
        with torch.no_grad():
            y = run()
    finally:
        for h in hooks:
            h.remove()
    return y, order, values


def reference(net: nn.Module, x: torch.Tensor, dtype=torch.float64) -> Reference:
    """The model's own torch composition on the CPU in ``dtype`` (float64: R64, float32: R32)."""
    m = copy.deepcopy(net).cpu().to(dtype).eval()
    xd = x.detach().cpu().to(dtype)
    y, order, values = tap_inputs(m, lambda: m(xd))
    assert sorted(order) == sorted(binary_names(net))
    return Reference(order, values, y.numpy())


@functools.lru_cache(maxsize=None)
def cpu_net(family: str) -> nn.Module:
    return build(family)


def r64(case) -> Reference:
    family, shape = case
    return reference(cpu_net(family), input_of(shape), torch.float64)


# ------------------------------------------------------------------------------------------------- the plane unpacker
def unpack_planes(P, M, C: int, nonneg: bool = False) -> torch.Tensor:
    """Bit planes ``[N, ceil(C / 64), H, W]`` (include/bnn_hip.h: channel ``64 g + b`` is bit ``b`` of word ``g``; P set:
    +1, M set: -1) -> int8 signs ``[N, C, H, W]`` on the planes' device.  Takes int64 tensors or uint64 arrays.
    ``nonneg``: planes of a non-negative tensor, whose M plane no reader looks at."""
    def bits(plane):
        if isinstance(plane, np.ndarray):
            plane = torch.from_numpy(np.ascontiguousarray(plane).view(np.int64))
        n, g, h, w = plane.shape
        shifts = torch.arange(64, dtype=torch.int64, device=plane.device).view(1, 1, 64, 1, 1)
        out = torch.empty((n, g * 64, h, w), dtype=torch.int8, device=plane.device)
        for n0 in range(0, n, 1):           # bound the [1, g, 64, h, w] temporary
            out[n0] = ((plane[n0:n0 + 1].unsqueeze(2) >> shifts) & 1).to(torch.int8).view(g * 64, h, w)
        return out
    p = bits(P)
    assert not bool(p[:, C:].any()), "pad channels of the P plane are set"
    if nonneg:
        return p[:, :C].contiguous()
    m = bits(M)
    assert not bool(m[:, C:].any()) and not bool((p & m).any()), "pad channels of the M plane, or both planes, are set"
    return (p - m)[:, :C].contiguous()


# ------------------------------------------------------------------------------------------------------------ the judge
@dataclass
class Verdict:
    images: int
    failures: List[str] = field(default_factory=list)
    # image -> (first diverging layer, differing elements there, the largest |v64| / max|v64| among them)
    diverged: Dict[int, Tuple[str, int, float]] = field(default_factory=dict)
    logit_dev: float = 0.0                  # largest |logits - R64| / max|R64 logits| over the images without a differing sign
    value_dev: Optional[float] = None       # largest |v - v64| / max|v64| over the judged layers (where values were given)

    def report(self) -> dict:
        return {"images": self.images, "diverged": {str(k): list(v) for k, v in self.diverged.items()},
                "logit_dev": self.logit_dev, "value_dev": self.value_dev, "failures": self.failures}


def _np(a) -> np.ndarray:
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def judge(got: Dict[str, object], logits, ref: Reference, bound: float = B) -> Verdict:
    """``got``: name -> the input of that binary layer, as int8 signs or as its values (a float array: the signs are taken
    here and ``value_dev`` is measured); ``logits``: ``[N, classes]``.  Applies rules 1 to 3 (the per-image part) above;
    the caller asserts ``not verdict.failures`` and counts ``verdict.diverged`` against ``MAX_DIVERGED``."""
    logits = _np(logits).astype(np.float64)
    N = ref.logits.shape[0]
    v = Verdict(N)
    if logits.shape != ref.logits.shape:
        v.failures.append(f"logits {logits.shape} != reference {ref.logits.shape}")
        return v
    if set(got) != set(ref.names):
        v.failures.append(f"binary layers differ: {sorted(set(got) ^ set(ref.names))}")
        return v
    alive = np.ones(N, bool)                # images with no differing sign so far
    for name in ref.names:
        a, v64 = _np(got[name]), ref.values[name]
        if a.shape != v64.shape:
            v.failures.append(f"{name}: shape {a.shape} != reference {v64.shape}")
            return v
        top = np.abs(v64).reshape(N, -1).max(1)
        if a.dtype.kind == "f":
            dev = np.abs(a.astype(np.float64) - v64).reshape(N, -1).max(1) / np.maximum(top, 1e-300)
            if alive.any():
                v.value_dev = max(v.value_dev or 0.0, float(dev[alive].max()))
            a = np.sign(a).astype(np.int8)
        diff = a != ref.signs(name)
        for n in np.nonzero(alive & diff.reshape(N, -1).any(1))[0]:
            alive[n] = False
            count = int(diff[n].sum())
            worst = float(np.abs(v64[n])[diff[n]].max() / max(top[n], 1e-300))
            v.diverged[int(n)] = (name, count, worst)
            if worst > bound:
                v.failures.append(f"image {n}, {name}: a differing sign where |v64| = {worst:.3g} of the tensor's maximum "
                                  f"(knife edge: <= {bound:.3g}); {count} elements differ")
            if count > MAX_ELEMS:
                v.failures.append(f"image {n}, {name}: {count} elements differ (at most {MAX_ELEMS})")
    scale = float(np.abs(ref.logits).max())
    err = np.abs(logits - ref.logits).max(1) / scale
    if not np.isfinite(logits).all():
        v.failures.append("logits are not finite")
    if alive.any():
        v.logit_dev = float(err[alive].max())
        for n in np.nonzero(alive & ~(err <= LOGIT_TOL))[0]:
            v.failures.append(f"image {n}: no differing sign, logits off by {err[n]:.3g} of the largest (at most {LOGIT_TOL})")
    return v

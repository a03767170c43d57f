"""A whole BATS network as one executor (reference: ``bnn/models/bats.py:108-206``).

``net(x)`` runs each ``Cell`` through its own executor: every cell binarises its two inputs itself, so a tensor that feeds
two cells is read and packed twice, and the CIFAR stem writes an fp32 ``[N, 3C, H, W]`` tensor that three ``ReLUConvBN``
preprocessors only take ``sign(BatchNorm(.))`` of.  ``FusedBATSNetwork(net)`` plans the network as a whole:

* the real-valued CIFAR stem (``Conv2d(3, 3C, 3, padding=1)`` -> BatchNorm -> ReLU) is ONE launch that leaves the sign
  planes of all its ``ReLUConvBN`` consumers and, only if somebody reads it, the fp32 tensor
  (``hipops.stem3x3_bn_relu_pack``, csrc/bats_stem.hip);
* the two real-valued ImageNet stems are one launch each: ``stem0`` with its 112 x 112 intermediate in LDS
  (``hipops.stem_s2x2``), ``stem1`` with the sign planes of its ``ReLUConvBN`` consumers (``hipops.gconv3x3s2_bn_pack``;
  csrc/bats_stem_in.hip); ``FUSE_IMAGENET_STEMS = False`` keeps them as modules;
* every other tensor between cells is packed once, for all the ``ReLUConvBN`` that read it (``bn_act_pack_multi``), and
  the planes are handed to the cells (``FusedCell.forward(s0, s1, planes=...)``);
* global pooling + a real-valued classifier is the head kernel (``hipops.avgpool_fc``);
* ``capture`` records one forward into a HIP graph on one stream, ``replay`` runs it.

It is an explicit entry point: ``net(x)`` keeps dispatching cell by cell.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch
import torch.nn as nn

from . import fastpath, hipops, native
from .cellops import MAX_PACK_SETS, FusedCell, _Executor
from .executor import FusionError, _is_float_layer, _is_float_layer_linear, fold_bn, param_signature

NETWORKS = {"BATSNetworkCIFAR": ("stem",), "BATSNetworkImageNet": ("stem0", "stem1")}
# kernel launches (native.launch_count()) per step kind; the other kinds are torch calls, or modules that dispatch
# themselves.  The head is two streaming launches through a workspace (bnn_hip_avgpool_fc_ws_f32).
LAUNCHES = {"stem3x3": 1, "stem_s2x2": 1, "stem_s2_pack": 1, "pack_handoff": 1, "pack": 1, "pack_s2": 1, "pack_multi": 1, "dense": 1, "grouped_node": 1,
            "avgpool_fc": 2}
# the fused plan of the real-valued ImageNet stems (read at refresh()); False: stem0 / stem1 run as modules
FUSE_IMAGENET_STEMS = True
# widest classifier input the two-launch head covers: 64 bytes of LDS per feature (csrc/tail.hip: avgpool_fc_ws_supported)
_HEAD_MAX_FEATURES = (160 * 1024 - 1024) // 64


def _pair(v) -> Tuple[int, int]:
    return (v, v) if isinstance(v, int) else tuple(v)


class FusedBATSNetwork(_Executor):
    """Inference executor of a ``BATSNetworkCIFAR`` / ``BATSNetworkImageNet``: ``FusedBATSNetwork(net)(x)`` returns
    ``(logits, None)`` like ``net(x)`` under ``eval()``.

    Recognition is by class name plus structure (``stem`` or ``stem0`` / ``stem1``, ``cells``, ``global_pooling``,
    ``classifier``; the cells as ``FusedCell`` recognises them), so a network of the reference's own classes works when
    handed over.  Training mode, ``use_shake_shake``, a real-valued 3x3 stem convolution with a bias and anything
    unrecognised raise ``FusionError``.

    ``steps`` lists the plan as ``(kind, detail)``: ``stem3x3`` (``sets`` plane sets, ``y``: whether the fp32 tensor is
    written), ``stem_s2x2`` + ``stem_s2_pack`` (the ImageNet stems; ``sets`` / ``y`` / ``consumers`` of ``stem1``) or ``module`` (a stem, pooling or classifier that runs by calling the module and so takes whatever path its
    layers dispatch to); ``pack_handoff`` (one ``bn_act_pack_multi`` of a stem or cell output ``of`` for its ``sets``
    ``ReLUConvBN`` ``consumers``, given as ``(cell, input)``); the steps of every cell with ``cell`` in the detail (without
    the ``pack`` of a preprocessor whose planes are handed over); ``avgpool_fc``.  ``LAUNCHES`` maps the kinds
    that launch kernels of the library to how many.

    Derived data is keyed on the identity, storage and version of every parameter and buffer of the network; writes
    through ``.data`` need ``refresh()`` or ``fastpath.invalidate(net)``.  ``capture(x)`` records a HIP graph of one
    forward, ``replay()`` runs it on the contents of ``input``; a refresh re-captures."""
    takes = "BATS network: the input must be a float32 NCHW tensor"
    _graph = None
    _gx: Optional[torch.Tensor] = None
    _gy: Optional[torch.Tensor] = None

    def __init__(self, model: nn.Module) -> None:
        super().__init__(model)
        fastpath.watch(model, self)

    def mark_stale(self) -> None:
        """The next call re-derives everything (``fastpath.invalidate`` calls this)."""
        self._sig = None

    # ---- recognition and planning ---------------------------------------------------------------------------------
    def _stem3x3(self, stem: nn.Module, n_sets: int):
        """``(conv, bn)`` when the stem is what ``stem3x3_bn_relu_pack`` computes, else None (it runs as a module)."""
        if not (isinstance(stem, nn.Sequential) and len(stem) == 3 and isinstance(stem[0], nn.Conv2d)
                and type(stem[1]) is nn.BatchNorm2d and type(stem[2]) is nn.ReLU):
            return None
        conv, bn = stem[0], stem[1]
        if not (_is_float_layer(conv) and conv.in_channels == 3 and tuple(conv.kernel_size) == (3, 3)
                and tuple(conv.stride) == (1, 1) and tuple(conv.padding) == (1, 1) and tuple(conv.dilation) == (1, 1)
                and conv.groups == 1 and conv.padding_mode == "zeros" and conv.weight.dtype == torch.float32):
            return None
        if conv.bias is not None:
            raise FusionError("BATS network: the real-valued 3x3 stem convolution has a bias, which the stem kernel does "
                              "not add")
        if (bn.running_mean is None or bn.running_var is None or bn.running_var.dtype != torch.float32
                or bn.num_features != conv.out_channels or not 1 <= n_sets <= MAX_PACK_SETS):
            return None
        return conv, bn

    def _stems_s2(self, stem0: nn.Module, stem1: nn.Module):
        """``(conv0, bn0, conv1, bn1, conv2, bn2, inplace)`` when the ImageNet stems are what ``stem_s2x2`` and
        ``gconv3x3s2_bn_pack`` compute (``inplace``: the ReLU at the head of ``stem1`` rewrites ``stem0``'s output), else
        None: they run as modules."""
        kinds0, kinds1 = (nn.Conv2d, nn.BatchNorm2d, nn.ReLU, nn.Conv2d, nn.BatchNorm2d), (nn.ReLU, nn.Conv2d, nn.BatchNorm2d)
        if not (FUSE_IMAGENET_STEMS and isinstance(stem0, nn.Sequential) and isinstance(stem1, nn.Sequential)
                and len(stem0) == len(kinds0) and len(stem1) == len(kinds1)):
            return None
        for mod, kind in list(zip(stem0, kinds0)) + list(zip(stem1, kinds1)):
            if not (isinstance(mod, kind) if kind is nn.Conv2d else type(mod) is kind):
                return None
        conv0, bn0, _, conv1, bn1 = stem0
        relu, conv2, bn2 = stem1
        for conv, bn in ((conv0, bn0), (conv1, bn1), (conv2, bn2)):
            if not (_is_float_layer(conv) and tuple(conv.kernel_size) == (3, 3) and tuple(conv.stride) == (2, 2)
                    and tuple(conv.padding) == (1, 1) and tuple(conv.dilation) == (1, 1) and conv.padding_mode == "zeros"
                    and conv.weight.dtype == torch.float32 and conv.bias is None):
                return None
            if (bn.running_mean is None or bn.running_var is None or bn.running_var.dtype != torch.float32
                    or bn.num_features != conv.out_channels):
                return None
        if not (conv0.in_channels == 3 and conv0.groups == 1 and conv1.in_channels == conv0.out_channels
                and conv2.in_channels == conv1.out_channels):
            return None
        # what the kernels cover (BNN_HIP_ERR_UNSUPPORTED otherwise): a group's input channels in LDS, groups / words in grid.y
        if (conv1.in_channels // conv1.groups > native.STEM_S2X2_MAX_GROUP_CHANNELS or conv1.groups > 65535
                or conv2.in_channels // conv2.groups > native.GCONV3X3S2_MAX_GROUP_CHANNELS
                or (conv2.out_channels + 63) // 64 > 65535):
            return None
        return conv0, bn0, conv1, bn1, conv2, bn2, bool(relu.inplace)

    def _head(self, pool: nn.Module, fc: nn.Module):
        """The pooling window the head kernel needs (None: any map, an int k: a k x k map), or False: modules."""
        if not (isinstance(fc, nn.Linear) and _is_float_layer_linear(fc) and fc.weight.dtype == torch.float32
                and fc.in_features <= _HEAD_MAX_FEATURES):
            return False
        if type(pool) is nn.AdaptiveAvgPool2d and pool.output_size in (1, (1, 1)):
            return None
        if type(pool) is nn.AvgPool2d:
            k = _pair(pool.kernel_size)
            if (k[0] == k[1] and _pair(pool.stride if pool.stride is not None else k) == k and _pair(pool.padding) == (0, 0)
                    and pool.divisor_override is None):
                return k[0]
        return False

    def refresh(self) -> None:
        """Re-derive everything from the network's current parameters and buffers (and re-capture a captured graph)."""
        recapture, self._graph, self._gy = self._graph is not None, None, None
        self._sig = None
        m = self.model
        stems = NETWORKS.get(type(m).__name__)
        if stems is None:
            raise FusionError(f"{type(m).__name__} is not a BATS network ({', '.join(NETWORKS)})")
        cells = getattr(m, "cells", None)
        if not (isinstance(cells, nn.ModuleList) and len(cells) > 0 and all(isinstance(getattr(m, s, None), nn.Module)
                                                                          for s in stems + ("global_pooling", "classifier"))):
            raise FusionError(f"{type(m).__name__} has no {' / '.join(stems)} / cells / global_pooling / classifier")
        if m.training:
            raise FusionError("FusedBATSNetwork is inference-only: call .eval() first")
        self._cells: List[FusedCell] = [FusedCell(c) for c in cells]        # (use_shake_shake is refused there)
        L = len(cells)
        # the tensors between the parts: ids 0 .. len(stems) - 1 are the stems' outputs, then one per cell; cell k reads
        # tensor reads[k] as s0 and reads[k + 1] as s1 (the CIFAR stem feeds both inputs of cell 0)
        S = len(stems)
        reads = ([0, 0] if S == 1 else [0, 1]) + [S + k for k in range(L)]
        names = list(stems) + list(range(L))
        users = {j: [] for j in range(S + L)}
        for k in range(L):
            for i in (0, 1):
                users[reads[k + i]].append((k, i))
        last_use = {j: max((k for k, _ in u), default=-1) for j, u in users.items()}
        plan = []

        def add(kind, detail, run):
            plan.append((kind, detail, run))

        def handoff(j):
            """(the ReLUConvBN consumers of tensor j, their stacked affines, whether anybody reads its fp32 values)"""
            pres = [(k, i, self._cells[k].preprocessor(i)) for k, i in users[j]]
            rcb = [(k, i) for k, i, p in pres if p.kind == "ReLUConvBN"]
            f32 = j == S + L - 1 or any(p.kind != "ReLUConvBN" or p.add_skip for _, _, p in pres)
            a = torch.stack([p.bn_a for _, _, p in pres if p.kind == "ReLUConvBN"]) if rcb else None
            b = torch.stack([p.bn_b for _, _, p in pres if p.kind == "ReLUConvBN"]) if rcb else None
            return rcb, a, b, f32

        def plan_pack(j):
            rcb, a, b, _ = handoff(j)
            for c0 in range(0, len(rcb), MAX_PACK_SETS):
                ch = rcb[c0:c0 + MAX_PACK_SETS]
                add("pack_handoff", {"of": names[j], "sets": len(ch), "consumers": list(ch)},
                    lambda env, j=j, ch=ch, a=a[c0:c0 + MAX_PACK_SETS], b=b[c0:c0 + MAX_PACK_SETS]: env["planes"].update(
                        zip(ch, hipops.bn_act_pack_multi(env["t"][j], a, b, relu=False))))

        # -- the stems
        rcb, a, b, f32 = handoff(0)
        fused_stem = self._stem3x3(getattr(m, stems[0]), len(rcb)) if S == 1 else None
        fused_s2 = self._stems_s2(m.stem0, m.stem1) if stems == NETWORKS["BATSNetworkImageNet"] else None
        if fused_s2 is not None:
            conv0, bn0, conv1, bn1, conv2, bn2, inplace = fused_s2
            (s1, t1), (s2, t2), (s3, t3) = fold_bn(bn0), fold_bn(bn1), fold_bn(bn2)

            # stem1's in-place ReLU rewrites s0 before any cell reads it: the cells then see relu(s0), written directly
            def run_stem0(env, s1=s1, t1=t1, s2=s2, t2=t2):
                env["t"][0] = hipops.stem_s2x2(env["x"], conv0.weight, s1, t1, conv1.weight, s2, t2, conv1.groups,
                                               relu_out=inplace)
            add("stem_s2x2", {"relu_out": inplace}, run_stem0)
            rcb, a, b, f32 = handoff(1)
            packs = 1 <= len(rcb) <= MAX_PACK_SETS       # (more consumers: fp32 only, plan_pack binarises)
            f32 = f32 or not packs

            def run_stem1(env, s3=s3, t3=t3, a=a if packs else None, b=b if packs else None, rcb=rcb, f32=f32):
                y, sets = hipops.gconv3x3s2_bn_pack(env["t"][0], conv2.weight, s3, t3, conv2.groups, a, b,
                                                    relu_in=not inplace, out_f32=f32)
                env["t"][1] = y
                env["planes"].update(zip(rcb, sets))
            add("stem_s2_pack", {"sets": len(rcb) if packs else 0, "y": f32, "consumers": list(rcb) if packs else []},
                run_stem1)
            plan_pack(0)
            if not packs:
                plan_pack(1)
        elif fused_stem is not None:
            conv, bn = fused_stem
            s, t = fold_bn(bn)

            def run_stem(env, conv=conv, s=s, t=t, a=a, b=b, rcb=rcb, f32=f32):
                y, sets = hipops.stem3x3_bn_relu_pack(env["x"], conv.weight, s, t, a, b, out_f32=f32)
                env["t"][0] = y
                env["planes"].update(zip(rcb, sets))
            add("stem3x3", {"sets": len(rcb), "y": f32, "consumers": list(rcb)}, run_stem)
        else:
            for j, name in enumerate(stems):
                add("module", {"name": name}, lambda env, j=j, mod=getattr(m, name): env["t"].__setitem__(
                    j, mod(env["x"] if j == 0 else env["t"][j - 1])))
            for j in range(S):                  # (after both: the ImageNet stem1 starts with an in-place ReLU of stem0's output)
                plan_pack(j)
        # -- the cells
        for k, eng in enumerate(self._cells):
            given = [kind == "ReLUConvBN" for kind in (eng.preprocessor(0).kind, eng.preprocessor(1).kind)]
            for kind, detail in eng.steps:
                if kind == "pack" and detail["op"] in [f"preprocess{i}" for i in (0, 1) if given[i]]:
                    continue
                plan.append((kind, dict(detail, cell=k), None))

            def run_cell(env, k=k, eng=eng, j0=reads[k], j1=reads[k + 1], out=S + k):
                env["t"][out] = eng(env["t"][j0], env["t"][j1],
                                    planes=(env["planes"].pop((k, 0), None), env["planes"].pop((k, 1), None)))
                for j in {j0, j1}:
                    if last_use[j] == k:
                        env["t"][j] = None
            add("cell", None, run_cell)
            if k < L - 1:
                plan_pack(S + k)
        # -- the head
        pool, fc = m.global_pooling, m.classifier
        window = self._head(pool, fc)
        last = S + L - 1
        if window is False:
            add("module", {"name": "global_pooling"}, lambda env: env["t"].__setitem__(last, pool(env["t"][last])))
            add("module", {"name": "classifier"},
                lambda env: env.__setitem__("out", fc(env["t"][last].view(env["t"][last].size(0), -1))))
        else:
            w_t = fc.weight.detach().t().contiguous() if fc.weight.is_cuda else None
            bias = None if fc.bias is None else fc.bias.detach()

            def run_head(env, window=window, w_t=w_t, bias=bias):
                y = env["t"][last]
                if window is not None and tuple(y.shape[2:]) != (window, window):
                    raise FusionError(f"BATS network: AvgPool2d({window}) in front of the classifier meets a "
                                      f"{y.shape[2]}x{y.shape[3]} map")
                env["out"] = hipops.avgpool_fc(y, w_t, bias)
            add("avgpool_fc", {"window": "global" if window is None else window}, run_head)
        self._plan = plan
        self._sig = param_signature(self.model)
        if recapture:
            self.capture(self._gx)

    @property
    def cell_executors(self) -> List[FusedCell]:
        """The ``FusedCell`` of every cell, in order (re-made by every refresh)."""
        return list(self._cells)

    @property
    def steps(self):
        """The planned steps as ``(kind, detail)``, in execution order."""
        return [(kind, dict(detail)) for kind, detail, _ in self._plan if detail is not None]

    # ---- forward --------------------------------------------------------------------------------------------------
    def _forward_impl(self, x: torch.Tensor) -> torch.Tensor:
        if next(self.model.parameters()).device != x.device:
            raise FusionError("BATS network: module and input live on different devices")
        native.require()
        env = {"x": x, "t": {}, "planes": {}, "out": None}
        for _, _, run in self._plan:
            if run is not None:
                run(env)
        return env["out"]

    @torch.no_grad()
    def forward(self, x: torch.Tensor):
        self._check_inputs(x)
        if not self._unchanged():
            self.refresh()
        return self._forward_impl(x), None

    # ---- HIP graph ------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def capture(self, example: torch.Tensor) -> "FusedBATSNetwork":
        """Record one forward for inputs shaped like ``example`` into a HIP graph: one warm-up forward (every weight is
        packed, no host round trip is left), then the capture, all on the current stream.  ``input`` is the graph's
        input buffer (it starts as a copy of ``example``), ``replay()`` runs the graph."""
        self._check_inputs(example)
        self._graph = None                    # (a refresh below must not re-capture by itself)
        if not self._unchanged():
            self.refresh()
        if self._gx is None or self._gx.shape != example.shape or self._gx.device != example.device:
            self._gx = torch.empty_like(example, memory_format=torch.contiguous_format)
        if self._gx.data_ptr() != example.data_ptr():
            self._gx.copy_(example)
        with torch.cuda.device(example.device):
            self._forward_impl(self._gx)
            torch.cuda.current_stream().synchronize()
            g = torch.cuda.CUDAGraph()
            # thread_local: HIP calls of other threads (data-loader pinning, a process group's watchdog) must not
            # invalidate the capture
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                self._gy = self._forward_impl(self._gx)
        self._graph = g
        return self

    @property
    def input(self) -> Optional[torch.Tensor]:
        """The captured graph's input buffer: fill it in place, then ``replay()``.  None before ``capture``."""
        return self._gx if self._graph is not None else None

    def replay(self) -> torch.Tensor:
        """Run the captured graph on the contents of ``input``; returns the graph's logits buffer (overwritten by the
        next replay).  A parameter change since the capture refreshes and re-captures first."""
        if self._graph is None:
            raise FusionError("FusedBATSNetwork.replay() needs capture(x) first")
        if not self._unchanged():
            self.refresh()
        self._graph.replay()
        return self._gy

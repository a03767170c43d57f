"""Tensor-level wrappers over the C-ABI (``include/bnn_hip.h``).

torch is used here for what the tier calls plumbing: device memory (caching allocator), the
current HIP stream and device guards.  All arithmetic happens inside ``libbnn_hip.so``.

Conventions (the C-ABI sees pointers, never strides, so every tensor passes one checker before its ``data_ptr()``):

* an fp32 NCHW activation: ``_nchw`` (device, fp32 — or fp16 / bf16 with ``lowp`` —, rank 4, made contiguous);
* per-channel constants: ``_per_channel`` (``[K, n]`` tables: ``_affine_table``); a read-only tensor of a known shape
  (``residual``, ``addend``, gradients, saved statistics): ``_shaped``; both make a strided view contiguous;
* a tensor the kernel writes in place (running statistics, ``out=``, ``gx`` of ``ste_mask_``): ``_written``, which
  rejects a strided view — a copy would swallow the update;
* an opaque buffer of a size the library states (``w8``, ``SconvWeight.data``, gradient weight packs): ``_opaque``;
* channel slices of a wider tensor, read or written in place: ``channel_view``.

A batch or row range larger than one launch addresses is cut by ``_split`` (descriptors: ``_desc_slices``).  Each wrapper
computes its own step from the limit of its kernels — ``_MAX_ELEMS`` / ``_MAX_INDEX_FACTOR`` (``_batch_step``),
``_MAX_DESC_BYTES``, ``_STEM3X3_MAX_ELEMS``, ``_STEM_S2_MAX_ELEMS``, ``_LINEAR_MAX_ELEMS``: module globals, read at call
time — and only the cutting is shared.  A new wrapper: check every operand with one of the above, compute the step,
allocate under ``torch.cuda.device``, loop over ``_split`` and hand each status to ``native.check``.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import native

_MAX_ELEMS = (1 << 30) - 1  # fp32 elements one conv launch addresses (32-bit byte offsets inside the kernels)
# the tiled conv kernels multiply indices with 24-bit multiplies (csrc/bconv.hip: small_indices()); a launch whose
# images x channels factor reaches 2^23 would silently take the slow shape-generic kernel — split the batch first
_MAX_INDEX_FACTOR = (1 << 23) - 1
_DIRECT_MIN_PIXELS = 16           # images up to this many pixels may take pack_act + bconv2d (_prefers_two_launches)
_MAX_DESC_BYTES = 0xFFFFFE00      # tensors addressed through a sized 32-bit buffer descriptor (capi.hip: kMaxDescBytes)


def _batch_step(n: int, per_img_elems: int, chan_factor: int) -> int:
    """Images per launch: as many as keep every tensor of the launch below ``_MAX_ELEMS`` elements and
    ``images * chan_factor`` (channels of the widest fp32 tensor, 64-channel groups of the planes) below the
    tiled kernels' index range."""
    step = min(n, _MAX_ELEMS // max(per_img_elems, 1), _MAX_INDEX_FACTOR // max(chan_factor, 1))
    return max(1, step)


def _launch_images(n: int, C: int, O: int, c_total: int, in_elems: int, out_pixels: int) -> int:
    """Images one convolution launch covers (``_batch_step``): the fp32 output holds ``c_total`` channels, the input
    ``in_elems`` fp32-sized elements per image (sign planes count twice: they are limited to 2^29 uint64 words per
    launch, half the fp32 element budget: capi.hip check_desc), the output planes ``O`` channels."""
    per_img = max(c_total * out_pixels, in_elems, 2 * out_pixels * ((O + 63) // 64))
    return _batch_step(n, per_img, max(c_total, O, (C + 63) // 64))


def _stem_launch_images(n: int, H: int, W: int, ho: int, wo: int) -> int:
    """Images one stem launch covers: the kernels address x ``[n, 3, H, W]`` and the output ``[n, 64, ho, wo]`` through
    32-bit buffer descriptors, so each stays below 2^32 - 512 bytes (include/bnn_hip.h)."""
    return max(1, min(n, _MAX_DESC_BYTES // max(12 * H * W, 256 * ho * wo)))


def _split(n: int, step: int):
    """``(n0, n1)`` for each launch of ``n`` images (or rows) cut into runs of ``step``; nothing for ``n == 0``."""
    for n0 in range(0, n, step):
        yield n0, min(n, n0 + step)


def _desc_slices(d, step: int):
    """``(n0, n1, descriptor of images [n0, n1))`` for each launch of the descriptor's batch cut into ``step`` images
    (``d``: any descriptor structure with an ``N`` field; it is left as it is)."""
    for n0, n1 in _split(d.N, step):
        dd = type(d).from_buffer_copy(d)
        dd.N = n1 - n0
        yield n0, n1, dd


def _half_hw(H: int, W: int) -> Tuple[int, int]:
    """Output extents of the stem's stride-2 stages: conv 7x7 / 2 / 3 and MaxPool 3x3 / 2 / 1 alike."""
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def _pair(v) -> Tuple[int, int]:
    if isinstance(v, int):
        return v, v
    if len(v) == 1:
        return int(v[0]), int(v[0])
    return int(v[0]), int(v[1])


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _stream(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _on_device(t: torch.Tensor, what: str, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    if not t.is_cuda:
        raise native.NativeError(f"bnn_amd: {what} must live on a HIP device, got {t.device}")
    if t.dtype != dtype:
        raise native.NativeError(f"bnn_amd: {what} must be {str(dtype)[6:]}, got {t.dtype}")
    return t


def _require_cuda_f32(t: torch.Tensor, what: str) -> torch.Tensor:
    return _on_device(t, what).contiguous()


def _shaped(t: Optional[torch.Tensor], shape, what: str, mismatch: Optional[str] = None,
            dtype: torch.dtype = torch.float32) -> Optional[torch.Tensor]:
    """A tensor the kernel only reads (None stays None): on the device, of ``dtype`` and ``shape``, made contiguous (the
    same object when it is already).  ``mismatch``: the text of the shape error (``{got}``: the shape that came)."""
    if t is None:
        return None
    _on_device(t, what, dtype)
    if tuple(t.shape) != tuple(shape):
        raise native.NativeError("bnn_amd: " + (mismatch or "{what} shape {got} != {want}").format(
            what=what, got=tuple(t.shape), want=tuple(shape)))
    return t.contiguous()


def _written(t: Optional[torch.Tensor], shape, what: str, error: Optional[str] = None) -> Optional[torch.Tensor]:
    """A tensor the kernel writes in place (None stays None): on the device, fp32, of ``shape`` (an int: that many
    elements in any shape) and contiguous.  A strided view is refused, never copied: the copy would take the update.
    ``error``: the text of wrappers that had one of their own."""
    if t is None:
        return None
    fits = t.numel() == shape if isinstance(shape, int) else tuple(t.shape) == tuple(shape)
    if not (t.is_cuda and t.dtype == torch.float32 and fits and t.is_contiguous()):
        raise native.NativeError("bnn_amd: " + (error or (
            f"{what} is written in place: it must be a contiguous fp32 HIP tensor of {shape} "
            f"{'entries' if isinstance(shape, int) else '(its shape)'}, got {tuple(t.shape)} {t.dtype} on {t.device}, "
            f"strides {t.stride()}")))
    return t


def _opaque(t: torch.Tensor, nbytes: int, what: str, dtype: torch.dtype) -> torch.Tensor:
    """A buffer whose layout only the library knows: on the device, ``dtype``, contiguous and exactly the ``nbytes`` the
    library's own ``*_bytes`` function states for it (0: it has no such buffer for this geometry, and the entry point
    refuses the call before reading any)."""
    _on_device(t, what, dtype)
    if not t.is_contiguous() or (nbytes and t.numel() * t.element_size() != int(nbytes)):
        raise native.NativeError(f"bnn_amd: {what} must be a contiguous buffer of {int(nbytes)} bytes, got "
                                 f"{t.numel() * t.element_size()} (strides {t.stride()})")
    return t


# The 16-bit formats the kernels read (C-ABI input type) and the one-launch layer stores (descriptor flag)
_LOWP_DTYPE = {torch.float16: native.DTYPE_F16, torch.bfloat16: native.DTYPE_BF16}
_LOWP_OUT_FLAG = {torch.float16: native.FLAG_OUT_F16, torch.bfloat16: native.FLAG_OUT_BF16}


def _act_dtype(x: torch.Tensor) -> int:
    """``BNN_HIP_DTYPE_*`` of an activation that passed ``_require_cuda_act``."""
    return _LOWP_DTYPE.get(x.dtype, native.DTYPE_F32)


def _check_out_dtype(out_dtype) -> None:
    if out_dtype is not None and out_dtype not in _LOWP_OUT_FLAG:
        raise ValueError("out_dtype must be None, torch.float16 or torch.bfloat16")


def round_lowp(out: torch.Tensor, post_scale: Optional[torch.Tensor], dtype: torch.dtype,
               channel_dim: int = 1) -> torch.Tensor:
    """The two rounding points of the reference layer on a 16-bit tensor, applied with torch to the fp32 result ``out`` of
    a launch that ran WITHOUT its post-scale: ``r = out.to(dtype)`` (round to nearest even, fp16 overflow -> +-inf), then
    — ``BasicScaleBinarizer``'s in-place ``x.mul_(alpha)`` — ``r = dtype(float(r) * post_scale[o])``, channels on
    dimension ``channel_dim``.  What the in-kernel store of ``bconv2d_direct(out_dtype=...)`` computes, for the routes
    that have no such store."""
    _check_out_dtype(dtype)
    r = out.to(dtype)
    if post_scale is not None:
        shape = [1] * r.dim()
        shape[channel_dim] = -1
        r.mul_(post_scale.detach().float().reshape(shape))
    return r


def _require_cuda_act(x: torch.Tensor) -> torch.Tensor:
    """An activation the packing kernels read: fp16 / bf16 stay as they are, everything else must be fp32, on a HIP
    device."""
    if x.dtype not in _LOWP_DTYPE:
        return _require_cuda_f32(x, "activation")
    if not x.is_cuda:
        raise native.NativeError(f"bnn_amd: activation must live on a HIP device, got {x.device}")
    return x.contiguous()


def _nchw(x: torch.Tensor, what: str, fn: str, lowp: bool = False) -> torch.Tensor:
    """An NCHW activation of the wrapper ``fn``: on the device, fp32 (``lowp``: or fp16 / bf16), rank 4, made contiguous."""
    x = _require_cuda_act(x) if lowp else _require_cuda_f32(x, what)
    if x.dim() != 4:
        raise native.NativeError(f"bnn_amd: {fn} expects NCHW, got shape {tuple(x.shape)}")
    return x


def _shuffle_groups(v, channels: int, noun: str) -> int:
    """``channel_shuffle``'s group count as an int that divides the ``channels`` (``noun``: what the error calls them)."""
    v = int(v)
    if v < 1 or channels % v:
        raise native.NativeError(f"bnn_amd: shuffle_groups={v} does not divide the {channels} {noun}")
    return v


def _per_channel(t: Optional[torch.Tensor], n: int, what: str) -> Optional[torch.Tensor]:
    if t is None:
        return None
    t = _require_cuda_f32(t.detach(), what).reshape(-1)
    if t.numel() != n:
        raise native.NativeError(f"bnn_amd: {what} must have one entry per output channel ({n})")
    return t


@dataclass
class PackedAct:
    """sign(x) as bit planes: ``P``/``M`` int64 ``[N,cw64,H,W]`` (format: include/bnn_hip.h)."""
    P: torch.Tensor
    M: torch.Tensor
    shape: Tuple[int, int, int, int]  # logical (N, C, H, W)
    # True when the producer guarantees M == 0 everywhere (values out of a ReLU are {0,+1}): the
    # 3x3 kernels then keep only the P plane in registers (BNN_HIP_FLAG_ACT_NONNEG).
    nonneg: bool = False

    def batch_slice(self, n0: int, n1: int) -> "PackedAct":
        return PackedAct(self.P[n0:n1], self.M[n0:n1], (n1 - n0,) + tuple(self.shape[1:]), self.nonneg)


@dataclass
class PackedWeight:
    """sign(W) in the kernel-facing layout + per-channel alpha (padded to ``o_pad``)."""
    wbits: torch.Tensor   # int32 [n_words]
    wnz: torch.Tensor     # int32 [n_words]
    alpha: torch.Tensor   # float32 [o_pad]
    has_zero: bool
    shape: Tuple[int, int, int, int]  # logical (O, C, KH, KW)
    # deferred zero check (pack_weight(..., sync=False)): pinned host copy of the flag + the event after it
    zero_probe: Optional[tuple] = None
    # pack_weight_grouped: shape = (O, C / groups, KH, KW) in the windowed block-diagonal layout (include/bnn_hip.h),
    # read only by bconv2d_grouped (windowed = True also for groups == 1 from that packer)
    groups: int = 1
    windowed: bool = False

    def zero_found_later(self) -> bool:
        """True if a pack made with ``sync=False`` turned out to contain a zero weight (waits for the copy)."""
        if self.zero_probe is None:
            return False
        host, ev = self.zero_probe
        ev.synchronize()
        return bool(host.item())


def empty_packed(N: int, C: int, H: int, W: int, device) -> PackedAct:
    cw64 = (C + 63) // 64
    return PackedAct(torch.empty((N, cw64, H, W), dtype=torch.int64, device=device),
                     torch.empty((N, cw64, H, W), dtype=torch.int64, device=device), (N, C, H, W))


def pack_act(x: torch.Tensor) -> PackedAct:
    """``BasicInputBinarizer`` on device: fp32 (or fp16 / bf16) NCHW -> bit planes (bnn/ops.py:151-152)."""
    x = _nchw(x, "activation", "pack_act", lowp=True)
    lib = native.require()
    N, C, H, W = x.shape
    if N == 0:  # empty batch: nothing to launch (the reference's conv2d returns an empty tensor too)
        return empty_packed(0, C, H, W, x.device)
    with torch.cuda.device(x.device):
        a = empty_packed(N, C, H, W, x.device)
        fn = {native.DTYPE_F32: lib.bnn_hip_pack_act_f32, native.DTYPE_F16: lib.bnn_hip_pack_act_f16,
              native.DTYPE_BF16: lib.bnn_hip_pack_act_bf16}[_act_dtype(x)]
        native.check(fn(x.data_ptr(), N, C, H, W, a.P.data_ptr(), a.M.data_ptr(), _stream(x.device)),
                     "bnn_hip_pack_act")
    return a


def bn_act_pack(x: torch.Tensor, bn_scale=None, bn_shift=None, relu: bool = False) -> PackedAct:
    """``sign(act(bn(x)))`` of an fp32 NCHW tensor in one pass: the input binarisation of a pre-activation
    block (bnn/models/layers/res_block.py:148, hierarchical_block.py:39)."""
    x = _nchw(x, "activation", "bn_act_pack")
    lib = native.require()
    N, C, H, W = x.shape
    bn_scale = _per_channel(bn_scale, C, "bn_scale")
    bn_shift = _per_channel(bn_shift, C, "bn_shift")
    if N == 0:
        a = empty_packed(0, C, H, W, x.device)
        a.nonneg = bool(relu)
        return a
    with torch.cuda.device(x.device):
        a = empty_packed(N, C, H, W, x.device)
        native.check(lib.bnn_hip_bn_act_pack_f32(x.data_ptr(), N, C, H, W, _ptr(bn_scale), _ptr(bn_shift),
                                                 int(bool(relu)), a.P.data_ptr(), a.M.data_ptr(),
                                                 _stream(x.device)), "bnn_hip_bn_act_pack_f32")
    a.nonneg = bool(relu)
    return a


def channel_view(t: torch.Tensor, what: str = "tensor"):
    """``(base tensor, c_offset, c_total)`` of ``t``: a contiguous fp32 NCHW tensor on a HIP device, or a slice
    ``base[:, c0:c1]`` of one (what a cell state is: a run of channels of the cell's concatenated output).  No copy."""
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 4):
        raise native.NativeError(f"bnn_amd: {what} must be a float32 NCHW tensor on a HIP device")
    if t.is_contiguous():
        return t, 0, t.shape[1]
    N, C, H, W = t.shape
    sn, sc, sh, sw = t.stride()
    hw = H * W
    off = t.storage_offset()
    if (sc, sh, sw) == (hw, W, 1) and hw > 0 and sn % hw == 0 and sn // hw >= C:
        c_total = sn // hw
        c_off = (off % sn) // hw
        if (off % sn) % hw == 0 and c_off + C <= c_total and off >= c_off * hw:
            base = torch.as_strided(t, (N, c_total, H, W), (sn, hw, W, 1), off - c_off * hw)
            return base, c_off, c_total
    raise native.NativeError(f"bnn_amd: {what} is neither contiguous nor a channel slice of a contiguous NCHW tensor")


def _view_struct(t: torch.Tensor, what: str):
    base, c_off, c_total = channel_view(t, what)
    return native.F32View(base.data_ptr(), c_off, c_total), base


def _affine_table(v, n: int, what: str) -> torch.Tensor:
    """``K`` per-channel affine vectors as one fp32 ``[K, n]`` tensor on the device (a sequence of vectors is stacked)."""
    v = torch.stack([_per_channel(e, n, what) for e in v]) if isinstance(v, (list, tuple)) else v
    v = _require_cuda_f32(v.detach(), what)
    if v.dim() != 2 or v.shape[1] != n:
        raise native.NativeError(f"bnn_amd: {what} must be [K, {n}]")
    return v


def bn_act_pack_multi(x: torch.Tensor, bn_scales, bn_shifts, relu: bool = False) -> list:
    """``K`` plane sets ``sign(bn_k(x))`` from ONE read of ``x`` (``bnn_hip_bn_act_pack_multi_f32``, ``1 <= K <= 4``):
    ``bn_scales`` / ``bn_shifts`` are ``[K, C]`` (or sequences of ``K`` vectors).  ``x`` may be a channel slice of a wider
    contiguous tensor (``channel_view``); it is read in place.  Returns ``K`` ``PackedAct``, each with the bits of
    ``bn_act_pack(x.contiguous(), scale_k, shift_k, relu)``."""
    view, _keep = _view_struct(x, "activation")
    N, C, H, W = x.shape
    a, b = _affine_table(bn_scales, C, "bn_scales"), _affine_table(bn_shifts, C, "bn_shifts")
    K = a.shape[0]
    if not 1 <= K <= 4 or b.shape[0] != K:
        raise native.NativeError(f"bnn_amd: bn_act_pack_multi takes 1..4 affines, got {K} / {b.shape[0]}")
    lib = native.require()
    cw64 = (C + 63) // 64
    with torch.cuda.device(x.device):
        P = torch.empty((K, N, cw64, H, W), dtype=torch.int64, device=x.device)
        M = torch.empty_like(P)
        if N:
            native.check(lib.bnn_hip_bn_act_pack_multi_f32(ctypes.byref(view), N, C, H, W, K, a.data_ptr(), b.data_ptr(),
                                                           int(bool(relu)), P.data_ptr(), M.data_ptr(), _stream(x.device)),
                         "bnn_hip_bn_act_pack_multi_f32")
    return [PackedAct(P[k], M[k], (N, C, H, W), bool(relu)) for k in range(K)]


def bn_act_pack_s2(x: torch.Tensor, bn_scale=None, bn_shift=None, relu: bool = False):
    """The binarisation inside ``FactorizedReduce`` (``bnn_hip_bn_act_pack_s2_f32``): ``(phase0, phase1)`` with the bits
    of ``bn_act_pack`` on ``x[:, :, ::2, ::2]`` and ``x[:, :, 1::2, 1::2]``, from one pass over ``x`` (H and W even;
    ``x`` may be a channel slice, like ``bn_act_pack_multi``)."""
    view, _keep = _view_struct(x, "activation")
    N, C, H, W = x.shape
    bn_scale = _per_channel(bn_scale, C, "bn_scale")
    bn_shift = _per_channel(bn_shift, C, "bn_shift")
    lib = native.require()
    cw64 = (C + 63) // 64
    with torch.cuda.device(x.device):
        P = torch.empty((2, N, cw64, H // 2, W // 2), dtype=torch.int64, device=x.device)
        M = torch.empty_like(P)
        if N:
            native.check(lib.bnn_hip_bn_act_pack_s2_f32(ctypes.byref(view), N, C, H, W, _ptr(bn_scale), _ptr(bn_shift),
                                                        int(bool(relu)), P.data_ptr(), M.data_ptr(), _stream(x.device)),
                         "bnn_hip_bn_act_pack_s2_f32")
    return tuple(PackedAct(P[k], M[k], (N, C, H // 2, W // 2), bool(relu)) for k in range(2))


def _join_plane_sets(parts: list, K: int, plane_shape, device):
    """``(P, M)`` ``[K, N, cw64, H, W]`` from the ``[K, n, cw64, H, W]`` pairs of each launch of a cut batch: the pair
    itself for one launch, a concatenation over the batch for several, empty ``[K, 0, *plane_shape]`` planes for none."""
    if len(parts) == 1:
        return parts[0]
    if parts:
        return torch.cat([p for p, _ in parts], 1), torch.cat([m for _, m in parts], 1)
    P = torch.empty((K, 0, *plane_shape), dtype=torch.int64, device=device)
    return P, torch.empty_like(P)


_STEM3X3_MAX_ELEMS = (1 << 31) - 1      # fp32 elements of x or y one stem3x3 launch covers (capi.hip: kMaxElems)


def stem3x3_bn_relu_pack(x: torch.Tensor, w: torch.Tensor, bn_scale: torch.Tensor, bn_shift: torch.Tensor, pack_scales,
                         pack_shifts, out_f32: bool = True):
    """The real-valued stem of a BATS CIFAR network with the binarisation of its ``K`` consumers in one launch
    (``bnn_hip_stem3x3_bn_relu_pack_f32``): ``y = relu(bn(conv3x3(x)))`` for ``x`` ``[N, 3, H, W]``, ``w`` ``[O, 3, 3, 3]``
    (stride 1, padding 1, no bias) and the folded BatchNorm ``bn_scale`` / ``bn_shift`` ``[O]``; ``pack_scales`` /
    ``pack_shifts`` are ``[K, O]`` (or sequences of ``K`` vectors), ``1 <= K <= 4``.  Returns ``(y | None, [K PackedAct])``
    where set ``k`` holds the bits of ``bn_act_pack_multi(y, pack_scales, pack_shifts)[k]``; ``out_f32=False``: ``y`` is
    not written.  A batch whose ``x`` or ``y`` would reach 2^31 elements is cut into several launches."""
    x = _require_cuda_f32(x, "stem input")
    w = _require_cuda_f32(w.detach(), "stem weight")
    if x.dim() != 4 or x.shape[1] != 3 or w.dim() != 4 or tuple(w.shape[1:]) != (3, 3, 3):
        raise native.NativeError(f"bnn_amd: stem3x3 expects x [N,3,H,W] and w [O,3,3,3], got {tuple(x.shape)} and "
                                 f"{tuple(w.shape)}")
    N, _, H, W = x.shape
    O = w.shape[0]
    bn_scale, bn_shift = _per_channel(bn_scale, O, "bn_scale"), _per_channel(bn_shift, O, "bn_shift")
    a, b = _affine_table(pack_scales, O, "pack_scales"), _affine_table(pack_shifts, O, "pack_shifts")
    K = a.shape[0]
    if not 1 <= K <= 4 or b.shape[0] != K:
        raise native.NativeError(f"bnn_amd: stem3x3 takes 1..4 affines, got {K} / {b.shape[0]}")
    lib = native.require()
    cw64 = (O + 63) // 64
    step = max(1, min(N, _STEM3X3_MAX_ELEMS // (max(O, 3) * H * W)))
    with torch.cuda.device(x.device):
        y = torch.empty((N, O, H, W), dtype=torch.float32, device=x.device) if out_f32 else None
        parts = []
        for n0, n1 in _split(N, step):          # (one launch unless the batch is cut: a plane set is [n, cw64, H, W])
            P = torch.empty((K, n1 - n0, cw64, H, W), dtype=torch.int64, device=x.device)
            M = torch.empty_like(P)
            native.check(lib.bnn_hip_stem3x3_bn_relu_pack_f32(
                x[n0:n1].data_ptr(), w.data_ptr(), bn_scale.data_ptr(), bn_shift.data_ptr(), a.data_ptr(), b.data_ptr(),
                n1 - n0, O, H, W, K, P.data_ptr(), M.data_ptr(), None if y is None else y[n0:n1].data_ptr(),
                _stream(x.device)), "bnn_hip_stem3x3_bn_relu_pack_f32")
            parts.append((P, M))
        P, M = _join_plane_sets(parts, K, (cw64, H, W), x.device)
    return y, [PackedAct(P[k], M[k], (N, O, H, W), False) for k in range(K)]


STEM_S2_TILE = native.STEM_S2_TILE      # (rows, columns) of output pixels one workgroup of the two kernels below owns
_STEM_S2_MAX_ELEMS = (1 << 31) - 1      # fp32 elements of the input or output one launch of them covers (capi.hip: kMaxElems)


def _half(v: int) -> int:
    """Output extent of a 3x3 / stride 2 / padding 1 convolution."""
    return (v + 1) // 2


def _grouped_w(w: torch.Tensor, c_in: int, groups: int, what: str) -> torch.Tensor:
    w = _require_cuda_f32(w.detach(), what)
    if (groups < 1 or c_in % groups or w.dim() != 4 or w.shape[0] % groups
            or tuple(w.shape[1:]) != (c_in // groups, 3, 3)):
        raise native.NativeError(f"bnn_amd: {what} must be [O, {c_in}/groups, 3, 3] with groups dividing both channel "
                                 f"counts, got {tuple(w.shape)} and groups = {groups}")
    return w


def stem_s2x2(x: torch.Tensor, w1: torch.Tensor, s1: torch.Tensor, t1: torch.Tensor, w2: torch.Tensor, s2: torch.Tensor,
              t2: torch.Tensor, groups: int, relu_out: bool = False) -> torch.Tensor:
    """``stem0`` of a BATS ImageNet network in one launch (``bnn_hip_stem_s2x2_f32``): ``Conv2d(3, C1, 3, stride 2, pad
    1)`` -> BatchNorm ``s1`` / ``t1`` -> ReLU -> ``Conv2d(C1, C, 3, stride 2, pad 1, groups)`` -> BatchNorm ``s2`` / ``t2``,
    and a ReLU on the way out when ``relu_out``.  ``x`` ``[N, 3, H, W]``, ``w1`` ``[C1, 3, 3, 3]``, ``w2``
    ``[C, C1 / groups, 3, 3]``, no biases; returns fp32 ``[N, C, ceil(ceil(H/2)/2), ceil(ceil(W/2)/2)]``.  The intermediate
    never reaches memory.  A batch whose input or output would reach 2^31 elements is cut into several launches."""
    x = _require_cuda_f32(x, "stem input")
    w1 = _require_cuda_f32(w1.detach(), "stem weight")
    if x.dim() != 4 or x.shape[1] != 3 or w1.dim() != 4 or tuple(w1.shape[1:]) != (3, 3, 3):
        raise native.NativeError(f"bnn_amd: stem_s2x2 expects x [N,3,H,W] and w1 [C1,3,3,3], got {tuple(x.shape)} and "
                                 f"{tuple(w1.shape)}")
    N, _, H, W = x.shape
    C1 = w1.shape[0]
    w2 = _grouped_w(w2, C1, groups, "second stem weight")
    C = w2.shape[0]
    s1, t1 = _per_channel(s1, C1, "s1"), _per_channel(t1, C1, "t1")
    s2, t2 = _per_channel(s2, C, "s2"), _per_channel(t2, C, "t2")
    lib = native.require()
    H2, W2 = _half(_half(H)), _half(_half(W))
    step = max(1, min(N, _STEM_S2_MAX_ELEMS // max(3 * H * W, C * H2 * W2, 1)))
    with torch.cuda.device(x.device):
        y = torch.empty((N, C, H2, W2), dtype=torch.float32, device=x.device)
        for n0, n1 in _split(N if H * W else 0, step):
            native.check(lib.bnn_hip_stem_s2x2_f32(
                x[n0:n1].data_ptr(), w1.data_ptr(), s1.data_ptr(), t1.data_ptr(), w2.data_ptr(), s2.data_ptr(),
                t2.data_ptr(), n1 - n0, C1, C, groups, H, W, int(bool(relu_out)), y[n0:n1].data_ptr(), _stream(x.device)),
                "bnn_hip_stem_s2x2_f32")
    return y


def gconv3x3s2_bn_pack(x: torch.Tensor, w: torch.Tensor, bn_scale: torch.Tensor, bn_shift: torch.Tensor, groups: int,
                       pack_scales=None, pack_shifts=None, relu_in: bool = False, out_f32: bool = True):
    """``stem1`` of a BATS ImageNet network with the binarisation of its ``K`` consumers in one launch
    (``bnn_hip_gconv3x3s2_bn_pack_f32``): ``y = bn(conv3x3(relu(x) if relu_in else x))`` for ``x`` ``[N, C, H, W]``, ``w``
    ``[O, C / groups, 3, 3]`` (stride 2, padding 1, no bias) and the folded BatchNorm ``bn_scale`` / ``bn_shift`` ``[O]``;
    ``pack_scales`` / ``pack_shifts`` are ``[K, O]`` (or sequences of ``K`` vectors), ``0 <= K <= 4`` (None: ``K = 0``).
    Returns ``(y | None, [K PackedAct])`` where set ``k`` holds the bits of ``bn_act_pack_multi(y, pack_scales,
    pack_shifts)[k]``; ``out_f32=False`` (``K >= 1`` only): ``y`` is not written.  A batch whose ``x`` or ``y`` would reach
    2^31 elements is cut into several launches."""
    x = _nchw(x, "activation", "gconv3x3s2_bn_pack")
    N, C, H, W = x.shape
    w = _grouped_w(w, C, groups, "weight")
    O = w.shape[0]
    bn_scale, bn_shift = _per_channel(bn_scale, O, "bn_scale"), _per_channel(bn_shift, O, "bn_shift")
    if (pack_scales is None) != (pack_shifts is None):
        raise native.NativeError("bnn_amd: gconv3x3s2_bn_pack takes pack_scales and pack_shifts together")
    none = pack_scales is None or len(pack_scales) == 0
    a, b = (None, None) if none else (_affine_table(pack_scales, O, "pack_scales"),
                                      _affine_table(pack_shifts, O, "pack_shifts"))
    K = 0 if none else a.shape[0]
    if K > 4 or (K and b.shape[0] != K):
        raise native.NativeError(f"bnn_amd: gconv3x3s2_bn_pack takes 0..4 affines, got {K}")
    if K == 0 and not out_f32:
        raise native.NativeError("bnn_amd: gconv3x3s2_bn_pack without affines must write the fp32 output")
    lib = native.require()
    Ho, Wo = _half(H), _half(W)
    cw64 = (O + 63) // 64
    step = max(1, min(N, _STEM_S2_MAX_ELEMS // max(C * H * W, O * Ho * Wo, 1)))
    with torch.cuda.device(x.device):
        y = torch.empty((N, O, Ho, Wo), dtype=torch.float32, device=x.device) if out_f32 else None
        parts = []
        for n0, n1 in _split(N if H * W else 0, step):   # (one launch unless the batch is cut: a plane set is [n, cw64, Ho, Wo])
            P = torch.empty((K, n1 - n0, cw64, Ho, Wo), dtype=torch.int64, device=x.device)
            M = torch.empty_like(P)
            native.check(lib.bnn_hip_gconv3x3s2_bn_pack_f32(
                x[n0:n1].data_ptr(), w.data_ptr(), bn_scale.data_ptr(), bn_shift.data_ptr(), _ptr(a), _ptr(b), n1 - n0, C, O,
                groups, H, W, int(bool(relu_in)), K, P.data_ptr() if K else None, M.data_ptr() if K else None,
                None if y is None else y[n0:n1].data_ptr(), _stream(x.device)), "bnn_hip_gconv3x3s2_bn_pack_f32")
            parts.append((P, M))
        P, M = _join_plane_sets(parts, K, (cw64, Ho, Wo), x.device)
    return y, [PackedAct(P[k], M[k], (N, O, Ho, Wo), False) for k in range(K)]


def avgpool_pack(x: torch.Tensor, k: int, nonneg: bool = False) -> PackedAct:
    """``AvgPool2d(k, k, ceil_mode=True, count_include_pad=False)`` + sign, fused
    (shortcut branch of bnn/models/resnet.py:128-133).  ``nonneg``: the caller knows ``x >= 0``
    (it is a ReLU output), so the averages are too."""
    x = _nchw(x, "activation", "avgpool_pack")
    lib = native.require()
    N, C, H, W = x.shape
    ho, wo = (H + k - 1) // k, (W + k - 1) // k
    with torch.cuda.device(x.device):
        a = empty_packed(N, C, ho, wo, x.device)
        native.check(lib.bnn_hip_avgpool_pack_f32(x.data_ptr(), N, C, H, W, k, a.P.data_ptr(),
                                                  a.M.data_ptr(), _stream(x.device)),
                     "bnn_hip_avgpool_pack_f32")
    a.nonneg = bool(nonneg)
    return a


def orpool_packed(a: PackedAct, k: int) -> PackedAct:
    """``sign(AvgPool2d(k, k, ceil_mode=True, count_include_pad=False)(x))`` from the sign planes of a
    NON-NEGATIVE ``x`` (``a.nonneg``): the OR of the P plane over each window (include/bnn_hip.h)."""
    if not a.nonneg:
        raise native.NativeError("bnn_amd: orpool_packed needs planes of a non-negative tensor (nonneg=True)")
    lib = native.require()
    N, C, H, W = a.shape
    ho, wo = (H + k - 1) // k, (W + k - 1) // k
    dev = a.P.device
    with torch.cuda.device(dev):
        out = empty_packed(N, C, ho, wo, dev)
        if N:
            native.check(lib.bnn_hip_orpool_packed(a.P.data_ptr(), N, C, H, W, k, out.P.data_ptr(), out.M.data_ptr(),
                                                   _stream(dev)), "bnn_hip_orpool_packed")
    out.nonneg = True
    return out


def stem7x7(x: torch.Tensor, w: torch.Tensor, bn_scale: torch.Tensor, bn_shift: torch.Tensor,
            out_f32: bool = True, out_packed: bool = True, exact_fp32: bool = False, fp16: bool = False,
            out: Optional[tuple] = None, pack_affine: Optional[tuple] = None):
    """conv 7x7/2/3 (3->64, no bias) -> folded BN -> ReLU -> MaxPool 3/2/1 in one MFMA kernel
    (bnn/models/resnet.py:93-96,150-153).  Returns (fp32 NCHW | None, PackedAct | None).
    ``out = (y, PackedAct)``: write into these preallocated results of an earlier call with the same input shape
    (the static buffers a captured HIP graph of the rest of the network reads: ``FusedResNet.forward_fresh``).
    ``pack_affine = (scale, shift)``: the planes are those of ``fmaf(y, scale[c], shift[c]) > 0`` — the input of a
    pre-activation block's first binary layer (its bn1 + ReLU) — instead of ``y > 0``; the fp32 output is unchanged.

    Arithmetic and what it admits (oracle and derivation: ``tests/stem_ref.py``).  Default: both fp32 operands split
    into fp16 ``hi + lo``, ``hi*hi + lo*hi + hi*lo`` with fp32 accumulation; the convolution is within
    ``147 * 2^-24 * (|x| conv |w|)`` of the exact one per element — the worst case of an fp32 fmaf chain —, the fused
    output within ``|bn_scale|`` times that plus one rounding.  Weights of any size are admitted: a channel whose largest
    ``|w|`` is below 2^-5 is multiplied by the power of two that brings it into [1, 2) before the split and its
    ``bn_scale`` by the inverse, inside the kernel and exactly (above 2^-5 nothing is scaled).  The image is not
    rescaled: the bound holds for images whose largest magnitude is at most 2^15 (``hi`` stays finite) and whose typical
    magnitude is at least 2^-8 (below that the ``lo`` halves of the pixels go subnormal and the error grows towards
    ``fp16``'s); normalised and [0, 1] images are well inside.  ``fp16``: one product of the rounded operands, the same
    bound with 2^-11 for 2^-24, same ranges.  ``exact_fp32``: an fp32 fmaf chain, any fp32 operands."""
    x = _require_cuda_f32(x, "stem input")
    w = _require_cuda_f32(w.detach(), "stem weight")
    if x.dim() != 4 or x.shape[1] != 3 or tuple(w.shape) != (64, 3, 7, 7):
        raise native.NativeError("bnn_amd: stem7x7 expects x [N,3,H,W] and w [64,3,7,7]")
    lib = native.require()
    N, _, H, W = x.shape
    hp, wp = _half_hw(*_half_hw(H, W))
    bn_scale = _per_channel(bn_scale, 64, "bn_scale")
    bn_shift = _per_channel(bn_shift, 64, "bn_shift")
    with torch.cuda.device(x.device):
        if out is not None:
            y, pk = out
            wrong = "stem7x7: `out` does not belong to this input shape / device"
            _written(y, (N, 64, hp, wp), "out", wrong)
            if (y is not None and y.device != x.device) or \
                    (pk is not None and (tuple(pk.shape) != (N, 64, hp, wp) or pk.P.device != x.device)):
                raise native.NativeError("bnn_amd: " + wrong)
        else:
            y = torch.empty((N, 64, hp, wp), dtype=torch.float32, device=x.device) if out_f32 else None
            pk = empty_packed(N, 64, hp, wp, x.device) if out_packed else None
        step = _stem_launch_images(N, H, W, hp, wp)   # larger batches go in several launches
        flags = native.STEM_EXACT_FP32 if exact_fp32 else (native.STEM_FP16 if fp16 else 0)
        symbol, affine = "bnn_hip_stem7x7_bn_relu_pool_pack_f32", ()
        if pack_affine is not None:
            if exact_fp32 or pk is None:
                raise native.NativeError("bnn_amd: stem7x7(pack_affine=...) needs packed output and is not built for the exact-fp32 stem")
            pa, pb = _per_channel(pack_affine[0], 64, "pack scale"), _per_channel(pack_affine[1], 64, "pack shift")
            symbol, affine = "bnn_hip_stem7x7_bn_relu_pool_pack_affine_f32", (pa.data_ptr(), pb.data_ptr())
        for n0, n1 in _split(N, step):
            native.check(getattr(lib, symbol)(
                x[n0:n1].data_ptr(), w.data_ptr(), bn_scale.data_ptr(), bn_shift.data_ptr(), *affine, n1 - n0, H, W, flags,
                None if y is None else y[n0:n1].data_ptr(),
                None if pk is None else pk.P[n0:n1].data_ptr(), None if pk is None else pk.M[n0:n1].data_ptr(),
                _stream(x.device)), symbol)
    if pk is not None:
        pk.nonneg = True  # ReLU output
    return y, pk


def stem7x7_conv(x: torch.Tensor, w: torch.Tensor, fp16: bool = False) -> torch.Tensor:
    """The stem's convolution alone — conv 7x7/2/3, 3 -> 64, no bias (bnn/models/resnet.py:93,150) — on the matrix cores
    (``bnn_hip_stem7x7_conv_f32``: the MFMA stream of ``stem7x7``): what a TRAINING step needs in front of its
    batch-statistics BatchNorm.  Returns fp32 ``[N, 64, Hc, Wc]``.
    Every element is within ``147 * 2^-24 * (|x| conv |w|)`` of the exact convolution (``fp16``: 2^-11 for 2^-24) for
    weights of any size — a channel below 2^-5 is split at a power-of-two scale and the stored value scaled back, exactly,
    on every launch, so a training step's changing weights need no preparation — and images whose largest magnitude is at
    most 2^15 and whose typical magnitude is at least 2^-8 (see ``stem7x7``; ``tests/stem_ref.py``)."""
    x = _require_cuda_f32(x, "stem input")
    w = _require_cuda_f32(w.detach(), "stem weight")
    if x.dim() != 4 or x.shape[1] != 3 or tuple(w.shape) != (64, 3, 7, 7):
        raise native.NativeError("bnn_amd: stem7x7_conv expects x [N,3,H,W] and w [64,3,7,7]")
    lib = native.require()
    N, _, H, W = x.shape
    hc, wc = _half_hw(H, W)
    with torch.cuda.device(x.device):
        y = torch.empty((N, 64, hc, wc), dtype=torch.float32, device=x.device)
        step = _stem_launch_images(N, H, W, hc, wc)
        for n0, n1 in _split(N, step):
            native.check(lib.bnn_hip_stem7x7_conv_f32(x[n0:n1].data_ptr(), w.data_ptr(), n1 - n0, H, W,
                                                      native.STEM_FP16 if fp16 else 0, y[n0:n1].data_ptr(),
                                                      _stream(x.device)), "bnn_hip_stem7x7_conv_f32")
    return y


def stem7x7_wgrad_supported(x: torch.Tensor) -> bool:
    """``stem7x7_wgrad`` implements this input size (image rows up to ~950 pixels: the kernel's LDS patch)."""
    lib = native.require()
    return x.dim() == 4 and x.shape[1] == 3 and lib.bnn_hip_stem7x7_wgrad_workspace_bytes(
        int(x.shape[0]), int(x.shape[2]), int(x.shape[3])) > 0


def stem7x7_wgrad(x: torch.Tensor, dy: torch.Tensor) -> torch.Tensor:
    """Weight gradient of the stem's convolution (``bnn_hip_stem7x7_wgrad_f32``; what
    ``aten::convolution_backward(dy, x, w, ...)[1]`` returns for conv 7x7/2/3, 3 -> 64): fp32 ``[64, 3, 7, 7]``.
    fp32 products on the matrix cores, partial sums added in index order — the same bits on every run."""
    x = _require_cuda_f32(x, "stem input")
    dy = _require_cuda_f32(dy, "stem output gradient")
    if x.dim() != 4 or x.shape[1] != 3:
        raise native.NativeError(f"bnn_amd: stem7x7_wgrad expects x [N,3,H,W], got {tuple(x.shape)}")
    N, _, H, W = x.shape
    if tuple(dy.shape) != (N, 64) + _half_hw(H, W):
        raise native.NativeError("bnn_amd: stem7x7_wgrad expects x [N,3,H,W] and dy [N,64,Hc,Wc]")
    lib = native.require()
    with torch.cuda.device(x.device):
        need = lib.bnn_hip_stem7x7_wgrad_workspace_bytes(N, H, W)
        if need == 0:
            raise native.NativeError(f"bnn_amd: stem7x7_wgrad does not implement input size {tuple(x.shape)}")
        work = torch.empty(need // 4, dtype=torch.float32, device=x.device)
        dw = torch.empty((64, 3, 7, 7), dtype=torch.float32, device=x.device)
        native.check(lib.bnn_hip_stem7x7_wgrad_f32(x.data_ptr(), dy.data_ptr(), N, H, W, work.data_ptr(), need,
                                                   dw.data_ptr(), _stream(x.device)), "bnn_hip_stem7x7_wgrad_f32")
    return dw


def avgpool2x2_backward(gy: torch.Tensor) -> torch.Tensor:
    """Backward of ``AvgPool2d(2, 2)`` on an even-sized map: ``gx[..., 2y + a, 2x + b] = gy[..., y, x] / 4``
    (``bnn_hip_avgpool2x2_backward_f32``)."""
    gy = _require_cuda_f32(gy, "pooled gradient")
    if gy.dim() != 4:
        raise native.NativeError("bnn_amd: avgpool2x2_backward expects [N,C,Ho,Wo]")
    lib = native.require()
    N, C, Ho, Wo = gy.shape
    with torch.cuda.device(gy.device):
        gx = torch.empty((N, C, 2 * Ho, 2 * Wo), dtype=torch.float32, device=gy.device)
        native.check(lib.bnn_hip_avgpool2x2_backward_f32(gy.data_ptr(), N, C, Ho, Wo, gx.data_ptr(), _stream(gy.device)),
                     "bnn_hip_avgpool2x2_backward_f32")
    return gx


def avgpool2_bn_pack2(x: torch.Tensor, bn1, relu1: bool, bn2=None, relu2: bool = False, out_f32: bool = False):
    """``AvgPool2d(2, 2)`` of an fp32 NCHW tensor (even H, W) + ``sign(act(bn(.)))`` of the pooled tensor for up to two
    BatchNorm branches in one pass (``bnn_hip_avgpool2_bn_pack2_f32``).  ``bn1`` / ``bn2``: (scale, shift).
    Returns ``(PackedAct 1, PackedAct 2 | None, pooled fp32 | None)``."""
    x = _nchw(x, "activation", "avgpool2_bn_pack2")
    lib = native.require()
    N, C, H, W = x.shape
    if H % 2 or W % 2:
        raise native.NativeError("bnn_amd: avgpool2_bn_pack2 needs even H and W")
    a1, b1 = _per_channel(bn1[0], C, "bn scale"), _per_channel(bn1[1], C, "bn shift")
    a2 = b2 = None
    if bn2 is not None:
        a2, b2 = _per_channel(bn2[0], C, "bn scale"), _per_channel(bn2[1], C, "bn shift")
    with torch.cuda.device(x.device):
        p1 = empty_packed(N, C, H // 2, W // 2, x.device)
        p2 = empty_packed(N, C, H // 2, W // 2, x.device) if bn2 is not None else None
        t = torch.empty((N, C, H // 2, W // 2), dtype=torch.float32, device=x.device) if out_f32 else None
        if N:
            native.check(lib.bnn_hip_avgpool2_bn_pack2_f32(
                x.data_ptr(), N, C, H, W, a1.data_ptr(), b1.data_ptr(), int(bool(relu1)), p1.P.data_ptr(), p1.M.data_ptr(),
                _ptr(a2), _ptr(b2), int(bool(relu2)), None if p2 is None else p2.P.data_ptr(),
                None if p2 is None else p2.M.data_ptr(), _ptr(t), _stream(x.device)), "bnn_hip_avgpool2_bn_pack2_f32")
    p1.nonneg = bool(relu1)
    if p2 is not None:
        p2.nonneg = bool(relu2)
    return p1, p2, t


def sign_thresholds(w: PackedWeight, bn_scale: torch.Tensor, bn_shift: torch.Tensor, bias=None, post_scale=None):
    """Integer form of ``sign(relu(bn(alpha * dot + bias)))`` for ``bconv2d_fused(..., sign_thresholds=...)``:
    int32 ``[O, 4]`` = (bound T, flip word of the channel's 32-channel block, the two comparands of the kernels'
    two-instruction form of the test), ``bit = (dot >= T) ^ flip``, derived on
    the device with the epilogue's own float operations
    (include/bnn_hip.h: bnn_hip_sign_thresholds_f32).  Valid for THIS weight pack and THESE BatchNorm constants."""
    lib = native.require()
    O, C, KH, KW = w.shape
    dev = w.alpha.device
    bn_scale = _per_channel(bn_scale, O, "bn_scale")
    bn_shift = _per_channel(bn_shift, O, "bn_shift")
    bias = _per_channel(bias, O, "bias")
    post_scale = _per_channel(post_scale, O, "post_scale")
    with torch.cuda.device(dev):
        thr = torch.empty(((O + 31) // 32 * 32, 4), dtype=torch.int32, device=dev)   # whole 32-channel blocks
        native.check(lib.bnn_hip_sign_thresholds_f32(w.alpha.data_ptr(), _ptr(bias), _ptr(post_scale), bn_scale.data_ptr(),
                                                     bn_shift.data_ptr(), O, C * KH * KW, thr.data_ptr(), _stream(dev)),
                     "bnn_hip_sign_thresholds_f32")
    return thr


def avgpool_fc(x: torch.Tensor, w_t: torch.Tensor, bias: Optional[torch.Tensor], one_kernel: bool = False) -> torch.Tensor:
    """``fc(flatten(avgpool(x)))`` of bnn/models/resnet.py:160-164.  ``x``: fp32 ``[N,C,H,W]``,
    ``w_t``: the Linear weight transposed to ``[C,O]`` (contiguous), ``bias``: ``[O]`` or None.
    Two streaming launches through a workspace (``bnn_hip_avgpool_fc_ws_f32``); ``one_kernel``: the round-2 single
    kernel (``bnn_hip_avgpool_fc_f32``: same means, another summation order of the product)."""
    x = _require_cuda_f32(x, "head input")
    w_t = _require_cuda_f32(w_t.detach(), "head weight")
    if x.dim() != 4 or w_t.dim() != 2 or w_t.shape[0] != x.shape[1]:
        raise native.NativeError("bnn_amd: avgpool_fc expects x [N,C,H,W] and w_t [C,O]")
    lib = native.require()
    N, C, H, W = x.shape
    O = w_t.shape[1]
    bias = _per_channel(bias, O, "head bias")
    with torch.cuda.device(x.device):
        out = torch.empty((N, O), dtype=torch.float32, device=x.device)
        if N and one_kernel:
            native.check(lib.bnn_hip_avgpool_fc_f32(x.data_ptr(), N, C, H * W, w_t.data_ptr(), _ptr(bias), O,
                                                    out.data_ptr(), _stream(x.device)), "bnn_hip_avgpool_fc_f32")
        elif N:
            nbytes = int(lib.bnn_hip_avgpool_fc_workspace_bytes(N, C))
            ws = torch.empty((max(nbytes, 16) + 3) // 4, dtype=torch.float32, device=x.device)
            native.check(lib.bnn_hip_avgpool_fc_ws_f32(x.data_ptr(), N, C, H * W, w_t.data_ptr(), _ptr(bias), O,
                                                       out.data_ptr(), ws.data_ptr(), nbytes, _stream(x.device)),
                         "bnn_hip_avgpool_fc_ws_f32")
    return out


def bn_relu_maxpool_pack(x: torch.Tensor, bn_scale=None, bn_shift=None, relu: bool = True, k: int = 3,
                         stride: int = 2, pad: int = 1, out_f32: bool = True, out_packed: bool = True):
    """Stem tail in one pass: folded BN -> MaxPool2d(k, stride, pad) -> ReLU, written as fp32
    and/or sign planes (bnn/models/resnet.py:150-153 + the first binary conv's binarizer)."""
    x = _nchw(x, "activation", "bn_relu_maxpool_pack")
    lib = native.require()
    N, C, H, W = x.shape
    ho, wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    bn_scale = _per_channel(bn_scale, C, "bn_scale")
    bn_shift = _per_channel(bn_shift, C, "bn_shift")
    with torch.cuda.device(x.device):
        y = torch.empty((N, C, ho, wo), dtype=torch.float32, device=x.device) if out_f32 else None
        pk = empty_packed(N, C, ho, wo, x.device) if out_packed else None
        native.check(lib.bnn_hip_bn_relu_maxpool_pack_f32(
            x.data_ptr(), N, C, H, W, _ptr(bn_scale), _ptr(bn_shift), int(bool(relu)), k, stride, pad,
            _ptr(y), None if pk is None else pk.P.data_ptr(), None if pk is None else pk.M.data_ptr(),
            _stream(x.device)), "bnn_hip_bn_relu_maxpool_pack_f32")
    if pk is not None:
        pk.nonneg = bool(relu)
    return y, pk


def _weight_f32(w: torch.Tensor) -> Tuple[torch.Tensor, bool]:
    """The weight as fp32 on its HIP device + whether it came as fp16 (a `.half()` model: the sign bits are those of the
    exact fp32 widening; ``_run_weight_pack`` rounds alpha to fp16)."""
    half = w.dtype == torch.float16
    if half:
        w = w.detach().float()
    return _require_cuda_f32(w.detach(), "weight"), half


def _run_weight_pack(w: torch.Tensor, half: bool, L: native.WLayout, what: str, sync: bool, launch, **kind) -> PackedWeight:
    """What ``pack_weight`` and ``pack_weight_grouped`` share: the buffers of layout ``L``, the launch
    (``launch(wbits, wnz, alpha, zero flag, stream)`` -> status of the entry point ``what``) and the zero-weight flag's
    way back to the host (their ``sync``).  ``kind``: the ``PackedWeight`` fields beyond those of a dense pack."""
    with torch.cuda.device(w.device):
        wbits = torch.empty(L.n_words, dtype=torch.int32, device=w.device)
        wnz = torch.empty(L.n_words, dtype=torch.int32, device=w.device)
        alpha = torch.empty(L.o_pad, dtype=torch.float32, device=w.device)
        flag = torch.zeros(1, dtype=torch.int32, device=w.device)
        native.check(launch(wbits.data_ptr(), wnz.data_ptr(), alpha.data_ptr(), flag.data_ptr(), _stream(w.device)), what)
        if half:  # the reference computes alpha in the weight's own dtype (bnn/ops.py:116-127)
            alpha = alpha.half().float()
        if not sync:
            host = torch.empty(1, dtype=torch.int32, pin_memory=True)
            host.copy_(flag, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(w.device))
            return PackedWeight(wbits, wnz, alpha, False, tuple(w.shape), (host, ev), **kind)
        has_zero = bool(flag.item())
    return PackedWeight(wbits, wnz, alpha, has_zero, tuple(w.shape), **kind)


def pack_weight(w: torch.Tensor, center: bool = False, compute_alpha: bool = True,
                sync: bool = True) -> PackedWeight:
    """``XNORWeightBinarizer`` on device (bnn/ops.py:116-140).  Synchronises once to read the
    zero-weight flag — call it when the weight changes, not per forward.

    ``sync=False`` (training: the weight changes every step) assumes "no exact zero" and returns at once;
    the flag travels to pinned host memory asynchronously and ``PackedWeight.zero_found_later()`` tells
    afterwards whether the assumption held (the caller then re-packs with ``sync=True``)."""
    w, half = _weight_f32(w)
    if w.dim() == 2:
        w = w[:, :, None, None]
    elif w.dim() == 3:
        w = w[:, :, None, :]
    if w.dim() != 4:
        raise native.NativeError(f"bnn_amd: unsupported weight rank {w.dim()}")
    w = w.contiguous()
    lib = native.require()
    O, C, KH, KW = w.shape
    return _run_weight_pack(w, half, native.weight_layout(O, C, KH, KW), "bnn_hip_pack_weight_f32", sync,
                            lambda *out: lib.bnn_hip_pack_weight_f32(w.data_ptr(), O, C, KH, KW, int(center),
                                                                     int(compute_alpha), *out))


def pack_weight_grouped(w: torch.Tensor, groups: int, center: bool = False, compute_alpha: bool = True,
                        sync: bool = True) -> PackedWeight:
    """``XNORWeightBinarizer`` of a grouped weight ``[O, C / groups, KH, KW]`` (``Conv1d``: ``[O, C / groups, K]``) into
    the windowed block-diagonal layout of ``bnn_hip_bconv2d_grouped`` (include/bnn_hip.h).  Centring and alpha reduce
    over the group's channels as the reference does; alpha has the bits of ``pack_weight`` of the same tensor.  fp16
    weights and ``sync`` as in ``pack_weight``."""
    w, half = _weight_f32(w)
    if w.dim() == 3:
        w = w[:, :, None, :]
    if w.dim() != 4:
        raise native.NativeError(f"bnn_amd: unsupported grouped weight rank {w.dim()}")
    w = w.contiguous()
    lib = native.require()
    O, Cg, KH, KW = w.shape
    if groups < 1 or O % groups:
        raise native.NativeError(f"bnn_amd: {O} output channels do not split into {groups} groups")
    L = native.grouped_weight_layout(O, Cg * groups, groups, KH, KW)
    return _run_weight_pack(w, half, L, "bnn_hip_pack_weight_grouped_f32", sync,
                            lambda *out: lib.bnn_hip_pack_weight_grouped_f32(w.data_ptr(), O, Cg, groups, KH, KW, int(center),
                                                                             int(compute_alpha), *out),
                            groups=groups, windowed=True)


def _ungrouped(w: PackedWeight, what: str) -> None:
    if w.groups != 1 or w.windowed:
        raise native.NativeError(f"bnn_amd: {what} takes a dense weight pack (pack_weight); this one is grouped "
                                 f"(groups={w.groups}, pack_weight_grouped): use bconv2d_grouped")


def conv_out_hw(H, W, KH, KW, stride, padding, dilation) -> Tuple[int, int]:
    sh, sw = _pair(stride)
    ph, pw = _pair(padding)
    dh, dw = _pair(dilation)
    return ((H + 2 * ph - dh * (KH - 1) - 1) // sh + 1, (W + 2 * pw - dw * (KW - 1) - 1) // sw + 1)


def _desc(act_shape, w_shape, stride, padding, dilation, flags) -> native.ConvDesc:
    N, C, H, W = act_shape
    O, C2, KH, KW = w_shape
    if C != C2:
        raise native.NativeError(f"bnn_amd: channel mismatch {C} vs {C2} (groups != 1 unsupported)")
    sh, sw = _pair(stride)
    ph, pw = _pair(padding)
    dh, dw = _pair(dilation)
    return native.ConvDesc(N, C, H, W, O, KH, KW, sh, sw, ph, pw, dh, dw, flags)


def _flags(w: PackedWeight, force_generic: bool, weights: Optional[str], a: Optional[PackedAct] = None,
           throughput: bool = False) -> int:
    f = (native.FLAG_FORCE_GENERIC if force_generic else 0) | \
        (native.FLAG_WEIGHT_ZEROS if w.has_zero else 0) | (native.FLAG_THROUGHPUT if throughput else 0)
    if a is not None and a.nonneg:
        f |= native.FLAG_ACT_NONNEG
    if weights == "sgpr":
        f |= native.FLAG_WEIGHTS_SGPR
    elif weights is not None:
        raise ValueError("weights must be None or 'sgpr' (the LDS-staged tile is test-only since ABI 12: "
                         "tests/helpers/legacy.py)")
    return f


def _conv_step(d: native.ConvDesc, stride, padding, dilation, c_total: Optional[int] = None) -> int:
    """``fused_launch_images`` of a descriptor: one launch addresses < 2^31 elements, a larger batch is split."""
    return fused_launch_images(d.N, d.C, d.H, d.W, d.O, (d.KH, d.KW), stride, padding, dilation, c_total)


def bconv2d(a: PackedAct, w: PackedWeight, bias: Optional[torch.Tensor] = None,
            post_scale: Optional[torch.Tensor] = None, stride=1, padding=0, dilation=1,
            force_generic: bool = False, raw_dot: bool = False,
            weights: Optional[str] = None) -> torch.Tensor:
    """Binary convolution on packed operands -> fp32 NCHW (or int32 dot when ``raw_dot``)."""
    _ungrouped(w, "bconv2d")
    lib = native.require()
    d = _desc(a.shape, w.shape, stride, padding, dilation, _flags(w, force_generic, weights, a))
    ho, wo = conv_out_hw(d.H, d.W, d.KH, d.KW, stride, padding, dilation)
    dev = a.P.device
    bias = _per_channel(bias, d.O, "bias")
    post_scale = _per_channel(post_scale, d.O, "post_scale")
    with torch.cuda.device(dev):
        out = torch.empty((d.N, d.O, ho, wo), dtype=torch.int32 if raw_dot else torch.float32,
                          device=dev)
        for n0, n1, dd in _desc_slices(d, _conv_step(d, stride, padding, dilation)):
            args = (ctypes.byref(dd), a.P[n0:n1].data_ptr(), a.M[n0:n1].data_ptr(),
                    w.wbits.data_ptr(), w.wnz.data_ptr())
            if raw_dot:
                st = lib.bnn_hip_bconv2d_dot(*args, out[n0:n1].data_ptr(), _stream(dev))
            else:
                st = lib.bnn_hip_bconv2d(*args, w.alpha.data_ptr(), _ptr(bias), _ptr(post_scale),
                                         out[n0:n1].data_ptr(), _stream(dev))
            native.check(st, "bnn_hip_bconv2d")
    return out


def _grouped_frame(a: PackedAct, w: PackedWeight, fn: str, stride, padding, dilation, bias, post_scale, prelu=None,
                   shuffle_groups=1):
    """What the three grouped wrappers (``fn``: which) share: ``(descriptor over all C input channels, (ho, wo), (bias,
    post_scale, prelu) checked per output channel, shuffle_groups validated)``."""
    if not w.windowed:
        raise native.NativeError(f"bnn_amd: {fn} reads the layout of pack_weight_grouped, not of pack_weight")
    N, C, H, W = a.shape
    O, Cg, KH, KW = w.shape
    if Cg * w.groups != C:
        raise native.NativeError(f"bnn_amd: grouped weight reads {Cg} x {w.groups} channels, the input has {C}")
    shuffle_groups = _shuffle_groups(shuffle_groups, O, "output channels")
    d = _desc(a.shape, (O, C, KH, KW), stride, padding, dilation, 0)
    consts = tuple(_per_channel(t, O, what) for t, what in ((bias, "bias"), (post_scale, "post_scale"), (prelu, "prelu")))
    return d, conv_out_hw(H, W, KH, KW, stride, padding, dilation), consts, shuffle_groups


def bconv2d_grouped(a: PackedAct, w: PackedWeight, bias: Optional[torch.Tensor] = None,
                    post_scale: Optional[torch.Tensor] = None, stride=1, padding=0, dilation=1,
                    raw_dot: bool = False) -> torch.Tensor:
    """Grouped / depthwise binary convolution on packed operands (``bnn_hip_bconv2d_grouped``): ``a`` holds all C input
    channels, ``w`` comes from ``pack_weight_grouped`` (any ``groups``, 1 included) -> fp32 NCHW, or the int32 dot when
    ``raw_dot``."""
    lib = native.require()
    d, (ho, wo), (bias, post_scale, _), _ = _grouped_frame(a, w, "bconv2d_grouped", stride, padding, dilation, bias,
                                                           post_scale)
    dev = a.P.device
    if raw_dot and (bias is not None or post_scale is not None):
        raise ValueError("raw_dot returns the integer dot: no bias / post_scale")
    with torch.cuda.device(dev):
        out = torch.empty((d.N, d.O, ho, wo), dtype=torch.int32 if raw_dot else torch.float32, device=dev)
        for n0, n1, dd in _desc_slices(d, _conv_step(d, stride, padding, dilation)):
            native.check(lib.bnn_hip_bconv2d_grouped(ctypes.byref(dd), w.groups, a.P[n0:n1].data_ptr(),
                                                     a.M[n0:n1].data_ptr(), w.wbits.data_ptr(), w.wnz.data_ptr(),
                                                     None if raw_dot else w.alpha.data_ptr(), _ptr(bias),
                                                     _ptr(post_scale), out[n0:n1].data_ptr(), _stream(dev)),
                         "bnn_hip_bconv2d_grouped")
    return out


def bconv2d_grouped_fused(a: PackedAct, w: PackedWeight, bias: Optional[torch.Tensor] = None,
                          post_scale: Optional[torch.Tensor] = None, stride=1, padding=0, dilation=1, *,
                          prelu: Optional[torch.Tensor] = None, shuffle_groups: int = 1,
                          residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``bconv2d_grouped`` with the rest of a BATS cell operation in the same launch
    (``bnn_hip_bconv2d_grouped_fused``): per-channel PReLU, ``channel_shuffle(., shuffle_groups)`` as the store index
    and the skip connection ``residual + .`` (fp32 ``[N, O, Ho, Wo]``) -> fp32 NCHW.  With none of the three it returns
    the bits of ``bconv2d_grouped``."""
    lib = native.require()
    d, (ho, wo), (bias, post_scale, prelu), shuffle_groups = _grouped_frame(
        a, w, "bconv2d_grouped_fused", stride, padding, dilation, bias, post_scale, prelu, shuffle_groups)
    dev = a.P.device
    residual = _shaped(residual, (d.N, d.O, ho, wo), "residual", "residual shape {got} != output")
    with torch.cuda.device(dev):
        out = torch.empty((d.N, d.O, ho, wo), dtype=torch.float32, device=dev)
        for n0, n1, dd in _desc_slices(d, _conv_step(d, stride, padding, dilation)):
            native.check(lib.bnn_hip_bconv2d_grouped_fused(
                ctypes.byref(dd), w.groups, a.P[n0:n1].data_ptr(), a.M[n0:n1].data_ptr(), w.wbits.data_ptr(),
                w.wnz.data_ptr(), w.alpha.data_ptr(), _ptr(bias), _ptr(post_scale), _ptr(prelu), shuffle_groups,
                None if residual is None else residual[n0:n1].data_ptr(), out[n0:n1].data_ptr(), _stream(dev)),
                "bnn_hip_bconv2d_grouped_fused")
    return out


def bconv2d_grouped_node(a: PackedAct, w: PackedWeight, bias: Optional[torch.Tensor] = None,
                         post_scale: Optional[torch.Tensor] = None, stride=1, padding=0, dilation=1, *,
                         prelu: Optional[torch.Tensor] = None, shuffle_groups: int = 1,
                         residual: Optional[torch.Tensor] = None, addend: Optional[torch.Tensor] = None,
                         out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``bconv2d_grouped_fused`` as one term of a cell node (``bnn_hip_bconv2d_grouped_node``):
    ``out = (residual + shuffle(prelu(conv))) + addend``, three roundings, a missing operand skipped.  ``residual``,
    ``addend`` and ``out`` are ``[N, O, Ho, Wo]`` and each may be a channel slice of a wider contiguous tensor
    (``channel_view``) — ``out`` typically the node's slice of the cell output, which makes ``torch.cat`` disappear.
    ``out`` may not share an element with an operand; slices of ONE tensor with disjoint channels are fine.  Returns
    ``out`` (a new tensor when not given)."""
    lib = native.require()
    d, (ho, wo), (bias, post_scale, prelu), shuffle_groups = _grouped_frame(
        a, w, "bconv2d_grouped_node", stride, padding, dilation, bias, post_scale, prelu, shuffle_groups)
    dev = a.P.device
    shape = (d.N, d.O, ho, wo)
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=dev)
        views = []
        for t, what in ((residual, "residual"), (addend, "addend"), (out, "out")):
            if t is not None and tuple(t.shape) != shape:
                raise native.NativeError(f"bnn_amd: {what} shape {tuple(t.shape)} != output {shape}")
            views.append(None if t is None else channel_view(t, what))
        if d.N == 0:
            return out
        c_max = max(v[2] for v in views if v is not None)

        def arg(v, n0, n1):
            if v is None:
                return None
            return native.F32View(v[0][n0:n1].data_ptr(), v[1], v[2])
        for n0, n1, dd in _desc_slices(d, _conv_step(d, stride, padding, dilation, c_max)):
            r, ad, o = (arg(v, n0, n1) for v in views)
            native.check(lib.bnn_hip_bconv2d_grouped_node(
                ctypes.byref(dd), w.groups, a.P[n0:n1].data_ptr(), a.M[n0:n1].data_ptr(), w.wbits.data_ptr(),
                w.wnz.data_ptr(), w.alpha.data_ptr(), _ptr(bias), _ptr(post_scale), _ptr(prelu), shuffle_groups,
                None if r is None else ctypes.byref(r), None if ad is None else ctypes.byref(ad), o.p, o.c_offset,
                o.c_total, _stream(dev)), "bnn_hip_bconv2d_grouped_node")
    return out


def _fconv_desc(N: int, C: int, H: int, W: int, K: int, stride: int, weight_zeros: bool = False) -> native.FconvDesc:
    return native.FconvDesc(N, C, H, W, K, stride, native.FLAG_WEIGHT_ZEROS if weight_zeros else 0, 0)


def fconv_supported(N: int, C: int, H: int, W: int, K: int, stride: int) -> bool:
    """Whether ``fconv_fused`` has a kernel for this geometry (``bnn_hip_fconv_supported``: ``K`` in 1 / 3 / 5 / 7,
    stride 1 or 2, ``K`` rows of the intermediate bit planes within a workgroup's LDS); asked per launch of a batch
    that ``fconv_fused`` would split."""
    lib = native.require()
    step = _fconv_launch_images(N, C, H, W, stride)
    return bool(lib.bnn_hip_fconv_supported(ctypes.byref(_fconv_desc(min(N, step) or 1, C, H, W, K, stride))))


def _fconv_launch_images(N: int, C: int, H: int, W: int, stride: int) -> int:
    ho, wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    return _launch_images(N, C, C, C, 2 * H * W * ((C + 63) // 64), ho * wo)


def fconv_fused(a: PackedAct, w1: PackedWeight, w2: PackedWeight, mid_scale: torch.Tensor, mid_shift: torch.Tensor, *,
                stride: int = 1, bias1=None, post_scale1=None, prelu1=None, bias2=None, post_scale2=None, prelu2=None,
                shuffle_groups: int = 1, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The BATS ``FactorizedConv`` behind its first BatchNorm in ONE launch (``bnn_hip_fconv_fused``): ``a`` holds
    ``sign(BatchNorm(x))``, ``w1`` / ``w2`` are the ``pack_weight`` of its ``[C, C, 1, K]`` and ``[C, C, K, 1]`` weights,
    ``mid_scale`` / ``mid_shift`` the folded BatchNorm between them; the rest per stage (``[C]`` each, optional).  The
    result ``[N, C, (H-1)//s + 1, (W-1)//s + 1]`` holds the bits of ``bconv2d_fused`` (1 x K, ``prelu1``,
    ``pack_scale`` / ``pack_shift``, planes only) -> ``bconv2d_fused`` (K x 1, ``prelu2``) -> ``channel_shuffle`` ->
    ``residual + .``; the tensor between the convolutions stays in LDS as bit planes.  ``NativeError`` where
    ``fconv_supported`` says no."""
    _ungrouped(w1, "fconv_fused")
    _ungrouped(w2, "fconv_fused")
    lib = native.require()
    N, C, H, W = a.shape
    K = w1.shape[3]
    if tuple(w1.shape) != (C, C, 1, K) or tuple(w2.shape) != (C, C, K, 1):
        raise native.NativeError(f"bnn_amd: fconv_fused takes [C, C, 1, K] and [C, C, K, 1] weights over the input's {C} "
                                 f"channels, got {tuple(w1.shape)} and {tuple(w2.shape)}")
    stride = int(stride)
    if stride < 1:
        raise native.NativeError(f"bnn_amd: stride={stride}")
    shuffle_groups = _shuffle_groups(shuffle_groups, C, "channels")
    ho, wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    dev = a.P.device
    mid_scale = _per_channel(mid_scale, C, "mid_scale")
    mid_shift = _per_channel(mid_shift, C, "mid_shift")
    consts = [[_per_channel(t, C, what) for t, what in ((b, "bias"), (s, "post_scale"), (p, "prelu"))]
              for b, s, p in ((bias1, post_scale1, prelu1), (bias2, post_scale2, prelu2))]
    stages = [native.FconvStage(w.alpha.data_ptr(), *map(_ptr, c)) for w, c in zip((w1, w2), consts)]
    residual = _shaped(residual, (N, C, ho, wo), "residual", "residual shape {got} != output")
    d = _fconv_desc(N, C, H, W, K, stride, w1.has_zero or w2.has_zero)
    with torch.cuda.device(dev):
        out = torch.empty((N, C, ho, wo), dtype=torch.float32, device=dev)
        for n0, n1, dd in _desc_slices(d, _fconv_launch_images(N, C, H, W, stride)):
            native.check(lib.bnn_hip_fconv_fused(
                ctypes.byref(dd), a.P[n0:n1].data_ptr(), a.M[n0:n1].data_ptr(), w1.wbits.data_ptr(), w1.wnz.data_ptr(),
                ctypes.byref(stages[0]), w2.wbits.data_ptr(), w2.wnz.data_ptr(), ctypes.byref(stages[1]),
                mid_scale.data_ptr(), mid_shift.data_ptr(), shuffle_groups,
                None if residual is None else residual[n0:n1].data_ptr(), out[n0:n1].data_ptr(), _stream(dev)),
                "bnn_hip_fconv_fused")
    return out


def direct_plan(x_shape, w: PackedWeight, stride=1, padding=0, dilation=1) -> Optional[native.FlyPlan]:
    """The band plan ``bconv2d_direct`` would use for this geometry, or None where the one-launch layer does not
    apply (include/bnn_hip.h: bnn_hip_bconv2d_direct_plan)."""
    lib = native.require()
    d = _desc(tuple(x_shape), w.shape, stride, padding, dilation, native.FLAG_WEIGHT_ZEROS if w.has_zero else 0)
    plan = native.FlyPlan()
    st = lib.bnn_hip_bconv2d_direct_plan(ctypes.byref(d), ctypes.byref(plan))
    if st == native.ERR_UNSUPPORTED:
        return None
    native.check(st, "bnn_hip_bconv2d_direct_plan")
    return plan


def _prefers_two_launches(d) -> bool:
    """Shapes where ``pack_act`` + ``bconv2d`` beats the one-launch kernel.  That kernel packs 64 consecutive pixels of
    a band per item: with 1 x 1 images (``Linear`` layers) an item holds ONE valid lane and its loads stride by a
    whole image — 1/64 lane utilisation.  Measured on MI355X (tools/bench_linear.py, us one-launch vs
    two launches): 1x1 images N=1024 C=512 49 vs 30, N=256 C=4096 450 vs 48, N=64 C=2048 69 vs 29, N=32768 C=256 105 vs
    85; 3x3 on 2x2 / 4x4 images 76 vs 30 / 77 vs 37 — but N=256 C=512 1x1 26 vs 31, 1x1 conv on 2x2 images 18 vs 29,
    3x3 on 7x7 30 vs 33: tiny images go the two-launch way when the kernel is larger than 1x1 or the input is wide or
    the batch large."""
    return d.H * d.W <= _DIRECT_MIN_PIXELS and (d.KH * d.KW > 1 or d.C >= 1024 or d.N * d.C >= (1 << 19))


def bconv2d_direct(x: torch.Tensor, w: PackedWeight, bias: Optional[torch.Tensor] = None,
                   post_scale: Optional[torch.Tensor] = None, stride=1, padding=0, dilation=1,
                   plan: Optional[native.FlyPlan] = None, force_generic: bool = False,
                   route: Optional[str] = None, out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """``Conv2d.forward`` of the reference (bnn/layers/conv.py:90-97) in ONE launch: fp32, fp16 or bf16 NCHW activations
    in, fp32 NCHW out, ``sign(x)`` computed on the fly inside the convolution kernel (csrc/bconv_fly.hip) — no packed
    copy of the activations in HBM.  Geometries the one-launch kernel does not cover (an output row with its halo
    larger than a CU's LDS) take ``pack_act`` + ``bconv2d``; the results are bit-identical either way.

    ``out_dtype`` (``torch.float16`` / ``torch.bfloat16``): the layer of a 16-bit network — a tensor of that type comes
    back, rounded where the reference rounds (``round_lowp``): by the kernel's own 16-bit store on the one-launch route
    (BNN_HIP_FLAG_OUT_*), by ``round_lowp`` on the fp32 result of the others.

    ``route``: ``None`` picks per shape (``_prefers_two_launches``); ``"direct"`` / ``"packed"`` force one (tools)."""
    if route not in (None, "direct", "packed"):
        raise ValueError("route must be None, 'direct' or 'packed'")
    _check_out_dtype(out_dtype)
    _ungrouped(w, "bconv2d_direct")
    x = _nchw(x, "activation", "bconv2d_direct", lowp=True)
    lib = native.require()
    d = _desc(tuple(x.shape), w.shape, stride, padding, dilation, _flags(w, force_generic, None))
    ho, wo = conv_out_hw(d.H, d.W, d.KH, d.KW, stride, padding, dilation)
    dev = x.device
    bias = _per_channel(bias, d.O, "bias")
    post_scale = _per_channel(post_scale, d.O, "post_scale")

    def two_launches(xs: torch.Tensor) -> torch.Tensor:
        if out_dtype is None:
            return bconv2d(pack_act(xs), w, bias, post_scale, stride, padding, dilation, force_generic=force_generic)
        return round_lowp(bconv2d(pack_act(xs), w, bias, None, stride, padding, dilation, force_generic=force_generic),
                          post_scale, out_dtype)

    if d.N and plan is None and (route == "packed" or (route is None and _prefers_two_launches(d))):
        return two_launches(x)
    if out_dtype is not None:
        d.flags |= _LOWP_OUT_FLAG[out_dtype]
    with torch.cuda.device(dev):
        out = torch.empty((d.N, d.O, ho, wo), dtype=out_dtype or torch.float32, device=dev)
        if d.N == 0:
            return out
        step = _launch_images(d.N, d.C, d.O, d.O, d.C * d.H * d.W, ho * wo)   # (the input is fp32 / 16-bit elements here)
        dtype = _act_dtype(x)
        for n0, n1, dd in _desc_slices(d, step):
            st = lib.bnn_hip_bconv2d_direct(ctypes.byref(dd), x[n0:n1].data_ptr(), dtype, w.wbits.data_ptr(),
                                            w.wnz.data_ptr(), w.alpha.data_ptr(), _ptr(bias), _ptr(post_scale),
                                            out[n0:n1].data_ptr(), None if plan is None else ctypes.byref(plan),
                                            _stream(dev))
            if st == native.ERR_UNSUPPORTED and plan is None:   # the two-launch form of the same layer
                out[n0:n1] = two_launches(x[n0:n1])
                continue
            native.check(st, "bnn_hip_bconv2d_direct")
    return out


def _fused_launches(a: PackedAct, w: PackedWeight, what: str, *, bias=None, post_scale=None, bn_scale=None,
                    bn_shift=None, residual=None, prelu=None, relu=False, out_f32=True,
                    out_packed=False, stride=1, padding=0, dilation=1, force_generic=False,
                    weights: Optional[str] = None, residual_after_act: bool = False,
                    pack_before_residual: bool = False, pack_scale=None, pack_shift=None,
                    pack_relu: bool = False, out: Optional[torch.Tensor] = None, out_c_offset: int = 0,
                    throughput: bool = False, sign_thresholds: Optional[torch.Tensor] = None,
                    shortcut: Optional[tuple] = None):
    """Everything ``bconv2d_fused`` does short of launching (shared with ``bconv2d_route``): checks the arguments,
    allocates the outputs and returns ``(y, pk, nonneg, launches)`` where ``launches`` yields one
    ``(descriptor, epilogue, n0, n1)`` per launch of the batch."""
    _ungrouped(w, what)
    d = _desc(a.shape, w.shape, stride, padding, dilation, _flags(w, force_generic, weights, a, throughput))
    ho, wo = conv_out_hw(d.H, d.W, d.KH, d.KW, stride, padding, dilation)
    dev = a.P.device
    bias = _per_channel(bias, d.O, "bias")
    post_scale = _per_channel(post_scale, d.O, "post_scale")
    bn_scale = _per_channel(bn_scale, d.O, "bn_scale")
    bn_shift = _per_channel(bn_shift, d.O, "bn_shift")
    prelu = _per_channel(prelu, d.O, "prelu")
    pack_scale = _per_channel(pack_scale, d.O, "pack_scale")
    pack_shift = _per_channel(pack_shift, d.O, "pack_shift")
    c_total = d.O
    if out is not None:
        wrong = "`out` must be a contiguous fp32 [N, C_total, Ho, Wo] tensor with room for O channels at out_c_offset"
        if out.dim() != 4 or not 0 <= out_c_offset <= out.shape[1] - d.O:
            raise native.NativeError("bnn_amd: " + wrong)
        c_total = out.shape[1]
        _written(out, (d.N, c_total, ho, wo), "out", wrong)
    residual = _shaped(residual, (d.N, c_total, ho, wo), "residual", "residual shape {got} != output")
    sc_in_hw = 0
    if shortcut is not None:
        sa, sw, sbn_a, sbn_b = shortcut
        # the shortcut planes at the output resolution, or UN-POOLED at twice it (the kernel ORs the 2 x 2 windows)
        pooled = tuple(sa.shape) == (d.N, sw.shape[1], ho, wo)
        unpooled = (sa.shape[0] == d.N and sa.shape[1] == sw.shape[1] and (sa.shape[2] + 1) // 2 == ho
                    and (sa.shape[3] + 1) // 2 == wo and max(sa.shape[2], sa.shape[3]) < 65536)
        if residual is not None or not sa.nonneg or not (pooled or unpooled) \
                or tuple(sw.shape) != (d.O, sa.shape[1], 1, 1) or sw.has_zero:
            raise native.NativeError("bnn_amd: folded shortcut: a non-negative packed [N, C, Ho, Wo] (or un-pooled "
                                     "[N, C, ~2 Ho, ~2 Wo]) input, a 1x1 [O, C, 1, 1] weight without zeros, and no "
                                     "separate residual")
        if not pooled:
            sc_in_hw = (sa.shape[2] << 16) | sa.shape[3]
        sbn_a = _per_channel(sbn_a, d.O, "shortcut bn_scale")
        sbn_b = _per_channel(sbn_b, d.O, "shortcut bn_shift")
    eflags = (native.EPI_RES_AFTER_ACT if residual_after_act else 0) | \
        (native.EPI_PACK_BEFORE_RES if pack_before_residual else 0) | (native.EPI_PACK_RELU if pack_relu else 0)
    with torch.cuda.device(dev):
        y = out if out is not None else (
            torch.empty((d.N, d.O, ho, wo), dtype=torch.float32, device=dev) if out_f32 else None)
        pk = empty_packed(d.N, d.O, ho, wo, dev) if out_packed else None
    step = _conv_step(d, stride, padding, dilation, c_total)

    def launches():
        for n0, n1, dd in _desc_slices(d, step):
            e = native.Epilogue(
                alpha=w.alpha.data_ptr(), bias=_ptr(bias), post_scale=_ptr(post_scale), bn_scale=_ptr(bn_scale),
                bn_shift=_ptr(bn_shift), residual=None if residual is None else residual[n0:n1].data_ptr(),
                prelu=_ptr(prelu), relu=int(bool(relu)), flags=eflags, out_f32=None if y is None else y[n0:n1].data_ptr(),
                out_P=None if pk is None else pk.P[n0:n1].data_ptr(), out_M=None if pk is None else pk.M[n0:n1].data_ptr(),
                pack_scale=_ptr(pack_scale), pack_shift=_ptr(pack_shift),
                out_c_offset=out_c_offset if out is not None else 0, out_c_total=c_total if out is not None else 0,
                sign_thresholds=_ptr(sign_thresholds))
            if shortcut is not None:
                e.sc_P, e.sc_wbits, e.sc_alpha = sa.P[n0:n1].data_ptr(), sw.wbits.data_ptr(), sw.alpha.data_ptr()
                e.sc_bn_scale, e.sc_bn_shift, e.sc_C, e.sc_in_hw = sbn_a.data_ptr(), sbn_b.data_ptr(), sa.shape[1], sc_in_hw
            yield dd, e, n0, n1

    # mirrors the kernel's rule for leaving the M plane at zero
    late = residual is not None and residual_after_act
    nonneg = bool(pack_relu) or (bool(relu) and prelu is None and pack_scale is None
                                 and (not late or pack_before_residual))
    return y, pk, nonneg, launches()


def _run_fused(symbol: str, a: PackedAct, w: PackedWeight, weight_ptrs: tuple, what: str, **kw):
    """The launches of the fused convolution ``symbol`` for the wrapper ``what``: ``_fused_launches``, then per launch
    ``symbol(descriptor, planes of a, *weight_ptrs, epilogue, stream)``, and the ``nonneg`` mark on the output planes."""
    fn = getattr(native.require(), symbol)
    y, pk, nonneg, launches = _fused_launches(a, w, what, **kw)
    dev = a.P.device
    with torch.cuda.device(dev):
        for dd, e, n0, n1 in launches:
            native.check(fn(ctypes.byref(dd), a.P[n0:n1].data_ptr(), a.M[n0:n1].data_ptr(), *weight_ptrs, ctypes.byref(e),
                            _stream(dev)), symbol)
    if pk is not None:
        pk.nonneg = nonneg
    return y, pk


def bconv2d_fused(a: PackedAct, w: PackedWeight, **kw):
    """Binary convolution + fused epilogue (see ``bnn_hip_epilogue``): returns
    ``(y_fp32 | None, PackedAct(sign(p)) | None)``.

    Keyword arguments (all optional): ``bias, post_scale, bn_scale, bn_shift, residual, prelu, relu=False, out_f32=True,
    out_packed=False, stride=1, padding=0, dilation=1, force_generic=False, weights=None, residual_after_act=False,
    pack_before_residual=False, pack_scale, pack_shift, pack_relu=False, out, out_c_offset=0, throughput=False,
    sign_thresholds, shortcut``.

    ``shortcut = (PackedAct, PackedWeight, bn_scale, bn_shift)``: the down-sampling block's shortcut branch folded into
    this launch (``bnn_hip_epilogue.sc_*``): the residual is ``BN(conv1x1(packed))`` computed in the kernel instead of
    an fp32 tensor; see ``shortcut_fold_supported``.

    ``out``: write the fp32 result into channels ``[out_c_offset, out_c_offset + O)`` of this
    preallocated ``[N, C_total, Ho, Wo]`` tensor (``torch.cat`` in place); ``residual`` then has
    ``C_total`` channels too.  The remaining keyword arguments are the pre-activation switches of
    ``BNN_HIP_EPI_*`` (include/bnn_hip.h); ``throughput``: ``BNN_HIP_FLAG_THROUGHPUT`` (several batches in flight)."""
    return _run_fused("bnn_hip_bconv2d_fused", a, w, (w.wbits.data_ptr(), w.wnz.data_ptr()), "bconv2d_fused", **kw)


def _mfma_pack(w: PackedWeight, kind: str, dims: tuple, *operands) -> Optional[torch.Tensor]:
    """The matrix-core form ``kind`` of a packed weight: ``None`` for a grouped or windowed pack and where
    ``bnn_hip_<kind>_bytes(*dims)`` is 0, else an int8 tensor of that size filled by ``bnn_hip_pack_<kind>(*operands, it)``."""
    lib = native.require()
    if w.windowed or w.groups != 1:
        return None
    nbytes = int(getattr(lib, f"bnn_hip_{kind}_bytes")(*dims))
    if nbytes == 0:
        return None
    dev = w.wbits.device
    with torch.cuda.device(dev):
        pack = torch.empty(nbytes, dtype=torch.int8, device=dev)
        native.check(getattr(lib, f"bnn_hip_pack_{kind}")(*operands, pack.data_ptr(), _stream(dev)), f"bnn_hip_pack_{kind}")
    return pack


def pack_weight_i8(w: PackedWeight) -> Optional[torch.Tensor]:
    """The int8 MFMA-fragment form of a packed 3x3 weight (``bnn_hip_pack_weight_i8``, layout: include/bnn_hip.h), or
    ``None`` where there is none (not 3x3, C or O no multiple of 64, a grouped pack).  One launch; ``w.alpha`` is used
    unchanged beside it."""
    return _mfma_pack(w, "weight_i8", w.shape, w.wbits.data_ptr(), w.wnz.data_ptr(), *w.shape)


def pack_weight_f4(w: PackedWeight) -> Optional[torch.Tensor]:
    """The FP4 (E2M1) MFMA-fragment form of a packed 3x3 weight (``bnn_hip_pack_weight_f4``, layout: include/bnn_hip.h):
    half the bytes of ``pack_weight_i8``, as an int8 tensor of nibble pairs.  ``None`` where there is none (as
    ``pack_weight_i8``, or C no multiple of 128)."""
    return _mfma_pack(w, "weight_f4", w.shape, w.wbits.data_ptr(), w.wnz.data_ptr(), *w.shape)


def bconv2d_mfma_supported(a_shape, w: PackedWeight, *, nonneg: bool = False, bias=False, post_scale=False, bn=False,
                           residual=False, prelu=False, relu=False, out_f32=True, out_packed=False, stride=1, padding=0,
                           dilation=1, sign_thresholds=False, shortcut=False, epi_flags: int = 0, pack_affine=False,
                           out_c_total: int = 0) -> bool:
    """Whether ``bconv2d_mfma_fused`` takes a launch of this geometry and epilogue (``bnn_hip_bconv2d_mfma_supported``:
    host only, nothing is launched or allocated).  The epilogue is given by what it contains (truth values), not by
    tensors: an aligned stand-in pointer takes the place of each operand that is present."""
    return _mfma_supported("bnn_hip_bconv2d_mfma_supported", a_shape, w, dict(
        nonneg=nonneg, bias=bias, post_scale=post_scale, bn=bn, residual=residual, prelu=prelu, relu=relu, out_f32=out_f32,
        out_packed=out_packed, stride=stride, padding=padding, dilation=dilation, sign_thresholds=sign_thresholds,
        shortcut=shortcut, epi_flags=epi_flags, pack_affine=pack_affine, out_c_total=out_c_total))


def _mfma_supported(symbol: str, a_shape, w: PackedWeight, k: dict) -> bool:    # k: every keyword of the public queries
    lib = native.require()
    if w.windowed or w.groups != 1:
        return False
    d = _desc(tuple(a_shape), w.shape, k["stride"], k["padding"], k["dilation"], native.FLAG_ACT_NONNEG if k["nonneg"] else 0)
    p = 0x10000   # never dereferenced
    on = lambda name: p if k[name] else None
    sc = on("shortcut")
    e = native.Epilogue(alpha=p, bias=on("bias"), post_scale=on("post_scale"), bn_scale=on("bn"), bn_shift=on("bn"),
                        residual=on("residual"), prelu=on("prelu"), relu=int(bool(k["relu"])), flags=k["epi_flags"],
                        out_f32=on("out_f32"), out_P=on("out_packed"), out_M=on("out_packed"), pack_scale=on("pack_affine"),
                        pack_shift=on("pack_affine"), out_c_total=k["out_c_total"], sign_thresholds=on("sign_thresholds"),
                        sc_P=sc, sc_wbits=sc, sc_alpha=sc, sc_bn_scale=sc, sc_bn_shift=sc, sc_C=64 if sc else 0)
    return bool(getattr(lib, symbol)(ctypes.byref(d), ctypes.byref(e)))


def bconv2d_mfma4_supported(a_shape, w: PackedWeight, *, nonneg: bool = False, bias=False, post_scale=False, bn=False,
                            residual=False, prelu=False, relu=False, out_f32=True, out_packed=False, stride=1, padding=0,
                            dilation=1, sign_thresholds=False, shortcut=False, epi_flags: int = 0, pack_affine=False,
                            out_c_total: int = 0) -> bool:
    """``bconv2d_mfma_supported`` for the FP4 form (``bnn_hip_bconv2d_mfma4_supported``): the same rule plus whole
    128-channel groups."""
    return _mfma_supported("bnn_hip_bconv2d_mfma4_supported", a_shape, w, dict(
        nonneg=nonneg, bias=bias, post_scale=post_scale, bn=bn, residual=residual, prelu=prelu, relu=relu, out_f32=out_f32,
        out_packed=out_packed, stride=stride, padding=padding, dilation=dilation, sign_thresholds=sign_thresholds,
        shortcut=shortcut, epi_flags=epi_flags, pack_affine=pack_affine, out_c_total=out_c_total))


def bconv2d_mfma_fused(a: PackedAct, w: PackedWeight, w8: torch.Tensor, **kw):
    """``bconv2d_fused`` with the dot on ``v_mfma_i32_16x16x64_i8`` (``bnn_hip_bconv2d_mfma_fused``): same arguments, same
    bits.  ``w8 = pack_weight_i8(w)``.  Raises where ``bconv2d_mfma_supported`` says no."""
    w8 = _opaque(w8, native.require().bnn_hip_weight_i8_bytes(*w.shape), "w8", torch.int8)
    return _run_fused("bnn_hip_bconv2d_mfma_fused", a, w, (w8.data_ptr(),), "bconv2d_mfma_fused", **kw)


def bconv2d_mfma4_fused(a: PackedAct, w: PackedWeight, w4: torch.Tensor, **kw):
    """``bconv2d_mfma_fused`` with the dot on ``v_mfma_f32_16x16x128_f8f6f4`` and FP4 operands
    (``bnn_hip_bconv2d_mfma4_fused``): same arguments, same bits.  ``w4 = pack_weight_f4(w)``.  Raises where
    ``bconv2d_mfma4_supported`` says no."""
    w4 = _opaque(w4, native.require().bnn_hip_weight_f4_bytes(*w.shape), "w4", torch.int8)
    return _run_fused("bnn_hip_bconv2d_mfma4_fused", a, w, (w4.data_ptr(),), "bconv2d_mfma4_fused", **kw)


def pack_weight1x1_f4(w: PackedWeight) -> Optional[torch.Tensor]:
    """The FP4 (E2M1) MFMA-fragment form of a packed 1x1 weight (``bnn_hip_pack_weight1x1_f4``, layout: include/bnn_hip.h:
    ``pack_weight_f4``'s with one tap), as an int8 tensor of nibble pairs.  ``None`` where there is none (not 1x1, O no
    multiple of 64, C no multiple of 128, a grouped pack).  One launch; ``w.alpha`` is used unchanged beside it."""
    if tuple(w.shape[2:]) != (1, 1):
        return None
    return _mfma_pack(w, "weight1x1_f4", w.shape[:2], w.wbits.data_ptr(), w.wnz.data_ptr(), *w.shape)


def bconv1x1_mfma4_supported(a_shape, w: PackedWeight, *, nonneg: bool = False, bias=False, post_scale=False, bn=False,
                             residual=False, prelu=False, relu=False, out_f32=True, out_packed=False, stride=1, padding=0,
                             dilation=1, sign_thresholds=False, shortcut=False, epi_flags: int = 0, pack_affine=False,
                             out_c_total: int = 0) -> bool:
    """``bconv2d_mfma_supported`` for the 1x1 convolution on the FP4 matrix cores (``bnn_hip_bconv1x1_mfma4_supported``):
    1x1 / stride 1 / padding 0, C % 128 == 0, O % 64 == 0, every epilogue of ``bconv2d_fused`` but the folded shortcut
    and a channel window."""
    return _mfma_supported("bnn_hip_bconv1x1_mfma4_supported", a_shape, w, dict(
        nonneg=nonneg, bias=bias, post_scale=post_scale, bn=bn, residual=residual, prelu=prelu, relu=relu, out_f32=out_f32,
        out_packed=out_packed, stride=stride, padding=padding, dilation=dilation, sign_thresholds=sign_thresholds,
        shortcut=shortcut, epi_flags=epi_flags, pack_affine=pack_affine, out_c_total=out_c_total))


def bconv1x1_mfma4_fused(a: PackedAct, w: PackedWeight, w4: torch.Tensor, **kw):
    """``bconv2d_fused`` for a 1x1 weight with the dot on ``v_mfma_f32_16x16x128_f8f6f4`` and FP4 operands
    (``bnn_hip_bconv1x1_mfma4_fused``): same arguments — the pre-activation switches included — same bits.
    ``w4 = pack_weight1x1_f4(w)``.  Raises where ``bconv1x1_mfma4_supported`` says no."""
    w4 = _opaque(w4, native.require().bnn_hip_weight1x1_f4_bytes(w.shape[0], w.shape[1]), "w4", torch.int8)
    return _run_fused("bnn_hip_bconv1x1_mfma4_fused", a, w, (w4.data_ptr(),), "bconv1x1_mfma4_fused", **kw)


def pack_shortcut_weight_i8(sw: PackedWeight) -> Optional[torch.Tensor]:
    """The int8 MFMA-fragment form of a shortcut's packed 1x1 weight (``bnn_hip_pack_shortcut_weight_i8``, layout:
    include/bnn_hip.h), or ``None`` where there is none (not 1x1, zero weights, O no multiple of 64, C not 64 / 128 / 256,
    a grouped pack).  One launch; ``sw.alpha`` is used unchanged beside it."""
    if sw.has_zero or tuple(sw.shape[2:]) != (1, 1):
        return None
    return _mfma_pack(sw, "shortcut_weight_i8", sw.shape[:2], sw.wbits.data_ptr(), *sw.shape[:2])


def bconv2d_mfma_fold_supported(a_shape, w: PackedWeight, sc_channels: int, *, nonneg: bool = True, stride=1, padding=1,
                                dilation=1, unpooled_hw: Optional[Tuple[int, int]] = None, throughput: bool = False) -> bool:
    """Whether ``bconv2d_mfma_fold_fused`` takes this convolution with a folded shortcut of ``sc_channels`` input channels
    (``bnn_hip_bconv2d_mfma_fold_supported``: host only).  The epilogue is the one the fold belongs to: BatchNorm +
    shortcut + ReLU -> fp32 + sign planes.  ``unpooled_hw``: the shortcut plane comes un-pooled at this size."""
    return _mfma_fold_supported("bnn_hip_bconv2d_mfma_fold_supported", a_shape, w, sc_channels, dict(
        nonneg=nonneg, stride=stride, padding=padding, dilation=dilation, unpooled_hw=unpooled_hw, throughput=throughput))


def _mfma_fold_supported(symbol: str, a_shape, w: PackedWeight, sc_channels: int, k: dict) -> bool:
    lib = native.require()
    if w.windowed or w.groups != 1:
        return False
    flags = (native.FLAG_ACT_NONNEG if k["nonneg"] else 0) | (native.FLAG_WEIGHT_ZEROS if w.has_zero else 0) | \
        (native.FLAG_THROUGHPUT if k["throughput"] else 0)
    d = _desc(tuple(a_shape), w.shape, k["stride"], k["padding"], k["dilation"], flags)
    p = 0x10000   # never dereferenced
    hw = 0 if k["unpooled_hw"] is None else (int(k["unpooled_hw"][0]) << 16) | int(k["unpooled_hw"][1])
    e = native.Epilogue(alpha=p, bn_scale=p, bn_shift=p, relu=1, out_f32=p, out_P=p, out_M=p, sc_P=p, sc_alpha=p,
                        sc_bn_scale=p, sc_bn_shift=p, sc_C=int(sc_channels), sc_in_hw=hw)
    return bool(getattr(lib, symbol)(ctypes.byref(d), ctypes.byref(e)))


def bconv2d_mfma4_fold_supported(a_shape, w: PackedWeight, sc_channels: int, *, nonneg: bool = True, stride=1, padding=1,
                                 dilation=1, unpooled_hw: Optional[Tuple[int, int]] = None, throughput: bool = False) -> bool:
    """``bconv2d_mfma_fold_supported`` for the FP4 form (``bnn_hip_bconv2d_mfma4_fold_supported``): the same rule plus
    whole 128-channel groups."""
    return _mfma_fold_supported("bnn_hip_bconv2d_mfma4_fold_supported", a_shape, w, sc_channels, dict(
        nonneg=nonneg, stride=stride, padding=padding, dilation=dilation, unpooled_hw=unpooled_hw, throughput=throughput))


def _mfma_fold_fused(kind: str, what: str, a: PackedAct, w: PackedWeight, pack: torch.Tensor, sc_w8: torch.Tensor, **kw):
    lib = native.require()
    if kw.get("shortcut") is None:
        raise native.NativeError(f"bnn_amd: {what} needs shortcut=(PackedAct, PackedWeight, bn_a, bn_b)")
    name = "w8" if kind == "i8" else "w4"
    pack = _opaque(pack, getattr(lib, f"bnn_hip_weight_{kind}_bytes")(*w.shape), name, torch.int8)
    sc_w8 = _opaque(sc_w8, lib.bnn_hip_shortcut_weight_i8_bytes(*kw["shortcut"][1].shape[:2]), "sc_w8", torch.int8)
    symbol = "bnn_hip_bconv2d_mfma_fold_fused" if kind == "i8" else "bnn_hip_bconv2d_mfma4_fold_fused"
    return _run_fused(symbol, a, w, (pack.data_ptr(), sc_w8.data_ptr()), what, **kw)


def bconv2d_mfma_fold_fused(a: PackedAct, w: PackedWeight, w8: torch.Tensor, sc_w8: torch.Tensor, **kw):
    """``bconv2d_fused(a, w, ..., shortcut=(sa, sw, bn_a, bn_b))`` with both dots on ``v_mfma_i32_16x16x64_i8``
    (``bnn_hip_bconv2d_mfma_fold_fused``): same arguments, same bits.  ``w8 = pack_weight_i8(w)``,
    ``sc_w8 = pack_shortcut_weight_i8(sw)``.  Raises where ``bconv2d_mfma_fold_supported`` says no."""
    return _mfma_fold_fused("i8", "bconv2d_mfma_fold_fused", a, w, w8, sc_w8, **kw)


def bconv2d_mfma4_fold_fused(a: PackedAct, w: PackedWeight, w4: torch.Tensor, sc_w8: torch.Tensor, **kw):
    """``bconv2d_mfma_fold_fused`` with the 3x3 dot on FP4 operands (``bnn_hip_bconv2d_mfma4_fold_fused``; the shortcut's
    1x1 dot stays on the int8 instruction): same arguments, same bits.  ``w4 = pack_weight_f4(w)``,
    ``sc_w8 = pack_shortcut_weight_i8(sw)``.  Raises where ``bconv2d_mfma4_fold_supported`` says no."""
    return _mfma_fold_fused("f4", "bconv2d_mfma4_fold_fused", a, w, w4, sc_w8, **kw)


def bconv2d_route(a: PackedAct, w: PackedWeight, *, fused: bool = True, raw_dot: bool = False, **kw) -> dict:
    """Which kernel ``bconv2d_fused(a, w, **kw)`` runs (``bnn_hip_bconv2d_route``: the launch ladder itself answers,
    nothing is launched) as a dict of the fields of ``bnn_hip_conv_route``; of the first launch when the batch is split.
    ``fused=False``: of ``bconv2d(a, w, **kw)`` instead (``bias, post_scale, stride, padding, dilation, force_generic,
    raw_dot, weights``)."""
    lib = native.require()
    r = native.ConvRoute()
    if fused:
        if raw_dot:
            raise ValueError("raw_dot belongs to bconv2d: fused=False")
        _, _, _, launches = _fused_launches(a, w, "bconv2d_route", **kw)
        dd, e, _, _ = next(launches)
        native.check(lib.bnn_hip_bconv2d_route(ctypes.byref(dd), ctypes.byref(e), ctypes.byref(r)), "bnn_hip_bconv2d_route")
        return r.as_dict()
    _ungrouped(w, "bconv2d_route")
    kw.pop("bias", None), kw.pop("post_scale", None)      # (the drop-in kernel takes them or not: one route)
    d = _desc(a.shape, w.shape, kw.pop("stride", 1), kw.pop("padding", 0), kw.pop("dilation", 1),
              _flags(w, kw.pop("force_generic", False), kw.pop("weights", None), a))
    if kw:
        raise TypeError(f"bconv2d_route(fused=False): unexpected arguments {sorted(kw)}")
    if raw_dot:
        native.check(lib.bnn_hip_bconv2d_dot_route(ctypes.byref(d), ctypes.byref(r)), "bnn_hip_bconv2d_dot_route")
    else:
        native.check(lib.bnn_hip_bconv2d_route(ctypes.byref(d), None, ctypes.byref(r)), "bnn_hip_bconv2d_route")
    return r.as_dict()


@dataclass
class HBlockPack:
    """Derived data of one hierarchical block for ``hblock_forward`` (include/bnn_hip.h: bnn_hip_hblock_forward): the
    three weight packs in the kernel's dense layout and ONE constants buffer (alphas, folded bn2 / bn3, the next
    block's folded bn1)."""
    weights: torch.Tensor     # int32 [weight_words]
    consts: torch.Tensor      # float32 [const_floats]
    c_in: int
    planes: int
    has_next: bool
    packs: tuple = ()                              # the three standard packs (kept for the other weight order)
    weights_cl: Optional[torch.Tensor] = None      # the same weights in the channel-lane kernel's order (made on first use)

    def channel_lane_weights(self) -> torch.Tensor:
        if self.weights_cl is None:
            lib = native.require()
            w1, w2, w3 = self.packs
            dev = self.weights.device
            with torch.cuda.device(dev):
                buf = torch.empty_like(self.weights)
                native.check(lib.bnn_hip_hblock_pack_weights_cl(self.c_in, self.planes, w1.wbits.data_ptr(), w2.wbits.data_ptr(),
                                                                w3.wbits.data_ptr(), buf.data_ptr(), _stream(dev)),
                             "bnn_hip_hblock_pack_weights_cl")
            self.weights_cl = buf
        return self.weights_cl


def hblock_pack(w1: PackedWeight, w2: PackedWeight, w3: PackedWeight, bn2, bn3, next_bn=None) -> HBlockPack:
    """``w1..w3``: standard packs of the block's three 3x3 convolutions (no zero weights); ``bn2`` / ``bn3`` /
    ``next_bn``: (scale, shift) of the folded BatchNorms in front of conv2 / conv3 / the NEXT block's conv1."""
    lib = native.require()
    planes, c_in = 2 * w1.shape[0], w1.shape[1]
    if (w1.has_zero or w2.has_zero or w3.has_zero or tuple(w1.shape[2:]) != (3, 3)
            or tuple(w2.shape) != (planes // 4, planes // 2, 3, 3) or tuple(w3.shape) != (planes // 4, planes // 4, 3, 3)):
        raise native.NativeError("bnn_amd: hblock_pack expects the three 3x3 packs of an HBlock without zero weights")
    L = native.HBlockLayout()
    native.check(lib.bnn_hip_hblock_layout_of(c_in, planes, ctypes.byref(L)), "bnn_hip_hblock_layout_of")
    dev = w1.wbits.device
    with torch.cuda.device(dev):
        wbuf = torch.empty(int(L.weight_words), dtype=torch.int32, device=dev)
        native.check(lib.bnn_hip_hblock_pack_weights(c_in, planes, w1.wbits.data_ptr(), w2.wbits.data_ptr(),
                                                     w3.wbits.data_ptr(), wbuf.data_ptr(), _stream(dev)),
                     "bnn_hip_hblock_pack_weights")
        consts = torch.zeros(int(L.const_floats), dtype=torch.float32, device=dev)
        for k, w in enumerate((w1, w2, w3)):
            consts[L.alpha_off[k]:L.alpha_off[k] + w.shape[0]] = w.alpha[:w.shape[0]]
        for k, bn in enumerate((bn2, bn3)):
            n = (planes // 2, planes // 4)[k]
            consts[L.pack_a_off[k]:L.pack_a_off[k] + n] = _per_channel(bn[0], n, "bn scale")
            consts[L.pack_b_off[k]:L.pack_b_off[k] + n] = _per_channel(bn[1], n, "bn shift")
        if next_bn is not None:
            consts[L.next_a_off:L.next_a_off + planes] = _per_channel(next_bn[0], planes, "next bn scale")
            consts[L.next_b_off:L.next_b_off + planes] = _per_channel(next_bn[1], planes, "next bn shift")
    return HBlockPack(wbuf, consts, c_in, planes, next_bn is not None, (w1, w2, w3))


def _hblock_desc(N, c_in, H, W, planes, throughput=False, rows_per_band=0, images_per_band=0, waves=0, channel_lanes=False):
    flags = (native.FLAG_THROUGHPUT if throughput else 0) | (native.HBLOCK_CHANNEL_LANES if channel_lanes else 0)
    return native.HBlockDesc(N, c_in, H, W, planes, flags, rows_per_band, images_per_band, waves, 0)


def _hblock_query(symbol: str, *geometry_and_plan) -> bool:
    """One of the ``bnn_hip_hblock_*_supported`` questions for ``_hblock_desc(*geometry_and_plan)``."""
    return bool(getattr(native.require(), symbol)(ctypes.byref(_hblock_desc(*geometry_and_plan))))


def _hblock_launch(pack: "HBlockPack", a: PackedAct, throughput, rows_per_band, images_per_band, waves, channel_lanes=False):
    """``(descriptor, weight buffer)`` of a launch on planes ``a``: the channel-lane kernels read their own weight order."""
    N, c_in, H, W = a.shape
    d = _hblock_desc(N, c_in, H, W, pack.planes, throughput, rows_per_band, images_per_band, waves, channel_lanes)
    return d, (pack.channel_lane_weights() if channel_lanes else pack.weights)


def _nonneg_planes(N: int, C: int, H: int, W: int, dev) -> PackedAct:
    """Planes a kernel fills for a non-negative tensor: a fresh P, and the shared all-zero M it never writes."""
    shp = (N, C // 64, H, W)
    return PackedAct(torch.empty(shp, dtype=torch.int64, device=dev), _zero_plane(shp, dev), (N, C, H, W), nonneg=True)


def hblock_supported(N: int, c_in: int, H: int, W: int, planes: int, throughput: bool = False, rows_per_band: int = 0,
                     images_per_band: int = 0, waves: int = 0, channel_lanes: bool = False) -> bool:
    """Whether ``hblock_forward`` covers this geometry (with this plan) on the current device.  ``channel_lanes``: the
    small-image form of the kernel (csrc/hblock_cl.hip: 14 x 14 / 7 x 7, lanes = output channels)."""
    return _hblock_query("bnn_hip_hblock_supported", N, c_in, H, W, planes, throughput, rows_per_band, images_per_band, waves,
                         channel_lanes)


def hblock_forward(a: PackedAct, pack: HBlockPack, residual: torch.Tensor, out_packed: bool = True,
                   throughput: bool = False, rows_per_band: int = 0, images_per_band: int = 0, waves: int = 0,
                   channel_lanes: bool = False):
    """``HBlock.forward`` behind its first BatchNorm + ReLU (bnn/models/layers/hierarchical_block.py:38-60) in ONE
    launch: ``a`` = planes of ``sign(relu(bn1(x)))`` (non-negative), ``residual`` = the shortcut (fp32 NCHW).
    Returns ``(y, PackedAct(sign(relu(next_bn(y)))) | None)``."""
    lib = native.require()
    N, c_in, H, W = a.shape
    if not a.nonneg or c_in != pack.c_in:
        raise native.NativeError("bnn_amd: hblock_forward needs non-negative input planes of the block's width")
    residual = _shaped(residual, (N, pack.planes, H, W), "residual", "residual shape {got} != block output")
    if out_packed and not pack.has_next:
        raise native.NativeError("bnn_amd: this HBlockPack holds no next-block BatchNorm")
    dev = a.P.device
    with torch.cuda.device(dev):
        y = torch.empty_like(residual)
        pk = _nonneg_planes(N, pack.planes, H, W, dev) if out_packed else None
        if N == 0:
            return y, pk
        d, wbuf = _hblock_launch(pack, a, throughput, rows_per_band, images_per_band, waves, channel_lanes)
        native.check(lib.bnn_hip_hblock_forward(ctypes.byref(d), a.P.data_ptr(), wbuf.data_ptr(),
                                                pack.consts.data_ptr(), residual.data_ptr(), y.data_ptr(),
                                                None if pk is None else pk.P.data_ptr(), _stream(dev)),
                     "bnn_hip_hblock_forward")
    return y, pk


def hblock_shortcut_supported(N: int, c_in: int, H: int, W: int, planes: int, throughput: bool = False, rows_per_band: int = 0,
                              images_per_band: int = 0, waves: int = 0, channel_lanes: bool = False) -> bool:
    """Whether ``hblock_shortcut_forward`` covers this geometry (with this plan) on the current device."""
    return _hblock_query("bnn_hip_hblock_shortcut_supported", N, c_in, H, W, planes, throughput, rows_per_band,
                         images_per_band, waves, channel_lanes)


def hblock_shortcut_pack(w: PackedWeight):
    """``(weights [planes][C_in / 32] int32, alpha [planes])`` of a block's 1x1 shortcut convolution for
    ``hblock_shortcut_forward`` (no zero weights)."""
    lib = native.require()
    planes, c_in = w.shape[0], w.shape[1]
    if w.has_zero or tuple(w.shape[2:]) != (1, 1) or c_in % 64:
        raise native.NativeError("bnn_amd: hblock_shortcut_pack expects the pack of a 1x1 convolution without zero weights")
    dev = w.wbits.device
    with torch.cuda.device(dev):
        buf = torch.empty(planes * (c_in // 32), dtype=torch.int32, device=dev)
        native.check(lib.bnn_hip_hblock_pack_shortcut_weights(c_in, planes, w.wbits.data_ptr(), buf.data_ptr(), _stream(dev)),
                     "bnn_hip_hblock_pack_shortcut_weights")
        alpha = w.alpha[:planes].contiguous().clone()
    return buf, alpha


def hblock_shortcut_forward(a: PackedAct, pack: HBlockPack, sc: PackedAct, sc_pack, throughput: bool = False,
                            rows_per_band: int = 0, images_per_band: int = 0, waves: int = 0, channel_lanes: bool = False):
    """The first hierarchical block of a stage with its shortcut (``BatchNorm -> sign -> conv1x1``,
    hierarchical_block.py:30-36) computed inside the launch from the sign planes ``sc`` of that binarisation:
    no shortcut launch, no fp32 shortcut tensor.  Returns ``(y, PackedAct of the next block's input)``."""
    lib = native.require()
    N, c_in, H, W = a.shape
    if not a.nonneg or c_in != pack.c_in or tuple(sc.shape) != tuple(a.shape) or not pack.has_next:
        raise native.NativeError("bnn_amd: hblock_shortcut_forward needs the block's input planes, the shortcut's planes of "
                                 "the same shape, and a pack with the next block's BatchNorm")
    wsc, asc = sc_pack
    if wsc.numel() != pack.planes * (c_in // 32) or asc.numel() != pack.planes:
        raise native.NativeError("bnn_amd: shortcut pack of another width")
    dev = a.P.device
    with torch.cuda.device(dev):
        y = torch.empty((N, pack.planes, H, W), dtype=torch.float32, device=dev)
        pk = _nonneg_planes(N, pack.planes, H, W, dev)
        if N == 0:
            return y, pk
        d, wbuf = _hblock_launch(pack, a, throughput, rows_per_band, images_per_band, waves, channel_lanes)
        native.check(lib.bnn_hip_hblock_shortcut_forward(ctypes.byref(d), a.P.data_ptr(), wbuf.data_ptr(),
                                                         pack.consts.data_ptr(), sc.P.data_ptr(), sc.M.data_ptr(),
                                                         wsc.data_ptr(), asc.data_ptr(), y.data_ptr(), pk.P.data_ptr(),
                                                         _stream(dev)), "bnn_hip_hblock_shortcut_forward")
    return y, pk


def hblock_pool_supported(N: int, c_in: int, H: int, W: int, planes: int, throughput: bool = False, rows_per_band: int = 0,
                          images_per_band: int = 0, waves: int = 0) -> bool:
    """Whether ``hblock_pool_forward`` covers this geometry (with this plan) on the current device."""
    return _hblock_query("bnn_hip_hblock_pool_supported", N, c_in, H, W, planes, throughput, rows_per_band, images_per_band,
                         waves)


def hblock_pool_consts(bn1, bn_ds, planes: int) -> torch.Tensor:
    """The constants of ``hblock_pool_forward`` (include/bnn_hip.h: ``[a1/4 | b1 | a2/4 | b2 | -a2/4 | -b2 | 0 | 0]``) from
    the folded bn1 of the next stage's first block and the folded BatchNorm of its shortcut (hierarchical_block.py:30-39).
    The average's division by 4 moves into the scales; raises when that is not exact (a scale next to the smallest normal)."""
    a1, b1, a2, b2 = (_per_channel(t, planes, "pool bn") for t in (bn1[0], bn1[1], bn_ds[0], bn_ds[1]))
    q1, q2 = a1 * 0.25, a2 * 0.25
    if not (bool((q1 * 4.0 == a1).all()) and bool((q2 * 4.0 == a2).all())):
        raise native.NativeError("bnn_amd: hblock_pool_consts: a BatchNorm scale too small to be divided by 4 exactly")
    z = torch.zeros_like(a1)
    return torch.cat((q1, b1, q2, b2, -q2, -b2, z, z)).contiguous()


def hblock_pool_forward(a: PackedAct, pack: HBlockPack, residual: torch.Tensor, pool_consts: torch.Tensor,
                        throughput: bool = False, rows_per_band: int = 0, images_per_band: int = 0, waves: int = 0):
    """The LAST hierarchical block of a stage + ``AvgPool2d(2, 2)`` + the two binarisations of the pooled tensor that the
    next stage's first block performs (its bn1 -> ReLU -> sign; its shortcut's BatchNorm -> sign), ONE launch, no fp32
    output (bnn/models/resnet.py: ``nn.Sequential(AvgPool2d(2, 2), HBlock(...))`` stages).  Returns
    ``(PackedAct of sign(relu(bn1(t))), PackedAct of sign(bn_ds(t)))`` with ``t = AvgPool2d(2, 2)(HBlock(x))``."""
    lib = native.require()
    N, c_in, H, W = a.shape
    if not a.nonneg or c_in != pack.c_in or c_in != pack.planes:
        raise native.NativeError("bnn_amd: hblock_pool_forward needs non-negative input planes of a width-preserving block")
    wrong = "residual shape {got} != block output (even height and width)"
    residual = _shaped(residual, (N, pack.planes, H, W), "residual", wrong)
    if H % 2 or W % 2:
        raise native.NativeError("bnn_amd: " + wrong.format(got=tuple(residual.shape)))
    if (pool_consts.dtype != torch.float32 or pool_consts.numel() != 8 * pack.planes or not pool_consts.is_contiguous()
            or pool_consts.device != a.P.device):
        raise native.NativeError("bnn_amd: pool_consts must be the buffer of hblock_pool_consts")
    dev = a.P.device
    with torch.cuda.device(dev):
        p1 = _nonneg_planes(N, pack.planes, H // 2, W // 2, dev)
        p2 = PackedAct(torch.empty_like(p1.P), torch.empty_like(p1.P), p1.shape)
        if N == 0:
            return p1, p2
        d, wbuf = _hblock_launch(pack, a, throughput, rows_per_band, images_per_band, waves)
        native.check(lib.bnn_hip_hblock_pool_forward(ctypes.byref(d), a.P.data_ptr(), wbuf.data_ptr(),
                                                     pack.consts.data_ptr(), pool_consts.data_ptr(), residual.data_ptr(),
                                                     p1.P.data_ptr(), p2.P.data_ptr(), p2.M.data_ptr(), _stream(dev)),
                     "bnn_hip_hblock_pool_forward")
    return p1, p2


_ZERO_PLANES = {}


def _zero_plane(shape, dev) -> torch.Tensor:
    """An all-zero M plane (read-only by convention: planes of non-negative activations), shared per shape and device."""
    key = (tuple(shape), dev.index)
    z = _ZERO_PLANES.get(key)
    if z is None:
        z = _ZERO_PLANES[key] = torch.zeros(shape, dtype=torch.int64, device=dev)
    return z


def fused_launch_images(N: int, C: int, H: int, W: int, O: int, kernel_size, stride=1, padding=0, dilation=1,
                        c_total: Optional[int] = None) -> int:
    """Images ONE launch of ``bconv2d_fused`` covers for this geometry (a batch whose tensors exceed the kernels'
    32-bit addressing is split into several launches): what shape-dependent decisions have to be taken on."""
    kh, kw = _pair(kernel_size)
    ho, wo = conv_out_hw(H, W, kh, kw, stride, padding, dilation)
    return _launch_images(N, C, O, O if c_total is None else c_total, 2 * H * W * ((C + 63) // 64), ho * wo)


def shortcut_fold_supported(a: PackedAct, w: PackedWeight, sc_channels: int, stride=1, padding=0, dilation=1,
                            throughput: bool = False) -> bool:
    """Whether ``bconv2d_fused(a, w, ..., shortcut=...)`` exists for this convolution and a shortcut 1x1 convolution of
    ``sc_channels`` input channels (``bnn_hip_shortcut_fold_supported``)."""
    lib = native.require()
    d = _desc(a.shape, w.shape, stride, padding, dilation, _flags(w, False, None, a, throughput))
    return bool(lib.bnn_hip_shortcut_fold_supported(ctypes.byref(d), int(sc_channels)))


def grad_supported(x_shape, w_shape, stride, padding, dilation) -> bool:
    """Shapes the binary-aware gradient kernels cover: 3x3 / stride 1 or 2 / padding 1 and 1x1 / stride 1 / padding 0,
    dilation 1, width <= 64."""
    k = tuple(w_shape[2:])
    if _pair(dilation) != (1, 1) or x_shape[3] > 64 or x_shape[0] <= 0:
        return False
    if k == (3, 3):
        return _pair(stride) in ((1, 1), (2, 2)) and _pair(padding) == (1, 1)
    return k == (1, 1) and _pair(stride) == (1, 1) and _pair(padding) == (0, 0)


def sconv_supported(x_shape, w_shape, stride, padding, dilation) -> bool:
    """Shapes the real-weight convolution kernel (csrc/sconv.hip) covers: exactly those of ``grad_supported``, whose
    weight-gradient kernel its training step uses (3x3 / stride 1 or 2 / padding 1 and 1x1 / stride 1 / padding 0,
    dilation 1, ``groups == 1``, input width <= 64)."""
    return len(x_shape) == 4 and len(w_shape) == 4 and x_shape[1] == w_shape[1] \
        and grad_supported(x_shape, w_shape, stride, padding, dilation)


@dataclass
class SconvWeight:
    """A real-valued weight ``[O,C,k,k]`` as the MFMA fragments of ``bnn_hip_sconv2d_f32`` (three bf16 terms per weight
    and one exponent per output channel: include/bnn_hip.h)."""
    data: torch.Tensor                  # uint8 [bnn_hip_sconv2d_weight_pack_bytes(O, C, k)]
    shape: Tuple[int, int, int, int]    # (O, C, k, k)


def sconv_pack_weight(w: torch.Tensor) -> SconvWeight:
    """``bnn_hip_sconv2d_pack_weight_f32``: ``W [O,C,k,k]`` fp32 (k = 3 or 1) -> ``SconvWeight``."""
    w = _require_cuda_f32(w.detach(), "weight")
    if w.dim() != 4 or w.shape[2] != w.shape[3]:
        raise native.NativeError(f"bnn_amd: sconv_pack_weight expects [O,C,k,k], got shape {tuple(w.shape)}")
    lib = native.require()
    O, C, k = w.shape[0], w.shape[1], w.shape[2]
    with torch.cuda.device(w.device):
        packed = torch.empty(int(lib.bnn_hip_sconv2d_weight_pack_bytes(O, C, k)), dtype=torch.uint8, device=w.device)
        native.check(lib.bnn_hip_sconv2d_pack_weight_f32(w.data_ptr(), O, C, k, packed.data_ptr(), _stream(w.device)),
                     "bnn_hip_sconv2d_pack_weight_f32")
    return SconvWeight(packed, (O, C, k, k))


def sconv2d(x: torch.Tensor, packed: SconvWeight, bias=None, post_scale=None, stride=1, padding=None) -> torch.Tensor:
    """``(conv2d(s(x), W) + bias[o]) * post_scale[o]`` in one launch from the fp32 NCHW ``x`` (``bnn_hip_sconv2d_f32``):
    ``s(x)`` = +1 / -1 / 0 for x > 0 / x < 0 / anything else.  ``padding`` must be ``k // 2`` (``None``: that).  A geometry
    outside ``sconv_supported`` raises (``BNN_HIP_ERR_UNSUPPORTED``)."""
    x = _require_cuda_f32(x, "activation")
    O, C, k, _ = packed.shape
    if x.dim() != 4 or x.shape[1] != C:
        raise native.NativeError(f"bnn_amd: sconv2d: input {tuple(x.shape)} does not match the weight {packed.shape}")
    st = _pair(stride)
    if st[0] != st[1] or (padding is not None and _pair(padding) != (k // 2, k // 2)):
        native.check(native.ERR_UNSUPPORTED, "bnn_hip_sconv2d_f32")
    bias = _per_channel(bias, O, "bias")
    post_scale = _per_channel(post_scale, O, "post_scale")
    lib = native.require()
    _opaque(packed.data, lib.bnn_hip_sconv2d_weight_pack_bytes(O, C, k), "packed weight", torch.uint8)
    N, _, H, W = x.shape
    with torch.cuda.device(x.device):
        y = torch.empty((N, O, (H - 1) // st[0] + 1, (W - 1) // st[0] + 1), dtype=torch.float32, device=x.device)
        if N:
            native.check(lib.bnn_hip_sconv2d_f32(x.data_ptr(), packed.data.data_ptr(), _ptr(bias), _ptr(post_scale),
                                                 y.data_ptr(), N, O, C, H, W, k, st[0], _stream(x.device)),
                         "bnn_hip_sconv2d_f32")
    return y


def _grad_pack(w: torch.Tensor, what: str, symbol: str, *switches):
    """The two packers of the input-gradient kernel's weight: ``[O,C,k,k]`` fp32 -> (sign fragments, alpha[O]) through the
    entry point ``symbol(w, O, C, k, *switches, packed, alpha, stream)``."""
    w = _require_cuda_f32(w.detach(), what)
    lib = native.require()
    O, C, k = w.shape[0], w.shape[1], w.shape[2]
    with torch.cuda.device(w.device):
        packed = torch.empty(int(lib.bnn_hip_grad_weight_pack_bytes(O, C, k)), dtype=torch.uint8, device=w.device)
        alpha = torch.empty(O, dtype=torch.float32, device=w.device)
        native.check(getattr(lib, symbol)(w.data_ptr(), O, C, k, *switches, packed.data_ptr(), alpha.data_ptr(),
                                          _stream(w.device)), symbol)
    return packed, alpha


def grad_pack_weight(w_hat: torch.Tensor):
    """``What = sign(Wc) * alpha`` ([O,C,k,k] fp32, k = 3 or 1) -> (sign fragments for the input-gradient kernel,
    alpha[O])."""
    return _grad_pack(w_hat, "w_hat", "bnn_hip_grad_pack_weight_f32")


def xnor_grad_pack_weight(w: torch.Tensor, center: bool, compute_alpha: bool):
    """``grad_pack_weight(xnor_what(w, center, compute_alpha))`` in one launch (``bnn_hip_xnor_grad_pack_weight_f32``): the
    sign fragments and ``alpha[O]`` the input-gradient kernel reads, straight from the raw weight — the same bytes."""
    return _grad_pack(w, "weight", "bnn_hip_xnor_grad_pack_weight_f32", int(center), int(compute_alpha))


@dataclass
class SavedAct:
    """What the backward of a binary convolution needs from its fp32 input, in 3 bits per element: the sign planes
    (``sign``: P = x > 0, M = x < 0) and the straight-through mask ``T`` = |x| < 1, int64 ``[N, ceil(C/64), H, W]`` each
    (csrc/pack_ste.hip).  The reference's autograd keeps the fp32 ``x`` and an fp32 ``sign(x)`` instead."""
    sign: "PackedAct"
    T: torch.Tensor
    shape: Tuple[int, int, int, int]

    def nbytes(self) -> int:
        return 3 * self.T.numel() * 8


def pack_act_ste(x: torch.Tensor) -> SavedAct:
    """``bnn_hip_pack_act_ste_f32``: one pass over ``x`` -> the three bit planes of ``SavedAct``."""
    x = _nchw(x, "activation", "pack_act_ste")
    lib = native.require()
    N, C, H, W = x.shape
    with torch.cuda.device(x.device):
        a = empty_packed(N, C, H, W, x.device)
        T = torch.empty_like(a.P)
        if N:
            native.check(lib.bnn_hip_pack_act_ste_f32(x.data_ptr(), N, C, H, W, a.P.data_ptr(), a.M.data_ptr(),
                                                      T.data_ptr(), _stream(x.device)), "bnn_hip_pack_act_ste_f32")
    return SavedAct(a, T, (N, C, H, W))


def _ste_planes(x: torch.Tensor, what: str):
    """What the three-plane producers share: the fp32 NCHW check of ``x`` and empty ``P`` / ``M`` / ``T``."""
    x = _nchw(x, "activation", what)
    N, C, H, W = x.shape
    a = empty_packed(N, C, H, W, x.device)
    return x, SavedAct(a, torch.empty_like(a.P), (N, C, H, W))


def bn_act_pack_ste(x: torch.Tensor, bn_scale=None, bn_shift=None) -> SavedAct:
    """``pack_act_ste(fma(x, scale[c], shift[c]))`` in one pass over ``x``, the affine result never written
    (``bnn_hip_bn_act_pack_ste_f32``).  Both constants or neither; neither: the bits of ``pack_act_ste(x)``."""
    if (bn_scale is None) != (bn_shift is None):
        raise native.NativeError("bnn_amd: bn_act_pack_ste takes bn_scale and bn_shift together")
    x, sv = _ste_planes(x, "bn_act_pack_ste")
    N, C, H, W = x.shape
    bn_scale = _per_channel(bn_scale, C, "bn_scale")
    bn_shift = _per_channel(bn_shift, C, "bn_shift")
    lib = native.require()
    if N:
        with torch.cuda.device(x.device):
            native.check(lib.bnn_hip_bn_act_pack_ste_f32(
                x.data_ptr(), N, C, H, W, _ptr(bn_scale), _ptr(bn_shift), sv.sign.P.data_ptr(), sv.sign.M.data_ptr(),
                sv.T.data_ptr(), _stream(x.device)), "bnn_hip_bn_act_pack_ste_f32")
    return sv


def _ste_planes_s2(x: torch.Tensor, what: str):
    """``_ste_planes`` for the two pixel lattices of ``FactorizedReduce``: ``P`` / ``M`` / ``T`` as ``[2, N, cw64, H/2,
    W/2]`` tensors (phase-major, what one launch writes) and the two ``SavedAct`` that view them."""
    x = _require_cuda_f32(x, "activation")
    if x.dim() != 4 or x.shape[2] % 2 or x.shape[3] % 2:
        raise native.NativeError(f"bnn_amd: {what} expects NCHW with even H and W, got shape {tuple(x.shape)}")
    N, C, H, W = x.shape
    shape = (N, C, H // 2, W // 2)
    P = torch.empty((2, N, (C + 63) // 64, H // 2, W // 2), dtype=torch.int64, device=x.device)
    M, T = torch.empty_like(P), torch.empty_like(P)
    return x, (P, M, T), tuple(SavedAct(PackedAct(P[k], M[k], shape), T[k], shape) for k in range(2))


def bn_act_pack_ste_s2(x: torch.Tensor, bn_scale=None, bn_shift=None):
    """``(bn_act_pack_ste(x[:, :, ::2, ::2]), bn_act_pack_ste(x[:, :, 1::2, 1::2]))`` — the three planes of the two pixel
    lattices ``FactorizedReduce`` reads — in one pass over ``x`` (``bnn_hip_bn_act_pack_ste_s2_f32``; H and W even).
    Both constants or neither."""
    if (bn_scale is None) != (bn_shift is None):
        raise native.NativeError("bnn_amd: bn_act_pack_ste_s2 takes bn_scale and bn_shift together")
    x, (P, M, T), phases = _ste_planes_s2(x, "bn_act_pack_ste_s2")
    N, C, H, W = x.shape
    bn_scale = _per_channel(bn_scale, C, "bn_scale")
    bn_shift = _per_channel(bn_shift, C, "bn_shift")
    lib = native.require()
    if N:
        with torch.cuda.device(x.device):
            native.check(lib.bnn_hip_bn_act_pack_ste_s2_f32(
                x.data_ptr(), N, C, H, W, _ptr(bn_scale), _ptr(bn_shift), P.data_ptr(), M.data_ptr(), T.data_ptr(),
                _stream(x.device)), "bnn_hip_bn_act_pack_ste_s2_f32")
    return phases


def _grad_shapes(g: torch.Tensor, x, stride: int):
    N, C, H, W = x.shape
    O = g.shape[1]
    if tuple(g.shape) != (N, O, (H - 1) // stride + 1, (W - 1) // stride + 1):
        raise native.NativeError(f"bnn_amd: grad_output {tuple(g.shape)} does not belong to input {tuple(x.shape)} "
                                 f"at stride {stride}")
    return N, O, C, H, W


def bconv_grad_input(g: torch.Tensor, x, packed: torch.Tensor, alpha: torch.Tensor,
                     ksize: int = 3, stride: int = 1) -> torch.Tensor:
    """dL/dx of the binary 3x3/p1 or 1x1/p0 conv incl. the hard-tanh STE mask (bnn/ops.py:68-73).  ``x``: the fp32
    input, or its ``SavedAct`` (the mask plane is all this kernel needs of it) — same bits either way."""
    g = _require_cuda_f32(g, "grad_output")
    lib = native.require()
    saved = isinstance(x, SavedAct)
    symbol = "bnn_hip_bconv_grad_input_packed_f32" if saved else "bnn_hip_bconv_grad_input_f32"
    if not saved:
        x = _require_cuda_f32(x, "input")
    N, O, C, H, W = _grad_shapes(g, x, stride)
    alpha = _per_channel(alpha, O, "alpha")
    packed = _opaque(packed, lib.bnn_hip_grad_weight_pack_bytes(O, C, ksize), "packed weight", torch.uint8)
    with torch.cuda.device(g.device):
        gx = torch.empty((N, C, H, W), dtype=torch.float32, device=g.device)
        native.check(getattr(lib, symbol)(g.data_ptr(), alpha.data_ptr(), packed.data_ptr(), (x.T if saved else x).data_ptr(),
                                          gx.data_ptr(), N, O, C, H, W, ksize, stride, _stream(g.device)), symbol)
    return gx


def bconv_grad_weight(g: torch.Tensor, x, ksize: int = 3, stride: int = 1, reduce: bool = True,
                      splits: Optional[int] = None) -> torch.Tensor:
    """dL/dWhat [O,C,k,k] of the binary 3x3/p1 or 1x1/p0 conv: correlation of g with sign(x).  ``x``: the fp32 input, or
    its ``SavedAct`` (the sign planes are all this kernel needs of it) — same bits either way.  ``reduce=False``: the
    kernel's split-K partial slabs ``[splits, O, C, k, k]`` as they are (``xnor_weight_backward`` adds them itself).
    ``splits=None``: the library's choice (``bnn_hip_bconv_grad_weight_splits``); a value of the caller's goes to the entry
    point as it is, which refuses one that is not ``ceil(N / ceil(N / splits))``."""
    g = _require_cuda_f32(g, "grad_output")
    if not isinstance(x, SavedAct):
        x = _require_cuda_f32(x, "input")
    lib = native.require()
    N, O, C, H, W = _grad_shapes(g, x, stride)
    splits = int(lib.bnn_hip_bconv_grad_weight_splits(N, O, C, ksize)) if splits is None else int(splits)
    if splits < 1 or splits > N:                     # (before `part` is sized by it)
        native.check(native.ERR_INVALID_ARG, "bnn_hip_bconv_grad_weight_f32")
    with torch.cuda.device(g.device):
        part = torch.empty((splits, O, C, ksize, ksize), dtype=torch.float32, device=g.device)
        if isinstance(x, SavedAct):
            native.check(lib.bnn_hip_bconv_grad_weight_packed_f32(
                g.data_ptr(), x.sign.P.data_ptr(), x.sign.M.data_ptr(), part.data_ptr(), splits, N, O, C, H, W, ksize,
                stride, _stream(g.device)), "bnn_hip_bconv_grad_weight_packed_f32")
        else:
            native.check(lib.bnn_hip_bconv_grad_weight_f32(g.data_ptr(), x.data_ptr(), part.data_ptr(), splits,
                                                           N, O, C, H, W, ksize, stride, _stream(g.device)),
                         "bnn_hip_bconv_grad_weight_f32")
        if not reduce:
            return part
        return part[0] if splits == 1 else part.sum(0)


def _grouped_grad_desc(x_shape, w_shape, groups, stride, padding, dilation) -> native.ConvDesc:
    """Descriptor of a grouped layer for the ``bnn_hip_bconv_grouped_grad_*`` entry points: all ``C`` input channels, the
    weight ``[O, C / groups, KH, KW]``."""
    N, C, H, W = x_shape
    O, Cg, KH, KW = w_shape
    if Cg * groups != C:
        raise native.NativeError(f"bnn_amd: grouped weight reads {Cg} x {groups} channels, the input has {C}")
    return _desc(x_shape, (O, C, KH, KW), stride, padding, dilation, 0)


def grouped_grad_supported(x_shape, w_shape, groups, stride, padding, dilation) -> bool:
    """Whether the grouped gradient kernels (csrc/grad_grouped.hip) cover the layer: the library's own answer
    (``bnn_hip_bconv_grouped_grad_supported``, a host function)."""
    return grouped_grad_weight_splits(x_shape, w_shape, groups, stride, padding, dilation) > 0


def grouped_grad_weight_splits(x_shape, w_shape, groups, stride, padding, dilation) -> int:
    """How many partial slabs ``bconv_grouped_grad_weight`` writes by default (the library's choice, a host function);
    0 when the gradient kernels do not cover the layer, or the weight does not belong to the input."""
    if len(x_shape) != 4 or len(w_shape) != 4 or groups < 1:
        return 0
    try:
        d = _grouped_grad_desc(x_shape, w_shape, groups, stride, padding, dilation)
    except native.NativeError:
        return 0
    return int(native.require().bnn_hip_bconv_grouped_grad_weight_splits(ctypes.byref(d), int(groups)))


def _grouped_grad_args(g: torch.Tensor, saved: "SavedAct", w_shape, groups, stride, padding, dilation):
    g = _require_cuda_f32(g, "grad_output")
    d = _grouped_grad_desc(saved.shape, w_shape, groups, stride, padding, dilation)
    ho, wo = conv_out_hw(d.H, d.W, d.KH, d.KW, stride, padding, dilation)
    if tuple(g.shape) != (d.N, d.O, ho, wo):
        raise native.NativeError(f"bnn_amd: grad_output {tuple(g.shape)} does not belong to input {tuple(saved.shape)} "
                                 f"and weight {tuple(w_shape)}")
    return g, d


def bconv_grouped_grad_input(g: torch.Tensor, saved: "SavedAct", what: torch.Tensor, groups: int, stride=1, padding=0,
                             dilation=1) -> torch.Tensor:
    """dL/dx of a grouped binary convolution incl. the hard-tanh STE mask (bnn/ops.py:68-73), from ``g``, the fp32
    ``What [O, C/groups, KH, KW]`` (``xnor_what``) and the mask plane of ``saved`` (``bnn_hip_bconv_grouped_grad_input_f32``)."""
    what = _require_cuda_f32(what.detach(), "w_hat")
    g, d = _grouped_grad_args(g, saved, what.shape, groups, stride, padding, dilation)
    lib = native.require()
    with torch.cuda.device(g.device):
        gx = torch.empty(saved.shape, dtype=torch.float32, device=g.device)
        if d.N:
            native.check(lib.bnn_hip_bconv_grouped_grad_input_f32(
                ctypes.byref(d), int(groups), g.data_ptr(), what.data_ptr(), saved.T.data_ptr(), gx.data_ptr(),
                _stream(g.device)), "bnn_hip_bconv_grouped_grad_input_f32")
    return gx


def bconv_grouped_grad_weight(g: torch.Tensor, saved: "SavedAct", w_shape, groups: int, stride=1, padding=0, dilation=1,
                              reduce: bool = True, splits: Optional[int] = None) -> torch.Tensor:
    """dL/dWhat ``[O, C/groups, KH, KW]`` of a grouped binary convolution: correlation of ``g`` with ``sign(x)`` read from
    the sign planes of ``saved`` (``bnn_hip_bconv_grouped_grad_weight_f32``).  ``splits=None``: the library's choice;
    ``reduce=False``: the deterministic partial slabs ``[splits, *w_shape]`` as they are."""
    g, d = _grouped_grad_args(g, saved, w_shape, groups, stride, padding, dilation)
    lib = native.require()
    if splits is None:
        splits = grouped_grad_weight_splits(saved.shape, w_shape, groups, stride, padding, dilation)
        if splits <= 0:
            native.check(native.ERR_UNSUPPORTED, "bnn_hip_bconv_grouped_grad_weight_splits")
    with torch.cuda.device(g.device):
        part = torch.empty((int(splits), *[int(v) for v in w_shape]), dtype=torch.float32, device=g.device)
        native.check(lib.bnn_hip_bconv_grouped_grad_weight_f32(
            ctypes.byref(d), int(groups), g.data_ptr(), saved.sign.P.data_ptr(), saved.sign.M.data_ptr(), part.data_ptr(),
            int(splits), _stream(g.device)), "bnn_hip_bconv_grouped_grad_weight_f32")
        if not reduce:
            return part
        return part[0] if splits == 1 else part.sum(0)


def xnor_what(w: torch.Tensor, center: bool, compute_alpha: bool, return_alpha: bool = False):
    """``XNORWeightBinarizer.forward`` value (bnn/ops.py:129-140) in one kernel: ``sign(Wc) * alpha`` as an fp32 tensor
    (no autograd graph).  Same centring / alpha reductions as ``pack_weight``.  ``return_alpha``: ``(What, alpha[O])``, the
    kernel's own per-channel scale (1 without ``compute_alpha``)."""
    w = _require_cuda_f32(w.detach(), "weight")
    lib = native.require()
    O, C = w.shape[0], w.shape[1]
    kh, kw = (w.shape[2], w.shape[3]) if w.dim() == 4 else (1, 1)
    with torch.cuda.device(w.device):
        what = torch.empty_like(w)
        alpha = torch.empty(O, dtype=torch.float32, device=w.device) if return_alpha else None
        native.check(lib.bnn_hip_xnor_weight_forward_f32(w.data_ptr(), O, C, kh, kw, int(center), int(compute_alpha),
                                                         what.data_ptr(), _ptr(alpha), _stream(w.device)),
                     "bnn_hip_xnor_weight_forward_f32")
    return (what, alpha) if return_alpha else what


def xnor_weight_backward(w: torch.Tensor, dwhat: torch.Tensor, center: bool, compute_alpha: bool) -> torch.Tensor:
    """dL/dW from dL/dWhat through ``XNORWeightBinarizer`` (sign STE, alpha = mean|Wc|, centring) in one kernel.
    ``dwhat``: the gradient (``w``'s shape), or the split-K partial slabs ``[splits, *w.shape]`` of
    ``bconv_grad_weight(..., reduce=False)`` — added inside the kernel, in slab order."""
    w = _require_cuda_f32(w.detach(), "weight")
    dwhat = _require_cuda_f32(dwhat, "weight gradient")
    if dwhat.dim() == w.dim():
        dwhat = dwhat.unsqueeze(0)
    if tuple(dwhat.shape[1:]) != tuple(w.shape):
        raise native.NativeError(f"bnn_amd: weight gradient {tuple(dwhat.shape)} does not belong to weight {tuple(w.shape)}")
    lib = native.require()
    O, C = w.shape[0], w.shape[1]
    kh, kw = (w.shape[2], w.shape[3]) if w.dim() == 4 else (1, 1)
    with torch.cuda.device(w.device):
        dw = torch.empty_like(w)
        native.check(lib.bnn_hip_xnor_weight_backward_f32(w.data_ptr(), dwhat.data_ptr(), int(dwhat.shape[0]), O, C, kh, kw,
                                                          int(center), int(compute_alpha), dw.data_ptr(),
                                                          _stream(w.device)), "bnn_hip_xnor_weight_backward_f32")
    return dw


# ---- Linear as GEMM-shaped kernels (csrc/blinear.hip): forward from the float input, gradients from bits ---------------
_LINEAR_MAX_ELEMS = (1 << 30) - 1       # M * F and M * O of one launch (include/bnn_hip.h)


def _linear_rows(M: int, F: int, O: int) -> int:
    """Rows per launch of the Linear kernels."""
    return max(1, min(M, _LINEAR_MAX_ELEMS // max(F, O)))


def _linear_weight(w: PackedWeight, what: str) -> Tuple[int, int]:
    _ungrouped(w, what)
    if tuple(w.shape[2:]) != (1, 1):
        raise native.NativeError(f"bnn_amd: {what} takes the pack of an [O, F] weight, got {tuple(w.shape)}")
    return int(w.shape[0]), int(w.shape[1])


def _linear_planes(M: int, F: int, device) -> "SavedAct":
    a = empty_packed(M, F, 1, 1, device)
    return SavedAct(a, torch.empty_like(a.P), (M, F, 1, 1))


def blinear_direct(x: torch.Tensor, w: PackedWeight, bias: Optional[torch.Tensor] = None,
                   post_scale: Optional[torch.Tensor] = None, want_planes: bool = False, lds_words: int = 0):
    """``Linear.forward`` of the reference (bnn/layers/linear.py:22-27) in ONE launch of the row-major kernel
    (``bnn_hip_blinear_direct``): fp32, fp16 or bf16 ``[..., F]`` in, fp32 ``[..., O]`` out, ``sign(x)`` taken inside — the bits
    of ``bconv2d_direct`` on ``M`` images of 1 x 1 pixels.  ``want_planes``: returns ``(out, SavedAct)`` with the three bit
    planes of ``pack_act_ste`` (shape ``(M, F, 1, 1)``, ``M`` the flattened leading dimensions) from the same pass over
    ``x``.  ``lds_words``: the kernel's LDS pass over ``F`` in 32-bit words per row (0: its default; tests force it)."""
    O, F = _linear_weight(w, "blinear_direct")
    x = _require_cuda_act(x)
    if x.dim() < 1 or x.shape[-1] != F:
        raise native.NativeError(f"bnn_amd: blinear_direct expects [..., {F}], got shape {tuple(x.shape)}")
    lib = native.require()
    lead = tuple(x.shape[:-1])
    x2 = x.reshape(-1, F)
    M = x2.shape[0]
    dev = x.device
    bias = _per_channel(bias, O, "bias")
    post_scale = _per_channel(post_scale, O, "post_scale")
    with torch.cuda.device(dev):
        out = torch.empty((M, O), dtype=torch.float32, device=dev)
        sv = _linear_planes(M, F, dev) if want_planes else None
        dtype = _act_dtype(x)
        for m0, m1 in _split(M, _linear_rows(M, F, O)):
            pl = [None, None, None] if sv is None else [t[m0:m1].data_ptr() for t in (sv.sign.P, sv.sign.M, sv.T)]
            native.check(lib.bnn_hip_blinear_direct(
                m1 - m0, F, O, x2[m0:m1].data_ptr(), dtype, w.wbits.data_ptr(), w.wnz.data_ptr(), int(w.has_zero),
                w.alpha.data_ptr(), _ptr(bias), _ptr(post_scale), out[m0:m1].data_ptr(), *pl, int(lds_words), _stream(dev)),
                "bnn_hip_blinear_direct")
    out = out.reshape(*lead, O)
    return (out, sv) if want_planes else out


def _linear_grad_shapes(g: torch.Tensor, saved: "SavedAct", O: Optional[int] = None):
    M, F = int(saved.shape[0]), int(saved.shape[1])
    if tuple(saved.shape[2:]) != (1, 1) or g.dim() < 1 or (O is not None and g.shape[-1] != O) or g.numel() != M * g.shape[-1]:
        raise native.NativeError(f"bnn_amd: grad_output {tuple(g.shape)} does not belong to the planes of a "
                                 f"{tuple(saved.shape[:2])} input")
    return M, F, int(g.shape[-1])


def blinear_grad_input(g: torch.Tensor, saved: "SavedAct", w: PackedWeight) -> torch.Tensor:
    """dL/dx ``[M, F]`` of the binary Linear incl. the hard-tanh STE mask: ``(sum_o g alpha sign(Wc)) * 1[|x| < 1]``, from
    the forward's own weight pack (sign bits and zero mask) and the mask plane of ``saved``."""
    O, F = _linear_weight(w, "blinear_grad_input")
    g = _require_cuda_f32(g, "grad_output")
    M, F2, _ = _linear_grad_shapes(g, saved, O)
    if F2 != F:
        raise native.NativeError(f"bnn_amd: planes of {F2} features against a weight of {F}")
    g = g.reshape(M, O)
    lib = native.require()
    with torch.cuda.device(g.device):
        gx = torch.empty((M, F), dtype=torch.float32, device=g.device)
        for m0, m1 in _split(M, _linear_rows(M, F, O)):
            native.check(lib.bnn_hip_blinear_grad_input_f32(
                g[m0:m1].data_ptr(), w.alpha.data_ptr(), w.wbits.data_ptr(), w.wnz.data_ptr(), saved.T[m0:m1].data_ptr(),
                gx[m0:m1].data_ptr(), m1 - m0, O, F, _stream(g.device)), "bnn_hip_blinear_grad_input_f32")
    return gx


def blinear_grad_weight_splits(M: int, O: int, F: int) -> int:
    """The default row split of ``blinear_grad_weight`` (``bnn_hip_blinear_grad_weight_splits``)."""
    s = int(native.require().bnn_hip_blinear_grad_weight_splits(M, O, F))
    if s < 1:
        native.check(s, "bnn_hip_blinear_grad_weight_splits")
    return s


def blinear_grad_weight(g: torch.Tensor, saved: "SavedAct", reduce: bool = True,
                        splits: Optional[int] = None) -> torch.Tensor:
    """dL/dWhat ``[O, F]`` of the binary Linear: ``sum_m g[m, o] sign(x)[m, f]`` from the sign planes of ``saved``.
    ``reduce=False``: the kernel's partial slabs ``[splits, O, F]`` as they are (``xnor_weight_backward`` adds them itself).
    ``splits=None``: the library's choice; a value of the caller's goes to the entry point as it is, which refuses one that
    is not ``ceil(M / ceil(M / splits))``."""
    g = _require_cuda_f32(g, "grad_output")
    M, F, O = _linear_grad_shapes(g, saved)
    g = g.reshape(M, O)
    lib = native.require()
    step = _linear_rows(M, F, O) if splits is None else M      # (a caller's split is one launch: the entry point judges it)
    parts = []
    with torch.cuda.device(g.device):
        for m0, m1 in _split(M, step):
            sp = blinear_grad_weight_splits(m1 - m0, O, F) if splits is None else int(splits)
            if sp < 1 or sp > m1 - m0:                 # (before `part` is sized by it)
                native.check(native.ERR_INVALID_ARG, "bnn_hip_blinear_grad_weight_f32")
            part = torch.empty((sp, O, F), dtype=torch.float32, device=g.device)
            native.check(lib.bnn_hip_blinear_grad_weight_f32(
                g[m0:m1].data_ptr(), saved.sign.P[m0:m1].data_ptr(), saved.sign.M[m0:m1].data_ptr(), part.data_ptr(), sp,
                m1 - m0, O, F, _stream(g.device)), "bnn_hip_blinear_grad_weight_f32")
            parts.append(part)
    part = parts[0] if len(parts) == 1 else torch.cat(parts, 0)
    if not reduce:
        return part
    return part[0] if part.shape[0] == 1 else part.sum(0)


# ---- Linear with binary activations and real weights (csrc/slinear.hip) -----------------------------------------------
def slinear_pack_weight(w: torch.Tensor) -> SconvWeight:
    """``W [O,F]`` fp32 -> the ``ksize = 1`` pack of ``sconv_pack_weight`` (shape ``(O, F, 1, 1)``): what ``slinear`` reads."""
    if w.dim() != 2:
        raise native.NativeError(f"bnn_amd: slinear_pack_weight expects [O,F], got shape {tuple(w.shape)}")
    return sconv_pack_weight(w.detach().reshape(w.shape[0], w.shape[1], 1, 1))


def slinear(x: torch.Tensor, packed: SconvWeight, bias=None, post_scale=None, want_planes: bool = False):
    """``(s(x) @ W.T + bias[o]) * post_scale[o]`` in one launch of the row-major kernel (``bnn_hip_slinear_f32``): fp32
    ``[..., F]`` in, fp32 ``[..., O]`` out, ``s(x)`` = +1 / -1 / 0 for x > 0 / x < 0 / anything else taken inside.
    ``want_planes``: returns ``(out, SavedAct)`` with the three bit planes of ``pack_act_ste`` (shape ``(M, F, 1, 1)``,
    ``M`` the flattened leading dimensions) from the same pass over ``x``."""
    x = _require_cuda_f32(x, "activation")
    O, F = int(packed.shape[0]), int(packed.shape[1])
    if tuple(packed.shape[2:]) != (1, 1):
        raise native.NativeError(f"bnn_amd: slinear takes the pack of an [O, F] weight, got {tuple(packed.shape)}")
    if x.dim() < 1 or x.shape[-1] != F:
        raise native.NativeError(f"bnn_amd: slinear expects [..., {F}], got shape {tuple(x.shape)}")
    bias = _per_channel(bias, O, "bias")
    post_scale = _per_channel(post_scale, O, "post_scale")
    lib = native.require()
    _opaque(packed.data, lib.bnn_hip_sconv2d_weight_pack_bytes(O, F, 1), "packed weight", torch.uint8)
    lead = tuple(x.shape[:-1])
    x2 = x.reshape(-1, F)
    M = x2.shape[0]
    dev = x.device
    with torch.cuda.device(dev):
        out = torch.empty((M, O), dtype=torch.float32, device=dev)
        sv = _linear_planes(M, F, dev) if want_planes else None
        for m0, m1 in _split(M, _linear_rows(M, F, O)):
            pl = [None, None, None] if sv is None else [t[m0:m1].data_ptr() for t in (sv.sign.P, sv.sign.M, sv.T)]
            native.check(lib.bnn_hip_slinear_f32(m1 - m0, F, O, x2[m0:m1].data_ptr(), packed.data.data_ptr(), _ptr(bias),
                                                 _ptr(post_scale), out[m0:m1].data_ptr(), *pl, _stream(dev)),
                         "bnn_hip_slinear_f32")
    out = out.reshape(*lead, O)
    return (out, sv) if want_planes else out


def ste_mask_(gx: torch.Tensor, saved: "SavedAct") -> torch.Tensor:
    """The hard-tanh straight-through mask in place (``bnn_hip_ste_mask_f32``): ``gx[m, f]`` becomes ``+0.0`` where the
    ``T`` plane of ``saved`` (shape ``(M, F, 1, 1)``) says ``|x| >= 1``.  ``gx``: contiguous fp32 with ``M * F`` elements."""
    M, F = int(saved.shape[0]), int(saved.shape[1])
    wrong = f"ste_mask_ expects a contiguous fp32 HIP tensor [..., {F}] of {M} rows, got {tuple(gx.shape)} {gx.dtype} on " \
            f"{gx.device}"
    if tuple(saved.shape[2:]) != (1, 1) or gx.dim() < 1 or gx.shape[-1] != F:
        raise native.NativeError("bnn_amd: " + wrong)
    lib = native.require()
    g2 = _written(gx, M * F, "gx", wrong).view(M, F)
    with torch.cuda.device(gx.device):
        for m0, m1 in _split(M, _linear_rows(M, F, 1)):
            native.check(lib.bnn_hip_ste_mask_f32(g2[m0:m1].data_ptr(), saved.T[m0:m1].data_ptr(), m1 - m0, F,
                                                  _stream(gx.device)), "bnn_hip_ste_mask_f32")
    return gx


_BLINEAR_MIN_ROWS = 4096


def blinear_preferred(M: int, F: int, O: int) -> bool:
    """Whether ``linear`` runs the row-major kernel for this shape: where tools/bench_linear.py measured it not slower than
    the 1x1-image route (profiles/linear_bench.jsonl; DESIGN.md section 4, "Linear").  Measured on an MI355X, blinear / conv
    in us: every shape of 4096 rows and more wins (4096 x 768 -> 3072: 75 / 110; 8192 x 1024 -> 1024: 76 / 124; 16384 and
    32768 rows: 0.27-0.41 of the conv route's time; 50176 x 768 -> 3072: 648 / 1469; 50176 x 3072 -> 768: 718 / 2501), the
    small batches lose or tie (32 x 4096 -> 4096: 96 / 42; 1024 x 1024 -> 1024: 43.6 / 39.6; 256 x 512 -> 1000: 26.5 / 26.3:
    a workgroup owns 64 rows, so few rows are few workgroups, each binarising its rows again for its share of the output
    channels) and stay on the conv route; nothing between 1024 and 4096 rows was measured, so the threshold is the smallest
    measured win."""
    return M >= _BLINEAR_MIN_ROWS


def linear(x: torch.Tensor, w: PackedWeight, bias: Optional[torch.Tensor] = None,
           post_scale: Optional[torch.Tensor] = None, route: Optional[str] = None) -> torch.Tensor:
    """``Linear.forward`` on ``[..., F]``: the row-major kernel (``blinear_direct``) where ``blinear_preferred`` says so,
    else ``bconv2d_direct`` on 1 x 1 images — the same bits either way.  ``route``: ``None`` picks per shape; ``"blinear"``
    / ``"conv"`` force one (tools, tests)."""
    if route not in (None, "blinear", "conv"):
        raise ValueError("route must be None, 'blinear' or 'conv'")
    O, F = int(w.shape[0]), int(w.shape[1])
    lead = tuple(x.shape[:-1])
    x2 = x.reshape(-1, x.shape[-1])
    if route == "blinear" or (route is None and x2.shape[0] > 0 and blinear_preferred(x2.shape[0], F, O)):
        return blinear_direct(x2, w, bias, post_scale).reshape(*lead, O)
    return bconv2d_direct(x2[:, :, None, None], w, bias, post_scale).reshape(*lead, O)


def bn_act(x: torch.Tensor, bn_scale: torch.Tensor, bn_shift: torch.Tensor, relu: bool = False,
           residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``relu?(fma(x, scale[c], shift[c]) (+ residual))``: eval-mode BatchNorm with folded constants + the residual add +
    ReLU of a residual block as ONE launch (include/bnn_hip.h: bnn_hip_bn_act_f32) — the tail of the per-layer path; the
    same float operations as the fused convolution epilogue."""
    x = _nchw(x, "BatchNorm input", "bn_act")
    lib = native.require()
    N, C, H, W = x.shape
    bn_scale = _per_channel(bn_scale, C, "bn_scale")
    bn_shift = _per_channel(bn_shift, C, "bn_shift")
    residual = _shaped(residual, x.shape, "residual", "residual shape differs from the BatchNorm input's")
    with torch.cuda.device(x.device):
        y = torch.empty_like(x)
        if x.numel():
            native.check(lib.bnn_hip_bn_act_f32(x.data_ptr(), N, C, H * W, bn_scale.data_ptr(), bn_shift.data_ptr(),
                                                _ptr(residual), int(bool(relu)), y.data_ptr(), _stream(x.device)),
                         "bnn_hip_bn_act_f32")
    return y


def _bn_train_buffers(lib, x: torch.Tensor):
    """What every training-BatchNorm entry point needs beside its tensors: two per-channel fp32 results (mean / invstd
    going forward, dgamma / dbeta going back) and the workspace of ``bnn_hip_bn_train_workspace_bytes``."""
    N, C, H, W = x.shape
    return (torch.empty(C, dtype=torch.float32, device=x.device), torch.empty(C, dtype=torch.float32, device=x.device),
            torch.empty(int(lib.bnn_hip_bn_train_workspace_bytes(N, C, H * W)), dtype=torch.uint8, device=x.device))


def _bn_train_affine(C: int, gamma, beta, running_mean, running_var):
    """The operands of a training BatchNorm going forward, each optional: ``gamma`` / ``beta`` per channel (read), the
    running statistics (written in place)."""
    return (_per_channel(gamma, C, "BatchNorm weight"), _per_channel(beta, C, "BatchNorm bias"),
            _written(running_mean, C, "running_mean"), _written(running_var, C, "running_var"))


def _bn_train_saved(C: int, mean, invstd, gamma):
    """The operands of a training BatchNorm going back: the forward's saved statistics and the optional ``gamma``."""
    return _shaped(mean, (C,), "mean"), _shaped(invstd, (C,), "invstd"), _per_channel(gamma, C, "BatchNorm weight")


def bn_train_forward(x: torch.Tensor, gamma, beta, running_mean, running_var, momentum: float, eps: float,
                     relu: bool = False, residual: Optional[torch.Tensor] = None):
    """``relu?(batch_norm(x, training=True) (+ residual))`` in three launches (csrc/bn_train.hip).  Updates the running
    statistics in place (unbiased variance, momentum) like ``torch.nn.BatchNorm2d`` in training mode.  Returns
    ``(y, save_mean, save_invstd)``."""
    x = _nchw(x, "BatchNorm input", "bn_train_forward")
    lib = native.require()
    N, C, H, W = x.shape
    gamma, beta, running_mean, running_var = _bn_train_affine(C, gamma, beta, running_mean, running_var)
    residual = _shaped(residual, x.shape, "residual", "residual shape differs from the BatchNorm input's")
    with torch.cuda.device(x.device):
        y = torch.empty_like(x)
        mean, invstd, ws = _bn_train_buffers(lib, x)
        native.check(lib.bnn_hip_bn_train_forward_f32(
            x.data_ptr(), N, C, H * W, _ptr(gamma), _ptr(beta), _ptr(residual), int(bool(relu)), float(eps),
            float(momentum), _ptr(running_mean), _ptr(running_var), y.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
            ws.data_ptr(), _stream(x.device)), "bnn_hip_bn_train_forward_f32")
    return y, mean, invstd


def bn_train_backward(gy: torch.Tensor, y: Optional[torch.Tensor], x: torch.Tensor, mean: torch.Tensor,
                      invstd: torch.Tensor, gamma, want_dres: bool = False):
    """Backward of ``bn_train_forward``: ``(dx, dgamma, dbeta, dres | None)``.  ``y``: the forward's output when a ReLU
    was fused (its mask), else None."""
    x = _nchw(x, "BatchNorm input", "bn_train_backward")
    gy, y = _shaped(gy, x.shape, "grad_output"), _shaped(y, x.shape, "BatchNorm output")
    lib = native.require()
    N, C, H, W = x.shape
    mean, invstd, gamma = _bn_train_saved(C, mean, invstd, gamma)
    with torch.cuda.device(x.device):
        dx = torch.empty_like(x)
        dres = torch.empty_like(x) if want_dres else None
        dgamma, dbeta, ws = _bn_train_buffers(lib, x)
        native.check(lib.bnn_hip_bn_train_backward_f32(
            gy.data_ptr(), _ptr(y), x.data_ptr(), mean.data_ptr(), invstd.data_ptr(), _ptr(gamma), N, C, H * W,
            dx.data_ptr(), _ptr(dres), dgamma.data_ptr(), dbeta.data_ptr(), ws.data_ptr(), _stream(x.device)),
            "bnn_hip_bn_train_backward_f32")
    return dx, dgamma, dbeta, dres


def _bn_train_pack(symbol: str, x: torch.Tensor, planes, gamma, beta, running_mean, running_var, momentum, eps):
    """The launch of ``bn_train_pack_ste`` and ``bn_train_pack_ste_s2``: the batch statistics of ``x``, the running
    statistics' update, and ``planes`` ``(P, M, T)`` filled -> ``(save_mean, save_invstd, scale, shift)``."""
    N, C, H, W = x.shape
    gamma, beta, running_mean, running_var = _bn_train_affine(C, gamma, beta, running_mean, running_var)
    lib = native.require()
    with torch.cuda.device(x.device):
        mean, invstd, ws = _bn_train_buffers(lib, x)
        scale, shift = torch.empty_like(mean), torch.empty_like(mean)
        native.check(getattr(lib, symbol)(
            x.data_ptr(), N, C, H, W, _ptr(gamma), _ptr(beta), float(eps), float(momentum), _ptr(running_mean),
            _ptr(running_var), *(t.data_ptr() for t in planes), mean.data_ptr(), invstd.data_ptr(), scale.data_ptr(),
            shift.data_ptr(), ws.data_ptr(), _stream(x.device)), symbol)
    return mean, invstd, scale, shift


def bn_train_pack_ste(x: torch.Tensor, gamma, beta, running_mean, running_var, momentum: float, eps: float):
    """``pack_act_ste(batch_norm(x, training=True))`` without writing the normalised tensor
    (``bnn_hip_bn_train_pack_ste_f32``: the statistics kernels of ``bn_train_forward``, then BatchNorm + sign + STE mask
    as three bit planes).  Updates the running statistics like ``bn_train_forward``.  Returns ``(SavedAct, save_mean,
    save_invstd, scale, shift)`` — ``scale`` / ``shift`` are what the planes were made with."""
    x, sv = _ste_planes(x, "bn_train_pack_ste")
    return (sv, *_bn_train_pack("bnn_hip_bn_train_pack_ste_f32", x, (sv.sign.P, sv.sign.M, sv.T), gamma, beta, running_mean,
                                running_var, momentum, eps))


def bn_train_backward_add(gy: torch.Tensor, x: torch.Tensor, mean: torch.Tensor, invstd: torch.Tensor, gamma,
                          addend: Optional[torch.Tensor] = None):
    """``bn_train_backward`` (no fused ReLU) with ``dx += addend`` in the dx kernel (``bnn_hip_bn_train_backward_add_f32``):
    ``(dx, dgamma, dbeta)``.  ``addend=None``: the bits of ``bn_train_backward``."""
    gy = _require_cuda_f32(gy, "grad_output")
    x = _require_cuda_f32(x, "BatchNorm input")
    if x.dim() != 4 or gy.shape != x.shape:
        raise native.NativeError(f"bnn_amd: bn_train_backward_add: grad_output {tuple(gy.shape)} does not belong to the "
                                 f"NCHW input {tuple(x.shape)}")
    addend = _shaped(addend, x.shape, "addend", "addend shape differs from the BatchNorm input's")
    lib = native.require()
    N, C, H, W = x.shape
    mean, invstd, gamma = _bn_train_saved(C, mean, invstd, gamma)
    with torch.cuda.device(x.device):
        dx = torch.empty_like(x)
        dgamma, dbeta, ws = _bn_train_buffers(lib, x)
        native.check(lib.bnn_hip_bn_train_backward_add_f32(
            gy.data_ptr(), None, x.data_ptr(), mean.data_ptr(), invstd.data_ptr(), _ptr(gamma), _ptr(addend), N, C, H * W,
            dx.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), ws.data_ptr(), _stream(x.device)),
            "bnn_hip_bn_train_backward_add_f32")
    return dx, dgamma, dbeta


def bn_train_pack_ste_s2(x: torch.Tensor, gamma, beta, running_mean, running_var, momentum: float, eps: float):
    """``bn_train_pack_ste`` for ``FactorizedReduce`` (``bnn_hip_bn_train_pack_ste_s2_f32``): the same statistics over all
    of ``x`` and the same running-statistics update, then the planes of ``bn_act_pack_ste_s2``.  Returns ``((SavedAct,
    SavedAct), save_mean, save_invstd, scale, shift)``."""
    x, planes, phases = _ste_planes_s2(x, "bn_train_pack_ste_s2")
    return (phases, *_bn_train_pack("bnn_hip_bn_train_pack_ste_s2_f32", x, planes, gamma, beta, running_mean, running_var,
                                    momentum, eps))


def bn_train_backward_s2(g0: torch.Tensor, g1: torch.Tensor, x: torch.Tensor, mean: torch.Tensor, invstd: torch.Tensor,
                         gamma):
    """Backward of training-mode BatchNorm for a gradient that lives on the two pixel lattices of ``FactorizedReduce``
    (``bnn_hip_bn_train_backward_s2_f32``): ``g0[n, c, i, j]`` at ``(2i, 2j)``, ``g1`` at ``(2i+1, 2j+1)``, zero
    elsewhere -> ``(dx, dgamma, dbeta)`` with the full-resolution ``dx`` written in one pass."""
    g0 = _require_cuda_f32(g0, "grad_output")
    g1 = _require_cuda_f32(g1, "grad_output")
    x = _require_cuda_f32(x, "BatchNorm input")
    if x.dim() != 4 or x.shape[2] % 2 or x.shape[3] % 2:
        raise native.NativeError(f"bnn_amd: bn_train_backward_s2 expects NCHW with even H and W, got {tuple(x.shape)}")
    N, C, H, W = x.shape
    if tuple(g0.shape) != (N, C, H // 2, W // 2) or g1.shape != g0.shape:
        raise native.NativeError(f"bnn_amd: bn_train_backward_s2: grad_outputs {tuple(g0.shape)} / {tuple(g1.shape)} do not "
                                 f"belong to the NCHW input {tuple(x.shape)}")
    if x.data_ptr() % 8:        # (a view one float into its storage: the kernels move rows as float2)
        x = x.clone()
    mean, invstd, gamma = _bn_train_saved(C, mean, invstd, gamma)
    lib = native.require()
    with torch.cuda.device(x.device):
        dx = torch.empty_like(x)
        dgamma, dbeta, ws = _bn_train_buffers(lib, x)
        native.check(lib.bnn_hip_bn_train_backward_s2_f32(
            g0.data_ptr(), g1.data_ptr(), x.data_ptr(), mean.data_ptr(), invstd.data_ptr(), _ptr(gamma), N, C, H, W,
            dx.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), ws.data_ptr(), _stream(x.device)),
            "bnn_hip_bn_train_backward_s2_f32")
    return dx, dgamma, dbeta


def prelu_shuffle_backward(gy: torch.Tensor, z: torch.Tensor, slope: torch.Tensor, shuffle_groups: int = 1,
                           inplace: bool = False):
    """Backward of ``channel_shuffle(prelu(z, slope), shuffle_groups)`` (``bnn_hip_prelu_shuffle_backward_f32``):
    ``gy`` in the output's channel order, ``z`` in the convolution's -> ``(gz, dslope)``, ``dslope`` shaped like
    ``slope`` (1 or O values).  Deterministic.  ``inplace``: ``gz`` overwrites ``z``."""
    gy = _require_cuda_f32(gy, "grad_output")
    z = _require_cuda_f32(z, "pre-activation")
    if z.dim() != 4 or gy.shape != z.shape:
        raise native.NativeError(f"bnn_amd: prelu_shuffle_backward: grad_output {tuple(gy.shape)} does not belong to the "
                                 f"NCHW pre-activation {tuple(z.shape)}")
    N, O, H, W = z.shape
    slope = _require_cuda_f32(slope.detach(), "PReLU slope").reshape(-1)
    if slope.numel() not in (1, O):
        raise native.NativeError(f"bnn_amd: PReLU slope must have 1 or {O} entries, got {slope.numel()}")
    shuffle_groups = _shuffle_groups(shuffle_groups, O, "channels")
    lib = native.require()
    with torch.cuda.device(z.device):
        gz = z if inplace else torch.empty_like(z)
        dslope = torch.zeros_like(slope)
        if z.numel():
            nbytes = int(lib.bnn_hip_prelu_shuffle_backward_workspace_bytes(N, O, H * W))
            ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=z.device)
            native.check(lib.bnn_hip_prelu_shuffle_backward_f32(
                gy.data_ptr(), z.data_ptr(), slope.data_ptr(), slope.numel(), N, O, H * W, shuffle_groups, gz.data_ptr(),
                dslope.data_ptr(), ws.data_ptr(), nbytes, _stream(z.device)), "bnn_hip_prelu_shuffle_backward_f32")
    return gz, dslope


def bn_relu_maxpool_train_forward(x: torch.Tensor, gamma, beta, running_mean, running_var, momentum: float, eps: float):
    """``maxpool3x3/2/1(relu(batch_norm(x, training=True)))`` without writing the normalised tensor (csrc/bn_train.hip):
    returns ``(pooled, code uint8, save_mean, save_invstd)``; ``code`` = which of the 9 window positions won."""
    x = _nchw(x, "BatchNorm input", "bn_relu_maxpool_train_forward")
    lib = native.require()
    N, C, H, W = x.shape
    gamma, beta, running_mean, running_var = _bn_train_affine(C, gamma, beta, running_mean, running_var)
    hp, wp = _half_hw(H, W)
    with torch.cuda.device(x.device):
        p = torch.empty((N, C, hp, wp), dtype=torch.float32, device=x.device)
        code = torch.empty((N, C, hp, wp), dtype=torch.uint8, device=x.device)
        mean, invstd, ws = _bn_train_buffers(lib, x)
        native.check(lib.bnn_hip_bn_relu_maxpool_train_forward_f32(
            x.data_ptr(), N, C, H, W, _ptr(gamma), _ptr(beta), float(eps), float(momentum), _ptr(running_mean),
            _ptr(running_var), p.data_ptr(), code.data_ptr(), mean.data_ptr(), invstd.data_ptr(), ws.data_ptr(),
            _stream(x.device)), "bnn_hip_bn_relu_maxpool_train_forward_f32")
    return p, code, mean, invstd


def bn_relu_maxpool_train_backward(gy: torch.Tensor, p: torch.Tensor, code: torch.Tensor, x: torch.Tensor,
                                   mean: torch.Tensor, invstd: torch.Tensor, gamma):
    """Backward of ``bn_relu_maxpool_train_forward``: ``(dx, dgamma, dbeta)``."""
    x = _nchw(x, "BatchNorm input", "bn_relu_maxpool_train_backward")
    lib = native.require()
    N, C, H, W = x.shape
    pooled = (N, C) + _half_hw(H, W)
    gy, p = _shaped(gy, pooled, "grad_output"), _shaped(p, pooled, "pooled output")
    code = _shaped(code, pooled, "code", dtype=torch.uint8)
    mean, invstd, gamma = _bn_train_saved(C, mean, invstd, gamma)
    with torch.cuda.device(x.device):
        dx = torch.empty_like(x)
        dgamma, dbeta, ws = _bn_train_buffers(lib, x)
        native.check(lib.bnn_hip_bn_relu_maxpool_train_backward_f32(
            gy.data_ptr(), p.data_ptr(), code.data_ptr(), x.data_ptr(), mean.data_ptr(), invstd.data_ptr(), _ptr(gamma),
            N, C, H, W, dx.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), ws.data_ptr(), _stream(x.device)),
            "bnn_hip_bn_relu_maxpool_train_backward_f32")
    return dx, dgamma, dbeta


PROBE_MODES = {0: "bitop3+bcnt", 1: "xor+bcnt", 2: "bcnt", 3: "bitop3", 4: "xor", 5: "fma_f32",
               6: "add_u32", 7: "and_vgpr", 8: "and_vgpr+bcnt", 9: "xor_vgpr", 10: "and_sgpr+bcnt"}


def probe_clock(device: Optional[torch.device] = None, spin_iters: int = 10000) -> float:
    """Engine clock right now in MHz, sampled on the current stream of ``device`` (bnn_hip_probe_clock)."""
    lib = native.require()
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    mhz = ctypes.c_double()
    us = ctypes.c_double()
    with torch.cuda.device(dev):
        native.check(lib.bnn_hip_probe_clock(spin_iters, ctypes.byref(mhz), ctypes.byref(us), _stream(dev)),
                     "bnn_hip_probe_clock")
    return mhz.value


def probe_int_alu(iters: int = 4096, device: Optional[torch.device] = None, mode: int = 0) -> dict:
    """Sustained lane-ops/s of a register-only instruction stream (roofline calibration)."""
    lib = native.require()
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    rate = ctypes.c_double()
    ms = ctypes.c_double()
    with torch.cuda.device(dev):
        native.check(lib.bnn_hip_probe_int_alu(mode, iters, ctypes.byref(rate), ctypes.byref(ms),
                                               _stream(dev)), "bnn_hip_probe_int_alu")
    return {"lane_ops_per_s": rate.value, "elapsed_ms": ms.value}

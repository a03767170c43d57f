#!/usr/bin/env python3
"""Generate ``tests/golden/lowp_layers.npz``: the REFERENCE ``bnn.layers.Conv2d`` under ``torch.autocast("cpu", dtype=D)``
for D = bfloat16 and float16, on five small layers (tests/test_gpu_lowp.py, tests/test_lowp_cpu.py).

Runs only where the reference package is installed (``BNN_REFERENCE``); the test-suite reads the committed ``.npz``.  Nothing
of the reference's source is stored — only inputs and the reference's numeric outputs.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_lowp.py

Per case ``s<i>``: ``meta`` (the integers of ``FIELDS``), ``w`` / ``b`` / ``sc`` (fp32 weight, bias, post-scale; absent
when the layer has none), and per dtype name ``bf16`` / ``f16``: ``x_<D>`` (fp32 values already rounded to D, with +-0,
NaN, +-inf and the smallest subnormals of D among them) and ``out_<D>`` (the reference's output, int16 bit patterns).

The generator refuses to write unless (a) C / groups * k^2 <= 8192 — partial sums n * alpha_D stay exact in fp32, so no
reduction order can change the fp32 value that is rounded — and (b) every fp32 alpha lies farther than 2^-20 (relative)
from a rounding boundary of both 16-bit formats — so a last-bit difference of a device's alpha reduction cannot flip the
rounding of the weight.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFERENCE = os.environ.get("BNN_REFERENCE", "/root/reference")
OUT = os.path.join(HERE, "lowp_layers.npz")

FIELDS = ("C", "O", "k", "stride", "pad", "groups", "bias", "scale", "center", "N", "H", "W")
#        C    O   k  s  p  groups bias scale centred N  H  W
CASES = ((8, 6, 3, 1, 1, 1, 1, 1, 0, 2, 9, 7),
         (128, 40, 3, 2, 1, 1, 1, 1, 1, 2, 6, 5),
         (70, 37, 1, 1, 0, 1, 0, 0, 0, 2, 7, 5),
         (64, 64, 3, 1, 1, 64, 1, 1, 0, 2, 5, 7),
         (96, 96, 5, 1, 2, 8, 0, 1, 1, 2, 6, 5))
DTYPES = (("bf16", "bfloat16"), ("f16", "float16"))
MAX_TERMS = 8192
ALPHA_GUARD = 2.0 ** -20


def round_to(a: np.ndarray, name: str) -> np.ndarray:
    """fp32 -> the 16-bit format -> fp32 (round to nearest even), in numpy."""
    a = np.ascontiguousarray(a, np.float32)
    if name == "f16":
        with np.errstate(over="ignore"):
            return a.astype(np.float16).astype(np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    out = r.astype(np.uint32).view(np.float32)
    return np.where(np.isnan(a), np.float32(np.nan), out).astype(np.float32)


def boundary_distance(alpha: np.ndarray, name: str) -> np.ndarray:
    """Relative distance of each fp32 alpha to the nearest rounding boundary (midpoint of two neighbours) of the format."""
    a = alpha.astype(np.float64)
    lo = round_to(alpha, name).astype(np.float64)
    mant = 8 if name == "bf16" else 11
    ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(lo), 1e-300))) - (mant - 1))
    if name == "f16":
        ulp = np.maximum(ulp, 2.0 ** -24)       # the subnormal spacing of fp16
    return np.minimum(np.abs(a - (lo + ulp / 2)), np.abs(a - (lo - ulp / 2))) / np.abs(a)


def specials(name: str) -> np.ndarray:
    tiny = 2.0 ** -133 if name == "bf16" else 2.0 ** -24        # the smallest subnormal of the format
    return np.array([0.0, -0.0, np.nan, np.inf, -np.inf, tiny, -tiny], np.float32)


def case_tensors(i: int, case) -> dict:
    c = dict(zip(FIELDS, case))
    rng = np.random.default_rng(1000 + i)
    cg = c["C"] // c["groups"]
    w = (rng.standard_normal((c["O"], cg, c["k"], c["k"])) * 0.1).astype(np.float32)
    w = (w.view(np.uint32) & np.uint32(0xFFFFF000)).view(np.float32)     # 12 mantissa bits: a smaller file, any weight will do
    t = {"meta": np.array(case, np.int32), "w": w}
    if c["bias"]:
        t["b"] = rng.standard_normal(c["O"]).astype(np.float32)
    if c["scale"]:
        t["sc"] = (0.25 + 3.0 * rng.random(c["O"])).astype(np.float32)
    for name, _ in DTYPES:
        x = (rng.standard_normal((c["N"], c["C"], c["H"], c["W"])) * 2.0).astype(np.float32)
        sp = specials(name)
        pos = rng.random(x.shape) < 0.08
        x[pos] = sp[rng.integers(0, len(sp), int(pos.sum()))]
        t["x_" + name] = round_to(x, name)
    return t


def main() -> None:
    sys.dont_write_bytecode = True
    sys.path.insert(0, REFERENCE)
    import torch
    import torch.nn as nn

    import bnn  # the reference package
    from bnn.ops import BasicInputBinarizer, BasicScaleBinarizer, XNORWeightBinarizer

    assert os.path.realpath(bnn.__file__).startswith(os.path.realpath(REFERENCE)), bnn.__file__
    torch.set_num_threads(4)
    arrays = {}
    for i, case in enumerate(CASES):
        c = dict(zip(FIELDS, case))
        assert c["C"] // c["groups"] * c["k"] ** 2 <= MAX_TERMS, "partial sums would leave the exact range of fp32"
        t = case_tensors(i, case)
        conv = nn.Conv2d(c["C"], c["O"], c["k"], stride=c["stride"], padding=c["pad"], groups=c["groups"], bias=bool(c["bias"]))
        conv.weight.data.copy_(torch.from_numpy(t["w"]))
        if c["bias"]:
            conv.bias.data.copy_(torch.from_numpy(t["b"]))
        cfg = bnn.BConfig(activation_pre_process=BasicInputBinarizer,
                          activation_post_process=BasicScaleBinarizer if c["scale"] else bnn.Identity,
                          weight_pre_process=XNORWeightBinarizer.with_args(compute_alpha=True,
                                                                           center_weights=bool(c["center"])))
        layer = bnn.prepare_binary_model(conv, cfg)
        assert type(layer) is bnn.layers.Conv2d
        if c["scale"]:
            layer.activation_post_process.alpha.data.copy_(torch.from_numpy(t["sc"]).view(1, -1, 1, 1))
        layer.eval()
        with torch.no_grad():
            what = layer.weight_pre_process(layer.weight)
        alpha = what.abs().flatten(1).amax(1).numpy()
        for name, tname in DTYPES:
            dist = boundary_distance(alpha, name)
            assert (dist > ALPHA_GUARD).all(), f"case {i}: an alpha lies {dist.min():.3g} from a {name} rounding boundary"
            D = getattr(torch, tname)
            x = torch.from_numpy(t["x_" + name]).to(D)
            assert torch.equal(x.float().nan_to_num(7.0), torch.from_numpy(t["x_" + name]).nan_to_num(7.0))
            with torch.no_grad(), torch.autocast("cpu", dtype=D):
                out = layer(x)
            assert out.dtype == D
            t["out_" + name] = out.contiguous().view(torch.int16).numpy()
        for k, v in t.items():
            arrays[f"s{i}/{k}"] = v
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(arrays)} arrays")


if __name__ == "__main__":
    main()

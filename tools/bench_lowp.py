#!/usr/bin/env python3
"""A binary 3x3 convolution layer of a 16-bit network at batch 256 (bnn_amd/fastpath.py: lowp_dtype, csrc/bconv_fly.hip):
per shape and per 16-bit dtype D (bfloat16, float16), device-event times of four arms on the same D input under
``torch.autocast("cuda", dtype=D)`` semantics (fp32 weight, post-scale, no bias: a ResNet-18 layer)

  * a_composition : the torch composition in D — what such a layer ran before (sign, weight hook, library convolution in
                    D, in-place scale),
  * b_f32_store   : the one-launch HIP kernel with its fp32 store, then ``hipops.round_lowp`` (``.to(D)`` and ``mul_``),
  * c_16_store    : the one-launch HIP kernel with the in-kernel 16-bit store (BNN_HIP_FLAG_OUT_*): ONE launch,
  * d_f32_layer   : the fp32 HIP layer of today on the fp32 input (one launch, fp32 in, fp32 out), for scale,

taken in ONE process in ROUNDS alternating rounds (a, b, c, d, a, ...), the median round of each reported with the rounds.
``c`` and ``d`` are launches alone (one kernel and one ``torch.empty`` per call).  Byte bounds: input + output + packed
weights over 6.3 TB/s achievable HBM — 2 + 2 bytes per element for c, 4 + 4 for d.  ``c_equals_a``: the share of output
elements of c that equal the GPU composition a bit for bit (informative: where the library convolution rounds).  One JSON
line per shape and dtype.

A shape whose c measures SLOWER than its b belongs into fastpath.LOWP_STORE_DECLINED_SHAPES (the admission rule, stated
there): the line says so in "admit".

    python tools/bench_lowp.py [--iters 100] [--warmup 10] [--rounds 5] [--batch 256] [--only NAME] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "binary-networks-pytorch_amd")]

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

import bnn_amd as bnn  # noqa: E402
from bnn_amd import fastpath, hipops, native  # noqa: E402
from bnn_amd.ops import BasicInputBinarizer, BasicScaleBinarizer, XNORWeightBinarizer  # noqa: E402
from tests.golden import gen  # noqa: E402

HBM_BYTES_PER_S = 6.3e12            # achievable HBM bandwidth (MI355X_MICROARCH)

SHAPES = [  # name, C, O, H = W, stride: the four stride-1 3x3 layer shapes of ResNet-18 and one stride-2 shape
    ("l1_64x56", 64, 64, 56, 1),
    ("l2_128x28", 128, 128, 28, 1),
    ("l3_256x14", 256, 256, 14, 1),
    ("l4_512x7", 512, 512, 7, 1),
    ("l2_0_64x56_s2", 64, 128, 56, 2),
]
DTYPES = [("bf16", torch.bfloat16), ("f16", torch.float16)]


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters   # us


def commit() -> str:
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        return "unknown"


def same_bits_share(a: torch.Tensor, b: torch.Tensor) -> float:
    """Share of elements with equal int16 patterns (two NaNs count as equal); an exact 1.0 means none differs."""
    nan = torch.isnan(a) & torch.isnan(b)
    differ = int(((a.view(torch.int16) != b.view(torch.int16)) & ~nan).sum())
    return (a.numel() - differ) / a.numel()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="revision to record (default: git rev-parse --short HEAD)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lowp.py needs a HIP device: nothing is measured without one")
    dev = torch.device("cuda:0")
    info = native.device_info(0)
    cfg = bnn.BConfig(activation_pre_process=BasicInputBinarizer, activation_post_process=BasicScaleBinarizer,
                      weight_pre_process=XNORWeightBinarizer)
    rev = args.commit or commit()
    lines = []
    for name, C, O, HW, s in SHAPES:
        if args.only and args.only not in name:
            continue
        N = args.batch
        x32 = torch.from_numpy(gen.activation("normal", gen.seed_of("bench-lowp", name), (8, C, HW, HW))).to(dev)
        x32 = x32.repeat(N // 8, 1, 1, 1)
        layer = bnn.prepare_binary_model(nn.Conv2d(C, O, 3, stride=s, padding=1, bias=False), cfg)
        shapes = {k: tuple(v.shape) for k, v in layer.state_dict().items()}
        state = {k: torch.from_numpy(v) for k, v in gen.model_state(shapes, gen.seed_of("bench-lowp", name)).items()}
        state["activation_post_process.alpha"] = 0.5 + torch.rand(shapes["activation_post_process.alpha"],
                                                                  generator=torch.Generator().manual_seed(1))
        layer.load_state_dict(state)
        layer = layer.to(dev).eval()
        geo = (layer.stride, layer.padding, layer.dilation)
        for dname, D in DTYPES:
            x = x32.to(D)
            with torch.no_grad():
                plan = fastpath.plan_conv2d(layer, x32)
                pw32 = fastpath.packed_weight(layer, plan)
                with torch.autocast("cuda", dtype=D):
                    assert fastpath.lowp_dtype(layer, x) is D
                    before = fastpath.stats()["conv2d"]
                    y_layer = layer(x)
                    assert fastpath.stats()["conv2d"] == before + 1 and y_layer.dtype == D
                pw, bias = fastpath.lowp_packed_weight(layer, plan, D)
                scale = plan.scale.detach().float()

                def a_composition():
                    old = fastpath._eligible
                    fastpath._eligible = lambda *a: False
                    try:
                        with torch.autocast("cuda", dtype=D):
                            return layer(x)
                    finally:
                        fastpath._eligible = old

                def b_f32_store():
                    return hipops.round_lowp(hipops.bconv2d_direct(x, pw, bias, None, *geo, route="direct"), scale, D)

                def c_16_store():
                    return hipops.bconv2d_direct(x, pw, bias, scale, *geo, route="direct", out_dtype=D)

                def d_f32_layer():
                    return hipops.bconv2d_direct(x32, pw32, None, scale, *geo, route="direct")

                ya, yb, yc = a_composition(), b_f32_store(), c_16_store()
                assert ya.dtype == yb.dtype == yc.dtype == D
                c_equals_b = same_bits_share(yc, yb)
                assert c_equals_b == 1.0 and same_bits_share(yc, y_layer) == 1.0, "the two HIP forms differ"
                c_equals_a = same_bits_share(yc, ya)
                legs = {"a_composition": a_composition, "b_f32_store": b_f32_store, "c_16_store": c_16_store,
                        "d_f32_layer": d_f32_layer}
                for fn in legs.values():
                    for _ in range(args.warmup):
                        fn()
                times = {k: [] for k in legs}
                for _ in range(args.rounds):
                    for k, fn in legs.items():      # alternating: every round times each leg once
                        times[k].append(timed(fn, args.iters))
            med = {k: statistics.median(v) for k, v in times.items()}
            wbytes = (pw.wbits.numel() + pw.wnz.numel() * int(pw.has_zero)) * 4
            c_bytes = x.numel() * 2 + yc.numel() * 2 + wbytes
            d_bytes = x32.numel() * 4 + yc.numel() * 4 + wbytes
            c_bound, d_bound = c_bytes / HBM_BYTES_PER_S * 1e6, d_bytes / HBM_BYTES_PER_S * 1e6
            rec = dict(op=name, dtype=dname, commit=rev, N=N, C=C, O=O, HW=[HW, HW], stride=s, out=list(yc.shape[1:]),
                       **{k + "_us": round(v, 2) for k, v in med.items()},
                       **{k + "_us_rounds": [round(t, 2) for t in v] for k, v in times.items()},
                       admit=bool(med["c_16_store"] <= med["b_f32_store"]),
                       store_declined_in_table=not fastpath.lowp_store_admitted(D, C, O, HW, HW, 3, s),
                       speedup_c_vs_a=round(med["a_composition"] / med["c_16_store"], 2),
                       speedup_c_vs_b=round(med["b_f32_store"] / med["c_16_store"], 2),
                       c_byte_bound_us=round(c_bound, 2), c_fraction_of_byte_bound=round(c_bound / med["c_16_store"], 3),
                       d_byte_bound_us=round(d_bound, 2), d_fraction_of_byte_bound=round(d_bound / med["d_f32_layer"], 3),
                       c_equals_b=c_equals_b, c_equals_a=round(c_equals_a, 6),
                       max_rel_diff_c_vs_a=float((yc.float() - ya.float()).abs().max() / ya.float().abs().max()),
                       iters=args.iters, warmup=args.warmup, rounds=args.rounds,
                       device=info["name"], clock_mhz=info["clock_khz"] / 1e3)
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

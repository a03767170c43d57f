#!/usr/bin/env python3
"""Grouped / depthwise binary convolutions at batch 256 (csrc/bconv_grouped.hip): per shape, device-event times over
ITERS iterations after a warm-up of

  * kernel : bnn_hip_bconv2d_grouped alone on packed planes,
  * layer  : the HIP layer forward (bnn_amd Conv2d(groups=G) under no_grad: pack_act + the grouped kernel),
  * torch  : the composition that layer ran before (sign(x) -> XNORWeightBinarizer(W) -> F.conv2d(groups=G)),

and the kernel's share of the binding bound: the lane-op bound (2 ceil(Cg KH KW / 32) 32-bit lane operations per output
element over CUs x 64 x clock, as tools/bench_conv.py counts) and the byte bound (both sign planes in + fp32 out over
6.3 TB/s achievable HBM).  One JSON line per shape.

    python tools/bench_grouped.py [--iters 200] [--warmup 20] [--batch 256] [--only NAME] [--out FILE]
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "binary-networks-pytorch_amd")]

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import bnn_amd as bnn  # noqa: E402
from bnn_amd import fastpath, hipops, native  # noqa: E402
from bnn_amd.ops import BasicInputBinarizer, XNORWeightBinarizer  # noqa: E402
from tests.golden import gen  # noqa: E402

HBM_BYTES_PER_S = 6.3e12   # achievable HBM bandwidth (MI355X_MICROARCH)

SHAPES = [  # name, C, O, G, H, W, k, stride, pad, dilation
    ("sepconv_3x3_c96_g12_32", 96, 96, 12, 32, 32, 3, 1, 1, 1),
    ("k5_c192_g12_16", 192, 192, 12, 16, 16, 5, 1, 2, 1),
    ("dilconv_3x3_d2_c384_g12_8", 384, 384, 12, 8, 8, 3, 1, 2, 2),
    ("stem_3x3_s2_40to80_g4_112", 40, 80, 4, 112, 112, 3, 2, 1, 1),
    ("depthwise_3x3_c256_14", 256, 256, 256, 14, 14, 3, 1, 1, 1),
    ("og2cg_3x3_64to128_g4_28", 64, 128, 4, 28, 28, 3, 1, 1, 1),
]


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters   # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    info = native.device_info(0)
    lane_ops_per_s = info["compute_units"] * 64 * info["clock_khz"] * 1e3
    cfg = bnn.BConfig(activation_pre_process=BasicInputBinarizer, activation_post_process=bnn.Identity,
                      weight_pre_process=XNORWeightBinarizer)
    lines = []
    for name, C, O, G, H, W, k, s, p, d in SHAPES:
        if args.only and args.only not in name:
            continue
        N = args.batch
        x = torch.from_numpy(gen.activation("normal", gen.seed_of("bench-grouped", name), (8, C, H, W))).to(dev)
        x = x.repeat(N // 8, 1, 1, 1)
        layer = bnn.prepare_binary_model(nn.Conv2d(C, O, k, s, p, d, groups=G, bias=False), cfg)
        layer.weight.data.copy_(torch.from_numpy(gen.conv_weight("kaiming", 5, (O, C // G, k, k))))
        layer = layer.to(dev).eval()
        w = layer.weight.detach()
        act = hipops.pack_act(x)
        pw = hipops.pack_weight_grouped(w, G)
        wpre = XNORWeightBinarizer()
        with torch.no_grad():
            before = fastpath.stats()["conv2d"]
            y = layer(x)
            assert fastpath.stats()["conv2d"] == before + 1, "the layer did not take the HIP path"
            ref = F.conv2d(torch.sign(x), wpre(w), None, s, p, d, G)
            err = float((y - ref).abs().max() / ref.abs().max())
            t_kernel = timed(lambda: hipops.bconv2d_grouped(act, pw, stride=s, padding=p, dilation=d), args.iters,
                             args.warmup)
            t_layer = timed(lambda: layer(x), args.iters, args.warmup)
            t_torch = timed(lambda: F.conv2d(torch.sign(x), wpre(w), None, s, p, d, G), args.iters, args.warmup)
        Ho, Wo = y.shape[2], y.shape[3]
        outs = N * O * Ho * Wo
        Cg = C // G
        ops = outs * 2 * math.ceil(Cg * k * k / 32)
        t_ops = ops / lane_ops_per_s * 1e6
        nbytes = 2 * N * ((C + 63) // 64) * H * W * 8 + outs * 4
        t_bytes = nbytes / HBM_BYTES_PER_S * 1e6
        bound, which = (t_ops, "lane_ops") if t_ops > t_bytes else (t_bytes, "bytes")
        rec = dict(shape=name, N=N, C=C, O=O, groups=G, HW=[H, W], k=k, stride=s, pad=p, dilation=d, out_hw=[Ho, Wo],
                   words_per_tap=native.grouped_weight_layout(O, C, G, k, k).cw32,
                   kernel_us=round(t_kernel, 2), layer_us=round(t_layer, 2), torch_us=round(t_torch, 2),
                   layer_speedup_vs_torch=round(t_torch / t_layer, 2),
                   lane_op_bound_us=round(t_ops, 2), byte_bound_us=round(t_bytes, 2), binding=which,
                   kernel_fraction_of_bound=round(bound / t_kernel, 3), max_rel_err_vs_torch=err,
                   iters=args.iters, warmup=args.warmup, device=info["name"], clock_mhz=info["clock_khz"] / 1e3)
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The BATS cell operations at batch 256 (bnn_amd/cellops.py, csrc/bconv_grouped.hip): per operation, device-event
times over ITERS iterations after a warm-up of

  * fused     : op(x) under eval() / no_grad() — bn_act_pack + one convolution launch with PReLU, shuffle and skip,
  * per_layer : the same module inside per_layer_forward() — torch BatchNorm, pack_act, the grouped kernel, torch
                PReLU, the shuffle copy, the add (the path every call took before the cell executor),
  * kernel    : the fused convolution launch alone on ready planes,

and the byte bound of the two fused launches: x read twice (by the pack and as the skip; once without a skip), y written
once, both sign planes written and read, over 6.3 TB/s achievable HBM.  One JSON line per operation.

    python tools/bench_cellops.py [--iters 200] [--warmup 20] [--batch 256] [--only NAME] [--out FILE] [--commit REV]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "binary-networks-pytorch_amd")]

import torch  # noqa: E402

import bnn_amd as bnn  # noqa: E402
from bnn_amd import fastpath, models, native  # noqa: E402
from bnn_amd.inference import OpFusion, per_layer_forward  # noqa: E402
from bnn_amd.ops import BasicInputBinarizer, XNORWeightBinarizer  # noqa: E402
from tests.golden import gen  # noqa: E402

HBM_BYTES_PER_S = 6.3e12   # achievable HBM bandwidth (MI355X_MICROARCH)

OPS = [  # name, constructor, C, H = W
    ("sepconv_3x3_c96_32", lambda: models.SepConv(96, 96, 3, 1, 1, groups=12), 96, 32),
    ("sepconv_5x5_c192_16", lambda: models.SepConv(192, 192, 5, 1, 2, groups=12), 192, 16),
    ("dilconv_3x3_d2_c384_8", lambda: models.DilConv(384, 384, 3, 1, 2, 2, groups=12), 384, 8),
    ("reluconvbn_1x1_c96_32", lambda: models.ReLUConvBN(96, 96, 1, 1, 0), 96, 32),
    ("sepconv_3x3_s2_c96_32", lambda: models.SepConv(96, 96, 3, 2, 1, groups=12), 96, 32),
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


def commit() -> str:
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="revision to record (default: git rev-parse --short HEAD)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    info = native.device_info(0)
    cfg = bnn.BConfig(activation_pre_process=BasicInputBinarizer, activation_post_process=bnn.Identity,
                      weight_pre_process=XNORWeightBinarizer)
    rev = args.commit or commit()
    lines = []
    for name, make, C, HW in OPS:
        if args.only and args.only not in name:
            continue
        N = args.batch
        x = torch.from_numpy(gen.activation("normal", gen.seed_of("bench-cellops", name), (8, C, HW, HW))).to(dev)
        x = x.repeat(N // 8, 1, 1, 1)
        op = bnn.prepare_binary_model(make(), cfg)
        shapes = {k: tuple(v.shape) for k, v in op.state_dict().items()}
        op.load_state_dict({k: torch.from_numpy(v) for k, v in gen.model_state(shapes, gen.seed_of(name)).items()})
        op = op.to(dev).eval()
        with torch.no_grad():
            before = fastpath.stats()["cell_op"]
            y = op(x)
            assert fastpath.stats()["cell_op"] == before + 1, "the operation did not take the fused path"
            with per_layer_forward():
                ref = op(x)
                assert fastpath.stats()["cell_op"] == before + 1
            err = float((y - ref).abs().max() / ref.abs().max())
            eng = OpFusion.of(op).engine
            conv = op.op[1]
            act = eng.pack(x)
            res = x if eng.add_skip else None

            def kernel():
                return eng.conv(act, x)
            t_fused = timed(lambda: op(x), args.iters, args.warmup)
            with per_layer_forward():
                t_layer = timed(lambda: op(x), args.iters, args.warmup)
            t_kernel = timed(kernel, args.iters, args.warmup)
        planes = 2 * N * ((C + 63) // 64) * HW * HW * 8
        nbytes = x.numel() * 4 * (2 if res is not None else 1) + y.numel() * 4 + 2 * planes
        t_bytes = nbytes / HBM_BYTES_PER_S * 1e6
        kbytes = planes + y.numel() * 4 * (2 if res is not None else 1)     # the convolution launch alone
        t_kbytes = kbytes / HBM_BYTES_PER_S * 1e6
        rec = dict(op=name, commit=rev, N=N, C=C, HW=[HW, HW], out=list(y.shape[1:]), groups=conv.groups,
                   skip=res is not None, fused_us=round(t_fused, 2), per_layer_us=round(t_layer, 2),
                   kernel_us=round(t_kernel, 2), speedup_vs_per_layer=round(t_layer / t_fused, 2),
                   byte_bound_us=round(t_bytes, 2), fused_fraction_of_byte_bound=round(t_bytes / t_fused, 3),
                   kernel_byte_bound_us=round(t_kbytes, 2), kernel_fraction_of_byte_bound=round(t_kbytes / t_kernel, 3),
                   max_rel_diff_vs_per_layer=err, iters=args.iters, warmup=args.warmup, device=info["name"],
                   clock_mhz=info["clock_khz"] / 1e3)
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

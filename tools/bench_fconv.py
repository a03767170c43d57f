#!/usr/bin/env python3
"""FactorizedConv ('conv_7x1_1x7') at batch 256 (bnn_amd/cellops.py: FusedFactorizedConv, csrc/fconv.hip): per shape,
device-event times of

  * fused     : op(x) under eval() / no_grad() — bn_act_pack + ONE launch for both convolutions (the sign between them in
                LDS), PReLU, shuffle and skip in its epilogue,
  * per_layer : the same module inside per_layer_forward() — two torch BatchNorms, two pack_act + shape-generic binary
                convolution launches, two torch PReLUs, the shuffle copy, the add: the kernels every call took before,
  * kernel    : the fused launch alone on ready planes,
  * composition: the executor's fallback (pack + two bconv2d_fused launches + torch shuffle and add),

taken in ONE process in ROUNDS alternating rounds (fused, per_layer, ...), the median round of each reported with the
spread.  Bounds: the three-pass byte bound — x read by the pack and as the skip (once without a skip), y written, both
sign planes written and read — over 6.3 TB/s achievable HBM; the integer-ALU bound — two vector instructions (bitop3 +
bcnt) per 32 input channels, tap and output element of both convolutions, halo rows not counted — over 39.32e12 lane
operations per second.  One JSON line per shape.

A shape whose fused leg measures SLOWER than its per-layer leg belongs into fastpath.FCONV_DECLINED_SHAPES (the
admission rule, stated there): the line says so in "admit".

    python tools/bench_fconv.py [--iters 100] [--warmup 10] [--rounds 5] [--batch 256] [--only NAME] [--out FILE]
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

import bnn_amd as bnn  # noqa: E402
from bnn_amd import fastpath, models, native  # noqa: E402
from bnn_amd.inference import FactorizedFusion, per_layer_forward  # noqa: E402
from bnn_amd.ops import BasicInputBinarizer, XNORWeightBinarizer  # noqa: E402
from tests.golden import gen  # noqa: E402

HBM_BYTES_PER_S = 6.3e12            # achievable HBM bandwidth (MI355X_MICROARCH)
INT_ALU_LANE_OPS_PER_S = 39.32e12   # 256 CUs x 64 lanes x 2.4 GHz

SHAPES = [  # name, C, H = W, stride: the CIFAR network's three widths, its two reductions, and C 80 at 28 x 28
    ("c48_32", 48, 32, 1),
    ("c96_16", 96, 16, 1),
    ("c192_8", 192, 8, 1),
    ("c96_32_s2", 96, 32, 2),
    ("c192_16_s2", 192, 16, 2),
    ("c80_28", 80, 28, 1),
]


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
        raise SystemExit("bench_fconv.py needs a HIP device: nothing is measured without one")
    dev = torch.device("cuda:0")
    info = native.device_info(0)
    cfg = bnn.BConfig(activation_pre_process=BasicInputBinarizer, activation_post_process=bnn.Identity,
                      weight_pre_process=XNORWeightBinarizer)
    rev = args.commit or commit()
    lines = []
    for name, C, HW, s in SHAPES:
        if args.only and args.only not in name:
            continue
        N, K = args.batch, 7
        x = torch.from_numpy(gen.activation("normal", gen.seed_of("bench-fconv", name), (8, C, HW, HW))).to(dev)
        x = x.repeat(N // 8, 1, 1, 1)
        op = bnn.prepare_binary_model(models.FactorizedConv(C, K, s), cfg)
        shapes = {k: tuple(v.shape) for k, v in op.state_dict().items()}
        op.load_state_dict({k: torch.from_numpy(v) for k, v in gen.model_state(shapes, gen.seed_of(name)).items()})
        op = op.to(dev).eval()
        with torch.no_grad():
            before = fastpath.stats()["fconv"]
            y = op(x)
            eng = FactorizedFusion.of(op).engine
            took_kernel = fastpath.stats()["fconv"] == before + 1
            with per_layer_forward():
                ref = op(x)
            err = float((y - ref).abs().max() / ref.abs().max())
            planes = eng.pack(x)
            assert torch.equal(eng.conv(planes, x), eng.composition(planes, x)), "kernel and composition differ"

            def per_layer():
                with per_layer_forward():
                    return op(x)
            # (a shape the admission rule declines is still measured through the kernel: that is how it gets re-admitted)
            legs = {"fused": (lambda: op(x)) if took_kernel else (lambda: eng.conv(eng.pack(x), x)), "per_layer": per_layer,
                    "kernel": lambda: eng.conv(planes, x), "composition": lambda: eng.composition(eng.pack(x), x)}
            for fn in legs.values():
                for _ in range(args.warmup):
                    fn()
            times = {k: [] for k in legs}
            for _ in range(args.rounds):
                for k, fn in legs.items():      # alternating: every round times each leg once
                    times[k].append(timed(fn, args.iters))
        med = {k: statistics.median(v) for k, v in times.items()}
        Ho = Wm = (HW - 1) // s + 1
        skip = s == 1
        plane_bytes = 2 * N * ((C + 63) // 64) * HW * HW * 8
        nbytes = x.numel() * 4 * (2 if skip else 1) + y.numel() * 4 + 2 * plane_bytes
        t_bytes = nbytes / HBM_BYTES_PER_S * 1e6
        words = (C + 31) // 32
        lane_ops = 2.0 * words * K * N * C * (HW * Wm + Ho * Wm)
        t_alu = lane_ops / INT_ALU_LANE_OPS_PER_S * 1e6
        rec = dict(op=name, commit=rev, N=N, C=C, HW=[HW, HW], K=K, stride=s, out=list(y.shape[1:]), skip=skip,
                   executor_takes_kernel=took_kernel,
                   fused_us=round(med["fused"], 2), per_layer_us=round(med["per_layer"], 2),
                   kernel_us=round(med["kernel"], 2), composition_us=round(med["composition"], 2),
                   fused_us_rounds=[round(t, 2) for t in times["fused"]],
                   per_layer_us_rounds=[round(t, 2) for t in times["per_layer"]],
                   speedup_vs_per_layer=round(med["per_layer"] / med["fused"], 2),
                   speedup_vs_composition=round(med["composition"] / med["fused"], 2),
                   admit=bool(med["fused"] <= med["per_layer"]),
                   byte_bound_us=round(t_bytes, 2), fused_fraction_of_byte_bound=round(t_bytes / med["fused"], 3),
                   int_alu_bound_us=round(t_alu, 2), kernel_fraction_of_int_alu_bound=round(t_alu / med["kernel"], 3),
                   bound="int_alu" if t_alu > t_bytes else "bytes",
                   max_rel_diff_vs_per_layer=err, iters=args.iters, warmup=args.warmup, rounds=args.rounds,
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

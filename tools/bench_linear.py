#!/usr/bin/env python3
"""Binary Linear layers on the MI355X (csrc/blinear.hip), forward and training step, one JSON line per row.

Forward, per shape (M, F, O), device-event times over ITERS calls after a warm-up, under torch.no_grad():

  * torch   : the layer's torch composition — sign(x), the weight hook's torch kernels, the library's fp32 GEMM,
  * conv    : the route every Linear took before the row-major kernel: bconv2d_direct on M images of 1 x 1 pixels
              (hipops.linear(route="conv"): pack_act + the 1x1 convolution kernel, or the one-launch layer),
  * blinear : the row-major XNOR GEMM kernel (hipops.linear(route="blinear"): bnn_hip_blinear_direct, one launch),

conv and blinear alternating in one process (conv, blinear, conv, blinear: each reported as the pair of its two runs),
their outputs compared bit for bit first, each with its fraction of the integer-ALU roofline as the project counts it
(2 M O ceil(F/32) lane-operations over 39.32e12 per second), and what the dispatcher picks (hipops.blinear_preferred).

Training, forward + backward of the layer on the three large shapes: the composition (training.LINEAR off) and the HIP
path (on), alternating (off, on, off, on), with torch.cuda.max_memory_allocated of one step each way; and the two gradient
kernels alone next to the library's fp32 GEMMs on the same operands (g @ What and g^T @ sign(x)).

    python tools/bench_linear.py [--iters 20] [--warmup 5] [--only M,F,O] [--sweep] [--commit ID] [--out FILE] [--dry]
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "binary-networks-pytorch_amd")]

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

import bnn_amd as bnn  # noqa: E402
from bnn_amd import fastpath, hipops, training  # noqa: E402
from bnn_amd.ops import BasicInputBinarizer, XNORWeightBinarizer  # noqa: E402
from tests.golden import gen  # noqa: E402

INT_ALU_LANE_OPS_PER_S = 39.32e12
SHAPES = [(256, 512, 1000),            # a classifier head
          (32, 4096, 4096),            # small batch
          (8192, 1024, 1024),
          (50176, 768, 3072),          # an FFN at 256 x 196 tokens
          (50176, 3072, 768)]
TRAIN_SHAPES = SHAPES[2:]
# --sweep: forward rows between the table's shapes, to place the dispatcher's threshold (hipops.blinear_preferred)
SWEEP_SHAPES = [(1024, 1024, 1024), (4096, 768, 3072), (16384, 1024, 1024), (16384, 768, 3072), (16384, 3072, 768),
                (32768, 1024, 1024), (32768, 256, 256)]


def source_id(commit):
    """What the numbers belong to: the commit given (or HEAD where this is a git checkout) and a hash of the kernels."""
    if commit is None:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True,
                                    text=True, check=True).stdout.strip()
            dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain", "-uno"], capture_output=True,
                                   text=True).stdout.strip()
            commit += "+changes" if dirty else ""
        except Exception:
            commit = "unknown"
    src = open(os.path.join(ROOT, "binary-networks-pytorch_amd", "csrc", "blinear.hip"), "rb").read()
    return commit, hashlib.sha256(src).hexdigest()[:16]


def timed(fn, iters, warmup):
    """us per call: device events around `iters` calls after `warmup`."""
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def roofline_us(M, F, O):
    return 2.0 * M * O * ((F + 31) // 32) / INT_ALU_LANE_OPS_PER_S * 1e6


def make_layer(F, O, dev):
    cfg = bnn.BConfig(activation_pre_process=BasicInputBinarizer, activation_post_process=bnn.Identity,
                      weight_pre_process=XNORWeightBinarizer)
    layer = bnn.prepare_binary_model(nn.Linear(F, O, bias=True), cfg)
    layer.weight.data.copy_(torch.from_numpy(gen.normal(gen.seed_of("bench-linear-w", F, O), (O, F))) * 0.05)
    return layer.to(dev)


def make_input(M, F, dev):
    base = torch.from_numpy(gen.normal(gen.seed_of("bench-linear-x", F), (min(M, 64), F)) * 0.8).float().to(dev)
    return base.repeat((M + 63) // 64, 1)[:M].contiguous()


def forward_line(M, F, O, args, dev, stamp):
    layer = make_layer(F, O, dev).eval()
    x = make_input(M, F, dev)
    pw = hipops.pack_weight(layer.weight.detach())
    bias = layer.bias.detach()
    with torch.no_grad():
        a, b = hipops.linear(x, pw, bias, None, route="conv"), hipops.linear(x, pw, bias, None, route="blinear")
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "the two routes differ"

        def composition():
            return layer.activation_post_process(
                torch.nn.functional.linear(layer.activation_pre_process(x), layer.weight_pre_process(layer.weight), bias), x)
        t_torch = timed(composition, args.iters, args.warmup)
        conv, blin = [], []
        for _ in range(2):
            conv.append(round(timed(lambda: hipops.linear(x, pw, bias, None, route="conv"), args.iters, args.warmup), 2))
            blin.append(round(timed(lambda: hipops.linear(x, pw, bias, None, route="blinear"), args.iters, args.warmup), 2))
    roof = roofline_us(M, F, O)
    return dict(stamp, kind="forward", M=M, F=F, O=O, torch_us=round(t_torch, 2), conv_us=conv, blinear_us=blin,
                int_alu_roofline_us=round(roof, 2), conv_roofline_fraction=round(roof / min(conv), 4),
                blinear_roofline_fraction=round(roof / min(blin), 4), blinear_over_conv=round(min(blin) / min(conv), 4),
                dispatcher_picks_blinear=bool(hipops.blinear_preferred(M, F, O)))


def train_line(M, F, O, args, dev, stamp):
    layer = make_layer(F, O, dev).train()
    x = make_input(M, F, dev).requires_grad_()
    g = torch.from_numpy(gen.normal(3, (64, O))).float().to(dev).repeat((M + 63) // 64, 1)[:M].contiguous()

    def step():
        layer.weight.grad = layer.bias.grad = x.grad = None
        layer(x).backward(g)

    off, on, mem = [], [], {}
    for _ in range(2):
        for flag, dst in ((False, off), (True, on)):
            training.LINEAR = flag
            try:
                n0 = fastpath.stats()["linear_train"]
                dst.append(round(timed(step, args.iters, args.warmup), 2))
                assert (fastpath.stats()["linear_train"] > n0) == flag
                layer.weight.grad = layer.bias.grad = x.grad = None
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                step()
                torch.cuda.synchronize()
                mem["on" if flag else "off"] = [int(torch.cuda.max_memory_allocated()), int(base)]
            finally:
                training.LINEAR = False
    # the two gradient kernels alone, next to the library's fp32 GEMMs on the same operands
    with torch.no_grad():
        pw = hipops.pack_weight(layer.weight.detach())
        _, sv = hipops.blinear_direct(x.detach(), pw, want_planes=True)
        what = hipops.xnor_what(layer.weight.detach(), False, True)
        sx = torch.sign(x.detach())
        t_dgrad = timed(lambda: hipops.blinear_grad_input(g, sv, pw), args.iters, args.warmup)
        t_wgrad = timed(lambda: hipops.blinear_grad_weight(g, sv, reduce=False), args.iters, args.warmup)
        t_fwd_planes = timed(lambda: hipops.blinear_direct(x.detach(), pw, want_planes=True), args.iters, args.warmup)
        t_lib_d = timed(lambda: g @ what, args.iters, args.warmup)
        t_lib_w = timed(lambda: g.t() @ sx, args.iters, args.warmup)
        splits = hipops.blinear_grad_weight_splits(M, O, F)
    return dict(stamp, kind="train", M=M, F=F, O=O, composition_us=off, hip_us=on,
                hip_over_composition=round(min(on) / min(off), 4), max_memory_allocated=mem,
                forward_with_planes_us=round(t_fwd_planes, 2), dgrad_us=round(t_dgrad, 2), wgrad_us=round(t_wgrad, 2),
                wgrad_splits=splits, library_gemm_dgrad_us=round(t_lib_d, 2), library_gemm_wgrad_us=round(t_lib_w, 2),
                saved_input_bytes_hip=3 * 8 * M * ((F + 63) // 64), saved_input_bytes_composition=8 * M * F)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default=None, help="M,F,O")
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sweep", action="store_true", help="also the forward rows of SWEEP_SHAPES (kind forward_sweep)")
    ap.add_argument("--dry", action="store_true", help="list the rows and their rooflines; no device needed")
    args = ap.parse_args()
    only = tuple(int(v) for v in args.only.split(",")) if args.only else None
    commit, src = source_id(args.commit)
    if args.dry:
        for s in SHAPES:
            print(json.dumps(dict(kind="forward", shape=s, int_alu_roofline_us=round(roofline_us(*s), 2), train=s in TRAIN_SHAPES)))
        return
    assert torch.cuda.is_available(), "bench_linear.py measures on a HIP device"
    dev = torch.device("cuda:0")
    stamp = dict(commit=commit, blinear_hip_sha256=src, device=torch.cuda.get_device_name(0), iters=args.iters)
    out = open(args.out, "a") if args.out else None
    rows = [("forward", SHAPES, forward_line), ("train", TRAIN_SHAPES, train_line)]
    if args.sweep:
        rows.insert(1, ("forward_sweep", SWEEP_SHAPES, forward_line))
    for kind, shapes, fn in rows:
        for s in shapes:
            if only and s != only:
                continue
            line = json.dumps(dict(fn(*s, args, dev, stamp), kind=kind))
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
            torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()

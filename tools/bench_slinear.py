#!/usr/bin/env python3
"""Linear with binary activations and real weights (csrc/slinear.hip) on the MI355X against the torch composition, one
JSON line per shape.

The yardstick is the composition ``F.linear(sign(x), W, b) * alpha`` with ``fastpath.REAL_WEIGHTS`` off, in the same
process; both sides alternate (off, on, off, on: each reported as the pair of its two runs), device-event times over ITERS
calls after a warm-up, outputs compared first.

Per shape (M rows, F features, O output channels):

  * forward under ``torch.no_grad()`` (eval: the cached weight fragments) and forward + backward of a training step, with
    ``torch.cuda.max_memory_allocated`` of a training step each way,
  * the forward's share of the matrix-pipe bound: 2 * 3 * MACs (three bf16 MFMAs per product) over the bf16 dense peak,
    and of its byte bound: x, out and the weight fragments once over the HBM rate,
  * the two halves of the backward alone — gx (the library's ``g @ W`` + the mask kernel) and gW (the weight-gradient
    kernel of csrc/blinear.hip) — and the share of ``torch.mm`` in their sum.

    python tools/bench_slinear.py [--iters 20] [--warmup 5] [--only M,F,O] [--commit ID] [--out FILE]
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
from bnn_amd import fastpath, hipops  # noqa: E402
from bnn_amd.ops import BasicInputBinarizer, BasicScaleBinarizer  # noqa: E402

BF16_DENSE_PEAK = 2.5e15          # FLOP/s, MI355X spec (v_mfma_f32_16x16x32_bf16)
HBM_PEAK = 8.0e12                 # bytes/s, MI355X spec
SHAPES = [(8192, 1024, 1024), (50176, 768, 3072), (50176, 3072, 768), (1024, 1024, 1024), (256, 512, 1000)]


def source_id(commit):
    """What the numbers belong to: the commit given (or HEAD where this is a git checkout) and a hash of the kernel."""
    if commit is None:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True,
                                    text=True, check=True).stdout.strip()
            dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain", "-uno"], capture_output=True,
                                   text=True).stdout.strip()
            commit += "+changes" if dirty else ""
        except Exception:
            commit = "unknown"
    src = open(os.path.join(ROOT, "binary-networks-pytorch_amd", "csrc", "slinear.hip"), "rb").read()
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


def alternate(fn, iters, warmup):
    """{'off': [us, us], 'on': [us, us]}: fn() with the switch off, on, off, on."""
    out = {"off": [], "on": []}
    for _ in range(2):
        for key in ("off", "on"):
            fastpath.REAL_WEIGHTS = key == "on"
            out[key].append(round(timed(fn, iters, warmup), 2))
    fastpath.REAL_WEIGHTS = False
    return out


def bench_shape(M, F, O, iters, warmup, dev):
    torch.manual_seed(0)
    cfg = bnn.BConfig(activation_pre_process=BasicInputBinarizer, activation_post_process=BasicScaleBinarizer,
                      weight_pre_process=nn.Identity)
    m = bnn.layers.Linear.from_module(nn.Linear(F, O), cfg).to(dev)
    with torch.no_grad():
        m.activation_post_process.alpha.uniform_(0.5, 1.0)
    x = torch.randn(M, F, device=dev)
    # same function first: |on - off| against twice the fp32 accumulation bound of the layer (both sides carry it)
    m.eval()
    with torch.no_grad():
        fastpath.REAL_WEIGHTS = False
        off = m(x)
        fastpath.REAL_WEIGHTS = True
        before = fastpath.stats()["linear_real"]
        on = m(x)
        assert fastpath.stats()["linear_real"] == before + 1
        fastpath.REAL_WEIGHTS = False
        bound = 2 * (3 * F * 2.0 ** -23 * m.weight.abs().sum(1).view(1, -1) + 2.0 ** -22 * off.abs())
        diff = (on - off).abs()
        same = bool((diff <= bound).all())
        max_diff = float(diff.max())
        del on, diff, bound
        fwd = alternate(lambda: m(x), iters, warmup)
    m.train()
    xg = x.clone().requires_grad_()
    g = torch.randn_like(off)
    del off

    def step():
        m.zero_grad(set_to_none=True)
        xg.grad = None
        m(xg).backward(g)
    mem = {}
    for key in ("off", "on"):
        fastpath.REAL_WEIGHTS = key == "on"
        step()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        step()
        torch.cuda.synchronize()
        mem[key] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
    fastpath.REAL_WEIGHTS = False
    fb = alternate(step, iters, warmup)
    m.zero_grad(set_to_none=True)
    xg.grad = None
    w = m.weight.detach()
    saved = hipops.pack_act_ste(x.view(M, F, 1, 1))
    t_mm = timed(lambda: torch.mm(g, w), iters, warmup)
    t_gx = timed(lambda: hipops.ste_mask_(torch.mm(g, w), saved), iters, warmup)
    t_gw = timed(lambda: hipops.blinear_grad_weight(g, saved, reduce=True), iters, warmup)
    pipe_us = 2 * 3 * M * F * O / BF16_DENSE_PEAK * 1e6
    pack_bytes = ((F + 31) // 32) * ((O + 15) // 16) * 3 * 1024
    byte_us = (4 * M * F + 4 * M * O + pack_bytes) / HBM_PEAK * 1e6
    best_on, best_off = min(fwd["on"]), min(fwd["off"])
    return {"row": "shape", "M": M, "F": F, "O": O, "forward_us": fwd, "forward_backward_us": fb,
            "forward_speedup": round(best_off / best_on, 3),
            "forward_backward_speedup": round(min(fb["off"]) / min(fb["on"]), 3),
            "step_peak_memory_above_resident_mb": mem, "outputs_within_bound": same, "max_abs_diff": max_diff,
            "matrix_pipe_bound_us": round(pipe_us, 2), "forward_share_of_matrix_pipe_bound": round(pipe_us / best_on, 4),
            "byte_bound_us": round(byte_us, 2), "forward_share_of_byte_bound": round(byte_us / best_on, 4),
            "bounds": "3 bf16 MFMAs per product at %.1f PFLOP/s; x + out + fragments once at %.1f TB/s"
                      % (BF16_DENSE_PEAK / 1e15, HBM_PEAK / 1e12),
            "gx_mm_us": round(t_mm, 2), "gx_mm_and_mask_us": round(t_gx, 2), "gw_kernel_us": round(t_gw, 2),
            "mm_share_of_backward": round(t_mm / (t_gx + t_gw), 4),
            "saved_input_bytes_hip": 3 * 8 * M * ((F + 63) // 64), "saved_input_bytes_composition": 8 * M * F}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default=None, help="M,F,O")
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slinear_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_slinear.py measures on a HIP device and found none")
    dev = torch.device("cuda:0")
    commit, src = source_id(args.commit)
    stamp = dict(commit=commit, slinear_hip_sha256=src, device=torch.cuda.get_device_name(0), iters=args.iters)
    shapes = [tuple(int(v) for v in args.only.split(","))] if args.only else SHAPES
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        for shape in shapes:
            line = json.dumps({**bench_shape(*shape, args.iters, args.warmup, dev), **stamp})
            print(line, flush=True)
            fh.write(line + "\n")
            fh.flush()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Grouped / depthwise binary convolutions in a TRAINING step at batch 256 (csrc/grad_grouped.hip, training.GROUPED):
per shape of tools/bench_grouped.py, device-event times over ITERS iterations after a warm-up of

  * composition : forward + backward of the layer with the switch off — sign(x) under autograd, the weight hook's torch
                  kernels, the library's grouped conv2d and its backward (what the layer ran before; the baseline),
  * hip         : the same with the switch on (pack_act_ste + bnn_hip_bconv2d_grouped forward, the two gradient kernels
                  and the fused weight hook backward),
  * dgrad/wgrad : bnn_hip_bconv_grouped_grad_input_f32 / _weight_f32 alone, each against its byte bound (g in, gx out
                  and the T plane; g and the P, M planes — over 6.3 TB/s achievable HBM),

the input state each way keeps for the backward (switch on: the three planes, counted by training.saved_input_bytes;
composition: the fp32 x and the fp32 sign(x) autograd keeps alive, 8 bytes per element, computed from the shape), and
last one training step (forward, loss, backward, SGD) of a small BATSNetworkCIFAR (C 48, 8 layers, 32 x 32) both ways.  Both ways run in the same process, alternating (off, on, off,
on): every time is reported as the pair of its two runs.  One JSON line per shape.

    python tools/bench_grouped_train.py [--iters 50] [--warmup 10] [--batch 256] [--only NAME] [--commit ID] [--out FILE]
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
from bnn_amd import fastpath, hipops, models, native, training  # noqa: E402
from bnn_amd.ops import BasicInputBinarizer, XNORWeightBinarizer  # noqa: E402
from tests.golden import cells_cases, gen  # noqa: E402
from tools.bench_grouped import HBM_BYTES_PER_S, SHAPES, timed  # noqa: E402


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
    src = open(os.path.join(ROOT, "binary-networks-pytorch_amd", "csrc", "grad_grouped.hip"), "rb").read()
    return commit, hashlib.sha256(src).hexdigest()[:16]


def both_ways(make_fn, iters, warmup):
    """``make_fn()`` -> the closure to time.  (off, on, off, on) in one process -> ([off_us, off_us], [on_us, on_us])."""
    off, on = [], []
    for _ in range(2):
        for flag, dst in ((False, off), (True, on)):
            training.GROUPED = flag
            try:
                dst.append(round(timed(make_fn(), iters, warmup), 2))
            finally:
                training.GROUPED = False
    return off, on


def layer_lines(args, dev, cfg, stamp):
    for name, C, O, G, H, W, k, s, p, d in SHAPES:
        if args.only and args.only not in name:
            continue
        N = args.batch
        x = torch.from_numpy(gen.activation("normal", gen.seed_of("bench-grouped", name), (8, C, H, W))).to(dev)
        x = x.repeat(N // 8, 1, 1, 1).requires_grad_()
        layer = bnn.prepare_binary_model(nn.Conv2d(C, O, k, s, p, d, groups=G, bias=False), cfg)
        layer.weight.data.copy_(torch.from_numpy(gen.conv_weight("kaiming", 5, (O, C // G, k, k))))
        layer = layer.to(dev).train()
        w = layer.weight
        geom = (G, (s, s), (p, p), (d, d))
        assert hipops.grouped_grad_supported(x.shape, w.shape, *geom), name
        with torch.no_grad():
            g = torch.randn_like(layer(x)) * 1e-3
        Ho, Wo = g.shape[2], g.shape[3]

        def step():
            def fn():
                torch.autograd.grad(layer(x), (x, w), g)
            return fn

        kept, res = {}, {}
        for flag in (False, True):      # what each way keeps of the input, and that they agree
            training.GROUPED = flag
            try:
                before = fastpath.stats()["conv2d_train"]
                training.saved_input_bytes(reset=True)
                y = layer(x)
                kept[flag] = training.saved_input_bytes(reset=True)      # (counts the HIP path only: 0 with the switch off)
                assert fastpath.stats()["conv2d_train"] == before + int(flag), "the switch did not select the path"
                assert kept[flag] == (3 * 8 * N * ((C + 63) // 64) * H * W if flag else 0)
                res[flag] = (y.detach(),) + torch.autograd.grad(y, (x, w), g)
            finally:
                training.GROUPED = False
        err = [float((a - r).abs().max() / r.abs().max()) for a, r in zip(res[True], res[False])]
        t_off, t_on = both_ways(step, args.iters, args.warmup)

        sv = hipops.pack_act_ste(x.detach())
        what = hipops.xnor_what(w, False, True)
        t_dgrad = timed(lambda: hipops.bconv_grouped_grad_input(g, sv, what, *geom), args.iters, args.warmup)
        t_wgrad = timed(lambda: hipops.bconv_grouped_grad_weight(g, sv, w.shape, *geom, reduce=False), args.iters, args.warmup)
        plane = N * ((C + 63) // 64) * H * W * 8
        b_dgrad = g.numel() * 4 + x.numel() * 4 + plane
        b_wgrad = g.numel() * 4 + 2 * plane
        bound_d, bound_w = b_dgrad / HBM_BYTES_PER_S * 1e6, b_wgrad / HBM_BYTES_PER_S * 1e6
        yield dict(shape=name, N=N, C=C, O=O, groups=G, HW=[H, W], k=k, stride=s, pad=p, dilation=d, out_hw=[Ho, Wo],
                   composition_fwd_bwd_us=t_off, hip_fwd_bwd_us=t_on,
                   hip_speedup_vs_composition=round(min(t_off) / min(t_on), 3),
                   dgrad_us=round(t_dgrad, 2), dgrad_byte_bound_us=round(bound_d, 2),
                   dgrad_fraction_of_byte_bound=round(bound_d / t_dgrad, 3),
                   wgrad_us=round(t_wgrad, 2), wgrad_byte_bound_us=round(bound_w, 2),
                   wgrad_fraction_of_byte_bound=round(bound_w / t_wgrad, 3),
                   wgrad_splits=hipops.grouped_grad_weight_splits(x.shape, w.shape, *geom),
                   gfma=round(N * O * Ho * Wo * (C // G) * k * k / 1e9, 3),
                   saved_input_bytes_composition=2 * 4 * x.numel(), saved_input_bytes_hip=kept[True],
                   max_rel_diff_y_gx_gw=err, iters=args.iters, warmup=args.warmup, **stamp)


def net_line(args, dev, cfg, stamp):
    N, C, layers = args.batch, 48, 8
    net = models.BATSNetworkCIFAR(C, 10, layers, False, cells_cases.genotype(models, "MIXED"), cells_cases.GROUPS)
    net.drop_path_prob = 0.0
    net = bnn.prepare_binary_model(net, cfg).to(dev).train()
    opt = torch.optim.SGD(net.parameters(), lr=0.01, momentum=0.9)
    x = torch.from_numpy(gen.activation("normal", 11, (8, 3, 32, 32))).to(dev).repeat(N // 8, 1, 1, 1)
    target = torch.arange(N, device=dev) % 10
    crit = nn.CrossEntropyLoss()
    loss_seen = []

    def step():
        def fn():
            opt.zero_grad(set_to_none=True)
            loss = crit(net(x)[0], target)
            loss.backward()
            opt.step()
            loss_seen.append(loss.detach())
        return fn

    grouped = sum(1 for m in net.modules() if isinstance(m, nn.Conv2d) and m.groups > 1 and hasattr(m, "activation_pre_process"))
    seen = []      # input elements of the grouped convolutions in one forward
    hooks = [m.register_forward_pre_hook(lambda mod, inp: seen.append(inp[0].numel())) for m in net.modules()
             if isinstance(m, nn.Conv2d) and m.groups > 1 and hasattr(m, "activation_pre_process")]
    kept = {}
    for flag in (False, True):
        training.GROUPED = flag
        try:
            training.saved_input_bytes(reset=True)
            crit(net(x)[0], target)
            kept[flag] = training.saved_input_bytes(reset=True)
        finally:
            training.GROUPED = False
    for h in hooks:
        h.remove()
    grouped_elems = sum(seen) // 2
    iters, warmup = max(5, args.iters // 5), max(2, args.warmup // 5)
    t_off, t_on = both_ways(step, iters, warmup)
    assert all(bool(torch.isfinite(v)) for v in loss_seen[-4:])
    return dict(shape="bats_cifar_c48_l8_train_step", N=N, C=C, layers=layers, HW=[32, 32], grouped_convs=grouped,
                composition_step_us=t_off, hip_step_us=t_on, hip_speedup_vs_composition=round(min(t_off) / min(t_on), 3),
                grouped_saved_input_bytes_composition=8 * grouped_elems, grouped_saved_input_bytes_hip=kept[True] - kept[False],
                iters=iters, warmup=warmup, **stamp)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--only", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--no-net", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grouped_train_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_grouped_train.py measures on the GPU: no HIP device visible")
    dev = torch.device("cuda:0")
    info = native.device_info(0)
    commit, src = source_id(args.commit)
    stamp = dict(device=info["name"], clock_mhz=info["clock_khz"] / 1e3, commit=commit, grad_grouped_hip_sha16=src)
    cfg = bnn.BConfig(activation_pre_process=BasicInputBinarizer, activation_post_process=bnn.Identity,
                      weight_pre_process=XNORWeightBinarizer)
    lines = []
    for rec in layer_lines(args, dev, cfg, stamp):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if not args.no_net and not args.only:
        lines.append(json.dumps(net_line(args, dev, cfg, stamp)))
        print(lines[-1], flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

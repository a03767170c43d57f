#!/usr/bin/env python3
"""Binary activations with real weights (csrc/sconv.hip) on the MI355X against the torch composition, one JSON line per row.

The yardstick is the composition with ``fastpath.REAL_WEIGHTS`` off, in the same process; both sides alternate (off, on,
off, on: each reported as the pair of its two runs), device-event times over ITERS calls after a warm-up, outputs compared
first.

Per layer, batch 256 (the 3x3 layers of a ResNet-18 at 224x224, its three stride-2 layers and one 1x1 shortcut):

  * forward under ``torch.no_grad()`` (eval: the cached weight fragments) and forward + backward of a training step,
  * the forward's share of the matrix-pipe bound: 2 * 3 * MACs (three bf16 MFMAs per product) over the bf16 dense peak,
  * the two halves of the backward alone — gx (the library's input gradient + the STE mask) and gW (the weight-gradient
    kernel of csrc/grad.hip) — and gx's share of their sum.

Whole network: one training step of the step-0 pre-activation PReLU ResNet-18 of examples/imagenet.py (the recipe's ignore
list) at 224x224, switch off and on, with ``torch.cuda.max_memory_allocated`` of a step each way.

    python tools/bench_sconv.py [--iters 20] [--warmup 5] [--batch 256] [--net-batch 128] [--out FILE] [--skip-net]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "binary-networks-pytorch_amd")]

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

import bnn_amd as bnn  # noqa: E402
from bnn_amd import fastpath, hipops  # noqa: E402
from bnn_amd.models import PreBasicBlock, resnet18  # noqa: E402
from bnn_amd.ops import BasicInputBinarizer, BasicScaleBinarizer  # noqa: E402

BF16_DENSE_PEAK = 2.5e15          # FLOP/s, MI355X spec (v_mfma_f32_16x16x32_bf16)
LAYERS = [  # (name, C, O, H = W, k, stride)
    ("64->64 56x56 3x3", 64, 64, 56, 3, 1), ("128->128 28x28 3x3", 128, 128, 28, 3, 1),
    ("256->256 14x14 3x3", 256, 256, 14, 3, 1), ("512->512 7x7 3x3", 512, 512, 7, 3, 1),
    ("64->128 56x56 3x3 s2", 64, 128, 56, 3, 2), ("128->256 28x28 3x3 s2", 128, 256, 28, 3, 2),
    ("256->512 14x14 3x3 s2", 256, 512, 14, 3, 2), ("64->128 28x28 1x1", 64, 128, 28, 1, 1)]
IGNORE = ["_last_", "_first_", "layer2.0.downsample.1", "layer3.0.downsample.1", "layer4.0.downsample.1"]


def step0_cfg():
    return bnn.BConfig(activation_pre_process=BasicInputBinarizer, activation_post_process=BasicScaleBinarizer,
                       weight_pre_process=nn.Identity)


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


def bench_layer(name, C, O, H, k, stride, batch, iters, warmup, dev):
    torch.manual_seed(0)
    m = bnn.layers.Conv2d.from_module(nn.Conv2d(C, O, k, stride, k // 2, bias=False), step0_cfg()).to(dev)
    with torch.no_grad():
        m.activation_post_process.alpha.uniform_(0.5, 1.0)
    x = torch.randn(batch, C, H, H, device=dev)
    assert hipops.sconv_supported(x.shape, m.weight.shape, m.stride, m.padding, m.dilation)
    # same function first: |on - off| against twice the fp32 accumulation bound of the layer (both sides carry it)
    m.eval()
    with torch.no_grad():
        fastpath.REAL_WEIGHTS = False
        off = m(x)
        fastpath.REAL_WEIGHTS = True
        before = fastpath.stats()["conv2d_real"]
        on = m(x)
        assert fastpath.stats()["conv2d_real"] == before + 1
        fastpath.REAL_WEIGHTS = False
        bound = 2 * (3 * C * k * k * 2.0 ** -23 * m.weight.abs().sum((1, 2, 3)).view(1, -1, 1, 1) + 2.0 ** -22 * off.abs())
        diff = (on - off).abs()
        same = bool((diff <= bound).all())
        fwd = alternate(lambda: m(x), iters, warmup)
    m.train()
    xg = x.clone().requires_grad_()
    g = torch.randn_like(off)

    def step():
        m.zero_grad(set_to_none=True)
        xg.grad = None
        m(xg).backward(g)
    fb = alternate(step, iters, warmup)
    w, pad = m.weight.detach(), k // 2
    t_gx = timed(lambda: torch.ops.aten.convolution_backward(g, x, w, None, [stride] * 2, [pad] * 2, [1, 1], False, [0, 0], 1,
                                                             [True, False, False])[0].masked_fill(x.abs() >= 1, 0),
                 iters, warmup)
    t_gw = timed(lambda: hipops.bconv_grad_weight(g, x, k, stride, reduce=True), iters, warmup)
    ho = (H - 1) // stride + 1
    macs = batch * O * ho * ho * C * k * k
    bound_us = 2 * 3 * macs / BF16_DENSE_PEAK * 1e6
    return {"row": "layer", "layer": name, "batch": batch, "C": C, "O": O, "H": H, "k": k, "stride": stride,
            "forward_us": fwd, "forward_backward_us": fb, "outputs_within_bound": same, "max_abs_diff": float(diff.max()),
            "matrix_pipe_bound_us": round(bound_us, 2), "forward_share_of_matrix_pipe_bound": round(bound_us / min(fwd["on"]), 4),
            "bounded_by": "matrix pipe (3 bf16 MFMAs per product at %.1f PFLOP/s)" % (BF16_DENSE_PEAK / 1e15),
            "gx_library_us": round(t_gx, 2), "gw_kernel_us": round(t_gw, 2), "gx_share_of_backward": round(t_gx / (t_gx + t_gw), 4)}


def bench_net(batch, iters, warmup, dev):
    def build():
        torch.manual_seed(0)
        net = resnet18(num_classes=1000, block_type=PreBasicBlock, activation=nn.PReLU)
        return bnn.prepare_binary_model(net, step0_cfg(), ignore_layers_name=list(IGNORE)).to(dev).train()
    x = torch.randn(batch, 3, 224, 224, device=dev)
    t = torch.randint(0, 1000, (batch,), device=dev)
    row = {"row": "network", "model": "step-0 pre-activation PReLU ResNet-18 (examples/imagenet.py), 224x224", "batch": batch,
           "step_ms": {"off": [], "on": []}, "max_memory_allocated_mb": {}, "first_loss": {}, "real_layers": {}}
    nets = {}
    for key in ("off", "on"):
        nets[key] = build()
        nets[key + "_opt"] = torch.optim.SGD(nets[key].parameters(), lr=0.01, momentum=0.9)

    def step(key):
        net, opt = nets[key], nets[key + "_opt"]
        opt.zero_grad(set_to_none=True)
        loss = nn.functional.cross_entropy(net(x), t)
        loss.backward()
        opt.step()
        return loss
    for rep in range(2):
        for key in ("off", "on"):
            fastpath.REAL_WEIGHTS = key == "on"
            if rep == 0:
                before = fastpath.stats()["conv2d_real_train"]
                row["first_loss"][key] = float(step(key).detach())
                row["real_layers"][key] = fastpath.stats()["conv2d_real_train"] - before
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                step(key)
                torch.cuda.synchronize()
                row["max_memory_allocated_mb"][key] = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)
            row["step_ms"][key].append(round(timed(lambda: step(key), iters, warmup) / 1e3, 3))
    fastpath.REAL_WEIGHTS = False
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--net-batch", type=int, default=128)
    ap.add_argument("--net-iters", type=int, default=6)
    ap.add_argument("--skip-net", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sconv_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_sconv.py measures on a HIP device and found none")
    dev = torch.device("cuda:0")
    rows = [bench_layer(*spec, args.batch, args.iters, args.warmup, dev) for spec in LAYERS]
    if not args.skip_net:
        rows.append(bench_net(args.net_batch, args.net_iters, 2, dev))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        for r in rows:
            line = json.dumps(r)
            print(line, flush=True)
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

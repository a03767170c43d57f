#!/usr/bin/env python3
"""``FactorizedReduce`` in a TRAINING step at batch 256 (training.CELL_OPS: training.ReduceTrainFn, csrc/pack_ste.hip,
csrc/bn_train.hip), with the method of tools/bench_cellops_train.py: forward + backward timed with device events over a
window of at least --window seconds after a warm-up, the variants alternating in one process, two rounds.  The shapes
are the four a C-48 8-layer BATSNetworkCIFAR contains.  Variants:

  * composition : the torch composition (training.GROUPED and CELL_OPS off, the training paths off),
  * parent      : GROUPED and CELL_OPS on with ``training.reduce_train`` declining — what the module ran before it had a
                  training path of its own: the library's BatchNorm, pack_act_ste + the stride-2 1x1 launch on all of u
                  (twice, once on a copy of u[:, :, 1:, 1:]), aten::convolution_backward, torch.cat and PReLU,
  * reduce      : this path — the module as one autograd function,

and for ``reduce`` every entry point it calls alone: its time, the bytes it has to move (from the shapes) and that byte
bound over 6.3 TB/s achievable HBM as a fraction of the time.  Last, one training step (forward, loss, backward, SGD) of
the BATSNetworkCIFAR of tools/bench_grouped_train.py (C 48, 8 layers, 32 x 32) with GROUPED and CELL_OPS on, without and
with the new dispatch: time, torch.cuda.max_memory_allocated, and the loss of the first step from equal weights.  One
JSON line per shape and one for the network.

    python tools/bench_reduce_train.py [--window 0.5] [--warmup 10] [--batch 256] [--only NAME] [--no-net] [--commit ID] [--out FILE]
"""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "binary-networks-pytorch_amd")]

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

import bnn_amd as bnn  # noqa: E402
from bnn_amd import fastpath, hipops, models, native, training  # noqa: E402
from bnn_amd.ops import BasicInputBinarizer, XNORWeightBinarizer  # noqa: E402
from tests.golden import cells_cases, gen  # noqa: E402
from tools.bench_cellops import HBM_BYTES_PER_S, commit  # noqa: E402
from tools.bench_cellops_train import windowed  # noqa: E402

# (name, C_in, C_out, H = W): preprocess0 behind a reduction cell and the skip_connect of a reduction cell, both stages
SHAPES = [("reduce_192_96_hw32", 192, 96, 32), ("reduce_96_96_hw32", 96, 96, 32),
          ("reduce_384_192_hw16", 384, 192, 16), ("reduce_192_192_hw16", 192, 192, 16)]
_REDUCE_TRAIN = training.reduce_train
VARIANTS = {"composition": dict(ENABLED=False, GROUPED=False, CELL_OPS=False, reduce_train=_REDUCE_TRAIN),
            "parent": dict(ENABLED=True, GROUPED=True, CELL_OPS=True, reduce_train=lambda m, x: None),
            "reduce": dict(ENABLED=True, GROUPED=True, CELL_OPS=True, reduce_train=_REDUCE_TRAIN)}


class variant:
    """The switches of one variant (``parent``: the new dispatch declines everything), restored on exit."""

    def __init__(self, name):
        self.new = VARIANTS[name]

    def __enter__(self):
        self.old = {k: getattr(training, k) for k in self.new}
        for k, v in self.new.items():
            setattr(training, k, v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            setattr(training, k, v)


def alternating(names, make_fn, window_s, warmup, rounds=2):
    """Every variant ``rounds`` times, interleaved (a, b, c, a, b, c) -> {name: [us, ...]}."""
    out = {n: [] for n in names}
    for _ in range(rounds):
        for n in names:
            with variant(n):
                out[n].append(windowed(make_fn(n), window_s, warmup)[0])
    return out


def launch_table(m, x, g, window_s, warmup):
    """Every entry point ReduceTrainFn calls, alone: time, bytes it must move, share of the byte bound."""
    bn, act = m.bn, m.activation
    convs = [m.conv_1[0], m.conv_2[0]]
    N, C, H, W = x.shape
    half = convs[0].out_channels
    plans = [fastpath._recognise(c, half) for c in convs]
    packed = [fastpath.packed_weight(c, p, sync=False, fresh=True) for c, p in zip(convs, plans)]
    rm, rv = bn.running_mean.clone(), bn.running_var.clone()
    xd = x.detach()
    phases, mean, invstd, scale, shift = hipops.bn_train_pack_ste_s2(xd, bn.weight, bn.bias, rm, rv, 0.1, bn.eps)
    slopes = act.weight.detach()
    y = torch.empty_like(g)
    z = torch.empty_like(g)

    def conv_fused():
        for k in range(2):
            hipops.bconv2d_fused(phases[k].sign, packed[k], prelu=slopes[k * half:(k + 1) * half], out=y, out_c_offset=k * half)

    def conv_z():
        for k in range(2):
            hipops.bconv2d_fused(phases[k].sign, packed[k], out=z, out_c_offset=k * half)
    conv_z()
    gz, _ = hipops.prelu_shuffle_backward(g, z, slopes, 1)
    split = lambda: gz.view(N, 2, half, H // 2, W // 2).transpose(0, 1).contiguous()      # noqa: E731
    gzk = split()
    w, plan = convs[0].weight, plans[0]
    gp, alpha = hipops.xnor_grad_pack_weight(w, plan.center, plan.compute_alpha)
    gu = [hipops.bconv_grad_input(gzk[k], phases[k], gp, alpha, 1, 1) for k in range(2)]
    slabs = hipops.bconv_grad_weight(gzk[0], phases[0], 1, 1, reduce=False)
    fx, fy, fu = xd.numel() * 4, g.numel() * 4, gu[0].numel() * 4
    plane = N * ((C + 63) // 64) * (H // 2) * (W // 2) * 8                # one plane of one phase
    steps = [
        # the pack alone: the lattice pixels sit in every 64-byte line of x, so all of x is fetched; six planes out
        ("bn_act_pack_ste_s2", lambda: hipops.bn_act_pack_ste_s2(xd, scale, shift), fx + 6 * plane),
        # statistics read x, the pack fetches it again
        ("bn_train_pack_ste_s2", lambda: hipops.bn_train_pack_ste_s2(xd, bn.weight, bn.bias, rm, rv, 0.1, bn.eps),
         2 * fx + 6 * plane),
        ("conv_fused_x2", conv_fused, 4 * plane + fy),                     # P and M of both phases in, y out
        ("conv_recompute_z_x2", conv_z, 4 * plane + fy),
        ("prelu_backward", lambda: hipops.prelu_shuffle_backward(g, z, slopes, 1), 3 * fy),
        ("split_gz_halves", split, 2 * fy),                                # the one extra pass: gz in, its two halves out
        ("grad_input_x1", lambda: hipops.bconv_grad_input(gzk[0], phases[0], gp, alpha, 1, 1), fy // 2 + plane + fu),
        ("grad_weight_x1", lambda: hipops.bconv_grad_weight(gzk[0], phases[0], 1, 1, reduce=False), fy // 2 + 2 * plane),
        ("xnor_weight_backward_x1", lambda: hipops.xnor_weight_backward(w, slabs, plan.center, plan.compute_alpha),
         (slabs.numel() + 2 * w.numel()) * 4),
        # the reduction fetches all lines of x and reads g0, g1; the dx kernel reads x, g0, g1 and writes dx
        ("bn_train_backward_s2", lambda: hipops.bn_train_backward_s2(gu[0], gu[1], xd, mean, invstd, bn.weight),
         3 * fx + 4 * fu),
    ]
    table = []
    for name, fn, nbytes in steps:
        us, _ = windowed(fn, window_s / 4, warmup)
        bound = nbytes / HBM_BYTES_PER_S * 1e6
        table.append(dict(launch=name, us=us, bytes=int(nbytes), byte_bound_us=round(bound, 2),
                          fraction_of_byte_bound=round(bound / us, 3)))
    return table


def shape_lines(args, dev, cfg, stamp):
    for name, C, O, HW in SHAPES:
        if args.only and args.only not in name:
            continue
        N = args.batch
        x = torch.from_numpy(gen.activation("normal", gen.seed_of("bench-reduce", name), (8, C, HW, HW))).to(dev)
        x = x.repeat(N // 8, 1, 1, 1).requires_grad_()
        m = bnn.prepare_binary_model(models.FactorizedReduce(C, O), cfg)
        shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
        m.load_state_dict({k: torch.from_numpy(v) for k, v in gen.model_state(shapes, gen.seed_of(name)).items()})
        m = m.to(dev).train()
        params = [x] + list(m.parameters())
        with torch.no_grad():
            g = torch.randn_like(m(x)) * 1e-3

        def step(_):
            def fn():
                torch.autograd.grad(m(x), params, g)
            return fn

        res, took = {}, {}
        for v in VARIANTS:          # which path each variant takes, and that they agree
            with variant(v):
                before = fastpath.stats()
                y = m(x)
                after = fastpath.stats()
                took[v] = {k: after[k] - before[k] for k in ("reduce_train", "conv2d_train")}
                res[v] = (y.detach(),) + torch.autograd.grad(y, params, g)
        assert took["composition"] == dict(reduce_train=0, conv2d_train=0), took
        assert took["parent"] == dict(reduce_train=0, conv2d_train=2), took
        assert took["reduce"] == dict(reduce_train=1, conv2d_train=0), took
        err = [float((a - r).abs().max() / r.abs().max()) for a, r in zip(res["reduce"], res["parent"])]
        t = alternating(list(VARIANTS), step, args.window, args.warmup)
        table = launch_table(m, x, g, args.window, args.warmup)
        yield dict(op=name, N=N, C_in=C, C_out=O, HW=[HW, HW], composition_fwd_bwd_us=t["composition"],
                   parent_fwd_bwd_us=t["parent"], reduce_fwd_bwd_us=t["reduce"],
                   reduce_over_parent=round(min(t["reduce"]) / min(t["parent"]), 3),
                   reduce_over_parent_worst_case=round(max(t["reduce"]) / min(t["parent"]), 3),
                   reduce_over_composition=round(min(t["reduce"]) / min(t["composition"]), 3),
                   reduce_launches=table, max_rel_diff_vs_parent_y_gx_gparams=err, window_s=args.window,
                   warmup=args.warmup, **stamp)


def net_line(args, dev, cfg, stamp):
    N, C, layers = args.batch, 48, 8
    torch.manual_seed(0)
    net0 = models.BATSNetworkCIFAR(C, 10, layers, False, cells_cases.genotype(models, "MIXED"), cells_cases.GROUPS)
    net0.drop_path_prob = 0.0
    net0 = bnn.prepare_binary_model(net0, cfg).to(dev).train()
    x = torch.from_numpy(gen.activation("normal", 11, (8, 3, 32, 32))).to(dev).repeat(N // 8, 1, 1, 1)
    target = torch.arange(N, device=dev) % 10
    crit = nn.CrossEntropyLoss()
    names = ("parent", "reduce")
    nets = {v: copy.deepcopy(net0) for v in names}
    opts = {v: torch.optim.SGD(nets[v].parameters(), lr=0.01, momentum=0.9) for v in names}
    modules = sum(1 for m in net0.modules() if type(m).__name__ == "FactorizedReduce")

    def one_step(v):
        opts[v].zero_grad(set_to_none=True)
        loss = crit(nets[v](x)[0], target)
        loss.backward()
        opts[v].step()
        return loss.detach()

    first, took, peak = {}, {}, {}
    for v in names:                 # the first step from equal weights: loss, path taken
        with variant(v):
            before = fastpath.stats()["reduce_train"]
            first[v] = float(one_step(v))
            took[v] = fastpath.stats()["reduce_train"] - before
    assert took["parent"] == 0, took
    for v in names:                 # the second step (both optimisers hold their momentum buffers by now): peak memory
        with variant(v):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            one_step(v)
            torch.cuda.synchronize()
            peak[v] = int(torch.cuda.max_memory_allocated())
    t = alternating(list(names), lambda v: (lambda: one_step(v)), args.window, max(2, args.warmup // 3))
    ref = first["parent"]
    agrees = abs(first["reduce"] - ref) <= 1e-4 * abs(ref) + 1e-5 * abs(ref)
    return dict(op="bats_cifar_c48_l8_train_step", N=N, C=C, layers=layers, HW=[32, 32], factorized_reduce_modules=modules,
                modules_on_the_fused_path=took["reduce"], parent_step_us=t["parent"], reduce_step_us=t["reduce"],
                reduce_over_parent=round(min(t["reduce"]) / min(t["parent"]), 3),
                reduce_over_parent_worst_case=round(max(t["reduce"]) / min(t["parent"]), 3),
                max_memory_allocated_parent=peak["parent"], max_memory_allocated_reduce=peak["reduce"],
                first_step_loss_parent=first["parent"], first_step_loss_reduce=first["reduce"],
                first_step_loss_agrees=bool(agrees), window_s=args.window, **stamp)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5, help="seconds each timed window lasts at least")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--only", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--no-net", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reduce_train_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_reduce_train.py measures on the GPU: no HIP device visible")
    dev = torch.device("cuda:0")
    info = native.device_info(0)
    stamp = dict(device=info["name"], clock_mhz=info["clock_khz"] / 1e3, commit=args.commit or commit())
    cfg = bnn.BConfig(activation_pre_process=BasicInputBinarizer, activation_post_process=bnn.Identity,
                      weight_pre_process=XNORWeightBinarizer)
    lines = []
    for rec in shape_lines(args, dev, cfg, stamp):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if not args.no_net and not args.only:
        lines.append(json.dumps(net_line(args, dev, cfg, stamp)))
        print(lines[-1], flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

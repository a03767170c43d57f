#!/usr/bin/env python3
"""The BATS cell operations in a TRAINING step at batch 256 (training.CELL_OPS: training.CellOpTrainFn, csrc/pack_ste.hip,
csrc/prelu_bwd.hip, csrc/bn_train.hip).  Per operation of tools/bench_cellops.py, forward + backward timed with device
events over a window of at least --window seconds after a warm-up, the three variants alternating in one process:

  * composition : the torch composition (training.ENABLED off): the library's BatchNorm, sign() under autograd, the
                  library's convolution, PReLU, the shuffle copy, the add,
  * per_layer   : training.GROUPED on, CELL_OPS off — the per-layer HIP path (torch BatchNorm, pack_act_ste, the
                  convolution, torch PReLU / shuffle / add; the gradient kernels backward),
  * cell_op     : CELL_OPS on — the operation as one autograd function,

and for cell_op every entry point it calls alone: its time, the bytes it has to move (fp32 tensors and bit planes, from
the shapes) and that byte bound over 6.3 TB/s achievable HBM as a fraction of the time.  Last, one training step
(forward, loss, backward, SGD) of the BATSNetworkCIFAR of tools/bench_grouped_train.py (C 48, 8 layers, 32 x 32) as
per_layer and as cell_op: time, torch.cuda.max_memory_allocated, and the loss of the first step from equal weights.
One JSON line per operation and one for the network.

    python tools/bench_cellops_train.py [--window 0.5] [--warmup 10] [--batch 256] [--only NAME] [--no-net] [--commit ID] [--out FILE]
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
from tools.bench_cellops import HBM_BYTES_PER_S, OPS, commit, timed  # noqa: E402

VARIANTS = {"composition": dict(ENABLED=False, GROUPED=False, CELL_OPS=False),
            "per_layer": dict(ENABLED=True, GROUPED=True, CELL_OPS=False),
            "cell_op": dict(ENABLED=True, GROUPED=True, CELL_OPS=True)}


class variant:
    """The switches of one variant, restored on exit."""

    def __init__(self, name):
        self.new = VARIANTS[name]

    def __enter__(self):
        self.old = {k: getattr(training, k) for k in self.new}
        for k, v in self.new.items():
            setattr(training, k, v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            setattr(training, k, v)


def windowed(fn, window_s, warmup):
    """us per call over a window of at least ``window_s`` seconds (the iteration count comes from a first short run)."""
    probe = timed(fn, 5, warmup)
    iters = max(10, int(window_s * 1e6 / max(probe, 1.0)) + 1)
    return round(timed(fn, iters, 2), 2), iters


def alternating(names, make_fn, window_s, warmup, rounds=2):
    """Every variant ``rounds`` times, interleaved (a, b, c, a, b, c) -> {name: [us, ...]}."""
    out = {n: [] for n in names}
    for _ in range(rounds):
        for n in names:
            with variant(n):
                out[n].append(windowed(make_fn(), window_s, warmup)[0])
    return out


def launch_table(op, x, g, window_s, warmup):
    """Every entry point CellOpTrainFn calls, alone: time, bytes it must move, share of the byte bound."""
    bn, conv, act = op.op
    N, C, H, W = x.shape
    O = g.shape[1]
    w = conv.weight
    groups, stride, padding, dilation = int(conv.groups), tuple(conv.stride), tuple(conv.padding), tuple(conv.dilation)
    shuffle = training.CELL_OP_SHUFFLE[type(op).__name__]
    conf = (groups, stride, padding, dilation, shuffle)
    skip = bool(op.skip and stride[0] == 1 and (groups != 1 or C == O))
    plan = fastpath._recognise(conv, O)
    packed = fastpath.packed_weight(conv, plan, sync=False, fresh=True)
    rm, rv = bn.running_mean.clone(), bn.running_var.clone()
    xd = x.detach()
    sv, mean, invstd, _, _ = hipops.bn_train_pack_ste(xd, bn.weight, bn.bias, rm, rv, 0.1, bn.eps)
    slopes = act.weight.detach()
    z = training._cell_conv(sv.sign, packed, conf)
    gz, _ = hipops.prelu_shuffle_backward(g, z, slopes, shuffle)
    what = hipops.xnor_what(w, plan.center, plan.compute_alpha)
    if groups != 1:
        geom = (groups, stride, padding, dilation)
        dgrad = lambda: hipops.bconv_grouped_grad_input(gz, sv, what, *geom)                         # noqa: E731
        wgrad = lambda: hipops.bconv_grouped_grad_weight(gz, sv, w.shape, *geom, reduce=False)       # noqa: E731
    else:
        gp, alpha = hipops.xnor_grad_pack_weight(w, plan.center, plan.compute_alpha)
        dgrad = lambda: hipops.bconv_grad_input(gz, sv, gp, alpha, w.shape[2], stride[0])            # noqa: E731
        wgrad = lambda: hipops.bconv_grad_weight(gz, sv, w.shape[2], stride[0], reduce=False)        # noqa: E731
    gu = dgrad()
    slabs = wgrad()
    fx, fy, plane = xd.numel() * 4, g.numel() * 4, N * ((C + 63) // 64) * H * W * 8
    steps = [
        # statistics read x, the pack reads it again and writes three planes
        ("bn_train_pack_ste", lambda: hipops.bn_train_pack_ste(xd, bn.weight, bn.bias, rm, rv, 0.1, bn.eps), 2 * fx + 3 * plane),
        # P and M in, the skip in, y out
        ("conv_fused", lambda: training._cell_conv(sv.sign, packed, conf, prelu=slopes, residual=xd if skip else None),
         2 * plane + (fx if skip else 0) + fy),
        ("conv_recompute_z", lambda: training._cell_conv(sv.sign, packed, conf), 2 * plane + fy),
        ("prelu_shuffle_backward", lambda: hipops.prelu_shuffle_backward(g, z, slopes, shuffle), 3 * fy),
        ("grad_input", dgrad, fy + plane + fx),                    # g in, the T plane, gx out
        ("grad_weight", wgrad, fy + 2 * plane),                    # g in, P and M
        ("xnor_weight_backward", lambda: hipops.xnor_weight_backward(w, slabs, plan.center, plan.compute_alpha),
         (slabs.numel() + 2 * w.numel()) * 4),
        # the reduction reads g and x, the dx kernel g, x and the addend and writes dx
        ("bn_train_backward_add", lambda: hipops.bn_train_backward_add(gu, xd, mean, invstd, bn.weight, g if skip else None),
         (5 if skip else 4) * fx + fx),
    ]
    table = []
    for name, fn, nbytes in steps:
        us, _ = windowed(fn, window_s / 4, warmup)
        bound = nbytes / HBM_BYTES_PER_S * 1e6
        table.append(dict(launch=name, us=us, bytes=int(nbytes), byte_bound_us=round(bound, 2),
                          fraction_of_byte_bound=round(bound / us, 3)))
    return table, skip


def op_lines(args, dev, cfg, stamp):
    for name, make, C, HW in OPS:
        if args.only and args.only not in name:
            continue
        N = args.batch
        x = torch.from_numpy(gen.activation("normal", gen.seed_of("bench-cellops", name), (8, C, HW, HW))).to(dev)
        x = x.repeat(N // 8, 1, 1, 1).requires_grad_()
        op = bnn.prepare_binary_model(make(), cfg)
        shapes = {k: tuple(v.shape) for k, v in op.state_dict().items()}
        op.load_state_dict({k: torch.from_numpy(v) for k, v in gen.model_state(shapes, gen.seed_of(name)).items()})
        op = op.to(dev).train()
        params = [x] + list(op.parameters())
        with torch.no_grad():
            g = torch.randn_like(op(x)) * 1e-3

        def step():
            def fn():
                torch.autograd.grad(op(x), params, g)
            return fn

        res, took = {}, {}
        for v in VARIANTS:          # which path each variant takes, and that they agree
            with variant(v):
                before = fastpath.stats()
                y = op(x)
                after = fastpath.stats()
                took[v] = {k: after[k] - before[k] for k in ("cell_op_train", "conv2d_train")}
                res[v] = (y.detach(),) + torch.autograd.grad(y, params, g)
        assert took["composition"] == dict(cell_op_train=0, conv2d_train=0), took
        assert took["per_layer"] == dict(cell_op_train=0, conv2d_train=1), took
        assert took["cell_op"] == dict(cell_op_train=1, conv2d_train=0), took
        err = [float((a - r).abs().max() / r.abs().max()) for a, r in zip(res["cell_op"], res["per_layer"])]
        t = alternating(list(VARIANTS), step, args.window, args.warmup)
        table, skip = launch_table(op, x, g, args.window, args.warmup)
        yield dict(op=name, N=N, C=C, HW=[HW, HW], out=list(g.shape[1:]), groups=op.op[1].groups, skip=skip,
                   composition_fwd_bwd_us=t["composition"], per_layer_fwd_bwd_us=t["per_layer"],
                   cell_op_fwd_bwd_us=t["cell_op"],
                   cell_op_over_per_layer=round(min(t["cell_op"]) / min(t["per_layer"]), 3),
                   cell_op_over_composition=round(min(t["cell_op"]) / min(t["composition"]), 3),
                   cell_op_launches=table, cell_op_launch_sum_us=round(sum(r["us"] for r in table), 2),
                   max_rel_diff_vs_per_layer_y_gx_gparams=err, window_s=args.window, warmup=args.warmup, **stamp)


def net_line(args, dev, cfg, stamp):
    N, C, layers = args.batch, 48, 8
    torch.manual_seed(0)
    net0 = models.BATSNetworkCIFAR(C, 10, layers, False, cells_cases.genotype(models, "MIXED"), cells_cases.GROUPS)
    net0.drop_path_prob = 0.0
    net0 = bnn.prepare_binary_model(net0, cfg).to(dev).train()
    x = torch.from_numpy(gen.activation("normal", 11, (8, 3, 32, 32))).to(dev).repeat(N // 8, 1, 1, 1)
    target = torch.arange(N, device=dev) % 10
    crit = nn.CrossEntropyLoss()
    names = ("per_layer", "cell_op")
    nets = {v: copy.deepcopy(net0) for v in names}
    opts = {v: torch.optim.SGD(nets[v].parameters(), lr=0.01, momentum=0.9) for v in names}
    ops = sum(1 for m in net0.modules() if type(m).__name__ in training.CELL_OP_SHUFFLE)

    def one_step(v):
        opts[v].zero_grad(set_to_none=True)
        loss = crit(nets[v](x)[0], target)
        loss.backward()
        opts[v].step()
        return loss.detach()

    first, took, peak = {}, {}, {}
    for v in names:                 # the first step from equal weights: loss, path taken
        with variant(v):
            before = fastpath.stats()["cell_op_train"]
            first[v] = float(one_step(v))
            took[v] = fastpath.stats()["cell_op_train"] - before
    assert took["per_layer"] == 0, took
    for v in names:                 # the second step (both optimisers hold their momentum buffers by now): peak memory
        with variant(v):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            one_step(v)
            torch.cuda.synchronize()
            peak[v] = int(torch.cuda.max_memory_allocated())

    def step_of():
        v = "cell_op" if training.CELL_OPS else "per_layer"
        return lambda: one_step(v)
    t = alternating(list(names), step_of, args.window, max(2, args.warmup // 3))
    ref = first["per_layer"]
    agrees = abs(first["cell_op"] - ref) <= 1e-4 * abs(ref) + 1e-5 * abs(ref)
    return dict(op="bats_cifar_c48_l8_train_step", N=N, C=C, layers=layers, HW=[32, 32], cell_operations=ops,
                cell_operations_on_the_fused_path=took["cell_op"], per_layer_step_us=t["per_layer"],
                cell_op_step_us=t["cell_op"], cell_op_over_per_layer=round(min(t["cell_op"]) / min(t["per_layer"]), 3),
                max_memory_allocated_per_layer=peak["per_layer"], max_memory_allocated_cell_op=peak["cell_op"],
                first_step_loss_per_layer=first["per_layer"], first_step_loss_cell_op=first["cell_op"],
                first_step_loss_agrees=bool(agrees), window_s=args.window, **stamp)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5, help="seconds each timed window lasts at least")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--only", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--no-net", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cellops_train_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_cellops_train.py measures on the GPU: no HIP device visible")
    dev = torch.device("cuda:0")
    info = native.device_info(0)
    stamp = dict(device=info["name"], clock_mhz=info["clock_khz"] / 1e3, commit=args.commit or commit())
    cfg = bnn.BConfig(activation_pre_process=BasicInputBinarizer, activation_post_process=bnn.Identity,
                      weight_pre_process=XNORWeightBinarizer)
    lines = []
    for rec in op_lines(args, dev, cfg, stamp):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if not args.no_net and not args.only:
        lines.append(json.dumps(net_line(args, dev, cfg, stamp)))
        print(lines[-1], flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

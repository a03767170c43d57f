#!/usr/bin/env python3
"""A whole BATS network at batch 256 (bnn_amd/batsnet.py: FusedBATSNetwork): BATSNetworkCIFAR(48, 10, 8, False, MIXED,
12) on 32 x 32 images with a real-valued stem and classifier, eval() / no_grad().  Device-event times around
synchronised work, after a warm-up, the variants alternating over ROUNDS rounds in one process (the median round is
reported, every round is kept in the line):

  * net            : net(x) — every cell through its own executor, the stem, pooling and classifier per layer,
  * fused_eager    : FusedBATSNetwork(net)(x),
  * graph_replay   : FusedBATSNetwork(net).capture(x) once, then replay(),

and, separately, the stem at that shape:

  * stem_library   : net.stem(x) (the library's convolution, BatchNorm, ReLU) + one bn_act_pack per consumer,
  * stem_fused     : the one launch of hipops.stem3x3_bn_relu_pack (three plane sets, no fp32 output),

with the fused launch's byte bound: (x read + K plane sets written) over 6.3 TB/s achievable HBM.  One JSON line per
variant.  ``--stem-only`` runs nothing but a few stem launches of each kind: the run to put under a kernel profiler
(``rocprofv3 --kernel-trace --stats -- python tools/bench_batsnet.py --stem-only``), whose kernel times are the ones to
quote for the stem.

``--net imagenet`` measures BATSNetworkImageNet(80, 1000, 8, False, MIXED, 10) at batch 128 on 224 x 224 images with real
stems and classifier instead (profiles/batsnet_imagenet_bench.jsonl):

  * stems_modules  : stem0 and stem1 as torch modules + one bn_act_pack_multi of s1 (the plan with the switch off),
  * stems_fused    : the two launches hipops.stem_s2x2 + hipops.gconv3x3s2_bn_pack; stem0_fused / stem1_fused: each alone,
                     with its byte bound (x + s0; s0 + s1 + planes) over 6.3 TB/s,
  * eager_modules / eager_fused, replay_modules / replay_fused: the executor and its graph with
    batsnet.FUSE_IMAGENET_STEMS off / on; the stems' share of the forward is stems_modules over eager_modules.

    python tools/bench_batsnet.py [--net cifar|imagenet] [--iters 20] [--warmup 5] [--rounds 3] [--batch N] [--out FILE]
                                  [--commit REV]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "binary-networks-pytorch_amd"), os.path.join(ROOT, "tools")]

import torch  # noqa: E402

import bnn_amd as bnn  # noqa: E402
from bench_cellops import HBM_BYTES_PER_S, commit, timed  # noqa: E402
from bnn_amd import hipops, models, native  # noqa: E402
from bnn_amd.batsnet import LAUNCHES, FusedBATSNetwork  # noqa: E402
from bnn_amd.ops import BasicInputBinarizer, XNORWeightBinarizer  # noqa: E402
from tests.golden import gen  # noqa: E402
from tests.golden.cells_cases import GROUPS, genotype  # noqa: E402

C, CLASSES, LAYERS, HW, GENOTYPE = 48, 10, 8, 32, "MIXED"


def build(dev):
    net = models.BATSNetworkCIFAR(C, CLASSES, LAYERS, False, genotype(models, GENOTYPE), GROUPS)
    net.drop_path_prob = 0.0
    cfg = bnn.BConfig(activation_pre_process=BasicInputBinarizer, activation_post_process=bnn.Identity,
                      weight_pre_process=XNORWeightBinarizer)
    net = bnn.prepare_binary_model(net, cfg, custom_config_layers_name={"stem.0": bnn.BConfig(),
                                                                        "classifier": bnn.BConfig()})
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict({k: torch.from_numpy(v) for k, v in gen.model_state(shapes, gen.seed_of("bench-batsnet")).items()})
    return net.to(dev).eval()


# (the cells' grouped convolutions need a group count that divides 80, 160 and 320: 10, not the 12 of the CIFAR network)
IMAGENET = dict(C=80, classes=1000, layers=8, hw=224, batch=128, groups=10)


def build_imagenet(dev):
    net = models.BATSNetworkImageNet(IMAGENET["C"], IMAGENET["classes"], IMAGENET["layers"], False,
                                     genotype(models, GENOTYPE), IMAGENET["groups"])
    net.drop_path_prob = 0.0
    cfg = bnn.BConfig(activation_pre_process=BasicInputBinarizer, activation_post_process=bnn.Identity,
                      weight_pre_process=XNORWeightBinarizer)
    real = ("stem0.0", "stem0.3", "stem1.1", "classifier")
    net = bnn.prepare_binary_model(net, cfg, custom_config_layers_name={n: bnn.BConfig() for n in real})
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict({k: torch.from_numpy(v) for k, v in
                         gen.model_state(shapes, gen.seed_of("bench-batsnet-imagenet")).items()})
    return net.to(dev).eval()


def main_imagenet(args, dev, info, rev):
    from bnn_amd import batsnet
    from bnn_amd.executor import fold_bn
    N, HW_ = args.batch or IMAGENET["batch"], IMAGENET["hw"]
    net = build_imagenet(dev)
    x = torch.from_numpy(gen.activation("normal", 7, (8, 3, HW_, HW_))).to(dev).repeat(N // 8, 1, 1, 1)
    engines = {}
    for name, on in (("modules", False), ("fused", True)):
        batsnet.FUSE_IMAGENET_STEMS = on
        engines[name] = FusedBATSNetwork(net)
        engines["graph_" + name] = FusedBATSNetwork(net)
    fused = engines["fused"]
    assert [k for k, _ in fused.steps[:2]] == ["stem_s2x2", "stem_s2_pack"], fused.steps[:2]
    assert [k for k, _ in engines["modules"].steps[:2]] == ["module", "module"], engines["modules"].steps[:2]
    detail = fused.steps[1][1]
    K = detail["sets"]
    pres = [fused.cell_executors[k].preprocessor(i) for k, i in detail["consumers"]]
    a, b = torch.stack([p.bn_a for p in pres]), torch.stack([p.bn_b for p in pres])
    conv0, bn0, _, conv1, bn1 = net.stem0
    relu, conv2, bn2 = net.stem1
    (s1, t1), (s2, t2), (s3, t3) = fold_bn(bn0), fold_bn(bn1), fold_bn(bn2)

    def stems_modules():
        return hipops.bn_act_pack_multi(net.stem1(net.stem0(x)), a, b, relu=False)

    def stem0_fused():
        return hipops.stem_s2x2(x, conv0.weight, s1, t1, conv1.weight, s2, t2, conv1.groups, relu_out=relu.inplace)

    with torch.no_grad():
        s0 = stem0_fused()

        def stem1_fused():
            return hipops.gconv3x3s2_bn_pack(s0, conv2.weight, s3, t3, conv2.groups, a, b, relu_in=not relu.inplace,
                                             out_f32=detail["y"])

        def stems_fused():
            return hipops.gconv3x3s2_bn_pack(stem0_fused(), conv2.weight, s3, t3, conv2.groups, a, b,
                                             relu_in=not relu.inplace, out_f32=detail["y"])

        lib, fus = stems_modules(), stems_fused()[1]
        flips = sum(int((p.P != q.P).sum() + (p.M != q.M).sum()) for p, q in zip(lib, fus))   # (words, not bits)
        want = {}
        for name, on in (("modules", False), ("fused", True)):
            batsnet.FUSE_IMAGENET_STEMS = on           # (read at refresh(): capture may refresh)
            want[name] = engines[name](x)[0]
            engines["graph_" + name].capture(x)
        rep_ = {name: engines["graph_" + name].replay().clone() for name in ("modules", "fused")}
        before = native.launch_count()
        fused(x)
        n_fused = native.launch_count() - before
        variants = {"stems_modules": stems_modules, "stems_fused": stems_fused, "stem0_fused": stem0_fused,
                    "stem1_fused": stem1_fused, "eager_modules": lambda: engines["modules"](x),
                    "eager_fused": lambda: fused(x), "replay_modules": engines["graph_modules"].replay,
                    "replay_fused": engines["graph_fused"].replay}
        rounds = {name: [] for name in variants}
        for _ in range(args.rounds):            # alternate: a slow phase of the machine hits every variant alike
            for name, fn in variants.items():
                rounds[name].append(timed(fn, args.iters * (5 if name.startswith("stem") else 1), args.warmup))
    us = {name: statistics.median(v) for name, v in rounds.items()}
    C_ = conv1.out_channels
    H2 = W2 = (HW_ + 3) // 4
    H3 = W3 = (H2 + 1) // 2
    bytes0 = 4 * N * (3 * HW_ * HW_ + C_ * H2 * W2)
    bytes1 = 4 * N * C_ * H2 * W2 + (4 * N * C_ * H3 * W3 if detail["y"] else 0) + K * 16 * ((C_ + 63) // 64) * N * H3 * W3
    kinds = [k for k, _ in fused.steps]
    base_of = {"stems": "stems_modules", "stem0": "stems_modules", "stem1": "stems_modules", "eager": "eager_modules",
               "replay": "replay_modules"}
    model = f"BATSNetworkImageNet({IMAGENET['C']}, {IMAGENET['classes']}, {IMAGENET['layers']}, False, {GENOTYPE}, {IMAGENET['groups']})"
    lines = []
    for name in variants:
        base = base_of[name.split("_")[0]]
        rec = dict(model=model, variant=name, commit=rev, N=N, HW=[HW_, HW_], us=round(us[name], 1),
                   rounds_us=[round(v, 1) for v in rounds[name]], **{f"speedup_vs_{base}": round(us[base] / us[name], 3)},
                   iters=args.iters, warmup=args.warmup, device=info["name"], clock_mhz=info["clock_khz"] / 1e3)
        if name == "stems_modules":
            rec.update(share_of_eager_modules=round(us[name] / us["eager_modules"], 3))
        elif name == "stems_fused":
            rec.update(K=K, y_written=detail["y"], share_of_eager_fused=round(us[name] / us["eager_fused"], 3),
                       plane_words_differing_from_modules=flips, plane_words=int(sum(p.P.numel() + p.M.numel() for p in lib)))
        elif name in ("stem0_fused", "stem1_fused"):
            nbytes = bytes0 if name == "stem0_fused" else bytes1
            bound = nbytes / HBM_BYTES_PER_S * 1e6
            rec.update(bytes=nbytes, byte_bound_us=round(bound, 2), fraction_of_byte_bound=round(bound / us[name], 3),
                       time_over_byte_bound=round(us[name] / bound, 2))
        elif name.startswith("eager"):
            rec.update(images_per_s=round(N / us[name] * 1e6))
            if name == "eager_fused":
                rec.update(hip_launches=n_fused, planned_launches=sum(LAUNCHES.get(k, 0) for k in kinds),
                           max_abs_diff_vs_modules=float((want["fused"] - want["modules"]).abs().max()),
                           max_abs_modules=float(want["modules"].abs().max()))
        else:
            which = name.split("_")[1]
            rec.update(images_per_s=round(N / us[name] * 1e6),
                       bit_identical_to_eager=bool(torch.equal(rep_[which], want[which])))
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--net", choices=("cifar", "imagenet"), default="cifar")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=None, help="default: 256 (cifar), 128 (imagenet)")
    ap.add_argument("--stem-only", action="store_true")
    ap.add_argument("--out", default=None, help="default: profiles/batsnet_bench.jsonl, or batsnet_imagenet_bench.jsonl")
    ap.add_argument("--commit", default=None, help="revision to record (default: git rev-parse --short HEAD)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    info = native.device_info(0)
    rev = args.commit or commit()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "batsnet_bench.jsonl" if args.net == "cifar" else
                                "batsnet_imagenet_bench.jsonl")
    if args.net == "imagenet":
        return main_imagenet(args, dev, info, rev)
    N = args.batch or 256
    net = build(dev)
    x = torch.from_numpy(gen.activation("normal", 7, (8, 3, HW, HW))).to(dev).repeat(N // 8, 1, 1, 1)
    eng = FusedBATSNetwork(net)
    stem_step = eng.steps[0]
    assert stem_step[0] == "stem3x3" and eng.steps[-1][0] == "avgpool_fc", eng.steps[:1] + eng.steps[-1:]
    K, O = stem_step[1]["sets"], net.stem[0].out_channels
    pres = [eng.cell_executors[k].preprocessor(i) for k, i in stem_step[1]["consumers"]]
    a, b = torch.stack([p.bn_a for p in pres]), torch.stack([p.bn_b for p in pres])
    from bnn_amd.executor import fold_bn
    s, t = fold_bn(net.stem[1])

    def stem_library():
        y = net.stem(x)
        return [hipops.bn_act_pack(y, a[k], b[k], relu=False) for k in range(K)]

    def stem_fused():
        return hipops.stem3x3_bn_relu_pack(x, net.stem[0].weight, s, t, a, b, out_f32=stem_step[1]["y"])[1]

    with torch.no_grad():
        lib, fus = stem_library(), stem_fused()
        flips = sum(int((p.P != q.P).sum() + (p.M != q.M).sum()) for p, q in zip(lib, fus))   # (words, not bits)
        if args.stem_only:
            for _ in range(args.iters):
                stem_library()
                stem_fused()
            torch.cuda.synchronize()
            print(json.dumps(dict(stem_only=True, iters=args.iters, words_differing=flips)))
            return
        want = net(x)[0]
        got = eng(x)[0]
        graph = FusedBATSNetwork(net).capture(x)
        rep = graph.replay().clone()
        before = native.launch_count()
        net(x)
        n_net = native.launch_count() - before
        before = native.launch_count()
        eng(x)
        n_eng = native.launch_count() - before
        variants = {"net": lambda: net(x), "fused_eager": lambda: eng(x), "graph_replay": graph.replay,
                    "stem_library": stem_library, "stem_fused": stem_fused}
        rounds = {name: [] for name in variants}
        for _ in range(args.rounds):            # alternate: a slow phase of the machine hits every variant alike
            for name, fn in variants.items():
                it = args.iters * (10 if name.startswith("stem") else 1)
                rounds[name].append(timed(fn, it, args.warmup))
    us = {name: statistics.median(v) for name, v in rounds.items()}
    ref = float(want.abs().max())
    stem_bytes = 4 * N * 3 * HW * HW + K * 16 * ((O + 63) // 64) * N * HW * HW
    bound = stem_bytes / HBM_BYTES_PER_S * 1e6
    kinds = [k for k, _ in eng.steps]
    lines = []
    for name in variants:
        base = "stem_library" if name.startswith("stem") else "net"
        rec = dict(model=f"BATSNetworkCIFAR({C}, {CLASSES}, {LAYERS}, False, {GENOTYPE}, {GROUPS})", variant=name, commit=rev,
                   N=N, HW=[HW, HW], us=round(us[name], 1), rounds_us=[round(v, 1) for v in rounds[name]],
                   **{f"speedup_vs_{base}": round(us[base] / us[name], 3)}, iters=args.iters, warmup=args.warmup,
                   device=info["name"], clock_mhz=info["clock_khz"] / 1e3)
        if name == "net":
            rec.update(images_per_s=round(N / us[name] * 1e6), hip_launches=n_net)
        elif name == "fused_eager":
            rec.update(images_per_s=round(N / us[name] * 1e6), hip_launches=n_eng,
                       planned_launches=sum(LAUNCHES.get(k, 0) for k in kinds),
                       steps={k: kinds.count(k) for k in sorted(set(kinds))},
                       max_abs_diff_vs_net=float((got - want).abs().max()), max_abs_net=ref)
        elif name == "graph_replay":
            rec.update(images_per_s=round(N / us[name] * 1e6), bit_identical_to_fused_eager=bool(torch.equal(rep, got)))
        elif name == "stem_fused":
            rec.update(K=K, O=O, y_written=stem_step[1]["y"], stem_bytes=stem_bytes, byte_bound_us=round(bound, 2),
                       fraction_of_byte_bound=round(bound / us[name], 3), plane_words_differing_from_library=flips)
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

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

    python tools/bench_batsnet.py [--iters 20] [--warmup 5] [--rounds 3] [--batch 256] [--out FILE] [--commit REV]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--stem-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batsnet_bench.jsonl"))
    ap.add_argument("--commit", default=None, help="revision to record (default: git rev-parse --short HEAD)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    info = native.device_info(0)
    rev = args.commit or commit()
    N = args.batch
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

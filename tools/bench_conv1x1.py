#!/usr/bin/env python3
"""The 1x1 binary convolutions of the two resnet50 networks on the MI355X: XNOR-popcount kernel against the FP4 matrix-core
kernel of csrc/bconv1x1_mfma.hip, launch by launch, batch 128 at 224 x 224.

Networks: ``resnet50()`` (Bottleneck, ReLU) and ``resnet50(block_type=PreBottleneck, activation=nn.PReLU)``.  One eager
forward of the fused executor is recorded; every DISTINCT 1x1 launch (input channels, output channels, image size,
epilogue) is then replayed on the operands it had in the network.

    python tools/bench_conv1x1.py                      # in-process: popcount and FP4 alternate (pop, f4, pop, f4), device
                                                       # events over --iters calls; one JSON line per launch, appended to --out
    python tools/bench_conv1x1.py --forward pre --mode all --schedule F.json
                                                       # the forwards a kernel trace is taken of (rocprofv3 --kernel-trace
                                                       # ... -- python tools/bench_conv1x1.py --forward ...); writes the
                                                       # ordered list of the forward's 1x1 launches to F.json
    python tools/bench_conv1x1.py --table DIR          # DIR/<net>_<mode><1|2>/ traces + DIR/<net>_<mode><1|2>.json
                                                       # schedules -> per-key table and the candidates of
                                                       # fastpath.MFMA_1X1_SHAPES / _TERNARY_SHAPES (both FP4 traces below both popcount traces by more
                                                       # than the trace-to-trace gap)

Each row carries the launch's byte bound (planes in, FP4 weights, fp32 / planes out, fp32 residual in, at 8 TB/s) and its
matrix bound (N H W O C products at the FP4 dense rate, 5e15 / s) and says which of the two binds.
"""
import argparse
import csv
import glob
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "binary-networks-pytorch_amd")]

HBM_BYTES_PER_S = 8e12
FP4_MACS_PER_S = 5e15
NETS = ("post", "pre")
NAMES = {"post": "resnet50 Bottleneck", "pre": "resnet50 PreBottleneck+PReLU"}
ONE_BY_ONE = re.compile(r"bconv1x1_mfma_kernel|bconv_sgpr_kernel<1, ?1,")


def build(net_id, mode, batch):
    """(executor planned under BNN_AMD_MFMA_1X1 = mode, input).  One stream: the shortcut convolution in program order."""
    import torch
    import torch.nn as nn
    import bnn_amd as bnn
    from bnn_amd import fastpath
    from bnn_amd.inference import FusedResNet
    from bnn_amd.models import PreBottleneck, resnet50
    from bnn_amd.ops import BasicInputBinarizer, XNORWeightBinarizer
    from tests.golden import gen
    dev = torch.device("cuda:0")
    cfg = bnn.BConfig(activation_pre_process=BasicInputBinarizer, activation_post_process=bnn.Identity,
                      weight_pre_process=XNORWeightBinarizer)
    net = resnet50() if net_id == "post" else resnet50(block_type=PreBottleneck, activation=nn.PReLU)
    net = bnn.prepare_binary_model(net, cfg, custom_config_layers_name={"conv1": bnn.BConfig(), "fc": bnn.BConfig()})
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict({k: torch.from_numpy(v) for k, v in gen.model_state(shapes, 1).items()})
    net = net.to(dev).eval()
    x = torch.from_numpy(gen.normal(1, (8, 3, 224, 224))).to(dev).repeat(batch // 8, 1, 1, 1)
    saved, fastpath.MFMA_1X1 = fastpath.MFMA_1X1, mode
    try:
        eng = FusedResNet(net, overlap_shortcut=False)
        with torch.no_grad():
            eng(x)          # every launch asks its admission on first use: under the same switch
    finally:
        fastpath.MFMA_1X1 = saved
    return eng, x


def record(eng, x):
    """[(layer name, act, keyword arguments of _Conv.run)] of the 1x1 launches of one eager forward, in order."""
    from bnn_amd import executor
    calls, orig = [], executor._Conv.run

    def run(self, act, **kw):
        if tuple(self.layer.kernel_size) == (1, 1):
            calls.append((self.name, act, kw))
        return orig(self, act, **kw)
    executor._Conv.run = run
    try:
        y = eng(x)
    finally:
        executor._Conv.run = orig
    return calls, y


def describe(conv, act, kw):
    N, C, H, W = act.shape
    O = conv.layer.out_channels
    res = kw.get("residual") is not None
    d = dict(C=C, O=O, H=H, W=W, N=N, nonneg=bool(act.nonneg), out_f32=bool(kw["out_f32"]), out_packed=bool(kw["out_packed"]),
             residual=res, late_residual=bool(res and kw.get("residual_after_act")), bn=conv.bn_scale is not None,
             relu=bool(conv.relu), prelu=conv.prelu is not None, pack_affine=kw.get("pack_scale") is not None)
    pix = N * H * W
    byts = pix * C / 8 * (1 if act.nonneg else 2) + O * C / 2 + (4 * pix * O if d["out_f32"] else 0) + \
        (4 * pix * O if res else 0) + (2 * pix * O / 8 if d["out_packed"] else 0)
    d["byte_bound_us"] = round(byts / HBM_BYTES_PER_S * 1e6, 2)
    d["matrix_bound_us"] = round(pix * O * C / FP4_MACS_PER_S * 1e6, 2)
    d["bound_by"] = "bytes" if d["byte_bound_us"] >= d["matrix_bound_us"] else "matrix"
    return d


def convs_by_name(eng):
    out = {}
    for b in eng._blocks:
        for c in list(getattr(b, "convs", [])) + ([b.ds] if getattr(b, "ds", None) is not None else []):
            out[c.name] = c
    return out


def fp4_form(conv):
    """Every launch of ``conv`` was routed, and to the FP4 1x1 kernel."""
    from bnn_amd.executor import Form
    return bool(conv.routes) and set(conv.routes.values()) == {Form.F4_1X1}


def timed(fn, iters, warmup):
    import torch
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


def bench(args):
    import torch
    rows = []
    for net_id in NETS:
        on, x = build(net_id, "all", args.batch)
        off, _ = build(net_id, "0", args.batch)
        with torch.no_grad():
            calls, y_on = record(on, x)
            assert torch.equal(off(x), y_on), "the two executors disagree"
            c_on, c_off = convs_by_name(on), convs_by_name(off)
            seen = set()
            for name, act, kw in calls:
                d = describe(c_on[name], act, kw)
                key = tuple(sorted((k, v) for k, v in d.items() if not k.endswith("_us") and k != "bound_by"))
                if key in seen:
                    continue
                seen.add(key)
                fp4 = fp4_form(c_on[name])
                us = {"popcount": [], "fp4": []}
                for _ in range(2):
                    us["popcount"].append(round(timed(lambda: c_off[name].run(act, **kw), args.iters, args.warmup), 2))
                    if fp4:
                        us["fp4"].append(round(timed(lambda: c_on[name].run(act, **kw), args.iters, args.warmup), 2))
                row = dict(row="launch", net=NAMES[net_id], layer=name, **d, fp4_form=fp4, us=us)
                rows.append(row)
                print(json.dumps(row), flush=True)
        del on, off, calls
        torch.cuda.empty_cache()
    with open(args.out, "a") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")


def forward(args):
    import torch
    eng, x = build(args.forward, args.mode, args.batch)
    with torch.no_grad():
        calls, _ = record(eng, x)
        convs = convs_by_name(eng)
        sched = [dict(layer=n, fp4=fp4_form(convs[n]), **describe(convs[n], a, kw))
                 for n, a, kw in calls]
        del calls
        for _ in range(args.steps):
            eng(x)
        torch.cuda.synchronize()
    with open(args.schedule, "w") as fh:
        json.dump(sched, fh)
    print("forward", args.forward, args.mode, len(sched), "1x1 launches per forward")


def last_forward(trace_dir, n):
    f = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
    ones = [r for r in rows if ONE_BY_ONE.search(r["Kernel_Name"])]
    assert len(ones) >= 2 * n and len(ones) % n == 0, (trace_dir, len(ones), n)
    step = ones[-n:]
    return [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in step], [r["Kernel_Name"] for r in step]


def table(args):
    rows, cand = [], []
    for net_id in NETS:
        us = {}
        for tag in ("01", "02", "all1", "all2"):
            sched = json.load(open(os.path.join(args.table, "%s_%s.json" % (net_id, tag))))
            us[tag], names = last_forward(os.path.join(args.table, "%s_%s" % (net_id, tag)), len(sched))
            for s, k in zip(sched, names):
                assert ("bconv1x1_mfma" in k) == s["fp4"], (net_id, tag, s["layer"], k)
        sched = json.load(open(os.path.join(args.table, "%s_all1.json" % net_id)))
        keys = {}
        for i, s in enumerate(sched):
            if s["fp4"]:
                keys.setdefault((s["C"], s["O"], s["H"], s["out_f32"], s["nonneg"]), []).append(i)
            rows.append(dict(row="trace", net=NAMES[net_id], layer=s["layer"], C=s["C"], O=s["O"], H=s["H"], out_f32=s["out_f32"],
                             nonneg=s["nonneg"], fp4_form=s["fp4"], byte_bound_us=s["byte_bound_us"], matrix_bound_us=s["matrix_bound_us"],
                             bound_by=s["bound_by"], popcount_us=[round(us["01"][i], 1), round(us["02"][i], 1)],
                             fp4_us=[round(us["all1"][i], 1), round(us["all2"][i], 1)]))
        for key, idx in sorted(keys.items()):
            z1, z2, a1, a2 = (sum(us[t][i] for i in idx) for t in ("01", "02", "all1", "all2"))
            gap = max(abs(z1 - z2), abs(a1 - a2))
            ok = max(a1, a2) < min(z1, z2) - gap
            r = dict(row="key", net=NAMES[net_id], key=list(key), launches=len(idx), popcount_us=[round(z1, 1), round(z2, 1)],
                     fp4_us=[round(a1, 1), round(a2, 1)], gap_us=round(gap, 1), admitted=ok)
            rows.append(r)
            if ok:
                cand.append((net_id, key, (z1 + z2) / 2 / len(idx), (a1 + a2) / 2 / len(idx), len(idx)))
        rows.append(dict(row="sum", net=NAMES[net_id], launches=len(sched),
                         popcount_us=[round(sum(us["01"]), 1), round(sum(us["02"]), 1)],
                         fp4_us=[round(sum(us["all1"]), 1), round(sum(us["all2"]), 1)]))
    with open(args.out, "a") as fh:
        for r in rows:
            print(json.dumps(r))
            fh.write(json.dumps(r) + "\n")
    print("fastpath candidates ((C, O, H, writes fp32): (popcount us, FP4 us) per launch):")
    for net_id, key, z, a, n in cand:
        print("    %s %s: (%.1f, %.1f),   # %s, %d launch(es)" % (
            "MFMA_1X1_SHAPES" if key[4] else "MFMA_1X1_TERNARY_SHAPES", key[:4], z, a, NAMES[net_id], n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--forward", choices=NETS)
    ap.add_argument("--mode", default="all", choices=("0", "1", "all"))
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--schedule")
    ap.add_argument("--table")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv1x1_mfma_bench.jsonl"))
    args = ap.parse_args()
    if args.table:
        return table(args)
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_conv1x1.py measures on a HIP device and found none")
    if args.forward:
        return forward(args)
    bench(args)


if __name__ == "__main__":
    main()

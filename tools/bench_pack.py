"""One activation-plane producer at the shape the networks use it at: time per call and achieved HBM read rate.

    python tools/bench_pack.py [--op NAME[,NAME ...]] [--json]

pack_act (BasicInputBinarizer on device) and bn_act_pack run on the config-2 tensor (256 x 128 x 56 x 56, BATCH
overrides the batch), the multi-affine and STE producers on a BATS ImageNet cell state (128 x 80 x 28 x 28),
avgpool2_bn_pack2 on the two hierarchical-block transitions that select its two kernels, bn_relu_maxpool_pack on the
ResNet stem's output; the remaining ops reach the kernels the networks use at other geometries (odd sizes, the
FactorizedReduce lattices, the BATS stems).  BNN_AMD_LIB selects the library, so two builds can be compared run by run."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "binary-networks-pytorch_amd")]
import torch
from bnn_amd import hipops
dev = torch.device("cuda:0")
BATCH = int(os.environ.get("BATCH", "256"))


def affine(C, K=None):
    g = torch.Generator().manual_seed(C)
    shape = (C,) if K is None else (K, C)
    return (0.5 + torch.rand(shape, generator=g)).to(dev), (0.3 * torch.randn(shape, generator=g)).to(dev)


def cell_state():
    return torch.randn(128, 80, 28, 28, device=dev)


def op_pack_act():
    x = torch.randn(BATCH, 128, 56, 56, device=dev).relu_()
    return x, lambda: hipops.pack_act(x)


def op_bn_act_pack():
    x = torch.randn(BATCH, 128, 56, 56, device=dev)
    a, b = affine(128)
    return x, lambda: hipops.bn_act_pack(x, a, b, True)


def op_multi(K):
    def make():
        x = cell_state()
        a, b = affine(80, K)
        return x, lambda: hipops.bn_act_pack_multi(x, a, b, relu=False)
    return make


def op_pack_act_ste():
    x = cell_state()
    return x, lambda: hipops.pack_act_ste(x)


def op_bn_act_pack_ste(hw=(28, 28)):
    def make():
        x = torch.randn(128, 80, *hw, device=dev)
        a, b = affine(80)
        return x, lambda: hipops.bn_act_pack_ste(x, a, b)
    return make


def op_s2(fn):
    def make():
        x = cell_state()
        a, b = affine(80)
        return x, lambda: fn(x, a, b)
    return make


def op_avgpool(shape):
    def make():
        x = torch.randn(*shape, device=dev)
        return x, lambda: hipops.avgpool_pack(x, 2)
    return make


def op_stem3x3():
    x, w = torch.randn(128, 3, 31, 31, device=dev), 0.2 * torch.randn(144, 3, 3, 3, device=dev)
    (s, t), (a, b) = affine(144), affine(144, 1)
    return x, lambda: hipops.stem3x3_bn_relu_pack(x, w, s, t, a, b, out_f32=False)


def op_gconv(K):
    def make():
        x, w = torch.randn(128, 80, 56, 56, device=dev), 0.1 * torch.randn(80, 8, 3, 3, device=dev)
        (s, t), (a, b) = affine(80), affine(80, K)
        return x, lambda: hipops.gconv3x3s2_bn_pack(x, w, s, t, 10, a, b, relu_in=True, out_f32=False)
    return make


def op_avgpool2(shape):
    def make():
        x = torch.randn(*shape, device=dev)
        bn1, bn2 = affine(shape[1]), affine(shape[1])
        return x, lambda: hipops.avgpool2_bn_pack2(x, bn1, True, bn2, False)
    return make


def op_maxpool(shape=None):
    def make():
        x = torch.randn(*(shape or (BATCH, 64, 112, 112)), device=dev)
        a, b = affine(64)
        return x, lambda: hipops.bn_relu_maxpool_pack(x, a, b)
    return make


OPS = {"pack_act": op_pack_act, "bn_act_pack": op_bn_act_pack, "bn_act_pack_multi_k2": op_multi(2),
       "bn_act_pack_multi_k4": op_multi(4), "pack_act_ste": op_pack_act_ste, "bn_act_pack_ste": op_bn_act_pack_ste(),
       "bn_act_pack_ste_vp2": op_bn_act_pack_ste((10, 9)), "bn_act_pack_ste_vp1": op_bn_act_pack_ste((7, 7)),
       "bn_act_pack_s2": op_s2(hipops.bn_act_pack_s2), "bn_act_pack_ste_s2": op_s2(hipops.bn_act_pack_ste_s2),
       "avgpool_pack_f4": op_avgpool((256, 64, 56, 56)),          # W % 4 == 0: avgpool2_pack_kernel
       "avgpool_pack_f2": op_avgpool((256, 256, 14, 14)),         # even, W % 4 != 0: avgpool2_pack_f2_kernel
       "avgpool_pack_ceil": op_avgpool((256, 512, 7, 7)),         # odd: the scalar kernel with clipped windows
       "stem3x3_vp1": op_stem3x3,                                 # odd H W, one consumer: stem3x3_kernel<1, 1>
       "gconv3x3s2_k1": op_gconv(1), "gconv3x3s2_k2": op_gconv(2), "gconv3x3s2_k3": op_gconv(3),
       "gconv3x3s2_k4": op_gconv(4),                              # stem1 of the BATS ImageNet network
       "avgpool2_bn_pack2_wide": op_avgpool2((128, 64, 56, 56)),       # 200704 (pixel, word) threads: one per word
       "avgpool2_bn_pack2_lds": op_avgpool2((128, 128, 28, 28)),      # 100352: the LDS form
       "bn_relu_maxpool_pack": op_maxpool(),
       "bn_relu_maxpool_pack_generic": op_maxpool((64, 64, 57, 57))}   # W % 4 != 0: the scalar-window kernel


def t(fn, n=200):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


ap = argparse.ArgumentParser()
ap.add_argument("--op", default="pack_act", help="one of, or a comma-separated list of: " + ", ".join(sorted(OPS)))
ap.add_argument("--json", action="store_true", help="one JSON line per op: the best of the three rounds")
args = ap.parse_args()
for op in args.op.split(","):
    if op not in OPS:
        ap.error("unknown op " + op)
    x, fn = OPS[op]()
    for _ in range(300): fn()
    best = None
    for _ in range(3):
        us = t(fn)
        best = us if best is None else min(best, us)
        if not args.json:
            print("%s %s: %.1f us  %.2f TB/s read" % (op, tuple(x.shape), us, x.numel() * 4 / us / 1e6))
    if args.json:
        print(json.dumps({"op": op, "shape": list(x.shape), "us": round(best, 2)}), flush=True)
    del x, fn
    torch.cuda.empty_cache()

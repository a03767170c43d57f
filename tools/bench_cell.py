#!/usr/bin/env python3
"""A whole BATS cell at batch 256 (bnn_amd/cellops.py: FusedCell): per cell, device-event times over ITERS iterations
after a warm-up (the protocol of tools/bench_cellops.py) of

  * fused          : cell(s0, s1, 0) under eval() / no_grad() — the cell executor,
  * no_cell_fusion : the same call inside no_cell_fusion() — every operation fused on its own, torch adds the two terms
                     of a node and concatenates the nodes (what a hand-built cell ran before the cell executor),
  * per_layer      : the same call inside per_layer_forward(),

and the byte bound of the fused plan, counted from FusedCell.steps over 6.3 TB/s achievable HBM.  The cells are normal
cells of the two genotypes of tests/golden/cells_cases.py with C = 96, C_prev_prev = C_prev = 384 on 32 x 32 images.
One JSON line per cell and variant.

    python tools/bench_cell.py [--iters 50] [--warmup 10] [--batch 256] [--only NAME] [--out FILE] [--commit REV]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "binary-networks-pytorch_amd"), os.path.join(ROOT, "tools")]

import torch  # noqa: E402

import bnn_amd as bnn  # noqa: E402
from bench_cellops import HBM_BYTES_PER_S, commit, timed  # noqa: E402
from bnn_amd import fastpath, models, native  # noqa: E402
from bnn_amd.cellops import FusedCell  # noqa: E402
from bnn_amd.inference import no_cell_fusion, per_layer_forward  # noqa: E402
from bnn_amd.ops import BasicInputBinarizer, XNORWeightBinarizer  # noqa: E402
from tests.golden import gen  # noqa: E402
from tests.golden.cells_cases import GROUPS, genotype  # noqa: E402

C, C_PREV, HW = 96, 384, 32


def plan_bytes(steps, N: int) -> int:
    """HBM bytes of the fused plan of a NORMAL cell (every tensor at HW x HW): fp32 tensors count 4 bytes per element and
    pass, a set of sign planes 2 x 8 bytes per pixel and 64 channels, written once and read once."""
    px = N * HW * HW
    f32 = lambda ch: 4 * ch * px                             # noqa: E731
    planes = lambda ch: 16 * ((ch + 63) // 64) * px          # noqa: E731
    total = 0
    for kind, d in steps:
        if kind == "pack":
            total += f32(C_PREV) + planes(C_PREV)
        elif kind == "dense":
            total += planes(C_PREV) + f32(C)
        elif kind == "pack_multi":
            total += f32(C) + d["sets"] * planes(C)
        elif kind == "grouped_node":                          # planes, the skip, [the addend], the store
            total += planes(C) + f32(C) * (3 if d["addend"] else 2)
        elif kind == "torch_pool" or kind == "copy":
            total += 2 * f32(C)
        elif kind == "torch_add":
            total += 3 * f32(C)
        elif kind == "zero":
            total += f32(C)
        else:
            raise ValueError(f"no byte count for step kind {kind!r}")
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cell_bench.jsonl"))
    ap.add_argument("--commit", default=None, help="revision to record (default: git rev-parse --short HEAD)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    info = native.device_info(0)
    cfg = bnn.BConfig(activation_pre_process=BasicInputBinarizer, activation_post_process=bnn.Identity,
                      weight_pre_process=XNORWeightBinarizer)
    rev = args.commit or commit()
    N = args.batch
    lines = []
    for gname in ("ALLCONV", "MIXED"):
        if args.only and args.only.lower() not in gname.lower():
            continue
        cell = bnn.prepare_binary_model(models.Cell(genotype(models, gname), C_PREV, C_PREV, C, False, False, GROUPS), cfg)
        shapes = {k: tuple(v.shape) for k, v in cell.state_dict().items()}
        seed = gen.seed_of("bench-cell", gname)
        cell.load_state_dict({k: torch.from_numpy(v) for k, v in gen.model_state(shapes, seed).items()})
        cell = cell.to(dev).eval()
        s0, s1 = (torch.from_numpy(gen.activation("normal", seed + i, (8, C_PREV, HW, HW))).to(dev).repeat(N // 8, 1, 1, 1)
                  for i in (1, 2))
        with torch.no_grad():
            before = fastpath.stats()["cell"]
            y = cell(s0, s1, 0.0)
            assert fastpath.stats()["cell"] == before + 1, "the cell did not take the fused path"
            with no_cell_fusion():
                same = bool(torch.equal(y, cell(s0, s1, 0.0)))
                assert fastpath.stats()["cell"] == before + 1
            steps = FusedCell(cell).steps
            before = native.launch_count()
            cell(s0, s1, 0.0)
            launches = native.launch_count() - before
            t = {"fused": timed(lambda: cell(s0, s1, 0.0), args.iters, args.warmup)}
            with no_cell_fusion():
                t["no_cell_fusion"] = timed(lambda: cell(s0, s1, 0.0), args.iters, args.warmup)
            with per_layer_forward():
                t["per_layer"] = timed(lambda: cell(s0, s1, 0.0), args.iters, args.warmup)
        nbytes = plan_bytes(steps, N)
        bound = nbytes / HBM_BYTES_PER_S * 1e6
        kinds = [k for k, _ in steps]
        for variant, us in t.items():
            rec = dict(cell=gname, variant=variant, commit=rev, N=N, C=C, C_prev=C_PREV, HW=[HW, HW], out=list(y.shape[1:]),
                       us=round(us, 1), speedup_vs_no_cell_fusion=round(t["no_cell_fusion"] / us, 3),
                       iters=args.iters, warmup=args.warmup, device=info["name"], clock_mhz=info["clock_khz"] / 1e3)
            if variant == "fused":
                rec.update(byte_bound_us=round(bound, 1), plan_bytes=nbytes, fraction_of_byte_bound=round(bound / us, 3),
                           hip_launches=launches, steps={k: kinds.count(k) for k in sorted(set(kinds))},
                           bit_identical_to_no_cell_fusion=same)
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

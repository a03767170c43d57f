#!/usr/bin/env python3
"""Generate tests/golden/cellops.npz by running the REFERENCE implementation of the BATS cell operations.

Runs only where the reference package is importable; the test-suite and the GPU box use the committed ``cellops.npz``.
Stored: the reference's outputs and state_dict key lists only (inputs and parameters come from cellops_cases.py / gen.py).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_cellops.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFERENCE = os.environ.get("BNN_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, REFERENCE)

import torch  # noqa: E402

import bnn  # the reference package  # noqa: E402
from bnn.models.layers import bats_ops  # noqa: E402
from bnn.ops import BasicInputBinarizer, XNORWeightBinarizer  # noqa: E402

from tests.golden.cellops_cases import CELL_CASES, MIN_BN_MARGIN, bn_margin  # noqa: E402

assert os.path.realpath(bnn.__file__).startswith(os.path.realpath(REFERENCE)), bnn.__file__
torch.set_num_threads(8)


def ref_op(case):
    cfg = bnn.BConfig(activation_pre_process=BasicInputBinarizer, activation_post_process=bnn.Identity,
                      weight_pre_process=XNORWeightBinarizer)
    op = bnn.prepare_binary_model(case.build(bats_ops), cfg)
    assert type(op.op[1]) is bnn.layers.Conv2d
    shapes = {k: tuple(v.shape) for k, v in op.state_dict().items()}
    st = case.state(shapes)
    op.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    op.eval()
    x = case.input()
    margin = bn_margin(x, st)
    assert margin >= MIN_BN_MARGIN, f"{case.name}: min |bn(x)| = {margin:.3g}: change the seed, not the bound"
    with torch.no_grad():
        out = op(torch.from_numpy(x)).numpy().copy()
    return out, list(shapes), margin


def main():
    blob = {}
    for case in CELL_CASES:
        out, keys, margin = ref_op(case)
        blob[case.name + "/out"] = out
        blob[case.name + "/keys"] = np.array(keys)
        print(f"cellop {case.name:20s} out{out.shape} |max|={np.abs(out).max():.4f} min|bn(x)|={margin:.3g} keys={keys}")
    np.savez_compressed(os.path.join(HERE, "cellops.npz"), **blob)


if __name__ == "__main__":
    main()

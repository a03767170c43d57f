#!/usr/bin/env python3
"""Generate tests/golden/batsnet_imagenet_stem.npz by running the stems of the REFERENCE implementation of
BATSNetworkImageNet with real-valued stem convolutions and classifier (tests/golden/batsnet_imagenet_cases.py).

Runs only where the reference package is importable; the test-suite and the GPU box use the committed file.  Stored: the
state_dict key list of the binarised network, and the reference's ``s0`` and ``s1`` for the case's input, ``s0`` read
AFTER ``stem1`` has run (its in-place ReLU has rectified the tensor ``stem0`` returned: what the cells see).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_batsnet_imagenet.py
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
from bnn import ops  # noqa: E402
from bnn.models import bats  # noqa: E402

from tests.golden import batsnet_imagenet_cases as case  # noqa: E402

assert os.path.realpath(bnn.__file__).startswith(os.path.realpath(REFERENCE)), bnn.__file__
torch.set_num_threads(8)


def main():
    model = case.binarise_real_stems(bnn, ops, case.build(bats))
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(v) for k, v in case.state(shapes).items()})
    model.eval()
    with torch.no_grad():
        raw, s0, s1 = case.run_stems(model, torch.from_numpy(case.inputs()))
    assert torch.equal(s0, torch.relu(raw)) and bool((raw < 0).any())      # the aliased tensor was rectified
    print(f"batsnet_imagenet {case.NAME} s0{tuple(s0.shape)} |max|={float(s0.abs().max()):.4f} s1{tuple(s1.shape)} "
          f"|max|={float(s1.abs().max()):.4f} keys={len(shapes)}")
    np.savez_compressed(os.path.join(HERE, "batsnet_imagenet_stem.npz"), **{
        case.NAME + "/keys": np.array(list(shapes)), case.NAME + "/s0": s0.numpy().copy(), case.NAME + "/s1": s1.numpy().copy()})


if __name__ == "__main__":
    main()

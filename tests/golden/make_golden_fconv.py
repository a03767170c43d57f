#!/usr/bin/env python3
"""Generate tests/golden/fconv.npz by running the REFERENCE implementation of FactorizedConv and OPS['sep_conv_7x7'].

Runs only where the reference package is importable; the test-suite and the GPU box use the committed ``fconv.npz``.
Stored: the reference's outputs, state_dict key lists and the names of its OPS table only (inputs and parameters come
from fconv_cases.py / gen.py).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_fconv.py
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

from tests.golden.fconv_cases import FCONV_CASES, MIN_BN_MARGIN, bn_margin  # noqa: E402

assert os.path.realpath(bnn.__file__).startswith(os.path.realpath(REFERENCE)), bnn.__file__
torch.set_num_threads(8)


def ref_op(case):
    cfg = bnn.BConfig(activation_pre_process=BasicInputBinarizer, activation_post_process=bnn.Identity,
                      weight_pre_process=XNORWeightBinarizer)
    op = bnn.prepare_binary_model(case.build(bats_ops), cfg)
    assert all(type(m) is bnn.layers.Conv2d for m in op.op if isinstance(m, torch.nn.Conv2d))
    assert type(op).__name__ == ("FactorizedConv" if case.kind == "conv_7x1_1x7" else "SepConv")
    shapes = {k: tuple(v.shape) for k, v in op.state_dict().items()}
    st = case.state(shapes)
    op.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    op.eval()
    x = case.input()
    margins = [bn_margin(x, st, "op.0.")]
    mids = []
    hook = op.op[3].register_forward_pre_hook(lambda m, inp: mids.append(inp[0].numpy().copy())) if len(op.op) == 6 else None
    with torch.no_grad():
        out = op(torch.from_numpy(x)).numpy().copy()
    if hook is not None:
        hook.remove()
        margins.append(bn_margin(mids[0], st, "op.3."))     # min |bn2(prelu(conv1))| in float64
    for i, m in enumerate(margins):
        assert m >= MIN_BN_MARGIN, f"{case.name}: BatchNorm {i + 1} margin = {m:.3g}: change the seed, not the bound"
    return out, list(shapes), margins


def main():
    blob = {"ops": np.array(list(bats_ops.OPS))}
    for case in FCONV_CASES:
        out, keys, margins = ref_op(case)
        blob[case.name + "/out"] = out
        blob[case.name + "/keys"] = np.array(keys)
        print(f"fconv {case.name:18s} out{out.shape} |max|={np.abs(out).max():.4f} margins="
              f"{[float('%.3g' % m) for m in margins]} keys={keys}")
    np.savez_compressed(os.path.join(HERE, "fconv.npz"), **blob)


if __name__ == "__main__":
    main()

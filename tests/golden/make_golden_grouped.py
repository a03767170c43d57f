#!/usr/bin/env python3
"""Generate tests/golden/grouped.npz by running the REFERENCE implementation (grouped / depthwise binary convolutions).

Runs only where the reference package is importable; the test-suite and the GPU box use the committed ``grouped.npz``.
Stored: the reference's numeric outputs only (inputs come from the generator parameters in grouped_cases.py / gen.py).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_grouped.py
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
import torch.nn as nn  # noqa: E402

import bnn  # the reference package  # noqa: E402
from bnn.ops import BasicInputBinarizer, BasicScaleBinarizer, XNORWeightBinarizer  # noqa: E402
from bnn.models.layers.bats_ops import DilConv, SepConv  # noqa: E402

from tests.golden import gen  # noqa: E402
from tests.golden.grouped_cases import GROUPED_CASES, OP_C, OP_CASES, op_input  # noqa: E402

assert os.path.realpath(bnn.__file__).startswith(os.path.realpath(REFERENCE)), bnn.__file__
torch.set_num_threads(8)


def t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def ref_case(case):
    x, w, b, sc = case.tensors()
    if case.conv1d:
        conv = nn.Conv1d(case.C, case.O, case.kw, stride=case.stride, padding=case.pad[1], dilation=case.dilation,
                         groups=case.groups, bias=case.bias)
    else:
        conv = nn.Conv2d(case.C, case.O, (case.kh, case.kw), stride=case.stride, padding=case.pad,
                         dilation=case.dilation, groups=case.groups, bias=case.bias)
    conv.weight.data.copy_(t(w))
    if b is not None:
        conv.bias.data.copy_(t(b))
    cfg = bnn.BConfig(
        activation_pre_process=BasicInputBinarizer,
        activation_post_process=BasicScaleBinarizer if case.post == "scale" else bnn.Identity,
        weight_pre_process=XNORWeightBinarizer.with_args(compute_alpha=case.compute_alpha,
                                                         center_weights=case.center))
    layer = bnn.prepare_binary_model(conv, cfg)
    assert type(layer) is (bnn.layers.Conv1d if case.conv1d else bnn.layers.Conv2d)
    if sc is not None:
        layer.activation_post_process.alpha.data.copy_(t(sc).view(1, -1, *([1] * (1 if case.conv1d else 2))))
    with torch.no_grad():
        out = layer(t(x)).numpy().copy()
        # the integer dot from the reference's own ops: conv(sign(x), sign(W - mean), groups)
        xs = layer.activation_pre_process(t(x))
        wsgn = XNORWeightBinarizer(compute_alpha=False, center_weights=case.center)(layer.weight)
        f = torch.nn.functional.conv1d if case.conv1d else torch.nn.functional.conv2d
        dot = f(xs.double(), wsgn.double(), None, case.stride, case.pad[1] if case.conv1d else case.pad,
                case.dilation, case.groups).numpy()
    assert np.array_equal(dot, np.round(dot)) or np.isnan(dot).any()
    return out, dot.astype(np.int32)


def ref_op(name):
    kw = OP_CASES[name]
    if name == "sepconv":
        op = SepConv(OP_C, OP_C, kw["kernel_size"], 1, kw["padding"], groups=12)
    else:
        op = DilConv(OP_C, OP_C, kw["kernel_size"], 1, kw["padding"], kw["dilation"], groups=12)
    cfg = bnn.BConfig(activation_pre_process=BasicInputBinarizer, activation_post_process=bnn.Identity,
                      weight_pre_process=XNORWeightBinarizer)
    op = bnn.prepare_binary_model(op, cfg)
    assert type(op.op[1]) is bnn.layers.Conv2d and op.op[1].groups == 12
    shapes = {k: tuple(v.shape) for k, v in op.state_dict().items()}
    st = gen.model_state(shapes, gen.seed_of("grouped-op", name))
    op.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    op.eval()
    with torch.no_grad():
        out = op(t(op_input(name))).numpy().copy()
    return out, list(shapes)


def main():
    blob = {}
    for case in GROUPED_CASES:
        out, dot = ref_case(case)
        blob[case.name + "/out"] = out
        blob[case.name + "/dot"] = dot
        print(f"grouped {case.name:22s} out{out.shape} |max|={np.nanmax(np.abs(out)):.4f}")
    for name in OP_CASES:
        out, keys = ref_op(name)
        blob["op/" + name + "/out"] = out
        blob["op/" + name + "/keys"] = np.array(keys)
        print(f"op {name} out{out.shape} keys={keys}")
    np.savez_compressed(os.path.join(HERE, "grouped.npz"), **blob)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generate tests/golden/prebottleneck.npz by running the REFERENCE's PreBottleneck (bnn/models/layers/res_block.py:170-229).

Two stacks, ``relu`` and ``prelu`` (the activation of every block): a down-sampling block behind the shortcut of
bnn/models/resnet.py:128-133 (AvgPool2d(2, ceil) -> conv1x1 -> BatchNorm) and an identity block, converted with
BasicInputBinarizer / XNORWeightBinarizer / Identity, on a 9 x 7 input (odd extents: the ceil-mode pool clips).  Stored per
stack, as make_golden.py's make_stacks() does: the names of the binary convolutions, the per-image sign checksums in front
of each, every 4th output channel in full and the per-channel sums of all of them — and the seed of the input.

The fixture is judged with 0 flipped images, so the reference alone has to stay inside that cap: an implementation that
folds BatchNorm into one fma differs from torch by a few fp32 roundings (about 1e-7 relative) of the values in front of a
sign().  The generator therefore asserts that no non-zero value in front of a binary layer lies within 1e-5 max|v| of
zero (a hundredfold margin) and takes the next input seed otherwise.

Needs the reference package (BNN_REFERENCE, as make_golden.py):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_prebottleneck.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.golden import make_golden as mg  # noqa: E402  (puts the reference on the path and checks it is the reference)
from tests.golden import gen  # noqa: E402

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
from bnn.models.layers import PreBottleneck as RefPreBottleneck, conv1x1 as ref_conv1x1  # noqa: E402

SHAPE = (2, 128, 9, 7)
MARGIN = 1e-5
ACTS = {"relu": nn.ReLU, "prelu": nn.PReLU}


def stack(act):
    ds = nn.Sequential(nn.AvgPool2d(2, 2, ceil_mode=True, count_include_pad=False), ref_conv1x1(128, 512),
                       nn.BatchNorm2d(512))
    return nn.Sequential(RefPreBottleneck(128, 128, 2, ds, activation=act), RefPreBottleneck(512, 128, activation=act))


def closest_to_zero(net, x):
    """min over the binary layers of (smallest non-zero |v| in front of the layer) / (largest |v| there)."""
    worst, hooks = [np.inf], []
    for mod in net.modules():
        if isinstance(mod, mg.bnn.layers.Conv2d) and isinstance(mod.activation_pre_process, mg.BasicInputBinarizer):
            def pre(m, inp):
                v = inp[0].detach().abs()
                nz = v[v > 0]
                if nz.numel():
                    worst[0] = min(worst[0], float(nz.min() / v.max()))
            hooks.append(mod.register_forward_pre_hook(pre))
    with torch.no_grad():
        net(mg.t(x))
    for h in hooks:
        h.remove()
    return worst[0]


def main():
    blob = {}
    for name, act in ACTS.items():
        net = mg.bnn.prepare_binary_model(stack(act), mg.xnor_cfg())
        mg.load_state(net, seed=gen.seed_of("prebottleneck", name))
        net.eval()
        seed = gen.seed_of("prebottleneckx", name)
        while True:
            x = gen.normal(seed, SHAPE)
            margin = closest_to_zero(net, x)
            if margin > MARGIN:
                break
            print("prebottleneck", name, "seed", seed, "has a value within", margin, "of zero: next seed")
            seed += 1
        y, names, h = mg._binary_inputs(net, x)
        assert y.shape == (2, 512, 5, 4) and len(names) == 7, (y.shape, names)
        blob[name + "/out_c4"], blob[name + "/out_sum"] = y[:, ::4].copy(), y.astype(np.float64).sum((2, 3))
        blob[name + "/sign_hash"], blob[name + "/layers"] = h, np.array(names)
        blob[name + "/x_seed"] = np.int64(seed)
        print("prebottleneck", name, y.shape, h.shape, float(np.abs(y).max()), "seed", seed, "margin", margin)
    np.savez_compressed(os.path.join(HERE, "prebottleneck.npz"), **blob)


if __name__ == "__main__":
    main()

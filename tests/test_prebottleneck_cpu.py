"""PreBottleneck without a GPU: ``bnn_amd.models.PreBottleneck`` composed of torch operations against the fixture generated
by RUNNING THE REFERENCE's block (tests/golden/make_golden_prebottleneck.py), and the fused executor's bookkeeping — the block
family is registered, by class and by name."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import bnn_amd as bnn
from bnn_amd import executor
from bnn_amd.models import PreBasicBlock, PreBottleneck, conv1x1
from bnn_amd.ops import BasicInputBinarizer, XNORWeightBinarizer
from tests.golden import gen, sighash

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPE = (2, 128, 9, 7)
ACTS = {"relu": nn.ReLU, "prelu": nn.PReLU}


def stack(act):
    ds = nn.Sequential(nn.AvgPool2d(2, 2, ceil_mode=True, count_include_pad=False), conv1x1(128, 512), nn.BatchNorm2d(512))
    net = nn.Sequential(PreBottleneck(128, 128, 2, ds, activation=act), PreBottleneck(512, 128, activation=act))
    return bnn.prepare_binary_model(net, bnn.BConfig(activation_pre_process=BasicInputBinarizer,
                                                     activation_post_process=bnn.Identity,
                                                     weight_pre_process=XNORWeightBinarizer))


def load(net, name):
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    state = gen.model_state(shapes, gen.seed_of("prebottleneck", name))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    return net.eval()


def fixture(name):
    g = np.load(os.path.join(HERE, "golden", "prebottleneck.npz"))
    return {k[len(name) + 1:]: g[k] for k in g.files if k.startswith(name + "/")}


def binary_names(net):
    return [n for n, m in net.named_modules()
            if isinstance(m, bnn.layers.Conv2d) and isinstance(m.activation_pre_process, BasicInputBinarizer)]


@pytest.mark.parametrize("name", list(ACTS))
def test_the_module_reproduces_the_reference_bit_for_bit(name):
    fx = fixture(name)
    net = load(stack(ACTS[name]), name)
    names = binary_names(net)
    hashes, hooks, mods = {}, [], dict(net.named_modules())
    for n in names:
        def pre(m, inp, n=n):
            hashes[n] = sighash.sign_hash_torch(inp[0])
        hooks.append(mods[n].register_forward_pre_hook(pre))
    x = torch.from_numpy(gen.normal(int(fx["x_seed"]), SHAPE))
    with torch.no_grad():
        y = net(x)
    for h in hooks:
        h.remove()
    assert y.shape == (2, 512, 5, 4)
    # execution order of the reference: the shortcut convolution runs last in a block (y += shortcut(x))
    assert sorted(names) == sorted(str(n) for n in fx["layers"]) and len(names) == 7
    got = torch.stack([hashes[str(n)] for n in fx["layers"]], 1).numpy()
    assert np.array_equal(got, fx["sign_hash"])
    assert torch.equal(y[:, ::4], torch.from_numpy(fx["out_c4"]))
    assert np.allclose(y.double().sum((2, 3)).numpy(), fx["out_sum"], rtol=1e-6, atol=1e-6 * np.abs(fx["out_sum"]).max())


def test_the_executor_knows_the_block_family():
    blk = PreBottleneck(128, 32)
    assert executor._block_kind(blk) is PreBottleneck
    assert executor._BLOCK_KINDS["PreBottleneck"] is PreBottleneck
    assert executor._BLOCK_ATTRS[PreBottleneck] == executor._BLOCK_ATTRS[executor.Bottleneck]
    assert executor._block_kind(PreBasicBlock(64, 64)) is PreBasicBlock


def test_a_foreign_class_of_the_same_name_and_layout_is_recognised():
    class Foreign(nn.Module):           # the reference's own block: same name, same attributes, another package
        def __init__(self):
            super().__init__()
            for a in ("conv1", "bn1", "act1", "conv2", "bn2", "act2", "conv3", "bn3", "act3"):
                setattr(self, a, nn.Identity())
            self.downsample = None
    Foreign.__name__ = "PreBottleneck"
    assert executor._block_kind(Foreign()) is PreBottleneck

    class Short(nn.Module):             # the name alone is not enough
        conv1 = bn1 = act1 = None
    Short.__name__ = "PreBottleneck"
    assert executor._block_kind(Short()) is None


def test_the_pre_record_holds_one_batchnorm_per_convolution():
    fields = {f.name for f in executor._Pre.__dataclass_fields__.values()}
    assert {"bn", "convs", "ds", "pool", "ds_float"} <= fields and not fields & {"bn1", "bn2"}

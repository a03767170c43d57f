"""What one launch of the fused executor leaves for a later block (bnn_amd/executor.py): sign planes that are not
``sign(t)`` but the input of one particular block's first binary convolution — that block's bn1 (and ReLU) already
applied — and, with them, the planes of that block's shortcut BatchNorm.  Every producer of such planes at batch 2:

* the stem kernel writing the first hierarchical block's planes;
* a hierarchical block's launch writing the next block's planes (``hblock_forward`` / ``hblock_shortcut_forward``);
* a stage's last block pooling and binarising for the next stage's first block (``hblock_pool_forward``, 56 x 56 and
  28 x 28: gated on H * W >= 784, hence the 224 x 224 input);
* the pool in front of a stage writing both sets of planes (``_pool_into_hblock``, 14 x 14 -> 7 x 7);
* a ``PreBasicBlock``'s last convolution binarising through the next block's bn1.

Each form must give the bits of the launch-by-launch form, eagerly, as a HIP graph and behind ``forward_fresh`` (which
keeps the stem's planes across calls); the launch counts prove that the planes travelled instead of being packed again.
"""
import pytest
import torch
import torch.nn as nn

import bnn_amd as bnn
from bnn_amd import native
from bnn_amd.inference import FusedBlocks, FusedResNet, tap_binary_inputs
from bnn_amd.models import HBlock, PreBasicBlock, ResNet, resnet18
from bnn_amd.ops import BasicInputBinarizer, BasicScaleBinarizer, XNORWeightBinarizer
from tests.golden import gen

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# stem (writes block 1's planes) + 8 blocks + the 14x14 -> 7x7 pool + 2 head launches: the accounting of
# tests/test_gpu_c3_full.py::test_c5_hblock_3463_at_its_stated_size for two blocks per stage
HNET_LAUNCHES = 12
# bn_act_pack of the first block (no stem in front) + 4 blocks; the pool between the stages is the first stage's last launch
HBLOCKS_LAUNCHES = 5
# stem + the first block's bn_act_pack + 8 x 2 convolutions + 3 x (shortcut packing pass + shortcut convolution) + 2 head
# launches: no bn_act_pack in front of blocks 2..8, their planes come out of the previous block's last epilogue
PRENET_LAUNCHES = 26


def _prepared(net, post, seed):
    cfg = bnn.BConfig(activation_pre_process=BasicInputBinarizer, activation_post_process=post,
                      weight_pre_process=XNORWeightBinarizer)
    net = bnn.prepare_binary_model(net, cfg, custom_config_layers_name={"conv1": bnn.BConfig(), "fc": bnn.BConfig()})
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict({k: torch.from_numpy(v) for k, v in gen.model_state(shapes, seed).items()})
    return net.to(DEV).eval()


def _binary_conv_names(net):
    return [n for n, m in net.named_modules()
            if isinstance(m, bnn.layers.Conv2d) and isinstance(m.activation_pre_process, BasicInputBinarizer)]


def _launches(engine, x):
    n0 = native.launch_count()
    engine(x)
    return native.launch_count() - n0


def _tapped(engine, x):
    seen = []
    with tap_binary_inputs(lambda name, act: seen.append(name)):
        y = engine(x).clone()
    return y, seen


def _fresh_twice(engine, xs):
    """``forward_fresh`` on two different tensors (the second call replays the graph captured by the first and reuses the
    stem's static planes), each against the plain forward of its own tensor."""
    for x in xs:
        want = engine(x).clone()
        assert torch.equal(engine.forward_fresh(x), want)


@pytest.fixture(scope="module")
def hnet():
    return _prepared(ResNet(HBlock, [2, 2, 2, 2], activation=nn.ReLU), bnn.Identity, 1)


def test_hblock_net_every_handoff(hnet):
    x, x2 = (torch.from_numpy(gen.normal(gen.seed_of("handoff", "hnet", k), (2, 3, 224, 224))).to(DEV) for k in (0, 1))
    fused = FusedResNet(hnet)
    assert fused.reads_caller_tensor
    y = fused(x).clone()
    assert y.shape == (2, 1000) and torch.isfinite(y).all()
    n = _launches(fused, x)
    print("launches of one hierarchical-net forward:", n)
    assert n == HNET_LAUNCHES
    assert torch.equal(FusedResNet(hnet, fuse_hblock=False)(x), y)
    yt, seen = _tapped(fused, x)
    assert sorted(seen) == sorted(_binary_conv_names(hnet)) and len(seen) == 8 * 3 + 3
    assert torch.equal(yt, y)
    assert torch.equal(FusedResNet(hnet, throughput_mode=True)(x), y)
    _fresh_twice(fused, (x, x2))
    fused.capture(x)
    assert torch.equal(fused(x), y)


def test_hblocks_without_a_stem(hnet):
    blocks = nn.Sequential(*hnet.layer1, *hnet.layer2).eval()
    x = torch.from_numpy(gen.normal(gen.seed_of("handoff", "hblocks"), (2, 64, 56, 56))).to(DEV)
    fused = FusedBlocks(blocks)
    y = fused(x).clone()
    assert y.shape == (2, 128, 28, 28) and torch.isfinite(y).all()
    n = _launches(fused, x)
    print("launches of two hierarchical stages without a stem:", n)
    assert n == HBLOCKS_LAUNCHES
    yt, seen = _tapped(fused, x)
    assert len(seen) == 4 * 3 + 1 and len(set(seen)) == len(seen)
    assert torch.equal(yt, y)


def test_prebasicblock_net_handoff():
    net = _prepared(resnet18(block_type=PreBasicBlock, activation=nn.ReLU, num_classes=50), BasicScaleBinarizer, 4)
    x, x2 = (torch.from_numpy(gen.normal(gen.seed_of("handoff", "prenet", k), (2, 3, 96, 96))).to(DEV) for k in (0, 1))
    fused = FusedResNet(net)
    y = fused(x).clone()
    assert y.shape == (2, 50) and torch.isfinite(y).all()
    n = _launches(fused, x)
    print("launches of one PreBasicBlock-net forward:", n)
    assert n == PRENET_LAUNCHES
    _fresh_twice(fused, (x, x2))
    fused.capture(x)
    assert torch.equal(fused(x), y)

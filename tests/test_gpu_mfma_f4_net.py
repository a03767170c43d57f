"""The fused ResNet-18 executor with its matrix-core convolutions in the FP4 form (fastpath.MFMA_F4) against the same
executor with them in the int8 form: logits and every sign plane a binary convolution reads are equal bit for bit, the
launch count stays 19, exactly the eleven convolutions with C >= 128 take the FP4 form and none of layer1 /
layer2.0.conv1 (C = 64) does.  Then the same through the two-stream graph replay."""
import pytest
import torch

from bnn_amd import fastpath, native
from bnn_amd.inference import FusedResNet, tap_binary_inputs
from bnn_amd.pipeline import PipelinedInference
from tests.golden import gen
from tests.test_gpu_mfma_net import DENSE, FOLD, FP4, _convs, net  # noqa: F401  (the module-scoped model fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAUNCHES = 19
ON_F4 = sorted(["layer2.0.conv2", "layer2.1.conv1", "layer2.1.conv2", "layer3.0.conv1", "layer3.0.conv2",
                "layer3.1.conv1", "layer3.1.conv2", "layer4.0.conv1", "layer4.0.conv2", "layer4.1.conv1",
                "layer4.1.conv2"])


def _engine(net, f4, monkeypatch):
    monkeypatch.setattr(fastpath, "MFMA_CONV", "all")
    monkeypatch.setattr(fastpath, "MFMA_FOLD", "all")
    monkeypatch.setattr(fastpath, "MFMA_F4", f4)
    return FusedResNet(net)


def _forward(engine, x):
    planes = {}
    with tap_binary_inputs(lambda name, act: planes.__setitem__(name, (act.P.clone(), act.M.clone()))):
        engine(x)
    n0 = native.launch_count()
    y = engine(x).clone()
    launches = native.launch_count() - n0
    convs = _convs(engine)
    on_cores = sorted(c.name for c in convs if (DENSE | FOLD) & set(c.routes.values()))
    on_f4 = sorted(c.name for c in convs if FP4 & set(c.routes.values()))
    return y, planes, launches, on_cores, on_f4


@pytest.mark.parametrize("n,size", [(2, 224), (3, 96)])
def test_fp4_on_equals_fp4_off(net, monkeypatch, n, size):  # noqa: F811
    x = torch.from_numpy(gen.normal(gen.seed_of("mfma-f4-net", n, size), (n, 3, size, size))).to(DEV)
    y0, planes0, launches0, cores0, f40 = _forward(_engine(net, "0", monkeypatch), x)
    y1, planes1, launches1, cores1, f41 = _forward(_engine(net, "all", monkeypatch), x)
    assert launches0 == LAUNCHES and launches1 == LAUNCHES
    assert cores0 == cores1 and len(cores0) == 16          # what runs on the matrix cores does not move
    assert f40 == [] and f41 == ON_F4
    assert not any(name.startswith("layer1.") or name == "layer2.0.conv1" for name in f41)
    assert torch.equal(y0, y1)
    assert len(planes0) == LAUNCHES and sorted(planes0) == sorted(planes1)
    for name in planes0:
        assert torch.equal(planes0[name][0], planes1[name][0]) and torch.equal(planes0[name][1], planes1[name][1]), name
    # the default: only shapes of the table — all eleven at 224 x 224, where the table was traced
    yd, _, launchesd, coresd, f4d = _forward(_engine(net, "1", monkeypatch), x)
    assert launchesd == LAUNCHES and coresd == cores0 and torch.equal(yd, y0)
    assert f4d == ON_F4 if (n, size) == (2, 224) else set(f4d) <= set(ON_F4)


def test_two_stream_graph_replay(net, monkeypatch):  # noqa: F811
    xs = [torch.from_numpy(gen.normal(gen.seed_of("mfma-f4-net", "pipe", k), (2, 3, 224, 224))).to(DEV) for k in range(2)]
    want = [_engine(net, "0", monkeypatch)(x).clone() for x in xs]
    monkeypatch.setattr(fastpath, "MFMA_F4", "all")
    pipe = PipelinedInference(net, xs[0], n_streams=2)
    for i in range(2):
        with torch.cuda.stream(pipe.stream(i)):
            pipe.input(i).copy_(xs[i])
    for _ in range(3):
        outs = [pipe.launch(i) for i in range(2)]
        pipe.synchronize()
        assert torch.equal(outs[0], want[0]) and torch.equal(outs[1], want[1])

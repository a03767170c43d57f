"""The fused ResNet-18 executor with the folded-shortcut convolutions on the int8 matrix cores (fastpath.MFMA_FOLD)
against the same executor with them on the popcount fold: logits and every sign plane a binary convolution reads are
equal bit for bit, the launch count stays 19, exactly layer{2,3,4}.0.conv2 take the fold launch, and
BNN_AMD_MFMA_CONV=0 turns it off too.  Then the same through the two-stream graph replay."""
import pytest
import torch

from bnn_amd import fastpath, native
from bnn_amd.inference import FusedResNet, tap_binary_inputs
from bnn_amd.pipeline import PipelinedInference
from tests.golden import gen
from tests.test_gpu_mfma_net import DENSE, FOLD, _convs, net  # noqa: F401  (the module-scoped model fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAUNCHES = 19
FOLDED = ["layer2.0.conv2", "layer3.0.conv2", "layer4.0.conv2"]


def _engine(net, fold, monkeypatch, conv="1"):
    monkeypatch.setattr(fastpath, "MFMA_CONV", conv)
    monkeypatch.setattr(fastpath, "MFMA_FOLD", fold)
    return FusedResNet(net)


def _forward(engine, x):
    planes = {}
    with tap_binary_inputs(lambda name, act: planes.__setitem__(name, (act.P.clone(), act.M.clone()))):
        engine(x)
    n0 = native.launch_count()
    y = engine(x).clone()
    launches = native.launch_count() - n0
    folded = sorted(c.name for c in _convs(engine) if FOLD & set(c.routes.values()))
    on_mfma = sorted(c.name for c in _convs(engine) if DENSE & set(c.routes.values()))
    return y, planes, launches, folded, on_mfma


@pytest.mark.parametrize("n,size", [(2, 224), (3, 96)])
def test_fold_on_equals_fold_off(net, monkeypatch, n, size):  # noqa: F811
    x = torch.from_numpy(gen.normal(gen.seed_of("mfma-fold-net", n, size), (n, 3, size, size))).to(DEV)
    y0, planes0, launches0, folded0, on0 = _forward(_engine(net, "0", monkeypatch), x)
    y1, planes1, launches1, folded1, on1 = _forward(_engine(net, "all", monkeypatch), x)
    assert launches0 == LAUNCHES and launches1 == LAUNCHES
    assert folded0 == [] and folded1 == FOLDED
    assert on0 == on1                                 # the other launches do not move
    assert torch.equal(y0, y1)
    assert len(planes0) == LAUNCHES and sorted(planes0) == sorted(planes1)
    for name in planes0:
        assert torch.equal(planes0[name][0], planes1[name][0]) and torch.equal(planes0[name][1], planes1[name][1]), name
    # the main switch turns the fold off too
    yc, _, launchesc, foldedc, onc = _forward(_engine(net, "all", monkeypatch, conv="0"), x)
    assert launchesc == LAUNCHES and foldedc == [] and onc == [] and torch.equal(yc, y0)
    # the default: only shapes of the table
    yd, _, launchesd, foldedd, _ = _forward(_engine(net, "1", monkeypatch), x)
    assert launchesd == LAUNCHES and set(foldedd) <= set(FOLDED) and torch.equal(yd, y0)


def test_two_stream_graph_replay(net, monkeypatch):  # noqa: F811
    xs = [torch.from_numpy(gen.normal(gen.seed_of("mfma-fold-net", "pipe", k), (2, 3, 224, 224))).to(DEV) for k in range(2)]
    want = [_engine(net, "0", monkeypatch)(x).clone() for x in xs]
    monkeypatch.setattr(fastpath, "MFMA_FOLD", "all")
    pipe = PipelinedInference(net, xs[0], n_streams=2)
    for i in range(2):
        with torch.cuda.stream(pipe.stream(i)):
            pipe.input(i).copy_(xs[i])
    for _ in range(3):
        outs = [pipe.launch(i) for i in range(2)]
        pipe.synchronize()
        assert torch.equal(outs[0], want[0]) and torch.equal(outs[1], want[1])

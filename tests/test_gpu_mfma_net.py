"""The fused ResNet-18 executor with its 3x3 convolutions on the int8 matrix cores (fastpath.MFMA_CONV) against the same
executor on the popcount kernels: logits and every sign plane a binary convolution reads are equal bit for bit, the
launch count stays 19, and the MFMA launches are really taken.  Then the same through the two-stream graph replay."""
import pytest
import torch

import bnn_amd as bnn
from bnn_amd import fastpath, native
from bnn_amd.executor import Form
from bnn_amd.inference import FusedResNet, tap_binary_inputs
from bnn_amd.models import resnet18
from bnn_amd.ops import BasicInputBinarizer, XNORWeightBinarizer
from bnn_amd.pipeline import PipelinedInference
from tests.golden import gen

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAUNCHES = 19
DENSE, FOLD, FP4 = {Form.I8_3X3, Form.F4_3X3}, {Form.I8_FOLD, Form.F4_FOLD}, {Form.F4_3X3, Form.F4_FOLD}


@pytest.fixture(scope="module")
def net():
    cfg = bnn.BConfig(activation_pre_process=BasicInputBinarizer, activation_post_process=bnn.Identity,
                      weight_pre_process=XNORWeightBinarizer)
    m = bnn.prepare_binary_model(resnet18(), cfg, custom_config_layers_name={"conv1": bnn.BConfig(), "fc": bnn.BConfig()})
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict({k: torch.from_numpy(v) for k, v in gen.model_state(shapes, 11).items()})
    return m.to(DEV).eval()


def _engine(net, switch, monkeypatch, **kw):
    monkeypatch.setattr(fastpath, "MFMA_CONV", switch)
    return FusedResNet(net, **kw)


def _forward(engine, x):
    """(logits, {layer: (P, M)} of every binary convolution's input, launches, layers that ran on the matrix cores)."""
    planes = {}
    with tap_binary_inputs(lambda name, act: planes.__setitem__(name, (act.P.clone(), act.M.clone()))):
        engine(x)
    n0 = native.launch_count()
    y = engine(x).clone()
    launches = native.launch_count() - n0
    on_mfma = sorted(c.name for c in _convs(engine) if DENSE & set(c.routes.values()))
    return y, planes, launches, on_mfma


def _convs(engine):
    from bnn_amd.executor import _Conv
    seen, todo, visited = [], [engine], set()
    while todo:
        o = todo.pop()
        if id(o) in visited:
            continue
        visited.add(id(o))
        if isinstance(o, _Conv):
            seen.append(o)
        elif isinstance(o, (list, tuple)):
            todo.extend(o)
        elif isinstance(o, dict):
            todo.extend(o.values())
        elif hasattr(o, "__dict__") and type(o).__module__.startswith("bnn_amd.executor"):
            todo.extend(v for k, v in vars(o).items() if k != "model")
    return seen


@pytest.mark.parametrize("n,size", [(2, 224), (3, 96)])
def test_switch_on_equals_switch_off(net, monkeypatch, n, size):
    x = torch.from_numpy(gen.normal(gen.seed_of("mfma-net", n, size), (n, 3, size, size))).to(DEV)
    y0, planes0, launches0, on0 = _forward(_engine(net, "0", monkeypatch), x)
    y1, planes1, launches1, on1 = _forward(_engine(net, "all", monkeypatch), x)
    assert launches0 == LAUNCHES and launches1 == LAUNCHES
    assert on0 == [] and len(on1) == 13          # every 3x3 convolution but the three with a folded shortcut
    assert torch.equal(y0, y1)
    assert len(planes0) == LAUNCHES and sorted(planes0) == sorted(planes1)
    for name in planes0:
        assert torch.equal(planes0[name][0], planes1[name][0]) and torch.equal(planes0[name][1], planes1[name][1]), name
    if size == 224:                              # the default: the table of shapes that measured faster
        yd, planesd, launchesd, ond = _forward(_engine(net, "1", monkeypatch), x)
        assert launchesd == LAUNCHES and 0 < len(ond) <= 13 and set(ond) <= set(on1)
        assert torch.equal(yd, y0)


def test_two_stream_graph_replay(net, monkeypatch):
    xs = [torch.from_numpy(gen.normal(gen.seed_of("mfma-net", "pipe", k), (2, 3, 224, 224))).to(DEV) for k in range(2)]
    want = [_engine(net, "0", monkeypatch)(x).clone() for x in xs]
    monkeypatch.setattr(fastpath, "MFMA_CONV", "all")
    pipe = PipelinedInference(net, xs[0], n_streams=2)
    for i in range(2):
        with torch.cuda.stream(pipe.stream(i)):
            pipe.input(i).copy_(xs[i])
    for _ in range(3):
        outs = [pipe.launch(i) for i in range(2)]
        pipe.synchronize()
        assert torch.equal(outs[0], want[0]) and torch.equal(outs[1], want[1])

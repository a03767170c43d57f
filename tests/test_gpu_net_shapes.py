"""Whole networks through the fused executors at odd, non-square and small resolutions (the table, the float64 reference
and the judge: tests/net_shapes.py).  For every family and input:

  1. the per-layer path, judged against the float64 reference;
  2. the fused executor with a tap on every binary convolution's input planes, judged against the float64 reference;
  3. the fused executor without a tap — the run that takes the one-launch forms a tap switches off: the tapped logits, bit
     for bit;
  4. ``capture`` + a replay: the eager logits; ``net(x)`` through AutoFusion: the executor's logits;
  5. the first and the last image alone: their rows of the full batch;
  6. the matrix-core switches all off, all on, on with the FP4 forms off, and at their defaults — and the defaults planned
     for several batches in flight (``throughput_mode``): the same logits and the same planes in front of every binary
     convolution.

Then: a hierarchical-block network with two blocks in its late stages at 112 x 112, where the first block of a stage meets
7 x 7 at 256 channels (its shortcut convolution inside a channel-lane launch); the default tables route launches of the
224 x 160 input (56 x 40, 28 x 20, ... : their keys hold no width) to each matrix-core form, and the table reached both
sides of every shape-keyed decision of bnn_amd/executor.py.
"""
import contextlib
import json

import pytest
import torch

import bnn_amd as bnn
from bnn_amd import executor, fastpath
from bnn_amd.executor import Form, HForm
from bnn_amd.inference import FusedResNet, auto_fusion, per_layer_forward, tap_binary_inputs
from bnn_amd.models import HBlock, ResNet
from tests import net_shapes as ns
from tests.test_gpu_mfma_net import DENSE, FOLD, FP4, _convs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SWITCHES = ("MFMA_CONV", "MFMA_FOLD", "MFMA_F4", "MFMA_1X1")
MODES = {"1": ("1", "1", "1", "1"),                 # the defaults: the tables of fastpath
         "0": ("0", "0", "0", "0"),                 # the popcount kernels only
         "all": ("all", "all", "all", "all"),       # every launch a matrix-core kernel's own query takes
         "i8": ("all", "all", "0", "all"),          # ... with the 3x3 and fold launches in their int8 form
         "tp": ("1", "1", "1", "1")}                # the defaults, planned for several batches in flight (throughput_mode)

JUDGED = {"per_layer": {}, "fused": {}}             # path -> {case id: Verdict.report()}
RAN = set()                                         # (case, mode) that went through _forward
POOLS = {}                                          # (N, C, H, W) in front of a stage's AvgPool2d -> _pool_into_hblock took it
POOL_ASKED = set()                                  # (H, W) that _H.route asked hipops.hblock_pool_supported about


# ------------------------------------------------------------------------------------------------------------- fixtures
@pytest.fixture(scope="module")
def nets():
    held = {}

    def get(family):
        if family not in held:
            held[family] = ns.build(family).to(DEV)
        return held[family]
    yield get
    held.clear()


@pytest.fixture(scope="module")
def engines():
    held = {}                                       # (family, mode) -> FusedResNet, planned and run under that mode only
    yield held
    held.clear()


def _switch(monkeypatch, mode):
    # read when an executor plans its layers AND when a launch's form is decided (its first run at a geometry)
    for name, value in zip(SWITCHES, MODES[mode]):
        monkeypatch.setattr(fastpath, name, value)


def _engine(nets, engines, family, mode, monkeypatch):
    _switch(monkeypatch, mode)
    key = (family, mode)
    if key not in engines:
        engines[key] = FusedResNet(nets(family), throughput_mode=mode == "tp")
    return engines[key]


@contextlib.contextmanager
def _watch_pools():
    """Notes, for every AvgPool2d in front of a stage that ``_run_blocks`` reaches, whether ``_pool_into_hblock`` took it,
    and the sizes at which ``_H.route`` gets as far as the pooled form's own query."""
    orig, query = FusedResNet._pool_into_hblock, executor.hipops.hblock_pool_supported

    def asked(N, c_in, H, W, *args, **kw):
        POOL_ASKED.add((H, W))
        return query(N, c_in, H, W, *args, **kw)

    def spy(self, pool, nxt, t):
        out = orig(self, pool, nxt, t)
        if t is not None and executor._TAP is None:
            POOLS[tuple(t.shape)] = POOLS.get(tuple(t.shape), False) or out is not None
        return out
    FusedResNet._pool_into_hblock, executor.hipops.hblock_pool_supported = spy, asked
    try:
        yield
    finally:
        FusedResNet._pool_into_hblock, executor.hipops.hblock_pool_supported = orig, query


def _forward(engine, x):
    """(logits of the tapped run, {layer: (P, M, channels, nonneg)} in front of every binary convolution, logits of the
    run without a tap)."""
    planes = {}

    def tap(name, act):
        assert name not in planes, f"{name} tapped twice"
        planes[name] = (act.P.clone(), act.M.clone(), act.shape, act.nonneg)
    with tap_binary_inputs(tap):
        tapped = engine(x).clone()
    with _watch_pools():
        plain = engine(x).clone()
    return tapped, planes, plain


class _Case:
    def __init__(self, case):
        self.case, (self.family, self.shape) = case, case
        self.id = ns.case_id(case)
        self.x = ns.input_of(self.shape).to(DEV)
        self.ref = ns.r64(case)                     # computed once, shared by the tests of the case, never written
        self.runs = {}

    def run(self, nets, engines, mode, monkeypatch):
        if mode not in self.runs:
            self.runs[mode] = _forward(_engine(nets, engines, self.family, mode, monkeypatch), self.x)
            RAN.add((self.case, mode))
        return self.runs[mode]


@pytest.fixture(scope="module", params=ns.CASES, ids=ns.case_id)
def case(request):
    c = _Case(request.param)
    yield c
    c.runs.clear()


def _signs(planes):
    return {name: ns.unpack_planes(P, M, shape[1], nonneg).cpu().numpy() for name, (P, M, shape, nonneg) in planes.items()}


def _same_planes(a, b):
    assert sorted(a) == sorted(b)
    for name in a:
        (P0, M0, shape0, nn0), (P1, M1, shape1, nn1) = a[name], b[name]
        assert tuple(shape0) == tuple(shape1) and nn0 == nn1, name
        assert torch.equal(P0, P1), name
        assert nn0 or torch.equal(M0, M1), name     # (the M plane of a non-negative tensor: no reader looks at it)


def _record(path, c, verdict):
    rep = verdict.report()
    JUDGED[path][c.id] = rep
    print(json.dumps({"path": path, "case": c.id, **rep}))
    assert not verdict.failures, verdict.failures


# ---------------------------------------------------------------------------------------------- 1, 2: against float64
def test_per_layer_path_against_float64(case, nets):
    net = nets(case.family)
    with per_layer_forward():
        y, order, values = ns.tap_inputs(net, lambda: net(case.x), keep=lambda t: t.detach().float().cpu().numpy())
    assert order == case.ref.names
    _record("per_layer", case, ns.judge(values, y, case.ref))


def test_fused_executor_against_float64(case, nets, engines, monkeypatch):
    if ns.JUDGED_STEM_EXACT:
        _switch(monkeypatch, "1")
        key = (case.family, "1", "exact-stem")
        if key not in engines:
            engines[key] = FusedResNet(nets(case.family), stem_exact_fp32=True)
        y, planes, _ = _forward(engines[key], case.x)
    else:
        y, planes, _ = case.run(nets, engines, "1", monkeypatch)
    _record("fused", case, ns.judge(_signs(planes), y, case.ref))


# ------------------------------------------------------------------------------------------------- 3 .. 6: bit for bit
def test_untapped_run_gives_the_tapped_logits(case, nets, engines, monkeypatch):
    tapped, planes, plain = case.run(nets, engines, "1", monkeypatch)
    assert sorted(planes) == sorted(case.ref.names)
    assert plain.shape == (case.shape[0], 1000) and torch.isfinite(plain).all()
    assert torch.equal(plain, tapped)


def test_captured_replay_and_the_model_call(case, nets, engines, monkeypatch):
    _, _, want = case.run(nets, engines, "1", monkeypatch)
    net = nets(case.family)
    fresh = FusedResNet(net)
    eager = fresh(case.x).clone()
    assert torch.equal(eager, want)
    fresh.capture(case.x)
    assert fresh._graph is not None and torch.equal(fresh(case.x), eager)
    assert torch.equal(fresh(case.x), eager)                       # a second replay
    auto = auto_fusion(net)
    before = auto.calls["eager"] + auto.calls["graph"]
    with torch.no_grad():
        y_call = net(case.x)                                        # AutoFusion: the executor the model call builds
    assert auto.engine is not None and auto.calls["eager"] + auto.calls["graph"] == before + 1
    assert torch.equal(y_call, want)


def test_first_and_last_image_alone(case, nets, engines, monkeypatch):
    N = case.shape[0]
    if N == 1:
        return                                                      # (the batch is its own slice)
    _, _, want = case.run(nets, engines, "1", monkeypatch)
    eng = _engine(nets, engines, case.family, "1", monkeypatch)
    assert torch.equal(eng(case.x[:1]), want[:1])
    assert torch.equal(eng(case.x[N - 1:]), want[N - 1:])


@pytest.mark.parametrize("mode", ["0", "all", "i8", "tp"])
def test_matrix_core_switches_change_no_bit(case, mode, nets, engines, monkeypatch):
    tapped1, planes1, plain1 = case.run(nets, engines, "1", monkeypatch)
    tapped, planes, plain = case.run(nets, engines, mode, monkeypatch)
    assert torch.equal(plain, plain1) and torch.equal(tapped, tapped1)
    _same_planes(planes, planes1)
    forms = {f for c in _convs(engines[(case.family, mode)]) for f in c.routes.values()}
    if mode == "0":
        assert forms == {Form.POPCOUNT}
    if mode == "i8":
        assert not forms & FP4


LATE = (2, 3, 112, 112)     # HBlock stages of 1, 1, 2, 2 blocks at 28x28, 14x14, 7x7, 3x3
LATE_RUNS = {}


def _late(engines, monkeypatch):
    """A hierarchical block with a shortcut convolution and a block behind it in its stage, at 7 x 7 and 256 channels (the
    channel-lane kernel takes widths from 256 on; the table's network has one block in each of its last two stages)."""
    if not LATE_RUNS:
        net = bnn.prepare_binary_model(ResNet(HBlock, [1, 1, 2, 2], num_classes=1000), ns._cfg(),
                                       custom_config_layers_name={"conv1": bnn.BConfig(), "fc": bnn.BConfig()})
        shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
        net.load_state_dict({k: torch.from_numpy(v) for k, v in ns.gen.model_state(shapes, 4).items()})
        net, x = net.eval().to(DEV), ns.input_of(LATE).to(DEV)
        for mode in ("1", "tp"):
            _switch(monkeypatch, mode)
            eng = engines[("hblock_late", mode)] = FusedResNet(net, throughput_mode=mode == "tp")
            LATE_RUNS[mode] = _forward(eng, x)
    return LATE_RUNS


def test_hblock_shortcut_launch_in_channel_lanes(engines, monkeypatch):
    """No network of the table puts a hierarchical block with a shortcut convolution in front of another block of its
    stage at a width and size the channel-lane kernel takes.  Here the run without a tap takes that launch; the tapped run
    goes launch by launch: the same logits and planes, alone and with several batches in flight."""
    runs = _late(engines, monkeypatch)
    for tapped, planes, plain in runs.values():
        assert plain.shape == (2, 1000) and torch.isfinite(plain).all() and torch.equal(plain, tapped)
    assert torch.equal(runs["tp"][2], runs["1"][2])
    _same_planes(runs["tp"][1], runs["1"][1])
    shortcut = {r.channel_lanes for mode in runs for b in engines[("hblock_late", mode)]._blocks if b.kind == "h"
                for r in b.routes.values() if r.form is HForm.SHORTCUT}
    assert True in shortcut


# ------------------------------------------------------------------------------------------- what the table reached
def _ensure(nets, engines, monkeypatch, modes=tuple(MODES), cases=ns.CASES):
    """The runs above, for whatever part of the table this session has not run (a selection with -k)."""
    for c in cases:
        for mode in modes:
            if (c, mode) not in RAN:
                _forward(_engine(nets, engines, c[0], mode, monkeypatch), ns.input_of(c[1]).to(DEV))
                RAN.add((c, mode))


def _routes(engines, mode=None):
    for (family, m, *_), eng in engines.items():
        if mode is None or m == mode:
            for c in _convs(eng):
                for key, form in c.routes.items():
                    yield family, c, key, form


def test_default_tables_match_at_a_foreign_width(nets, engines, monkeypatch):
    """The route tables are keyed on C, O, H: at 224 x 160 the stages are 56 x 40, 28 x 20, 14 x 10 and 7 x 5, and the
    default must send launches there to each of the four matrix-core forms."""
    shape = (2, 3, 224, 160)
    _ensure(nets, engines, monkeypatch, modes=("1",), cases=[(f, shape) for f in ns.FAMILIES])
    sizes = set(ns.STAGES[shape])
    took = {}
    for family, c, key, form in _routes(engines, "1"):
        if key.shape[0] == 2 and tuple(key.shape[2:]) in sizes and form is not Form.POPCOUNT:
            took.setdefault(form, set()).add((family, c.name, tuple(key.shape)))
    print(json.dumps({str(f.value): sorted(map(str, v)) for f, v in took.items()}))
    assert DENSE & set(took), "no dense 3x3 launch on the matrix cores"
    assert FOLD & set(took), "no folded-shortcut launch on the matrix cores"
    assert FP4 & set(took), "no launch in an FP4 3x3 form"
    assert Form.F4_1X1 in took, "no 1x1 launch on the FP4 kernel"
    nonneg = {k.nonneg for _, c, k, f in _routes(engines, "1") if f is Form.F4_1X1 and tuple(k.shape[2:]) in sizes}
    assert nonneg == {True, False}                      # MFMA_1X1_SHAPES and MFMA_1X1_TERNARY_SHAPES


def test_the_table_reached_both_sides_of_every_decision(nets, engines, monkeypatch):
    _ensure(nets, engines, monkeypatch)
    _late(engines, monkeypatch)
    missing = []

    def need(cond, what):
        if not cond:
            missing.append(what)

    # hierarchical blocks: b.routes[(N, H, W)]
    pooled_hit, pooled_small, pooled_odd, lanes, pixels, refused, sc = set(), set(), set(), set(), set(), set(), set()
    reached = set()
    for (family, *_), eng in engines.items():
        blocks = eng._blocks
        for i, b in enumerate(blocks):
            if b.kind != "h" or b.hpack is None:
                continue
            ends_stage = i + 1 < len(blocks) and blocks[i + 1].kind == "pool"
            assert ends_stage == (b.end_pool is not None) and (b.behind is blocks[i + 2] if ends_stage else b.behind is None)
            for (N, H, W), r in b.routes.items():
                reached.add((r.form, r.channel_lanes))
                (lanes if r.channel_lanes else refused if r.form is HForm.STEPS else pixels).add((H, W))
                if b.hsc is not None:
                    sc.add(r.form is HForm.SHORTCUT)
                if ends_stage and r.form in (HForm.POOLED, HForm.ONE):      # the pooled form was considered
                    if r.form is HForm.POOLED:
                        assert r.pool_consts is not None
                        pooled_hit.add((H, W))
                    elif H % 2 or W % 2:
                        pooled_odd.add((H, W))
                    elif H * W < 784:
                        pooled_small.add((H, W))
    need(pooled_hit, "_pooled_form: a hit")
    need(pooled_small, "_pooled_form: a decline on size")
    need(pooled_odd, "_pooled_form: a decline on oddness")
    # the two declines are the executor's own: the kernel's query (which refuses odd sizes too) is asked at neither —
    # one odd stage end of the table, 53 x 56, is large enough for the size rule to pass it on
    need(any(H * W >= 784 for H, W in pooled_odd), "_pooled_form: a decline on oddness at a size the size rule admits")
    need(POOL_ASKED and pooled_hit <= POOL_ASKED and all(H % 2 == 0 and W % 2 == 0 and H * W >= 784 for H, W in POOL_ASKED),
         f"_pooled_form asks the kernel at even sizes of 784 pixels or more alone: asked at {sorted(POOL_ASKED)}")
    need(any(POOLS.values()), "_pool_into_hblock: a hit")
    need(any(not hit and (s[2] % 2 or s[3] % 2) for s, hit in POOLS.items()), "_pool_into_hblock: a decline at an odd size")
    # (the channel-lane kernel is built for 7 x 7 and 14 x 14 alone: csrc/hblock_cl.hip.  _H.route asks for it at H == 7,
    #  and at every size with several batches in flight; at 7 x 5 the kernel's own query says no and pixel lanes run)
    need((7, 7) in lanes, "the channel-lane form at 7 x 7")
    need(any(W != 7 for _, W in lanes), "the channel-lane form at a width other than 7")
    need((7, 5) in pixels, "channel lanes asked for at 7 x 5, refused by the kernel's query, pixel lanes taken")
    need(any(H != W for H, W in pixels), "the pixel-lane form at a non-square size")
    need(True in sc, "the shortcut convolution inside the hierarchical block's launch")
    for form, channel_lanes in ((HForm.ONE, False), (HForm.ONE, True), (HForm.SHORTCUT, False), (HForm.SHORTCUT, True),
                                (HForm.POOLED, False)):
        need((form, channel_lanes) in reached, f"{form.name} in {'channel' if channel_lanes else 'pixel'} lanes")
    # (a geometry hblock_supported refuses in both forms: none exists in the table — printed below, were one to appear)
    # the folded shortcut: b.fold_geo[(images per launch, Ho, Wo)]
    fold = set()
    for eng in engines.values():
        for b in eng._blocks:
            if b.kind == "post":
                fold |= {(ok, bool(ho % 2 or wo % 2)) for (_, ho, wo), ok in b.fold_geo.items()}
    need((True, True) in fold, "the folded shortcut taken at an odd size")
    need((False, True) in fold, "the folded shortcut refused at an odd size")
    need((True, False) in fold and (False, False) in fold, "the folded shortcut taken and refused at an even size")
    # every kernel form at a non-square shape
    forms = {form for _, _, key, form in _routes(engines) if key.shape[2] != key.shape[3]}
    for form in Form:
        need(form in forms, f"{form.value} at a non-square shape")
    print(json.dumps({"pooled_hit": sorted(pooled_hit), "pooled_small": sorted(pooled_small), "pooled_odd": sorted(pooled_odd),
                      "pools": {str(k): v for k, v in sorted(POOLS.items())}, "channel_lanes": sorted(lanes),
                      "pixel_lanes": sorted(pixels), "hblock_refused": sorted(refused), "fold": sorted(fold),
                      "shortcut_in_hblock": sorted(sc),
                      "pool_asked": sorted(POOL_ASKED)}))
    assert not missing, missing


def test_at_most_one_image_in_four_diverged():
    """Rule 3 of the judge over the table, per path; prints what diverged and where."""
    for path, reports in JUDGED.items():
        images = sum(r["images"] for r in reports.values())
        diverged = {cid: r["diverged"] for cid, r in reports.items() if r["diverged"]}
        print(json.dumps({"path": path, "cases": len(reports), "images": images, "diverged": diverged}))
        assert sum(len(d) for d in diverged.values()) <= ns.MAX_DIVERGED * images, diverged

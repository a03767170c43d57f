"""How every hierarchical block of the fused executor runs (``executor._H.route``) and what ``executor._link_hblocks`` records
at plan time, without a GPU: both are pure Python once ``hblock_supported``, ``hblock_shortcut_supported``,
``hblock_pool_supported``, ``hblock_pool_consts`` and the two pack functions of ``hipops`` are stubbed.  Short chains of
``_H`` / ``_Pool`` / ``_Post`` records are built by hand from CPU layers; over every block position and disqualifying recipe,
eight geometries, both throughput modes, the five ``BNN_AMD_*HBLOCK*`` variables and every answer of the queries, the
links, the packs and ``route`` equal an oracle written out here from the wording of ``_H.route`` and ``_link_hblocks`` (it
reads the chains' specifications and no function of ``executor``), ``route`` asks exactly the oracle's queries in its order
with the block's own arguments and nothing the second time, a tapped run asks and caches nothing, and no producer drops
the fp32 tensor in front of a block that runs launch by launch."""
import itertools
from typing import NamedTuple, Optional

import pytest
import torch
import torch.nn as nn

from bnn_amd import BConfig, Identity, executor, fastpath, hipops, native
from bnn_amd.executor import FusedResNet, HForm, _Conv, _H, _Pool, _Post
from bnn_amd.layers import Conv2d as BinaryConv2d
from bnn_amd.ops import BasicInputBinarizer, XNORWeightBinarizer

T = torch.empty(0)
N = 2
GEOMETRIES = [(N, 56, 56), (N, 53, 56), (N, 28, 28), (N, 27, 28), (N, 14, 14), (N, 14, 10), (N, 7, 7), (N, 7, 5)]
CFG = BConfig(activation_pre_process=BasicInputBinarizer, activation_post_process=Identity,
              weight_pre_process=XNORWeightBinarizer)
NO_INSTANCE = 192           # a width (a multiple of 64) for which the stubbed ``hblock_pack`` raises, as the kernel's would
POOL2, POOL3, POST = "AvgPool2d(2, 2)", "AvgPool2d(3, 2, 1)", "a BasicBlock"


class Spec(NamedTuple):
    """One hierarchical block: ``c_in`` -> ``planes`` channels; ``prelu``: which of its three activations is a PReLU."""
    c_in: int
    planes: int
    ds: bool = False                    # a shortcut: BatchNorm -> binary 1x1
    prelu: Optional[int] = None
    bias: bool = False
    zero: bool = False                  # a zero among the weights
    widths: Optional[tuple] = None      # output channels of the three convolutions, where not planes / 2, / 4, / 4

    def outs(self):
        return self.widths or (self.planes // 2, self.planes // 4, self.planes // 4)


CHAINS = [
    # first block of a stage with a shortcut, a middle block, a stage end in front of a pool and a block with a shortcut,
    # a stage end in front of a pool and another kind of block, which is the last of the network
    [Spec(64, 128, ds=True), Spec(128, 128), Spec(128, 128), POOL2, Spec(128, 256, ds=True), Spec(256, 256), POOL2, POST],
    # a successor whose first activation is a PReLU (in the stage, and behind the pool); a block with a PReLU of its own,
    # last of the network
    [Spec(128, 128), Spec(128, 128, prelu=0), POOL2, Spec(128, 256, ds=True, prelu=0), Spec(256, 256, prelu=1)],
    # the recipes without a one-launch form, each behind a pool that could have fed it and in front of a block that does qualify
    [Spec(128, 128), POOL2, Spec(128, 128, ds=True, bias=True), Spec(128, 128), POOL2, Spec(128, 128, ds=True, zero=True),
     Spec(128, 128, ds=True), Spec(128, 128, widths=(64, 32, 16)), Spec(128, 96), Spec(96, 96),
     Spec(96, NO_INSTANCE, ds=True), Spec(NO_INSTANCE, NO_INSTANCE)],
    # a pool that is not 2 x 2, a block behind a pool that has no shortcut, a pool that ends the network, a shortcut of
    # another width ratio, and a next block of another input width
    [Spec(128, 128), POOL3, Spec(128, 128, ds=True), POOL2, Spec(128, 128), Spec(128, 128, ds=True), Spec(64, 128), POOL2],
    # stages of one block: the block changes its width, so its launch cannot pool its own output
    [Spec(64, 128, ds=True), POOL2, Spec(128, 256, ds=True), POOL2, Spec(256, 256, ds=True), Spec(256, 256)],
]


# ------------------------------------------------------------------------------------------------------------ the oracle
class Oracle:
    """The rule, from the specifications alone.  ``fuse`` / ``shortcut`` / ``cl`` / ``pool``: the four switches are on;
    ``pool_min``: pixels; ``yes``: the answers of the queries."""

    def __init__(self, chain, fuse, shortcut, cl, pool, pool_min, thr, yes):
        self.chain, self.fuse, self.shortcut, self.cl, self.pool, self.pool_min = chain, fuse, shortcut, cl, pool, pool_min
        self.thr, self.yes, self.decided, self.asked = thr, yes, {}, []

    def at(self, i):
        return self.chain[i] if i is not None and i < len(self.chain) else None

    def next(self, i):                  # the next block of the stage
        return i + 1 if self.at(i + 1) not in (None, POOL2, POOL3) else None

    def behind(self, i):                # the block behind the AvgPool2d(2, 2) that ends the stage
        return i + 2 if self.at(i + 1) == POOL2 and self.at(i + 2) is not None else None

    def takes_planes(self, j, channels):
        s = self.at(j)
        return isinstance(s, Spec) and self.has_pack(j) and s.prelu != 0 and s.c_in == channels

    def qualifies(self, i):             # ``hblock_pack`` is asked for the one-launch pack
        s = self.chain[i]
        return (self.fuse and s.prelu is None and not s.bias and not s.zero and s.planes % 64 == 0
                and s.outs() == (s.planes // 2, s.planes // 4, s.planes // 4))

    def has_pack(self, i):
        return self.qualifies(i) and self.chain[i].planes != NO_INSTANCE

    def has_next(self, i):              # the launch writes the next block's input planes
        s, j = self.chain[i], self.next(i)
        return j is not None and isinstance(self.at(j), Spec) and self.at(j).prelu != 0 and self.at(j).c_in == s.planes

    def has_shortcut_pack(self, i):
        s = self.chain[i]
        return self.has_pack(i) and s.ds and self.has_next(i) and s.c_in * 2 == s.planes and self.shortcut

    def route(self, i, n, H, W):
        if (i, n, H, W) not in self.decided:
            self.decided[(i, n, H, W)] = self.decide(i, n, H, W)
        return self.decided[(i, n, H, W)]

    def decide(self, i, n, H, W):
        """(form, channel lanes, has pool constants)"""
        s = self.chain[i]
        if not self.has_pack(i):
            return HForm.STEPS, False, False
        geo = (n, s.c_in, H, W, s.planes, self.thr)

        def ask(q, answer, args=geo, **kw):
            self.asked.append((q, args, kw))
            return self.yes[answer]

        cl = self.cl and (H == 7 or self.thr) and ask("hblock_supported", "cl", channel_lanes=True)
        if not cl and not ask("hblock_supported", "px"):
            return HForm.STEPS, False, False
        if self.has_shortcut_pack(i) and ask("hblock_shortcut_supported", "sc", channel_lanes=cl):
            return HForm.SHORTCUT, cl, False
        j = self.behind(i)
        if (self.pool and j is not None and self.takes_planes(j, s.planes) and self.at(j).ds and H % 2 == 0 and W % 2 == 0
                and s.c_in == s.planes and H * W >= self.pool_min and self.route(j, n, H // 2, W // 2)[0] is not HForm.STEPS
                and ask("hblock_pool_supported", "pool")
                and ask("hblock_pool_consts", "consts", args=(("bn1", j), ("ds_bn", j), s.planes))):
            return HForm.POOLED, False, True
        return HForm.ONE, cl, False


# --------------------------------------------------------------------------------------------------- records and stubs
def _conv(c_in, c_out, k, bias=False, zero=False):
    with torch.device("meta"):
        layer = BinaryConv2d(c_in, c_out, k, padding=k // 2, bias=bias, bconfig=CFG)
    empty = torch.empty(0, dtype=torch.int32)
    weight = hipops.PackedWeight(empty, empty, T, zero, (c_out, c_in, k, k))
    return _Conv(layer, fastpath.Plan(False, True, None), weight, None, None, relu=False, prelu=None)


def records(chain, thr):
    out = []
    for s in chain:
        if s in (POOL2, POOL3):
            out.append(_Pool(nn.AvgPool2d(2, 2) if s == POOL2 else nn.AvgPool2d(3, 2, 1)))
        elif s == POST:
            out.append(_Post([_conv(256, 256, 3), _conv(256, 256, 3)]))
        else:
            o1, o2, o3 = s.outs()
            b = _H(planes=s.planes, bn=[(torch.empty(1), torch.empty(1)) for _ in range(3)],
                   relu=[k != s.prelu for k in range(3)],
                   convs=[_conv(s.c_in, o1, 3, s.bias, s.zero), _conv(o1, o2, 3), _conv(o2, o3, 3)], throughput=thr)
            if s.ds:
                b.ds_bn, b.ds = (torch.empty(1), torch.empty(1)), _conv(s.c_in, s.planes, 1)
            out.append(b)
    return out


@pytest.fixture
def stubs(monkeypatch):
    """``calls``: (name, positional arguments, keywords) of every stubbed call; ``yes``: the answers."""
    calls, yes = [], dict(cl=True, px=True, sc=True, pool=True, consts=True)

    def query(name, answer):
        def stub(*a, channel_lanes=None, **kw):
            assert not kw
            lanes = {} if channel_lanes is None else {"channel_lanes": channel_lanes}
            calls.append((name, a, lanes))
            return yes["cl" if name == "hblock_supported" and channel_lanes else answer]
        return stub

    def consts(*a):
        calls.append(("hblock_pool_consts", a, {}))
        if not yes["consts"]:
            raise native.NativeError("a scale that cannot take the 1 / 4")
        return T

    def pack(w1, w2, w3, bn2, bn3, next_bn=None):
        calls.append(("hblock_pack", (w1, w2, w3, bn2, bn3, next_bn), {}))
        if 2 * w1.shape[0] == NO_INSTANCE:
            raise native.NativeError("no instance")
        return hipops.HBlockPack(T, T, w1.shape[1], 2 * w1.shape[0], next_bn is not None, (w1, w2, w3))

    def shortcut_pack(w):
        calls.append(("hblock_shortcut_pack", (w,), {}))
        return (T, T)
    monkeypatch.setattr(hipops, "hblock_supported", query("hblock_supported", "px"))
    monkeypatch.setattr(hipops, "hblock_shortcut_supported", query("hblock_shortcut_supported", "sc"))
    monkeypatch.setattr(hipops, "hblock_pool_supported", query("hblock_pool_supported", "pool"))
    monkeypatch.setattr(hipops, "hblock_pool_consts", consts)
    monkeypatch.setattr(hipops, "hblock_pack", pack)
    monkeypatch.setattr(hipops, "hblock_shortcut_pack", shortcut_pack)
    # what a producer that takes its pool launches: no part of the decision
    monkeypatch.setattr(hipops, "avgpool2_bn_pack2", lambda t, bn1, relu1, bn2, relu2, out_f32: (T, T, T if out_f32 else None))
    return calls, yes


VARIABLES = ("FUSE_HBLOCK", "HBLOCK_SHORTCUT", "HBLOCK_CL", "HBLOCK_POOL", "HBLOCK_POOL_MIN")


@pytest.fixture(autouse=True)
def unset(monkeypatch):
    _setenv(monkeypatch, **dict.fromkeys(VARIABLES))


def _setenv(monkeypatch, **values):
    for name, value in values.items():
        if value is None:
            monkeypatch.delenv("BNN_AMD_" + name, raising=False)
        else:
            monkeypatch.setenv("BNN_AMD_" + name, value)


def _link(recs):
    """As ``FusedResNet`` does: ``BNN_AMD_FUSE_HBLOCK`` when it is built, ``BNN_AMD_HBLOCK_SHORTCUT`` at ``refresh``."""
    executor._link_hblocks(recs, executor._hblock_env("FUSE_HBLOCK") != "0", executor._hblock_env("HBLOCK_SHORTCUT") != "0")


def _resolve(recs, call):
    """A stubbed call with its tensor operands named as the oracle names them."""
    name, a, kw = call
    if name == "hblock_pool_consts":
        who = {id(b.bn[0]): ("bn1", j) for j, b in enumerate(recs) if b.kind == "h"}
        who.update({id(b.ds_bn): ("ds_bn", j) for j, b in enumerate(recs) if b.kind == "h" and b.ds_bn is not None})
        a = (who[id(a[0])], who[id(a[1])], a[2])
    return name, a, kw


def check_links(recs, o, calls):
    """The plan-time half: neighbours, packs and what the pack functions were handed."""
    want = []
    for i, b in enumerate(recs):
        if b.kind != "h":
            continue
        assert b.next is (None if o.next(i) is None else recs[o.next(i)]), i
        j = o.behind(i)
        assert (b.end_pool, b.behind) == ((None, None) if j is None else (recs[i + 1].mod, recs[j])), i
        s = o.chain[i]
        if o.qualifies(i):
            nbn = recs[o.next(i)].bn[0] if o.has_next(i) else None
            want.append(("hblock_pack", (*(c.weight for c in b.convs), b.bn[1], b.bn[2], nbn), {}))
        assert (b.hpack is not None) == o.has_pack(i), i
        if o.has_pack(i):
            assert (b.hpack.c_in, b.hpack.planes, b.hpack.has_next) == (s.c_in, s.planes, o.has_next(i)), i
        if o.has_shortcut_pack(i):
            want.append(("hblock_shortcut_pack", (b.ds.weight,), {}))
        assert (b.hsc is not None) == o.has_shortcut_pack(i), i
    assert len(calls) == len(want)
    for got, w in zip(calls, want):
        assert got[0] == w[0] and len(got[1]) == len(w[1]) and all(x is y for x, y in zip(got[1], w[1])), (got, w)


def check_routes(recs, o, calls, geometry):
    """The per-geometry half, block by block in the order of the chain (so a block behind a pool may have been decided by
    the stage end in front of it: then it asks nothing itself, in the oracle and in ``route``)."""
    n, H, W = geometry
    for i, b in enumerate(recs):
        if b.kind != "h":
            continue
        del calls[:], o.asked[:]
        form, cl, has_consts = o.route(i, n, H, W)
        r = b.route(n, H, W)
        assert (r.form, r.channel_lanes, r.pool_consts is not None) == (form, cl, has_consts), (i, geometry)
        assert [_resolve(recs, c) for c in calls] == o.asked, (i, geometry)
        assert b.route(n, H, W) is r and len(calls) == len(o.asked)             # the second call asks nothing
        if form is HForm.POOLED:            # no fp32 tensor is left: the consumer must not run launch by launch
            assert recs[i + 2].routes[(n, H // 2, W // 2)].form is not HForm.STEPS
    for i, b in enumerate(recs):            # the other producer that may leave no fp32 tensor: the pool in front of a stage
        if b.kind == "pool" and 0 < i < len(recs) - 1 and recs[i - 1].kind == "h":
            nxt = recs[i + 1]
            t = torch.empty((n, recs[i - 1].planes, H, W), device="meta")
            out = FusedResNet._pool_into_hblock(None, b.mod, nxt, t)
            if out is not None:
                assert o.chain[i] == POOL2 and H % 2 == 0 and W % 2 == 0 and o.takes_planes(i + 1, t.shape[1])
                assert out[2].owner is nxt and (out[0] is None) == (nxt.ds_bn is not None)
                assert nxt.routes[(n, H // 2, W // 2)].form is not HForm.STEPS
            else:
                assert not (o.chain[i] == POOL2 and H % 2 == 0 and W % 2 == 0 and o.takes_planes(i + 1, t.shape[1])
                            and o.route(i + 1, n, H // 2, W // 2)[0] is not HForm.STEPS)


# ------------------------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("thr", [False, True], ids=["alone", "throughput"])
@pytest.mark.parametrize("fuse", [None, "0"], ids=["fuse", "fuse0"])
@pytest.mark.parametrize("shortcut", [None, "0"], ids=["shortcut", "shortcut0"])
def test_route_and_links_equal_the_oracle(monkeypatch, stubs, thr, fuse, shortcut):
    calls, yes = stubs
    _setenv(monkeypatch, FUSE_HBLOCK=fuse, HBLOCK_SHORTCUT=shortcut)
    forms = set()
    for chain in CHAINS:
        del calls[:]
        recs = records(chain, thr)
        _link(recs)
        check_links(recs, Oracle(chain, fuse is None, shortcut is None, True, True, 784, thr, yes), calls)
        for cl, pool, pool_min in itertools.product((None, "0"), (None, "0"), (None, "0", "100000")):
            _setenv(monkeypatch, HBLOCK_CL=cl, HBLOCK_POOL=pool, HBLOCK_POOL_MIN=pool_min)
            for answers in itertools.product((True, False), repeat=len(yes)):
                yes.update(zip(yes, answers))
                for geometry in GEOMETRIES:
                    for b in recs:
                        if b.kind == "h":
                            b.routes.clear()
                    o = Oracle(chain, fuse is None, shortcut is None, cl is None, pool is None,
                               784 if pool_min is None else int(pool_min), thr, yes)
                    check_routes(recs, o, calls, geometry)
                    forms |= {(f, lanes) for f, lanes, _ in o.decided.values()}
    want = {(HForm.STEPS, False)}
    if fuse is None:                        # every form was reached, in both lane forms where it has them
        want |= {(HForm.ONE, False), (HForm.ONE, True), (HForm.POOLED, False)}
        if shortcut is None:
            want |= {(HForm.SHORTCUT, False), (HForm.SHORTCUT, True)}
    assert forms == want


def test_the_defaults_on_a_stage(stubs):
    """The first chain as an HBlock ResNet meets it, every query answering yes and no variable set."""
    calls, _ = stubs
    recs = records(CHAINS[0], False)
    _link(recs)
    a, b, c, _, d, e, _, _ = recs
    assert [x.route(N, 56, 56).form for x in (a, b, c)] == [HForm.SHORTCUT, HForm.ONE, HForm.POOLED]
    assert [x.route(N, 28, 28).form for x in (d, e)] == [HForm.SHORTCUT, HForm.ONE]       # (e: no block that takes planes)
    assert c.route(N, 14, 14).form is HForm.ONE and c.route(N, 53, 56).form is HForm.ONE  # below 784 pixels; odd
    assert not b.route(N, 14, 14).channel_lanes and b.route(N, 7, 7).channel_lanes
    assert ("hblock_pool_supported", (N, 128, 56, 56, 128, False), {}) in calls
    assert not [q for q in calls if q[0] == "hblock_pool_supported" and q[1][2:4] != (56, 56)]


def test_a_tapped_run_asks_nothing_and_caches_nothing(monkeypatch, stubs):
    calls, _ = stubs
    monkeypatch.setattr(hipops, "bn_act_pack", lambda t, *a, **kw: hipops.PackedAct(T, T, tuple(t.shape), kw["relu"]))
    monkeypatch.setattr(_Conv, "run", lambda self, act, **kw: (None, act))
    for chain in CHAINS:
        recs = records(chain, False)
        _link(recs)
        del calls[:]
        with executor.tap_binary_inputs(lambda name, act: None):
            for i, b in enumerate(recs):
                if b.kind == "h":
                    t = torch.empty((N, chain[i].c_in, 56, 56), device="meta")
                    y, planes, left = FusedResNet._run_h(None, b, t)
                    assert y.shape == (N, b.planes, 56, 56) and planes is None and left is None
                elif b.kind == "pool" and i + 1 < len(recs):
                    t = torch.empty((N, 128, 56, 56), device="meta")
                    assert FusedResNet._pool_into_hblock(None, b.mod, recs[i + 1], t) is None
        assert not calls and not any(b.routes for b in recs if b.kind == "h")

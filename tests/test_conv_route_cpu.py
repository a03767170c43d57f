"""The kernel form of every binary-convolution launch of the fused ResNet executor (``executor._Conv.route``), without a
GPU: the decision is pure Python once the five ``hipops.*_supported`` queries are stubbed.  Over all 81 settings of the four
switches, every key of the five admission tables, the declined shapes their comments name and one launch of each kind with
a disqualifying argument, ``route`` equals an oracle written out here from the rule's own wording (it reads the tables of
``fastpath`` but calls none of its functions), asks exactly the queries the oracle expects, in its order, hands them the
launch's own description, and asks none of them a second time."""
import itertools
from typing import NamedTuple, Optional

import pytest
import torch

from bnn_amd import BConfig, Identity, fastpath, hipops, native
from bnn_amd.executor import Form, RouteKey, _Conv
from bnn_amd.layers import Conv2d as BinaryConv2d
from bnn_amd.ops import BasicInputBinarizer, XNORWeightBinarizer

SWITCHES = ("MFMA_CONV", "MFMA_FOLD", "MFMA_F4", "MFMA_1X1")
QUERIES = ("bconv2d_mfma_supported", "bconv2d_mfma4_supported", "bconv2d_mfma_fold_supported",
           "bconv2d_mfma4_fold_supported", "bconv1x1_mfma4_supported")
EPI_1X1 = {"residual_after_act", "pack_before_residual", "pack_relu", "pack_scale", "pack_shift"}
ALL_PACKS = frozenset({Form.I8_3X3, Form.F4_3X3, Form.F4_1X1})
T = torch.empty(0)          # stands for any tensor operand: ``route`` only asks whether it is there
N = 2
CFG = BConfig(activation_pre_process=BasicInputBinarizer, activation_post_process=Identity,
              weight_pre_process=XNORWeightBinarizer)


class Launch(NamedTuple):
    """One launch: the layer (C -> O, kernel ``k``, ``stride``), its input (H x H planes) and the arguments of ``run``."""
    k: int
    C: int
    O: int
    H: int
    stride: int = 1
    nonneg: bool = True
    residual: bool = False
    out_f32: bool = False
    out_packed: bool = True
    thr: bool = False
    epi: tuple = ()                         # ((name, value), ...)
    shortcut: Optional[tuple] = None        # (channels, H) of the folded shortcut's planes
    shortcut_w8: bool = False
    packs: frozenset = ALL_PACKS            # what the plan built, before the kernel size sorts it out
    prelu: bool = False


def dense(C, O, H, stride, **kw):
    """The two launches of a BasicBlock's 3x3 convolutions: conv1 (planes only, thresholds) and conv2 (residual)."""
    return [Launch(3, C, O, H, stride, thr=True, **kw),
            Launch(3, C, O, H, stride, residual=True, out_f32=True, **kw)]


def fold(C, O, H, sc_C, sc_H=None, **kw):
    kw = dict(dict(out_f32=True, shortcut=(sc_C, sc_H or H), shortcut_w8=True), **kw)
    return Launch(3, C, O, H, **kw)


def one(C, O, H, out_f32, nonneg):
    """A 1x1 launch as the nets make it: behind ReLU conv1 writes planes and conv3 adds the residual; the pre-activation
    blocks carry the next BatchNorm as a pack affine and add the residual late."""
    epi = () if nonneg else (("pack_scale", T), ("pack_shift", T)) + ((("residual_after_act", True),) if out_f32 else ())
    return Launch(1, C, O, H, nonneg=nonneg, residual=out_f32, out_f32=out_f32, epi=epi)


def launches():
    out = []
    for key in list(fastpath.MFMA_CONV_SHAPES) + [k for k in fastpath.MFMA_F4_SHAPES if len(k) == 5]:
        assert key[4] is False
        out += dense(*key[:4])
    out += dense(64, 64, 56, 1) + dense(64, 128, 56, 2)                       # declined: layer1, layer2.0.conv1
    for key in list(fastpath.MFMA_FOLD_SHAPES) + [k for k in fastpath.MFMA_F4_SHAPES if len(k) == 4]:
        out += [fold(*key), fold(*key, sc_H=2 * key[2])]                      # the shortcut plane pooled and un-pooled
    for key in fastpath.MFMA_1X1_SHAPES:
        out.append(one(*key, nonneg=True))
    for key in fastpath.MFMA_1X1_TERNARY_SHAPES:
        out.append(one(*key, nonneg=False))
    out += [one(256, 512, 28, True, True), one(256, 512, 28, True, False),    # declined: the shortcuts
            one(512, 1024, 14, True, False), one(1024, 2048, 7, True, False)]
    # one disqualifying argument each
    out += [Launch(3, 256, 256, 14, epi=(("pack_relu", False),)),             # an ``epi`` key, though it is off
            Launch(1, 512, 128, 28, nonneg=False, epi=(("pack_scale", T),)),  # pack_scale without pack_shift
            Launch(1, 512, 128, 28, epi=(("out_c_offset", 0),)),              # a key the 1x1 kernel does not take
            fold(256, 256, 14, 128, out_packed=False),
            fold(256, 256, 14, 128, residual=True),
            fold(256, 256, 14, 128, prelu=True),
            fold(256, 256, 14, 128, shortcut_w8=False),                        # missing packs
            fold(256, 256, 14, 128, packs=frozenset({Form.I8_3X3})),
            fold(256, 256, 14, 128, packs=frozenset())]
    out += dense(256, 256, 14, 1, packs=frozenset()) + dense(256, 256, 14, 1, packs=frozenset({Form.I8_3X3}))
    out.append(one(512, 128, 28, False, True)._replace(packs=frozenset()))
    return list(dict.fromkeys(out))


LAUNCHES = launches()


def packs_of(L):
    """A 3x3 weight has no 1x1 pack and a 1x1 weight no 3x3 pack, whatever the plan wanted."""
    return L.packs & ({Form.F4_1X1} if L.k == 1 else {Form.I8_3X3, Form.F4_3X3})


def switch_says(own, in_table, *parents):
    """"0" in the form's switch or a parent's -> no; "all" -> yes; "1" -> the table."""
    return "0" not in (own,) + parents and (own == "all" or in_table)


def oracle(sw, L, yes):
    """(form, the queries asked in order) for the launch ``L`` under the switches ``sw`` = (conv, fold, f4, 1x1) when the
    query ``q`` answers ``yes[q]``: the rule of ``_Conv.route``'s docstring, line for line."""
    conv, fold_, f4, x1 = sw
    packs, names, asked = packs_of(L), {n for n, _ in L.epi} | ({"shortcut"} if L.shortcut else set()), []
    on = {n for n, v in L.epi if v is not None and v is not False}

    def ask(q):
        asked.append(q)
        return yes[q]

    if Form.F4_1X1 in packs and names <= EPI_1X1 and ("pack_scale" in on) == ("pack_shift" in on):
        table = fastpath.MFMA_1X1_SHAPES if L.nonneg else fastpath.MFMA_1X1_TERNARY_SHAPES
        if switch_says(x1, (L.C, L.O, L.H, L.out_f32) in table, conv) and ask("bconv1x1_mfma4_supported"):
            return Form.F4_1X1, asked
    if Form.I8_3X3 in packs and not names:
        key = (L.C, L.O, L.H, L.stride, False)
        if switch_says(conv, key in fastpath.MFMA_CONV_SHAPES) and ask("bconv2d_mfma_supported"):
            fp4 = (Form.F4_3X3 in packs and switch_says(f4, key in fastpath.MFMA_F4_SHAPES)
                   and ask("bconv2d_mfma4_supported"))
            return (Form.F4_3X3 if fp4 else Form.I8_3X3), asked
    if (not L.residual and Form.I8_3X3 in packs and L.shortcut_w8 and names == {"shortcut"} and L.out_f32 and L.out_packed
            and not L.prelu and L.k == 3):          # (no bias, no post-scale, a BatchNorm and ReLU: every layer here)
        key = (L.C, L.O, L.H, L.shortcut[0])
        if switch_says(fold_, key in fastpath.MFMA_FOLD_SHAPES, conv) and ask("bconv2d_mfma_fold_supported"):
            fp4 = (Form.F4_3X3 in packs and switch_says(f4, key in fastpath.MFMA_F4_SHAPES)
                   and ask("bconv2d_mfma4_fold_supported"))
            return (Form.F4_FOLD if fp4 else Form.I8_FOLD), asked
    return Form.POPCOUNT, asked


def record(L):
    """(the ``_Conv`` of the launch's layer, the arguments of ``route``)."""
    with torch.device("meta"):
        layer = BinaryConv2d(L.C, L.O, L.k, stride=L.stride, padding=L.k // 2, bias=False, bconfig=CFG)
    empty = torch.empty(0, dtype=torch.int32)
    weight = hipops.PackedWeight(empty, empty, T, False, (L.O, L.C, L.k, L.k))
    conv = _Conv(layer, fastpath.Plan(False, True, None), weight, T, T, relu=not L.prelu, prelu=T if L.prelu else None,
                 packs={form: T for form in packs_of(L)})
    epi = dict(L.epi)
    if L.shortcut is not None:
        sc_C, sc_H = L.shortcut
        sa = hipops.PackedAct(T, T, (N, sc_C, sc_H, sc_H), True)
        epi["shortcut"] = (sa, hipops.PackedWeight(empty, empty, T, False, (L.O, sc_C, 1, 1)), T, T)
    act = hipops.PackedAct(T, T, (N, L.C, L.H, L.H), L.nonneg)
    args = (act, T if L.residual else None, L.out_f32, L.out_packed, T if L.thr else None, epi,
            T if L.shortcut_w8 else None)
    return conv, args


RECORDS = [(L, *record(L)) for L in LAUNCHES]


@pytest.fixture
def queries(monkeypatch):
    """The five queries stubbed: ``calls`` lists (name, positional arguments, keywords) of each one asked; ``yes[name]``
    is its answer."""
    calls, yes = [], dict.fromkeys(QUERIES, True)
    for q in QUERIES:
        monkeypatch.setattr(hipops, q, lambda *a, _q=q, **kw: calls.append((_q, a, kw)) or yes[_q])
    return calls, yes


def check_description(L, call):
    """The query was handed this launch: its geometry, what its epilogue contains, and the form's own extras."""
    q, a, kw = call
    assert tuple(a[0]) == (N, L.C, L.H, L.H) and a[1].shape == (L.O, L.C, L.k, L.k)
    assert kw["nonneg"] == L.nonneg and kw["stride"] == (L.stride, L.stride) and kw["padding"] == (L.k // 2, L.k // 2)
    if "fold" in q:
        sc_C, sc_H = L.shortcut
        assert a[2] == sc_C and kw["unpooled_hw"] == (None if sc_H == L.H else (sc_H, sc_H)) and kw["throughput"] is False
        return
    want = dict(bias=False, post_scale=False, bn=True, residual=L.residual, prelu=L.prelu, relu=not L.prelu,
                out_f32=L.out_f32, out_packed=L.out_packed, sign_thresholds=L.thr)
    assert {k: kw[k] for k in want} == want
    if q == "bconv1x1_mfma4_supported":
        on = {n for n, v in L.epi if v is not None and v is not False}
        flags = (native.EPI_RES_AFTER_ACT if "residual_after_act" in on else 0) | \
            (native.EPI_PACK_BEFORE_RES if "pack_before_residual" in on else 0) | \
            (native.EPI_PACK_RELU if "pack_relu" in on else 0)
        assert kw["epi_flags"] == flags and kw["pack_affine"] == ("pack_scale" in on)
    else:
        assert "epi_flags" not in kw and "pack_affine" not in kw


def sweep(monkeypatch, queries, refused):
    calls, yes = queries
    for q in QUERIES:
        yes[q] = q != refused
    for sw in itertools.product(("0", "1", "all"), repeat=4):
        for name, value in zip(SWITCHES, sw):
            monkeypatch.setattr(fastpath, name, value)
        for L, conv, args in RECORDS:
            conv.routes.clear()
            del calls[:]
            want, asked = oracle(sw, L, yes)
            assert conv.route(*args) is want, (sw, L, refused)
            assert [c[0] for c in calls] == asked, (sw, L, refused)       # nothing else, a missing pack's query included
            for c in calls:
                check_description(L, c)
            assert conv.route(*args) is want and len(calls) == len(asked)   # the second call asks nothing
            assert list(conv.routes.values()) == [want]


def test_every_switch_setting_every_launch_all_queries_yes(monkeypatch, queries):
    assert len({L.k for L in LAUNCHES}) == 2 and len(LAUNCHES) > 60
    sweep(monkeypatch, queries, refused=None)


@pytest.mark.parametrize("refused", QUERIES)
def test_every_switch_setting_every_launch_one_query_no(monkeypatch, queries, refused):
    sweep(monkeypatch, queries, refused)


@pytest.fixture
def defaults(monkeypatch):
    for name in SWITCHES:
        monkeypatch.setattr(fastpath, name, "1")


def test_the_route_key_names_what_it_holds(queries, defaults):
    L = fold(256, 256, 14, 128, sc_H=28)
    conv, args = record(L)
    conv.throughput = True
    conv.route(*args)
    (key,) = conv.routes
    assert key == RouteKey(shape=(N, 256, 14, 14), nonneg=True, residual=False, out_f32=True, out_packed=True, thr=False,
                           epi=("shortcut",), epi_off=(), shortcut=(N, 128, 28, 28), shortcut_w8=True, throughput=True)
    conv, args = record(Launch(1, 512, 128, 28, epi=(("pack_shift", T), ("pack_relu", False), ("pack_scale", T))))
    conv.route(*args)
    (key,) = conv.routes
    assert key.epi == ("pack_scale", "pack_shift") and key.epi_off == ("pack_relu",) and key.shortcut is None
    # a key that is present but off and no key at all are two launches: only the second may leave the popcount kernels
    conv, args = record(Launch(3, 256, 256, 14))
    off = args[:5] + ({"pack_relu": False},) + args[6:]
    assert conv.route(*off) is Form.POPCOUNT and conv.route(*args) is Form.F4_3X3 and len(conv.routes) == 2


def test_the_default_switches(queries, defaults):
    def forms(ls):
        return {record(L)[0].route(*record(L)[1]) for L in ls}

    assert len(fastpath.MFMA_F4_SHAPES) == 8           # ResNet-18's eleven launches: three dense keys hold two each
    for key in fastpath.MFMA_F4_SHAPES:
        assert forms(dense(*key[:4])) == {Form.F4_3X3} if len(key) == 5 else forms([fold(*key)]) == {Form.F4_FOLD}
    assert forms(dense(64, 64, 56, 1) + dense(64, 128, 56, 2)) == {Form.POPCOUNT}
    assert forms(one(*key, nonneg=True) for key in fastpath.MFMA_1X1_SHAPES) == {Form.F4_1X1}
    assert forms(one(*key, nonneg=False) for key in fastpath.MFMA_1X1_TERNARY_SHAPES) == {Form.F4_1X1}


def test_which_packs_are_worth_building(monkeypatch):
    for sw in itertools.product(("0", "1", "all"), repeat=4):
        for name, value in zip(SWITCHES, sw):
            monkeypatch.setattr(fastpath, name, value)
        conv, fold_, f4, x1 = (s != "0" for s in sw)
        want = {Form.I8_3X3: conv, Form.F4_3X3: conv and f4, Form.I8_FOLD: conv and fold_, Form.F4_1X1: conv and x1}
        assert fastpath.mfma_packs() == {form for form, on in want.items() if on}, sw

"""The batch and row loops of bnn_amd.hipops that no other test forces to cut: each wrapper with its family's limit
patched so that 3 images go as 2 + 1 (5 rows as 2 + 2 + 1), bit for bit against the unpatched single launch.  (bconv2d,
bconv2d_fused, bconv2d_direct, stem3x3_bn_relu_pack, stem_s2x2 and gconv3x3s2_bn_pack are cut by their own tests.)"""
import numpy as np
import pytest
import torch

from bnn_amd import hipops, native
from tests.golden import gen
from tests.golden.fconv_cases import FACTORIZED

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def whole_and_cut(monkeypatch, limit, value, call, pieces):
    """``call()`` as it is and with ``hipops.<limit> = value``; the second must take ``pieces`` times the launches."""
    before = native.launch_count()
    whole = call()
    one = native.launch_count() - before
    with monkeypatch.context() as m:
        m.setattr(hipops, limit, value)
        before = native.launch_count()
        cut = call()
        assert one >= 1 and native.launch_count() - before == pieces * one
    return whole, cut


def same(a, b):
    if isinstance(a, torch.Tensor):
        return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, hipops.PackedAct):
        return a.shape == b.shape and a.nonneg == b.nonneg and same(a.P, b.P) and same(a.M, b.M)
    if isinstance(a, hipops.SavedAct):
        return a.shape == b.shape and same(a.sign, b.sign) and same(a.T, b.T)
    return a is None and b is None


# ---- the grouped trio: N = 3, C = 8, 5 x 7, 3 x 3 / stride 1 / padding 1 -------------------------------------------
N, C, O, H, W = 3, 8, 8, 5, 7


@pytest.fixture(scope="module", params=[2, C], ids=["groups2", "depthwise"])
def grouped(request):
    groups = request.param
    seed = gen.seed_of("split-grouped", groups)
    planes = hipops.pack_act(dev(gen.activation("sparse", seed, (N, C, H, W))))
    pw = hipops.pack_weight_grouped(dev(gen.conv_weight("kaiming", seed + 1, (O, C // groups, 3, 3))), groups)
    vec = lambda k: dev(0.5 + gen.uniform(seed + k, (O,)))                                                 # noqa: E731
    return dict(planes=planes, pw=pw, bias=vec(2), post_scale=vec(3), prelu=vec(4) - 0.75,
                residual=dev(gen.normal(seed + 5, (N, O, H, W))), wide=dev(gen.normal(seed + 6, (N, 3 * O, H, W))))


def test_grouped(grouped, monkeypatch):
    g = grouped
    for raw in (False, True):
        kw = dict(raw_dot=True) if raw else dict(bias=g["bias"], post_scale=g["post_scale"])
        whole, cut = whole_and_cut(monkeypatch, "_MAX_ELEMS", 2 * O * H * W,
                                   lambda: hipops.bconv2d_grouped(g["planes"], g["pw"], padding=1, **kw), 2)
        assert same(whole, cut) and whole.dtype == (torch.int32 if raw else torch.float32)


def test_grouped_fused(grouped, monkeypatch):
    g = grouped
    whole, cut = whole_and_cut(
        monkeypatch, "_MAX_ELEMS", 2 * O * H * W,
        lambda: hipops.bconv2d_grouped_fused(g["planes"], g["pw"], g["bias"], g["post_scale"], padding=1, prelu=g["prelu"],
                                             shuffle_groups=2, residual=g["residual"]), 2)
    assert same(whole, cut)


def test_grouped_node_writing_a_channel_slice(grouped, monkeypatch):
    g = grouped

    def call():
        wide = g["wide"].clone()                        # addend: channels [0, O), out: channels [O, 2 O) of ONE tensor
        out = hipops.bconv2d_grouped_node(g["planes"], g["pw"], g["bias"], g["post_scale"], padding=1, prelu=g["prelu"],
                                          shuffle_groups=4, residual=g["residual"], addend=wide[:, :O], out=wide[:, O:2 * O])
        assert out.data_ptr() == wide[:, O:2 * O].data_ptr()
        return wide
    whole, cut = whole_and_cut(monkeypatch, "_MAX_ELEMS", 2 * 3 * O * H * W, call, 2)      # (the wide tensor sets the step)
    assert same(whole, cut)
    assert torch.equal(whole[:, :O], g["wide"][:, :O]) and torch.equal(whole[:, 2 * O:], g["wide"][:, 2 * O:])
    assert not torch.equal(whole[:, O:2 * O], g["wide"][:, O:2 * O])


# ---- FactorizedConv in one launch ------------------------------------------------------------------------------------
def test_fconv_fused(monkeypatch):
    c = min(FACTORIZED, key=lambda c: c.C * c.H * c.W)                  # the smallest of tests/test_gpu_fconv.py
    Cf, K, s, Hf, Wf = c.C, 7, c.stride, c.H, c.W
    assert hipops.fconv_supported(3, Cf, Hf, Wf, K, s)
    seed = gen.seed_of("split-fconv", c.name)
    planes = hipops.pack_act(dev(gen.activation("sparse", seed, (3, Cf, Hf, Wf))))
    p1 = hipops.pack_weight(dev(gen.conv_weight("kaiming", seed + 1, (Cf, Cf, 1, K))))
    p2 = hipops.pack_weight(dev(gen.conv_weight("withzeros", seed + 2, (Cf, Cf, K, 1))))
    vec = lambda k: dev(0.5 + gen.uniform(seed + k, (Cf,)))                                                # noqa: E731
    ho, wo = (Hf - 1) // s + 1, (Wf - 1) // s + 1
    res = dev(gen.normal(seed + 9, (3, Cf, ho, wo)))
    per_image = max(Cf * ho * wo, 2 * Hf * Wf * ((Cf + 63) // 64))
    whole, cut = whole_and_cut(
        monkeypatch, "_MAX_ELEMS", 2 * per_image,
        lambda: hipops.fconv_fused(planes, p1, p2, vec(3), vec(4) - 1.0, stride=s, bias1=vec(5), prelu1=vec(6) - 0.75,
                                   post_scale2=vec(7), prelu2=vec(8) - 0.75, shuffle_groups=4, residual=res), 2)
    assert same(whole, cut)


# ---- the 7 x 7 stem: the smallest input of the stem tests, three images ---------------------------------------------
@pytest.fixture(scope="module")
def stem():
    seed = gen.seed_of("split-stem")
    return dict(x=dev(gen.normal(seed, (3, 3, 7, 9))), w=dev(gen.conv_weight("kaiming", 3, (64, 3, 7, 7))),
                a=dev(0.5 + gen.uniform(seed + 1, (64,))), b=dev(0.3 * gen.normal(seed + 2, (64,))))


@pytest.mark.parametrize("affine", [False, True], ids=["plain", "pack_affine"])
def test_stem7x7(stem, monkeypatch, affine):
    s = stem
    kw = dict(pack_affine=(s["a"] - 1.0, s["b"])) if affine else {}
    (y0, p0), (y1, p1) = whole_and_cut(monkeypatch, "_MAX_DESC_BYTES", 2 * 256 * 2 * 3,          # the output: [n, 64, 2, 3]
                                       lambda: hipops.stem7x7(s["x"], s["w"], s["a"], s["b"], **kw), 2)
    assert same(y0, y1) and same(p0, p1) and tuple(y0.shape) == (3, 64, 2, 3)


def test_stem7x7_conv(stem, monkeypatch):
    s = stem
    whole, cut = whole_and_cut(monkeypatch, "_MAX_DESC_BYTES", 2 * 256 * 4 * 5,                  # the output: [n, 64, 4, 5]
                               lambda: hipops.stem7x7_conv(s["x"], s["w"]), 2)
    assert same(whole, cut) and tuple(whole.shape) == (3, 64, 4, 5)


# ---- the Linear wrappers: M = 5 rows, F = 70, O = 9, two rows per launch ----------------------------------------------
M_, F_, O_ = 5, 70, 9
ROWS2 = 2 * F_                          # _LINEAR_MAX_ELEMS // max(F, O) == 2


@pytest.fixture(scope="module")
def lin():
    seed = gen.seed_of("split-linear")
    x = gen.normal(seed, (M_, F_)) * 0.8
    x[1, :7] = 0.0                                                      # exact zeros: ternary planes
    w = gen.conv_weight("kaiming", seed + 1, (O_, F_))
    d = dict(x=dev(x), w=dev(w), pw=hipops.pack_weight(dev(w)), g=dev(gen.normal(seed + 2, (M_, O_))),
             bias=dev(0.1 * gen.normal(seed + 3, (O_,))), post_scale=dev(0.5 + gen.uniform(seed + 4, (O_,))))
    d["saved"] = hipops.blinear_direct(d["x"], d["pw"], want_planes=True)[1]
    return d


def test_blinear_direct_with_planes(lin, monkeypatch):
    (o0, s0), (o1, s1) = whole_and_cut(
        monkeypatch, "_LINEAR_MAX_ELEMS", ROWS2,
        lambda: hipops.blinear_direct(lin["x"], lin["pw"], lin["bias"], lin["post_scale"], want_planes=True), 3)
    assert same(o0, o1) and same(s0, s1) and tuple(s0.shape) == (M_, F_, 1, 1)


def test_blinear_grad_input(lin, monkeypatch):
    whole, cut = whole_and_cut(monkeypatch, "_LINEAR_MAX_ELEMS", ROWS2,
                               lambda: hipops.blinear_grad_input(lin["g"], lin["saved"], lin["pw"]), 3)
    assert same(whole, cut) and tuple(whole.shape) == (M_, F_)


def test_blinear_grad_weight_slabs_per_launch(lin, monkeypatch):
    """The slab count depends on the cut (each launch splits its own rows), so the slabs of the cut call are compared
    with those of the same rows run on their own."""
    sv, g = lin["saved"], lin["g"]

    def rows(m0, m1):
        sign = hipops.PackedAct(sv.sign.P[m0:m1], sv.sign.M[m0:m1], (m1 - m0, F_, 1, 1))
        return hipops.blinear_grad_weight(g[m0:m1], hipops.SavedAct(sign, sv.T[m0:m1], (m1 - m0, F_, 1, 1)), reduce=False)
    want = torch.cat([rows(0, 2), rows(2, 4), rows(4, 5)], 0)
    with monkeypatch.context() as m:
        m.setattr(hipops, "_LINEAR_MAX_ELEMS", ROWS2)
        before = native.launch_count()
        got = hipops.blinear_grad_weight(g, sv, reduce=False)
        assert native.launch_count() - before == 3
        total = hipops.blinear_grad_weight(g, sv)
    assert same(got, want) and got.shape[1:] == (O_, F_)
    assert same(total, want.sum(0))
    with monkeypatch.context() as m:                    # a caller's own split is one launch whatever the limit says
        m.setattr(hipops, "_LINEAR_MAX_ELEMS", ROWS2)
        before = native.launch_count()
        one = hipops.blinear_grad_weight(g, sv, reduce=False, splits=1)
        assert native.launch_count() - before == 1 and tuple(one.shape) == (1, O_, F_)


def test_slinear_with_planes(lin, monkeypatch):
    packed = hipops.slinear_pack_weight(lin["w"])
    (o0, s0), (o1, s1) = whole_and_cut(
        monkeypatch, "_LINEAR_MAX_ELEMS", ROWS2,
        lambda: hipops.slinear(lin["x"], packed, lin["bias"], lin["post_scale"], want_planes=True), 3)
    assert same(o0, o1) and same(s0, s1)


def test_ste_mask_(lin, monkeypatch):
    gx = dev(gen.normal(gen.seed_of("split-ste"), (M_, F_)))

    def call():
        t = gx.clone()
        assert hipops.ste_mask_(t, lin["saved"]) is t
        return t
    whole, cut = whole_and_cut(monkeypatch, "_LINEAR_MAX_ELEMS", ROWS2, call, 3)
    assert same(whole, cut) and not torch.equal(whole, gx)

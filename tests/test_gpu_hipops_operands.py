"""The operand checks of bnn_amd.hipops in front of pointers that used to cross the C-ABI unchecked (the C side sees a
pointer, never a stride): a strided view of a tensor the kernel reads gives the bits of its ``.contiguous()`` copy; a
strided view of a tensor the kernel writes in place, or of an opaque buffer, is refused and left as it was; a wrong dtype
or a wrong size is refused.

Every bad operand here is one an unchecked launch would still read or write INSIDE its allocation — views start at the
front of a storage twice their size, wrong sizes are larger, wrong dtypes wider — so that a missing check fails the test
instead of faulting the device."""
import numpy as np
import pytest
import torch

from bnn_amd import hipops, native
from bnn_amd.native import NativeError
from tests import bn_ref
from tests.golden import gen

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WIDER = {torch.float32: torch.float64, torch.uint8: torch.int16, torch.int8: torch.int16}


def dev(a):
    a = np.asarray(a)
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32 if a.dtype == np.float64 else a.dtype)).to(DEV)


def strided(t, fill=3):
    """``(view, storage)``: ``t``'s values as every second element of a storage twice its size, from its front."""
    big = torch.full((*t.shape[:-1], 2 * t.shape[-1]), fill, dtype=t.dtype, device=t.device)
    big[..., ::2] = t
    view = big[..., ::2]
    assert not view.is_contiguous() and view.data_ptr() == big.data_ptr() and torch.equal(view, t)
    return view, big


def longer(t, extra=1):
    """``t`` with ``extra`` more entries along its last dimension (a per-channel vector of C + 1, a buffer with spare bytes)."""
    return torch.cat([t, torch.zeros((*t.shape[:-1], extra), dtype=t.dtype, device=t.device)], -1).contiguous()


def flat(out):
    """The tensors of a wrapper's result (nested tuples, SavedAct, PackedAct), in order."""
    if isinstance(out, (tuple, list)):
        return [t for o in out for t in flat(o)]
    if isinstance(out, hipops.SavedAct):
        return [out.sign.P, out.sign.M, out.T]
    if isinstance(out, hipops.PackedAct):
        return [out.P, out.M]
    return [] if out is None else [out]


def same(a, b):
    a, b = flat(a), flat(b)
    return len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype and
                                    torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))


def refused(call, args, name, bad, storage=None):
    """``call`` with ``args[name] = bad`` raises NativeError, launches nothing and leaves ``storage`` as it was."""
    keep = None if storage is None else storage.clone()
    before = native.launch_count()
    with pytest.raises(NativeError):
        call(**{**args, name: bad})
    torch.cuda.synchronize()
    assert native.launch_count() == before, name
    assert storage is None or torch.equal(storage.view(torch.uint8), keep.view(torch.uint8)), name


def check(call, args, read=(), written=(), opaque=(), sized=()):
    """``read``: strided -> the same bits; ``written`` / ``opaque``: strided -> refused; all of them: a wider dtype is
    refused; ``sized`` (and every opaque buffer): one entry (64 bytes) too many is refused."""
    want = call(**args)
    for name in read:
        assert same(call(**{**args, name: strided(args[name])[0]}), want), name
    for name in (*written, *opaque):
        refused(call, args, name, *strided(args[name]))
    for name in (*read, *written, *opaque):
        refused(call, args, name, args[name].to(WIDER[args[name].dtype]))
    for name in sized:
        refused(call, args, name, longer(args[name]))
    for name in opaque:
        refused(call, args, name, longer(args[name], 64))
    assert same(call(**args), want)                                 # and nothing above disturbed the operands


def test_a_contiguous_operand_comes_back_as_the_same_object():
    """No copy and no launch on the paths that run today."""
    t, v, b = dev(gen.normal(1, (2, 3, 4, 5))), dev(gen.normal(2, (3,))), torch.zeros(64, dtype=torch.int8, device=DEV)
    before = native.launch_count()
    assert hipops._nchw(t, "activation", "test") is t and hipops._shaped(t, (2, 3, 4, 5), "residual") is t
    assert hipops._written(v, 3, "running_mean") is v and hipops._written(t, (2, 3, 4, 5), "out") is t
    assert hipops._opaque(b, 64, "w8", torch.int8) is b
    assert hipops._per_channel(v, 3, "gamma").data_ptr() == v.data_ptr()
    assert hipops._shaped(None, (3,), "y") is None and hipops._written(None, 3, "running_var") is None
    assert native.launch_count() == before


def smallest(names, even=False):
    ok = [n for n in names if not even or (bn_ref.CASES[n][0][2] % 2 == 0 and bn_ref.CASES[n][0][3] % 2 == 0)]
    return min(ok, key=lambda n: int(np.prod(bn_ref.CASES[n][0])))


# ---- training BatchNorm ----------------------------------------------------------------------------------------------
BN, BN_EVEN, POOL = smallest(bn_ref.BN_CASES), smallest(bn_ref.BN_CASES, even=True), smallest(bn_ref.POOL_CASES)
MOM, EPS = bn_ref.MOMENTUM, bn_ref.EPS


def with_stats(fn):
    """A forward whose running statistics are cloned per call and returned with its results (a refused view is passed
    as it is: that is the operand under test)."""
    def call(rm, rv, **kw):
        rm, rv = (t.clone() if t.is_contiguous() and t.dtype == torch.float32 else t for t in (rm, rv))
        return (*fn(running_mean=rm, running_var=rv, momentum=MOM, eps=EPS, **kw), rm, rv)
    return call


def test_bn_train_forward():
    i = {k: dev(v) for k, v in bn_ref.bn_inputs(BN).items()}
    args = dict(x=i["x"], gamma=i["gamma"], beta=i["beta"], rm=i["rm"], rv=i["rv"], relu=True, residual=i["residual"])
    check(with_stats(hipops.bn_train_forward), args, read=("x", "residual", "gamma", "beta"), written=("rm", "rv"),
          sized=("gamma", "beta", "rm", "rv"))


def test_bn_relu_maxpool_train_forward():
    i = {k: dev(v) for k, v in bn_ref.pool_inputs(POOL).items()}
    args = dict(x=i["x"], gamma=i["gamma"], beta=i["beta"], rm=i["rm"], rv=i["rv"])
    check(with_stats(hipops.bn_relu_maxpool_train_forward), args, read=("x", "gamma", "beta"), written=("rm", "rv"),
          sized=("gamma", "beta", "rm", "rv"))


@pytest.mark.parametrize("fn, case", [(hipops.bn_train_pack_ste, BN), (hipops.bn_train_pack_ste_s2, BN_EVEN)],
                         ids=["pack_ste", "pack_ste_s2"])
def test_bn_train_pack_ste_refuses_a_view_of_the_running_statistics(fn, case):
    i = {k: dev(v) for k, v in bn_ref.bn_inputs(case).items()}
    args = dict(x=i["x"], gamma=i["gamma"], beta=i["beta"], rm=i["rm"], rv=i["rv"])
    check(with_stats(fn), args, read=("x", "gamma", "beta"), written=("rm", "rv"), sized=("gamma", "rm", "rv"))


def test_bn_train_backward():
    i = {k: dev(v) for k, v in bn_ref.backward_inputs(BN).items()}
    args = {k: i[k] for k in ("gy", "y", "x", "mean", "invstd", "gamma")}
    check(lambda **kw: hipops.bn_train_backward(want_dres=True, **kw), args, read=tuple(args),
          sized=("mean", "invstd", "gamma"))
    args["y"] = None
    assert len(flat(hipops.bn_train_backward(**args))) == 3


def test_bn_train_backward_add():
    i = {k: dev(v) for k, v in bn_ref.backward_inputs(BN).items()}
    args = {k: i[k] for k in ("gy", "x", "mean", "invstd", "gamma", "addend")}
    check(hipops.bn_train_backward_add, args, read=tuple(args), sized=("mean", "invstd", "gamma"))


def test_bn_train_backward_s2():
    i = {k: dev(v) for k, v in bn_ref.backward_inputs(BN_EVEN).items()}
    args = dict(g0=i["gy"][:, :, ::2, ::2].contiguous(), g1=i["gy"][:, :, 1::2, 1::2].contiguous(), x=i["x"],
                mean=i["mean"], invstd=i["invstd"], gamma=i["gamma"])
    check(hipops.bn_train_backward_s2, args, read=tuple(args), sized=("mean", "invstd", "gamma"))


def test_bn_relu_maxpool_train_backward():
    i = {k: dev(v) for k, v in bn_ref.pool_backward_inputs(POOL).items()}
    args = {k: i[k] for k in ("gy", "p", "code", "x", "mean", "invstd", "gamma")}
    check(hipops.bn_relu_maxpool_train_backward, args, read=tuple(args), sized=("mean", "invstd", "gamma"))


# ---- opaque buffers --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("saved", [False, True], ids=["fp32_input", "saved_planes"])
def test_bconv_grad_input(saved):
    seed = gen.seed_of("operands-dgrad")
    x = dev(gen.normal(seed, (2, 8, 5, 5)))
    packed, alpha = hipops.grad_pack_weight(dev(gen.conv_weight("kaiming", seed + 1, (8, 8, 3, 3))))
    args = dict(g=dev(gen.normal(seed + 2, (2, 8, 5, 5))), x=hipops.pack_act_ste(x) if saved else x, packed=packed,
                alpha=alpha)
    check(lambda g, x, packed, alpha: hipops.bconv_grad_input(g, x, packed, alpha, 3, 1), args, read=("g", "alpha"),
          opaque=("packed",), sized=("alpha",))


@pytest.fixture(scope="module")
def conv64():
    seed = gen.seed_of("operands-mfma")
    act = hipops.pack_act(dev(gen.activation("relu", seed, (2, 64, 7, 7))))
    act.nonneg = True
    pw = hipops.pack_weight(dev(gen.conv_weight("kaiming", seed + 1, (64, 64, 3, 3))))
    a, b = dev((0.5 + gen.uniform(seed + 2, (64,))).astype(np.float32)), dev(0.3 * gen.normal(seed + 3, (64,)))
    return act, pw, dict(bn_scale=a, bn_shift=b, relu=True, out_f32=True, out_packed=True, padding=1)


def test_w8_of_the_int8_matrix_core_convolution(conv64):
    act, pw, kw = conv64
    assert hipops.bconv2d_mfma_supported(act.shape, pw, nonneg=True, bn=True, relu=True, out_packed=True, padding=1)
    check(lambda w8: hipops.bconv2d_mfma_fused(act, pw, w8, **kw), dict(w8=hipops.pack_weight_i8(pw)), opaque=("w8",))
    assert same(hipops.bconv2d_mfma_fused(act, pw, hipops.pack_weight_i8(pw), **kw), hipops.bconv2d_fused(act, pw, **kw))


def test_w8_and_sc_w8_of_the_folded_shortcut():
    from tests.test_gpu_ds_fold_stream import _case
    c = _case(2, 64, 64, 7, 7)
    act2, pw2, pws = c["act2"], c["pw2"], c["pws"]
    kw = dict(shortcut=(c["pooled"], pws, *c["bns"]), bn_scale=c["bn2"][0], bn_shift=c["bn2"][1], relu=True, stride=1,
              padding=1, out_f32=True, out_packed=True)
    assert hipops.bconv2d_mfma_fold_supported(act2.shape, pw2, 64, nonneg=True)
    check(lambda w8, sc_w8: hipops.bconv2d_mfma_fold_fused(act2, pw2, w8, sc_w8, **kw),
          dict(w8=hipops.pack_weight_i8(pw2), sc_w8=hipops.pack_shortcut_weight_i8(pws)), opaque=("w8", "sc_w8"))


def test_sconv_weight_data():
    seed = gen.seed_of("operands-sconv")
    x, w = dev(gen.normal(seed, (2, 8, 5, 5))), dev(gen.conv_weight("kaiming", seed + 1, (8, 8, 3, 3)))
    pk = hipops.sconv_pack_weight(w)
    check(lambda data: hipops.sconv2d(x, hipops.SconvWeight(data, pk.shape)), dict(data=pk.data), opaque=("data",))
    x2, lw = dev(gen.normal(seed + 2, (5, 70))), hipops.slinear_pack_weight(dev(gen.conv_weight("kaiming", seed + 3, (9, 70))))
    check(lambda data: hipops.slinear(x2, hipops.SconvWeight(data, lw.shape), want_planes=True), dict(data=lw.data),
          opaque=("data",))


def test_ste_mask_refuses_a_view_and_leaves_it():
    saved = hipops.pack_act_ste(dev(gen.normal(7, (5, 70, 1, 1))))
    gx = dev(gen.normal(8, (5, 70)))
    check(lambda gx: hipops.ste_mask_(gx.clone() if gx.is_contiguous() and gx.dtype == torch.float32 else gx, saved),
          dict(gx=gx), written=("gx",))

"""The 7x7 stem (csrc/stem_rows.hip, csrc/stem.hip, csrc/stem_wgrad.hip) against the float64 oracle of tests/stem_ref.py at
the shapes of its CASES table: every entry point into pre-dirtied buffers with poisoned guard regions on both sides;
bit for bit on the exact grid and its planted patterns in all three arithmetics; within the per-element bound on
real-valued images with every per-channel weight scale 2^0 .. 2^-20 in one tensor; at both ends of the admitted image
scale; the same bits whatever the batch around an image and wherever the tensor starts in its storage."""
import numpy as np
import pytest
import torch

from bnn_amd import hipops, native
from tests import stem_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = np.float32, np.float64
ARITH = {"f16x3": {}, "fp16": dict(fp16=True), "exact_fp32": dict(exact_fp32=True)}
GUARD = 64                                # elements of poison on either side of every output
POISON = {torch.float32: 0x7FC0DEAD, torch.int64: 0x5A5AA5A55A5AA5A5}    # (a NaN payload; a pattern no plane has)
_RAW = {torch.float32: torch.int32, torch.int64: torch.int64}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def dev_x(a, aligned=True):
    """The input on the device; `aligned=False`: as a view one float into its storage (an 8-byte aligned base + 4)."""
    t = dev(a)
    if aligned:
        return t
    buf = torch.empty(t.numel() + 2, dtype=torch.float32, device=DEV)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert buf.data_ptr() % 8 == 0 and v.data_ptr() % 8 == 4 and v.is_contiguous()
    return v


class Guarded:
    """An output tensor in the middle of a poisoned buffer, itself poisoned: every element must be written, and nothing
    around it."""

    def __init__(self, shape, dtype=torch.float32):
        n = int(np.prod(shape))
        self.raw = torch.empty(n + 2 * GUARD, dtype=_RAW[dtype], device=DEV)
        self.poison = POISON[dtype]
        self.t = self.raw[GUARD:GUARD + n].view(dtype).view(shape)
        self.n = n
        self.dirty()

    def dirty(self):
        self.raw.fill_(self.poison)
        return self.t

    def result(self):
        """The tensor as numpy, after checking the guards and that no poison is left inside."""
        r = self.raw.cpu().numpy()
        assert (r[:GUARD] == self.poison).all() and (r[GUARD + self.n:] == self.poison).all(), "a guard region was written"
        assert not (r[GUARD:GUARD + self.n] == self.poison).any(), "an output element was not written"
        return self.t.cpu().numpy().copy()


def u64(a):
    return a.view(np.uint64)


class Buffers:
    """The guarded outputs of one input shape, reused by every call on it."""

    def __init__(self, N, H, W):
        hc, wc = R.half(H), R.half(W)
        hp, wp = R.half(hc), R.half(wc)
        self.y = Guarded((N, 64, hp, wp))
        self.P, self.M = Guarded((N, 1, hp, wp), torch.int64), Guarded((N, 1, hp, wp), torch.int64)
        self.pk = hipops.PackedAct(self.P.t, self.M.t, (N, 64, hp, wp))
        self.conv = Guarded((N, 64, hc, wc))
        self.dw = Guarded((64, 3, 7, 7))

    def dirty(self):
        for g in (self.y, self.P, self.M, self.conv, self.dw):
            g.dirty()


def run_stem(buf, x, w, a, b, arith, pack_affine=None):
    """stem7x7 in one arithmetic: (y, P, M) of the call with both outputs, after checking that each output on its own
    gives the same bits (all into the reused, re-dirtied guarded buffers)."""
    kw = dict(ARITH[arith])
    if pack_affine is not None:
        kw["pack_affine"] = pack_affine
    buf.dirty()
    y_, pk_ = hipops.stem7x7(x, w, a, b, out=(buf.y.t, buf.pk), **kw)
    assert y_.data_ptr() == buf.y.t.data_ptr() and pk_ is buf.pk and pk_.nonneg
    y, P, M = buf.y.result(), u64(buf.P.result()), u64(buf.M.result())
    buf.dirty()
    hipops.stem7x7(x, w, a, b, out=(None, buf.pk), **kw)
    assert np.array_equal(u64(buf.P.result()), P) and np.array_equal(u64(buf.M.result()), M)
    if pack_affine is None:
        buf.dirty()
        hipops.stem7x7(x, w, a, b, out=(buf.y.t, None), **kw)
        assert np.array_equal(buf.y.result().view(np.uint32), y.view(np.uint32))
        y2, pk2 = hipops.stem7x7(x, w, a, b, **kw)                      # and into tensors of its own
        assert np.array_equal(y2.cpu().numpy().view(np.uint32), y.view(np.uint32))
        assert np.array_equal(u64(pk2.P.cpu().numpy()), P) and np.array_equal(u64(pk2.M.cpu().numpy()), M)
    return y, P, M


def run_conv(buf, x, w, fp16):
    """stem7x7_conv: the C entry point into the guarded buffer, and the wrapper with the same bits."""
    lib = native.require()
    N, _, H, W = x.shape
    buf.conv.dirty()
    native.check(lib.bnn_hip_stem7x7_conv_f32(x.data_ptr(), w.data_ptr(), N, H, W, native.STEM_FP16 if fp16 else 0,
                                              buf.conv.t.data_ptr(), torch.cuda.current_stream().cuda_stream), "conv")
    c = buf.conv.result()
    c2 = hipops.stem7x7_conv(x, w, fp16=fp16).cpu().numpy()
    assert np.array_equal(c2.view(np.uint32), c.view(np.uint32))
    return c


def run_wgrad(buf, x, dy):
    lib = native.require()
    N, _, H, W = x.shape
    need = lib.bnn_hip_stem7x7_wgrad_workspace_bytes(N, H, W)
    assert need > 0 and need % 4 == 0
    work = Guarded((need // 4,))
    buf.dw.dirty()
    native.check(lib.bnn_hip_stem7x7_wgrad_f32(x.data_ptr(), dy.data_ptr(), N, H, W, work.t.data_ptr(), need,
                                               buf.dw.t.data_ptr(), torch.cuda.current_stream().cuda_stream), "wgrad")
    dw = buf.dw.result()
    work.result()
    assert np.array_equal(hipops.stem7x7_wgrad(x, dy).cpu().numpy().view(np.uint32), dw.view(np.uint32))
    return dw


def split_for(name, monkeypatch, N, H, W):
    """The batch_split case: the descriptor limit patched so that its three images go in more than one launch."""
    if name != "batch_split":
        return
    hp, wp = R.half(R.half(H)), R.half(R.half(W))
    monkeypatch.setattr(hipops, "_MAX_DESC_BYTES", 2 * max(12 * H * W, 256 * hp * wp))
    before = native.launch_count()
    hipops.stem7x7(torch.zeros((N, 3, H, W), device=DEV), torch.zeros((64, 3, 7, 7), device=DEV),
                   torch.ones(64, device=DEV), torch.zeros(64, device=DEV))
    assert native.launch_count() - before == 2 and N == 3


# ---------------------------------------------------------------------------------------------------- the exact grid
def grid_case(name):
    """(inputs on the unique images, image index of the batch, aligned) of a grid input: a case of the table or a pattern."""
    seed = R.gen.seed_of("stem-edges-grid", name)
    if name in R.CASES:
        (N, H, W), aligned, unique, _ = R.CASES[name]
        t = R.exact_grid((unique or N, H, W), seed)
        return t, R.batch_index(name), aligned
    t = {"pixel_walk": lambda: R.pattern_pixel_walk(seed), "pool_positions": R.pattern_pool_positions,
         "zero_image": lambda: R.pattern_zero_image(seed), "single_weight0": lambda: R.pattern_single_weight(seed, 0),
         "single_weight1": lambda: R.pattern_single_weight(seed, 1),
         "single_weight2": lambda: R.pattern_single_weight(seed, 2)}[name]()
    return t, np.arange(t[0].shape[0]), True


PATTERNS = ["pixel_walk", "pool_positions", "zero_image", "single_weight0", "single_weight1", "single_weight2"]


@pytest.mark.parametrize("name", list(R.CASES) + PATTERNS)
def test_exact_grid_bit_for_bit(name, monkeypatch):
    """Inputs on which every arithmetic is exact: the fp32 outputs, both sign planes, the planes behind pack_affine, the
    raw convolution and dw equal the float64 reference in all three arithmetics.  (Compared by value, so a -0.0 of the
    kernel equals the reference's +0.0; its plane bit is then clear because the planes equal the reference's.)"""
    (x, w, a, b, pa, pb), idx, aligned = grid_case(name)
    N, (_, _, H, W) = len(idx), x.shape
    split_for(name, monkeypatch, N, H, W)
    p_ref, (P_ref, M_ref) = R.stem_ref(x, w, a, b)
    Pa_ref, Ma_ref = R.affine_planes_ref(p_ref, pa, pb)
    c_ref = R.conv_ref(x, w)
    assert not M_ref.any() and not Ma_ref.any() and Pa_ref.any() and np.array_equal(p_ref.astype(F32).astype(F64), p_ref)
    count = N // x.shape[0]
    dy = R.grid_dy((N, H, W), R.gen.seed_of("stem-edges-grid", name))[:x.shape[0]]
    dw_ref = count * R.wgrad_ref(x, dy)
    assert np.abs(dw_ref).max() < 2 ** 24
    xd, wd, ad, bd, pad_, pbd = dev_x(x[idx], aligned), dev(w), dev(a), dev(b), dev(pa), dev(pb)
    buf = Buffers(N, H, W)
    for arith in ARITH:
        y, P, M = run_stem(buf, xd, wd, ad, bd, arith)
        assert np.array_equal(y.astype(F64), p_ref[idx]), arith
        assert np.array_equal(P, P_ref[idx]) and not M.any(), arith
        if arith != "exact_fp32":
            y2, Pa, Ma = run_stem(buf, xd, wd, ad, bd, arith, pack_affine=(pad_, pbd))
            assert np.array_equal(y2.view(np.uint32), y.view(np.uint32)), arith
            assert np.array_equal(Pa, Pa_ref[idx]) and np.array_equal(Ma, Ma_ref[idx]), arith
            assert np.array_equal(run_conv(buf, xd, wd, arith == "fp16").astype(F64), c_ref[idx]), arith
    assert np.array_equal(run_wgrad(buf, xd, dev(dy[idx])).astype(F64), dw_ref)


# ---------------------------------------------------------------------------------------------------- real values
def worst(got, ref, bound):
    """max |got - ref| / bound (inf where the bound is 0 and the values differ)."""
    err = np.abs(got.astype(F64) - ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    return float(r.max())


def bits_differing(P, Q):
    return int(np.unpackbits((P ^ Q).view(np.uint8)).sum())


def plane_bits(P):
    """bool [N, 64, H, W] of a plane [N, 1, H, W]."""
    return ((P[:, 0, :, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).transpose(0, 3, 1, 2).astype(bool)


def check_real(name, kind, xscale, monkeypatch, report):
    x, w, a, b, pa, pb, dy = R.real_inputs(name, kind, xscale)
    (N, H, W), aligned, unique, _ = R.CASES[name]
    idx = R.batch_index(name)
    split_for(name, monkeypatch, N, H, W)
    p_ref, (P_ref, _) = R.stem_ref(x, w, a, b)
    c_ref = R.conv_ref(x, w)
    aff_ref = p_ref * pa.astype(F64).reshape(1, -1, 1, 1) + pb.astype(F64).reshape(1, -1, 1, 1)
    Pa_ref, Ma_ref = R.affine_planes_ref(p_ref, pa, pb)
    xd, wd, ad, bd, pad_, pbd = dev_x(x[idx], aligned), dev(w), dev(a), dev(b), dev(pa), dev(pb)
    buf = Buffers(N, H, W)
    cap = max(1, p_ref[idx].size // 1000)
    failures = []
    for arith in ARITH:
        cb = R.bound_fp16 if arith == "fp16" else R.bound_fp32
        pooled_b = R.bound_pooled(x, w, a, b, cb)
        y, P, M = run_stem(buf, xd, wd, ad, bd, arith)
        r = worst(y, p_ref[idx], pooled_b[idx])
        report(f"{name} {kind} 2^{xscale} {arith}: pooled err/bound {r:.4g}")
        if not r <= 1.0:
            failures.append((arith, "pooled", r))
        Pk, Mk = R.oracle.pack_act(y)                                   # the planes are those of the kernel's own output
        assert np.array_equal(P, Pk) and np.array_equal(M, Mk) and not M.any(), arith
        diff = plane_bits(P ^ P_ref[idx])                               # and differ from the reference's only at a knife edge
        if not ((np.abs(p_ref[idx])[diff] <= pooled_b[idx][diff]).all() and diff.sum() <= cap):
            failures.append((arith, "signs", int(diff.sum())))
        if arith == "exact_fp32":
            continue
        y2, Pa, Ma = run_stem(buf, xd, wd, ad, bd, arith, pack_affine=(pad_, pbd))
        assert np.array_equal(y2.view(np.uint32), y.view(np.uint32)), arith
        own = R.affine_planes_ref(y, pa, pb)                            # (one fma: the sign of the exact value)
        assert np.array_equal(Pa, own[0]) and np.array_equal(Ma, own[1]), arith
        aff_b = R.bound_affine(x, w, a, b, pa, pb, cb)
        diff = plane_bits(Pa ^ Pa_ref[idx])
        if not ((np.abs(aff_ref[idx])[diff] <= aff_b[idx][diff]).all() and diff.sum() <= cap and not Ma.any()):
            failures.append((arith, "affine signs", int(diff.sum())))
        r = worst(run_conv(buf, xd, wd, arith == "fp16"), c_ref[idx], cb(x, w)[idx])
        report(f"{name} {kind} 2^{xscale} {arith}: conv err/bound {r:.4g}")
        if not r <= 1.0:
            failures.append((arith, "conv", r))
    count = N // x.shape[0]
    r = worst(run_wgrad(buf, xd, dev(dy[idx])), count * R.wgrad_ref(x, dy), count * count * R.bound_wgrad(x, dy))
    report(f"{name} {kind} 2^{xscale} wgrad: err/bound {r:.4g}")
    if not r <= 1.0:
        failures.append(("wgrad", "dw", r))
    assert not failures, failures


@pytest.fixture
def report(capsys):
    def say(line):
        with capsys.disabled():
            print("\n[stem-edges] " + line, end="")
    return say


@pytest.mark.parametrize("kind", ["normal", "uniform", "constant"])
@pytest.mark.parametrize("name", list(R.CASES))
def test_real_values_within_the_bound(name, kind, monkeypatch, report):
    """Normal, uniform [0, 1] and constant images, Kaiming weights with channel o scaled by 2^-(o % 21), bn_a of either
    sign: f16x3, exact_fp32 and the weight gradient within the per-element fp32 bound of the float64 reference, fp16
    within the bound with 2^-11; planes exactly those of the kernel's own output, differing from the reference's only
    where the reference is within its bound of zero, on at most 0.1 % of the elements."""
    check_real(name, kind, 0, monkeypatch, report)


@pytest.mark.parametrize("kind,xscale", [("normal", R.X_SCALES[0]), ("uniform", R.X_SCALES[1])])
def test_both_ends_of_the_admitted_image_scale(kind, xscale, monkeypatch, report):
    check_real("hp5_wp13", kind, xscale, monkeypatch, report)


# ---------------------------------------------------------------------------------------------------- invariances
def all_outputs(x, w, a, b, pa, pb, arith):
    kw = ARITH[arith]
    y, pk = hipops.stem7x7(x, w, a, b, **kw)
    out = [y, pk.P, pk.M]
    if arith != "exact_fp32":
        _, pa_ = hipops.stem7x7(x, w, a, b, pack_affine=(pa, pb), **kw)
        out += [pa_.P, pa_.M, hipops.stem7x7_conv(x, w, fp16=arith == "fp16")]
    return out


@pytest.mark.parametrize("name", ["hp5_wp15", "chunks", "round_robin"])
def test_an_image_does_not_depend_on_its_batch(name):
    """Image j of a batch and the same image alone (another tile list, another position): the same bits."""
    x, w, a, b, pa, pb, _ = R.real_inputs(name, "normal")
    idx = R.batch_index(name)
    xb = dev(x[idx])
    rest = [dev(v) for v in (w, a, b, pa, pb)]
    picks = sorted({0, len(idx) // 2, len(idx) - 1})
    for arith in ARITH:
        whole = all_outputs(xb, *rest, arith)
        for j in picks:
            alone = all_outputs(xb[j:j + 1].clone(), *rest, arith)
            assert all(torch.equal(t[j:j + 1], s) for t, s in zip(whole, alone)), (arith, j)
        pair = all_outputs(torch.cat([xb[picks[-1]:picks[-1] + 1], xb[:1]]), *rest, arith)      # another position
        assert all(torch.equal(t[0], s[picks[-1]]) and torch.equal(t[1], s[0]) for t, s in zip(pair, whole)), arith


def test_a_view_one_float_into_its_storage_gives_the_same_bits():
    """The same tensor 8-byte aligned (column pairs as one load) and at an aligned base + 4 (the scalar form)."""
    x, w, a, b, pa, pb, dy = R.real_inputs("misaligned", "normal")
    rest = [dev(v) for v in (w, a, b, pa, pb)]
    x0, x1 = dev_x(x), dev_x(x, aligned=False)
    assert x0.data_ptr() % 8 == 0
    for arith in ARITH:
        assert all(torch.equal(s, t) for s, t in zip(all_outputs(x0, *rest, arith), all_outputs(x1, *rest, arith))), arith
    assert torch.equal(hipops.stem7x7_wgrad(x0, dev(dy)), hipops.stem7x7_wgrad(x1, dev(dy)))


def test_the_tile_lists_of_the_table_are_the_ones_this_device_takes():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for name in ("chunks", "round_robin"):
        (N, H, W), aligned, _, why = R.CASES[name]
        assert set(why) <= R.paths(N, H, W, aligned, cus), (name, cus)

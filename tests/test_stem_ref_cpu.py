"""tests/stem_ref.py checked without a GPU: the references against torch in float64, the exact grid's properties, the
emulated arithmetics against the bound (and the accuracy loss of an unscaled fp16 split of small weights, which is why
the kernel rescales them), every mutant told apart on the input named for it, the case table complete."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import stem_ref as R

F64 = np.float64


def t64(a):
    return torch.from_numpy(np.asarray(a, F64))


@pytest.fixture(scope="module")
def small():
    return R.real_inputs("hp5_wp13", "normal")


def test_references_equal_torch_float64(small):
    x, w, a, b, pa, pb, dy = small
    conv = F.conv2d(t64(x), t64(w), None, 2, 3)
    assert np.allclose(R.conv_ref(x, w), conv.numpy(), rtol=1e-12, atol=1e-12 * float(conv.abs().max()))
    pre = conv * t64(a).view(1, -1, 1, 1) + t64(b).view(1, -1, 1, 1)
    ref = F.max_pool2d(F.relu(pre), 3, 2, 1).numpy()
    got, (P, M) = R.stem_ref(x, w, a, b)
    assert got.shape == ref.shape and np.allclose(got, ref, rtol=1e-12, atol=1e-12 * np.abs(ref).max())
    assert P.dtype == np.uint64 and P.shape == (x.shape[0], 1) + ref.shape[2:] and not M.any()
    bit = (P[:, 0, :, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)
    assert np.array_equal(bit.transpose(0, 3, 1, 2).astype(bool), got > 0)
    aff = got * pa.astype(F64).reshape(1, -1, 1, 1) + pb.astype(F64).reshape(1, -1, 1, 1)
    Pa, Ma = R.affine_planes_ref(got, pa, pb)
    bits = lambda Q: ((Q[:, 0, :, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).transpose(0, 3, 1, 2).astype(bool)  # noqa: E731
    assert np.array_equal(bits(Pa), aff > 0) and not Ma.any() and (aff < 0).any()
    wt = t64(w).requires_grad_(True)
    F.conv2d(t64(x), wt, None, 2, 3).backward(t64(dy))
    g = wt.grad.numpy()
    assert np.allclose(R.wgrad_ref(x, dy), g, rtol=1e-12, atol=1e-12 * np.abs(g).max())
    for shape in [(1, 1, 1), (2, 3, 24), (1, 7, 9)]:                   # the extents at the small end
        xs = R.exact_grid(shape, 1)[0]
        assert R.conv_ref(xs, w).shape == F.conv2d(t64(xs), t64(w), None, 2, 3).shape
        assert np.array_equal(R.conv_ref(xs, w), F.conv2d(t64(xs), t64(w), None, 2, 3).numpy())


def test_exact_grid_properties():
    x, w, a, b, pa, pb = R.exact_grid((3, 18, 27), 7)
    assert np.array_equal(x, np.round(x)) and np.abs(x).max() == 8 and x.min() == -8
    assert np.array_equal(w * 64, np.round(w * 64)) and np.abs(w).max() <= 1 and np.abs(w).max() > 0.9
    for v in (a, pa):
        assert set(np.abs(v)) == {0.5, 1.0, 2.0} and (v < 0).any() and (v > 0).any()
    for v in (b, pb):
        assert np.array_equal(v * 64, np.round(v * 64))
    for v in (x, w):                                                   # both operands are fp16 numbers: lo == 0
        assert np.array_equal(v.astype(np.float16).astype(np.float32), v)
    assert R.K * 8 * 1 < 2 ** 11                                       # 147 products of magnitude <= 8
    y = R.conv_ref(x, w)
    assert np.array_equal(y * 64, np.round(y * 64)) and np.abs(y).max() < 2 ** 11
    assert (R.weight_scale(w) == 1).all()                              # the grid is not rescaled either
    for arith in ("f16x3", "fp16", "fp32"):                            # every arithmetic is exact on it
        assert np.array_equal(R.emulate(x, w, arith).astype(F64), y), arith
        assert np.array_equal(R.emulate_stem(x, w, a, b, arith).astype(F64), R.stem_ref(x, w, a, b)[0]), arith
    p = R.stem_ref(x, w, a, b)[0]
    assert np.array_equal(p.astype(np.float32).astype(F64), p)
    assert not p[:, [5, 37, 11]].any() and (p > 0).mean() > 0.5        # the never-positive channels; the rest is alive
    aff = p * pa.astype(F64).reshape(1, -1, 1, 1) + pb.astype(F64).reshape(1, -1, 1, 1)
    assert np.array_equal(aff.astype(np.float32).astype(F64), aff) and (aff > 0).any() and (aff < 0).any()
    dy = R.grid_dy((3, 18, 27), 7)
    dw = R.wgrad_ref(x, dy)
    assert np.array_equal(dw, np.round(dw)) and np.abs(dw).max() < 2 ** 24 and np.abs(dy).max() == 4


def test_planted_patterns_cover_what_they_name():
    x, w, a, b, _, _ = R.pattern_pixel_walk(3)
    c = R.cols(x)
    for k in range(R.K):                                               # image k: tap k of output (3, 3), nothing else of it
        assert c[k, k, 3, 3] != 0 and np.count_nonzero(c[k, :, 3, 3]) == 1 and np.count_nonzero(x[k]) == 1
    taps = set()
    for j in range(3):
        wj = R.pattern_single_weight(3, j)[1].reshape(R.COUT, R.K)
        assert (np.count_nonzero(wj, axis=1) <= 1).all()
        taps |= set(np.nonzero(wj)[1])
    assert taps == set(range(R.K))
    x, w, a, b, pa, pb = R.pattern_pool_positions()
    y = R.conv_ref(x, w)
    assert np.array_equal(y[:, 0], x[:, 0, ::2, ::2].astype(F64)) and y.shape[2:] == (5, 7)   # both far borders cut windows
    p = R.stem_ref(x, w, a, b)[0]
    for d in range(9):                                                 # where the planted position exists, it is the maximum
        dy, dx = d // 3, d % 3
        for py in (0, 2):
            for px in (0, 3):
                i, j = 2 * py - 1 + dy, 2 * px - 1 + dx
                if 0 <= i < 5 and 0 <= j < 7:
                    win = y[d, 0, max(i - dy, 0):i - dy + 3, max(j - dx, 0):j - dx + 3]
                    assert p[d, 0, py, px] == 8 == y[d, 0, i, j] and (win == 8).sum() == 1
    x = R.pattern_zero_image(3)[0]
    assert not x[1].any() and x[0].any() and x[2].any()


def _ratio(got, ref, bound):
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(got.astype(F64) - ref) / bound
    return float(np.nanmax(np.where(bound > 0, r, np.where(got == ref, 0.0, np.inf))))


def test_emulations_against_the_bound(small):
    x, w0, a, b, _, _, _ = small
    w1 = R.real_inputs("hp5_wp13", "normal")[1]
    from tests.golden import gen
    kaiming = gen.conv_weight("kaiming", 3, (64, 3, 7, 7))
    ref, B = R.conv_ref(x, kaiming), R.bound_fp32(x, kaiming)
    assert _ratio(R.emulate(x, kaiming, "fp32"), ref, B) <= 1.0
    assert (R.weight_scale(kaiming) == 1).all()                        # the rule is the identity at this scale
    assert _ratio(R.emulate(x, kaiming, "f16x3", prescale=False), ref, B) <= 0.5
    small_w = (kaiming.astype(F64) * 2.0 ** -12).astype(np.float32)
    refs, Bs = R.conv_ref(x, small_w), R.bound_fp32(x, small_w)
    assert _ratio(R.emulate(x, small_w, "fp32"), refs, Bs) <= 1.0
    assert _ratio(R.emulate(x, small_w, "f16x3", prescale=False), refs, Bs) > 4.0     # the finding: an unscaled split
    assert _ratio(R.emulate(x, small_w, "f16x3"), refs, Bs) <= 0.5                    # ... and the rule that mends it
    refm, Bm = R.conv_ref(x, w1), R.bound_fp32(x, w1)                  # every scale 2^0 .. 2^-20 in one tensor
    assert _ratio(R.emulate(x, w1, "f16x3", prescale=False), refm, Bm) > 4.0
    assert _ratio(R.emulate(x, w1, "f16x3"), refm, Bm) <= 0.5
    assert _ratio(R.emulate(x, w1, "fp32"), refm, Bm) <= 1.0
    assert _ratio(R.emulate(x, w1, "fp16"), refm, R.bound_fp16(x, w1)) <= 0.5
    assert np.array_equal(w0, w1)


@pytest.mark.parametrize("kind,xscale", [("normal", R.X_SCALES[0]), ("uniform", R.X_SCALES[1])])
def test_the_admitted_image_scales_keep_the_emulation_within_half_the_bound(kind, xscale):
    x, w, a, b, _, _, _ = R.real_inputs("hp5_wp13", kind, xscale)
    assert np.abs(x).max() <= 2.0 ** 15
    assert _ratio(R.emulate(x, w, "f16x3"), R.conv_ref(x, w), R.bound_fp32(x, w)) <= 0.5
    assert _ratio(R.emulate_stem(x, w, a, b), R.stem_ref(x, w, a, b)[0], R.bound_pooled(x, w, a, b)) <= 0.5


def _bits_differing(P, Q):
    d = P ^ Q
    return int(sum(bin(int(v)).count("1") for v in d.ravel()))


@pytest.mark.parametrize("name", list(R.CASES))
@pytest.mark.parametrize("kind", ["normal", "uniform", "constant"])
def test_knife_edge_signs_of_the_chosen_seeds_stay_under_the_cap(name, kind):
    """The GPU test allows sign differences from the float64 reference on at most 0.1 % of a case's elements: the
    emulation itself stays within that on the inputs the test uses."""
    x, w, a, b, pa, pb, _ = R.real_inputs(name, kind)
    p, (P, M) = R.stem_ref(x, w, a, b)
    e = R.emulate_stem(x, w, a, b)
    cap = max(1, p.size // 1000)
    assert _bits_differing(R.planes_of(e.astype(F64))[0], P) <= cap
    Pa, Ma = R.affine_planes_ref(p, pa, pb)
    got = R.affine_planes_ref(e, pa, pb)
    assert _bits_differing(got[0], Pa) + _bits_differing(got[1], Ma) <= cap


def test_every_mutant_is_detected():
    """On the grid a mutant changes a bit; on real inputs it leaves the bound by more than a factor of four."""
    grids = [R.exact_grid((2, 18, 27), 11), R.pattern_pool_positions(), R.pattern_pixel_walk(11)]
    x, w, a, b, pa, pb, dy = R.real_inputs("hp5_wp13", "normal")
    for name, (fn, where) in R.MUTANTS.items():
        if where == "grid":
            assert any(not np.array_equal(fn(*g[:4]), R.stem_ref(*g[:4])[0]) for g in grids), name
            assert not np.array_equal(fn(*grids[0][:4]), R.stem_ref(*grids[0][:4])[0]) or name == "pool_edge", name
        else:
            assert _ratio(fn(x, w, a, b), R.stem_ref(x, w, a, b)[0], R.bound_pooled(x, w, a, b)) > 4.0, name
    assert not np.array_equal(R.MUTANTS["pool_edge"][0](*grids[1][:4]), R.stem_ref(*grids[1][:4])[0])
    for name, fn in R.EQUIVALENT.items():
        assert np.array_equal(fn(*grids[0][:4]), R.stem_ref(*grids[0][:4])[0]), name
    g = grids[0]
    Pm, Mm = R.mut_affine_unpooled(*g)
    Pr, Mr = R.affine_planes_ref(R.stem_ref(*g[:4])[0], g[4], g[5])
    assert not np.array_equal(Pm, Pr) or not np.array_equal(Mm, Mr)
    gdy = R.grid_dy((2, 18, 27), 11)
    for shift in [(1, 0), (0, 1)]:
        assert not np.array_equal(R.mut_wgrad_offset(g[0], gdy, shift), R.wgrad_ref(g[0], gdy))
        assert _ratio(R.mut_wgrad_offset(x, dy, shift), R.wgrad_ref(x, dy), R.bound_wgrad(x, dy)) > 4.0


def test_the_case_table_is_complete():
    assert R.check_cases()
    for name, ((N, H, W), aligned, unique, why) in R.CASES.items():
        assert unique is None or N % unique == 0
    assert R.paths(1, 40, 114) >= {"pair_interior", "pair_edge", "scalar_rows"}
    assert R.paths(1, 40, 114, aligned=False) & set(R.FETCH) == {"scalar_misaligned"}
    assert R.tile_list(600, 40, 10) == (512, 3, 2, 3, 1)               # 600 strips on 512 workgroups: a partial round
    assert R.tile_list(1, 100, 20) == (8, 1, 1, 7, 1)                  # seven one-tile chunks of one strip

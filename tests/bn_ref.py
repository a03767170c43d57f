"""numpy oracle of the training BatchNorm kernels and the stem tail (csrc/bn_train.hip): float64 references, a counted
per-element error bound for every floating-point output, fp32 emulations of the kernels' operation sequences with named
wrong variants (MUTANTS), the host-side rules (splits, which kernel form a launcher takes) restated once, and the one
table of cases (CASES) with the inputs that go with it.  No torch, no GPU.

The bounds.  u = 2^-24 is the relative error of one fp32 rounding to nearest; each bound is u times the magnitude of every
rounded intermediate of the sequence the header comments of bn_train.hip state, first order in u, plus an allowance for
the double-precision steps.  A contraction of a * b + c into one fma removes a rounding: covered.  What the functions
return is MARGIN = 2 times the counted sum: the emulations below (numpy's order of operations) must stay within the counted
sum itself, i.e. half the bound, and the other half is for the compiler's contractions and its order of the four-term
float4 sums, which move single roundings across a boundary but add none.

  double-precision steps.  A block sums <= ceil(units / 256) terms per thread (float4: four per step), then 6 + 2 tree
  levels, then <= 64 splits in order: `sum_depth` roundings of 2^-53 each, and CASES keeps sum_depth <= 2^8, so a sum of
  terms t_i is within 2^-45 * sum |t_i| (the products x * x and g * xhat of two fp32 numbers are exact in double).
  mean = a / count: within 2^-44 * E|x|.   var = b / count - mean^2: within 3 * 2^-45 * E[x^2] = 3 * 2^-45 * (var + mean^2),
  and CASES keeps mean^2 <= 2^20 * (var + eps), so var + eps is within 3 * 2^-25 relative and invstd = (var + eps)^-1/2
  within 1.5 * 2^-25 < u relative.  Allowed: u on invstd; A64 = 2^-40 times the summed magnitudes elsewhere (32 times what
  was counted: it is 2^-16 u and never decides a comparison).

  forward.  save_mean = fl(mean): u |mean| + A64 E|x|.   save_invstd = fl(invstd): (1 + 1) u |invstd|.
    scale = fl(gamma * invstd32): within 3 u of gamma * invstd.   shift = fl(beta - mean * scale) WITH THE ROUNDED scale,
    so x * scale + shift = (x - mean) * scale + beta + d, |d| <= u |shift| <= u (|beta| + |mean * scale|): the error of
    scale multiplies x * scale and mean * scale only.   pre = fl(fma(x, scale, shift)): u |pre|.   (+ residual: u |y|.)
      |y - y_ref| <= u * ( 3 (|x scale| + |mean scale|) + (|beta| + |mean scale|) + |pre| [+ |pre + residual|] )
    ReLU is 1-Lipschitz and exact.   running_mean = fl((1 - m) rm + m mean) in double with m the fp32 momentum:
    u |new| + A64 (|rm| + E|x|);   running_var likewise with the unbiased variance: u |new| + A64 (|rv| + m f E[x^2]),
    f = count / (count - 1) (1 when count == 1: the kernel keeps the biased value there).

  backward (inputs: the fp32 gy, y, x, mean, invstd, gamma the kernel takes; g = gy where y > 0, exact).
    xhat = fl(fl(x - mean) * invstd): 2 u |xhat|.   With G = sum |g|, T = sum |g xhat| over the channel, m = count:
    dbeta = fl(sum g): u |dbeta| + A64 G.   dgamma = fl(sum g xhat): u |dgamma| + (2 u + A64) T.
    k = fl(gamma invstd): u.   mb = fl(sb / m): u |mb| + A64 G / m.   kg = fl(invstd * fl(sg / m)): 2 u |kg| + 2 u invstd T / m.
    dx = fl(k * fl(fl(g - mb) - fl(fl(x - mean) * kg))) [+ addend]:
      |dx - dx_ref| <= u |k| ( |g - mb| + |mb| + |x - mean| (4 |kg| + 2 invstd T / m) + |t3| ) + 2 u |dx| [+ u |dx + addend|]
                       + A64 |k| (G / m + |x - mean| invstd T / m),            t3 = g - mb - (x - mean) kg
    dres = g: bit-equal.

  stem tail.  forward: an element is pre above without residual; p is a maximum of such elements, and |max a - max b| <=
    max |a - b|: the bound of p is the maximum of the window's element bounds.  backward: g[pixel] is an fp32 sum of the
    <= 4 window gradients that name it, in the kernel's order: (n - 1) u sum |gy_w| for n of them; the reductions run over
    the windows in double (no such term), then the dx bound above with g's own error added inside the bracket.
"""
import numpy as np

from tests.golden import gen

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
A64 = 2.0 ** -40
MARGIN = 2.0
TINY = 2.0 ** -149           # one subnormal step: results that underflow

# ---------------------------------------------------------------------------------------------------- host rules
NT, MAX_SPLITS, LDS_PLANE, LDS_PER = 256, 64, 16384, 16


def splits(N, C):
    """(splits, images per split) of bn_train_splits and the launchers' `per`."""
    s = max(1, min((1024 + C - 1) // C, MAX_SPLITS, N))
    per = (N + s - 1) // s
    S = (N + per - 1) // per
    return S, (N + S - 1) // S


def split_regimes(N, C):
    """Which of the four regimes of the split arithmetic (N, C) is in (more than one can hold)."""
    S, per = splits(N, C)
    out = set()
    if S == 1:
        out.add("single")
    if per == 1 and S > 1:
        out.add("per_image")
    if per > 1 and N % per:
        out.add("ragged")
    if (1024 + C - 1) // C > MAX_SPLITS and N > MAX_SPLITS:
        out.add("capped")
    return out


def sum_depth(N, C, HW, vec):
    """Roundings on the longest path of a channel's double sum (see the module docstring)."""
    S, per = splits(N, C)
    units = per * (HW // vec)
    return -(-units // NT) * vec + 8 + S


def half(n):
    return (n - 1) // 2 + 1


def bn_form(HW, aligned=True):
    """Units of the BatchNorm kernels (stats, apply, reduce, dx): float4 or float."""
    return 4 if HW % 4 == 0 and aligned else 1


def units_per_block(N, C, HW, aligned=True):
    """Work items one block of a statistics / reduction kernel walks."""
    return splits(N, C)[1] * (HW // bn_form(HW, aligned))


def pool_fwd_form(H, W, aligned=True):
    return "lds" if (H * W) % 4 == 0 and H * W <= LDS_PLANE and aligned else "gather"


def pool_bwd_form(H, W, aligned=True):
    """('lds',) or ('gather4' | 'gather1', lpr_shift, lane loop?)."""
    hw, hwp = H * W, half(H) * half(W)
    if hw % 4 == 0 and hw <= LDS_PLANE and aligned and hwp <= LDS_PER * NT:
        return ("lds",)
    v4 = W % 4 == 0 and aligned
    upr = W // 4 if v4 else W
    shift = 0
    while (1 << shift) < upr and shift < 6:
        shift += 1
    return ("gather4" if v4 else "gather1", shift, upr > 64)


# ---------------------------------------------------------------------------------------------------- references
def _stats64(x):
    x = np.asarray(x, F64)
    mean = x.mean(axis=(0, 2, 3))
    var = ((x - mean[None, :, None, None]) ** 2).mean(axis=(0, 2, 3))
    return mean, var, x.shape[0] * x.shape[2] * x.shape[3]


def _c(v):
    return np.asarray(v, F64)[None, :, None, None]


def _affine(gamma, beta, C):
    return (np.ones(C) if gamma is None else np.asarray(gamma, F64)), (np.zeros(C) if beta is None else np.asarray(beta, F64))


def _forward(x, gamma, beta, running_mean, running_var, momentum, eps, relu, residual):
    x64 = np.asarray(x, F64)
    C = x64.shape[1]
    g, b = _affine(gamma, beta, C)
    mean, var, count = _stats64(x64)
    eps, m = float(F32(eps)), float(F32(momentum))
    invstd = 1.0 / np.sqrt(var + eps)
    scale = g * invstd
    pre = (x64 - _c(mean)) * _c(scale) + _c(b)
    by = 3 * (np.abs(x64 * _c(scale)) + np.abs(_c(mean * scale))) + np.abs(_c(b)) + np.abs(_c(mean * scale)) + np.abs(pre)
    y = pre
    if residual is not None:
        y = pre + np.asarray(residual, F64)
        by = by + np.abs(y)
    if relu:
        y = np.where(y < 0, 0.0, y)          # keeps NaN
    ex, ex2 = np.abs(x64).mean(axis=(0, 2, 3)), (x64 * x64).mean(axis=(0, 2, 3))
    ref = {"y": y, "mean": mean, "invstd": invstd}
    bound = {"y": U * by + TINY, "mean": U * np.abs(mean) + A64 * ex + TINY, "invstd": 2 * U * invstd}
    if running_mean is not None:
        f = count / (count - 1.0) if count > 1 else 1.0
        rm, rv = np.asarray(running_mean, F64), np.asarray(running_var, F64)
        ref["rm"] = (1 - m) * rm + m * mean
        ref["rv"] = (1 - m) * rv + m * var * f
        bound["rm"] = U * np.abs(ref["rm"]) + A64 * (np.abs(rm) + ex) + TINY
        bound["rv"] = U * np.abs(ref["rv"]) + A64 * (np.abs(rv) + m * f * ex2) + TINY
    else:
        ref["rm"] = ref["rv"] = bound["rm"] = bound["rv"] = None
    ref["scale"], ref["shift"], ref["var"], ref["eps"] = scale, b - mean * scale, var, eps
    bound = {k: None if v is None else MARGIN * v for k, v in bound.items()}
    return ref, bound


KEYS = ("y", "mean", "invstd", "rm", "rv")


def forward_ref(x, gamma, beta, running_mean, running_var, momentum, eps, relu=False, residual=None):
    """float64 (y, save_mean, save_invstd, new running_mean, new running_var) of bn_train_forward: biased variance
    normalises, unbiased goes to running_var (count == 1: the biased value, as the kernel), momentum and eps as the fp32
    numbers the entry point takes."""
    ref, _ = _forward(x, gamma, beta, running_mean, running_var, momentum, eps, relu, residual)
    return tuple(ref[k] for k in KEYS)


def forward_bound(x, gamma, beta, running_mean, running_var, momentum, eps, relu=False, residual=None):
    """The per-element bounds of forward_ref's five results (module docstring)."""
    _, bound = _forward(x, gamma, beta, running_mean, running_var, momentum, eps, relu, residual)
    return tuple(bound[k] for k in KEYS)


def cancellation_ok(x, eps):
    """mean^2 <= 2^20 (var + eps) in every channel without a NaN: what the invstd allowance rests on."""
    mean, var, _ = _stats64(x)
    ok = mean * mean <= 2.0 ** 20 * (var + float(F32(eps)))
    return bool(np.all(ok | np.isnan(mean)))


def _backward(g, x, mean32, invstd32, gamma, addend, g_err=None, gabs=None):
    """The BatchNorm backward of the (already masked / routed) float64 gradient g, and its bounds.  `gabs`: the summed
    magnitudes behind every element of g where g is itself a sum (the stem tail); `g_err`: the error g arrives with."""
    x64 = np.asarray(x, F64)
    C = x64.shape[1]
    count = x64.shape[0] * x64.shape[2] * x64.shape[3]
    mu, is_ = np.asarray(mean32, F64), np.asarray(invstd32, F64)
    gam = np.ones(C) if gamma is None else np.asarray(gamma, F64)
    d = x64 - _c(mu)
    xhat = d * _c(is_)
    sb, sg = g.sum(axis=(0, 2, 3)), (g * xhat).sum(axis=(0, 2, 3))
    gabs = np.abs(g) if gabs is None else gabs
    G, T = gabs.sum(axis=(0, 2, 3)), (gabs * np.abs(xhat)).sum(axis=(0, 2, 3))
    k, mb, kg = gam * is_, sb / count, is_ * sg / count
    t3 = g - _c(mb) - d * _c(kg)
    dx = _c(k) * t3
    br = (np.abs(g - _c(mb)) + np.abs(_c(mb)) + np.abs(d) * _c(4 * np.abs(kg) + 2 * is_ * T / count) + np.abs(t3))
    if g_err is not None:
        br = br + g_err / U
    bdx = U * np.abs(_c(k)) * br + 2 * U * np.abs(dx) + A64 * np.abs(_c(k)) * (_c(G / count) + np.abs(d) * _c(is_ * T / count))
    if addend is not None:
        dx = dx + np.asarray(addend, F64)
        bdx = bdx + U * np.abs(dx)
    ref = {"dx": dx, "dgamma": sg, "dbeta": sb}
    bound = {"dx": MARGIN * (bdx + TINY), "dgamma": MARGIN * (U * np.abs(sg) + (2 * U + A64) * T + TINY),
             "dbeta": MARGIN * (U * np.abs(sb) + A64 * G + TINY)}
    return ref, bound


def _masked(gy, y):
    gy = np.asarray(gy, F32)
    return gy if y is None else np.where(np.asarray(y, F32) > 0, gy, F32(0))


def backward_ref(gy, y, x, mean32, invstd32, gamma, addend=None):
    """float64 (dx, dgamma, dbeta, dres) of bn_train_backward[_add] from the fp32 tensors the kernel takes: the ReLU mask
    is `y > 0` on those bits (y None: no ReLU), xhat = (x - mean32) * invstd32 in float64.  dres is the fp32 masked gy."""
    g = _masked(gy, y)
    ref, _ = _backward(g.astype(F64), x, mean32, invstd32, gamma, addend)
    return ref["dx"], ref["dgamma"], ref["dbeta"], g


def backward_bound(gy, y, x, mean32, invstd32, gamma, addend=None):
    """Bounds of backward_ref's (dx, dgamma, dbeta)."""
    _, b = _backward(_masked(gy, y).astype(F64), x, mean32, invstd32, gamma, addend)
    return b["dx"], b["dgamma"], b["dbeta"]


def _windows(v, fill):
    """[9, N, C, Hp, Wp]: position 3 * dy + dx of every 3x3 / stride 2 / pad 1 window of v, `fill` outside the image."""
    N, C, H, W = v.shape
    Hp, Wp = half(H), half(W)
    pv = np.full((N, C, 2 * Hp + 1, 2 * Wp + 1), fill, v.dtype)
    pv[:, :, 1:H + 1, 1:W + 1] = v
    return np.stack([pv[:, :, dy:dy + 2 * Hp:2, dx:dx + 2 * Wp:2] for dy in range(3) for dx in range(3)])


def _first_max(win, last=False):
    """(value, code) per window: the first maximum in raster order — the LAST NaN where there is one (`v > best || v != v`,
    torch's max_pool2d rule too).  `last`: the last maximum (a mutant)."""
    nan = np.isnan(win)
    w = np.where(nan, np.inf, win)
    code = 8 - np.argmax(w[::-1], axis=0) if last else np.argmax(w, axis=0)
    anyn = nan.any(axis=0)
    code = np.where(anyn, 8 - np.argmax(nan[::-1], axis=0), code)
    return np.take_along_axis(win, code[None], axis=0)[0], code.astype(np.uint8)


def pool_forward_ref(x, scale, shift):
    """float64 (p, code) of the stem tail's pooling pass: p = max over the window of relu(x * scale + shift), code =
    3 * dy + dx of the first maximum."""
    v = np.asarray(x, F64) * _c(scale) + _c(shift)
    v = np.where(v < 0, 0.0, v)
    return _first_max(_windows(v, -1.0))


def window_max(b):
    """The maximum of a per-element bound over each window (outside the image: 0)."""
    return _windows(np.asarray(b, F64), 0.0).max(axis=0)


def route(gy, p, code, shape, dtype=F64, mask_ge=False):
    """g[pixel] = sum of gy over the windows that name the pixel and have p > 0; also the sum of |gy| and the count."""
    N, C, H, W = shape
    Hp, Wp = half(H), half(W)
    p, code = np.asarray(p, F32), np.asarray(code).astype(np.int64)
    open_ = (p >= 0) if mask_ge else (p > 0)
    n, c, py, px = np.nonzero(open_)
    cd = code[n, c, py, px]
    r, q = 2 * py - 1 + cd // 3, 2 * px - 1 + cd % 3
    assert r.size == 0 or (r.min() >= 0 and r.max() < H and q.min() >= 0 and q.max() < W), "a code names no pixel"
    g, ga, cnt = np.zeros(shape, dtype), np.zeros(shape, F64), np.zeros(shape, np.int64)
    vals = np.asarray(gy, dtype)[n, c, py, px]
    np.add.at(g, (n, c, r, q), vals)
    np.add.at(ga, (n, c, r, q), np.abs(vals.astype(F64)))
    np.add.at(cnt, (n, c, r, q), 1)
    return g, ga, cnt


def pool_backward_ref(gy, p, code, x, mean32, invstd32, gamma):
    """float64 (dx, dgamma, dbeta) of bn_relu_maxpool_train_backward from the kernel's own fp32 p and uint8 code."""
    g, _, _ = route(gy, p, code, np.shape(x))
    ref, _ = _backward(g, x, mean32, invstd32, gamma, None)
    return ref["dx"], ref["dgamma"], ref["dbeta"]


def pool_backward_bound(gy, p, code, x, mean32, invstd32, gamma):
    g, ga, cnt = route(gy, p, code, np.shape(x))
    _, b = _backward(g, x, mean32, invstd32, gamma, None, g_err=U * np.maximum(cnt - 1, 0) * ga, gabs=ga)
    return b["dx"], b["dgamma"], b["dbeta"]


def avgpool2x2_backward_ref(gy):
    """fp32, exact: gx[..., 2y + a, 2x + b] = 0.25 * gy[..., y, x]."""
    g = F32(0.25) * np.asarray(gy, F32)
    return np.repeat(np.repeat(g, 2, axis=2), 2, axis=3)


# ---------------------------------------------------------------------------------------------------- emulations
MUTANTS = {
    "unbiased_var_normalises": "forward", "biased_running_var": "forward", "eps_after_sqrt": "forward",
    "momentum_wrong_term": "forward", "ragged_split_dropped": "forward", "channel_by_hw": "forward",
    "relu_mask_ge": "backward", "dres_unmasked": "backward", "dx_no_mb": "backward", "dx_no_kg": "backward",
    "dx_gamma_without_invstd": "backward", "addend_dropped": "backward",
    "pool_last_max": "pool_forward", "pool_zero_winner_passes": "pool_backward", "pool_origin_off_by_one": "pool_forward",
    "pool_py1_not_skipped": "pool_backward",
}


def _fl(v):
    return np.asarray(v, F64).astype(F32)


def _channel_of(shape, vec, by_hw=False):
    """The channel every element is given: (unit / units-per-row) % C — `by_hw`: (unit / HW) % C, the mutant."""
    N, C, H, W = shape
    unit = np.arange(N * C * H * W, dtype=np.int64) // vec
    return ((unit // (H * W if by_hw else (H * W) // vec)) % C).reshape(shape)


def _emulate_stats(x, gamma, beta, running_mean, running_var, momentum, eps, mutant):
    x32 = np.asarray(x, F32)
    N, C, H, W = x32.shape
    x64 = x32.astype(F64)
    S, per = splits(N, C)
    used = (N // per) * per if (mutant == "ragged_split_dropped" and N % per) else N
    count = float(N * H * W)
    a, b = x64[:used].sum(axis=(0, 2, 3)), (x64[:used] * x64[:used]).sum(axis=(0, 2, 3))
    mean = a / count
    var = np.maximum(b / count - mean * mean, 0.0)
    unb = var * count / (count - 1.0) if count > 1 else var
    eps64, m = float(F32(eps)), float(F32(momentum))
    vn = unb if mutant == "unbiased_var_normalises" else var
    invstd = _fl(1.0 / (np.sqrt(vn) + eps64) if mutant == "eps_after_sqrt" else 1.0 / np.sqrt(vn + eps64))
    g = np.ones(C, F32) if gamma is None else np.asarray(gamma, F32)
    bt = np.zeros(C, F32) if beta is None else np.asarray(beta, F32)
    scale = g * invstd                                        # fp32 product
    shift = _fl(bt.astype(F64) - mean * scale.astype(F64))
    rm = rv = None
    if running_mean is not None:
        rm64, rv64 = np.asarray(running_mean, F32).astype(F64), np.asarray(running_var, F32).astype(F64)
        rvar = var if mutant == "biased_running_var" else unb
        if mutant == "momentum_wrong_term":
            rm, rv = _fl(m * rm64 + (1 - m) * mean), _fl(m * rv64 + (1 - m) * rvar)
        else:
            rm, rv = _fl((1 - m) * rm64 + m * mean), _fl((1 - m) * rv64 + m * rvar)
    return _fl(mean), invstd, scale, shift, rm, rv


def emulate_forward(x, gamma, beta, running_mean, running_var, momentum, eps, relu=False, residual=None, mutant=None):
    """bn_train_forward in numpy fp32 (double sums, then the kernel's casts): (y, mean, invstd, rm, rv)."""
    x32 = np.asarray(x, F32)
    mean, invstd, scale, shift, rm, rv = _emulate_stats(x32, gamma, beta, running_mean, running_var, momentum, eps, mutant)
    ch = _channel_of(x32.shape, bn_form(x32.shape[2] * x32.shape[3]), mutant == "channel_by_hw")
    y = _fl(x32.astype(F64) * scale.astype(F64)[ch] + shift.astype(F64)[ch])          # one rounding: fmaf
    if residual is not None:
        y = y + np.asarray(residual, F32)
    if relu:
        y = np.where(y < 0, F32(0), y)
    return y, mean, invstd, rm, rv


def _emulate_bwd_tail(g, x32, mean32, invstd32, gamma, addend, mutant, g_sums=None):
    """reduce + finalize + dx of the kernels on the fp32 gradient g (`g_sums`: what the reductions see instead: the stem
    tail's run over the windows in double, not over the fp32 pixel sums)."""
    N, C, H, W = x32.shape
    count = float(N * H * W)
    mu, is_ = np.asarray(mean32, F32), np.asarray(invstd32, F32)
    gam = np.ones(C, F32) if gamma is None else np.asarray(gamma, F32)
    d = x32 - mu[None, :, None, None]
    xhat = d * is_[None, :, None, None]
    gs = g.astype(F64) if g_sums is None else g_sums
    sb = gs.sum(axis=(0, 2, 3))
    sg = (gs * xhat.astype(F64)).sum(axis=(0, 2, 3))
    k = gam if mutant == "dx_gamma_without_invstd" else gam * is_
    mb = _fl(sb / count)
    kg = is_ * _fl(sg / count)
    if mutant == "dx_no_mb":
        mb = np.zeros_like(mb)
    if mutant == "dx_no_kg":
        kg = np.zeros_like(kg)
    c4 = lambda v: v[None, :, None, None]
    dx = c4(k) * ((g - c4(mb)) - d * c4(kg))
    if addend is not None and mutant != "addend_dropped":
        dx = dx + np.asarray(addend, F32)
    return dx.astype(F32), _fl(sg), _fl(sb)


def emulate_backward(gy, y, x, mean32, invstd32, gamma, addend=None, mutant=None):
    """bn_train_backward[_add] in numpy fp32: (dx, dgamma, dbeta, dres)."""
    gy, x32 = np.asarray(gy, F32), np.asarray(x, F32)
    if y is None:
        g = gy
    else:
        y = np.asarray(y, F32)
        g = np.where((y >= 0) if mutant == "relu_mask_ge" else (y > 0), gy, F32(0))
    dx, dgamma, dbeta = _emulate_bwd_tail(g, x32, mean32, invstd32, gamma, addend, mutant)
    return dx, dgamma, dbeta, (gy if mutant == "dres_unmasked" else g)


def emulate_pool_forward(x, gamma, beta, running_mean, running_var, momentum, eps, mutant=None):
    """bn_relu_maxpool_train_forward in numpy fp32: (p, code, mean, invstd, rm, rv)."""
    x32 = np.asarray(x, F32)
    mean, invstd, scale, shift, rm, rv = _emulate_stats(x32, gamma, beta, running_mean, running_var, momentum, eps, mutant)
    v = _fl(x32.astype(F64) * _c(scale) + _c(shift))
    v = np.where(v < 0, F32(0), v)
    if mutant == "pool_origin_off_by_one":               # window columns 2 px .. 2 px + 2 instead of 2 px - 1 .. 2 px + 1
        v = np.concatenate([v[..., 1:], np.full_like(v[..., :1], -1)], axis=-1)
    p, code = _first_max(_windows(v, F32(-1)), last=mutant == "pool_last_max")
    return p.astype(F32), code, mean, invstd, rm, rv


# what stands behind the pooled tensors in the backward cases: one more pooled row whose codes name window row 0 with an
# open window and a large gradient.  The kernel never reads it (py1 >= Hp is skipped); a kernel that does adds it to dx.
TAIL_P, TAIL_GY = F32(1.0), F32(4096.0)


def emulate_pool_backward(gy, p, code, x, mean32, invstd32, gamma, mutant=None):
    """bn_relu_maxpool_train_backward in numpy fp32: (dx, dgamma, dbeta).  The pixel sums are fp32 adds in raster order
    of the windows."""
    x32 = np.asarray(x, F32)
    N, C, H, W = x32.shape
    g, _, _ = route(gy, p, code, x32.shape, dtype=F32, mask_ge=mutant == "pool_zero_winner_passes")
    g64, _, _ = route(gy, p, code, x32.shape, mask_ge=mutant == "pool_zero_winner_passes")
    dx, dgamma, dbeta = _emulate_bwd_tail(g, x32, mean32, invstd32, gamma, None, mutant, g_sums=g64)
    if mutant == "pool_py1_not_skipped" and H % 2 == 0:
        # the last image row of every plane also takes "pooled row Hp": the next plane's row 0 (its codes name window
        # rows 1 and 2, never the row 0 asked for: nothing) — and behind the last plane the tail above: code px % 3
        Wp = half(W)
        px = np.arange(Wp)
        q = 2 * px - 1 + px % 3
        ok = (q >= 0) & (q < W)
        extra = np.zeros(W, F32)
        np.add.at(extra, q[ok], TAIL_GY)
        k = (np.ones(C, F32) if gamma is None else np.asarray(gamma, F32))[C - 1] * np.asarray(invstd32, F32)[C - 1]
        dx = dx.copy()
        dx[N - 1, C - 1, H - 1] += k * extra
    return dx, dgamma, dbeta


# ---------------------------------------------------------------------------------------------------- cases and inputs
EPS, MOMENTUM = 1e-5, 0.1

# name: (shape, what the row is there to reach, the mutants this row is designed to catch)
CASES = {
    # ---- the BatchNorm op (bn_train_forward / backward / backward_add)
    "bn_per_image_odd": ((2, 40, 3, 3), "scalar units, one image per split, < 64 units per block",
                         ("unbiased_var_normalises", "biased_running_var", "eps_after_sqrt", "momentum_wrong_term",
                          "relu_mask_ge", "dres_unmasked", "dx_no_mb", "dx_no_kg", "dx_gamma_without_invstd", "addend_dropped")),
    "bn_ragged": ((5, 300, 3, 4), "float4 units, splits of 2 + 2 + 1 images", ("ragged_split_dropped", "channel_by_hw")),
    "bn_capped": ((130, 3, 2, 2), "the 64-split cap: 44 splits of 3, the last with one image", ()),
    "bn_single": ((2, 1024, 2, 2), "one split for everything", ()),
    "bn_odd_channels": ((3, 65, 5, 8), "float4 units, a second finalize block with one channel", ()),
    "bn_long_block": ((2, 3, 9, 128), "more than 256 units per block: the block's stride loop", ()),
    "bn_one_pixel": ((2, 3, 1, 1), "count == 2", ()),
    # ---- the stem tail (bn_relu_maxpool_train_forward / backward); every one is a BatchNorm-op case as well
    "pool_both_limits": ((1, 2, 128, 128), "H*W == 16384 and Hp*Wp == 4096: the LDS forms at both limits",
                         ("pool_last_max", "pool_zero_winner_passes", "pool_origin_off_by_one")),
    "pool_over_plane": ((1, 2, 128, 129), "H*W just over: gather forward, scalar gather backward with a lane loop", ()),
    "pool_hwp_limit": ((1, 1, 2, 8192), "Hp*Wp == 4096 in one pooled row", ()),
    "pool_hwp_over": ((1, 1, 1, 16384), "LDS forward, Hp*Wp == 8192: float4 gather backward, lane loop of 64 steps", ()),
    "pool_v4_loop": ((1, 2, 66, 260), "gather forward, float4 gather backward with W / 4 == 65: one lane loops", ()),
    "pool_v4_rows": ((1, 2, 130, 128), "float4 gather backward with two rows per wave (lpr_shift 5)",
                     ("pool_py1_not_skipped",)),
    "pool_scalar_ragged": ((3, 5, 9, 67), "odd everything: scalar forms, ragged last block", ()),
    "pool_scalar_rows": ((2, 2, 6, 7), "scalar gather backward with eight rows per wave, even H", ()),
    "pool_lds_small": ((2, 3, 6, 10), "LDS forms with W % 4 != 0", ()),
    "pool_1x1": ((2, 3, 1, 1), "a single pixel", ()),
    "pool_2x1": ((2, 3, 2, 1), "one column", ()),
    "pool_1x2": ((1, 2, 1, 2), "count == 2", ()),
}
BN_CASES = tuple(CASES)
POOL_CASES = tuple(k for k in CASES if k.startswith("pool_"))


def mutant_case(mutant):
    return next(k for k, (_, _, ms) in CASES.items() if mutant in ms)


def _seed(name, what):
    return gen.seed_of("bn_ref", name, what)


def _per_channel(name, C):
    """gamma (negative every fifth channel), beta, running statistics, the gradient scale 1e-6 .. 1e4 of each channel."""
    c = np.arange(C)
    gamma = (0.75 + 0.75 * gen.uniform(_seed(name, "gamma"), (C,))) * np.where(c % 5 == 4, -1.0, 1.0)
    beta = 0.3 * gen.normal(_seed(name, "beta"), (C,))
    rm = 0.5 * gen.normal(_seed(name, "rm"), (C,))
    rv = 0.5 + gen.uniform(_seed(name, "rv"), (C,))
    gscale = 10.0 ** np.array([0, -6, 4, -3, 2])[c % 5]
    return gamma.astype(F32), beta.astype(F32), rm.astype(F32), rv.astype(F32), gscale


def bn_inputs(name):
    """The tensors of a BatchNorm-op case: x with channels of mean 30 / std 2 (c % 7 == 1), mean -1 / std 30 (c % 7 == 2)
    and one constant channel (c % 7 == 3: var == 0), a residual, gy on the per-channel scales, an addend."""
    shape = CASES[name][0]
    N, C, H, W = shape
    c = np.arange(C)
    x = gen.normal(_seed(name, "x"), shape).astype(F64)
    mu = np.where(c % 7 == 1, 30.0, np.where(c % 7 == 2, -1.0, 0.25 * (c % 3)))
    sd = np.where(c % 7 == 1, 2.0, np.where(c % 7 == 2, 30.0, 1.0))
    x = x * _c(sd) + _c(mu)
    x[:, c % 7 == 3] = 0.75
    gamma, beta, rm, rv, gscale = _per_channel(name, C)
    gy = gen.normal(_seed(name, "gy"), shape) * _c(gscale)
    return {"x": x.astype(F32), "gamma": gamma, "beta": beta, "rm": rm, "rv": rv,
            "residual": (2.0 * gen.normal(_seed(name, "res"), shape)).astype(F32), "gy": gy.astype(F32),
            "addend": (gen.normal(_seed(name, "add"), shape) * _c(gscale)).astype(F32)}


def plant_y(y):
    """The forward's y with +0, -0, the smallest subnormal and a negative planted along the flat index (what a ReLU
    output never holds is there on purpose: the mask is `y > 0` on whatever bits arrive)."""
    y = np.array(y, F32)
    f = y.reshape(-1)
    i = np.arange(f.size)
    f[i % 11 == 0], f[i % 11 == 1], f[i % 11 == 2], f[i % 11 == 3] = F32(0.0), F32(-0.0), F32(2.0 ** -149), F32(-1.5)
    return y


def pool_inputs(name):
    """x on the grid k / 4, |k| <= 12 (+ 32 in channel 1: a large mean, still exact), so that equal inputs give
    bit-equal values and distinct ones differ by |scale| / 4 >= 1/8; on top, in every fourth interior window of both
    directions, a tie of two equal extreme levels at the position pair (window index mod 36); a 5 x 5 corner of the
    opposite extreme where both extents reach 8 (windows the ReLU closes); and a higher level at the pixels (5 + 8i, 5 + 8j), which win four
    windows each."""
    shape = CASES[name][0]
    N, C, H, W = shape
    gamma, beta, rm, rv, gscale = _per_channel(name, C)
    gamma = np.where(gamma < 0, gamma - F32(0.25), gamma + F32(0.25)).astype(F32)       # |gamma| >= 1
    sgn = np.sign(gamma).astype(F64)
    x = np.clip(np.round(gen.normal(_seed(name, "x"), shape).astype(F64) * 4), -12, 12) / 4
    pairs = [(a, b) for a in range(9) for b in range(a + 1, 9)]
    Hp, Wp = half(H), half(W)
    lev = _c(sgn)[0, :, 0, 0]
    if H >= 8 and W >= 8:
        x[:, :, :5, :5] = -6.0 * _c(sgn)
    w = 0
    for py in range(1, Hp, 4):
        for px in range(1, Wp, 4):
            if 2 * py + 1 < H and 2 * px + 1 < W and (py, px) != (1, 1):
                for pos in pairs[w % 36]:
                    x[:, :, 2 * py - 1 + pos // 3, 2 * px - 1 + pos % 3] = (4.0 + 0.25 * (w % 3)) * lev
                w += 1
    x[:, :, 5::8, 5::8] = 5.0 * _c(sgn)
    if C > 1:
        x[:, 1] += 32.0
    gy = gen.normal(_seed(name, "gp"), (N, C, Hp, Wp)) * _c(gscale)
    return {"x": x.astype(F32), "gamma": gamma, "beta": beta, "rm": rm, "rv": rv, "gy": gy.astype(F32)}


def handmade_codes(name):
    """Valid (p, code) that no forward would give: every window of each 2 x 2 neighbourhood of pooled outputs names
    the pixel (2 py + 1, 2 px + 1) they share (where that pixel exists), the others their centre; p is 0 (closed), the
    smallest subnormal or 1 along the flat index."""
    N, C, H, W = CASES[name][0]
    Hp, Wp = half(H), half(W)
    py, px = np.meshgrid(np.arange(Hp), np.arange(Wp), indexing="ij")
    by, bx = 2 * (py // 2) + 1, 2 * (px // 2) + 1                    # the shared pixel of the neighbourhood
    wy, wx = by - (2 * py - 1), bx - (2 * px - 1)
    ok = (by < H) & (bx < W) & (wy >= 0) & (wy < 3) & (wx >= 0) & (wx < 3)
    code = np.where(ok, 3 * wy + wx, 4).astype(np.uint8)
    code = np.broadcast_to(code, (N, C, Hp, Wp)).copy()
    i = np.arange(code.size).reshape(code.shape)
    p = np.where(i % 7 == 3, F32(0), np.where(i % 7 == 5, F32(2.0 ** -149), F32(1))).astype(F32)
    return p, code


def backward_inputs(name):
    """bn_inputs plus what the backward entry points take from a forward: oracle-made fp32 y (ReLU and residual, then
    plant_y), save_mean and save_invstd."""
    i = dict(bn_inputs(name))
    y, mean, invstd, _, _ = forward_ref(i["x"], i["gamma"], i["beta"], None, None, MOMENTUM, EPS, True, i["residual"])
    i["y"], i["mean"], i["invstd"] = plant_y(y.astype(F32)), mean.astype(F32), invstd.astype(F32)
    return i


def pool_backward_inputs(name):
    """pool_inputs plus oracle-made fp32 save_mean / save_invstd, the oracle's own (p, code) and the hand-made pair."""
    i = dict(pool_inputs(name))
    ref, _ = _forward(i["x"], i["gamma"], i["beta"], None, None, MOMENTUM, EPS, False, None)
    p, code = pool_forward_ref(i["x"], ref["scale"], ref["shift"])
    i["mean"], i["invstd"], i["p"], i["code"] = ref["mean"].astype(F32), ref["invstd"].astype(F32), p.astype(F32), code
    i["hand_p"], i["hand_code"] = handmade_codes(name)
    return i


def pool_forward_oracle(i):
    """float64 (p, code, bound of p, the pre-ReLU values, their bound) of a pool_inputs dict."""
    ref, bound = _forward(i["x"], i["gamma"], i["beta"], None, None, MOMENTUM, EPS, False, None)
    p, code = pool_forward_ref(i["x"], ref["scale"], ref["shift"])
    return p, code, window_max(bound["y"]), ref["y"], bound["y"]

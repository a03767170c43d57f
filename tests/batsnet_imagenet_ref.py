"""Float64 restatements of the two ImageNet stem kernels (csrc/bats_stem_in.hip) with their rounding bounds, shared by
tests/test_batsnet_imagenet_cpu.py and tests/test_gpu_batsnet_imagenet.py.  u = 2^-24 is the unit roundoff of fp32; an
fp32 chain of n fused multiply-adds is within gamma_n <= (n + small) u of the exact sum of the magnitudes."""
import torch
import torch.nn.functional as F

U = 2.0 ** -24


def _col(v):
    return v.double().view(1, -1, 1, 1)


def stem_s2x2_f64(x, w1, s1, t1, w2, s2, t2, groups, relu_out):
    """``(y64, bound)`` of kernel (a) for CPU tensors:
        A1 = |s1| conv(|x|, |w1|) + |t1|,  e1 = 32 u A1            (27 fmaf + the BatchNorm's, rounded up; ReLU is 1-Lipschitz)
        n2 = 9 C1 / G + 1,  A2 = |s2| gconv(|y1|, |w2|) + |t2|
        bound = (n2 + 4) u A2 + (1 + (n2 + 4) u) |s2| gconv(e1, |w2|)
    F.conv2d pads with zeros: taps of the second convolution outside the H1 x W1 map contribute nothing."""
    x, w1, w2 = x.double(), w1.double(), w2.double()
    s1, t1, s2, t2 = _col(s1), _col(t1), _col(s2), _col(t2)
    y1 = torch.clamp_min(s1 * F.conv2d(x, w1, stride=2, padding=1) + t1, 0.0)
    y = s2 * F.conv2d(y1, w2, stride=2, padding=1, groups=groups) + t2
    e1 = 32 * U * (s1.abs() * F.conv2d(x.abs(), w1.abs(), stride=2, padding=1) + t1.abs())
    n2 = 9 * (w1.shape[0] // groups) + 1
    a2 = s2.abs() * F.conv2d(y1.abs(), w2.abs(), stride=2, padding=1, groups=groups) + t2.abs()
    bound = (n2 + 4) * U * a2 + (1 + (n2 + 4) * U) * s2.abs() * F.conv2d(e1, w2.abs(), stride=2, padding=1, groups=groups)
    return (torch.clamp_min(y, 0.0) if relu_out else y), bound


def gconv3x3s2_f64(x, w, s, t, groups, relu_in):
    """``(y64, bound)`` of kernel (b): bound = (9 C_in / G + 5) u (|s| gconv(|x'|, |w|) + |t|), x' the input as loaded."""
    x, w, s, t = x.double(), w.double(), _col(s), _col(t)
    if relu_in:
        x = torch.clamp_min(x, 0.0)
    y = s * F.conv2d(x, w, stride=2, padding=1, groups=groups) + t
    n = 9 * (x.shape[1] // groups) + 5
    return y, n * U * (s.abs() * F.conv2d(x.abs(), w.abs(), stride=2, padding=1, groups=groups) + t.abs())

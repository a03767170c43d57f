// pack_ste.hip — what the backward of a binary convolution needs from its input, in 3 bits per element.
//
// Reference: the autograd graph of bnn/layers/conv.py:90-97 keeps the fp32 input x alive for the backward of
// SignActivation (bnn/ops.py:68-73: grad * 1[|x| < 1]) and the fp32 sign(x) for the weight gradient.  Both are
// functions of three bits per element:
//     P = x > 0,  M = x < 0        (sign(x): the planes bnn_hip_pack_act_f32 writes, same format)
//     T = |x| < 1                  (the hard-tanh straight-through mask; NaN -> 0, like masked_fill(x.abs() >= 1, 0))
// written here in ONE pass over x as three [N][ceil(C/64)][H][W] uint64 planes — 32 -> 3 bits per element of saved
// state for every binary layer of a training step (csrc/grad.hip reads them: dgrad the T plane, wgrad P and M).
// HBM-bound: 4 B read + 3 bits written per element.  Same thread mapping as pack_act.hip.
#include "planes.h"

namespace bnn {

// AFF: the planes of u = fmaf(x, a[c], b[c]) — BatchNorm in front of sign(), as pack_act_kernel<VP, true> evaluates it (the
// expression of bn_apply_kernel, so the bits of packing its output) — without ever writing u: the training forward of a
// BATS cell operation (bnn_hip_bn_act_pack_ste_f32 / bnn_hip_bn_train_pack_ste_f32); a == NULL there: u = x, the planes
// of the plain kernel.  Plain loads: the convolution launch behind it reads x again as the skip connection.
// The affine travels as ONE kernel argument, empty for the plain kernel: its argument block is then the parent's
// (x .. cw64, P, M, T; the empty struct sits in the padding behind cw64).  Keep the order x .. cw64, bn, P, M, T.
template <bool AFF>
struct SteAffine {
  const float *__restrict__ a, *__restrict__ b;
};
template <>
struct SteAffine<false> {};
static_assert(std::is_empty_v<SteAffine<false>> && sizeof(SteAffine<true>) == 2 * sizeof(const float*), "see above");

template <int VP, bool AFF>
__global__ __launch_bounds__(256) void pack_ste_kernel(const float* __restrict__ x, int C, int HW, long long npix,
                                                       int cw64, SteAffine<AFF> bn, uint64_t* __restrict__ P,
                                                       uint64_t* __restrict__ M, uint64_t* __restrict__ T) {
  using V = PixVec<float, VP>;
  const float *__restrict__ bn_a = nullptr, *__restrict__ bn_b = nullptr;
  if constexpr (AFF) { bn_a = bn.a; bn_b = bn.b; }
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long pix0 = t * VP;
  if (pix0 >= npix) return;
  const int g = blockIdx.y;
  const int n = (int)(pix0 / HW);
  const int r = (int)(pix0 - (long long)n * HW);
  const float* xb = x + ((size_t)n * C) * HW + r;
  uint32_t pw[2][VP], mw[2][VP], tw[2][VP];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int v = 0; v < VP; ++v) { pw[h][v] = 0u; mw[h][v] = 0u; tw[h][v] = 0u; }
    const int c0 = g * 64 + h * 32;
    for (int b = 0; b < 32 && c0 + b < C; ++b) {
      const V xv = *reinterpret_cast<const V*>(xb + (size_t)(c0 + b) * HW);
      const Affine f = channel_affine(bn_a, bn_b, c0 + b);
#pragma unroll
      for (int v = 0; v < VP; ++v) {
        const float u = f(xv.v[v]);
        pw[h][v] = with_p(pw[h][v], u, b);
        mw[h][v] = with_m(mw[h][v], u, b);
        tw[h][v] = with_t(tw[h][v], u, b);
      }
    }
  }
  const size_t o = word_off(n, cw64, g, HW, r);
#pragma unroll
  for (int v = 0; v < VP; ++v) {
    P[o + v] = join_halves(pw[0][v], pw[1][v]);
    M[o + v] = join_halves(mw[0][v], mw[1][v]);
    T[o + v] = join_halves(tw[0][v], tw[1][v]);
  }
}

template <bool AFF>
static int launch_ste(const float* x, int N, int C, int H, int W, const float* bn_a, const float* bn_b, uint64_t* P,
                      uint64_t* M, uint64_t* T, hipStream_t stream) {
  const int HW = H * W;
  const long long npix = (long long)N * HW;
  const int cw64 = (C + 63) / 64;
  SteAffine<AFF> bn;
  if constexpr (AFF) bn = {bn_a, bn_b};
  with_width(HW, x, sizeof(float), [&](auto vp) {
    constexpr int VP = decltype(vp)::value;
    hipLaunchKernelGGL((pack_ste_kernel<VP, AFF>), stream_grid(npix / VP, cw64), dim3(256), 0, stream, x, C, HW, npix,
                       cw64, bn, P, M, T);
  });
  return launch_status();
}

int launch_pack_ste(const float* x, int N, int C, int H, int W, uint64_t* P, uint64_t* M, uint64_t* T,
                    hipStream_t stream) {
  return launch_ste<false>(x, N, C, H, W, nullptr, nullptr, P, M, T, stream);
}

int launch_bn_pack_ste(const float* x, int N, int C, int H, int W, const float* bn_a, const float* bn_b, uint64_t* P,
                       uint64_t* M, uint64_t* T, hipStream_t stream) {
  return launch_ste<true>(x, N, C, H, W, bn_a, bn_b, P, M, T, stream);
}

// The three planes of the two pixel lattices FactorizedReduce reads (bnn/models/layers/bats_ops.py:204-206): phase 0 =
// u[2i, 2j], phase 1 = u[2i+1, 2j+1], u = fmaf(x, a[c], b[c]) as above — the training forward of that module
// (bnn_hip_bn_act_pack_ste_s2_f32 / bnn_hip_bn_train_pack_ste_s2_f32).  Thread mapping of pack_act_s2_kernel
// (pack_act.hip): one thread = one output pixel of one 64-channel word, two loads per channel (rows 2i and 2i+1 of the
// plane: every line of x is fetched once), three words per phase out.  Each plane is [2][N][cw64][H/2][W/2]; the ragged
// last word as above.  Plain loads: the backward reads x again.
__global__ __launch_bounds__(256) void bn_pack_ste_s2_kernel(const float* __restrict__ x, int C, int W, int Ho, int Wo,
                                                             long long npix, int cw64, const float* __restrict__ bn_a,
                                                             const float* __restrict__ bn_b, uint64_t* __restrict__ P,
                                                             uint64_t* __restrict__ M, uint64_t* __restrict__ T,
                                                             size_t set_stride) {
  const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
  if (q >= npix) return;
  const int g = blockIdx.y;
  const int HWo = Ho * Wo;
  const size_t HW = (size_t)4 * HWo;
  const auto [n, r, i, j] = out_pixel(q, HWo, Wo);
  const float* xb = x + ((size_t)n * C) * HW + (size_t)(2 * i) * W + 2 * j;
  uint32_t pw[2][2] = {{0u, 0u}, {0u, 0u}}, mw[2][2] = {{0u, 0u}, {0u, 0u}}, tw[2][2] = {{0u, 0u}, {0u, 0u}};  // [phase][half]
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int c0 = g * 64 + h * 32;
    for (int b = 0; b < 32 && c0 + b < C; ++b) {
      const float* xc = xb + (size_t)(c0 + b) * HW;
      const float v[2] = {xc[0], xc[W + 1]};
      const Affine f = channel_affine(bn_a, bn_b, c0 + b);
#pragma unroll
      for (int ph = 0; ph < 2; ++ph) {
        const float u = f(v[ph]);
        pw[ph][h] = with_p(pw[ph][h], u, b);
        mw[ph][h] = with_m(mw[ph][h], u, b);
        tw[ph][h] = with_t(tw[ph][h], u, b);
      }
    }
  }
  const size_t o = word_off(n, cw64, g, HWo, r);
#pragma unroll
  for (int ph = 0; ph < 2; ++ph) {
    P[ph * set_stride + o] = join_halves(pw[ph][0], pw[ph][1]);
    M[ph * set_stride + o] = join_halves(mw[ph][0], mw[ph][1]);
    T[ph * set_stride + o] = join_halves(tw[ph][0], tw[ph][1]);
  }
}

// H and W even (capi.hip has checked that).
int launch_bn_pack_ste_s2(const float* x, int N, int C, int H, int W, const float* bn_a, const float* bn_b, uint64_t* P,
                          uint64_t* M, uint64_t* T, hipStream_t stream) {
  const int Ho = H / 2, Wo = W / 2;
  const long long npix = (long long)N * Ho * Wo;
  const int cw64 = (C + 63) / 64;
  hipLaunchKernelGGL(bn_pack_ste_s2_kernel, stream_grid(npix, cw64), dim3(256), 0, stream, x, C, W, Ho, Wo, npix, cw64,
                     bn_a, bn_b, P, M, T, plane_set_stride(npix, cw64));
  return launch_status();
}

}  // namespace bnn

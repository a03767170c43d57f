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
#include "bnn_dev.h"

namespace bnn {

template <int VP>
__global__ __launch_bounds__(256) void pack_ste_kernel(const float* __restrict__ x, int C, int HW, long long npix,
                                                       int cw64, uint64_t* __restrict__ P, uint64_t* __restrict__ M,
                                                       uint64_t* __restrict__ T) {
  struct alignas(4 * VP) V { float v[VP]; };
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
#pragma unroll
      for (int v = 0; v < VP; ++v) {
        const float u = xv.v[v];
        pw[h][v] |= (is_pos(u) ? 1u : 0u) << b;
        mw[h][v] |= (is_neg(u) ? 1u : 0u) << b;
        tw[h][v] |= (fabsf(u) < 1.0f ? 1u : 0u) << b;
      }
    }
  }
  const size_t o = ((size_t)n * cw64 + g) * HW + r;
#pragma unroll
  for (int v = 0; v < VP; ++v) {
    P[o + v] = (uint64_t)pw[0][v] | ((uint64_t)pw[1][v] << 32);
    M[o + v] = (uint64_t)mw[0][v] | ((uint64_t)mw[1][v] << 32);
    T[o + v] = (uint64_t)tw[0][v] | ((uint64_t)tw[1][v] << 32);
  }
}

int launch_pack_ste(const float* x, int N, int C, int H, int W, uint64_t* P, uint64_t* M, uint64_t* T,
                    hipStream_t stream) {
  const int HW = H * W;
  const long long npix = (long long)N * HW;
  const int cw64 = (C + 63) / 64;
  const bool a4 = (reinterpret_cast<uintptr_t>(x) & 15) == 0, a2 = (reinterpret_cast<uintptr_t>(x) & 7) == 0;
  auto grid = [&](long long nthr) { return dim3((unsigned)((nthr + 255) / 256), (unsigned)cw64); };
  if (HW % 4 == 0 && a4)
    hipLaunchKernelGGL(pack_ste_kernel<4>, grid(npix / 4), dim3(256), 0, stream, x, C, HW, npix, cw64, P, M, T);
  else if (HW % 2 == 0 && a2)
    hipLaunchKernelGGL(pack_ste_kernel<2>, grid(npix / 2), dim3(256), 0, stream, x, C, HW, npix, cw64, P, M, T);
  else
    hipLaunchKernelGGL(pack_ste_kernel<1>, grid(npix), dim3(256), 0, stream, x, C, HW, npix, cw64, P, M, T);
  return hipGetLastError() == hipSuccess ? BNN_HIP_OK : BNN_HIP_ERR_LAUNCH;
}

// The same three planes of u = fmaf(x, a[c], b[c]) — BatchNorm in front of sign(), as pack_act_kernel<VP, true> evaluates
// it (the expression of bn_apply_kernel, so the bits of packing its output) — without ever writing u: the training
// forward of a BATS cell operation (bnn_hip_bn_act_pack_ste_f32 / bnn_hip_bn_train_pack_ste_f32).  a == NULL: u = x,
// the planes of pack_ste_kernel.  Same thread mapping, vector forms and ragged last word as above.  Plain loads: the
// convolution launch behind it reads x again as the skip connection.
template <int VP>
__global__ __launch_bounds__(256) void bn_pack_ste_kernel(const float* __restrict__ x, int C, int HW, long long npix,
                                                          int cw64, const float* __restrict__ bn_a,
                                                          const float* __restrict__ bn_b, uint64_t* __restrict__ P,
                                                          uint64_t* __restrict__ M, uint64_t* __restrict__ T) {
  struct alignas(4 * VP) V { float v[VP]; };
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
      const float ca = bn_a ? bn_a[c0 + b] : 1.0f, cb = bn_a ? bn_b[c0 + b] : 0.0f;
#pragma unroll
      for (int v = 0; v < VP; ++v) {
        const float u = bn_a ? fmaf(xv.v[v], ca, cb) : xv.v[v];
        pw[h][v] |= (is_pos(u) ? 1u : 0u) << b;
        mw[h][v] |= (is_neg(u) ? 1u : 0u) << b;
        tw[h][v] |= (fabsf(u) < 1.0f ? 1u : 0u) << b;
      }
    }
  }
  const size_t o = ((size_t)n * cw64 + g) * HW + r;
#pragma unroll
  for (int v = 0; v < VP; ++v) {
    P[o + v] = (uint64_t)pw[0][v] | ((uint64_t)pw[1][v] << 32);
    M[o + v] = (uint64_t)mw[0][v] | ((uint64_t)mw[1][v] << 32);
    T[o + v] = (uint64_t)tw[0][v] | ((uint64_t)tw[1][v] << 32);
  }
}

int launch_bn_pack_ste(const float* x, int N, int C, int H, int W, const float* bn_a, const float* bn_b, uint64_t* P,
                       uint64_t* M, uint64_t* T, hipStream_t stream) {
  const int HW = H * W;
  const long long npix = (long long)N * HW;
  const int cw64 = (C + 63) / 64;
  const bool a4 = (reinterpret_cast<uintptr_t>(x) & 15) == 0, a2 = (reinterpret_cast<uintptr_t>(x) & 7) == 0;
  auto grid = [&](long long nthr) { return dim3((unsigned)((nthr + 255) / 256), (unsigned)cw64); };
  if (HW % 4 == 0 && a4)
    hipLaunchKernelGGL(bn_pack_ste_kernel<4>, grid(npix / 4), dim3(256), 0, stream, x, C, HW, npix, cw64, bn_a, bn_b, P, M, T);
  else if (HW % 2 == 0 && a2)
    hipLaunchKernelGGL(bn_pack_ste_kernel<2>, grid(npix / 2), dim3(256), 0, stream, x, C, HW, npix, cw64, bn_a, bn_b, P, M, T);
  else
    hipLaunchKernelGGL(bn_pack_ste_kernel<1>, grid(npix), dim3(256), 0, stream, x, C, HW, npix, cw64, bn_a, bn_b, P, M, T);
  return hipGetLastError() == hipSuccess ? BNN_HIP_OK : BNN_HIP_ERR_LAUNCH;
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
  const int n = (int)(q / HWo);
  const int r = (int)(q - (long long)n * HWo);
  const int i = r / Wo, j = r - i * Wo;
  const float* xb = x + ((size_t)n * C) * HW + (size_t)(2 * i) * W + 2 * j;
  uint32_t pw[2][2] = {{0u, 0u}, {0u, 0u}}, mw[2][2] = {{0u, 0u}, {0u, 0u}}, tw[2][2] = {{0u, 0u}, {0u, 0u}};  // [phase][half]
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int c0 = g * 64 + h * 32;
    for (int b = 0; b < 32 && c0 + b < C; ++b) {
      const float* xc = xb + (size_t)(c0 + b) * HW;
      const float v[2] = {xc[0], xc[W + 1]};
      const float ca = bn_a ? bn_a[c0 + b] : 1.0f, cb = bn_a ? bn_b[c0 + b] : 0.0f;
#pragma unroll
      for (int ph = 0; ph < 2; ++ph) {
        const float u = bn_a ? fmaf(v[ph], ca, cb) : v[ph];
        pw[ph][h] |= (is_pos(u) ? 1u : 0u) << b;
        mw[ph][h] |= (is_neg(u) ? 1u : 0u) << b;
        tw[ph][h] |= (fabsf(u) < 1.0f ? 1u : 0u) << b;
      }
    }
  }
  const size_t o = ((size_t)n * cw64 + g) * HWo + r;
#pragma unroll
  for (int ph = 0; ph < 2; ++ph) {
    P[ph * set_stride + o] = (uint64_t)pw[ph][0] | ((uint64_t)pw[ph][1] << 32);
    M[ph * set_stride + o] = (uint64_t)mw[ph][0] | ((uint64_t)mw[ph][1] << 32);
    T[ph * set_stride + o] = (uint64_t)tw[ph][0] | ((uint64_t)tw[ph][1] << 32);
  }
}

// H and W even (capi.hip has checked that).
int launch_bn_pack_ste_s2(const float* x, int N, int C, int H, int W, const float* bn_a, const float* bn_b, uint64_t* P,
                          uint64_t* M, uint64_t* T, hipStream_t stream) {
  const int Ho = H / 2, Wo = W / 2;
  const long long npix = (long long)N * Ho * Wo;
  const int cw64 = (C + 63) / 64;
  const dim3 grid((unsigned)((npix + 255) / 256), (unsigned)cw64);
  hipLaunchKernelGGL(bn_pack_ste_s2_kernel, grid, dim3(256), 0, stream, x, C, W, Ho, Wo, npix, cw64, bn_a, bn_b, P, M, T,
                     (size_t)npix * cw64);
  return hipGetLastError() == hipSuccess ? BNN_HIP_OK : BNN_HIP_ERR_LAUNCH;
}

}  // namespace bnn

// pack_act.hip — sign() of an fp32 NCHW activation tensor as two pixel-major bit planes.
//
// Replaces bnn/ops.py:63-66 (SignActivation.forward: `input.sign()`) as called by
// bnn/ops.py:151-152 (BasicInputBinarizer.forward).  The reference materialises a full
// fp32 tensor of {-1,0,+1}; here the same information is 2 bits per element:
//   P bit = x > 0, M bit = x < 0, neither = 0 / -0 / NaN  (torch.sign semantics).
//
// HBM-bound: reads 4 B/element, writes 2 bits/element.
// Mapping: one thread owns VP consecutive pixels of one image and ONE 64-channel group
// (blockIdx.y), so every global load is a coalesced 4*VP-byte-per-lane row segment of one
// channel plane, every store is VP contiguous uint64 words of the [n][group][y][x] output
// plane, and small images with many channels still fill the chip (parallelism = pixels/VP x
// channel groups).
#include "planes.h"

namespace bnn {

// AFF: v = fmaf(x, bn_a[c], bn_b[c]) first (eval-mode BatchNorm in front of a pre-activation block's
// binary conv: res_block.py:148, hierarchical_block.py:39); relu != 0: planes of sign(max(v, 0)).
template <int VP, bool AFF = false, typename T = float>
__global__ __launch_bounds__(256) void pack_act_kernel(const T* __restrict__ x, int C, int HW, long long npix, int cw64,
                                                       uint64_t* __restrict__ P, uint64_t* __restrict__ M,
                                                       const float* __restrict__ bn_a = nullptr,
                                                       const float* __restrict__ bn_b = nullptr, int relu = 0) {
  using V = PixVec<T, VP>;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long pix0 = t * VP;
  if (pix0 >= npix) return;
  const int g = blockIdx.y;
  const int n = (int)(pix0 / HW);
  const int r = (int)(pix0 - (long long)n * HW);
  const T* xb = x + ((size_t)n * C) * HW + r;

  uint32_t pw[2][VP], mw[2][VP];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int v = 0; v < VP; ++v) { pw[h][v] = 0u; mw[h][v] = 0u; }
    const int c0 = g * 64 + h * 32;
    if (c0 + 32 <= C) {  // (the two walks of a half-word and their inserts: planes.h)
#pragma unroll 16
      for (int b = 31; b >= 0; --b) {
        const V xv = load_once(reinterpret_cast<const V*>(xb + (size_t)(c0 + b) * HW));
        float xs[VP];
#pragma unroll
        for (int v = 0; v < VP; ++v) xs[v] = widen(xv.v[v]);
        const Affine f = channel_affine(AFF ? bn_a : nullptr, bn_b, c0 + b);
#pragma unroll
        for (int v = 0; v < VP; ++v) {
          const float u = f(xs[v]);
          pw[h][v] = with_p<kShiftIn>(pw[h][v], u, b);
          mw[h][v] = with_m<kShiftIn>(mw[h][v], u, b, AFF && relu);
        }
      }
    } else {
      for (int b = 0; b < 32 && c0 + b < C; ++b) {
        const V xv = load_once(reinterpret_cast<const V*>(xb + (size_t)(c0 + b) * HW));
        float xs[VP];
#pragma unroll
        for (int v = 0; v < VP; ++v) xs[v] = widen(xv.v[v]);
        const Affine f = channel_affine(AFF ? bn_a : nullptr, bn_b, c0 + b);
#pragma unroll
        for (int v = 0; v < VP; ++v) {
          const float u = f(xs[v]);
          pw[h][v] = with_p<kOrAt>(pw[h][v], u, b);
          mw[h][v] = with_m<kOrAt>(mw[h][v], u, b, AFF && relu);
        }
      }
    }
  }
  // the VP words of this thread are contiguous
  const size_t o = word_off(n, cw64, g, HW, r);
#pragma unroll
  for (int v = 0; v < VP; ++v) {
    P[o + v] = join_halves(pw[0][v], pw[1][v]);
    M[o + v] = join_halves(mw[0][v], mw[1][v]);
  }
}

template <bool AFF, typename T>
static int launch_pack_act_t(const T* x, int N, int C, int H, int W, const float* bn_a, const float* bn_b, int relu,
                             uint64_t* P, uint64_t* M, hipStream_t stream) {
  const int HW = H * W;
  const long long npix = (long long)N * HW;
  const int cw64 = (C + 63) / 64;
  with_width(HW, x, sizeof(T), [&](auto vp) {
    constexpr int VP = decltype(vp)::value;
    hipLaunchKernelGGL((pack_act_kernel<VP, AFF, T>), stream_grid(npix / VP, cw64), dim3(256), 0, stream, x, C, HW, npix,
                       cw64, P, M, bn_a, bn_b, relu);
  });
  return launch_status();
}

int launch_pack_act(const float* x, int N, int C, int H, int W, uint64_t* P, uint64_t* M, hipStream_t stream) {
  return launch_pack_act_t<false>(x, N, C, H, W, nullptr, nullptr, 0, P, M, stream);
}

int launch_pack_act_f16(const void* x, int N, int C, int H, int W, uint64_t* P, uint64_t* M, hipStream_t stream) {
  return launch_pack_act_t<false>(static_cast<const __half*>(x), N, C, H, W, nullptr, nullptr, 0, P, M, stream);
}

int launch_pack_act_bf16(const void* x, int N, int C, int H, int W, uint64_t* P, uint64_t* M, hipStream_t stream) {
  return launch_pack_act_t<false>(static_cast<const Bf16Bits*>(x), N, C, H, W, nullptr, nullptr, 0, P, M, stream);
}

int launch_bn_act_pack(const float* x, int N, int C, int H, int W, const float* bn_a, const float* bn_b,
                       int relu, uint64_t* P, uint64_t* M, hipStream_t stream) {
  return launch_pack_act_t<true>(x, N, C, H, W, bn_a, bn_b, relu, P, M, stream);
}

// K BatchNorm + sign() plane sets from ONE read of x (a BATS cell state that feeds K SepConv / DilConv operations, each
// with a BatchNorm of its own): pack_act_kernel<VP, true> with K affines per loaded value — K fmaf and 2 K class tests.
// x points at the first element of a channel-slice VIEW: channels [c_off, c_off + C) of [N, c_total, H, W], so the image
// stride is c_total HW (img_stride) while channel planes stay HW apart.  Plane set k is [N][cw64][H][W] at
// P + k set_stride, and holds the bits bn_act_pack writes for affine k.  A thread keeps 4 K VP plane words: VP = 4 only up
// to K = 2 (32 words, as many as K = 4 at VP = 2).
template <int VP, int K>
__global__ __launch_bounds__(256) void pack_act_multi_kernel(const float* __restrict__ x, int C, int HW, size_t img_stride,
                                                             long long npix, int cw64, uint64_t* __restrict__ P,
                                                             uint64_t* __restrict__ M, size_t set_stride,
                                                             const float* __restrict__ scale,
                                                             const float* __restrict__ shift, int relu) {
  using V = PixVec<float, VP>;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long pix0 = t * VP;
  if (pix0 >= npix) return;
  const int g = blockIdx.y;
  const int n = (int)(pix0 / HW);
  const int r = (int)(pix0 - (long long)n * HW);
  const float* xb = x + (size_t)n * img_stride + r;

  uint32_t pw[K][2][VP], mw[K][2][VP];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
      for (int v = 0; v < VP; ++v) { pw[k][h][v] = 0u; mw[k][h][v] = 0u; }
    }
    const int c0 = g * 64 + h * 32;
    if (c0 + 32 <= C) {
#pragma unroll 8
      for (int b = 31; b >= 0; --b) {
        const V xv = load_once(reinterpret_cast<const V*>(xb + (size_t)(c0 + b) * HW));
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const float ca = scale[k * C + c0 + b], cb = shift[k * C + c0 + b];
#pragma unroll
          for (int v = 0; v < VP; ++v) {
            const float u = fmaf(xv.v[v], ca, cb);
            pw[k][h][v] = with_p<kShiftIn>(pw[k][h][v], u, b);
            mw[k][h][v] = with_m<kShiftIn>(mw[k][h][v], u, b, relu);
          }
        }
      }
    } else {
      for (int b = 0; b < 32 && c0 + b < C; ++b) {
        const V xv = load_once(reinterpret_cast<const V*>(xb + (size_t)(c0 + b) * HW));
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const float ca = scale[k * C + c0 + b], cb = shift[k * C + c0 + b];
#pragma unroll
          for (int v = 0; v < VP; ++v) {
            const float u = fmaf(xv.v[v], ca, cb);
            pw[k][h][v] = with_p<kOrAt>(pw[k][h][v], u, b);
            mw[k][h][v] = with_m<kOrAt>(mw[k][h][v], u, b, relu);
          }
        }
      }
    }
  }
  const size_t o = word_off(n, cw64, g, HW, r);
#pragma unroll
  for (int k = 0; k < K; ++k) {
#pragma unroll
    for (int v = 0; v < VP; ++v) {
      P[k * set_stride + o + v] = join_halves(pw[k][0][v], pw[k][1][v]);
      M[k * set_stride + o + v] = join_halves(mw[k][0][v], mw[k][1][v]);
    }
  }
}

// x: the tensor's base; the view is channels [c_off, c_off + C) of c_tot (capi.hip has checked it and 1 <= K <= 4).
int launch_bn_act_pack_multi(const float* x, int c_off, int c_tot, int N, int C, int H, int W, int K, const float* scale,
                             const float* shift, int relu, uint64_t* P, uint64_t* M, hipStream_t stream) {
  const int HW = H * W;
  const long long npix = (long long)N * HW;
  const int cw64 = (C + 63) / 64;
  const float* x0 = x + (size_t)c_off * HW;
  const size_t img_stride = (size_t)c_tot * HW;
  with_k(K, [&](auto kc) {
    constexpr int KV = decltype(kc)::value;
    // the vector width follows HW and the alignment of the VIEW's first element; VP = 4 only up to K = 2 (above)
    with_width<(KV <= 2 ? 4 : 2)>(HW, x0, sizeof(float), [&](auto vp) {
      constexpr int VP = decltype(vp)::value;
      hipLaunchKernelGGL((pack_act_multi_kernel<VP, KV>), stream_grid(npix / VP, cw64), dim3(256), 0, stream, x0, C, HW,
                         img_stride, npix, cw64, P, M, plane_set_stride(npix, cw64), scale, shift, relu);
    });
  });
  return launch_status();
}

// The binarisation inside FactorizedReduce (bnn/models/layers/bats_ops.py:204-206: conv_1(bn(x)) at stride 2 and
// conv_2(bn(x)[:, :, 1:, 1:]) at stride 2, both 1x1): the two convolutions read the pixels (2i, 2j) and (2i+1, 2j+1) of
// bn(x) and nothing else.  One thread = one output pixel and one 64-channel group; per channel it loads those two values
// (rows 2i and 2i+1 of the plane: every line of x is fetched once) and writes phase 0 / phase 1 as two plane sets
// [2][N][cw64][H/2][W/2] with the bits bn_act_pack gives for x[:, :, ::2, ::2] and x[:, :, 1::2, 1::2].
__global__ __launch_bounds__(256) void pack_act_s2_kernel(const float* __restrict__ x, int C, int W, int Ho, int Wo,
                                                          size_t img_stride, long long npix, int cw64,
                                                          uint64_t* __restrict__ P, uint64_t* __restrict__ M,
                                                          size_t set_stride, const float* __restrict__ bn_a,
                                                          const float* __restrict__ bn_b, int relu) {
  const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
  if (q >= npix) return;
  const int g = blockIdx.y;
  const int HWo = Ho * Wo;
  const size_t HW = (size_t)4 * HWo;
  const auto [n, r, i, j] = out_pixel(q, HWo, Wo);
  const float* xb = x + (size_t)n * img_stride + (size_t)(2 * i) * W + 2 * j;
  uint32_t pw[2][2] = {{0u, 0u}, {0u, 0u}}, mw[2][2] = {{0u, 0u}, {0u, 0u}};  // [phase][half]
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int c0 = g * 64 + h * 32;
    for (int b = 0; b < 32 && c0 + b < C; ++b) {
      const float* xc = xb + (size_t)(c0 + b) * HW;
      const float v[2] = {load_once(xc), load_once(xc + W + 1)};
      const Affine f = channel_affine(bn_a, bn_b, c0 + b);
#pragma unroll
      for (int ph = 0; ph < 2; ++ph) {
        const float u = f(v[ph]);
        pw[ph][h] = with_p(pw[ph][h], u, b);
        mw[ph][h] = with_m(mw[ph][h], u, b, relu);
      }
    }
  }
  const size_t o = word_off(n, cw64, g, HWo, r);
#pragma unroll
  for (int ph = 0; ph < 2; ++ph) {
    P[ph * set_stride + o] = join_halves(pw[ph][0], pw[ph][1]);
    M[ph * set_stride + o] = join_halves(mw[ph][0], mw[ph][1]);
  }
}

// H and W even (capi.hip has checked that and the view).
int launch_bn_act_pack_s2(const float* x, int c_off, int c_tot, int N, int C, int H, int W, const float* bn_a,
                          const float* bn_b, int relu, uint64_t* P, uint64_t* M, hipStream_t stream) {
  const int Ho = H / 2, Wo = W / 2;
  const long long npix = (long long)N * Ho * Wo;
  const int cw64 = (C + 63) / 64;
  hipLaunchKernelGGL(pack_act_s2_kernel, stream_grid(npix, cw64), dim3(256), 0, stream, x + (size_t)c_off * H * W, C, W,
                     Ho, Wo, (size_t)c_tot * H * W, npix, cw64, P, M, plane_set_stride(npix, cw64), bn_a, bn_b, relu);
  return launch_status();
}

// AvgPool2d(k, stride=k, ceil_mode=True, count_include_pad=False) + sign() in one pass: the
// shortcut branch of a down-sampling stage (bnn/models/resnet.py:128-133).  The planes are those
// of the AVERAGE, s / count over the in-image taps of the window, not of the sum s: the two
// differ where the average underflows to zero (one 2^-149 among zeros: s > 0, s / 4 == 0, and the
// reference's sign is 0).  Clipped windows at the ragged edge skip their out-of-image taps and
// divide by the taps they kept.
// One thread = one output pixel x one 32-channel word.
__global__ __launch_bounds__(256) void avgpool_pack_kernel(const float* __restrict__ x, int C, int H, int W, int k, int Ho,
                                                           int Wo, long long npix_out, int cw32,
                                                           uint32_t* __restrict__ P, uint32_t* __restrict__ M) {
  const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
  if (q >= npix_out) return;
  const int word = blockIdx.y;
  const int hw = Ho * Wo;
  const auto [n, r, oy, ox] = out_pixel(q, hw, Wo);
  uint32_t pw = 0u, mw = 0u;
  for (int b = 0; b < 32; ++b) {
    const int c = word * 32 + b;
    if (c >= C) break;
    const float* xc = x + ((size_t)n * C + c) * H * W;
    float s = 0.0f;
    int cnt = 0;
    for (int dy = 0; dy < k; ++dy) {
      const int iy = oy * k + dy;
      if (iy >= H) break;
      for (int dx = 0; dx < k; ++dx) {
        const int ix = ox * k + dx;
        if (ix >= W) break;
        s += xc[(size_t)iy * W + ix];
        ++cnt;
      }
    }
    const float t = s / (float)cnt;  // (IEEE division: hipcc's default for fp32)
    pw = with_p(pw, t, b);
    mw = with_m(mw, t, b);
  }
  const size_t o = half_off(n, cw32, word, hw, r);
  P[o] = pw;
  M[o] = mw;
}

// The same shortcut input when the tensor is NON-NEGATIVE (a ReLU output — every ResNet stage transition) and its
// sign planes already exist: an average of non-negative values is positive iff one of them is (unless it underflows,
// below), so
//     sign(AvgPool_k(x)) = OR over the k x k window of the P plane,   M = 0,
// computed from 2 bits per element instead of re-reading the fp32 tensor (206 MB -> 6.4 MB for the 64-channel
// 56x56 stage at batch 256: 38 us -> launch-bound).  Exact for finite inputs whose window average does not underflow to
// zero (a sum of non-negative floats is positive iff a term is, but the planes hold no magnitudes: a window whose sum is
// below count * 2^-150 averages to 0 in the reference and still ORs to 1); a NaN element makes the reference's average
// NaN (sign 0) while the OR ignores it.
__global__ __launch_bounds__(256) void orpool_packed_kernel(const uint64_t* __restrict__ P, int H, int W, int k,
                                                            int Ho, int Wo, long long nwords,
                                                            uint64_t* __restrict__ outP,
                                                            uint64_t* __restrict__ outM) {
  const long long q = (long long)blockIdx.x * 256 + threadIdx.x;  // (n * cw64 + g, oy, ox)
  if (q >= nwords) return;
  const int hw = Ho * Wo;
  const long long plane = q / hw;
  const int r = (int)(q - plane * hw);
  const int oy = r / Wo, ox = r - oy * Wo;
  const uint64_t* src = P + plane * H * W;
  uint64_t acc = 0;
  for (int dy = 0; dy < k; ++dy) {
    const int iy = oy * k + dy;
    if (iy >= H) break;
    for (int dx = 0; dx < k; ++dx) {
      const int ix = ox * k + dx;
      if (ix >= W) break;
      acc |= src[(size_t)iy * W + ix];
    }
  }
  outP[q] = acc;
  outM[q] = 0;
}

int launch_orpool_packed(const uint64_t* P, int N, int C, int H, int W, int k, uint64_t* outP, uint64_t* outM,
                         hipStream_t stream) {
  const int Ho = (H + k - 1) / k, Wo = (W + k - 1) / k;
  const long long nwords = (long long)N * ((C + 63) / 64) * Ho * Wo;
  hipLaunchKernelGGL(orpool_packed_kernel, dim3((unsigned)((nwords + 255) / 256)), dim3(256), 0, stream, P, H, W, k,
                     Ho, Wo, nwords, outP, outM);
  return launch_status();
}

// k == 2 on even images with W % 4 == 0 (every ResNet stage transition): one thread produces two
// adjacent outputs from one aligned float4 per input row.  Same tap order as the scalar kernel.
__global__ __launch_bounds__(256) void avgpool2_pack_kernel(const float* __restrict__ x, int C, int H, int W, int Ho,
                                                            int Wo, long long npairs, int cw32,
                                                            uint32_t* __restrict__ P, uint32_t* __restrict__ M) {
  const long long q = (long long)blockIdx.x * 256 + threadIdx.x;  // (n, oy, ox/2)
  if (q >= npairs) return;
  const int word = blockIdx.y;
  const int wp = Wo >> 1;
  const auto [n, rr, oy, t] = out_pixel(q, (long long)Ho * wp, wp);  // t: the pair in its row
  const int hw = Ho * Wo;
  const int r = oy * Wo + 2 * t;
  uint32_t pw0 = 0u, mw0 = 0u, pw1 = 0u, mw1 = 0u;
  for (int b = 0; b < 32; ++b) {
    const int c = word * 32 + b;
    if (c >= C) break;
    const float* row = x + (((size_t)n * C + c) * H + 2 * oy) * W + 4 * t;
    const float4 u = *reinterpret_cast<const float4*>(row);
    const float4 v = *reinterpret_cast<const float4*>(row + W);
    const float s0 = avg2x2(u.x, u.y, v.x, v.y), s1 = avg2x2(u.z, u.w, v.z, v.w);
    pw0 = with_p(pw0, s0, b);
    mw0 = with_m(mw0, s0, b);
    pw1 = with_p(pw1, s1, b);
    mw1 = with_m(mw1, s1, b);
  }
  const size_t o = half_off(n, cw32, word, hw, r);
  P[o] = pw0; M[o] = mw0;
  P[o + 2] = pw1; M[o + 2] = mw1;
}

// k == 2 on even images whose width is not a multiple of 4 (14x14 -> 7x7): one aligned float2 per
// input row and output.  Same tap order as the scalar kernel.
__global__ __launch_bounds__(256) void avgpool2_pack_f2_kernel(const float* __restrict__ x, int C, int H, int W, int Ho,
                                                               int Wo, long long npix_out, int cw32,
                                                               uint32_t* __restrict__ P, uint32_t* __restrict__ M) {
  const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
  if (q >= npix_out) return;
  const int word = blockIdx.y;
  const int hw = Ho * Wo;
  const auto [n, r, oy, ox] = out_pixel(q, hw, Wo);
  uint32_t pw = 0u, mw = 0u;
  const float* base = x + (((size_t)n * C + (size_t)word * 32) * H + 2 * oy) * W + 2 * ox;
  const size_t cstride = (size_t)H * W;
#pragma unroll 8
  for (int b = 0; b < 32; ++b) {
    if (word * 32 + b >= C) break;
    const float2 u = *reinterpret_cast<const float2*>(base + b * cstride);
    const float2 v = *reinterpret_cast<const float2*>(base + b * cstride + W);
    const float s = avg2x2(u.x, u.y, v.x, v.y);
    pw = with_p(pw, s, b);
    mw = with_m(mw, s, b);
  }
  const size_t o = half_off(n, cw32, word, hw, r);
  P[o] = pw;
  M[o] = mw;
}

int launch_avgpool_pack(const float* x, int N, int C, int H, int W, int k, uint64_t* P, uint64_t* M,
                        hipStream_t stream) {
  const int Ho = (H + k - 1) / k, Wo = (W + k - 1) / k;
  const long long npix = (long long)N * Ho * Wo;
  const int cw32 = 2 * ((C + 63) / 64);
  if (k == 2 && H % 2 == 0 && W % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15u) == 0) {
    const long long npairs = npix / 2;
    hipLaunchKernelGGL(avgpool2_pack_kernel, stream_grid(npairs, cw32),
                       dim3(256), 0, stream, x, C, H, W, Ho, Wo, npairs, cw32,
                       reinterpret_cast<uint32_t*>(P), reinterpret_cast<uint32_t*>(M));
    return launch_status();
  }
  if (k == 2 && H % 2 == 0 && W % 2 == 0 && (reinterpret_cast<uintptr_t>(x) & 7u) == 0) {
    hipLaunchKernelGGL(avgpool2_pack_f2_kernel, stream_grid(npix, cw32),
                       dim3(256), 0, stream, x, C, H, W, Ho, Wo, npix, cw32,
                       reinterpret_cast<uint32_t*>(P), reinterpret_cast<uint32_t*>(M));
    return launch_status();
  }
  hipLaunchKernelGGL(avgpool_pack_kernel, stream_grid(npix, cw32),
                     dim3(256), 0, stream, x, C, H, W, k, Ho, Wo, npix, cw32,
                     reinterpret_cast<uint32_t*>(P), reinterpret_cast<uint32_t*>(M));
  return launch_status();
}

// AvgPool2d(2, 2) in front of a pre-activation stage + the sign planes of up to TWO BatchNorm branches of its result in one
// pass (a hierarchical-block stage behind a pool, bnn_amd/models/resnet.py: the block's bn1 -> act -> conv1 and its
// shortcut's bn -> conv1x1 both binarise the pooled tensor):
//     t  = avg2x2(x00, x01, x10, x11)             ATen's avg_pool2d (planes.h)
//     u1 = fmaf(t, a1[c], b1[c]) -> P1 / M1 (relu1: M1 = 0);   u2 = fmaf(t, a2[c], b2[c]) -> P2 / M2
// The fp32 tensor t is written only when `out` is given (nobody reads it when both consumers take planes).
// A workgroup = 64 consecutive output pixels x one 32-channel word; wave w of it = channels 8w .. 8w+7 of the word (lane =
// pixel: coalesced float2 loads, 16 in flight per lane); the four 8-bit pieces meet in LDS.  Even H and W.
// (large tensors — the 56x56 -> 28x28 transition at batch 128 — stream at 4.9 TB/s in the one-thread-per-word form below;
// this one is for the smaller transitions, where that form has too few threads: 19.4 -> 14.3 us and 18.4 -> 11.0 us)
// One channel of both forms: tap = the window's first element; bit b of the four words; t goes to out[o] when `store`.
struct Bn2Words {
  uint32_t p1, m1, p2, m2;
};
__device__ __forceinline__ Bn2Words pool_bn2_channel(Bn2Words w, const float* tap, int W, int c, int b, const float* a1,
                                                     const float* b1, int relu1, const float* a2, const float* b2,
                                                     int relu2, bool store, float* out, size_t o) {
  const float2 u = *reinterpret_cast<const float2*>(tap);
  const float2 v = *reinterpret_cast<const float2*>(tap + W);
  const float t = avg2x2(u.x, u.y, v.x, v.y);
  if (store) out[o] = t;
  const float u1 = fmaf(t, a1[c], b1[c]);
  w.p1 = with_p(w.p1, u1, b);
  w.m1 = with_m(w.m1, u1, b, relu1);
  if (a2) {
    const float u2 = fmaf(t, a2[c], b2[c]);
    w.p2 = with_p(w.p2, u2, b);
    w.m2 = with_m(w.m2, u2, b, relu2);
  }
  return w;
}

__global__ __launch_bounds__(256) void avgpool2_bn_pack2_kernel(
    const float* __restrict__ x, int C, int H, int W, int Ho, int Wo, long long npix_out, int cw32,
    const float* __restrict__ a1, const float* __restrict__ b1, int relu1, uint32_t* __restrict__ P1,
    uint32_t* __restrict__ M1, const float* __restrict__ a2, const float* __restrict__ b2, int relu2,
    uint32_t* __restrict__ P2, uint32_t* __restrict__ M2, float* __restrict__ out) {
  __shared__ uint32_t pieces[4][64];  // [plane][pixel]: byte w = the piece of wave w
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long q0 = (long long)blockIdx.x * 64 + lane;
  const long long q = q0 < npix_out ? q0 : npix_out - 1;  // lanes past the end copy the last pixel (nothing stored)
  const int word = blockIdx.y;
  const int hw = Ho * Wo;
  const auto [n, r, oy, ox] = out_pixel(q, hw, Wo);
  if (wv == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) pieces[k][lane] = 0u;
  }
  __syncthreads();
  Bn2Words w = {0u, 0u, 0u, 0u};
  const int c0 = word * 32 + wv * 8;
  const float* base = x + (((size_t)n * C + (size_t)c0) * H + 2 * oy) * W + 2 * ox;
  const size_t cstride = (size_t)H * W;
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const int c = c0 + b;
    if (c >= C) break;
    w = pool_bn2_channel(w, base + b * cstride, W, c, b, a1, b1, relu1, a2, b2, relu2, out && q0 < npix_out, out,
                         ((size_t)n * C + c) * hw + r);
  }
  unsigned char* pb = reinterpret_cast<unsigned char*>(&pieces[0][0]);
  pb[(0 * 64 + lane) * 4 + wv] = (unsigned char)w.p1;
  pb[(1 * 64 + lane) * 4 + wv] = (unsigned char)w.m1;
  pb[(2 * 64 + lane) * 4 + wv] = (unsigned char)w.p2;
  pb[(3 * 64 + lane) * 4 + wv] = (unsigned char)w.m2;
  __syncthreads();
  if (wv == 0 && q0 < npix_out) {
    const size_t o = half_off(n, cw32, word, hw, r);
    P1[o] = pieces[0][lane];
    M1[o] = pieces[1][lane];
    if (a2) {
      P2[o] = pieces[2][lane];
      M2[o] = pieces[3][lane];
    }
  }
}

// One thread = one output pixel x one 32-channel word.
__global__ __launch_bounds__(256) void avgpool2_bn_pack2_wide_kernel(
    const float* __restrict__ x, int C, int H, int W, int Ho, int Wo, long long npix_out, int cw32,
    const float* __restrict__ a1, const float* __restrict__ b1, int relu1, uint32_t* __restrict__ P1,
    uint32_t* __restrict__ M1, const float* __restrict__ a2, const float* __restrict__ b2, int relu2,
    uint32_t* __restrict__ P2, uint32_t* __restrict__ M2, float* __restrict__ out) {
  const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
  if (q >= npix_out) return;
  const int word = blockIdx.y;
  const int hw = Ho * Wo;
  const auto [n, r, oy, ox] = out_pixel(q, hw, Wo);
  Bn2Words w = {0u, 0u, 0u, 0u};
  const float* base = x + (((size_t)n * C + (size_t)word * 32) * H + 2 * oy) * W + 2 * ox;
  const size_t cstride = (size_t)H * W;
#pragma unroll 8
  for (int b = 0; b < 32; ++b) {
    const int c = word * 32 + b;
    if (c >= C) break;
    w = pool_bn2_channel(w, base + b * cstride, W, c, b, a1, b1, relu1, a2, b2, relu2, out != nullptr, out,
                         ((size_t)n * C + c) * hw + r);
  }
  const size_t o = half_off(n, cw32, word, hw, r);
  P1[o] = w.p1;
  M1[o] = w.m1;
  if (a2) {
    P2[o] = w.p2;
    M2[o] = w.m2;
  }
}

int launch_avgpool2_bn_pack2(const float* x, int N, int C, int H, int W, const float* a1, const float* b1, int relu1,
                             uint64_t* P1, uint64_t* M1, const float* a2, const float* b2, int relu2, uint64_t* P2,
                             uint64_t* M2, float* out, hipStream_t stream) {
  const int Ho = H / 2, Wo = W / 2;
  const long long npix = (long long)N * Ho * Wo;
  const int cw32 = 2 * ((C + 63) / 64);
  if (npix * cw32 >= 150000LL) {  // enough threads to fill the chip with one per (pixel, word)
    hipLaunchKernelGGL(avgpool2_bn_pack2_wide_kernel, stream_grid(npix, cw32), dim3(256), 0,
                       stream, x, C, H, W, Ho, Wo, npix, cw32, a1, b1, relu1, reinterpret_cast<uint32_t*>(P1),
                       reinterpret_cast<uint32_t*>(M1), a2, b2, relu2, reinterpret_cast<uint32_t*>(P2),
                       reinterpret_cast<uint32_t*>(M2), out);
    return launch_status();
  }
  hipLaunchKernelGGL(avgpool2_bn_pack2_kernel, dim3((unsigned)((npix + 63) / 64), (unsigned)cw32), dim3(256), 0, stream,
                     x, C, H, W, Ho, Wo, npix, cw32, a1, b1, relu1, reinterpret_cast<uint32_t*>(P1),
                     reinterpret_cast<uint32_t*>(M1), a2, b2, relu2, reinterpret_cast<uint32_t*>(P2),
                     reinterpret_cast<uint32_t*>(M2), out);
  return launch_status();
}

// Tail of the real-valued stem in ONE pass over the stem conv's output
// (bnn/models/resnet.py:150-153: bn1 -> relu -> maxpool, then the first binary conv's sign()):
//     v = fma(x, bn_a[c], bn_b[c])   eval-mode BatchNorm (optional)
//     m = max over the k x k window (padding taps ignored, like nn.MaxPool2d)
//     y = relu(m)                    relu and max commute, so ReLU runs once per output
//     out_f32 = y ; P/M = sign(y)
// Reads the big tensor once (HBM-bound) instead of four times (BN, ReLU, pool, pack).
// One thread = one output pixel x one 32-channel word; consecutive lanes = consecutive ox, so
// fp32 stores are coalesced and the stride-2 window reads of neighbouring lanes share lines.
__global__ __launch_bounds__(256) void bn_relu_maxpool_pack_kernel(
    const float* __restrict__ x, int C, int H, int W, const float* __restrict__ bn_a,
    const float* __restrict__ bn_b, int relu, int k, int stride, int pad, int Ho, int Wo,
    long long npix_out, int cw32, float* __restrict__ out, uint32_t* __restrict__ P,
    uint32_t* __restrict__ M) {
  const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
  if (q >= npix_out) return;
  const int word = blockIdx.y;
  const int hw = Ho * Wo;
  const auto [n, r, oy, ox] = out_pixel(q, hw, Wo);
  const int y0 = oy * stride - pad, x0 = ox * stride - pad;
  uint32_t pw = 0u, mw = 0u;
  for (int b = 0; b < 32; ++b) {
    const int c = word * 32 + b;
    if (c >= C) break;
    const float* xc = x + ((size_t)n * C + c) * H * W;
    const float a = bn_a ? bn_a[c] : 1.0f, sh = bn_b ? bn_b[c] : 0.0f;
    float m = -INFINITY;
    for (int dy = 0; dy < k; ++dy) {
      const int iy = y0 + dy;
      if ((unsigned)iy >= (unsigned)H) continue;
      for (int dx = 0; dx < k; ++dx) {
        const int ix = x0 + dx;
        if ((unsigned)ix >= (unsigned)W) continue;
        m = fmaxf(m, fmaf(xc[(size_t)iy * W + ix], a, sh));
      }
    }
    if (relu) m = fmaxf(m, 0.0f);
    if (out) out[((size_t)n * C + c) * hw + r] = m;
    pw = with_p(pw, m, b);
    mw = with_m(mw, m, b);
  }
  if (P) {
    const size_t o = half_off(n, cw32, word, hw, r);
    P[o] = pw;
    M[o] = mw;
  }
}

// The ResNet stem's geometry (3x3 window, stride 2, pad 1, W % 4 == 0) with vector loads: one
// thread produces TWO horizontally adjacent outputs from one aligned float4 + one scalar per
// input row, i.e. 6 loads per channel for 2 outputs instead of 18 stride-2 dword loads.
__global__ __launch_bounds__(256) void bn_relu_maxpool3s2_pack_kernel(
    const float* __restrict__ x, int C, int H, int W, const float* __restrict__ bn_a,
    const float* __restrict__ bn_b, int relu, int Ho, int Wo, long long npairs, int cw32,
    float* __restrict__ out, uint32_t* __restrict__ P, uint32_t* __restrict__ M) {
  const long long q = (long long)blockIdx.x * 256 + threadIdx.x;  // (n, oy, ox/2)
  if (q >= npairs) return;
  const int word = blockIdx.y;
  const int wp = Wo >> 1;
  const auto [n, rr, oy, t] = out_pixel(q, (long long)Ho * wp, wp);  // t: the pair in its row
  const int hw = Ho * Wo;
  const int r = oy * Wo + 2 * t;
  uint32_t pw0 = 0u, mw0 = 0u, pw1 = 0u, mw1 = 0u;
  for (int b = 0; b < 32; ++b) {
    const int c = word * 32 + b;
    if (c >= C) break;
    const float* xc = x + ((size_t)n * C + c) * H * W;
    const float a = bn_a ? bn_a[c] : 1.0f, sh = bn_b ? bn_b[c] : 0.0f;
    float m0 = -INFINITY, m1 = -INFINITY;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
      const int iy = 2 * oy - 1 + dy;
      if ((unsigned)iy < (unsigned)H) {
        const float* row = xc + (size_t)iy * W + 4 * t;
        const float4 v = *reinterpret_cast<const float4*>(row);
        const float e = t > 0 ? fmaf(row[-1], a, sh) : -INFINITY;
        const float v0 = fmaf(v.x, a, sh), v1 = fmaf(v.y, a, sh), v2 = fmaf(v.z, a, sh),
                    v3 = fmaf(v.w, a, sh);
        m0 = fmaxf(m0, fmaxf(e, fmaxf(v0, v1)));
        m1 = fmaxf(m1, fmaxf(v1, fmaxf(v2, v3)));
      }
    }
    if (relu) { m0 = fmaxf(m0, 0.0f); m1 = fmaxf(m1, 0.0f); }
    if (out) *reinterpret_cast<float2*>(out + ((size_t)n * C + c) * hw + r) = make_float2(m0, m1);
    pw0 = with_p(pw0, m0, b);
    mw0 = with_m(mw0, m0, b);
    pw1 = with_p(pw1, m1, b);
    mw1 = with_m(mw1, m1, b);
  }
  if (P) {
    const size_t o = half_off(n, cw32, word, hw, r);
    P[o] = pw0; M[o] = mw0;
    P[o + 2] = pw1; M[o + 2] = mw1;
  }
}

int launch_bn_relu_maxpool_pack(const float* x, int N, int C, int H, int W, const float* bn_a,
                                const float* bn_b, int relu, int k, int stride, int pad, float* out,
                                uint64_t* P, uint64_t* M, hipStream_t stream) {
  const int Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
  const long long npix = (long long)N * Ho * Wo;
  const int cw32 = 2 * ((C + 63) / 64);
  if (k == 3 && stride == 2 && pad == 1 && W % 4 == 0 && Wo == W / 2 &&
      (reinterpret_cast<uintptr_t>(x) & 15u) == 0 &&
      (!out || (reinterpret_cast<uintptr_t>(out) & 7u) == 0)) {
    const long long npairs = npix / 2;
    hipLaunchKernelGGL(bn_relu_maxpool3s2_pack_kernel,
                       stream_grid(npairs, cw32), dim3(256), 0, stream, x,
                       C, H, W, bn_a, bn_b, relu, Ho, Wo, npairs, cw32, out,
                       reinterpret_cast<uint32_t*>(P), reinterpret_cast<uint32_t*>(M));
    return launch_status();
  }
  hipLaunchKernelGGL(bn_relu_maxpool_pack_kernel,
                     stream_grid(npix, cw32), dim3(256), 0, stream, x, C,
                     H, W, bn_a, bn_b, relu, k, stride, pad, Ho, Wo, npix, cw32, out,
                     reinterpret_cast<uint32_t*>(P), reinterpret_cast<uint32_t*>(M));
  return launch_status();
}

}  // namespace bnn

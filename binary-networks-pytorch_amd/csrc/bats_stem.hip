// bats_stem.hip — the real-valued CIFAR stem of a BATS network and the binarisation of its consumers in ONE launch.
//
// Replaces bnn/models/bats.py:118-122 (stem = Conv2d(3, 3C, 3, padding=1, bias=False) -> BatchNorm2d -> ReLU) followed by
// the BatchNorm + sign() of every ReLUConvBN that reads the stem output (bnn/models/layers/bats_ops.py:78-105:
// cells[0].preprocess0, cells[0].preprocess1, cells[1].preprocess0).  The reference writes the fp32 [N, 3C, H, W] tensor
// and reads it once per consumer; here it stays in registers and leaves the kernel as K <= 4 sets of bit planes (2 bits
// per element and consumer), and as fp32 only when somebody asks for it.
//
// The arithmetic is fixed (tests restate it):
//     acc = 0.0f;  for c, kh, kw (in that order):  acc = fmaf(x[n, c, y + kh - 1, x + kw - 1], w[o, c, kh, kw], acc)
//     y   = fmaxf(fmaf(acc, s[o], t[o]), 0.0f)
//     u_k = fmaf(y, a[k][o], b[k][o]);   P bit = p_bit(u_k), M bit = m_bit(u_k)        (planes.h; pack_act_multi_kernel, relu = 0)
// A padding tap enters as x = 0.0f: for a finite weight the fmaf returns acc unchanged (acc is never -0.0f: it starts at
// +0.0f), so padding taps contribute nothing; for a non-finite weight it is the NaN the reference's zero padding gives.
//
// Mapping: as pack_act_multi_kernel — one thread owns VP consecutive pixels of one image and ONE 64-channel group
// (blockIdx.y).  The 27 VP inputs of its pixels sit in registers for the whole kernel (x is 12 bytes per pixel and comes
// out of the cache: every pixel is read by 9 neighbours and by every channel group); the 27 weights, the BatchNorm and the
// 2 K affine constants of a channel are the same for the whole wave, so they are scalar loads; every lane shifts its
// 64-channel words together and stores VP contiguous uint64 per plane, coalesced across the lanes.
#include "planes.h"

namespace bnn {

template <int VP, int K>
__global__ __launch_bounds__(256) void stem3x3_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                      const float* __restrict__ bn_s, const float* __restrict__ bn_t,
                                                      const float* __restrict__ pk_a, const float* __restrict__ pk_b,
                                                      int O, int H, int W, long long npix, int cw64,
                                                      uint64_t* __restrict__ P, uint64_t* __restrict__ M,
                                                      size_t set_stride, float* __restrict__ y) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long pix0 = t * VP;
  if (pix0 >= npix) return;
  const int HW = H * W;
  const int g = blockIdx.y;
  const int n = (int)(pix0 / HW);
  const int r = (int)(pix0 - (long long)n * HW);   // (HW is a multiple of VP: the VP pixels are in image n)
  const float* xn = x + (size_t)n * 3 * HW;

  // the receptive fields: in[v][c * 9 + kh * 3 + kw], padding taps 0.0f (the load of one reads pixel 0 and is dropped)
  float in[VP][27];
#pragma unroll
  for (int v = 0; v < VP; ++v) {
    const int py = (r + v) / W, px = (r + v) - py * W;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
      for (int kh = 0; kh < 3; ++kh) {
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          const int yy = py + kh - 1, xx = px + kw - 1;
          const bool inb = (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
          const float val = xn[inb ? (c * H + yy) * W + xx : 0];
          in[v][c * 9 + kh * 3 + kw] = inb ? val : 0.0f;
        }
      }
    }
  }

  // one output channel for the thread's VP pixels: y stays in registers (yv) and is stored when asked for
  auto channel = [&](int c, float (&yv)[VP]) {
    const float* wo = w + (size_t)c * 27;
    float acc[VP];
#pragma unroll
    for (int v = 0; v < VP; ++v) acc[v] = 0.0f;
#pragma unroll
    for (int j = 0; j < 27; ++j) {
      const float wj = wo[j];
#pragma unroll
      for (int v = 0; v < VP; ++v) acc[v] = fmaf(in[v][j], wj, acc[v]);
    }
    const float s = bn_s[c], sh = bn_t[c];
#pragma unroll
    for (int v = 0; v < VP; ++v) yv[v] = fmaxf(fmaf(acc[v], s, sh), 0.0f);
    if (y) {
      PixVec<float, VP> out;
#pragma unroll
      for (int v = 0; v < VP; ++v) out.v[v] = yv[v];
      *reinterpret_cast<PixVec<float, VP>*>(y + ((size_t)n * O + c) * HW + r) = out;
    }
  };

  uint32_t pw[K][2][VP], mw[K][2][VP];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
      for (int v = 0; v < VP; ++v) { pw[k][h][v] = 0u; mw[k][h][v] = 0u; }
    }
    const int c0 = g * 64 + h * 32;
    if (c0 + 32 <= O) {
#pragma unroll 2
      for (int b = 31; b >= 0; --b) {  // high -> low: shifting left leaves channel c0 + b in bit b
        float yv[VP];
        channel(c0 + b, yv);
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const float ca = pk_a[(size_t)k * O + c0 + b], cb = pk_b[(size_t)k * O + c0 + b];
#pragma unroll
          for (int v = 0; v < VP; ++v) {
            const float u = fmaf(yv[v], ca, cb);
            pw[k][h][v] = with_p<kShiftIn>(pw[k][h][v], u, b);
            mw[k][h][v] = with_m<kShiftIn>(mw[k][h][v], u, b);
          }
        }
      }
    } else {
      for (int b = 0; b < 32 && c0 + b < O; ++b) {
        float yv[VP];
        channel(c0 + b, yv);
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const float ca = pk_a[(size_t)k * O + c0 + b], cb = pk_b[(size_t)k * O + c0 + b];
#pragma unroll
          for (int v = 0; v < VP; ++v) {
            const float u = fmaf(yv[v], ca, cb);
            pw[k][h][v] = with_p<kOrAt>(pw[k][h][v], u, b);
            mw[k][h][v] = with_m<kOrAt>(mw[k][h][v], u, b);
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

// capi.hip has checked the pointers, 1 <= K <= 4, the sizes and ceil(O / 64) <= 65535 (grid.y).
int launch_stem3x3_bn_relu_pack(const float* x, const float* w, const float* bn_s, const float* bn_t, const float* pk_a,
                                const float* pk_b, int N, int O, int H, int W, int K, uint64_t* P, uint64_t* M, float* y,
                                hipStream_t stream) {
  const long long npix = (long long)N * H * W;
  const int cw64 = (O + 63) / 64;
  with_k(K, [&](auto kc) {
    constexpr int KV = decltype(kc)::value;
    // pixels per thread: as many as HW and the alignment of y allow (y is stored as one VP-float vector per channel;
    // a null y is not written), and 4 K VP plane words per thread: VP = 4 up to K = 2
    with_width<(KV <= 2 ? 4 : 2)>(H * W, y, sizeof(float), [&](auto vp) {
      constexpr int VP = decltype(vp)::value;
      hipLaunchKernelGGL((stem3x3_kernel<VP, KV>), stream_grid(npix / VP, cw64), dim3(256), 0, stream, x, w, bn_s, bn_t, pk_a,
                         pk_b, O, H, W, npix, cw64, P, M, plane_set_stride(npix, cw64), y);
    });
  });
  return launch_status();
}

}  // namespace bnn

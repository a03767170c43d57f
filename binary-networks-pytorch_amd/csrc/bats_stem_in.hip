// bats_stem_in.hip — the two real-valued stems of a BATS ImageNet network, one launch each.
//
// Replaces bnn/models/bats.py:161-172:
//     stem0 = Conv2d(3, C1, 3, stride 2, pad 1) -> BatchNorm -> ReLU -> Conv2d(C1, C, 3, stride 2, pad 1, groups G) -> BatchNorm
//     stem1 = ReLU -> Conv2d(C, C, 3, stride 2, pad 1, groups G) -> BatchNorm
// followed by the BatchNorm + sign() of the ReLUConvBN preprocessors that read stem1's output.  The reference writes the
// [N, C1, H/2, W/2] intermediate of stem0 three times and reads it once; here it lives in LDS, per output tile.
//
// The arithmetic is fixed (tests restate it).  With H1 = (H + 1) / 2, H2 = (H1 + 1) / 2 (W alike), Cig input and Cog output
// channels per group, g = o / Cog:
//   (a) stem_s2x2:
//     acc1 = 0.0f; for (ci, kh, kw) in that order: acc1 = fmaf(x[n, ci, 2p + kh - 1, 2q + kw - 1], w1[c, ci, kh, kw], acc1)
//     y1[n, c, p, q] = fmaxf(fmaf(acc1, s1[c], t1[c]), 0.0f)                                   for (p, q) in H1 x W1
//     acc2 = 0.0f; for (j, kh, kw) in that order:
//                      acc2 = fmaf(y1[n, g Cig + j, 2p + kh - 1, 2q + kw - 1], w2[o, j, kh, kw], acc2)
//     y[n, o, p, q] = fmaf(acc2, s2[o], t2[o]), then fmaxf(., 0.0f) when relu_out                  for (p, q) in H2 x W2
//   (b) gconv3x3s2_bn_pack:  x' = relu_in ? fmaxf(x, 0.0f) : x
//     acc = 0.0f; for (j, kh, kw) in that order: acc = fmaf(x'[n, g Cig + j, 2p + kh - 1, 2q + kw - 1], w[o, j, kh, kw], acc)
//     y[n, o, p, q] = fmaf(acc, s[o], t[o])
//     u_k = fmaf(y, a[k][o], b[k][o]);  P bit = is_pos(u_k), M bit = is_neg(u_k)               (pack_act_multi_kernel, relu = 0)
// A tap outside the image enters as 0.0f: for a finite weight the fmaf returns the accumulator unchanged (it is never
// -0.0f: it starts at +0.0f), so the tap contributes nothing.  A tap of the SECOND convolution of (a) outside the H1 x W1
// map is such a padding tap too: the tile of y1 holds 0.0f there, never the max(t1, 0) the first convolution would give.
//
// Mapping.  A workgroup of four waves owns one image and one kTH x kTW tile of output pixels (a lane per pixel), and
//   (a) one convolution group: it stages the 19 x 67 x 3 window of x in LDS, computes its group's Cig channels of y1 on the
//       9 x 33 positions the tile reads (first convolution recomputed on the one-pixel halo only) into LDS, then the
//       group's Cog output channels, kChunk at a time per wave;
//   (b) one 64-channel plane word: it walks through the convolution groups the word spans, stages each group's Cig input
//       channels on the 9 x 33 window in LDS, and every wave computes kChunk output channels at a time and sets their bits
//       in its copy of the K plane words; the four copies are OR-ed through LDS and stored once.
// Both tiles are stored with even and odd columns apart, so that the stride-2 reads of a wave are consecutive words; the
// row strides put the two rows of a half-wave on disjoint banks.  Weights, BatchNorm and affine constants are indexed by
// wave-uniform values only, so they are scalar loads, as in bats_stem.hip.
#include "planes.h"

namespace bnn {

namespace {

constexpr int kTH = BNN_HIP_STEM_S2_TILE_H, kTW = BNN_HIP_STEM_S2_TILE_W;   // output tile: one wave's lanes
static_assert(kTH * kTW == kWave, "a lane per output pixel");
constexpr int kChunk = 5;                   // output channels a wave accumulates at once
// the tile a 3x3 / stride 2 convolution reads ("mid": y1 in (a), x' in (b)): kMR x kMC positions per channel; a row holds
// the even columns at [0, 17) and the odd ones at [kMO, kMO + 16)
constexpr int kMR = 2 * kTH + 1, kMC = 2 * kTW + 1, kMPos = kMR * kMC;
constexpr int kMO = 20, kMRS = 40, kMCS = kMR * kMRS;
// the window of x the first convolution of (a) reads for that tile: kXR x kXC per channel, even columns at [0, kXE)
constexpr int kXR = 2 * kMR + 1, kXC = 2 * kMC + 1, kXE = kMC + 1, kXRS = 68, kXCS = kXR * kXRS;
static_assert(kMO >= kTW + 1 && kMO + kTW <= kMRS && kXE + kMC <= kXRS, "the two column halves of a row do not overlap");

__device__ __forceinline__ int mid_off(int r, int c) { return r * kMRS + (c & 1) * kMO + (c >> 1); }

// acc[i] = the fmaf chain over (j, kh, kw) of output channel i of a chunk, for the pixel (py, px) of the tile.  `w` is the
// weight of the chunk's first channel ([.][Cig][3][3]); the chunk has nv <= kChunk channels (the others repeat the last).
__device__ __forceinline__ void gconv_chunk(const float* mid, int Cig, const float* __restrict__ w, int nv, int py, int px,
                                            float (&acc)[kChunk]) {
  const float* wp[kChunk];
#pragma unroll
  for (int i = 0; i < kChunk; ++i) {
    wp[i] = w + (size_t)(i < nv ? i : nv - 1) * Cig * 9;
    acc[i] = 0.0f;
  }
  const float* m = mid + 2 * py * kMRS + px;
  for (int j = 0; j < Cig; ++j, m += kMCS) {
    float v[9];
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      v[kh * 3 + 0] = m[kh * kMRS];
      v[kh * 3 + 1] = m[kh * kMRS + kMO];
      v[kh * 3 + 2] = m[kh * kMRS + 1];
    }
#pragma unroll
    for (int i = 0; i < kChunk; ++i) {
#pragma unroll
      for (int t = 0; t < 9; ++t) acc[i] = fmaf(v[t], wp[i][j * 9 + t], acc[i]);
    }
  }
}

}  // namespace

extern __shared__ __align__(16) float stem_in_smem[];

__global__ __launch_bounds__(256) void stem_s2x2_kernel(const float* __restrict__ x, const float* __restrict__ w1,
                                                        const float* __restrict__ s1, const float* __restrict__ t1,
                                                        const float* __restrict__ w2, const float* __restrict__ s2,
                                                        const float* __restrict__ t2, int Cig, int Cog, int C, int H, int W,
                                                        int H1, int W1, int H2, int W2, int tiles_w, int tiles, int relu_out,
                                                        float* __restrict__ y) {
  float* xt = stem_in_smem;                  // [3][kXR][kXRS]
  float* mid = stem_in_smem + 3 * kXCS;      // [Cig][kMR][kMRS]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = blockIdx.y;
  const int n = blockIdx.x / tiles, tl = blockIdx.x - n * tiles;
  const int p0 = (tl / tiles_w) * kTH, q0 = (tl % tiles_w) * kTW;

  // the window of x: rows 4 p0 - 3 .., columns 4 q0 - 3 .., 0.0f outside the image (the load of such a tap reads element 0)
  const float* xn = x + (size_t)n * 3 * H * W;
  for (int i = tid; i < 3 * kXR * kXC; i += 256) {
    const int ch = i / (kXR * kXC), rem = i - ch * (kXR * kXC), r = rem / kXC, c = rem - r * kXC;
    const int gy = 4 * p0 - 3 + r, gx = 4 * q0 - 3 + c;
    const bool inb = (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W;
    const float v = xn[inb ? ((size_t)ch * H + gy) * W + gx : 0];
    xt[ch * kXCS + r * kXRS + (c & 1) * kXE + (c >> 1)] = inb ? v : 0.0f;
  }
  __syncthreads();

  // y1 of the group on the tile's kMR x kMC positions: a wave takes 64 positions and kChunk channels at a time
  constexpr int kBlk = (kMPos + 63) / 64;
  const int items = kBlk * ((Cig + kChunk - 1) / kChunk);
  for (int it = wave; it < items; it += 4) {
    const int c0 = (it / kBlk) * kChunk;
    const int pos = (it % kBlk) * 64 + lane;
    const bool live = pos < kMPos;
    const int r = (live ? pos : 0) / kMC, c = (live ? pos : 0) - r * kMC;
    const int gr = 2 * p0 - 1 + r, gc = 2 * q0 - 1 + c;
    const bool inmap = (unsigned)gr < (unsigned)H1 && (unsigned)gc < (unsigned)W1;
    float in[27];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
#pragma unroll
      for (int kh = 0; kh < 3; ++kh) {
        const float* b = xt + ch * kXCS + (2 * r + kh) * kXRS + c;
        in[ch * 9 + kh * 3 + 0] = b[0];
        in[ch * 9 + kh * 3 + 1] = b[kXE];
        in[ch * 9 + kh * 3 + 2] = b[1];
      }
    }
    for (int i = 0; i < kChunk && c0 + i < Cig; ++i) {
      const int c1 = g * Cig + c0 + i;
      const float* wo = w1 + (size_t)c1 * 27;
      float acc = 0.0f;
#pragma unroll
      for (int t = 0; t < 27; ++t) acc = fmaf(in[t], wo[t], acc);
      const float v = fmaxf(fmaf(acc, s1[c1], t1[c1]), 0.0f);
      if (live) mid[(c0 + i) * kMCS + mid_off(r, c)] = inmap ? v : 0.0f;    // (outside the map: padding of the 2nd conv)
    }
  }
  __syncthreads();

  // the group's output channels for the tile
  const int py = lane >> 4, px = lane & (kTW - 1);
  const int p = p0 + py, q = q0 + px;
  const bool inside = p < H2 && q < W2;
  for (int ol = wave * kChunk; ol < Cog; ol += 4 * kChunk) {
    const int nv = Cog - ol < kChunk ? Cog - ol : kChunk;
    const int o0 = g * Cog + ol;
    float acc[kChunk];
    gconv_chunk(mid, Cig, w2 + (size_t)o0 * Cig * 9, nv, py, px, acc);
#pragma unroll
    for (int i = 0; i < kChunk; ++i) {
      if (i < nv) {
        const int o = o0 + i;
        float v = fmaf(acc[i], s2[o], t2[o]);
        if (relu_out) v = fmaxf(v, 0.0f);
        if (inside) y[(((size_t)n * C + o) * H2 + p) * W2 + q] = v;
      }
    }
  }
}

template <int K>
__global__ __launch_bounds__(256) void gconv3x3s2_pack_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                              const float* __restrict__ bn_s, const float* __restrict__ bn_t,
                                                              const float* __restrict__ pk_a, const float* __restrict__ pk_b,
                                                              int Cig, int Cog, int C, int O, int H, int W, int Ho, int Wo,
                                                              int tiles_w, int tiles, int relu_in, int cw64,
                                                              uint64_t* __restrict__ P, uint64_t* __restrict__ M,
                                                              size_t set_stride, float* __restrict__ y) {
  constexpr int KK = K > 0 ? K : 1;
  float* mid = stem_in_smem;                 // [Cig][kMR][kMRS]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wd = blockIdx.y;
  const int n = blockIdx.x / tiles, tl = blockIdx.x - n * tiles;
  const int p0 = (tl / tiles_w) * kTH, q0 = (tl % tiles_w) * kTW;
  const int py = lane >> 4, px = lane & (kTW - 1);
  const int p = p0 + py, q = q0 + px;
  const bool inside = p < Ho && q < Wo;
  const int o_lo = wd * 64, o_hi = O < o_lo + 64 ? O : o_lo + 64;

  uint64_t pw[KK], mw[KK];
#pragma unroll
  for (int k = 0; k < KK; ++k) { pw[k] = 0; mw[k] = 0; }
  int turn = 0;                              // chunks handed out so far: the next one goes to wave turn % 4
  // the word's channels lie in groups o_lo / Cog .. (o_hi - 1) / Cog: one after the other through the same tile
  for (int g = o_lo / Cog; g * Cog < o_hi; ++g) {
    if (g * Cog > o_lo) __syncthreads();     // (every wave is done with the previous group's tile)
    const float* xg = x + ((size_t)n * C + (size_t)g * Cig) * H * W;
    for (int i = tid; i < Cig * kMPos; i += 256) {
      const int j = i / kMPos, rem = i - j * kMPos, r = rem / kMC, c = rem - r * kMC;
      const int gy = 2 * p0 - 1 + r, gx = 2 * q0 - 1 + c;
      const bool inb = (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W;
      float v = xg[inb ? ((size_t)j * H + gy) * W + gx : 0];
      if (relu_in) v = fmaxf(v, 0.0f);
      mid[j * kMCS + mid_off(r, c)] = inb ? v : 0.0f;
    }
    __syncthreads();
    const int a_lo = g * Cog > o_lo ? g * Cog : o_lo, a_hi = (g + 1) * Cog < o_hi ? (g + 1) * Cog : o_hi;
    const int nchunk = (a_hi - a_lo + kChunk - 1) / kChunk;
    for (int ck = (wave - turn) & 3; ck < nchunk; ck += 4) {
      const int o0 = a_lo + ck * kChunk;
      const int nv = a_hi - o0 < kChunk ? a_hi - o0 : kChunk;
      float acc[kChunk];
      gconv_chunk(mid, Cig, w + (size_t)o0 * Cig * 9, nv, py, px, acc);
#pragma unroll
      for (int i = 0; i < kChunk; ++i) {
        if (i < nv) {
          const int o = o0 + i;
          const float v = fmaf(acc[i], bn_s[o], bn_t[o]);
          if (y && inside) y[(((size_t)n * O + o) * Ho + p) * Wo + q] = v;
#pragma unroll
          for (int k = 0; k < K; ++k) {
            const float u = fmaf(v, pk_a[(size_t)k * O + o], pk_b[(size_t)k * O + o]);
            pw[k] |= (uint64_t)p_bit(u) << (o & 63);
            mw[k] |= (uint64_t)m_bit(u) << (o & 63);
          }
        }
      }
    }
    turn += nchunk;
  }
  if constexpr (K > 0) {
    // OR the four waves' copies of the words: [wave][k][P | M][pixel] over the tile's LDS
    __syncthreads();
    uint64_t* comb = reinterpret_cast<uint64_t*>(stem_in_smem);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      comb[((wave * K + k) * 2 + 0) * 64 + lane] = pw[k];
      comb[((wave * K + k) * 2 + 1) * 64 + lane] = mw[k];
    }
    __syncthreads();
    for (int i = tid; i < K * 2 * 64; i += 256) {
      const int k = i >> 7, pm = (i >> 6) & 1, ln = i & 63;
      uint64_t v = 0;
#pragma unroll
      for (int wv = 0; wv < 4; ++wv) v |= comb[((wv * K + k) * 2 + pm) * 64 + ln];
      const int pp = p0 + (ln >> 4), qq = q0 + (ln & (kTW - 1));
      if (pp < Ho && qq < Wo)
        (pm ? M : P)[(size_t)k * set_stride + word_off(n, cw64, wd, Ho * Wo, pp * Wo + qq)] = v;
    }
  }
}

namespace {

// grid.x = images x tiles of one image; 0 when that does not fit (capi.hip keeps N * C * Ho * Wo below 2^31, so it does)
unsigned tile_grid(int N, int Ho, int Wo, int* tiles_w, int* tiles) {
  const long long tw = (Wo + kTW - 1) / kTW, th = (Ho + kTH - 1) / kTH;
  if (tw * th * N > 0x7fffffffLL) return 0;
  *tiles_w = (int)tw;
  *tiles = (int)(tw * th);
  return (unsigned)(tw * th * N);
}

}  // namespace

// capi.hip has checked the pointers, the sizes, G | C1, G | C, C1 / G <= BNN_HIP_STEM_S2X2_MAX_GROUP_CHANNELS, G <= 65535.
int launch_stem_s2x2(const float* x, const float* w1, const float* s1, const float* t1, const float* w2, const float* s2,
                     const float* t2, int N, int C1, int C, int G, int H, int W, int relu_out, float* y, hipStream_t stream) {
  const int H1 = H / 2 + H % 2, W1 = W / 2 + W % 2, H2 = H1 / 2 + H1 % 2, W2 = W1 / 2 + W1 % 2;
  int tiles_w = 0, tiles = 0;
  const unsigned gx = tile_grid(N, H2, W2, &tiles_w, &tiles);
  if (gx == 0) return BNN_HIP_ERR_UNSUPPORTED;
  const size_t lds = (size_t)(3 * kXCS + (C1 / G) * kMCS) * sizeof(float);
  hipLaunchKernelGGL(stem_s2x2_kernel, dim3(gx, (unsigned)G), dim3(256), lds, stream, x, w1, s1, t1, w2, s2, t2, C1 / G,
                     C / G, C, H, W, H1, W1, H2, W2, tiles_w, tiles, relu_out, y);
  return launch_status();
}

// capi.hip has checked the pointers (P / M / pk_a / pk_b when K >= 1, y when K == 0), 0 <= K <= 4, the sizes, G | C, G | O,
// C / G <= BNN_HIP_GCONV3X3S2_MAX_GROUP_CHANNELS and ceil(O / 64) <= 65535.
int launch_gconv3x3s2_bn_pack(const float* x, const float* w, const float* bn_s, const float* bn_t, const float* pk_a,
                              const float* pk_b, int N, int C, int O, int G, int H, int W, int relu_in, int K, uint64_t* P,
                              uint64_t* M, float* y, hipStream_t stream) {
  const int Ho = H / 2 + H % 2, Wo = W / 2 + W % 2;
  int tiles_w = 0, tiles = 0;
  const unsigned gx = tile_grid(N, Ho, Wo, &tiles_w, &tiles);
  if (gx == 0) return BNN_HIP_ERR_UNSUPPORTED;
  const int cw64 = (O + 63) / 64;
  const size_t set_stride = plane_set_stride((long long)N * Ho * Wo, cw64);
  size_t lds = (size_t)(C / G) * kMCS * sizeof(float);
  const size_t comb = (size_t)4 * K * 2 * 64 * sizeof(uint64_t);
  if (lds < comb) lds = comb;
  const dim3 grid(gx, (unsigned)cw64);
  with_k<0>(K, [&](auto kc) {
    hipLaunchKernelGGL((gconv3x3s2_pack_kernel<decltype(kc)::value>), grid, dim3(256), lds, stream, x, w, bn_s, bn_t, pk_a,
                       pk_b, C / G, O / G, C, O, H, W, Ho, Wo, tiles_w, tiles, relu_in, cw64, P, M, set_stride, y);
  });
  return launch_status();
}

}  // namespace bnn

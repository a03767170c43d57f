// slinear.hip — forward of a fully-connected layer with BINARY ACTIVATIONS AND REAL WEIGHTS on a row-major input: the
// Linear of step 0 of the reference's two-stage recipe (examples/recepies/imagenet-baseline.yaml: BasicInputBinarizer,
// BasicScaleBinarizer, weight: nn.Identity), which bnn/layers/linear.py:22-27 evaluates as F.linear(sign(x), W, b) * alpha.
//
//     out[m,o] = (sum_f s(x[m,f]) * W[o,f] + bias[o]) * scale[o]
//
// The arithmetic is that of csrc/sconv.hip (csrc/tgemm.h) — s(x) = +1 / -1 / 0 for x > 0 / x < 0 / anything else is exact
// in bf16, the weight is the ksize = 1 pack of sconv.hip's packer (three bf16 terms hi + mid + lo of W * 2^kexp[o], one
// row exponent per output channel), each product is three bf16 MFMAs (tg::mfma3) with fp32 accumulation, the epilogue
// multiplies by 2^-kexp[o], adds the bias, multiplies by the scale — on the tiling of a GEMM instead of a convolution's
// pixel slots: the 1x1-image route of sconv.hip spends a 64-pixel slot on every row of x.
//
// Per workgroup (256 threads) 64 rows x 64 NSUB output channels; the K loop walks blocks of 64 features: wave w reads
// the rows 16 w .. 16 w + 15 of the tile, lane l feature l of the block — one instruction is 256 contiguous bytes of one
// row (x is 4-byte aligned only — an odd F misaligns every second row — so the loads are dwords, range-checked by the
// buffer descriptor: a feature past F or a row past M is an out-of-range offset and reads 0) — writes s(x) as bf16 into
// ONE LDS plane [row][64 f] (144 bytes per row: conflict-free 16-byte reads) and has the next block's 16 values in flight
// while the matrix cores work on this one.
// Two k-steps of 32 per block; a wave owns all four 16-row sub-tiles of a quarter of the channel groups, so no two waves
// read the same B fragment; the fragments stream from the pack, 1 KB per wave and term, and those of the next K block are
// requested before this block's MFMAs.
//
// Planes: the workgroups of the FIRST output-channel block also write P = x > 0, Mn = x < 0, T = |x| < 1 as
// [M][ceil(F/64)] 64-bit words (one K block of a row = one word = one wave-wide ballot of the fill),
// the bytes of bnn_hip_pack_act_ste_f32(x, M, F, 1, 1): the training forward keeps them instead of x.
//
// ste_mask_kernel: gx[m,f] = T bit (m,f) ? gx[m,f] : +0.0f in place — the hard-tanh straight-through mask on an input
// gradient a library GEMM produced.
#include "tgemm.h"

namespace bnn {

namespace slinear {
constexpr int BM = 64;    // rows per workgroup
constexpr int BK = 64;    // features per K block: one word of the planes
constexpr int APIT = 72;  // LDS plane: halves per row (64 features + 8 pad)
}  // namespace slinear

using namespace tg;  // (kOOB: M * F, M * O < 2^30 elements keep x and out far below the descriptor limit)

// GEMM: M = rows of x (64 per workgroup), N = output channels (64 NSUB per workgroup), K = features.  blockIdx.x =
// row tile * OB + output-channel block (the blocks that share a row tile of x are neighbours).
template <int NSUB>
__global__ __launch_bounds__(NT) void slinear_kernel(const float* __restrict__ x, const bf16x8* __restrict__ Wp,
                                                     const int* __restrict__ kexp, const float* __restrict__ bias,
                                                     const float* __restrict__ scale, float* __restrict__ out,
                                                     unsigned long long* __restrict__ P,
                                                     unsigned long long* __restrict__ Mn,
                                                     unsigned long long* __restrict__ T, int M, int F, int O, int OB) {
  using namespace slinear;
  __shared__ __attribute__((aligned(16))) u16 pa[BM * APIT];

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lg = lane >> 4;
  const int ob = blockIdx.x % OB, m0 = (blockIdx.x / OB) * BM;
  const int CB = (F + 31) / 32, OS = (O + 15) / 16, KB = (F + BK - 1) / BK;
  constexpr int NB = NSUB;                    // channel groups (B fragments x 3 terms) per wave
  const int os0 = (ob * 4 + wave) * NSUB;     // first 16-channel group of this wave
  const bool planes = P != nullptr && ob == 0;

  f32x4 acc[4][NB];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int ns = 0; ns < NB; ++ns) acc[i][ns] = f32x4{0.f, 0.f, 0.f, 0.f};

  // fill role: rows 16 wave + r of the tile, feature `lane` of every K block
  const int fm0 = m0 + 16 * wave;
  const BufRsrc r_x = make_rsrc_sized(x, (unsigned)M * (unsigned)F * 4u);
  float xv[16];
  auto load_x = [&](int kb) {
    const int f = BK * kb + lane;
    const unsigned voff = f < F ? (unsigned)f * 4u : kOOB;
#pragma unroll
    for (int r = 0; r < 16; ++r) {  // the row is wave-uniform: a scalar offset (a row past M: the out-of-range lane offset)
      const bool rlive = fm0 + r < M;
      xv[r] = buf_ld(r_x, rlive ? voff : kOOB, rlive ? (unsigned)(fm0 + r) * (unsigned)F * 4u : 0u);
    }
  };
  load_x(0);
  // the B fragments of both k-steps of K block kb; a k-step past CB or a channel group past OS is zeros
  auto load_w = [&](bf16x8 (&dst)[2][NB][3], int kb) {
#pragma unroll
    for (int st = 0; st < 2; ++st)
#pragma unroll
      for (int ns = 0; ns < NB; ++ns) {
        const int os = os0 + ns, cb = 2 * kb + st;
        const bool live = os < OS && cb < CB;
        const bf16x8* src = Wp + real_frag(live ? cb : 0, 0, live ? os : 0, 1, OS, lane);
#pragma unroll
        for (int t = 0; t < 3; ++t) dst[st][ns][t] = live ? src[64 * t] : zero_frag();
      }
  };
  bf16x8 b[2][NB][3];
  load_w(b, 0);

  for (int kb = 0; kb < KB; ++kb) {
    __syncthreads();  // the previous block's plane is consumed
    const bool two = 2 * kb + 1 < CB;  // the block's second k-step exists (workgroup-uniform)

    // s(x) of this block -> LDS, and the words of the three planes: bit `lane` of a row's word is this lane's feature
    u16* dst = pa + 16 * wave * APIT + lane;
#pragma unroll
    for (int r = 0; r < 16; ++r) dst[r * APIT] = ternary_code(xv[r]);
    if (planes) {  // workgroup-uniform
      const bool flive = BK * kb + lane < F;  // (an out-of-range load is 0: |0| < 1 would set T)
      unsigned long long wp = 0ull, wm = 0ull, wt = 0ull;
#pragma unroll
      for (int r = 0; r < 16; ++r) {  // lane r keeps the words of row r
        const unsigned long long bp = __ballot(xv[r] > 0.0f), bm = __ballot(xv[r] < 0.0f),
                                 bt = __ballot(flive && fabsf(xv[r]) < 1.0f);
        wp = lane == r ? bp : wp;
        wm = lane == r ? bm : wm;
        wt = lane == r ? bt : wt;
      }
      if (lane < 16 && fm0 + lane < M) {
        const size_t word = (size_t)(fm0 + lane) * KB + kb;
        P[word] = wp;
        Mn[word] = wm;
        T[word] = wt;
      }
    }
    __syncthreads();
    load_x(kb + 1);  // past the last block every offset is out of range: zeros nobody reads
    bf16x8 bn[2][NB][3];
    load_w(bn, kb + 1);

    auto step = [&](const bf16x8 (&b)[NB][3], int koff) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(pa + (16 * i + li) * APIT + koff + 8 * lg);
#pragma unroll
        for (int ns = 0; ns < NB; ++ns) acc[i][ns] = mfma3(a, b[ns], acc[i][ns]);
      }
    };
    step(b[0], 0);
    if (two) step(b[1], 32);
#pragma unroll
    for (int st = 0; st < 2; ++st)
#pragma unroll
      for (int ns = 0; ns < NB; ++ns)
#pragma unroll
        for (int t = 0; t < 3; ++t) b[st][ns][t] = bn[st][ns][t];
  }

  // D layout: column = li (output channel within the 16-group), row = 4 lg + r (row within the sub-tile): a store
  // instruction writes 64 contiguous bytes of four rows of out
  const BufRsrc r_o = make_rsrc_sized(out, (unsigned)M * (unsigned)O * 4u);
#pragma unroll
  for (int ns = 0; ns < NB; ++ns) {
    const int o = 16 * (os0 + ns) + li;
    const bool olive = o < O;
    const int ke = olive ? kexp[o] : 0;
    const float bv = (olive && bias) ? bias[o] : 0.0f;
    const float sc = (olive && scale) ? scale[o] : 1.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + 16 * i + 4 * lg + r;
        float v = ldexpf(acc[i][ns][r], -ke);
        if (bias) v = v + bv;
        if (scale) v = v * sc;
        buf_st(r_o, (olive && m < M) ? ((unsigned)m * (unsigned)O + (unsigned)o) * 4u : kOOB, 0u, v);
      }
  }
}

// gx[m,f] = T bit (m,f) ? gx[m,f] : +0.0f; one thread per element, idx < M * F < 2^30
__global__ __launch_bounds__(256) void ste_mask_kernel(float* __restrict__ gx, const unsigned long long* __restrict__ T,
                                                       int M, int F, int FW) {
  const unsigned idx = blockIdx.x * 256u + threadIdx.x;
  if (idx >= (unsigned)M * (unsigned)F) return;
  const unsigned m = idx / (unsigned)F, f = idx - m * (unsigned)F;
  const unsigned long long word = T[(size_t)m * FW + (f >> 6)];
  if (!((word >> (f & 63u)) & 1ull)) gx[idx] = 0.0f;
}

// ------------------------------------------------------------------------------------------------- host side
// Output channels per workgroup: 128 above 64 channels (the choice of sconv.hip), else 64.
int slinear_block_channels(int O) { return 64 * tile_nsub(O); }

int launch_slinear(const float* x, const void* packed, const float* bias, const float* scale, float* out, uint64_t* P,
                   uint64_t* Mn, uint64_t* T, int M, int F, int O, hipStream_t s) {
  using namespace slinear;
  const int bc = slinear_block_channels(O);
  const int OB = (O + bc - 1) / bc, MT = (M + BM - 1) / BM;
  const bf16x8* Wp = static_cast<const bf16x8*>(packed);
  const int* kexp = real_kexp(packed, O, F, 1);
  auto* p = reinterpret_cast<unsigned long long*>(P);
  auto* mn = reinterpret_cast<unsigned long long*>(Mn);
  auto* t = reinterpret_cast<unsigned long long*>(T);
  const dim3 grid((unsigned)((long long)MT * OB));  // M * O < 2^30: below 2^18 + 2^24 workgroups
  if (bc == 128)
    hipLaunchKernelGGL((slinear_kernel<2>), grid, dim3(NT), 0, s, x, Wp, kexp, bias, scale, out, p, mn, t, M, F, O, OB);
  else
    hipLaunchKernelGGL((slinear_kernel<1>), grid, dim3(NT), 0, s, x, Wp, kexp, bias, scale, out, p, mn, t, M, F, O, OB);
  return hipGetLastError() == hipSuccess ? BNN_HIP_OK : BNN_HIP_ERR_LAUNCH;
}

int launch_ste_mask(float* gx, const uint64_t* T, int M, int F, hipStream_t s) {
  const unsigned total = (unsigned)M * (unsigned)F;
  hipLaunchKernelGGL(ste_mask_kernel, dim3((total + 255u) / 256u), dim3(256), 0, s, gx,
                     reinterpret_cast<const unsigned long long*>(T), M, F, (F + 63) / 64);
  return hipGetLastError() == hipSuccess ? BNN_HIP_OK : BNN_HIP_ERR_LAUNCH;
}

}  // namespace bnn

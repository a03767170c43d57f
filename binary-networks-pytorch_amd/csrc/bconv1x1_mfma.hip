// bconv1x1_mfma.hip — the 1x1 binary convolution as a plain GEMM on v_mfma_f32_16x16x128_f8f6f4 (FP4 operands).
//
// Same arithmetic as bconv.hip (bnn/layers/conv.py:90-97) on the same operands: the integer dot of sign(x) in {-1,0,+1}
// with sign(W) in {-1,0,+1} over the C input channels of ONE pixel.  -1, 0 and +1 are exact in E2M1 (0xA, 0x0, 0x2),
// every product is in {-1, 0, +1} and every partial sum is an integer of magnitude <= C <= 2^20 < 2^24, so every fp32
// addition is exact in any order; the accumulator converted to int IS the popcount kernels' dot.  It then enters
// bconv_core.h: epilogue<>() — the same float operations in the same order — and the results are the same bits.
//
// GEMM view: [O, C] x [C, N H W].  Rows = output channels (operand A: the FP4 weight pack, straight from global / L2
// into registers), columns = output pixels = input pixels (operand B: expanded in registers, no LDS), k = channels.
//   workgroup (4 waves) = TP consecutive pixels (linear index over N x H x W: a tile may span images) x TO output
//                         channels, TP x TO = 256 x 64 or 128 x 128; one wave = 64 pixels x 64 channels = 4 x 4 MFMA
//                         tiles of 16 x 16, 64 fp32 accumulators per lane
//   per k-step (one 128-channel group = two consecutive uint64 plane words of a pixel): nibble e of lane l is channel
//                         32 (l >> 4) + e of the group in BOTH operands, so lane l needs exactly ONE 32-bit half-word of P
//                         (and of M) of pixel l & 15 of each of its four pixel tiles: half-word (l >> 4) & 1 of plane
//                         group 2 k + (l >> 5).  4 + 4 global_load_dword and 4 global_load_dwordx4 (A) feed 16 MFMAs;
//                         the half-words are expanded with expand8_f4 (P bit -> 0x2, M bit -> 0xA), four per fragment.
//                         The loads of k-step k + 1 are requested before the MFMAs of k-step k.
// Lanes of columns past N H W read the last pixel's words (never past the planes) and, in the epilogue, hold a copy of
// that pixel: they store the same values to the same addresses (bconv_core.h: epilogue<.., FULL>).
// Epilogue: the accumulators go through LDS, 32 channels at a time, to lane = pixel, as in bconv_mfma.hip; from there on
// it is the popcount kernels' straight-line epilogue.  Every switch bnn_hip_bconv2d_fused knows is taken: the profiles a
// Bottleneck issues are compiled in (BN + ReLU -> planes, with and without thresholds; BN -> fp32; BN + residual + ReLU
// -> fp32 and / or planes) and so are those of a PreBottleneck (ReLU or PReLU -> pack affine -> planes; ReLU or PReLU -> late
// residual -> fp32, with and without such planes); everything else runs the run-time profile.
#include "bconv_mfma.h"

namespace bnn {

namespace {

constexpr int kPreMid = EF_PACK | EF_PACK_AFF;             // planes of sign(bn_next(v)), nothing else written
constexpr int kPreOut = EF_RES | EF_RES_LATE | EF_OUTF;    // the shortcut added behind the activation -> fp32

struct Mfma1Geo {
  int tp;       // pixels per workgroup: 256 (four waves side by side) or 128 (two by two)
  int kgroups;  // C / 128: the k-steps
  int nn;       // M plane all zero
};

// FLAGS != 0 (with EP_RUNTIME): a pre-activation profile — the run-time profile's code with its flag word a compile-time
// constant, so that the switches it does not have cost nothing (same float operations in the same order: same bits).
template <int EP, int FLAGS = 0>
__global__ __launch_bounds__(kMfmaThreads) void bconv1x1_mfma_kernel(const uint32_t* __restrict__ P,
                                                                     const uint32_t* __restrict__ M,
                                                                     const int8_t* __restrict__ W4, BNN_EPI_PARAMS,
                                                                     const Geo g_arg, const Mfma1Geo mg) {
  static_assert(FLAGS == 0 || EP == EP_RUNTIME, "a constant flag word belongs to the run-time profile");
  Geo g = g_arg;
  if constexpr (FLAGS != 0) g.flags = FLAGS;
  BNN_EPI_INIT;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  // (wave-uniform by construction; said so, the per-channel constants of the epilogue stay on the scalar path)
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lrow = lane & 15, lgrp = lane >> 4;
  const int pwaves = mg.tp >> 6;              // waves along the pixels: 4 or 2
  const int wave_pix = (wave % pwaves) * 64;  // first pixel of this wave inside the tile
  const int wave_ch = (wave / pwaves) * 64;   // first channel of this wave inside the workgroup's channels
  const int q0 = blockIdx.x * mg.tp;
  const int o_wave = blockIdx.y * (64 * (4 / pwaves)) + wave_ch;
  const int hw = g.Ho * g.Wo;  // = H W

  // this lane's four B columns (pixels 16 pt + lrow of the wave): index of its 32-bit half-word in k-step 0
  unsigned wi[4];
#pragma unroll
  for (int pt = 0; pt < 4; ++pt) {
    const int q = min(q0 + wave_pix + 16 * pt + lrow, g.npix - 1);
    const int n = (int)fast_div((uint32_t)q, g.m_hw, g.s_hw);
    const int r = q - n * hw;
    // uint64 word (n (C / 64) + group) H W + r of the [N][C / 64][H][W] planes, two half-words each
    wi[pt] = 2u * ((unsigned)(n * (2 * mg.kgroups) + (lgrp >> 1)) * (unsigned)hw + (unsigned)r) + (unsigned)(lgrp & 1);
  }
  const unsigned kstride = 4u * (unsigned)hw;  // half-words from one 128-channel group to the next

  f32x4 acc[4][4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) acc[ct][pt] = f32x4{0, 0, 0, 0};

  const bool nn = mg.nn != 0;
  // A fragments of this wave: [o / 64][128-channel group][16-channel tile][lane][16 bytes]
  const int8_t* wbase = W4 + (size_t)(o_wave >> 6) * mg.kgroups * 4096 + lane * 16;
  auto request = [&](i32x4 (&a)[4], uint32_t (&pw)[4], uint32_t (&mw)[4], int k) {
    const int kk = min(k, mg.kgroups - 1);  // (past the end: the last k-step's again, never used)
    const int8_t* src = wbase + (size_t)kk * 4096;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) a[ct] = *reinterpret_cast<const i32x4*>(src + ct * 1024);
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) {
      pw[pt] = P[wi[pt] + (unsigned)kk * kstride];
      mw[pt] = nn ? 0u : M[wi[pt] + (unsigned)kk * kstride];
    }
  };

  i32x4 a_cur[4], a_nxt[4];
  uint32_t p_cur[4], m_cur[4], p_nxt[4], m_nxt[4];
  request(a_cur, p_cur, m_cur, 0);
#pragma unroll 1
  for (int k = 0; k < mg.kgroups; ++k) {
    request(a_nxt, p_nxt, m_nxt, k + 1);
    i32x4 b[4];
#pragma unroll
    for (int pt = 0; pt < 4; ++pt)
      b[pt] = i32x4{(int)expand8_f4(p_cur[pt], m_cur[pt], 0, nn), (int)expand8_f4(p_cur[pt], m_cur[pt], 8, nn),
                    (int)expand8_f4(p_cur[pt], m_cur[pt], 16, nn), (int)expand8_f4(p_cur[pt], m_cur[pt], 24, nn)};
    __builtin_amdgcn_sched_barrier(0);  // keep the requests in front of the MFMAs they hide behind
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int pt = 0; pt < 4; ++pt) acc[ct][pt] = mma_step<true>(a_cur[ct], b[pt], acc[ct][pt]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      a_cur[i] = a_nxt[i];
      p_cur[i] = p_nxt[i];
      m_cur[i] = m_nxt[i];
    }
  }

  // ---- epilogue: lane = pixel, 32 channels at a time through LDS (each wave its own 32 x kAccStride words) ----
  const Pix px = decode_pixel<true>(g, q0 + wave_pix + lane);
  int* tbuf = reinterpret_cast<int*>(lds) + wave * (32 * kAccStride);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int o0 = o_wave + 32 * h;
    float resv[32];
    prefetch_residual<32, EP, true>(g, px, o0, epi, resv);
    __syncthreads();  // the first half's values (h = 1) have been read
#pragma unroll
    for (int c2 = 0; c2 < 2; ++c2)
#pragma unroll
      for (int pt = 0; pt < 4; ++pt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          tbuf[(16 * c2 + 4 * lgrp + r) * kAccStride + 16 * pt + lrow] = (int)acc[2 * h + c2][pt][r];  // (exact)
    __syncthreads();
    int dot[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) dot[j] = tbuf[j * kAccStride + lane];
    uint32_t pbits = 0u, mbits = 0u;
    // EP_MIDT: bit = (dot >= T) ^ flip, written as dot * 1 + 0 >= T
    epilogue<32, EP, true>(g, px, o0, dot, resv, epi, pbits, mbits, 0, 1.0f, 0.0f);
    uint32_t xorw = 0u;
    if constexpr (EP == EP_MIDT) xorw = (uint32_t)epi.thr[kThrStride * o0 + 1];
    store_packed(g, px, o0 >> 5, pbits, mbits, epi, true, xorw);
  }
}

template <int EP, int FLAGS = 0>
void launch_ep(const ConvP& p, const Geo& g, const Mfma1Geo& mg, const void* w4, dim3 grid, hipStream_t s) {
  hipLaunchKernelGGL((bconv1x1_mfma_kernel<EP, FLAGS>), grid, dim3(kMfmaThreads), (size_t)kAccBytes, s, p.P, p.M,
                     static_cast<const int8_t*>(w4), BNN_EPI_ACTUALS, g, mg);
}

}  // namespace

size_t weight1x1_f4_bytes(int O, int C) {
  if (O <= 0 || C <= 0 || O % 64 != 0 || C % 128 != 0) return 0;
  return (size_t)O * (size_t)C / 2;
}

// What the kernel covers, stated once (capi.hip asks here for the launch and for bnn_hip_bconv1x1_mfma4_supported):
// a dense 1x1 / stride 1 / padding 0 / dilation 1 convolution over whole 128-channel groups into whole 64-channel tiles,
// inside the index ranges of the tiled kernels, writing all channels of its output tensor; every epilogue of
// bnn_hip_bconv2d_fused but the folded shortcut (and the int32 dot, which that entry point does not have).
bool mfma1x1_applies(const ConvP& p, int flags) {
  if (flags & BNN_HIP_FLAG_FORCE_GENERIC) return false;
  if (p.KH != 1 || p.KW != 1 || p.sh != 1 || p.sw != 1 || p.ph != 0 || p.pw != 0 || p.dh != 1 || p.dw != 1) return false;
  if (weight1x1_f4_bytes(p.O, p.C) == 0 || !small_indices(p)) return false;
  if (p.raw || p.ds_P || p.out16 != 0) return false;
  if (p.c_off != 0 || p.c_tot != p.O) return false;
  if ((long long)p.N * p.H * p.Wd >= (1ll << 30)) return false;
  return true;
}

int launch_bconv1x1_mfma(const ConvP& p, int flags, const void* w4, hipStream_t s) {
  if (!mfma1x1_applies(p, flags)) return BNN_HIP_ERR_UNSUPPORTED;
  const Geo g = make_geo(p);
  Mfma1Geo mg;
  mg.tp = p.O % 128 == 0 ? 128 : 256;  // 128 x 128: half the activation expansions per output
  mg.kgroups = p.C / 128;
  mg.nn = (flags & BNN_HIP_FLAG_ACT_NONNEG) ? 1 : 0;
  const dim3 grid((unsigned)((p.npix + mg.tp - 1) / mg.tp), (unsigned)(p.O / (mg.tp == 256 ? 64 : 128)));
  const int f = g.flags;
  const bool fused = (f & (EF_BN | EF_RES | EF_RELU | EF_PRELU | EF_PACK)) != 0;
  if (f == kFlagsMid && p.thr) launch_ep<EP_MIDT>(p, g, mg, w4, grid, s);
  else if (f == kFlagsMid) launch_ep<EP_MID>(p, g, mg, w4, grid, s);
  else if (f == kFlagsOut) launch_ep<EP_OUT>(p, g, mg, w4, grid, s);
  else if (f == kFlagsOutP) launch_ep<EP_OUTP>(p, g, mg, w4, grid, s);
  else if (f == kFlagsLast) launch_ep<EP_LAST>(p, g, mg, w4, grid, s);
  else if (f == kFlagsDs) launch_ep<EP_DS>(p, g, mg, w4, grid, s);
  // the launches of a pre-activation bottleneck: act -> next BatchNorm -> planes; act -> + shortcut -> fp32 [+ such planes]
  else if (f == (EF_RELU | kPreMid)) launch_ep<EP_RUNTIME, EF_RELU | kPreMid>(p, g, mg, w4, grid, s);
  else if (f == (EF_PRELU | kPreMid)) launch_ep<EP_RUNTIME, EF_PRELU | kPreMid>(p, g, mg, w4, grid, s);
  else if (f == (EF_RELU | kPreOut)) launch_ep<EP_RUNTIME, EF_RELU | kPreOut>(p, g, mg, w4, grid, s);
  else if (f == (EF_PRELU | kPreOut)) launch_ep<EP_RUNTIME, EF_PRELU | kPreOut>(p, g, mg, w4, grid, s);
  else if (f == (EF_RELU | kPreOut | kPreMid)) launch_ep<EP_RUNTIME, EF_RELU | kPreOut | kPreMid>(p, g, mg, w4, grid, s);
  else if (f == (EF_PRELU | kPreOut | kPreMid)) launch_ep<EP_RUNTIME, EF_PRELU | kPreOut | kPreMid>(p, g, mg, w4, grid, s);
  else if (fused) launch_ep<EP_RUNTIME>(p, g, mg, w4, grid, s);
  else launch_ep<EP_PLAIN>(p, g, mg, w4, grid, s);
  return hipGetLastError() == hipSuccess ? BNN_HIP_OK : BNN_HIP_ERR_LAUNCH;
}

}  // namespace bnn

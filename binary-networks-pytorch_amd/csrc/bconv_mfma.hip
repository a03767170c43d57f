// bconv_mfma.hip — the dense 3x3 binary convolution as an implicit GEMM on v_mfma_i32_16x16x64_i8.
//
// Same arithmetic as bconv.hip (bnn/layers/conv.py:90-97): the integer dot of sign(x) in {-1,0,+1} with sign(W) in
// {-1,0,+1} over the 3x3 window.  Both operands are exact in int8 and the int32 accumulation of at most 9 C <= 2^20
// products of magnitude <= 1 is exact, so the accumulator IS the popcount kernels' dot; it then enters
// bconv_core.h: epilogue<>() — the same float operations in the same order — and the results are the same bits.
//
// GEMM view: rows = output channels (operand A: the int8 weight pack, straight from global / L2 into registers), columns
// = output pixels (operand B: int8 activations from LDS), k = (64-channel group, tap, channel in the group).
//   workgroup (4 waves) = TP consecutive output pixels (linear index over N x Ho x Wo: a tile may span rows and images)
//                         x TO output channels, TP x TO = 256 x 64 or 128 x 128; one wave = 64 pixels x 64 channels
//                         = 4 x 4 MFMA tiles of 16 x 16, 64 int32 accumulators per lane
//   per 64-channel group: the sign-plane words of every input pixel the tile touches — one contiguous run of the linear
//                         input index n H W + y W + x, its neighbours one row up and down included — are expanded once
//                         into LDS as 64 int8 per pixel (P bit -> 0x01, M bit -> 0xFF; P and M are exclusive).  The nine
//                         taps are shifted 16-byte reads of that patch; a tap in the zero padding (or in the neighbouring
//                         row / image, where the shifted index lands) reads a row of zero bytes instead.
//   per k-step (one tap of one group): 4 ds_read_b128 + 4 global_load_dwordx4 feed 16 MFMAs.
// The k order inside a fragment is the kernel's own choice (integer sums do not depend on it): byte e of lane l is
// channel 16 (l >> 4) + e of the group in BOTH operands.  What the hardware fixes is that lane l holds row / column
// l & 15 of A / B and that D has column l & 15 and rows 4 (l >> 4) + r in register r.
// Epilogue: the accumulators go through LDS, 32 channels at a time, to lane = pixel; from there on it is the popcount
// kernels' straight-line epilogue (coalesced NCHW stores, one 32-channel plane word per lane).
//
// FP4 form (F4, C % 128 == 0): the same kernel on v_mfma_f32_16x16x128_f8f6f4 with E2M1 operands (cbsz:4 blgp:4, no
// scales): -1, 0 and +1 are exact in E2M1 (0xA, 0x0, 0x2), every product is in {-1, 0, +1} and every partial sum is an
// integer of magnitude <= 9 C <= 2^20 < 2^24, so every fp32 addition is exact in any order and the accumulator converted
// to int is the same dot.  A k-step is one tap of a 128-channel group = two consecutive 64-channel plane groups: the same
// 16 bytes per lane and operand as the int8 form at half the k-steps.  The LDS patch stays 64 bytes per pixel, now 128
// nibbles (P bit -> 0x2, M bit -> 0xA); nibble e of lane l is channel 32 (l >> 4) + e of the group in BOTH operands, so
// lane group l >> 4 reads the 16 bytes that come from 32-bit plane word l >> 4 of the group.  Tile choice, pipeline and
// epilogue are the int8 form's; the folded shortcut's 1x1 prologue stays on the int8 instruction with int32
// accumulators of its own, dead before the main loop.
#include "bconv_mfma.h"

#include <type_traits>

namespace bnn {

namespace {

constexpr int kMaxLds = 64 * 1024;
constexpr int kPatchSlots = 4;  // patch pixels per thread (1024 pixels = the LDS limit): the plane words of the next group wait in registers
// Folded shortcut (DS): the shortcut's dots wait in LDS behind the patch / transpose buffer while the main loop runs, as
// int16 (|dot| <= 256), one row of 64 channels per pixel of a wave.  72 int16 = 36 dwords per row: a lane's four
// ds_read_b128 of a half land 4 banks apart from its neighbour's, eight lanes cover the 32 banks.
constexpr int kParkStride = 72;
constexpr int kParkBytes = 4 * 64 * kParkStride * 2;  // four waves x 64 pixels
constexpr int kMaxLdsFold = 80 * 1024;  // two workgroups in the CU's 160 KB

struct MfmaGeo {
  int tp;          // output pixels per workgroup: 256 (four waves side by side) or 128 (two by two)
  int groups;      // C / 64
  int ihw;         // H * W
  int patch_cap;   // pixels of the LDS patch (the zero row sits behind them)
  int nn;          // M plane all zero
  int n_in;        // N * H * W
  uint32_t m_ihw;  // fast_div by ihw
  int s_ihw;
  int park_off;    // DS: byte offset of the parked shortcut dots in the LDS
};

// The folded shortcut convolution (bconv_core.h: ShortcutArgs) with its weight as int8 A fragments.
struct ShortcutArgs8 {
  const uint32_t* P;
  const int8_t* W8;  // [o / 64][group][16-channel tile][lane][16 bytes] (include/bnn_hip.h: bnn_hip_pack_shortcut_weight_i8)
  const float* alpha;
  const float* a;
  const float* b;
};

// 4 bits -> 4 bytes of 0 / 1: bit i lands at 8 i  (0x00204081 = 1 + 2^7 + 2^14 + 2^21; both factors below 2^24)
__device__ __forceinline__ uint32_t spread4(uint32_t word, int sh) {
  return __umul24((word >> sh) & 15u, 0x00204081u) & 0x01010101u;
}
__device__ __forceinline__ uint32_t expand4(uint32_t pw, uint32_t mw, int sh, bool nn) {
  const uint32_t p = spread4(pw, sh);
  if (nn) return p;
  return p | (spread4(mw, sh) * 0xFFu);  // bytes of 0 / 1 times 255: no carry between bytes
}

// (nibbles8 / expand8_f4, the FP4 expansion, and mma_step, one k-step of one 16 x 16 tile: bconv_mfma.h)
template <bool First, class A, class B>
__device__ __forceinline__ auto& pick(A& a, B& b) {
  if constexpr (First) return a;
  else return b;
}

// linear input index of the window centre of output pixel q (monotone in q)
__device__ __forceinline__ int centre_of(const Geo& g, const MfmaGeo& mg, int q, int* oy, int* ox) {
  const int hw = g.Ho * g.Wo;
  const int n = (int)fast_div((uint32_t)q, g.m_hw, g.s_hw);
  const int r = q - n * hw;
  *oy = (int)fast_div((uint32_t)r, g.m_wo, g.s_wo);
  *ox = r - *oy * g.Wo;
  return n * mg.ihw + *oy * g.sh * g.Wd + *ox * g.sw;
}

// DS: the block's shortcut convolution folded in (EP_OUT only).  The residual of channel o at a pixel is
//     r = fmaf(fmaf(alpha_ds[o], (float)dot1x1, 0), a_ds[o], b_ds[o])
// — the float operations of the popcount fold (bconv_core.h: shortcut_values_cw) on the same integer.  The 1, 2 or 4
// k-steps of the 1x1 convolution run FIRST, through the same A / B pipeline into `acc`: B = the OR-pooled P plane of the
// tile's own output pixels expanded into the (still unused) patch, A = the shortcut's int8 pack.  Their result is parked
// in LDS as int16 in the layout the epilogue reads (lane = pixel, 32 channels = four ds_read_b128), `acc` starts again
// from zero and the main loop runs unchanged: no register lives across it, and the epilogue gains only the conversion.
// (The shortcut's pointers travel behind the geometry: the kernel arguments of the plain form keep their places.)
// F4: the FP4 form (file comment): W8 is then the FP4 pack of bnn_hip_pack_weight_f4 (the shortcut's stays int8).
template <int EP, bool DS = false, bool F4 = false>
__global__ __launch_bounds__(kMfmaThreads) void bconv_mfma_kernel(const uint32_t* __restrict__ P,
                                                                  const uint32_t* __restrict__ M,
                                                                  const int8_t* __restrict__ W8, BNN_EPI_PARAMS,
                                                                  const Geo g, const MfmaGeo mg,
                                                                  const uint32_t* __restrict__ dsP,
                                                                  const int8_t* __restrict__ dsW8,
                                                                  const float* __restrict__ ds_alpha,
                                                                  const float* __restrict__ ds_a,
                                                                  const float* __restrict__ ds_b) {
  static_assert(!DS || EP == EP_OUT, "the fold belongs to BN + residual + ReLU -> fp32 + planes");
  BNN_EPI_INIT;
  [[maybe_unused]] const ShortcutArgs8 sc{dsP, dsW8, ds_alpha, ds_a, ds_b};
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  // (wave-uniform by construction; said so, the per-channel constants of the epilogue stay on the scalar path)
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lrow = lane & 15, lgrp = lane >> 4;
  const int pwaves = mg.tp >> 6;                 // waves along the pixels: 4 or 2
  const int wave_pix = (wave % pwaves) * 64;     // first pixel of this wave inside the tile
  const int wave_ch = (wave / pwaves) * 64;      // first channel of this wave inside the workgroup's channels
  const int q0 = blockIdx.x * mg.tp;
  const int o_wave = blockIdx.y * (64 * (4 / pwaves)) + wave_ch;

  // the tile's run of input pixels
  int ty, tx;
  const int c_first = centre_of(g, mg, q0, &ty, &tx);
  const int c_last = centre_of(g, mg, min(q0 + mg.tp, g.npix) - 1, &ty, &tx);
  const int l_lo = max(c_first - g.Wd - 1, 0);
  const int patch_len = min(min(c_last + g.Wd + 1, mg.n_in - 1) - l_lo + 1, mg.patch_cap);
  const int zero_idx = mg.patch_cap;

  // this lane's four B columns (pixels 16 pt + lrow of the wave): patch index of the window centre, valid taps
  int base[4];
  uint32_t okm[4];
#pragma unroll
  for (int pt = 0; pt < 4; ++pt) {
    const int q = min(q0 + wave_pix + 16 * pt + lrow, g.npix - 1);
    int oy, ox;
    base[pt] = centre_of(g, mg, q, &oy, &ox) - l_lo;
    uint32_t m = 0u;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int iy = oy * g.sh - 1 + t / 3, ix = ox * g.sw - 1 + t % 3;
      const bool ok = (unsigned)iy < (unsigned)g.H && (unsigned)ix < (unsigned)g.Wd;
      m |= (ok ? 1u : 0u) << t;
    }
    okm[pt] = m;
  }

  using acc_t = std::conditional_t<F4, f32x4, i32x4>;
  acc_t acc[4][4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) acc[ct][pt] = acc_t{0, 0, 0, 0};

  if (tid < 4) reinterpret_cast<uint4*>(lds + (size_t)zero_idx * 64)[tid] = uint4{0u, 0u, 0u, 0u};

  const bool nn = mg.nn != 0;
  const uint2* P2 = reinterpret_cast<const uint2*>(P);
  const uint2* M2 = reinterpret_cast<const uint2*>(M);
  // A fragments of this wave: [o / 64][group][tap][16-channel tile][lane][16 bytes]
  // (FP4: [o / 64][128-channel group][tap][16-channel tile][lane][16 bytes], the same 4096 bytes per k-step)
  const int kgroups = F4 ? mg.groups >> 1 : mg.groups;  // groups of the k loop: 128 or 64 channels
  const int8_t* wbase = W8 + (size_t)(o_wave >> 6) * kgroups * (9 * 4096) + lane * 16;

  // Software pipeline.  A fragments: k-step k + 2 (contiguous behind k and k + 1, across groups too) is requested before
  // the MFMAs of k-step k — three register sets in rotation, and nine taps per group bring the rotation back to its
  // start.  B fragments: the next tap's, within a group.  Plane words: the next group's are requested into registers
  // before the current group's MFMAs and expanded into the patch behind them.
  const int ksteps = kgroups * 9;
  auto a_load = [&](i32x4 (&dst)[4], int k) {
    const int8_t* src = wbase + (size_t)min(k, ksteps - 1) * 4096;  // (past the end: the last k-step's again, never used)
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) dst[ct] = *reinterpret_cast<const i32x4*>(src + ct * 1024);
  };
  auto b_frag = [&](int pt, int t) -> i32x4 {
    const int off = (t / 3 - 1) * g.Wd + (t % 3 - 1);
    const int idx = ((okm[pt] >> t) & 1u) ? min(base[pt] + off, zero_idx) : zero_idx;
    return *reinterpret_cast<const i32x4*>(lds + (size_t)idx * 64 + lgrp * 16);
  };
  // patch pixels tid, tid + 256, ... (patch_cap <= kPatchSlots * 256: choose_tile)
  unsigned wi0[kPatchSlots];
  uint2 pv[kPatchSlots], mv[kPatchSlots];
  [[maybe_unused]] uint2 pv1[F4 ? kPatchSlots : 1], mv1[F4 ? kPatchSlots : 1];  // FP4: the second plane group of the 128
#pragma unroll
  for (int sl = 0; sl < kPatchSlots; ++sl) {
    const int L = l_lo + min(tid + sl * kMfmaThreads, patch_len - 1);
    const int n = (int)fast_div((uint32_t)L, mg.m_ihw, mg.s_ihw);
    wi0[sl] = (unsigned)(n * mg.groups * mg.ihw + (L - n * mg.ihw));  // uint64 words, group 0
    pv[sl] = uint2{0u, 0u};
    mv[sl] = uint2{0u, 0u};
    if constexpr (F4) {
      pv1[sl] = uint2{0u, 0u};
      mv1[sl] = uint2{0u, 0u};
    }
  }
  auto request = [&](int gi) {
#pragma unroll
    for (int sl = 0; sl < kPatchSlots; ++sl)
      if (sl * kMfmaThreads < patch_len) {  // (wave-uniform; lanes past the end re-read the last pixel)
        if constexpr (F4) {  // plane groups 2 gi and 2 gi + 1
          pv[sl] = P2[wi0[sl] + (unsigned)(2 * gi * mg.ihw)];
          pv1[sl] = P2[wi0[sl] + (unsigned)((2 * gi + 1) * mg.ihw)];
          if (!nn) {
            mv[sl] = M2[wi0[sl] + (unsigned)(2 * gi * mg.ihw)];
            mv1[sl] = M2[wi0[sl] + (unsigned)((2 * gi + 1) * mg.ihw)];
          }
        } else {
          pv[sl] = P2[wi0[sl] + (unsigned)(gi * mg.ihw)];
          if (!nn) mv[sl] = M2[wi0[sl] + (unsigned)(gi * mg.ihw)];
        }
      }
  };
  auto expand = [&]() {
#pragma unroll
    for (int sl = 0; sl < kPatchSlots; ++sl) {
      const int i = tid + sl * kMfmaThreads;
      if (i < patch_len) {
        uint4* dst = reinterpret_cast<uint4*>(lds + (size_t)i * 64);
        if constexpr (F4) {  // 16 bytes per 32-bit plane word of the group
          const uint32_t pw4[4] = {pv[sl].x, pv[sl].y, pv1[sl].x, pv1[sl].y};
          const uint32_t mw4[4] = {mv[sl].x, mv[sl].y, mv1[sl].x, mv1[sl].y};
#pragma unroll
          for (int h = 0; h < 4; ++h)
            dst[h] = uint4{expand8_f4(pw4[h], mw4[h], 0, nn), expand8_f4(pw4[h], mw4[h], 8, nn),
                           expand8_f4(pw4[h], mw4[h], 16, nn), expand8_f4(pw4[h], mw4[h], 24, nn)};
        } else {
#pragma unroll
          for (int h = 0; h < 4; ++h) {
            const uint32_t pw = h < 2 ? pv[sl].x : pv[sl].y, mw = h < 2 ? mv[sl].x : mv[sl].y;
            const int s0 = 16 * (h & 1);
            dst[h] = uint4{expand4(pw, mw, s0, nn), expand4(pw, mw, s0 + 4, nn), expand4(pw, mw, s0 + 8, nn),
                           expand4(pw, mw, s0 + 12, nn)};
          }
        }
      }
    }
  };

  request(0);
  i32x4 a_buf[3][4];
  [[maybe_unused]] i32x4 sc_acc[F4 && DS ? 4 : 1][4];  // FP4: the int8 prologue's own accumulators
  if constexpr (DS) {
    i32x4(&sacc)[4][4] = pick<F4>(sc_acc, acc);
    if constexpr (F4) {
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int pt = 0; pt < 4; ++pt) sacc[ct][pt] = i32x4{0, 0, 0, 0};
    }
    const int sg = g.ds_cw >> 1;  // 64-channel groups of the shortcut input = its k-steps: 1, 2 or 4
    // the shortcut plane words of tile pixel `tid` (threads past the tile hold a clamped copy and write nothing)
    uint2 scw[4];
    {
      const int q = min(q0 + tid, g.npix - 1), hw = g.Ho * g.Wo;
      const int n = (int)fast_div((uint32_t)q, g.m_hw, g.s_hw), r = q - n * hw;
      const int oy = (int)fast_div((uint32_t)r, g.m_wo, g.s_wo), ox = r - oy * g.Wo;
      const uint2* S2 = reinterpret_cast<const uint2*>(sc.P);
      if (g.ds_w > 0) {  // un-pooled plane: OR of the 2 x 2 window, clipped at odd edges (load_shortcut_field)
        const unsigned shw = (unsigned)(g.ds_h * g.ds_w);
        const int y0 = 2 * oy, x0 = 2 * ox;
        const bool x1 = x0 + 1 < g.ds_w, y1 = y0 + 1 < g.ds_h;
        const unsigned b0 = (unsigned)n * (unsigned)sg * shw + (unsigned)(y0 * g.ds_w + x0);
        static_for<4>([&](auto GI) {
          constexpr int gi = GI;
          uint2 v{0u, 0u};
          if (gi < sg) {
            const unsigned b = b0 + (unsigned)gi * shw;
            v = S2[b];
            const uint2 a = S2[x1 ? b + 1 : b], c = S2[y1 ? b + (unsigned)g.ds_w : b],
                        e = S2[(x1 && y1) ? b + (unsigned)g.ds_w + 1 : b];
            v.x |= a.x | c.x | e.x;
            v.y |= a.y | c.y | e.y;
          }
          scw[gi] = v;
        });
      } else {
        const unsigned b0 = (unsigned)n * (unsigned)sg * (unsigned)hw + (unsigned)r;
        static_for<4>([&](auto GI) {
          constexpr int gi = GI;
          scw[gi] = gi < sg ? S2[b0 + (unsigned)(gi * hw)] : uint2{0u, 0u};
        });
      }
    }
    const int8_t* sbase = sc.W8 + (size_t)(o_wave >> 6) * sg * 4096 + lane * 16;
    auto sa_load = [&](i32x4 (&dst)[4], int k) {
      const int8_t* src = sbase + (size_t)min(k, sg - 1) * 4096;  // (past the end: the last k-step's again, never used)
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) dst[ct] = *reinterpret_cast<const i32x4*>(src + ct * 1024);
    };
    sa_load(a_buf[0], 0);
    sa_load(a_buf[1], 1);
    static_for<4>([&](auto K) {
      constexpr int k = K;
      if (k < sg) {  // (wave-uniform)
        if (k > 0) __syncthreads();  // the previous group's reads are done
        if (tid < mg.tp) {
          uint4* dst = reinterpret_cast<uint4*>(lds + (size_t)tid * 64);
#pragma unroll
          for (int h = 0; h < 4; ++h) {
            const uint32_t pw = h < 2 ? scw[k].x : scw[k].y;
            const int s0 = 16 * (h & 1);
            dst[h] = uint4{expand4(pw, 0u, s0, true), expand4(pw, 0u, s0 + 4, true), expand4(pw, 0u, s0 + 8, true),
                           expand4(pw, 0u, s0 + 12, true)};
          }
        }
        __syncthreads();
        sa_load(a_buf[(k + 2) % 3], k + 2);
        i32x4 b_sc[4];
#pragma unroll
        for (int pt = 0; pt < 4; ++pt)
          b_sc[pt] = *reinterpret_cast<const i32x4*>(lds + (size_t)(wave_pix + 16 * pt + lrow) * 64 + lgrp * 16);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
#pragma unroll
          for (int pt = 0; pt < 4; ++pt)
            sacc[ct][pt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_buf[k % 3][ct], b_sc[pt], sacc[ct][pt], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    });
  }
  a_load(a_buf[0], 0);
  a_load(a_buf[1], 1);
  if constexpr (DS) {
    // park the shortcut dots (this wave's 64 pixels x 64 channels; only this wave reads them back, in the epilogue)
    short* park = reinterpret_cast<short*>(lds + mg.park_off) + wave * (64 * kParkStride);
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int pt = 0; pt < 4; ++pt) {
        const i32x4 v = pick<F4>(sc_acc, acc)[ct][pt];
        *reinterpret_cast<uint2*>(park + (16 * pt + lrow) * kParkStride + 16 * ct + 4 * lgrp) =
            uint2{((uint32_t)v[0] & 0xFFFFu) | ((uint32_t)v[1] << 16), ((uint32_t)v[2] & 0xFFFFu) | ((uint32_t)v[3] << 16)};
        acc[ct][pt] = acc_t{0, 0, 0, 0};
      }
  }
#pragma unroll 1
  for (int gi = 0; gi < kgroups; ++gi) {
    __syncthreads();  // the previous group's reads of the patch (gi = 0, DS: of the shortcut operand) are done
    expand();
    __syncthreads();
    if (gi + 1 < kgroups) request(gi + 1);
    i32x4 b_cur[4];
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) b_cur[pt] = b_frag(pt, 0);
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      i32x4 b_nxt[4];
      a_load(a_buf[(t + 2) % 3], gi * 9 + t + 2);
      if (t < 8) {
#pragma unroll
        for (int pt = 0; pt < 4; ++pt) b_nxt[pt] = b_frag(pt, t + 1);
      }
      __builtin_amdgcn_sched_barrier(0);  // keep the requests in front of the MFMAs they hide behind
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int pt = 0; pt < 4; ++pt)
          acc[ct][pt] = mma_step<F4>(a_buf[t % 3][ct], b_cur[pt], acc[ct][pt]);
      __builtin_amdgcn_sched_barrier(0);
      if (t < 8) {
#pragma unroll
        for (int pt = 0; pt < 4; ++pt) b_cur[pt] = b_nxt[pt];
      }
    }
  }

  // ---- epilogue: lane = pixel, 32 channels at a time through LDS ----
  const Pix px = decode_pixel<true>(g, q0 + wave_pix + lane);
  int* tbuf = reinterpret_cast<int*>(lds) + wave * (32 * kAccStride);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int o0 = o_wave + 32 * h;
    float resv[32];
    if constexpr (DS) {
      using f2 = __attribute__((ext_vector_type(2))) float;
      const uint4* pr = reinterpret_cast<const uint4*>(reinterpret_cast<const short*>(lds + mg.park_off) +
                                                       wave * (64 * kParkStride) + lane * kParkStride + 32 * h);
      uint32_t w[16];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const uint4 v = pr[i];
        w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
      }
#pragma unroll
      for (int j = 0; j < 32; j += 2) {
        const int o = o0 + j;
        const f2 d = f2{(float)((int)(w[j >> 1] << 16) >> 16), (float)((int)w[j >> 1] >> 16)};
        const f2 t = __builtin_elementwise_fma(f2{sc.alpha[o], sc.alpha[o + 1]}, d, f2{0.0f, 0.0f});
        const f2 r = __builtin_elementwise_fma(t, f2{sc.a[o], sc.a[o + 1]}, f2{sc.b[o], sc.b[o + 1]});
        resv[j] = r.x;
        resv[j + 1] = r.y;
      }
    } else {
      prefetch_residual<32, EP, true>(g, px, o0, epi, resv);
    }
    __syncthreads();  // the patch (h = 0) / the first half's values (h = 1) have been read
#pragma unroll
    for (int c2 = 0; c2 < 2; ++c2)
#pragma unroll
      for (int pt = 0; pt < 4; ++pt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          tbuf[(16 * c2 + 4 * lgrp + r) * kAccStride + 16 * pt + lrow] = (int)acc[2 * h + c2][pt][r];  // (FP4: exact)
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

// wbits / wnz (bnn_hip_pack_weight_f32) -> int8 A fragments (include/bnn_hip.h: bnn_hip_pack_weight_i8).  One thread per
// four bytes.  wnz == null: no zero weights (the folded shortcut's 1x1 weight: taps = 1).
__global__ __launch_bounds__(256) void pack_weight_i8_kernel(const uint32_t* __restrict__ wbits,
                                                             const uint32_t* __restrict__ wnz, int O, int taps,
                                                             int cw32, int cwc, uint32_t* __restrict__ w8) {
  const int groups = cw32 >> 1, nchunk = cw32 / cwc, per_o = taps * cwc;
  const size_t total = (size_t)O * groups * taps * 16;  // dwords
  const size_t d = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (d >= total) return;
  const int e4 = (int)(d & 3), lane = (int)((d >> 2) & 63), ct = (int)((d >> 8) & 3);
  size_t rest = d >> 10;
  const int t = (int)(rest % taps);
  rest /= taps;
  const int gi = (int)(rest % groups), ob64 = (int)(rest / groups);
  const int o = 64 * ob64 + 16 * ct + (lane & 15);
  const int c0 = 64 * gi + 16 * (lane >> 4) + 4 * e4;  // four consecutive input channels, inside one 32-bit word
  const int cw_abs = c0 >> 5, ch = cw_abs / cwc, cw = cw_abs - ch * cwc;
  const size_t wi = ((size_t)((o >> 5) * nchunk + ch) * kOCB + (o & 31)) * per_o + t * cwc + cw;
  const uint32_t b = wbits[wi] >> (c0 & 31), z = wnz ? wnz[wi] >> (c0 & 31) : 15u;
  uint32_t v = 0u;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t byte = ((z >> k) & 1u) ? (((b >> k) & 1u) ? 0x01u : 0xFFu) : 0u;
    v |= byte << (8 * k);
  }
  w8[d] = v;
}

// wbits / wnz -> FP4 (E2M1) A fragments (include/bnn_hip.h: bnn_hip_pack_weight_f4).  One thread per dword = eight
// consecutive input channels of one output channel and tap: +1 -> 0x2, -1 -> 0xA, a zero weight -> 0x0.
__global__ __launch_bounds__(256) void pack_weight_f4_kernel(const uint32_t* __restrict__ wbits,
                                                             const uint32_t* __restrict__ wnz, int O, int taps,
                                                             int cw32, int cwc, uint32_t* __restrict__ w4) {
  const int groups = cw32 >> 2, nchunk = cw32 / cwc, per_o = taps * cwc;
  const size_t total = (size_t)O * groups * taps * 16;  // dwords
  const size_t d = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (d >= total) return;
  const int e8 = (int)(d & 3), lane = (int)((d >> 2) & 63), ct = (int)((d >> 8) & 3);
  size_t rest = d >> 10;
  const int t = (int)(rest % taps);
  rest /= taps;
  const int gi = (int)(rest % groups), ob64 = (int)(rest / groups);
  const int o = 64 * ob64 + 16 * ct + (lane & 15);
  const int c0 = 128 * gi + 32 * (lane >> 4) + 8 * e8;  // eight consecutive input channels, inside one 32-bit word
  const int cw_abs = c0 >> 5, ch = cw_abs / cwc, cw = cw_abs - ch * cwc;
  const size_t wi = ((size_t)((o >> 5) * nchunk + ch) * kOCB + (o & 31)) * per_o + t * cwc + cw;
  const uint32_t b = wbits[wi] >> (c0 & 31), z = wnz[wi] >> (c0 & 31);
  uint32_t v = 0u;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint32_t nib = ((z >> k) & 1u) ? (((b >> k) & 1u) ? 0x2u : 0xAu) : 0u;
    v |= nib << (4 * k);
  }
  w4[d] = v;
}

// Input pixels between the window centres of the first and the last pixel of any run of `tp` output pixels, at most:
// (tp - 1) steps of `s`, plus what a change of row and a change of image add beyond such a step.
long long centre_span(const ConvP& p, int tp) {
  const long long s = p.sw, k = tp - 1, hw = (long long)p.Ho * p.Wo;
  const long long row_extra = (long long)p.sh * p.Wd - (long long)p.Wo * s;
  const long long img_extra = (long long)p.H * p.Wd - (long long)p.Ho * p.sh * p.Wd;
  return k * s + (k + p.Wo - 1) / p.Wo * (row_extra > 0 ? row_extra : 0) + (k + hw - 1) / hw * (img_extra > 0 ? img_extra : 0);
}

size_t lds_bytes_of(int patch_cap) {
  const size_t patch = (size_t)(patch_cap + 1) * 64;
  return patch > (size_t)kAccBytes ? patch : (size_t)kAccBytes;
}

// The tile of a launch: 256 pixels x 64 channels where only 64 channels exist or the patch of 128 pixels would not be
// smaller anyway; 128 x 128 (half the weight traffic per pixel) otherwise.  0: no tile fits the LDS.
// `park`: LDS the launch needs behind the patch (the folded shortcut's parked dots); such a launch may ask for more than
// the default 64 KB, up to half the CU's LDS: two workgroups per CU either way.
int choose_tile(const ConvP& p, int* patch_cap, size_t park = 0) {
  const size_t lds_max = park ? (size_t)kMaxLdsFold : (size_t)kMaxLds;
  const int order[2] = {(p.O % 128 == 0 && p.C >= 128) ? 128 : 256, (p.O % 128 == 0 && p.C >= 128) ? 256 : 128};
  for (int tp : order) {
    if (tp == 128 && p.O % 128 != 0) continue;
    const long long cap = centre_span(p, tp) + 2LL * p.Wd + 3;
    if (cap <= kPatchSlots * kMfmaThreads && lds_bytes_of((int)cap) + park <= lds_max) {
      *patch_cap = (int)cap;
      return tp;
    }
  }
  return 0;
}

template <int EP, bool F4>
void launch_ep(const ConvP& p, const Geo& g, const MfmaGeo& mg, const void* w8, dim3 grid, size_t ldsb, hipStream_t s) {
  hipLaunchKernelGGL((bconv_mfma_kernel<EP, false, F4>), grid, dim3(kMfmaThreads), ldsb, s, p.P, p.M,
                     static_cast<const int8_t*>(w8), BNN_EPI_ACTUALS, g, mg, static_cast<const uint32_t*>(nullptr),
                     static_cast<const int8_t*>(nullptr), static_cast<const float*>(nullptr),
                     static_cast<const float*>(nullptr), static_cast<const float*>(nullptr));
}

}  // namespace

size_t weight_i8_bytes(int O, int C, int KH, int KW) {
  if (O <= 0 || C <= 0 || KH != 3 || KW != 3 || O % 64 != 0 || C % 64 != 0) return 0;
  return (size_t)O * (size_t)C * 9;
}

int launch_pack_weight_i8(const uint32_t* wbits, const uint32_t* wnz, const bnn_hip_wlayout& L, int O, void* w8,
                          hipStream_t s) {
  const size_t dwords = (size_t)O * (L.cw32 >> 1) * L.taps * 16;
  hipLaunchKernelGGL(pack_weight_i8_kernel, dim3((unsigned)((dwords + 255) / 256)), dim3(256), 0, s, wbits, wnz, O, L.taps,
                     L.cw32, L.cwc, static_cast<uint32_t*>(w8));
  return hipGetLastError() == hipSuccess ? BNN_HIP_OK : BNN_HIP_ERR_LAUNCH;
}

size_t weight_f4_bytes(int O, int C, int KH, int KW) {
  if (weight_i8_bytes(O, C, KH, KW) == 0 || C % 128 != 0) return 0;
  return (size_t)O * (size_t)C * 9 / 2;
}

int launch_pack_weight_f4(const uint32_t* wbits, const uint32_t* wnz, const bnn_hip_wlayout& L, int O, void* w4,
                          hipStream_t s) {
  const size_t dwords = (size_t)O * (L.cw32 >> 2) * L.taps * 16;  // (taps = 1: the pack of bconv1x1_mfma.hip)
  hipLaunchKernelGGL(pack_weight_f4_kernel, dim3((unsigned)((dwords + 255) / 256)), dim3(256), 0, s, wbits, wnz, O, L.taps,
                     L.cw32, L.cwc, static_cast<uint32_t*>(w4));
  return hipGetLastError() == hipSuccess ? BNN_HIP_OK : BNN_HIP_ERR_LAUNCH;
}

size_t shortcut_weight_i8_bytes(int O, int C) {
  if (O <= 0 || O % 64 != 0 || (C != 64 && C != 128 && C != 256)) return 0;
  return (size_t)O * (size_t)C;
}

int launch_pack_shortcut_weight_i8(const uint32_t* wbits, int O, int C, void* w8, hipStream_t s) {
  // the dense layout of a 1x1 weight of these widths is [o][C / 32] words: one chunk (bnn_hip_weight_layout)
  const int cw32 = C / 32;
  const size_t dwords = (size_t)O * (cw32 >> 1) * 16;
  hipLaunchKernelGGL(pack_weight_i8_kernel, dim3((unsigned)((dwords + 255) / 256)), dim3(256), 0, s, wbits,
                     static_cast<const uint32_t*>(nullptr), O, 1, cw32, cw32, static_cast<uint32_t*>(w8));
  return hipGetLastError() == hipSuccess ? BNN_HIP_OK : BNN_HIP_ERR_LAUNCH;
}

namespace {
// The dense rule both forms share; `park`: choose_tile.
bool mfma_dense_rule(const ConvP& p, int flags, size_t park) {
  if (flags & BNN_HIP_FLAG_FORCE_GENERIC) return false;
  if (p.KH != 3 || p.KW != 3 || p.ph != 1 || p.pw != 1 || p.dh != 1 || p.dw != 1) return false;
  if (p.sh != p.sw || (p.sh != 1 && p.sh != 2)) return false;
  if (p.C % 64 != 0 || p.O % 64 != 0 || !small_indices(p)) return false;
  if (p.raw || p.prelu || p.pack_a || p.pack_b || p.eflags != 0) return false;
  if (p.c_off != 0 || p.c_tot != p.O) return false;
  if ((long long)p.N * p.H * p.Wd >= (1ll << 30)) return false;
  int cap = 0;
  return choose_tile(p, &cap, park) != 0;
}
}  // namespace

// What the kernel covers, stated once (capi.hip asks here for the launch and for bnn_hip_bconv2d_mfma_supported).
bool mfma_conv_applies(const ConvP& p, int flags) { return !p.ds_P && mfma_dense_rule(p, flags, 0); }

// The same for the folded-shortcut form (bnn_hip_bconv2d_mfma_fold_supported): the dense rule; BN + shortcut + ReLU ->
// fp32 + sign planes (kFlagsOut) and nothing else; non-negative activations (the shortcut operand is a P plane); no zero
// weights (the shortcut pack has none); a shortcut of 64, 128 or 256 channels (1, 2 or 4 k-steps); the patch and the
// parked dots within half the CU's LDS.
bool mfma_fold_applies(const ConvP& p, int flags) {
  if (!p.ds_P || p.res || p.thr) return false;
  if (!(flags & BNN_HIP_FLAG_ACT_NONNEG) || (flags & BNN_HIP_FLAG_WEIGHT_ZEROS)) return false;
  if (shortcut_weight_i8_bytes(p.O, p.ds_C) == 0) return false;
  if (make_geo(p).flags != kFlagsOut) return false;
  return mfma_dense_rule(p, flags, (size_t)kParkBytes);
}

// The FP4 forms (bnn_hip_bconv2d_mfma4_supported / _fold_supported): the dense rule, or the fold rule, plus whole
// 128-channel groups.
bool mfma4_conv_applies(const ConvP& p, int flags) { return p.C % 128 == 0 && mfma_conv_applies(p, flags); }
bool mfma4_fold_applies(const ConvP& p, int flags) { return p.C % 128 == 0 && mfma_fold_applies(p, flags); }

namespace {
MfmaGeo make_mfma_geo(const ConvP& p, int flags, int tp, int cap) {
  MfmaGeo mg;
  mg.tp = tp;
  mg.groups = p.C / 64;
  mg.ihw = p.H * p.Wd;
  mg.patch_cap = cap;
  mg.nn = (flags & BNN_HIP_FLAG_ACT_NONNEG) ? 1 : 0;
  mg.n_in = p.N * p.H * p.Wd;
  div_magic((uint32_t)mg.ihw, mg.m_ihw, mg.s_ihw);
  mg.park_off = (int)lds_bytes_of(cap);
  return mg;
}
}  // namespace

int launch_bconv_mfma_fold(const ConvP& p, int flags, const void* w8, const void* sc_w8, hipStream_t s, bool f4) {
  int cap = 0;
  const int tp = choose_tile(p, &cap, (size_t)kParkBytes);
  if (!(f4 ? mfma4_fold_applies(p, flags) : mfma_fold_applies(p, flags)) || tp == 0) return BNN_HIP_ERR_UNSUPPORTED;
  const Geo g = make_geo(p);
  const MfmaGeo mg = make_mfma_geo(p, flags, tp, cap);
  const dim3 grid((unsigned)((p.npix + tp - 1) / tp), (unsigned)(p.O / (tp == 256 ? 64 : 128)));
  const size_t ldsb = lds_bytes_of(cap) + (size_t)kParkBytes;  // above the 64 KB default
  auto kern = f4 ? bconv_mfma_kernel<EP_OUT, true, true> : bconv_mfma_kernel<EP_OUT, true>;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                          kMaxDynamicLds) != hipSuccess)
    return BNN_HIP_ERR_LAUNCH;
  hipLaunchKernelGGL(kern, grid, dim3(kMfmaThreads), ldsb, s, p.P, p.M, static_cast<const int8_t*>(w8), BNN_EPI_ACTUALS, g,
                     mg, p.ds_P, static_cast<const int8_t*>(sc_w8), p.ds_alpha, p.ds_a, p.ds_b);
  return hipGetLastError() == hipSuccess ? BNN_HIP_OK : BNN_HIP_ERR_LAUNCH;
}

namespace {
template <bool F4>
void launch_dense(const ConvP& p, const Geo& g, const MfmaGeo& mg, const void* w8, dim3 grid, size_t ldsb, hipStream_t s) {
  const int f = g.flags;
  const bool fused = (f & (EF_BN | EF_RES | EF_RELU | EF_PACK)) != 0;
  if (f == kFlagsMid && p.thr) launch_ep<EP_MIDT, F4>(p, g, mg, w8, grid, ldsb, s);
  else if (f == kFlagsMid) launch_ep<EP_MID, F4>(p, g, mg, w8, grid, ldsb, s);
  else if (f == kFlagsOut) launch_ep<EP_OUT, F4>(p, g, mg, w8, grid, ldsb, s);
  else if (f == kFlagsOutP) launch_ep<EP_OUTP, F4>(p, g, mg, w8, grid, ldsb, s);
  else if (f == kFlagsLast) launch_ep<EP_LAST, F4>(p, g, mg, w8, grid, ldsb, s);
  else if (fused) launch_ep<EP_RUNTIME, F4>(p, g, mg, w8, grid, ldsb, s);
  else launch_ep<EP_PLAIN, F4>(p, g, mg, w8, grid, ldsb, s);
}
}  // namespace

int launch_bconv_mfma(const ConvP& p, int flags, const void* w8, hipStream_t s, bool f4) {
  int cap = 0;
  const int tp = choose_tile(p, &cap);
  if (!(f4 ? mfma4_conv_applies(p, flags) : mfma_conv_applies(p, flags)) || tp == 0) return BNN_HIP_ERR_UNSUPPORTED;
  const Geo g = make_geo(p);
  const MfmaGeo mg = make_mfma_geo(p, flags, tp, cap);
  const dim3 grid((unsigned)((p.npix + tp - 1) / tp), (unsigned)(p.O / (tp == 256 ? 64 : 128)));
  const size_t ldsb = lds_bytes_of(cap);
  if (f4) launch_dense<true>(p, g, mg, w8, grid, ldsb, s);
  else launch_dense<false>(p, g, mg, w8, grid, ldsb, s);
  return hipGetLastError() == hipSuccess ? BNN_HIP_OK : BNN_HIP_ERR_LAUNCH;
}

}  // namespace bnn

// blinear.hip — the binary fully-connected layer as GEMM-shaped kernels: forward from the float input, input gradient
// and weight gradient (reference: bnn/layers/linear.py:22-27, its autograd graph with the straight-through estimator of
// bnn/ops.py:68-73).  Every kernel sees a row-major [M, F] input (leading dimensions are flattened by the host).
//
//     forward:  out[m, o]   = fmaf(alpha[o], dot(sign(x[m, :]), sign(Wc[o, :])), bias[o]) [* post_scale[o]]
//     dgrad  :  gx[m, f]    = (sum_o g[m, o] alpha[o] sign(Wc)[o, f]) * 1[|x[m, f]| < 1]
//     wgrad  :  part[s,o,f] = sum over the rows m of split s of g[m, o] sign(x)[m, f]
//
// Forward.  Decomposition "lanes = rows": a workgroup owns 64 rows of x.  Stage 1 binarises them: a wave reads 64
// consecutive floats of a row (one coalesced 256-byte load), the ballots of x > 0 / x < 0 (/ |x| < 1) ARE the row's
// 64-bit plane words (no bit-by-bit assembly as in the NCHW packers), lane 0 puts them into LDS word-major ([word][row]:
// the transposition costs nothing) and — optional outputs — into the P / M / T planes of the training step, the layout
// of bnn_hip_pack_act_ste_f32 with H = W = 1.  Stage 2 is the convolution kernels' own inner loop: lane = row keeps its
// words of a chunk in registers, the packed 1x1 weight (bnn_hip_pack_weight_f32: runs of 32 channels x cwc words) streams
// through the scalar cache (stream_weights of bconv_core.h: the same integer expression), 32 int32 accumulators per
// lane, one 32-channel block per wave at a time; the waves of the workgroup share the LDS planes and walk the
// workgroup's channel blocks, so a row tile is binarised once per `obs_per_block` blocks.  Epilogue: the conv
// epilogue's float operations, then a transposition through LDS so that the [M, O] stores are runs of 16 channels (the
// 1x1-image route stores one float per lane with a stride of O floats).
// F that does not fit the LDS pass (128 words = 4096 features by default) is walked in passes; a workgroup then owns at
// most one channel block per wave, whose accumulators live across the passes.
//
// Gradients.  The arithmetic class of csrc/grad.hip (csrc/tgemm.h): the real operand (g' = alpha[o] g, rounded once in
// fp32; g for the weight gradient) is split into three bf16 terms hi + mid + lo (truncations: 24 mantissa bits, fp32 exponent range),
// the ternary operand is exact in bf16, three bf16 MFMAs (tg::mfma3) per product, fp32 accumulation, smallest term
// first.  Both kernels decode their ternary fragments from BITS: dgrad from the forward's own weight pack (sign bit +
// non-zero mask: no second packing launch, 1/16 of the bytes of bf16 fragments), wgrad from the P / M planes; the STE
// mask is read from the T plane at the store.  A 64 x 32 tile of the real operand is split once per k-step by the whole
// workgroup and shared through LDS; a wave owns 64 x 64 outputs (16 accumulator tiles).
#include "tgemm.h"

namespace bnn {
namespace blin {

constexpr int ROWS = 64;        // rows of x per workgroup of the forward (lane = row in the popcount stage); 4 x 8 waves divide it
constexpr int SHALF = 17;       // floats per row of the output staging tile: 16 channels + 1 pad (conflict-free both ways)
constexpr int PASS_WORDS = 128; // default 32-bit words per row and plane of one LDS pass (64 KB of planes)
constexpr int APAD = 40;        // gradient kernels: 16-bit containers per row of the 64 x 32 real-operand tile (80 B)
constexpr int NB = 4;           // gradient kernels: 16-column tiles per wave

using namespace tg;

// ------------------------------------------------------------------------------------------------- forward
template <typename XT, int CWC, bool WZ>
__global__ __launch_bounds__(512) void blinear_fwd_kernel(const XT* __restrict__ x, const uint32_t* __restrict__ wbits,
                                                          const uint32_t* __restrict__ wnz,
                                                          const float* __restrict__ alpha, const float* __restrict__ bias,
                                                          const float* __restrict__ scale, float* __restrict__ out,
                                                          uint64_t* __restrict__ oP, uint64_t* __restrict__ oM,
                                                          uint64_t* __restrict__ oT, int M, int F, int O, int nchunk,
                                                          int sc_chunks, int obs_per_block) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nwaves = (int)(blockDim.x >> 6);
  const int scw = sc_chunks * CWC;                   // 32-bit words per row and plane of one LDS pass
  uint32_t* sP = reinterpret_cast<uint32_t*>(lds_raw);   // [scw][64 rows]
  uint32_t* sM = sP + scw * ROWS;
  float* stage = reinterpret_cast<float*>(sM + scw * ROWS) + wave * (ROWS * SHALF);
  const int row0 = blockIdx.x * ROWS;
  const int cw64 = (nchunk * CWC) >> 1;
  const int nob = (O + kOCB - 1) / kOCB;
  const int ob_begin = blockIdx.y * obs_per_block;
  const int ob_end = min(nob, ob_begin + obs_per_block);
  const int nsc = (nchunk + sc_chunks - 1) / sc_chunks;        // LDS passes over F
  const int npass = (obs_per_block + nwaves - 1) / nwaves;     // (the host keeps npass == 1 when nsc > 1)
  const bool planes = oP != nullptr && blockIdx.y == 0;

  // stage 1: the plane words of LDS pass `sc` for the workgroup's 64 rows (rows past M and features past F: zeros)
  auto binarise = [&](int sc) __attribute__((always_inline)) {
    const int k0 = (sc * scw) >> 1, k1 = min(cw64, k0 + (scw >> 1));
    // four rows per iteration (ROWS is a multiple of 4 x the waves of either workgroup size): their loads are in flight
    // together, a row at a time the loop waits out one memory round trip per 64 features
    for (int r = wave; r < ROWS; r += 4 * nwaves) {
      const XT* xr[4];
      bool rok[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        rok[j] = row0 + r + j * nwaves < M;
        xr[j] = x + (size_t)(rok[j] ? row0 + r + j * nwaves : 0) * F;
      }
      for (int k = k0; k < k1; ++k) {
        const int col = 64 * k + lane;
        float xv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) xv[j] = (float)xr[j][col < F ? col : 0];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int rj = r + j * nwaves;
          const bool ok = rok[j] && col < F;
          const float v = ok ? xv[j] : 0.0f;
          const unsigned long long p = __ballot(is_pos(v)), m = __ballot(is_neg(v));
          const unsigned long long t = __ballot(ok && fabsf(v) < 1.0f);
          if (lane == 0) {
            const int w = 2 * (k - k0);
            sP[w * ROWS + rj] = (uint32_t)p;
            sP[(w + 1) * ROWS + rj] = (uint32_t)(p >> 32);
            sM[w * ROWS + rj] = (uint32_t)m;
            sM[(w + 1) * ROWS + rj] = (uint32_t)(m >> 32);
            if (planes && rok[j]) {
              const size_t pw = (size_t)(row0 + rj) * cw64 + k;
              oP[pw] = p;
              oM[pw] = m;
              oT[pw] = t;
            }
          }
        }
      }
    }
  };

  for (int pass = 0; pass < npass; ++pass) {
    const int ob = ob_begin + pass * nwaves + wave;      // wave-uniform
    const bool active = ob < ob_end;
    int acc[kOCB];
    [[maybe_unused]] int nzacc[kOCB];
    int nz = 0;
#pragma unroll
    for (int j = 0; j < kOCB; ++j) {
      acc[j] = 0;
      if constexpr (WZ) nzacc[j] = 0;
    }
    for (int sc = 0; sc < nsc; ++sc) {
      if (nsc > 1 || pass == 0) {
        __syncthreads();          // the previous pass's words are consumed
        binarise(sc);
        __syncthreads();
      }
      if (active) {
        const int ch0 = sc * sc_chunks, ch1 = min(nchunk, ch0 + sc_chunks);
        for (int ch = ch0; ch < ch1; ++ch) {
          uint32_t pr[CWC], mr[CWC];
#pragma unroll
          for (int i = 0; i < CWC; ++i) {
            pr[i] = sP[((ch - ch0) * CWC + i) * ROWS + lane];
            mr[i] = sM[((ch - ch0) * CWC + i) * ROWS + lane];
          }
          const size_t woff = ((size_t)ob * nchunk + ch) * kOCB * CWC;
          if constexpr (WZ) {
            stream_weights_wz<CWC, kOCB>(wbits + woff, wnz + woff, pr, mr, acc, nzacc);
          } else {
            nz = count_nonzero<CWC>(pr, mr, nz);
            stream_weights<CWC, kOCB>(wbits + woff, pr, mr, acc);
          }
        }
      }
    }
    if (active) {
      // dot = non-zeros - 2 * disagreements; y = fmaf(alpha, dot, bias) [* scale]: the conv epilogue's operations
      const int o0 = ob * kOCB;
      const bool hb = bias != nullptr, hs = scale != nullptr;
      float y[kOCB];
#pragma unroll
      for (int j = 0; j < kOCB; ++j) {
        const int o = o0 + j;
        const int dot = WZ ? nzacc[j] - 2 * acc[j] : nz - 2 * acc[j];
        float v = 0.0f;
        if (o < O) {
          v = fmaf(alpha[o], (float)dot, hb ? bias[o] : 0.0f);
          if (hs) v *= scale[o];
        }
        y[j] = v;
      }
      // [row = lane][32 channels] -> stores of 16 consecutive channels per row, through the wave's own LDS tile
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int j = 0; j < 16; ++j) stage[lane * SHALF + j] = y[16 * h + j];
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int r = 4 * i + (lane >> 4), c = lane & 15;
          const float v = stage[r * SHALF + c];
          const int row = row0 + r, o = o0 + 16 * h + c;
          if (row < M && o < O) out[(size_t)row * O + o] = v;
        }
      }
    }
  }
}

template <typename XT, int CWC, bool WZ>
static int launch_fwd_t(const void* x, const uint32_t* wbits, const uint32_t* wnz, const float* alpha, const float* bias,
                        const float* scale, float* out, uint64_t* P, uint64_t* Mn, uint64_t* T, int M, int F, int O,
                        int nchunk, int lds_words, hipStream_t s) {
  int sc_chunks = (lds_words > 0 ? lds_words : PASS_WORDS) / CWC;
  if (sc_chunks < 1) sc_chunks = 1;
  if (sc_chunks > nchunk) sc_chunks = nchunk;
  const int nsc = (nchunk + sc_chunks - 1) / sc_chunks;
  const size_t plane_bytes = (size_t)2 * sc_chunks * CWC * ROWS * sizeof(uint32_t);
  const int nwaves = plane_bytes > 32 * 1024 ? 8 : 4;
  const int nob = (O + kOCB - 1) / kOCB, tiles = (M + ROWS - 1) / ROWS;
  int obs_per_block = nwaves;
  if (nsc == 1) {
    // a row tile is binarised once per workgroup: as many channel blocks per workgroup as still leave ~2 workgroups per CU
    long long gy = (2LL * current_device_cus() + tiles - 1) / tiles;
    const long long gy_max = (nob + nwaves - 1) / nwaves;
    if (gy > gy_max) gy = gy_max;
    if (gy < 1) gy = 1;
    obs_per_block = (int)((nob + gy - 1) / gy);
    obs_per_block = (obs_per_block + nwaves - 1) / nwaves * nwaves;
  }
  const long long gy = (nob + obs_per_block - 1) / obs_per_block;
  if (gy > 65535) return BNN_HIP_ERR_UNSUPPORTED;
  const size_t lds = plane_bytes + (size_t)nwaves * ROWS * SHALF * sizeof(float);
  auto kern = blinear_fwd_kernel<XT, CWC, WZ>;
  if (lds > 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                            kMaxDynamicLds) != hipSuccess)
    return BNN_HIP_ERR_LAUNCH;
  hipLaunchKernelGGL(kern, dim3((unsigned)tiles, (unsigned)gy), dim3(64 * nwaves), lds, s, static_cast<const XT*>(x), wbits,
                     wnz, alpha, bias, scale, out, P, Mn, T, M, F, O, nchunk, sc_chunks, obs_per_block);
  return hipGetLastError() == hipSuccess ? BNN_HIP_OK : BNN_HIP_ERR_LAUNCH;
}

template <typename XT, bool WZ>
static int launch_fwd_c(int cwc, const void* x, const uint32_t* wbits, const uint32_t* wnz, const float* alpha,
                        const float* bias, const float* scale, float* out, uint64_t* P, uint64_t* Mn, uint64_t* T, int M,
                        int F, int O, int nchunk, int lds_words, hipStream_t s) {
  switch (cwc) {
    case 16: return launch_fwd_t<XT, 16, WZ>(x, wbits, wnz, alpha, bias, scale, out, P, Mn, T, M, F, O, nchunk, lds_words, s);
    case 8: return launch_fwd_t<XT, 8, WZ>(x, wbits, wnz, alpha, bias, scale, out, P, Mn, T, M, F, O, nchunk, lds_words, s);
    case 4: return launch_fwd_t<XT, 4, WZ>(x, wbits, wnz, alpha, bias, scale, out, P, Mn, T, M, F, O, nchunk, lds_words, s);
    case 2: return launch_fwd_t<XT, 2, WZ>(x, wbits, wnz, alpha, bias, scale, out, P, Mn, T, M, F, O, nchunk, lds_words, s);
    default: return BNN_HIP_ERR_UNSUPPORTED;
  }
}

// ------------------------------------------------------------------------------------------------- input gradient
// GEMM: rows m (64 per workgroup), columns f (64 NB per workgroup, 16 NB per wave), K = o in steps of 32 (one block of the
// weight pack).  Per step: g' = alpha[o] g of the 64 x 32 tile -> three bf16 planes in LDS (thread t: row t / 4, eight
// consecutive o); a wave decodes its NB ternary fragments from the pack — lane (li, lg) of a fragment holds
// sign(Wc)[o = 32 ob + 8 lg + e][f = f0 + li], bit (f & 31) of word f / 32 of channel o — and runs 4 x NB x 3 MFMAs.
__global__ __launch_bounds__(256) void blinear_dgrad_kernel(const float* __restrict__ g, const float* __restrict__ alpha,
                                                            const uint32_t* __restrict__ wbits,
                                                            const uint32_t* __restrict__ wnz,
                                                            const uint32_t* __restrict__ T32, float* __restrict__ gx,
                                                            int M, int O, int F, int cwc, int nchunk) {
  __shared__ __attribute__((aligned(16))) u16 a_hi[64 * APAD];
  __shared__ __attribute__((aligned(16))) u16 a_mid[64 * APAD];
  __shared__ __attribute__((aligned(16))) u16 a_lo[64 * APAD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
  const int row0 = blockIdx.x * 64, f_blk = blockIdx.y * (64 * NB) + wave * (16 * NB);
  const int cw32 = cwc * nchunk, OB = (O + 31) / 32;

  f32x4 acc[4][NB];
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[rt][nb] = f32x4{0.f, 0.f, 0.f, 0.f};

  // fill role: row tid / 4 of the tile, output channels 8 (tid & 3) .. + 7 of the step
  const int frow = tid >> 2, fkg = tid & 3;
  const bool frok = row0 + frow < M;
  const float* grow = g + (size_t)(frok ? row0 + frow : 0) * O;
  // fragment role: word offset of (channel 8 lg, this tile's word) inside one 32-channel block of the pack, and the bit
  unsigned boff[NB], bsh[NB];
  bool bok[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int f0 = f_blk + 16 * nb, w32 = f0 >> 5;
    bok[nb] = w32 < cw32;
    const int w = bok[nb] ? w32 : 0, ch = w / cwc, cw = w - ch * cwc;
    boff[nb] = (unsigned)((ch * 32 + 8 * lg) * cwc + cw);
    bsh[nb] = (unsigned)((f0 & 31) + li);
  }

  for (int ob = 0; ob < OB; ++ob) {
    __syncthreads();   // the previous step's tile is consumed
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int o = 32 * ob + 8 * fkg + e;
      const bool ok = frok && o < O;
      float t = grow[ok ? o : 0] * alpha[ok ? o : 0];   // rounded once in fp32
#if defined(__HIP_DEVICE_COMPILE__)
      asm volatile("" : "+v"(t));                       // (the product itself is split: no contraction into the remainders)
#endif
      v[e] = ok ? t : 0.0f;
    }
    bf16x8 hi, mid, lo;
    split3(v, hi, mid, lo);
    *reinterpret_cast<bf16x8*>(a_hi + frow * APAD + 8 * fkg) = hi;
    *reinterpret_cast<bf16x8*>(a_mid + frow * APAD + 8 * fkg) = mid;
    *reinterpret_cast<bf16x8*>(a_lo + frow * APAD + 8 * fkg) = lo;
    bf16x8 b[NB];
    const size_t wblk = (size_t)ob * 32 * cw32;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      unsigned code[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const size_t wi = wblk + boff[nb] + (size_t)e * cwc;
        const unsigned wb = wbits[wi], wz = wnz[wi];
        const bool nzb = bok[nb] && ((wz >> bsh[nb]) & 1u), bit = (wb >> bsh[nb]) & 1u;
        code[e] = nzb ? ternary_code(bit, !bit) : (u16)0;
      }
      b[nb] = pack_codes(code);
    }
    __syncthreads();
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) {
      const int ao = (16 * rt + li) * APAD + 8 * lg;
      const bf16x8 ah = *reinterpret_cast<const bf16x8*>(a_hi + ao);
      const bf16x8 am = *reinterpret_cast<const bf16x8*>(a_mid + ao);
      const bf16x8 al = *reinterpret_cast<const bf16x8*>(a_lo + ao);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[rt][nb] = mfma3(ah, am, al, b[nb], acc[rt][nb]);
    }
  }
  // D layout: column = li (feature within the tile), row = 4 lg + r; the STE mask is bit f of row m of the T plane
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const int f = f_blk + 16 * nb + li;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = row0 + 16 * rt + 4 * lg + r;
        if (row < M && f < F) {
          const unsigned tw = T32[(size_t)row * cw32 + (f >> 5)];
          gx[(size_t)row * F + f] = ((tw >> (f & 31)) & 1u) ? acc[rt][nb][r] : 0.0f;
        }
      }
    }
}

// ------------------------------------------------------------------------------------------------- weight gradient
// GEMM: rows o (64 per workgroup), columns f (64 NB per workgroup, 16 NB per wave), K = the rows m of the split in steps
// of 32.  Per step: g[m, o] of the 32 x 64 tile -> three bf16 planes in LDS, [o][m] (thread t: channel t & 63, rows
// 8 (t >> 6) .. + 7: every load instruction reads 64 consecutive floats of one row); a wave decodes sign(x)[m = m0 + 8 lg
// + e][f = f0 + li] from the P / M plane words of its columns (one word pair serves two 16-column tiles).
__global__ __launch_bounds__(256) void blinear_wgrad_kernel(const float* __restrict__ g, const uint32_t* __restrict__ P32,
                                                            const uint32_t* __restrict__ M32, float* __restrict__ part,
                                                            int M, int O, int F, int cw32, int per) {
  static_assert(NB % 2 == 0, "two tiles per plane word");
  __shared__ __attribute__((aligned(16))) u16 a_hi[64 * APAD];
  __shared__ __attribute__((aligned(16))) u16 a_mid[64 * APAD];
  __shared__ __attribute__((aligned(16))) u16 a_lo[64 * APAD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
  const int o0 = blockIdx.z * 64, f_blk = blockIdx.y * (64 * NB) + wave * (16 * NB);
  const int m_begin = blockIdx.x * per, m_end = min(M, m_begin + per);

  f32x4 acc[4][NB];
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[rt][nb] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int fo = tid & 63, fmg = tid >> 6;
  const bool fok = o0 + fo < O;
  const int foc = fok ? o0 + fo : 0;
  int wc[NB / 2];
#pragma unroll
  for (int h = 0; h < NB / 2; ++h) {
    const int w32 = (f_blk + 32 * h) >> 5;
    wc[h] = w32 < cw32 ? w32 : cw32 - 1;     // (columns past F are never stored)
  }

  for (int m0 = m_begin; m0 < m_end; m0 += 32) {
    __syncthreads();   // the previous step's tile is consumed
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int m = m0 + 8 * fmg + e;
      const bool ok = fok && m < m_end;
      const float t = g[(size_t)(ok ? m : m_begin) * O + foc];
      v[e] = ok ? t : 0.0f;
    }
    bf16x8 hi, mid, lo;
    split3(v, hi, mid, lo);
    *reinterpret_cast<bf16x8*>(a_hi + fo * APAD + 8 * fmg) = hi;
    *reinterpret_cast<bf16x8*>(a_mid + fo * APAD + 8 * fmg) = mid;
    *reinterpret_cast<bf16x8*>(a_lo + fo * APAD + 8 * fmg) = lo;
    bf16x8 b[NB];
#pragma unroll
    for (int h = 0; h < NB / 2; ++h) {
      unsigned c0[8], c1[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int m = m0 + 8 * lg + e;
        // (rows past the split's end meet g = 0: any row of the split stands in for them)
        const size_t wi = (size_t)(m < m_end ? m : m_begin) * cw32 + wc[h];
        const unsigned pw = P32[wi], mw = M32[wi];
        c0[e] = ternary_code((pw >> li) & 1u, (mw >> li) & 1u);
        c1[e] = ternary_code((pw >> (16 + li)) & 1u, (mw >> (16 + li)) & 1u);
      }
      b[2 * h] = pack_codes(c0);
      b[2 * h + 1] = pack_codes(c1);
    }
    __syncthreads();
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) {
      const int ao = (16 * rt + li) * APAD + 8 * lg;
      const bf16x8 ah = *reinterpret_cast<const bf16x8*>(a_hi + ao);
      const bf16x8 am = *reinterpret_cast<const bf16x8*>(a_mid + ao);
      const bf16x8 al = *reinterpret_cast<const bf16x8*>(a_lo + ao);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[rt][nb] = mfma3(ah, am, al, b[nb], acc[rt][nb]);
    }
  }
  // D layout: column = li (feature within the tile), row = 4 lg + r (output channel within the 16-row tile)
  float* dst = part + (size_t)blockIdx.x * O * F;
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const int f = f_blk + 16 * nb + li;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int o = o0 + 16 * rt + 4 * lg + r;
        if (o < O && f < F) dst[(size_t)o * F + f] = acc[rt][nb][r];
      }
    }
}

}  // namespace blin

// ------------------------------------------------------------------------------------------------- host side
int launch_blinear_fwd(const void* x, int x_dtype, const uint32_t* wbits, const uint32_t* wnz, int weight_zeros,
                       const float* alpha, const float* bias, const float* scale, float* out, uint64_t* P, uint64_t* Mn,
                       uint64_t* T, int M, int F, int O, int lds_words, hipStream_t s) {
  const int cw32 = 2 * ((F + 63) / 64), cwc = choose_cwc(cw32, 1, 1), nchunk = cw32 / cwc;
  if (x_dtype == BNN_HIP_DTYPE_BF16) {  // (float)__bf16 is the exact widening: the same planes
    return weight_zeros ? blin::launch_fwd_c<__bf16, true>(cwc, x, wbits, wnz, alpha, bias, scale, out, P, Mn, T, M, F, O,
                                                           nchunk, lds_words, s)
                        : blin::launch_fwd_c<__bf16, false>(cwc, x, wbits, wnz, alpha, bias, scale, out, P, Mn, T, M, F, O,
                                                            nchunk, lds_words, s);
  }
  if (x_dtype == BNN_HIP_DTYPE_F16) {
    return weight_zeros ? blin::launch_fwd_c<_Float16, true>(cwc, x, wbits, wnz, alpha, bias, scale, out, P, Mn, T, M, F, O,
                                                             nchunk, lds_words, s)
                        : blin::launch_fwd_c<_Float16, false>(cwc, x, wbits, wnz, alpha, bias, scale, out, P, Mn, T, M, F, O,
                                                              nchunk, lds_words, s);
  }
  return weight_zeros ? blin::launch_fwd_c<float, true>(cwc, x, wbits, wnz, alpha, bias, scale, out, P, Mn, T, M, F, O, nchunk,
                                                        lds_words, s)
                      : blin::launch_fwd_c<float, false>(cwc, x, wbits, wnz, alpha, bias, scale, out, P, Mn, T, M, F, O,
                                                         nchunk, lds_words, s);
}

int launch_blinear_dgrad(const float* g, const float* alpha, const uint32_t* wbits, const uint32_t* wnz, const uint64_t* T,
                         float* gx, int M, int O, int F, hipStream_t s) {
  const int cw32 = 2 * ((F + 63) / 64), cwc = choose_cwc(cw32, 1, 1), nchunk = cw32 / cwc;
  const long long gy = ((long long)F + 64 * blin::NB - 1) / (64 * blin::NB);
  if (gy > 65535) return BNN_HIP_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(blin::blinear_dgrad_kernel, dim3((unsigned)((M + 63) / 64), (unsigned)gy), dim3(256), 0, s, g, alpha,
                     wbits, wnz, reinterpret_cast<const uint32_t*>(T), gx, M, O, F, cwc, nchunk);
  return hipGetLastError() == hipSuccess ? BNN_HIP_OK : BNN_HIP_ERR_LAUNCH;
}

// ~4 workgroups per CU in total, at least 32 rows (one k-step) per split; the result satisfies the rule of the entry
// point: splits == ceil(M / ceil(M / splits))
int blinear_wgrad_splits(int M, int O, int F) {
  const long long blocks = (((long long)O + 63) / 64) * (((long long)F + 64 * blin::NB - 1) / (64 * blin::NB));
  long long s = (1024 + blocks - 1) / blocks;
  const long long steps = ((long long)M + 31) / 32;
  if (s > steps) s = steps;
  if (s > M) s = M;
  if (s < 1) s = 1;
  const long long per = (M + s - 1) / s;
  return (int)((M + per - 1) / per);
}

int launch_blinear_wgrad(const float* g, const uint64_t* P, const uint64_t* Mn, float* part, int splits, int M, int O, int F,
                         hipStream_t s) {
  if (splits < 1 || splits > M) return BNN_HIP_ERR_INVALID_ARG;
  const int per = (M + splits - 1) / splits;
  if ((M + per - 1) / per != splits) return BNN_HIP_ERR_INVALID_ARG;
  const long long gy = ((long long)F + 64 * blin::NB - 1) / (64 * blin::NB), gz = ((long long)O + 63) / 64;
  if (gy > 65535 || gz > 65535) return BNN_HIP_ERR_UNSUPPORTED;
  const int cw32 = 2 * ((F + 63) / 64);
  hipLaunchKernelGGL(blin::blinear_wgrad_kernel, dim3((unsigned)splits, (unsigned)gy, (unsigned)gz), dim3(256), 0, s, g,
                     reinterpret_cast<const uint32_t*>(P), reinterpret_cast<const uint32_t*>(Mn), part, M, O, F, cw32, per);
  return hipGetLastError() == hipSuccess ? BNN_HIP_OK : BNN_HIP_ERR_LAUNCH;
}

}  // namespace bnn

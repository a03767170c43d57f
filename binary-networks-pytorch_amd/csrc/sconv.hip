// sconv.hip — forward of a convolution with BINARY ACTIVATIONS AND REAL WEIGHTS: step 0 of the reference's two-stage
// recipe (examples/recepies/imagenet-baseline.yaml: BasicInputBinarizer, BasicScaleBinarizer, weight: nn.Identity), the
// layer bnn/layers/conv.py:90-97 evaluates as conv2d(sign(x), W, b) * alpha in fp32.
//
//     y[n,o,p] = (sum_{c,tap} s(x)[n,c,p*st + tap - pad] * W[o,c,tap] + bias[o]) * scale[o]
//
// s(x) is the predicate of the bit planes (csrc/pack_act.hip): x > 0 -> +1, x < 0 -> -1, everything else (+-0, NaN, the
// zero padding) -> 0.  The GEMM has one operand that is exactly {-1,0,+1} and one real operand: the arithmetic of
// csrc/grad.hip with the roles swapped — there the image side (g) is real and the weight side ternary, here the image
// side is ternary and the weight side real — as csrc/tgemm.h states it: the real operand in three truncated bf16 terms,
// the ternary operand exact in bf16, three bf16 MFMAs (tg::mfma3) per product with fp32 accumulation: the rounding
// class of an fp32 convolution.
//
// Row exponent.  bf16 has fp32's exponent RANGE but its subnormals end at 2^-133, and the remainder of a weight below
// 2^-110 has bits under that: a plain split of W loses them.  So the packer scales every output channel o whose largest
// |W[o]| is below 1 by 2^kexp[o] (a power of two: exact) so that the largest lies in [1, 2), splits the scaled row, and
// the kernel's epilogue multiplies the accumulator by 2^-kexp[o] (v_ldexp: exact unless the result is subnormal, where it
// rounds once).  Rows with max |W| >= 1, zero rows and rows with a non-finite weight keep kexp = 0.  For every finite
// weight no smaller than 2^-100 of its row's largest (or 2^-100 itself for rows >= 1) hi + mid + lo == W * 2^kexp
// exactly — every finite fp32, subnormals included, when it is the largest of its row.  Infinities and NaN travel in
// `hi` (their remainders are NaN, as in the fp32 product they stand for).
//
// Packed weight (bnn_hip_sconv2d_weight_pack_bytes(O, C, k) bytes, 16-byte aligned), CB = ceil(C/32), OS = ceil(O/16),
// T = k * k:
//
//     Wp[cb][tap][os][term][lane][e]   bf16, term 0 / 1 / 2 = hi / mid / lo   (one 16-byte MFMA B fragment per lane)
//         = term(W[o = 16 os + (lane & 15)][c = 32 cb + 8 (lane >> 4) + e][tap] * 2^kexp[o])
//           and 0 for o >= O or c >= C (pad channels);
//     kexp[16 OS]                      int32, behind the fragments (byte offset CB * T * OS * 3 * 1024); 0 for o >= O.
//
// (tg::real_frag, real_frag_bytes, real_kexp compute these addresses.)
//
// K-slots (tg::Slots) over the OUTPUT grid (Wo <= 64 pixels).  Per workgroup one chunk x 64 NSUB output channels;
// the K loop walks blocks of 32 input channels: the chunk's input patch (rows st*y0 - pad .., halo included) enters LDS
// as ONE bf16 plane of s(x), [patch pixel][32 c] (80 bytes per pixel: conflict-free 16-byte reads), filled by buffer
// loads whose out-of-range offsets ARE the zero padding; k*k taps = k*k k-steps of 32 whose A fragment is the patch
// pixel (st * row + ky, st * column + kx).  Stride 2 reads the same patch at every second pixel.
#include "tgemm.h"

namespace bnn {

using namespace tg;

namespace {

struct SGeo {
  int N, O, C;
  int Hx, Wx;        // input  [N,C,Hx,Wx]
  int Hg, Wg;        // output [N,O,Hg,Wg], Hg = (Hx - 1) / st + 1: the pixel domain the 64-slot chunks tile
  int slot, R;       // pixels per row slot (pow2 >= Wg, >= 8); output rows a chunk holds = min(64 / slot, Hg)
  int chunks;        // chunks per image = ceil(Hg / R)
  int gshift;        // log2(slot / 8)
  unsigned x_bytes, y_bytes;  // ranges of the buffer descriptors of x and y
};

}  // namespace

// ------------------------------------------------------------------------------------------------- weight operand
// kexp[o] for o < 16 OS: 1 - exponent(max |W[o]|) when 0 < max < 1 (so that max * 2^kexp lies in [1, 2)), else 0
// (fmaxf drops NaN; an infinite maximum is >= 1).  One wave per output channel.
__global__ __launch_bounds__(64) void sconv_row_exp_kernel(const float* __restrict__ w, int O, int per_o,
                                                           int* __restrict__ kexp) {
  const int o = blockIdx.x;
  float m = 0.0f;
  if (o < O) {
    const float* p = w + (size_t)o * per_o;
    for (int i = threadIdx.x; i < per_o; i += 64) m = fmaxf(m, fabsf(p[i]));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
  if (threadIdx.x == 0) {
    int k = 0;
    if (m > 0.0f && m < 1.0f) {
      int e;
      (void)frexpf(m, &e);  // m = f * 2^e, f in [0.5, 1)
      k = 1 - e;
    }
    kexp[o] = k;
  }
}

__global__ __launch_bounds__(64) void sconv_pack_weight_kernel(const float* __restrict__ w, int O, int C, int OS, int T,
                                                               const int* __restrict__ kexp, bf16x8* __restrict__ Wp) {
  const int lane = threadIdx.x, li = lane & 15, lg = lane >> 4;
  const int os = blockIdx.x % OS, tap = (blockIdx.x / OS) % T, cb = blockIdx.x / (OS * T);
  const int o = 16 * os + li;
  const int k = kexp[o];  // (written for all 16 OS rows)
  float v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int c = 32 * cb + 8 * lg + e;
    v[e] = (o < O && c < C) ? ldexpf(w[((size_t)o * C + c) * T + tap], k) : 0.0f;
  }
  bf16x8 hi, mid, lo;
  split3(v, hi, mid, lo);
  bf16x8* dst = Wp + real_frag(cb, tap, os, T, OS, lane);
  dst[0] = hi;
  dst[64] = mid;
  dst[128] = lo;
}

// ------------------------------------------------------------------------------------------------- forward
// GEMM: M = output pixels (one 64-slot chunk per workgroup), N = output channels (64 NSUB per workgroup, grid.y blocks),
// K = (c, tap).  2 x 2 register blocking as in dgrad_kernel: a wave owns two of the four 16-pixel sub-tiles and half of
// the workgroup's 4 NSUB channel groups.  FK: 64-pixel sweeps over the patch (stride 1: <= 198 pixels, stride 2: <= 330).
template <int NSUB, int KS, int ST>
__global__ __launch_bounds__(NT) void sconv_kernel(const float* __restrict__ x, const bf16x8* __restrict__ Wp,
                                                   const int* __restrict__ kexp, const float* __restrict__ bias,
                                                   const float* __restrict__ scale, float* __restrict__ y,
                                                   const SGeo q) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  constexpr int PD = KS / 2, T = KS * KS;
  constexpr int FK = ST == 2 ? 6 : 4;
  const int PW = q.Wx + 2 * PD, PR = ST * (q.R - 1) + KS, PP = PR * PW;  // patch width / rows / pixels (halo included)
  u16* pa = reinterpret_cast<u16*>(lds_raw);
  float* stage = reinterpret_cast<float*>(lds_raw);  // reused after the K loop

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lg = lane >> 4;
  const int n = blockIdx.x / q.chunks, y0 = (blockIdx.x - n * q.chunks) * q.R;  // first output row of the chunk
  const int HWx = q.Hx * q.Wx, HWg = q.Hg * q.Wg;
  const int CB = (q.C + 31) / 32, OS = (q.O + 15) / 16;
  constexpr int NB = 2 * NSUB;                       // channel groups (B fragments x 3 terms) per wave
  const int ph = wave & 1, chh = wave >> 1;          // pixel half, channel half
  const int os0 = blockIdx.y * 4 * NSUB + chh * NB;  // first 16-channel group of this wave

  // A-fragment base addresses: output pixel (ry, ox) of the chunk reads patch pixel (ST ry + ky, ST ox + kx) at tap (ky, kx)
  int abase[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) abase[i] = patch_base(16 * (2 * ph + i) + li, q.slot, q.Wg, q.R, PW, ST, 0, lg);

  f32x4 acc[2][NB];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int ns = 0; ns < NB; ++ns) acc[i][ns] = f32x4{0.f, 0.f, 0.f, 0.f};

  // ---- fill roles, once per workgroup: wave w fills input channels 8 w .. 8 w + 7 of every 32-channel block, lane l the
  // patch pixels l, l + 64, ...; the pixel's byte offset inside a channel plane of x (out of range: the zero padding) and
  // its LDS address do not depend on the block.
  const BufRsrc r_x = make_rsrc_sized(x, q.x_bytes);
  unsigned fvoff[FK];
  int flds[FK];
  patch_fill_roles(lane, wave, PW, PP, ST * y0 - PD, -PD, q.Hx, q.Wx, fvoff, flds);
  const unsigned xplane4 = (unsigned)HWx * 4u;

  for (int cb = 0; cb < CB; ++cb) {
    __syncthreads();  // the previous block's patch is consumed
    auto load_w = [&](bf16x8 (&dst)[NB][3], int tap) {
#pragma unroll
      for (int ns = 0; ns < NB; ++ns) {
        const int os = os0 + ns;
        const bf16x8* src = Wp + real_frag(cb, tap, os < OS ? os : 0, T, OS, lane);
#pragma unroll
        for (int t = 0; t < 3; ++t) dst[ns][t] = os < OS ? src[64 * t] : zero_frag();
      }
    };
    bf16x8 b[NB][3];
    load_w(b, 0);
    const int c0 = 32 * cb + 8 * wave;
#pragma unroll
    for (int k = 0; k < FK; ++k) {
      if (64 * k >= PP) break;  // workgroup-uniform
      u16 sv[8];
      unsigned soff = (unsigned)(n * q.C + c0) * xplane4;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        // channels past C: an out-of-range offset reads 0 (a select, not a branch)
        sv[e] = ternary_code(buf_ld(r_x, c0 + e < q.C ? fvoff[k] : kOOB, c0 + e < q.C ? soff : 0u));
        soff += xplane4;
      }
      if (flds[k] >= 0) *reinterpret_cast<bf16x8*>(pa + flds[k]) = pack_codes(sv);
    }
    __syncthreads();
#pragma unroll 1
    for (int tap = 0; tap < T; ++tap) {
      const int ky = tap / KS, kx = tap - ky * KS;
      const int toff = (ky * PW + kx) * APIX;
      // the next tap's weight fragments are requested before this tap's MFMAs (tap 0's before the fill)
      bf16x8 bn[NB][3];
#pragma unroll
      for (int ns = 0; ns < NB; ++ns)
#pragma unroll
        for (int t = 0; t < 3; ++t) bn[ns][t] = b[ns][t];
      if (tap + 1 < T) load_w(bn, tap + 1);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(pa + abase[i] + toff);
#pragma unroll
        for (int ns = 0; ns < NB; ++ns) acc[i][ns] = mfma3(a, b[ns], acc[i][ns]);
      }
#pragma unroll
      for (int ns = 0; ns < NB; ++ns)
#pragma unroll
        for (int t = 0; t < 3; ++t) b[ns][t] = bn[ns][t];
    }
  }
  __syncthreads();  // the patch is dead: its LDS becomes the [channel][pixel] staging tile
  stage_acc(stage, acc, ph, chh, li, lg);
  __syncthreads();
  // a thread keeps ONE pixel of the chunk (its lane) and walks the channels wave, wave + 4, ...: coalesced NCHW stores
  const int o_blk = blockIdx.y * 64 * NSUB;
  constexpr int IT = 16 * NSUB;
  int ery, ex;
  const bool elive = chunk_pixel(lane, q.slot, q.gshift, q.Wg, q.R, y0, q.Hg, ery, ex);
  const unsigned elane = elive ? (unsigned)((y0 + ery) * q.Wg + ex) * 4u : kOOB;
  [[maybe_unused]] const BufRsrc r_y = make_rsrc_sized(y, q.y_bytes);
  const unsigned yplane4 = (unsigned)HWg * 4u;
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int o = o_blk + wave + 4 * i;  // wave-uniform
    float v = stage[(wave + 4 * i) * SROW + lane];
    if (o < q.O) {
      v = ldexpf(v, -kexp[o]);
      if (bias) v = v + bias[o];
      if (scale) v = v * scale[o];
    }
    buf_st(r_y, o < q.O ? elane : kOOB, o < q.O ? (unsigned)(n * q.O + o) * yplane4 : 0u, v);
  }
}

// ------------------------------------------------------------------------------------------------- host side
static bool sconv_ks_ok(int ks, int stride) { return ks == 3 ? (stride == 1 || stride == 2) : (ks == 1 && stride == 1); }

static bool make_sgeo(int N, int O, int C, int Hx, int Wx, int ks, int st, SGeo* q) {
  if (N <= 0 || O <= 0 || C <= 0 || Hx <= 0 || Wx <= 0 || Wx > 64 || !sconv_ks_ok(ks, st)) return false;
  q->N = N; q->O = O; q->C = C; q->Hx = Hx; q->Wx = Wx;
  q->Hg = (Hx - 1) / st + 1;
  q->Wg = (Wx - 1) / st + 1;
  Slots sl;
  if (!make_slots(q->Hg, q->Wg, &sl)) return false;
  q->slot = sl.slot; q->R = sl.R; q->chunks = sl.chunks; q->gshift = sl.gshift;
  // x and y are addressed through 32-bit buffer offsets; dead elements are the offset tg::kOOB
  if (!fits_descriptor(N, C, Hx, Wx, &q->x_bytes) || !fits_descriptor(N, O, q->Hg, q->Wg, &q->y_bytes)) return false;
  if ((unsigned long long)N * q->chunks > 0x7FFFFFFFull) return false;
  const int PP = (st * (q->R - 1) + ks) * (Wx + 2 * (ks / 2));
  return PP <= 64 * (st == 2 ? 6 : 4);  // the sweeps of the fill cover the patch
}

size_t sconv_weight_pack_bytes(int O, int C, int ks) {
  return real_frag_bytes(O, C, ks * ks) + (size_t)((O + 15) / 16) * 16 * sizeof(int);
}

int launch_sconv_pack_weight(const float* w, int O, int C, int ks, void* packed, hipStream_t s) {
  if (ks != 1 && ks != 3) return BNN_HIP_ERR_UNSUPPORTED;
  const int CB = (C + 31) / 32, OS = (O + 15) / 16, T = ks * ks;
  int* kexp = reinterpret_cast<int*>(static_cast<unsigned char*>(packed) + real_frag_bytes(O, C, T));
  hipLaunchKernelGGL(sconv_row_exp_kernel, dim3(16 * OS), dim3(64), 0, s, w, O, C * T, kexp);
  hipLaunchKernelGGL(sconv_pack_weight_kernel, dim3(CB * T * OS), dim3(64), 0, s, w, O, C, OS, T, kexp,
                     static_cast<bf16x8*>(packed));
  return hipGetLastError() == hipSuccess ? BNN_HIP_OK : BNN_HIP_ERR_LAUNCH;
}

template <int KS, int ST>
static int launch_sconv_t(const float* x, const void* packed, const float* bias, const float* scale, float* y,
                          const SGeo& q, hipStream_t s) {
  const int nsub = tile_nsub(q.O);
  const size_t lds = tile_lds_bytes(1, (ST * (q.R - 1) + KS) * (q.Wx + 2 * (KS / 2)), nsub);
  const bf16x8* Wp = static_cast<const bf16x8*>(packed);
  const int* kexp = real_kexp(packed, q.O, q.C, KS * KS);
  const dim3 grid((unsigned)(q.N * q.chunks), (unsigned)((q.O + 64 * nsub - 1) / (64 * nsub)));
  if (nsub == 2)
    hipLaunchKernelGGL((sconv_kernel<2, KS, ST>), grid, dim3(NT), lds, s, x, Wp, kexp, bias, scale, y, q);
  else
    hipLaunchKernelGGL((sconv_kernel<1, KS, ST>), grid, dim3(NT), lds, s, x, Wp, kexp, bias, scale, y, q);
  return hipGetLastError() == hipSuccess ? BNN_HIP_OK : BNN_HIP_ERR_LAUNCH;
}

int launch_sconv(const float* x, const void* packed, const float* bias, const float* scale, float* y, int N, int O,
                 int C, int H, int W, int ks, int stride, hipStream_t s) {
  SGeo q;
  if (!make_sgeo(N, O, C, H, W, ks, stride, &q)) return BNN_HIP_ERR_UNSUPPORTED;
  if (ks == 1) return launch_sconv_t<1, 1>(x, packed, bias, scale, y, q, s);
  return stride == 2 ? launch_sconv_t<3, 2>(x, packed, bias, scale, y, q, s)
                     : launch_sconv_t<3, 1>(x, packed, bias, scale, y, q, s);
}

}  // namespace bnn

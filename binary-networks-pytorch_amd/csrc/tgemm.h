// tgemm.h — what the ternary-GEMM kernels share: grad.hip (dgrad, wgrad), sconv.hip, slinear.hip, the gradient kernels of
// blinear.hip and the fragment writer of xnor_train.hip.  Each computes products of a real fp32 operand with an operand
// that is exactly {-1, 0, +1}, and this header is the one statement of their ARITHMETIC CONTRACT: the real operand is
// split into three truncated bf16 terms (split3), the ternary operand is a bf16 code (ternary_code), and a product is
// three v_mfma_f32_16x16x32_bf16 with fp32 accumulation, smallest term first (mfma3) — the order the references
// tests/grad_ref.py, sconv_ref.py and linear_ref.py reproduce bit for bit.  Behind it: the K-slot geometry, the tile code
// dgrad_kernel and sconv_kernel have in common, and the two packed fragment layouts.
#pragma once
#include "bconv_core.h"  // buffer-descriptor helpers

namespace bnn {
namespace tg {

using f32x4 = __attribute__((ext_vector_type(4))) float;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;  // one MFMA A / B fragment of a lane (16 bytes)
using u32x4 = __attribute__((ext_vector_type(4))) unsigned;
using u16 = unsigned short;                                  // the LDS planes are arrays of 16-bit containers
constexpr u16 kOne = 0x3F80, kMinusOne = 0xBF80;             // +-1 as bf16
// Tensors are addressed through buffer descriptors with 32-bit lane offsets; an offset behind the descriptor's range
// reads 0 and stores nothing: the zero padding and every dead element.  fits_descriptor() keeps every tensor of a
// launch at or below kMaxTensorBytes, so kOOB is out of range for all of them — and so is kOOBNear +- the few
// elements (< 0x100 bytes) wgrad_kernel's immediate element offsets add to or subtract from it.
constexpr unsigned long long kMaxTensorBytes = 0xFFFFFE00ull;
constexpr unsigned kOOB = 0xFFFFFFF0u, kOOBNear = 0xFFFFFF00u;

constexpr int NT = 256;    // 4 waves
constexpr int APIX = 40;   // patch: halves per pixel (32 channels + 8 pad: 80 B, conflict-free 16-byte reads)
constexpr int SROW = 68;   // output staging: floats per channel row of 64 pixels

// ------------------------------------------------------------------------------------------------- arithmetic
// v = hi + mid + lo (+ at most 2^-24 |v|): each term the TRUNCATION of what is left to bf16 (the remainders are exact
// in fp32, so the three terms carry the leading 24 mantissa bits; truncation needs no rounding logic and one
// v_perm_b32 packs two terms into a dword).  NaN / infinities travel in `hi` (the remainder of an infinity is NaN,
// as in the fp32 product it stands for).
__device__ __forceinline__ void split3(const float (&v)[8], bf16x8& hi, bf16x8& mid, bf16x8& lo) {
  unsigned h[8], m[8], l[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    h[e] = __float_as_uint(v[e]) & 0xFFFF0000u;
    const float r1 = v[e] - __uint_as_float(h[e]);
    m[e] = __float_as_uint(r1) & 0xFFFF0000u;
    const float r2 = r1 - __uint_as_float(m[e]);
    l[e] = __float_as_uint(r2);
  }
  u32x4 ph, pm, pl;
#pragma unroll
  for (int e = 0; e < 4; ++e) {  // the upper halves of two dwords -> one dword
    ph[e] = __builtin_amdgcn_perm(h[2 * e + 1], h[2 * e], 0x07060302u);
    pm[e] = __builtin_amdgcn_perm(m[2 * e + 1], m[2 * e], 0x07060302u);
    pl[e] = __builtin_amdgcn_perm(l[2 * e + 1], l[2 * e], 0x07060302u);
  }
  hi = __builtin_bit_cast(bf16x8, ph);
  mid = __builtin_bit_cast(bf16x8, pm);
  lo = __builtin_bit_cast(bf16x8, pl);
}

// The ternary operand as a bf16 code.  From plane bits: pos (the P plane) -> +1, else neg (the M plane) -> -1, else 0;
// a (sign bit, non-zero mask) pair is nonzero ? ternary_code(bit, !bit) : 0.  From a float: x > 0 -> +1, x < 0 -> -1,
// everything else (+-0, NaN) -> 0.
__device__ __forceinline__ u16 ternary_code(bool pos, bool neg) { return pos ? kOne : neg ? kMinusOne : (u16)0; }
__device__ __forceinline__ u16 ternary_code(float v) { return ternary_code(v > 0.0f, v < 0.0f); }
template <typename T>
__device__ __forceinline__ bf16x8 pack_codes(const T (&c)[8]) {  // codes in 16- or 32-bit containers
  u32x4 pk;
#pragma unroll
  for (int e = 0; e < 4; ++e) pk[e] = (unsigned)c[2 * e] | ((unsigned)c[2 * e + 1] << 16);
  return __builtin_bit_cast(bf16x8, pk);
}
__device__ __forceinline__ bf16x8 zero_frag() { return __builtin_bit_cast(bf16x8, u32x4{0u, 0u, 0u, 0u}); }

// c += a * b with one real operand in three terms: lo, mid, hi IN THAT ORDER (smallest terms first).  Real A (ah, am,
// al) x ternary B, or ternary A x real B (b[0 / 1 / 2] = hi / mid / lo, the term order of the packed real weight).
__device__ __forceinline__ f32x4 mfma3(bf16x8 ah, bf16x8 am, bf16x8 al, bf16x8 b, f32x4 c) {
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, b, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am, b, c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma3(bf16x8 a, const bf16x8 (&b)[3], f32x4 c) {
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b[2], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b[1], c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b[0], c, 0, 0, 0);
}

// ------------------------------------------------------------------------------------------------- K-slots
// A row of W <= 64 pixels is given a power-of-two slot (8, 16, 32 or 64 pixels, zero filled); a 64-pixel chunk of the
// GEMM's pixel dimension is 64 / slot consecutive image rows: an 8-element fragment never straddles an image row.
struct Slots {
  int slot, RR;  // pixels per row slot (pow2 >= W, >= 8); row slots per 64-pixel chunk = 64 / slot
  int R;         // image rows a chunk advances by = min(RR, H)
  int chunks;    // chunks per image = ceil(H / R)
  int gshift;    // log2(slot / 8): 8-pixel groups per row slot
};
inline bool make_slots(int H, int W, Slots* s) {
  if (H <= 0 || W <= 0 || W > 64) return false;
  s->slot = 8;
  s->gshift = 0;
  while (s->slot < W) s->slot *= 2, ++s->gshift;
  s->RR = 64 / s->slot;
  s->R = s->RR < H ? s->RR : H;
  s->chunks = (H + s->R - 1) / s->R;
  return true;
}
// bytes of an [N,C,H,W] fp32 tensor, if a sized descriptor can hold them with every kOOB marker out of range
inline bool fits_descriptor(int N, int C, int H, int W, unsigned* bytes) {
  const unsigned long long b = (unsigned long long)N * C * H * W * 4ull;
  *bytes = (unsigned)b;
  return b <= kMaxTensorBytes;
}

// ------------------------------------------------------------------------------------------------- the shared tile
// dgrad_kernel and sconv_kernel: one chunk x 64 NSUB channels per workgroup; a wave owns two of the four 16-pixel
// sub-tiles (pixel half ph) and half of the 4 NSUB channel groups (channel half chh); the K loop's operand is a patch
// [patch pixel][32 k] in LDS, the epilogue goes through a [channel][pixel] tile in the same LDS.
inline int tile_nsub(int channels) { return channels > 64 ? 2 : 1; }
inline size_t tile_lds_bytes(int planes, int PP, int nsub) {  // `planes` patch planes of PP pixels, or the staging tile
  const size_t patch = (size_t)planes * PP * APIX * sizeof(u16), stage = (size_t)64 * nsub * SROW * sizeof(float);
  return patch > stage ? patch : stage;
}
// A-fragment base address of pixel m of the chunk: patch pixel (st * row + org, st * column + org), patch rows of PW
// pixels.  A dead slot (past the row's end or the chunk's rows) gets pixel (0, 0): any valid address, never stored.
__device__ __forceinline__ int patch_base(int m, int slot, int W, int R, int PW, int st, int org, int lg) {
  int ry = m / slot, x = m - ry * slot;
  if (x >= W || ry >= R) { ry = 0; x = 0; }
  return ((st * ry + org) * PW + (st * x + org)) * APIX + 8 * lg;
}
// Fill roles, once per workgroup: wave w fills k-elements 8 w .. 8 w + 7 of every 32-block, lane l the patch pixels l,
// l + 64, ...  Patch pixel (pr, pc) is pixel (y_org + pr, x_org + pc) of an H x W channel plane: its byte offset there
// (kOOB outside the plane: the zero padding) and its LDS address (-1: past the patch) do not depend on the block.
template <int FK>
__device__ __forceinline__ void patch_fill_roles(int lane, int wave, int PW, int PP, int y_org, int x_org, int H, int W,
                                                 unsigned (&fvoff)[FK], int (&flds)[FK]) {
#pragma unroll
  for (int k = 0; k < FK; ++k) {
    const int pix = lane + 64 * k;
    const int pr = pix / PW, pc = pix - pr * PW;
    const int y = y_org + pr, x = x_org + pc;
    const bool in = pix < PP && y >= 0 && x >= 0 && y < H && x < W;
    fvoff[k] = in ? (unsigned)(y * W + x) * 4u : kOOB;
    flds[k] = pix < PP ? pix * APIX + 8 * wave : -1;
  }
}
// Accumulators -> staging tile.  D layout: column = li (channel within the 16-group), row = 4 lg + r (pixel within
// the sub-tile).
template <int NB>
__device__ __forceinline__ void stage_acc(float* stage, const f32x4 (&acc)[2][NB], int ph, int chh, int li, int lg) {
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int ns = 0; ns < NB; ++ns)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        stage[((chh * NB + ns) * 16 + li) * SROW + 16 * (2 * ph + i) + 4 * lg + r] = acc[i][ns][r];
}
// Epilogue: a thread keeps ONE pixel of the chunk (its lane) -> (row, column) of the chunk and whether it is a pixel
// of the H x W domain the chunks tile
__device__ __forceinline__ bool chunk_pixel(int lane, int slot, int gshift, int W, int R, int y0, int H, int& ery, int& ex) {
  ery = lane >> (gshift + 3);
  ex = lane & (slot - 1);
  return ex < W && ery < R && y0 + ery < H;
}

// ------------------------------------------------------------------------------------------------- fragment layouts
// Sign fragments of dgrad's weight, CS = ceil(C/16), T taps:
//   Bp[ob][tap][cs][lane][e] = sign(W[o = 32 ob + 8 (lane >> 4) + e][c = 16 cs + (lane & 15)][tap])   (bf16 codes)
// -> index of lane `lane`'s bf16x8 fragment (x 8 + e: of a code).
__host__ __device__ constexpr size_t sign_frag(int ob, int tap, int cs, int T, int CS, int lane) {
  return ((size_t)(ob * T + tap) * CS + cs) * 64 + lane;
}
// Packed real weight, CB = ceil(C/32), OS = ceil(O/16), T taps (the bytes sconv.hip's header documents):
//   Wp[cb][tap][os][term][lane][e], term 0 / 1 / 2 = hi / mid / lo; kexp[16 OS] int32 behind the fragments
// -> index of lane `lane`'s bf16x8 fragment of term 0 (+ 64 per term); bytes of the fragments = offset of kexp.
__host__ __device__ constexpr size_t real_frag(int cb, int tap, int os, int T, int OS, int lane) {
  return ((size_t)(cb * T + tap) * OS + os) * 3 * 64 + lane;
}
constexpr size_t real_frag_bytes(int O, int C, int T) {
  return (size_t)((C + 31) / 32) * T * ((O + 15) / 16) * 3 * 64 * sizeof(bf16x8);
}
inline const int* real_kexp(const void* packed, int O, int C, int T) {
  return reinterpret_cast<const int*>(static_cast<const unsigned char*>(packed) + real_frag_bytes(O, C, T));
}

}  // namespace tg
}  // namespace bnn

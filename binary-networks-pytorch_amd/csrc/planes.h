// planes.h — what the activation-plane producers share: pack_act.hip, pack_ste.hip and the packing halves of
// bats_stem.hip and bats_stem_in.hip.  Each turns real values into sign planes, and this header is the one statement of
// their CONTRACT: which bit a value sets (the rules), how the bit enters its word (the two inserts), where the word
// lives (the layout), and how a launcher chooses its vector width.  The kernels keep their own mappings and loads.
// (hblock*.hip, bconv_fly.hip, blinear.hip, slinear.hip, stem*.hip and the convolution epilogues produce planes with
// other instruction forms — ballot, bconv_core.h's shift_in — and are not users of this header.)
#pragma once
#include <hip/hip_fp16.h>

#include <type_traits>

#include "bnn_dev.h"

namespace bnn {

// ---------------------------------------------------------------------------------------------- input vectors
// VP consecutive pixels of one channel, loaded with ONE instruction (4..16 bytes per lane).
// T = float, or __half / Bf16Bits for 16-bit models and autocast (sign() of a 16-bit value is the sign of its exact fp32
// widening).
template <typename T, int VP>
struct alignas(sizeof(T) * VP) PixVec {
  T v[VP];
};
// For a tensor that is read exactly once: non-temporal loads (no L2 / MALL allocation).  Measured on the config-2
// tensor (411 MB, warm clocks): 79-82 us = 5.1 TB/s with plain loads, 68.8 us = 5.97 TB/s non-temporal.
template <typename V>
__device__ __forceinline__ V load_once(const V* p) {
  if constexpr (sizeof(V) == 16) {
    typedef uint32_t u4 __attribute__((ext_vector_type(4)));
    return __builtin_bit_cast(V, __builtin_nontemporal_load(reinterpret_cast<const u4*>(p)));
  } else if constexpr (sizeof(V) == 8) {
    typedef uint32_t u2 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(V, __builtin_nontemporal_load(reinterpret_cast<const u2*>(p)));
  } else if constexpr (sizeof(V) == 4) {
    return __builtin_bit_cast(V, __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(p)));
  } else {
    return __builtin_bit_cast(V, __builtin_nontemporal_load(reinterpret_cast<const uint16_t*>(p)));
  }
}
__device__ __forceinline__ float widen(float v) { return v; }
__device__ __forceinline__ float widen(__half v) { return __half2float(v); }
// bf16 is the upper half of an fp32 word: the widening is one shift, exact for every value (NaN, +-0, subnormals)
struct Bf16Bits {
  uint16_t u;
};
__device__ __forceinline__ float widen(Bf16Bits v) { return __uint_as_float((uint32_t)v.u << 16); }

// -------------------------------------------------------------------------------------------------- bit rules
// Sign rule (torch.sign): P = u > 0, M = u < 0, neither for 0 / -0 / NaN — by the class tests of bnn_dev.h (is_pos /
// is_neg, see the comment there), not float compares.  `nonneg`: the producer's value is relu(u), so M = 0 and P is
// unchanged (relu(u) > 0 iff u > 0).  STE rule: T = |u| < 1, the hard-tanh straight-through mask (NaN -> 0).
__device__ __forceinline__ uint32_t p_bit(float u) { return is_pos(u) ? 1u : 0u; }
__device__ __forceinline__ uint32_t m_bit(float u, bool nonneg = false) { return (!nonneg && is_neg(u)) ? 1u : 0u; }
__device__ __forceinline__ uint32_t t_bit(float u) { return fabsf(u) < 1.0f ? 1u : 0u; }

// The value in front of the rules: u = fmaf(x, a[c], b[c]) (eval-mode BatchNorm, the expression of bn_apply_kernel), or
// u = x when the producer has no affine (a == NULL).
struct Affine {
  bool on;
  float a, b;
  __device__ __forceinline__ float operator()(float x) const { return on ? fmaf(x, a, b) : x; }
};
__device__ __forceinline__ Affine channel_affine(const float* __restrict__ a, const float* __restrict__ b, int c) {
  return {a != nullptr, a ? a[c] : 1.0f, a ? b[c] : 0.0f};
}

// The two ways a channel's bit enters its 32-bit half-word.  kShiftIn: the channels arrive high -> low and every insert
// shifts the word left, which leaves channel c0 + b in bit b after all 32 (a full half-word: c0 + 32 <= C).  kOrAt: OR
// at bit b, in any order (a ragged half-word, walked `for (b = 0; b < 32 && c0 + b < C; ++b)`, and every kernel that keeps
// one walk for both).  One insert per plane: w = with_p<form>(w, u, b), with_m<form>(w, u, b, nonneg), with_t(w, u, b).
//
// What these helpers are NOT, and why (profiles/planes_isa_identity.md has the figures): the word goes in and comes out
// by value and the rule is applied inside, because a `void put(uint32_t& w, uint32_t bit, int b)` form reorders the
// streams of the scalar-accumulator kernels and of pack_act_kernel at VP >= 2; and the walk is not a function over a
// per-channel body, because a loop (or only its condition) that reaches a kernel through an inlined function is unrolled
// differently (pack_ste_kernel<4>: 366 -> 799 instructions, 41 -> 64 VGPRs), and a body that reaches both walks as one
// lambda reschedules pack_act_kernel, pack_act_multi_kernel and stem3x3_kernel.  So the kernels with two walks keep
// both loop statements, with these inserts inside.
constexpr bool kShiftIn = true, kOrAt = false;
template <bool SHIFT = kOrAt>
__device__ __forceinline__ uint32_t with_p(uint32_t w, float u, int b) {
  if constexpr (SHIFT) return (w << 1) | p_bit(u);
  else return w | (p_bit(u) << b);
}
template <bool SHIFT = kOrAt>
__device__ __forceinline__ uint32_t with_m(uint32_t w, float u, int b, bool nonneg = false) {
  if constexpr (SHIFT) return (w << 1) | m_bit(u, nonneg);
  else return w | (m_bit(u, nonneg) << b);
}
__device__ __forceinline__ uint32_t with_t(uint32_t w, float u, int b) { return w | (t_bit(u) << b); }

// ----------------------------------------------------------------------------------------------- plane layout
// A plane is [n][group][y][x] uint64 (include/bnn_hip.h): word (n, g, r) holds the bits of channels 64 g .. 64 g + 63 at
// pixel r = y W + x of image n, channel 64 g + b in bit b.  Producers that own 32 channels per thread address the same
// memory as uint32 halves: half `word` (= channel / 32) of a pixel is the low (even) or high (odd) dword of its uint64.
// K plane sets of one launch lie set_stride words apart.
__device__ __forceinline__ size_t word_off(int n, int cw64, int g, size_t hw, size_t r) {
  return ((size_t)n * cw64 + g) * hw + r;
}
__device__ __forceinline__ size_t half_off(int n, int cw32, int word, size_t hw, size_t r) {
  return ((((size_t)n * (cw32 >> 1) + (word >> 1)) * hw + r) << 1) + (word & 1);
}
__host__ __device__ __forceinline__ uint64_t join_halves(uint32_t lo, uint32_t hi) {
  return (uint64_t)lo | ((uint64_t)hi << 32);
}
inline size_t plane_set_stride(long long npix, int cw64) { return (size_t)npix * cw64; }

// Output pixel q of a launch over N images of hw = rows x Wo pixels: image n, pixel r in it, row oy, column ox.
struct OutPix {
  int n, r, oy, ox;
};
__device__ __forceinline__ OutPix out_pixel(long long q, long long hw, int Wo) {
  OutPix p;
  p.n = (int)(q / hw);
  p.r = (int)(q - (long long)p.n * hw);
  p.oy = p.r / Wo;
  p.ox = p.r - p.oy * Wo;
  return p;
}

// The 2 x 2 average as ATen's avg_pool2d computes it: the window summed row by row, then divided (x / 4 and x * 0.25f
// are the same float for every x).  The tap order is what makes the planes of the result equal the reference's.
__device__ __forceinline__ float avg2x2(float x00, float x01, float x10, float x11) {
  return (((x00 + x01) + x10) + x11) * 0.25f;
}

// ------------------------------------------------------------------------------------------------------- host
// Pixels per thread of a streaming producer: the widest of 4 / 2 / 1 (at most `widest`) that divides HW and for which
// the first element is aligned to the vector — every channel plane and image then starts on the same alignment.
inline int vector_width(int HW, const void* first, size_t elem_size, int widest = 4) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(first);
  if (widest >= 4 && HW % 4 == 0 && (a & (4 * elem_size - 1)) == 0) return 4;
  if (widest >= 2 && HW % 2 == 0 && (a & (2 * elem_size - 1)) == 0) return 2;
  return 1;
}
// f(std::integral_constant<int, VP>) for that width, at most WIDEST (wider forms are not instantiated).
template <int WIDEST = 4, typename F>
inline void with_width(int HW, const void* first, size_t elem_size, F&& f) {
  const int vp = vector_width(HW, first, elem_size, WIDEST);
  if constexpr (WIDEST >= 4) {
    if (vp == 4) return f(std::integral_constant<int, 4>{});
  }
  if (vp == 2) return f(std::integral_constant<int, 2>{});
  f(std::integral_constant<int, 1>{});
}
// f(std::integral_constant<int, K>) for K in KMIN .. 4 (capi.hip has checked the range; anything else runs as 4).
template <int KMIN = 1, typename F>
inline void with_k(int K, F&& f) {
  if constexpr (KMIN == 0) {
    if (K == 0) return f(std::integral_constant<int, 0>{});
  }
  switch (K) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    default: f(std::integral_constant<int, 4>{}); break;
  }
}
// 256 threads per workgroup over nthr threads, one grid row per plane word
inline dim3 stream_grid(long long nthr, int words) { return dim3((unsigned)((nthr + 255) / 256), (unsigned)words); }
inline int launch_status() { return hipGetLastError() == hipSuccess ? BNN_HIP_OK : BNN_HIP_ERR_LAUNCH; }

}  // namespace bnn

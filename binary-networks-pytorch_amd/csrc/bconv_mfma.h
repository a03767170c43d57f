// bconv_mfma.h — what the matrix-core binary convolutions share (bconv_mfma.hip: 3x3; bconv1x1_mfma.hip: 1x1): the
// register types of the MFMA operands, the expansion of sign-plane bits into FP4 (E2M1) nibbles, one k-step of one
// 16 x 16 tile, and the stride of the accumulator transpose through LDS.
#pragma once
#include "bconv_core.h"

namespace bnn {

using i32x4 = __attribute__((ext_vector_type(4))) int;
using i32x8 = __attribute__((ext_vector_type(8))) int;
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int kMfmaThreads = 256;
constexpr int kAccStride = 68;  // int32 per channel row of the transpose buffer: 4 rows apart = 16 banks apart
constexpr int kAccBytes = 4 * 32 * kAccStride * 4;  // four waves x 32 channels

// FP4: 8 bits -> 8 nibbles, bit i in nibble i.  The bits go two to a byte, and each byte looks its two nibbles up in the
// four bytes of `lut` (v_perm_b32): 0x22200200 turns a set bit into 0x2, 0x88800800 into 0x8.
__device__ __forceinline__ uint32_t nibbles8(uint32_t word, int sh, uint32_t lut) {
  uint32_t t = (word >> sh) & 0xFFu;
  t = (t | (t << 12)) & 0x000F000Fu;
  t = (t | (t << 6)) & 0x03030303u;
  return __builtin_amdgcn_perm(lut, lut, t);
}
// P or M set -> 0x2, M set -> 0x8 on top of it: +1 = 0x2, -1 = 0xA (P and M are exclusive)
__device__ __forceinline__ uint32_t expand8_f4(uint32_t pw, uint32_t mw, int sh, bool nn) {
  if (nn) return nibbles8(pw, sh, 0x22200200u);
  return nibbles8(pw | mw, sh, 0x22200200u) | nibbles8(mw, sh, 0x88800800u);
}

// One k-step of one 16 x 16 tile.  FP4: the operands are the low four of the instruction's eight dwords.
template <bool F4, class Acc>
__device__ __forceinline__ Acc mma_step(const i32x4 a, const i32x4 b, const Acc c) {
  if constexpr (F4) {
    const i32x8 a8{a[0], a[1], a[2], a[3], 0, 0, 0, 0}, b8{b[0], b[1], b[2], b[3], 0, 0, 0, 0};
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a8, b8, c, 4, 4, 0, 0, 0, 0);
  } else {
    return __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c, 0, 0, 0);
  }
}

}  // namespace bnn

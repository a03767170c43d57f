// bnn_dev.h — device-side helpers shared by the gfx950 kernels.
// Hand-written for CDNA4 (wave64, v_bitop3_b32, v_bcnt_u32_b32); no portability layer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "../../include/bnn_hip.h"

namespace bnn {

constexpr int kWave = 64;          // CDNA wavefront
// hipFuncAttributeMaxDynamicSharedMemorySize for every kernel that can ask for more than 64 KB of dynamic LDS: ONE
// constant (the CU's whole LDS), never a launch's own size — a per-launch value set from two threads could be lowered
// between one thread's set and its launch.
constexpr int kMaxDynamicLds = 160 * 1024;
constexpr int kOCB = BNN_HIP_OCB;  // output channels per weight block

// Disagreement word of 32 ternary activations against 32 binary weights.
//   w bit = 1 (weight +1): disagree where the activation is negative  -> take M
//   w bit = 0 (weight -1): disagree where the activation is positive  -> take P
// The expression is matched by hipcc to ONE v_bitop3_b32 (truth table 0xe4) on gfx950.
__device__ __forceinline__ uint32_t disagree(uint32_t w, uint32_t m, uint32_t p) {
  return (w & m) | (~w & p);
}

// v_cmp_class_f32 masks: bit0 sNaN,1 qNaN,2 -inf,3 -normal,4 -denorm,5 -0,6 +0,7 +denorm,8 +normal,9 +inf.
// Using the class test (not a float compare) makes the planes independent of the
// kernel's denormal mode and maps NaN to "zero", exactly like torch.sign on CPU.
constexpr int kClassPos = 0x380;  // +denorm | +normal | +inf
constexpr int kClassNeg = 0x01C;  // -inf | -normal | -denorm

#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ bool is_pos(float x) { return __builtin_amdgcn_classf(x, kClassPos); }
__device__ __forceinline__ bool is_neg(float x) { return __builtin_amdgcn_classf(x, kClassNeg); }
#else  // host pass of hipcc only parses these; the amdgcn builtin does not exist for x86
__device__ __forceinline__ bool is_pos(float) { return false; }
__device__ __forceinline__ bool is_neg(float) { return false; }
#endif

template <int N>
struct WordVec;
template <>
struct WordVec<1> { using type = uint32_t; };
template <>
struct WordVec<2> { using type = uint2; };
template <>
struct WordVec<4> { using type = uint4; };

// Everything one binary-convolution launch needs (device pointers + geometry + epilogue).
struct ConvP {
  const uint32_t* P;
  const uint32_t* M;
  const uint32_t* W;
  const uint32_t* Z;
  // epilogue (see bnn_hip_epilogue in include/bnn_hip.h)
  const float* alpha;
  const float* bias;
  const float* scale;
  const float* bn_a;
  const float* bn_b;
  const float* prelu;
  const float* res;
  void* out;       // fp32 NCHW, or int32 NCHW when raw
  uint32_t* outP;  // packed sign planes of the output, or null
  uint32_t* outM;
  // generalised epilogue (BNN_HIP_EPI_*): next layer's BN before packing, residual after the
  // activation, packing the pre-residual value, channel slice of a wider output tensor
  const float* pack_a;
  const float* pack_b;
  const int32_t* thr;  // sign thresholds {T, flip word of the block} per channel (BN + ReLU -> packed-only epilogue), or null
  int eflags;
  int c_off, c_tot;
  bool raw;
  bool relu;
  int N, H, Wd, Ho, Wo, O;
  int KH, KW, sh, sw, ph, pw, dh, dw;
  int cw32, cwc, nchunk;
  int npix;  // N*Ho*Wo
  int C;     // input channels
  int out16; // one-launch layer only: `out` holds 16-bit floats, rounded in the epilogue (0 = fp32, BNN_HIP_DTYPE_F16 / _BF16)
  // shortcut convolution folded into this one (bconv_core.h ShortcutArgs): 1x1 / stride 1 over ds_C channels at the
  // OUTPUT resolution, P plane only; null = none
  const uint32_t* ds_P;
  const uint32_t* ds_W;
  const float* ds_alpha;
  const float* ds_a;
  const float* ds_b;
  int ds_C;
  int ds_inH, ds_inW;  // 0: ds_P is at the output resolution; else ds_P is un-pooled [N, C/64, ds_inH, ds_inW] and the kernel
                   // ORs the 2 x 2 window itself (ceil(ds_inH / 2) == Ho, ceil(ds_inW / 2) == Wo)
};

// Compute units of the current device (for grids of persistent workgroups).  Cached per device in atomics: a
// launch must not pay hipGetDeviceProperties (a slow host call in eager mode), and the C-ABI promises re-entrancy.
inline int current_device_cus() {
  static std::atomic<int> cache[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 256;
  const bool cacheable = dev >= 0 && dev < 64;
  if (cacheable) {
    const int c = cache[dev].load(std::memory_order_relaxed);
    if (c > 0) return c;
  }
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) return 256;
  if (cacheable) cache[dev].store(cus, std::memory_order_relaxed);
  return cus;
}

// host-side launchers (one per .hip file); return a bnn_hip_status
int choose_cwc(int cw32, int KH, int KW);
int launch_sign_thresholds(const float* alpha, const float* bias, const float* scale, const float* bn_a,
                           const float* bn_b, int O, int kmax, int32_t* thr, hipStream_t stream);
int launch_pack_act(const float* x, int N, int C, int H, int W, uint64_t* P, uint64_t* M,
                    hipStream_t stream);
int launch_pack_act_f16(const void* x, int N, int C, int H, int W, uint64_t* P, uint64_t* M,
                        hipStream_t stream);
int launch_pack_act_bf16(const void* x, int N, int C, int H, int W, uint64_t* P, uint64_t* M,
                         hipStream_t stream);
int launch_bn_act_pack(const float* x, int N, int C, int H, int W, const float* bn_a, const float* bn_b,
                       int relu, uint64_t* P, uint64_t* M, hipStream_t stream);
// the same from channels [c_off, c_off + C) of x [N, c_tot, H, W]: K plane sets [K][N][cw64][H][W] for K affines
// (scale / shift [K][C]) from one read; and the two stride-2 phases FactorizedReduce reads, [2][N][cw64][H/2][W/2]
int launch_bn_act_pack_multi(const float* x, int c_off, int c_tot, int N, int C, int H, int W, int K, const float* scale,
                             const float* shift, int relu, uint64_t* P, uint64_t* M, hipStream_t stream);
int launch_bn_act_pack_s2(const float* x, int c_off, int c_tot, int N, int C, int H, int W, const float* bn_a,
                          const float* bn_b, int relu, uint64_t* P, uint64_t* M, hipStream_t stream);
// bats_stem.hip: Conv2d(3, O, 3, padding 1) -> folded BatchNorm -> ReLU and K plane sets [K][N][cw64][H][W] of its output
// (pk_a / pk_b [K][O]) in one launch; y (fp32 [N, O, H, W]) may be null
int launch_stem3x3_bn_relu_pack(const float* x, const float* w, const float* bn_s, const float* bn_t, const float* pk_a,
                                const float* pk_b, int N, int O, int H, int W, int K, uint64_t* P, uint64_t* M, float* y,
                                hipStream_t stream);
// bats_stem_in.hip: the two ImageNet stems.  stem0 (conv 3x3 / 2 -> BN -> ReLU -> grouped conv 3x3 / 2 -> BN [-> ReLU]) with
// its intermediate in LDS; stem1 ([ReLU ->] grouped conv 3x3 / 2 -> BN) with K (0..4) plane sets [K][N][cw64][Ho][Wo] of its
// output, y (fp32 [N, O, Ho, Wo]) null only when K >= 1
int launch_stem_s2x2(const float* x, const float* w1, const float* s1, const float* t1, const float* w2, const float* s2,
                     const float* t2, int N, int C1, int C, int G, int H, int W, int relu_out, float* y, hipStream_t stream);
int launch_gconv3x3s2_bn_pack(const float* x, const float* w, const float* bn_s, const float* bn_t, const float* pk_a,
                              const float* pk_b, int N, int C, int O, int G, int H, int W, int relu_in, int K, uint64_t* P,
                              uint64_t* M, float* y, hipStream_t stream);
int launch_avgpool_pack(const float* x, int N, int C, int H, int W, int k, uint64_t* P, uint64_t* M,
                        hipStream_t stream);
int launch_avgpool2_bn_pack2(const float* x, int N, int C, int H, int W, const float* a1, const float* b1, int relu1,
                             uint64_t* P1, uint64_t* M1, const float* a2, const float* b2, int relu2, uint64_t* P2,
                             uint64_t* M2, float* out, hipStream_t stream);
int launch_orpool_packed(const uint64_t* P, int N, int C, int H, int W, int k, uint64_t* outP, uint64_t* outM,
                         hipStream_t stream);
int launch_bn_relu_maxpool_pack(const float* x, int N, int C, int H, int W, const float* bn_a,
                                const float* bn_b, int relu, int k, int stride, int pad, float* out,
                                uint64_t* P, uint64_t* M, hipStream_t stream);
int launch_stem(const float* x, const float* w, const float* bn_a, const float* bn_b, int N, int H,
                int W, int flags, float* out, uint64_t* P, uint64_t* M, hipStream_t stream);
// csrc/legacy/ (libbnn_hip_legacy.so, test-only): the round-2 stem kernel and the LDS-staged weight tile
int launch_stem_split(const float* x, const float* w, const float* bn_a, const float* bn_b, int N, int H,
                      int W, int half, float* out, uint64_t* P, uint64_t* M, hipStream_t stream);
int launch_bconv_lds(const ConvP& p, hipStream_t s);
int launch_stem_rows(const float* x, const float* w, const float* bn_a, const float* bn_b, int N, int H,
                      int W, int half, float* out, uint64_t* P, uint64_t* M, hipStream_t stream);
int launch_stem_conv(const float* x, const float* w, int N, int H, int W, int half, float* out, hipStream_t stream);
int launch_stem_rows_aff(const float* x, const float* w, const float* bn_a, const float* bn_b, const float* pk_a,
                         const float* pk_b, int N, int H, int W, int half, float* out, uint64_t* P, uint64_t* M,
                         hipStream_t stream);
// stem_wgrad.hip: weight gradient of the stem convolution (fp32 MFMA; partial slabs in `work`, reduced in index order)
bool stem_wgrad_supported(int H, int W);
size_t stem_wgrad_workspace_bytes(int N, int H, int W);
int launch_stem_wgrad(const float* x, const float* dy, int N, int H, int W, float* work, float* dw, hipStream_t stream);
int launch_avgpool2x2_bwd(const float* gy, int N, int C, int Ho, int Wo, float* gx, hipStream_t s);
int launch_avgpool_fc(const float* x, const float* wt, const float* bias, float* out, int N, int C, int HW,
                      int O, hipStream_t stream);
size_t avgpool_fc_workspace_bytes(int N, int C);
bool avgpool_fc_ws_supported(int C, int HW);
int launch_avgpool_fc_ws(const float* x, const float* wt, const float* bias, float* out, float* ws, int N, int C, int HW,
                         int O, hipStream_t stream);
size_t grad_weight_pack_bytes(int O, int C, int ks);
int launch_grad_pack_weight(const float* what, int O, int C, int ks, void* packed, float* alpha, hipStream_t s);
int launch_dgrad(const float* g, const float* alpha, const void* packed, const void* xin, int x_planes, float* gx, int N,
                 int O, int C, int H, int W, int ks, int stride, hipStream_t s);
int grad_wgrad_splits(int N, int O, int C, int ks);
int launch_wgrad(const float* g, const void* xin, const void* xin2, int x_planes, float* part, int splits, int N, int O,
                 int C, int H, int W, int ks, int stride, hipStream_t s);
// sconv.hip: forward of a convolution with binary activations and REAL weights (three bf16 terms per weight)
size_t sconv_weight_pack_bytes(int O, int C, int ks);
int launch_sconv_pack_weight(const float* w, int O, int C, int ks, void* packed, hipStream_t s);
int launch_sconv(const float* x, const void* packed, const float* bias, const float* scale, float* y, int N, int O,
                 int C, int H, int W, int ks, int stride, hipStream_t s);
// slinear.hip: the same layer as a GEMM on a row-major [M, F] input (the ksize = 1 pack of sconv.hip); P / Mn / T (all or
// none) receive the three bit planes [M][ceil(F/64)].  launch_ste_mask: gx[m,f] = T bit ? gx[m,f] : +0 in place.
int slinear_block_channels(int O);
int launch_slinear(const float* x, const void* packed, const float* bias, const float* scale, float* out, uint64_t* P,
                   uint64_t* Mn, uint64_t* T, int M, int F, int O, hipStream_t s);
int launch_ste_mask(float* gx, const uint64_t* T, int M, int F, hipStream_t s);
int launch_pack_ste(const float* x, int N, int C, int H, int W, uint64_t* P, uint64_t* M, uint64_t* T,
                    hipStream_t stream);
// the same planes of fmaf(x, bn_a[c], bn_b[c]) (bn_a == bn_b == null: of x), u never written
int launch_bn_pack_ste(const float* x, int N, int C, int H, int W, const float* bn_a, const float* bn_b, uint64_t* P,
                       uint64_t* M, uint64_t* T, hipStream_t stream);
// the same planes of the pixel lattices (2i, 2j) and (2i+1, 2j+1) only: [2][N][cw64][H/2][W/2] each (H, W even)
int launch_bn_pack_ste_s2(const float* x, int N, int C, int H, int W, const float* bn_a, const float* bn_b, uint64_t* P,
                          uint64_t* M, uint64_t* T, hipStream_t stream);
int launch_pack_weight(const float* w, int O, int C, int KH, int KW, int center, int compute_alpha,
                       const bnn_hip_wlayout& L, uint32_t* wbits, uint32_t* wnz, float* alpha,
                       int32_t* zero_flag, hipStream_t stream);
bool ds_fold_applies(const ConvP& p, int flags);
// route != null: the kernel the ladder picks is described there (include/bnn_hip.h, bnn_hip_conv_route); dry: nothing is
// launched and no HIP function is called (bnn_hip_bconv2d_route: the query IS the launch ladder)
int launch_bconv(const ConvP& p, int flags, hipStream_t s, bnn_hip_conv_route* route = nullptr, bool dry = false);
// bconv_mfma.hip: the dense 3x3 convolution on v_mfma_i32_16x16x64_i8.  weight_i8_bytes: size of the int8 pack, 0 where
// there is none; mfma_conv_applies: what the kernel covers (p from capi.hip's check_conv).
size_t weight_i8_bytes(int O, int C, int KH, int KW);
int launch_pack_weight_i8(const uint32_t* wbits, const uint32_t* wnz, const bnn_hip_wlayout& L, int O, void* w8,
                          hipStream_t s);
bool mfma_conv_applies(const ConvP& p, int flags);
// f4: the FP4 form (v_mfma_f32_16x16x128_f8f6f4, C % 128 == 0), `w8` then the pack of launch_pack_weight_f4
int launch_bconv_mfma(const ConvP& p, int flags, const void* w8, hipStream_t s, bool f4);
size_t weight_f4_bytes(int O, int C, int KH, int KW);
// (L.taps = 9, or 1 for the pack of bconv1x1_mfma.hip)
int launch_pack_weight_f4(const uint32_t* wbits, const uint32_t* wnz, const bnn_hip_wlayout& L, int O, void* w4,
                          hipStream_t s);
bool mfma4_conv_applies(const ConvP& p, int flags);
bool mfma4_fold_applies(const ConvP& p, int flags);
// bconv1x1_mfma.hip: the dense 1x1 convolution on the same FP4 instruction, every epilogue of bnn_hip_bconv2d_fused.
// `w4`: launch_pack_weight_f4 with the layout of the 1x1 weight (one tap), weight1x1_f4_bytes(O, C) = O C / 2 bytes
size_t weight1x1_f4_bytes(int O, int C);
bool mfma1x1_applies(const ConvP& p, int flags);
int launch_bconv1x1_mfma(const ConvP& p, int flags, const void* w4, hipStream_t s);
// the same with the shortcut convolution folded in (p.ds_*; p.ds_W is not read: the 1x1 weight comes as its int8 pack)
size_t shortcut_weight_i8_bytes(int O, int C);
int launch_pack_shortcut_weight_i8(const uint32_t* wbits, int O, int C, void* w8, hipStream_t s);
bool mfma_fold_applies(const ConvP& p, int flags);
int launch_bconv_mfma_fold(const ConvP& p, int flags, const void* w8, const void* sc_w8, hipStream_t s, bool f4);
// grouped / depthwise convolutions: pack_weight.hip (the windowed layout, L from bnn_hip_grouped_weight_layout) and
// bconv_grouped.hip (p.C = all input channels, p.W / p.Z in that layout with S words per tap)
int launch_pack_weight_grouped(const float* w, int O, int Cg, int groups, int center, int compute_alpha,
                               const bnn_hip_wlayout& L, uint32_t* wbits, uint32_t* wnz, float* alpha,
                               int32_t* zero_flag, hipStream_t stream);
int launch_bconv_grouped(const ConvP& p, int groups, int S, hipStream_t s);
// the same convolution with the cell-operation epilogue (PReLU p.prelu, channel_shuffle as a store index, skip p.res)
int launch_bconv_grouped_cell(const ConvP& p, int groups, int S, int shuffle_groups, hipStream_t s);
// one term of a cell node: out windowed by p.c_off / p.c_tot, p.res and `add` at channel 0 of their slices of tensors
// with ct_res / ct_add channels
int launch_bconv_grouped_node(const ConvP& p, int groups, int S, int shuffle_groups, const float* add, int ct_res,
                              int ct_add, hipStream_t s);
// grad_grouped.hip: the two gradients of a grouped convolution from the saved bit planes (fp32 VALU).  Geometry of a
// descriptor that passed capi.hip's check_grouped_grad (the one statement of what the kernels cover).
struct GroupedGradP {
  int N, C, H, W, O, Ho, Wo, KH, KW;
  int stride, ph, pw, dh, dw;   // stride_h == stride_w
  int G;                        // groups; Cg = C / G <= 32, Og = O / G
};
int grouped_wgrad_splits(int N, int O, int G, int taps);   // 1 .. min(N, 64)
int launch_grouped_dgrad(const GroupedGradP& q, const float* g, const float* what, const uint64_t* T, float* gx,
                         hipStream_t s);
int launch_grouped_wgrad(const GroupedGradP& q, const float* g, const uint64_t* P, const uint64_t* M, float* part,
                         int splits, hipStream_t s);
// bconv_fly.hip: the whole layer in one launch, activations (x_dtype: BNN_HIP_DTYPE_*) binarised on the fly into LDS.
// p.P / p.M are unused; p.alpha / bias / scale / out as for launch_bconv.  `plan` may be null (default plan).
bool fly_supported(const ConvP& p);
int fly_default_plan(const ConvP& p, int flags, bnn_hip_fly_plan* plan);
int launch_bconv_fly(const ConvP& p, const void* x, int x_dtype, int flags, const bnn_hip_fly_plan* plan, hipStream_t s);
// blinear.hip: the fully-connected layer on a row-major [M, F] input.  Forward from the float input (x_dtype: BNN_HIP_DTYPE_*) in one
// launch, P / Mn / T (all or none) receive the three bit planes [M][ceil(F/64)]; lds_words: 32-bit words per row of one LDS
// pass over F (0 = default).  Gradients from the forward's weight pack and the planes (bf16 x 3 MFMA).
int launch_blinear_fwd(const void* x, int x_dtype, const uint32_t* wbits, const uint32_t* wnz, int weight_zeros,
                       const float* alpha, const float* bias, const float* scale, float* out, uint64_t* P, uint64_t* Mn,
                       uint64_t* T, int M, int F, int O, int lds_words, hipStream_t s);
int launch_blinear_dgrad(const float* g, const float* alpha, const uint32_t* wbits, const uint32_t* wnz, const uint64_t* T,
                         float* gx, int M, int O, int F, hipStream_t s);
int blinear_wgrad_splits(int M, int O, int F);
int launch_blinear_wgrad(const float* g, const uint64_t* P, const uint64_t* Mn, float* part, int splits, int M, int O, int F,
                         hipStream_t s);
// hblock.hip: the hierarchical block in one launch
bool hblock_supported(const bnn_hip_hblock_desc* d);
int hblock_layout(int C_in, int planes, bnn_hip_hblock_layout* L);
int launch_hblock_pack_weights(int C_in, int planes, const uint32_t* const w[3], uint32_t* dst, hipStream_t s);
int launch_hblock(const bnn_hip_hblock_desc* d, const uint64_t* inP, const uint32_t* W, const float* Kc, const float* res,
                  float* out, uint64_t* outP, hipStream_t stream);
int launch_hblock_pool(const bnn_hip_hblock_desc* d, const uint64_t* inP, const uint32_t* W, const float* Kc, const float* Kp,
                       const float* res, uint64_t* outP1, uint64_t* outP2, uint64_t* outM2, hipStream_t stream);
bool hblock_pool_supported(const bnn_hip_hblock_desc* d);
int launch_hblock_ds(const bnn_hip_hblock_desc* d, const uint64_t* inP, const uint32_t* W, const float* Kc,
                     const uint64_t* dsP, const uint64_t* dsM, const uint32_t* dsW, const float* dsA, float* out,
                     uint64_t* outP, hipStream_t stream);
bool hblock_ds_supported(const bnn_hip_hblock_desc* d);
int launch_hblock_ds_pack_weights(int C_in, int planes, const uint32_t* w, uint32_t* dst, hipStream_t s);
// hblock_cl.hip: the same block for 14 x 14 / 7 x 7 images, lanes = output channels
bool hblock_cl_supported(const bnn_hip_hblock_desc* d);
int launch_hblock_cl_pack_weights(int C_in, int planes, const uint32_t* const w[3], uint32_t* dst, hipStream_t s);
int launch_hblock_cl(const bnn_hip_hblock_desc* d, const uint64_t* inP, const uint32_t* W, const float* Kc, const float* res,
                     float* out, uint64_t* outP, hipStream_t stream);
bool hblock_cl_ds_supported(const bnn_hip_hblock_desc* d);
int launch_hblock_cl_ds(const bnn_hip_hblock_desc* d, const uint64_t* inP, const uint32_t* W, const float* Kc,
                        const uint64_t* dsP, const uint64_t* dsM, const uint32_t* dsW, const float* dsA, float* out,
                        uint64_t* outP, hipStream_t stream);
// fconv.hip: the BATS FactorizedConv (1 x K then K x 1 dense binary convolutions) in one launch, the tensor between
// them as bit planes in LDS.  Operands of a call that passed capi.hip's checks.
struct FconvP {
  const uint64_t* P;
  const uint64_t* M;
  const uint32_t* W1;
  const uint32_t* Z1;   // null unless wz
  const uint32_t* W2;
  const uint32_t* Z2;
  bnn_hip_fconv_stage s1, s2;
  const float* mid_a;
  const float* mid_b;
  const float* res;     // or null
  float* out;
  int N, C, H, W, K, stride, shuffle_groups;
  bool wz;              // honour the zero masks Z1 / Z2
};
bool fconv_supported(int C, int H, int W, int K, int stride);
int launch_fconv(const FconvP& p, hipStream_t s);
// xnor_train.hip: XNORWeightBinarizer under autograd, value and backward
int launch_xnor_grad_pack(const float* w, int O, int C, int ks, int center, int compute_alpha, void* packed, float* alpha,
                          hipStream_t s);
int launch_xnor_what(const float* w, int O, int C, int taps, int center, int compute_alpha, float* what, float* alpha,
                     hipStream_t s);
int launch_xnor_weight_bwd(const float* w, const float* dwhat, int splits, int O, int C, int taps, int center,
                           int compute_alpha, float* dw, hipStream_t s);
// bn_train.hip: training-mode BatchNorm (+ residual) (+ ReLU), forward and backward
int bn_train_splits(int N, int C, int HW);
int launch_bn_stats(const float* x, int N, int C, int HW, int splits, double* partial, hipStream_t s);
int launch_bn_apply(const float* x, const double* partial, int splits, const float* gamma, const float* beta,
                    const float* res, int relu, float* y, int N, int C, int HW, float eps, float momentum, float* rm,
                    float* rv, float* mean_out, float* invstd_out, float* work, hipStream_t s);
int launch_bn_act(const float* x, const float* scale, const float* shift, const float* res, int relu, float* y, int N,
                  int C, int HW, hipStream_t s);
int launch_bn_bwd_reduce(const float* gy, const float* y, const float* x, const float* mean, const float* invstd, int N,
                         int C, int HW, int splits, double* partial, hipStream_t s);
int launch_bn_bwd_dx(const float* gy, const float* y, const float* x, const float* mean, const float* invstd,
                     const float* gamma, const double* partial, int splits, float* dx, float* dres, float* dgamma,
                     float* dbeta, int N, int C, int HW, float* work, hipStream_t s);
int launch_bn_finalize(const double* partial, int splits, const float* gamma, const float* beta, int N, int C, int HW,
                       float eps, float momentum, float* rm, float* rv, float* mean_out, float* invstd_out, float* scale_out,
                       float* shift_out, hipStream_t s);
int launch_bn_bwd_dx_add(const float* gy, const float* y, const float* x, const float* mean, const float* invstd,
                         const float* gamma, const double* partial, int splits, const float* addend, float* dx,
                         float* dgamma, float* dbeta, int N, int C, int HW, float* work, hipStream_t s);
// BatchNorm backward of a gradient that lives on those two lattices (g0, g1: [N, C, H/2, W/2]); reduce + finalize + dx
int launch_bn_bwd_s2(const float* g0, const float* g1, const float* x, const float* mean, const float* invstd,
                     const float* gamma, int N, int C, int H, int W, int splits, double* partial, float* work, float* dx,
                     float* dgamma, float* dbeta, hipStream_t s);
// prelu_bwd.hip: backward of channel_shuffle(PReLU(z), sg); `partial`: O * splits doubles, splits = bn_train_splits(N, O, HW)
int launch_prelu_shuffle_bwd(const float* gy, const float* z, const float* slope, int slope_count, int N, int O, int HW,
                             int sg, int splits, float* gz, float* dslope, double* partial, hipStream_t s);
int launch_bn_relu_pool_fwd(const float* x, const double* partial, int splits, const float* gamma, const float* beta,
                            float* p, unsigned char* code, int N, int C, int H, int W, float eps, float momentum, float* rm,
                            float* rv, float* mean_out, float* invstd_out, float* work, hipStream_t s);
int launch_bn_relu_pool_bwd(const float* gy, const float* p, const unsigned char* code, const float* x, const float* mean,
                            const float* invstd, const float* gamma, int N, int C, int H, int W, int splits,
                            double* partial, float* work, float* dx, float* dgamma, float* dbeta, hipStream_t s);
int launch_probe_int_alu(int mode, int iters, double* lane_ops_per_s, double* elapsed_ms, hipStream_t s);
int launch_probe_clock(int spin_iters, double* shader_mhz, double* elapsed_us, hipStream_t s);

}  // namespace bnn

/*
 * bnn_hip.h — C-ABI of the MI355X (gfx950) binary-convolution inference path.
 *
 * This is the drop-in boundary for ONE hot path of 1adrianb/binary-networks-pytorch
 * (package `bnn`): the fake-binarized Conv2d / Linear forward
 *
 *     out = post( conv2d( sign(x), sign(W) * mean|W| , bias ), x )
 *
 * Reference call sites that each entry point replaces (paths relative to the
 * reference repository root):
 *
 *   bnn_hip_pack_act_f32      <- bnn/ops.py:63-66,151-152   SignActivation.forward / BasicInputBinarizer.forward
 *   bnn_hip_pack_weight_f32   <- bnn/ops.py:116-140         XNORWeightBinarizer._compute_alpha / .forward
 *   bnn_hip_bconv2d           <- bnn/layers/conv.py:90-97   Conv2d.forward  (nn.Conv2d._conv_forward + post-process)
 *   bnn_hip_bconv2d_direct    <- bnn/layers/conv.py:90-97   the same forward from the FLOAT input, sign() on the fly
 *   bnn_hip_blinear           <- bnn/layers/linear.py:22-27 Linear.forward  (F.linear + post-process)
 *   post_scale argument       <- bnn/ops.py:200-202         BasicScaleBinarizer.forward (out.mul_(alpha))
 *   (Identity post-process    <- bnn/bconfig.py:6-8 : pass post_scale = NULL)
 *
 * The reference has no FFI of its own (pure Python on top of PyTorch), so these
 * are the functions a ctypes / cgo / JNI stub binds; see INTEGRATION.md.
 *
 * Conventions
 *   - every function returns an int status: 0 = ok, negative = bnn_hip_status
 *   - no function throws, aborts, allocates device memory or synchronises the device
 *   - all pointers are DEVICE pointers on the *current* HIP device unless stated
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream)
 *   - functions are re-entrant and keep no global mutable state except a
 *     monotonically increasing launch counter (bnn_hip_launch_count)
 *
 * Data formats
 *   Activations are ternary {-1,0,+1} because the reference's sign(0) == 0 and its
 *   zero padding is applied AFTER binarisation (bnn/layers/conv.py:91-92).  They are
 *   stored as two bit-planes, channel-group planar ("N C/64 H W" of uint64 words):
 *       P[n][g][y][x]  bit b set  <=>  x[n][64*g + b][y][x] > 0
 *       M[n][g][y][x]  bit b set  <=>  x[n][64*g + b][y][x] < 0
 *   with g < cw64 = ceil(C/64); pad bits are 0 in both planes.  (Consecutive pixels of one
 *   group are contiguous, so a wavefront whose lanes are pixels reads 512 contiguous bytes
 *   per load for any C; a pixel-major layout wastes 3/4 of every cache line at C = 512.)
 *   NaN -> neither plane (torch.sign(nan) == 0), denormals keep their sign.
 *
 *   Weights are one bit-plane (+1 -> 1, -1 -> 0) plus a non-zero mask, in the
 *   kernel-facing layout  wbits[ob][chunk][j][tap][cwc]  (uint32 words) where
 *       ob    = o / 32, j = o % 32           (output channels padded to a multiple of 32)
 *       tap   = ky*KW + kx
 *       chunk = which group of `cwc` consecutive 32-channel words of the input channels
 *   (cwc, nchunk) are a pure function of (C, KH, KW): bnn_hip_weight_layout().
 *
 *   Integer dot product per output element (exact):
 *       D   = popcount( (W & M) | (~W & P) )       disagreeing non-zero positions
 *       dot = popcount(P | M) - 2*D                 (= sum of sign(x)*sign(w)), over the window
 *   and the float result  out = fmaf(alpha[o], (float)dot, bias[o]) [* post_scale[o]].
 */
#ifndef BNN_HIP_H_
#define BNN_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Additive entry points of ABI 16 for the 1x1 convolution on the FP4 matrix cores (no struct or signature changed):
 * + bnn_hip_weight1x1_f4_bytes, bnn_hip_pack_weight1x1_f4, bnn_hip_bconv1x1_mfma4_supported, bnn_hip_bconv1x1_mfma4_fused.
 * Additive entry points of ABI 16 for the BATS FactorizedConv (no struct or signature changed): + bnn_hip_fconv_desc,
 * bnn_hip_fconv_stage, bnn_hip_fconv_supported, bnn_hip_fconv_fused (csrc/fconv.hip).
 * Additive entry points of ABI 16 for the Linear with binary activations and real weights (no struct or signature
 * changed): + bnn_hip_slinear_f32, bnn_hip_ste_mask_f32 (csrc/slinear.hip).
 * Additive entry points of ABI 16 for the convolution with binary activations and real weights (no struct or signature
 * changed): + bnn_hip_sconv2d_weight_pack_bytes, bnn_hip_sconv2d_pack_weight_f32, bnn_hip_sconv2d_f32 (csrc/sconv.hip).
 * ABI 16: + bnn_hip_bconv2d_route, bnn_hip_bconv2d_dot_route and bnn_hip_conv_route (which kernel a convolution runs:
 * host-only queries answered by the launch ladder itself; no other struct or signature changed).
 * Additive entry points of ABI 16 for the fully-connected layer (no struct or signature changed): + bnn_hip_blinear_direct,
 * bnn_hip_blinear_grad_input_f32, bnn_hip_blinear_grad_weight_f32, bnn_hip_blinear_grad_weight_splits (csrc/blinear.hip).
 * Additive entry points of ABI 15 for the training step of FactorizedReduce (no struct or signature changed):
 * + bnn_hip_bn_act_pack_ste_s2_f32, bnn_hip_bn_train_pack_ste_s2_f32 (the three bit planes of the two pixel lattices its
 * convolutions read); + bnn_hip_bn_train_backward_s2_f32 (the BatchNorm backward of a gradient that lives on those lattices).
 * Additive entry points of ABI 15 for the training step of a BATS cell operation (no struct or signature changed):
 * + bnn_hip_bn_act_pack_ste_f32, bnn_hip_bn_train_pack_ste_f32 (BatchNorm + sign + straight-through mask as three bit
 * planes, the normalised tensor never written); + bnn_hip_prelu_shuffle_backward_f32 / _workspace_bytes (backward of
 * channel_shuffle(PReLU(.))); + bnn_hip_bn_train_backward_add_f32 (the BatchNorm backward with the skip's gradient added).
 * ABI 15 (round 6): + bnn_hip_hblock_{supported,layout_of,pack_weights,forward} (the hierarchical block in one launch);
 * + bnn_hip_avgpool2_bn_pack2_f32 (the pool in front of a pre-activation stage + both sign planes it feeds);
 * + bnn_hip_grouped_weight_layout, bnn_hip_pack_weight_grouped_f32, bnn_hip_bconv2d_grouped (grouped / depthwise
 * convolutions: additive entry points of ABI 15, no struct or signature changed); + bnn_hip_bconv2d_grouped_fused (the
 * same convolution with PReLU, channel shuffle and skip connection in its launch: additive too);
 * + bnn_hip_f32_view, bnn_hip_bn_act_pack_multi_f32, bnn_hip_bn_act_pack_s2_f32, bnn_hip_bconv2d_grouped_node (a whole
 * BATS cell as fused launches: additive as well); + bnn_hip_stem3x3_bn_relu_pack_f32 (the real-valued stem of a BATS
 * CIFAR network with the sign planes of its consumers in one launch: additive too).
 * ABI 14 (round 5): + bnn_hip_stem7x7_wgrad_f32 / bnn_hip_stem7x7_wgrad_workspace_bytes (weight gradient of the stem
 * convolution: the training backward of that layer); + bnn_hip_avgpool2x2_backward_f32, bnn_hip_xnor_grad_pack_weight_f32; + bnn_hip_avgpool_fc_ws_f32 / bnn_hip_avgpool_fc_workspace_bytes (the head as two streaming launches
 * through a workspace); + bnn_hip_stem7x7_conv_f32 (the stem's convolution alone: the training forward); the table of bnn_hip_sign_thresholds_f32 holds FOUR words per channel (was two) and kmax < 2^20.
 * ABI 13 (round 4): + bnn_hip_bn_act_f32 (eval-mode BatchNorm + residual + ReLU tail of the per-layer path);
 * bnn_hip_xnor_weight_backward_f32 takes `splits` partial slabs.
 * ABI 12 (round 4): + bnn_hip_probe_clock; + the training-side entry points bnn_hip_pack_act_ste_f32,
 * bnn_hip_bconv_grad_{input,weight}_packed_f32 (3-bit saved state), bnn_hip_bn_train_{workspace_bytes,forward,backward}_f32,
 * bnn_hip_bn_relu_maxpool_train_{forward,backward}_f32, bnn_hip_xnor_weight_{forward,backward}_f32;
 * - BNN_HIP_STEM_STAGED and BNN_HIP_FLAG_WEIGHTS_LDS (those kernels are test-only now: csrc/legacy/);
 * stem tensors capped at the 32-bit buffer-descriptor range; size arithmetic of all validators saturating.          */
#define BNN_HIP_ABI_VERSION 16
#define BNN_HIP_OCB 32 /* output channels per weight block (padding granularity of O) */

typedef enum bnn_hip_status {
  BNN_HIP_OK = 0,
  BNN_HIP_ERR_INVALID_ARG = -1,  /* null pointer, non-positive size, misaligned buffer        */
  BNN_HIP_ERR_UNSUPPORTED = -2,  /* shape outside what the kernels implement                   */
  BNN_HIP_ERR_LAUNCH = -3,       /* hipGetLastError() != hipSuccess after a launch             */
  BNN_HIP_ERR_TOO_LARGE = -4,    /* a tensor exceeds one launch's addressing: 2^30 fp32 elements (4 GiB) for the
                                    convolution entry points, 2^31 elements elsewhere — split the batch */
  BNN_HIP_ERR_NO_DEVICE = -5     /* no HIP device / wrong architecture                         */
} bnn_hip_status;

/* Geometry of one binary convolution (mirrors torch.nn.Conv2d hyper-parameters that
 * bnn.layers.Conv2d forwards unchanged: bnn/layers/conv.py:68-83). groups == 1, except for
 * bnn_hip_bconv2d_grouped, which takes `groups` as an argument of its own. */
typedef struct bnn_hip_conv_desc {
  int32_t N, C, H, W;          /* input  [N,C,H,W]                        */
  int32_t O, KH, KW;           /* weight [O,C,KH,KW]                      */
  int32_t stride_h, stride_w;
  int32_t pad_h, pad_w;        /* zero padding, applied after sign()      */
  int32_t dil_h, dil_w;
  int32_t flags;               /* BNN_HIP_FLAG_*                          */
} bnn_hip_conv_desc;

#define BNN_HIP_FLAG_FORCE_GENERIC 1 /* use the shape-generic kernel even if a tiled one exists */
#define BNN_HIP_FLAG_WEIGHT_ZEROS 2  /* some sign(W) == 0: honour the wnz mask (slower kernel)  */
#define BNN_HIP_FLAG_WEIGHTS_SGPR 4  /* tiled kernel: force the scalar-cache weight stream       */
/* bit 8 (BNN_HIP_FLAG_WEIGHTS_LDS until ABI 11: the LDS-staged weight tile, 2x slower than the scalar-cache stream on
 * every shape) is ignored since ABI 12; that kernel is a test-only cross-check now (csrc/legacy/).            */
#define BNN_HIP_FLAG_ACT_NONNEG 32   /* caller vouches that the M plane is ALL ZERO (activations
                                        out of a ReLU / max-pool of a ReLU are {0,+1}): 3x3 kernels
                                        then keep only the P plane in registers.  M must still be a
                                        valid pointer.  A wrong promise gives wrong results.      */
#define BNN_HIP_FLAG_THROUGHPUT 64   /* other work shares the GPU (several batches in flight): prefer fewer,
                                        longer waves — the multi-chunk 3x3 kernels then do not split a
                                        32-channel block over two waves (same results; ResNet-18 b256:
                                        -3 % with one batch in flight, +2 % with two)              */
/* bnn_hip_bconv2d_direct only (every other entry point answers BNN_HIP_ERR_INVALID_ARG): `out` is a tensor of 16-bit
 * floats, 2-byte aligned, and the kernel rounds the result itself, where Tensor.to() and the reference's in-place
 * post-scale on a 16-bit tensor round it:  r = D(fmaf(alpha[o], dot, bias[o]));  with post_scale: r = D(float(r) *
 * post_scale[o]).  Round to nearest even, fp16 overflow gives +-inf.  At most one of the two.          */
#define BNN_HIP_FLAG_OUT_F16 256
#define BNN_HIP_FLAG_OUT_BF16 512

/* Everything that happens to the integer dot after the popcount loop, fused into the conv
 * kernel so that activations can stay bit-packed between binary layers (callers:
 * bnn/models/layers/res_block.py:40-56, conv -> BN -> ReLU -> conv -> BN -> +identity -> ReLU):
 *     y = fmaf(alpha[o], dot, bias[o])                 XNOR scale + conv bias   (required)
 *     y = y * post_scale[o]                            BasicScaleBinarizer      (optional)
 *     y = fmaf(y, bn_scale[o], bn_shift[o])            eval-mode BatchNorm      (optional)
 *     y = y + residual[n,o,y,x]                        shortcut                 (optional)
 *     y = relu(y)  |  y = y >= 0 ? y : prelu[o]*y      activation               (optional)
 * Outputs: out_f32 (fp32 NCHW) and/or out_P/out_M (sign(y) as bit planes, format above, with
 * C := O; every word is written, pad bits 0).  At least one output is required.
 *
 * Pre-activation dataflows (bnn/models/layers/res_block.py:121-167 PreBasicBlock,
 * hierarchical_block.py:38-60 HBlock) order things differently; `flags` and the trailing fields
 * cover them without leaving the kernel:
 *     BNN_HIP_EPI_RES_AFTER_ACT    the residual is added AFTER the activation   (y = act(conv); y += id)
 *     p = value that is binarised for the next binary layer:
 *         default                      p = y (the stored value)
 *         BNN_HIP_EPI_PACK_BEFORE_RES  p = the value before a RES_AFTER_ACT residual was added
 *     pack_scale/pack_shift != NULL    p = fmaf(p, pack_scale[o], pack_shift[o])   (the NEXT layer's BatchNorm)
 *     BNN_HIP_EPI_PACK_RELU            planes of sign(relu(p)):  P = (p > 0), M = 0
 *     out_c_total != 0                 out_f32 and residual are [N,out_c_total,Ho,Wo] tensors and this
 *                                      convolution owns channels [out_c_offset, out_c_offset + O)
 *                                      (torch.cat of HBlock written in place).                     */
#define BNN_HIP_EPI_RES_AFTER_ACT 1
#define BNN_HIP_EPI_PACK_BEFORE_RES 2
#define BNN_HIP_EPI_PACK_RELU 4
typedef struct bnn_hip_epilogue {
  const float* alpha;      /* [o_pad]                                   */
  const float* bias;       /* [O] or NULL                               */
  const float* post_scale; /* [O] or NULL                               */
  const float* bn_scale;   /* [O] or NULL  gamma / sqrt(var + eps)      */
  const float* bn_shift;   /* [O] or NULL  beta - mean * bn_scale       */
  const float* residual;   /* [N,O,Ho,Wo] or NULL                       */
  const float* prelu;      /* [O] or NULL                               */
  int32_t relu;            /* non-zero: clamp at 0 after the residual   */
  int32_t flags;           /* BNN_HIP_EPI_*                             */
  float* out_f32;          /* [N,O,Ho,Wo] or NULL                       */
  uint64_t* out_P;         /* [N,ceil(O/64),Ho,Wo] or NULL              */
  uint64_t* out_M;
  const float* pack_scale; /* [O] or NULL (both or neither)             */
  const float* pack_shift;
  int32_t out_c_offset;    /* see above; 0/0 = plain [N,O,Ho,Wo]        */
  int32_t out_c_total;
  const int32_t* sign_thresholds; /* NULL, or [32*ceil(O/32)][4] from bnn_hip_sign_thresholds_f32 for THIS alpha / bn_scale /
                                     bn_shift: used when the epilogue is exactly BN + ReLU -> planes only (no bias,
                                     scale, residual, fp32 output): the sign bit then comes from an integer compare
                                     of the dot — same bits as the float path, fewer instructions.  Ignored
                                     otherwise.                                                          */
  /* ABI 11 — the shortcut branch of a down-sampling residual block folded into the block's second convolution
   * (bnn/models/layers/res_block.py:31-37,52-54: AvgPool2d(2) -> Conv2d 1x1 -> BatchNorm, added before the last ReLU):
   *     residual[n,o,y,x] = fmaf(fmaf(sc_alpha[o], dot1x1(sc_P[n,:,y,x], sc_wbits[o]), 0), sc_bn_scale[o], sc_bn_shift[o])
   * is computed inside the kernel with the float operations of the stand-alone 1x1 convolution + BN epilogue (same
   * bits), instead of being written to and read back from an fp32 tensor.  sc_P: sign plane P of the 1x1 conv's
   * input at the OUTPUT resolution, [N, ceil(sc_C/64), Ho, Wo] uint64, non-negative activations (its M plane is all
   * zero and not passed); sc_wbits / sc_alpha: bnn_hip_pack_weight_f32 of the [O, sc_C, 1, 1] weight.  Either all five
   * pointers or none (then sc_C is ignored); not together with `residual`.  Supported where
   * bnn_hip_shortcut_fold_supported() says so; BNN_HIP_ERR_UNSUPPORTED otherwise.
   * ABI 12 — sc_in_hw != 0: sc_P is the UN-POOLED plane of the block's input, [N, ceil(sc_C/64), H, W] with
   * sc_in_hw = (H << 16) | W, ceil(H/2) == Ho, ceil(W/2) == Wo: the kernel ORs the 2 x 2 window of every output pixel
   * itself (sign of AvgPool2d(2, ceil_mode=True, count_include_pad=False) of non-negative values) — no
   * bnn_hip_orpool_packed launch, same bits.  0 (the field was `reserved` until ABI 11): sc_P at the output resolution. */
  const uint64_t* sc_P;
  const uint32_t* sc_wbits;
  const float* sc_alpha;
  const float* sc_bn_scale;
  const float* sc_bn_shift;
  int32_t sc_C;
  int32_t sc_in_hw;
} bnn_hip_epilogue;

/* Per channel the integer dots (|dot| <= kmax = C*KH*KW) whose epilogue value
 *   fmaf(fmaf(alpha, dot, bias) [* post_scale], bn_scale, bn_shift)   is > 0.
 * Every step is monotone in dot, so that set is one-sided:  bit = (dot >= T) XOR flip.
 * `thresholds` holds 4 * 32 * ceil(O / 32) int32 (whole 32-channel blocks; pad channels are written as "never").
 * thresholds[4o] = T; thresholds[4o+1] = for EVEN o the flip bits of o's 32-channel block as one word (bit k = channel
 * 32*(o/32)+k), for ODD o the parities of the block's T (bit k = T of channel k is odd); thresholds[4o+2], [4o+3] = the
 * comparands of the kernels'
 * two-instruction form of the same test on the agreement / disagreement count (ceil(T/2) + 2^20 and
 * max(floor(-T/2) + 1 + 2^20, 0): csrc/bconv_core.h midt2_shift_in).  Found by bisection with the conv epilogue's
 * own float operations.  Re-derive when any input changes.  kmax < 2^20.
 * (ABI 14: four words per channel; ABI 9-13: {T, flip}; up to ABI 8 the table held {lo, span} of an interval.)     */
int bnn_hip_sign_thresholds_f32(const float* alpha, const float* bias, const float* post_scale,
                                const float* bn_scale, const float* bn_shift, int O, int kmax,
                                int32_t* thresholds, void* stream);

typedef struct bnn_hip_wlayout {
  int32_t cw32;     /* 32-bit words per pixel per plane (= 2*ceil(C/64))          */
  int32_t cwc;      /* words per chunk                                            */
  int32_t nchunk;   /* cw32 / cwc                                                 */
  int32_t taps;     /* KH*KW                                                      */
  int32_t o_pad;    /* O rounded up to a multiple of BNN_HIP_OCB                  */
  int32_t reserved;
  int64_t n_words;  /* uint32 words in wbits (and in wnz): o_pad*taps*cw32        */
} bnn_hip_wlayout;

typedef struct bnn_hip_devinfo {
  char name[64];
  char arch[32];          /* e.g. "gfx950:sramecc+:xnack-"                        */
  int32_t compute_units;
  int32_t clock_khz;      /* max engine clock                                     */
  int32_t mem_clock_khz;
  int32_t mem_bus_bits;
  int32_t wavefront;
  int32_t lds_bytes_per_block;
  int64_t total_mem_bytes;
  int32_t l2_bytes;
  int32_t reserved;
} bnn_hip_devinfo;

int bnn_hip_abi_version(void);
const char* bnn_hip_status_string(int status);
/* number of kernel launches issued through this library since load (host counter) */
uint64_t bnn_hip_launch_count(void);

/* HOST: fill *out for HIP device `device`.                                        */
int bnn_hip_device_info(int device, bnn_hip_devinfo* out);

/* HOST: uint64 words per pixel per activation plane for C channels: ceil(C/64).  */
int bnn_hip_act_words(int C);
/* HOST: weight layout for a [O,C,KH,KW] weight.                                   */
int bnn_hip_weight_layout(int O, int C, int KH, int KW, bnn_hip_wlayout* out);

/* sign(x) as two bit planes.  x: float32 NCHW contiguous.  P, M: [N,ceil(C/64),H,W]
 * uint64 each, 16-byte aligned.                                                    */
int bnn_hip_pack_act_f32(const float* x, int N, int C, int H, int W,
                         uint64_t* P, uint64_t* M, void* stream);

/* Same planes from an IEEE half-precision tensor (a `.half()` model: Tensor.sign() of fp16 values,
 * bnn/ops.py:66).  x: [N,C,H,W] of 16-bit floats, 2-byte aligned.  sign() is exact in any precision, so
 * the planes equal those of the widened fp32 tensor bit for bit.                                  */
int bnn_hip_pack_act_f16(const void* x, int N, int C, int H, int W,
                         uint64_t* P, uint64_t* M, void* stream);

/* Same planes from a bfloat16 tensor (a `.bfloat16()` model, or the activations of a network under bf16 autocast):
 * x: [N,C,H,W] of 16-bit brain floats, 2-byte aligned.  A bf16 value is the upper half of an fp32 word: the widening
 * is exact, the planes equal those of the widened fp32 tensor bit for bit.  (Additive entry point of ABI 16.)  */
int bnn_hip_pack_act_bf16(const void* x, int N, int C, int H, int W,
                          uint64_t* P, uint64_t* M, void* stream);

/* AvgPool2d(kernel=k, stride=k, ceil_mode=True, count_include_pad=False) followed by
 * sign(): the shortcut branch of a down-sampling residual stage
 * (bnn/models/resnet.py:128-133: AvgPool2d -> binary conv1x1 -> BN).  Output planes have
 * ceil(H/k) x ceil(W/k) pixels.  The planes are those of the average (the window summed row by
 * row in fp32, divided by its in-image taps), so an average that underflows to zero sets no bit,
 * as in the reference and in bnn_hip_avgpool2_bn_pack2_f32.                          */
int bnn_hip_avgpool_pack_f32(const float* x, int N, int C, int H, int W, int k,
                             uint64_t* P, uint64_t* M, void* stream);

/* AvgPool2d(2, 2) (even H, W; bnn_amd/models/resnet.py: the pool in front of a hierarchical-block stage) + the sign planes
 * of up to two BatchNorm branches of the pooled tensor in one pass:  t = window sum (row by row) / 4 as ATen computes it,
 * P1/M1 = sign(act1(fmaf(t, a1, b1))), P2/M2 = sign(act2(fmaf(t, a2, b2))) (relu: M = 0).  a2 == NULL: one branch.
 * out_f32: NULL, or the pooled tensor [N, C, H/2, W/2] when somebody needs it.                                     */
int bnn_hip_avgpool2_bn_pack2_f32(const float* x, int N, int C, int H, int W, const float* a1, const float* b1, int relu1,
                                  uint64_t* P1, uint64_t* M1, const float* a2, const float* b2, int relu2, uint64_t* P2,
                                  uint64_t* M2, float* out_f32, void* stream);

/* The same shortcut input from the SIGN PLANES of a NON-NEGATIVE tensor (a ReLU output: M == 0): the average of
 * non-negative values is positive iff one of them is, so sign(AvgPool_k(x)) is the OR of the P plane over each
 * k x k window (ceil mode: windows are clipped at the border) — 2 bits per element read instead of 32.
 * P: [N,ceil(C/64),H,W]; out_P / out_M: [N,ceil(C/64),ceil(H/k),ceil(W/k)], out_M is written as 0.
 * Exact for finite inputs whose window average does not underflow to zero (the planes hold no magnitudes: a window of
 * zeros and one 2^-149 averages to 0 in the reference and ORs to 1); the caller vouches for x >= 0 (as with
 * BNN_HIP_FLAG_ACT_NONNEG).                                                                              */
int bnn_hip_orpool_packed(const uint64_t* P, int N, int C, int H, int W, int k,
                          uint64_t* out_P, uint64_t* out_M, void* stream);

/* BatchNorm(eval) -> [ReLU] -> sign() of an fp32 NCHW tensor in one pass: the input binarisation of a
 * pre-activation block (res_block.py:148 `conv1(bn1(x))`, hierarchical_block.py:39 `conv1(act1(bn1(x)))`).
 *   v = fmaf(x, bn_scale[c], bn_shift[c])  (both NULL: v = x);  relu != 0: planes of sign(max(v, 0)).  */
int bnn_hip_bn_act_pack_f32(const float* x, int N, int C, int H, int W, const float* bn_scale,
                            const float* bn_shift, int relu, uint64_t* P, uint64_t* M, void* stream);

/* Tail of the real-valued stem, one pass over the stem conv's fp32 NCHW output
 * (bnn/models/resnet.py:150-153: bn1 -> relu -> maxpool, then the sign() of the first binary
 * conv):  v = fma(x, bn_scale[c], bn_shift[c]) (both NULL = no BN);  m = max over the k x k
 * window with stride/pad of nn.MaxPool2d;  y = relu ? max(m,0) : m.
 * Outputs (either may be NULL): out_f32 [N,C,Ho,Wo] and sign(y) as planes P, M.     */
int bnn_hip_bn_relu_maxpool_pack_f32(const float* x, int N, int C, int H, int W,
                                     const float* bn_scale, const float* bn_shift, int relu,
                                     int k, int stride, int pad,
                                     float* out_f32, uint64_t* P, uint64_t* M, void* stream);

/* The whole real-valued stem of the reference's ResNets as one MFMA kernel
 * (bnn/models/resnet.py:93-96,150-153): conv 7x7 / stride 2 / pad 3, 3 -> 64 channels, no bias
 * (w: float32 [64,3,7,7]) -> y*bn_scale[c] + bn_shift[c] -> ReLU -> MaxPool 3x3 / 2 / 1.
 * x: float32 [N,3,H,W].  Outputs (either may be NULL): out_f32 [N,64,Hp,Wp] and its sign planes
 * P, M ([N,1,Hp,Wp] uint64), Hp = ((H-1)/2 + 1 - 1)/2 + 1 (56 for H = 224).
 * flags = 0: fp32 operands split into fp16 hi+lo halves (22 mantissa bits), products as
 *            hi*hi + hi*lo + lo*hi on v_mfma_f32_16x16x32_f16 with fp32 accumulation, at 3/16 of the matrix
 *            time.  Every element of the convolution is within 147 * 2^-24 * (|x| conv |w|) of the exact one (the
 *            worst case of an fp32 fmaf chain; ~3e-7 relative) for weights of any size — a channel whose largest
 *            |w| is below 2^-5 is split at a power-of-two scale that bn_scale takes back, inside the kernel — and
 *            images whose largest magnitude is at most 2^15 and whose typical magnitude is at least 2^-8;
 * flags = BNN_HIP_STEM_EXACT_FP32: v_mfma_f32_16x16x4_f32, bit-for-bit an fp32 fmaf chain.     */
#define BNN_HIP_STEM_EXACT_FP32 1
/* Plain fp16 operands, one MFMA per product, fp32 accumulation (the "fp16 MFMA stem" of BASELINE config 5):
 * ~5e-4 relative error instead of ~3e-7, one third of the matrix work.  Opt-in; not with EXACT_FP32.        */
#define BNN_HIP_STEM_FP16 4
/* (flag 8, BNN_HIP_STEM_STAGED until ABI 11 — the round-2 kernel of the same arithmetic — is rejected since ABI 12:
 * that kernel is a test-only cross-check now, csrc/legacy/stem_split.hip in libbnn_hip_legacy.so.)
 * Every tensor of a launch stays below 2^32 - 512 bytes (32-bit buffer descriptors): BNN_HIP_ERR_TOO_LARGE above
 * that — split the batch (~7100 images of 224 x 224 per launch).                                                    */
int bnn_hip_stem7x7_bn_relu_pool_pack_f32(const float* x, const float* w,
                                          const float* bn_scale, const float* bn_shift,
                                          int N, int H, int W, int flags,
                                          float* out_f32, uint64_t* P, uint64_t* M, void* stream);

/* ABI 14 — the stem's convolution ALONE, for the training forward (bnn/models/resnet.py:150: `x = self.conv1(x)`; the
 * BatchNorm of a training step needs the raw conv output for its batch statistics): conv 7x7 / stride 2 / pad 3,
 * 3 -> 64 channels, no bias.  x: float32 [N,3,H,W], w: float32 [64,3,7,7], out: float32 [N,64,Hc,Wc] with
 * Hc = (H - 1) / 2 + 1.  The same MFMA stream as the fused stem (fp32 operands as fp16 hi + lo, three products, fp32
 * accumulation; flags = BNN_HIP_STEM_FP16: plain fp16 operands): the values the fused kernel normalises and pools, bit
 * for bit.  Same size limits as the fused stem.                                                                     */
/* The same kernel with the sign planes taken behind a per-channel affine of its output (ABI 15):
 *     P = fmaf(y, pack_scale[c], pack_shift[c]) > 0,  M = 0          (y: the pooled ReLU output, written to out_f32 unchanged)
 * — what the first binary layer of a pre-activation network reads (HBlock: bn1 -> relu -> conv1, hierarchical_block.py:39):
 * the packing pass over the fp32 tensor (bnn_hip_bn_act_pack_f32, relu = 1) disappears, same bits.  flags: 0 or
 * BNN_HIP_STEM_FP16.                                                                                              */
int bnn_hip_stem7x7_bn_relu_pool_pack_affine_f32(const float* x, const float* w, const float* bn_scale,
                                                 const float* bn_shift, const float* pack_scale, const float* pack_shift,
                                                 int N, int H, int W, int flags, float* out_f32, uint64_t* P, uint64_t* M,
                                                 void* stream);
int bnn_hip_stem7x7_conv_f32(const float* x, const float* w, int N, int H, int W, int flags, float* out, void* stream);

/* ABI 14 — the weight gradient of that convolution: the training backward of bnn/models/resnet.py:150 (the input is data,
 * so this is the layer's whole backward; torch: aten::convolution_backward with output_mask = {0, 1, 0}).
 *   dw[o][c][ky][kx] = sum over n, y, x of dy[n][o][y][x] * x[n][c][2y + ky - 3][2x + kx - 3]        (zero padding)
 * x: float32 [N,3,H,W], dy: float32 [N,64,Hc,Wc] (Hc = (H - 1) / 2 + 1), dw: float32 [64,3,7,7] (overwritten).
 * fp32 products and fp32 accumulation on the matrix cores (v_mfma_f32_16x16x4_f32), per-workgroup partial sums in
 * `workspace` added in index order in fp64: deterministic, no atomics.  Two launches.  workspace: at least
 * bnn_hip_stem7x7_wgrad_workspace_bytes(N, H, W) bytes (0 = this shape is not supported: image rows wider than ~950
 * pixels do not fit the kernel's LDS patch, BNN_HIP_ERR_UNSUPPORTED — the caller keeps its own backward).          */
size_t bnn_hip_stem7x7_wgrad_workspace_bytes(int N, int H, int W);
int bnn_hip_stem7x7_wgrad_f32(const float* x, const float* dy, int N, int H, int W, float* workspace,
                              size_t workspace_bytes, float* dw, void* stream);

/* ABI 14 — backward of the shortcut's AvgPool2d(2, 2) on an even-sized map (bnn/models/resnet.py:128-133 in a training
 * step): gx[n, c, 2y + a, 2x + b] = gy[n, c, y, x] / 4.  gy: float32 [N,C,Ho,Wo], gx: float32 [N,C,2 Ho,2 Wo]
 * (overwritten).  One streaming launch.                                                                              */
int bnn_hip_avgpool2x2_backward_f32(const float* gy, int N, int C, int Ho, int Wo, float* gx, void* stream);

/* The real-valued head of the reference's ResNets in one kernel (bnn/models/resnet.py:160-164:
 * avgpool -> flatten -> fc):  out[n,o] = bias[o] + sum_c w_t[c,o] * mean_hw x[n,c,hw].
 * x: float32 [N,C,HW] (an NCHW tensor with HW = H*W), w_t: the Linear weight TRANSPOSED to [C,O]
 * (so that a wavefront reads contiguous bytes; nn.Linear stores [O,C]), bias: [O] or NULL,
 * out: float32 [N,O].  fp32 fmaf accumulation in index order; C*16 bytes of LDS (C <= 10240).       */
int bnn_hip_avgpool_fc_f32(const float* x, int N, int C, int HW, const float* w_t, const float* bias,
                           int O, float* out, void* stream);
/* ABI 14 — the same head as two launches through a caller-provided workspace (the library allocates nothing):
 * a streaming average-pool kernel (coalesced loads, the same index-order fp32 sums) into the workspace, then the
 * product as 16-image x 64-output tiles with the k range split over eight waves whose partial sums are added in
 * segment order.  workspace: bnn_hip_avgpool_fc_workspace_bytes(N, C) bytes, 16-byte aligned, contents undefined
 * before and after.  Shapes the two-launch form does not cover (C * 64 bytes of LDS above the CU's 160 KB) run the
 * one-kernel form.  Per-image results do not depend on N or on the image's position in the batch.
 * ResNet-18, batch 256: see profiles/ (round 5) — the one-kernel form is 28 us, latency-bound.                     */
size_t bnn_hip_avgpool_fc_workspace_bytes(int N, int C);
int bnn_hip_avgpool_fc_ws_f32(const float* x, int N, int C, int HW, const float* w_t, const float* bias,
                              int O, float* out, void* workspace, size_t workspace_bytes, void* stream);

/* XNOR-Net weight binarisation.  w: float32 [O,C,KH,KW] contiguous.
 *   center        != 0: subtract the mean over C per (o,ky,kx) first  (ops.py:130-132)
 *   compute_alpha != 0: alpha[o] = mean |w[o]| (after centering)      (ops.py:116-127)
 *                 == 0: alpha[o] = 1
 * Outputs: wbits, wnz (bnn_hip_weight_layout().n_words uint32 each), alpha[o_pad]
 * (pad channels get alpha 0), *zero_flag (int32, device) is OR-ed with 1 when some
 * in-range sign(w) == 0 (zero or NaN weight) — the caller clears it beforehand.    */
int bnn_hip_pack_weight_f32(const float* w, int O, int C, int KH, int KW,
                            int center, int compute_alpha,
                            uint32_t* wbits, uint32_t* wnz, float* alpha,
                            int32_t* zero_flag, void* stream);

/* ---- training: gradients of  out = conv2d(sign(x), What), What = sign(Wc) * alpha, for the
 * 3x3 / stride 1 or 2 / padding 1 layer and the 1x1 / stride 1 / padding 0 layer, dilation 1
 * (bnn/layers/conv.py:90-97 under autograd; input STE bnn/ops.py:68-73).  `ksize` is 3 or 1, p = ksize / 2.
 * Each is a GEMM with one real operand (the incoming gradient g, split into fp16 hi + lo) and one operand that is
 * exactly {-1,0,+1}: two v_mfma_f32_16x16x32_f16 per product, fp32 accumulation (fp32-convolution rounding class).
 * x: the layer's fp32 input [N,C,H,W], W <= 64; g: float32 [N,O,Hg,Wg] with Hg = (H-1)/stride + 1 (same for W).
 * Anything else (other kernel sizes, a strided 1x1, W > 64): BNN_HIP_ERR_UNSUPPORTED — the caller keeps its
 * fp32 path for those.
 *
 *   bnn_hip_grad_pack_weight_f32   What [O,C,k,k] (= +-alpha[o] or 0) -> alpha[o] = max|What[o]| and sign(What) as
 *                                  fp16 MFMA fragments in `packed` (bnn_hip_grad_weight_pack_bytes(O, C, k) bytes,
 *                                  16-byte aligned); once per optimiser step.
 *   bnn_hip_bconv_grad_input_f32   gx[n,c,y,x] = 1[|x| < 1] * sum_{o,ky,kx} g[n,o,(y+p-ky)/s,(x+p-kx)/s] * What[o,c,ky,kx]
 *                                  (terms whose (y+p-ky, x+p-kx) is not a multiple of the stride s do not exist)
 *   bnn_hip_bconv_grad_weight_f32  partial[s,o,c,ky,kx] = sum over the images of split s and all pixels of
 *                                  g[n,o,y,x] * sign(x)[n,c,s*y+ky-p,s*x+kx-p];  dL/dWhat = sum_s partial[s]
 *                                  (s < splits = bnn_hip_bconv_grad_weight_splits(N, O, C, k); the caller adds
 *                                  the `splits` slabs — a deterministic reduction instead of float atomics).       */
size_t bnn_hip_grad_weight_pack_bytes(int O, int C, int ksize);
int bnn_hip_grad_pack_weight_f32(const float* w_hat, int O, int C, int ksize, void* packed, float* alpha,
                                 void* stream);
int bnn_hip_bconv_grad_input_f32(const float* g, const float* alpha, const void* packed, const float* x, float* gx,
                                 int N, int O, int C, int H, int W, int ksize, int stride, void* stream);
int bnn_hip_bconv_grad_weight_splits(int N, int O, int C, int ksize);
int bnn_hip_bconv_grad_weight_f32(const float* g, const float* x, float* partial, int splits,
                                  int N, int O, int C, int H, int W, int ksize, int stride, void* stream);

/* ---- binary activations, REAL weights (additive entry points of ABI 16, no struct or signature changed): step 0 of
 * the reference's two-stage recipe (examples/recepies/imagenet-baseline.yaml: weight: nn.Identity), the layer
 * bnn/layers/conv.py:90-97 evaluates as conv2d(sign(x), W, b) * alpha in fp32.  One launch from the fp32 NCHW input:
 *
 *   bnn_hip_sconv2d_f32   y[n,o,p] = (sum_{c,tap} s(x)[n,c,p*stride + tap - ksize/2] * W[o,c,tap] + bias[o]) * post_scale[o]
 *
 * s(x) = +1 for x > 0, -1 for x < 0, 0 otherwise (+-0, NaN, the zero padding: the predicate of the bit planes).  A GEMM
 * with one operand exactly {-1,0,+1} and one real operand split into three bf16 terms: three v_mfma_f32_16x16x32_bf16
 * per product, every product exact, fp32 accumulation (the rounding class of an fp32 convolution).
 * Geometry: that of the gradient kernels above — ksize 3 (padding 1, stride 1 or 2) or 1 (padding 0, stride 1),
 * dilation 1, groups 1, W <= 64, any N, C, O.  Anything else: BNN_HIP_ERR_UNSUPPORTED (the caller keeps its fp32 path).
 * x: float32 [N,C,H,W]; y: float32 [N,O,Ho,Wo], Ho = (H-1)/stride + 1; bias, post_scale: float32 [O], each may be NULL
 * (no add / no multiply).
 *
 *   bnn_hip_sconv2d_pack_weight_f32   W [O,C,k,k] fp32 -> `packed` (bnn_hip_sconv2d_weight_pack_bytes(O, C, k) bytes,
 *                                     16-byte aligned); two launches; once per weight update.
 *
 * Byte layout of `packed`, CB = ceil(C/32), OS = ceil(O/16), T = k*k:
 *   Wp[cb][tap][os][term][lane][e]  bf16 (2 bytes), term 0/1/2 = hi/mid/lo, lane < 64, e < 8: one 16-byte MFMA B
 *                                   fragment per lane
 *       = term(W[o = 16 os + (lane & 15)][c = 32 cb + 8 (lane >> 4) + e][tap] * 2^kexp[o]);  0 for o >= O or c >= C
 *   kexp[16 OS]                     int32 at byte offset CB*T*OS*3*1024; 0 for o >= O
 * hi = the upper 16 bits of the fp32 value (truncation to bf16), mid the same of (value - hi), lo of (value - hi - mid),
 * each difference in fp32 (exact).  kexp[o] = 1 - exponent of the largest |W[o,:,:,:]| if that lies in (0, 1) — the
 * scaled row's largest magnitude is then in [1, 2) — and 0 otherwise; the kernel multiplies its accumulator by
 * 2^-kexp[o].  bf16 terms of the unscaled weight could not hold what lies below 2^-133: with the row exponent
 * hi + mid + lo == W * 2^kexp exactly for every finite weight within 2^-100 of its row's largest, subnormals included. */
size_t bnn_hip_sconv2d_weight_pack_bytes(int O, int C, int ksize);
int bnn_hip_sconv2d_pack_weight_f32(const float* w, int O, int C, int ksize, void* packed, void* stream);
int bnn_hip_sconv2d_f32(const float* x, const void* packed, const float* bias, const float* post_scale, float* y, int N,
                        int O, int C, int H, int W, int ksize, int stride, void* stream);

/* ABI 12: the same two gradients from 3 BITS per input element instead of the fp32 tensor — what a training step has
 * to keep of x between forward and backward (the reference's autograd keeps the fp32 x and the fp32 sign(x),
 * bnn/ops.py:63-73).  bnn_hip_pack_act_ste_f32 writes, in one pass over x, the sign planes P = x > 0, M = x < 0 (the
 * format of bnn_hip_pack_act_f32) and the straight-through mask T = |x| < 1 (NaN -> 0); the *_packed_* kernels read T
 * (input gradient) resp. P and M (weight gradient).  Results are bit-identical to the fp32-x entry points.            */
int bnn_hip_pack_act_ste_f32(const float* x, int N, int C, int H, int W, uint64_t* P, uint64_t* M, uint64_t* T,
                             void* stream);
/* The same three planes of u = fmaf(x, bn_scale[c], bn_shift[c]) — the expression of bnn_hip_bn_act_pack_f32 and of the
 * apply pass of bnn_hip_bn_train_forward_f32, so the bits of bnn_hip_pack_act_ste_f32 on their output — in one pass over
 * x, u never written.  bn_scale / bn_shift: fp32 [C], both or neither; both NULL: the bits of bnn_hip_pack_act_ste_f32.  */
int bnn_hip_bn_act_pack_ste_f32(const float* x, int N, int C, int H, int W, const float* bn_scale, const float* bn_shift,
                                uint64_t* P, uint64_t* M, uint64_t* T, void* stream);
/* The same three planes on the two pixel lattices FactorizedReduce reads (bnn/models/layers/bats_ops.py:204-206): phase 0
 * = u[2i, 2j], phase 1 = u[2i+1, 2j+1].  P, M, T: uint64 [2][N][ceil(C/64)][H/2][W/2] each (phase-major), 8-byte
 * aligned — per phase the bits of bnn_hip_bn_act_pack_ste_f32 on a contiguous copy of x[:, :, ::2, ::2] resp.
 * x[:, :, 1::2, 1::2]; P and M are the planes of bnn_hip_bn_act_pack_s2_f32 (relu = 0).  Pixels off the lattices are not
 * read.  H and W must be even (INVALID_ARG otherwise).  One launch.                                                  */
int bnn_hip_bn_act_pack_ste_s2_f32(const float* x, int N, int C, int H, int W, const float* bn_scale, const float* bn_shift,
                                   uint64_t* P, uint64_t* M, uint64_t* T, void* stream);
int bnn_hip_bconv_grad_input_packed_f32(const float* g, const float* alpha, const void* packed_w, const uint64_t* T,
                                        float* gx, int N, int O, int C, int H, int W, int ksize, int stride,
                                        void* stream);
int bnn_hip_bconv_grad_weight_packed_f32(const float* g, const uint64_t* P, const uint64_t* M, float* partial, int splits,
                                         int N, int O, int C, int H, int W, int ksize, int stride, void* stream);

/* Binary convolution on packed operands.  out: float32 [N,O,Ho,Wo] contiguous.
 *   out[n,o,y,x] = fmaf(alpha[o], dot, bias ? bias[o] : 0) * (post_scale ? post_scale[o] : 1)
 * wnz may be NULL unless BNN_HIP_FLAG_WEIGHT_ZEROS is set.                         */
int bnn_hip_bconv2d(const bnn_hip_conv_desc* d,
                    const uint64_t* P, const uint64_t* M,
                    const uint32_t* wbits, const uint32_t* wnz,
                    const float* alpha, const float* bias, const float* post_scale,
                    float* out, void* stream);

/* Binary convolution with the fused epilogue described at bnn_hip_epilogue.        */
int bnn_hip_bconv2d_fused(const bnn_hip_conv_desc* d,
                          const uint64_t* P, const uint64_t* M,
                          const uint32_t* wbits, const uint32_t* wnz,
                          const bnn_hip_epilogue* epi, void* stream);

/* HOST: 1 when bnn_hip_bconv2d_fused() takes a folded shortcut convolution of sc_C input channels (bnn_hip_epilogue
 * sc_*) for this convolution — 3x3 tiled kernels on non-negative activations (BNN_HIP_FLAG_ACT_NONNEG) without zero
 * weights, epilogue = BatchNorm + shortcut + ReLU -> fp32 + sign planes, sc_C in {64, 128, 256}; 0 otherwise.       */
int bnn_hip_shortcut_fold_supported(const bnn_hip_conv_desc* d, int sc_C);

/* ---- The dense 3x3 convolution on the int8 matrix cores (additive entry points of ABI 16, no struct or signature
 * changed; csrc/bconv_mfma.hip).  The same layer as bnn_hip_bconv2d_fused on the same sign planes, the dot taken by
 * v_mfma_i32_16x16x64_i8 instead of XNOR + popcount: operands in {-1,0,+1} are exact in int8 and the int32 accumulation
 * of at most 9 C such products is exact, so the integer dot — and, through the same float epilogue, every output bit —
 * equals bnn_hip_bconv2d_fused's.  About four times the popcount rate of the int ALU.
 *
 * Covered (bnn_hip_bconv2d_mfma_supported == 1): KH = KW = 3, padding 1, dilation 1, stride 1 or 2 (both directions
 * alike), C % 64 == 0, O % 64 == 0, sizes within the limits of the tiled popcount kernels, an image row narrow enough
 * for the kernel's LDS patch (64 KB: W up to ~380 at stride 1); epilogue: alpha [, bias] [, post_scale] [, BatchNorm]
 * [, residual] [, ReLU] -> fp32 and / or sign planes, sign_thresholds honoured as in bnn_hip_bconv2d_fused.  Not covered
 * (BNN_HIP_ERR_UNSUPPORTED, nothing launched): PReLU, the BNN_HIP_EPI_* flags, pack_scale / pack_shift, a channel window
 * (out_c_total != O), the folded shortcut (sc_*), BNN_HIP_FLAG_FORCE_GENERIC.  BNN_HIP_FLAG_ACT_NONNEG is honoured (M is
 * not read); the zero weights of the pack are always honoured, with or without BNN_HIP_FLAG_WEIGHT_ZEROS.
 *
 * bnn_hip_pack_weight_i8: wbits / wnz of bnn_hip_pack_weight_f32 -> `w8`, bnn_hip_weight_i8_bytes(O, C, KH, KW) = 9 O C
 * bytes (0: no int8 pack for this weight shape), 16-byte aligned; once per weight version.  alpha is used unchanged.
 * Byte layout, G = C / 64:
 *   w8[o / 64][g][tap][ct][lane][e]   int8, g < G, tap = 3 ky + kx, ct < 4, lane < 64, e < 16: one 16-byte MFMA operand
 *                                     fragment per lane, 4 KB per (64 output channels, group, tap)
 *       = sign(W[o = 64 (o / 64) + 16 ct + (lane & 15)][c = 64 g + 16 (lane >> 4) + e][tap])   as +1 / -1 / 0
 * (wnz bit ? (wbits bit ? +1 : -1) : 0).  The kernel expands the activation planes with the same channel order inside a
 * fragment; the sum over a fragment does not depend on that order, only on both operands sharing it.                 */
size_t bnn_hip_weight_i8_bytes(int O, int C, int KH, int KW);
int bnn_hip_pack_weight_i8(const uint32_t* wbits, const uint32_t* wnz, int O, int C, int KH, int KW, void* w8,
                           void* stream);
/* HOST: 1 when bnn_hip_bconv2d_mfma_fused() takes this convolution with this epilogue, 0 otherwise (invalid arguments
 * included).                                                                                                          */
int bnn_hip_bconv2d_mfma_supported(const bnn_hip_conv_desc* d, const bnn_hip_epilogue* epi);
int bnn_hip_bconv2d_mfma_fused(const bnn_hip_conv_desc* d, const uint64_t* P, const uint64_t* M, const void* w8,
                               const bnn_hip_epilogue* epi, void* stream);

/* ---- The same with the block's shortcut convolution folded in (additive entry points of ABI 16).  The launch of
 * bnn_hip_bconv2d_fused with epi->sc_* set (BatchNorm + shortcut + ReLU -> fp32 + sign planes), both dots on
 * v_mfma_i32_16x16x64_i8: the shortcut's 1x1 dot runs first through the same pipeline (operand B: the P plane sc_P at the
 * output pixels, OR-pooled in the kernel when sc_in_hw != 0), waits in LDS as int16 and enters the epilogue as
 *     r = fmaf(fmaf(sc_alpha[o], (float)dot, 0), sc_bn_scale[o], sc_bn_shift[o])
 * — the float operations of the popcount fold on the same integer, so every output bit equals bnn_hip_bconv2d_fused's.
 * epi->sc_wbits is not read (it may be NULL): the shortcut weight comes as `sc_w8`.
 *
 * Covered (bnn_hip_bconv2d_mfma_fold_supported == 1): what bnn_hip_bconv2d_mfma_supported covers, and: sc_* present;
 * epilogue exactly alpha, BatchNorm, ReLU, out_f32 and out_P / out_M (no bias, post_scale, residual, sign_thresholds);
 * BNN_HIP_FLAG_ACT_NONNEG; no BNN_HIP_FLAG_WEIGHT_ZEROS (the shortcut pack has no zero weights); sc_C in {64, 128,
 * 256}; the LDS patch plus 36 KB of parked shortcut dots within 80 KB (two workgroups per CU).
 *
 * bnn_hip_pack_shortcut_weight_i8: wbits of the 1x1 weight [O, C, 1, 1] (bnn_hip_pack_weight_f32; bit ? +1 : -1, no
 * zeros) -> `sc_w8`, bnn_hip_shortcut_weight_i8_bytes(O, C) = O C bytes (0: O % 64 != 0 or C not in {64, 128, 256}),
 * 16-byte aligned.  Byte layout, G = C / 64 — bnn_hip_pack_weight_i8's with one tap:
 *   sc_w8[o / 64][g][ct][lane][e]   int8, g < G, ct < 4, lane < 64, e < 16
 *       = W[o = 64 (o / 64) + 16 ct + (lane & 15)][c = 64 g + 16 (lane >> 4) + e]   as +1 / -1                        */
size_t bnn_hip_shortcut_weight_i8_bytes(int O, int C);
int bnn_hip_pack_shortcut_weight_i8(const uint32_t* wbits, int O, int C, void* sc_w8, void* stream);
/* HOST: 1 when bnn_hip_bconv2d_mfma_fold_fused() takes this convolution with this epilogue, 0 otherwise.            */
int bnn_hip_bconv2d_mfma_fold_supported(const bnn_hip_conv_desc* d, const bnn_hip_epilogue* epi);
int bnn_hip_bconv2d_mfma_fold_fused(const bnn_hip_conv_desc* d, const uint64_t* P, const uint64_t* M, const void* w8,
                                    const void* sc_w8, const bnn_hip_epilogue* epi, void* stream);

/* ---- Both of the above on the FP4 matrix-core instruction (additive entry points of ABI 16; csrc/bconv_mfma.hip, the
 * F4 form).  v_mfma_f32_16x16x128_f8f6f4 with E2M1 operands and no scales: -1, 0 and +1 are exact in E2M1 (0xA, 0x0,
 * 0x2), every product is in {-1, 0, +1} and every partial sum is an integer of magnitude <= 9 C <= 2^20 < 2^24, so every
 * fp32 addition is exact in any order; the accumulator converted to int is the same dot and every output bit equals
 * bnn_hip_bconv2d_fused's.  Half the matrix cycles, half the operand bytes and half the k-steps of the int8 form.
 *
 * Covered: bnn_hip_bconv2d_mfma4_supported == bnn_hip_bconv2d_mfma_supported && C % 128 == 0, and
 * bnn_hip_bconv2d_mfma4_fold_supported == bnn_hip_bconv2d_mfma_fold_supported && C % 128 == 0.  The arguments are those
 * of the int8 twins with `w4` in place of `w8`; the folded shortcut's weight stays bnn_hip_pack_shortcut_weight_i8's
 * `sc_w8` (its 1x1 prologue runs on the int8 instruction).
 *
 * bnn_hip_pack_weight_f4: wbits / wnz of bnn_hip_pack_weight_f32 -> `w4`, bnn_hip_weight_f4_bytes(O, C, KH, KW) =
 * 9 O C / 2 bytes (0: no int8 pack for this weight shape, or C % 128 != 0), 16-byte aligned; once per weight version.
 * Byte layout, G = C / 128:
 *   w4[o / 64][g][tap][ct][lane][e]   E2M1 nibbles, g < G, tap = 3 ky + kx, ct < 4, lane < 64, e < 32: nibble e is the
 *                                     low (e even) or high (e odd) half of byte e / 2 of the lane's 16-byte fragment,
 *                                     4 KB per (64 output channels, 128-channel group, tap)
 *       = sign(W[o = 64 (o / 64) + 16 ct + (lane & 15)][c = 128 g + 32 (lane >> 4) + e][tap])   as 0x2 / 0xA / 0x0
 * (wnz bit ? (wbits bit ? +1 : -1) : 0).  The kernel expands the activation planes with the same channel order.     */
size_t bnn_hip_weight_f4_bytes(int O, int C, int KH, int KW);
int bnn_hip_pack_weight_f4(const uint32_t* wbits, const uint32_t* wnz, int O, int C, int KH, int KW, void* w4,
                           void* stream);
int bnn_hip_bconv2d_mfma4_supported(const bnn_hip_conv_desc* d, const bnn_hip_epilogue* epi);
int bnn_hip_bconv2d_mfma4_fused(const bnn_hip_conv_desc* d, const uint64_t* P, const uint64_t* M, const void* w4,
                                const bnn_hip_epilogue* epi, void* stream);
int bnn_hip_bconv2d_mfma4_fold_supported(const bnn_hip_conv_desc* d, const bnn_hip_epilogue* epi);
int bnn_hip_bconv2d_mfma4_fold_fused(const bnn_hip_conv_desc* d, const uint64_t* P, const uint64_t* M, const void* w4,
                                     const void* sc_w8, const bnn_hip_epilogue* epi, void* stream);

/* ---- The dense 1x1 convolution on the FP4 matrix-core instruction (additive entry points of ABI 16, no struct or
 * signature changed; csrc/bconv1x1_mfma.hip).  The launch of bnn_hip_bconv2d_fused for KH = KW = 1 as a plain GEMM
 * [O, C] x [C, N H W] on v_mfma_f32_16x16x128_f8f6f4 with E2M1 operands: every partial sum is an integer of magnitude
 * <= C < 2^24, exact in fp32 in any order, and the accumulator converted to int enters the popcount kernels' epilogue, so
 * every output bit equals bnn_hip_bconv2d_fused's.
 *
 * Covered (bnn_hip_bconv1x1_mfma4_supported == 1): KH = KW = 1, stride 1, padding 0, dilation 1, C % 128 == 0,
 * O % 64 == 0, sizes within the limits of the tiled popcount kernels, N H W < 2^30; EVERY epilogue of
 * bnn_hip_bconv2d_fused — alpha [, bias] [, post_scale] [, BatchNorm] [, residual, early or BNN_HIP_EPI_RES_AFTER_ACT]
 * [, ReLU | PReLU] [, pack_scale / pack_shift] and the other BNN_HIP_EPI_* flags -> fp32 and / or sign planes,
 * sign_thresholds honoured as in bnn_hip_bconv2d_mfma_fused (BatchNorm + ReLU -> planes only; ignored elsewhere).  Not
 * covered (BNN_HIP_ERR_UNSUPPORTED, nothing launched): the folded shortcut (sc_*), a channel window (out_c_offset != 0 or
 * out_c_total != O), BNN_HIP_FLAG_FORCE_GENERIC.  BNN_HIP_FLAG_ACT_NONNEG is honoured (M is not read); the zero weights
 * of the pack are always honoured, with or without BNN_HIP_FLAG_WEIGHT_ZEROS.
 *
 * bnn_hip_pack_weight1x1_f4: wbits / wnz of bnn_hip_pack_weight_f32 for a [O, C, 1, 1] weight -> `w4`,
 * bnn_hip_weight1x1_f4_bytes(O, C) = O C / 2 bytes (0: O % 64 != 0 or C % 128 != 0), 16-byte aligned; KH = KW = 1, else
 * BNN_HIP_ERR_UNSUPPORTED.  Byte layout, G = C / 128 — bnn_hip_pack_weight_f4's with one tap:
 *   w4[o / 64][g][ct][lane][e]   E2M1 nibbles, g < G, ct < 4, lane < 64, e < 32 (nibble e: low / high half of byte e / 2)
 *       = sign(W[o = 64 (o / 64) + 16 ct + (lane & 15)][c = 128 g + 32 (lane >> 4) + e])   as 0x2 / 0xA / 0x0
 * The existing queries keep their answers: bnn_hip_weight_f4_bytes(O, C, 1, 1) == 0 and bnn_hip_bconv2d_mfma*_supported
 * say no to 1x1 weights, to PReLU and to a late residual.                                                              */
size_t bnn_hip_weight1x1_f4_bytes(int O, int C);
int bnn_hip_pack_weight1x1_f4(const uint32_t* wbits, const uint32_t* wnz, int O, int C, int KH, int KW, void* w4,
                              void* stream);
int bnn_hip_bconv1x1_mfma4_supported(const bnn_hip_conv_desc* d, const bnn_hip_epilogue* epi);
int bnn_hip_bconv1x1_mfma4_fused(const bnn_hip_conv_desc* d, const uint64_t* P, const uint64_t* M, const void* w4,
                                 const bnn_hip_epilogue* epi, void* stream);

/* ---- Which kernel a convolution runs (ABI 16): the route of bnn_hip_bconv2d / _fused / _dot, for tests. ----
 * The launch ladder of csrc/bconv.hip picks one instantiation per call from the kernel size, the chunk width, the
 * epilogue, the flags and the size of the grid.  The route query walks THAT ladder (the same statements, with the
 * launch itself skipped) and reports where it ends, so that a test can assert which kernel it is about to check.    */
enum {                          /* bnn_hip_conv_route.profile: the epilogue the kernel was compiled for */
  BNN_HIP_ROUTE_EP_PLAIN = 0,   /* alpha [, bias] [, post-scale] -> fp32                                */
  BNN_HIP_ROUTE_EP_RUNTIME = 1, /* anything, decided at run time (also every shape-generic launch)      */
  BNN_HIP_ROUTE_EP_MID = 2,     /* BN + ReLU -> planes                                                  */
  BNN_HIP_ROUTE_EP_OUT = 3,     /* BN + residual + ReLU -> fp32 + planes                                */
  BNN_HIP_ROUTE_EP_DS = 4,      /* BN -> fp32 (1x1 shortcut convolution)                                */
  BNN_HIP_ROUTE_EP_LAST = 5,    /* BN + residual + ReLU -> fp32                                         */
  BNN_HIP_ROUTE_EP_HB = 6,      /* hierarchical-block stages 1, 2                                       */
  BNN_HIP_ROUTE_EP_HB3 = 7,     /* hierarchical-block stage 3                                           */
  BNN_HIP_ROUTE_EP_MIDT = 8,    /* EP_MID through the integer sign thresholds                           */
  BNN_HIP_ROUTE_EP_OUTP = 9     /* BN + residual + ReLU -> planes                                       */
};
enum {                          /* bnn_hip_conv_route.site: the launch statement of the ladder, in source order */
  BNN_HIP_SITE_SINGLE_OBW = 0,      /* single-chunk 3x3, EP_PLAIN, several 32-channel blocks per wave           */
  BNN_HIP_SITE_SINGLE_SPLIT = 1,    /* single-chunk 3x3 split into pieces (compiled out: BNN_SINGLE_GSPLIT == 1) */
  BNN_HIP_SITE_SINGLE_FOLD = 2,     /* single-chunk 3x3 with the folded shortcut                                */
  BNN_HIP_SITE_SINGLE = 3,          /* single-chunk 3x3                                                         */
  BNN_HIP_SITE_MULTI4_SPLIT4 = 4,   /* multi-chunk 3x3 of chunk width 4, four pieces per block                  */
  BNN_HIP_SITE_MULTI4_SPLIT2_FOLD = 5, /* ... two pieces, folded shortcut                                      */
  BNN_HIP_SITE_MULTI4_SPLIT2 = 6,   /* ... two pieces                                                           */
  BNN_HIP_SITE_MULTI4_FOLD = 7,     /* ... unsplit, folded shortcut                                             */
  BNN_HIP_SITE_MULTI4 = 8,          /* ... unsplit                                                              */
  BNN_HIP_SITE_CHUNKS_FOLD = 9,     /* multi-chunk 3x3 of chunk width 2 with the folded shortcut                */
  BNN_HIP_SITE_CHUNKS = 10,         /* multi-chunk 3x3 of chunk width 2, and every 1x1                          */
  BNN_HIP_SITE_WZ_SINGLE = 11,      /* zero-weight kernel, single-chunk 3x3                                     */
  BNN_HIP_SITE_WZ_CHUNKS = 12,      /* zero-weight kernel, everything else                                      */
  BNN_HIP_SITE_GENERIC_WZ = 13,     /* shape-generic kernel honouring zero weights                              */
  BNN_HIP_SITE_GENERIC = 14,        /* shape-generic kernel                                                     */
  BNN_HIP_ROUTE_SITES = 15          /* number of launch statements                                              */
};
typedef struct bnn_hip_conv_route {
  int32_t tiled;           /* 1: bconv_sgpr_kernel; 0: the shape-generic bconv_generic_kernel                    */
  int32_t kh, kw;          /* kernel size the kernel was compiled for (generic: of the descriptor)               */
  int32_t cwc, nchunk;     /* 32-bit words per chunk of input channels, chunks (bnn_hip_weight_layout)           */
  int32_t profile;         /* BNN_HIP_ROUTE_EP_*                                                                 */
  int32_t nonneg;          /* 1: the P-only kernel (BNN_HIP_FLAG_ACT_NONNEG honoured; never for 1x1 or generic)   */
  int32_t weight_zeros;    /* 1: the kernel reads the wnz mask                                                   */
  int32_t multi;           /* 1: the kernel walks chunks (every 1x1 kernel does, also over one chunk)            */
  int32_t pieces;          /* waves that share one 32-channel block: 1, 2 or 4                                   */
  int32_t blocks_per_wave; /* 32-channel blocks one wave produces                                                */
  int32_t shortcut_fold;   /* 1: the kernel computes the folded shortcut convolution (bnn_hip_epilogue sc_*)      */
  int32_t site;            /* BNN_HIP_SITE_*                                                                     */
  int32_t reserved;        /* 0                                                                                  */
  int64_t waves;           /* workgroups (of one wave) of the launch                                             */
} bnn_hip_conv_route;

/* HOST: the route bnn_hip_bconv2d_fused(d, ..., e, ...) takes, or with e == NULL the route of bnn_hip_bconv2d(d, ...)
 * with any alpha / bias / post_scale.  Validates d and *e through the validator of those entry points (same status
 * codes, including BNN_HIP_ERR_UNSUPPORTED for a shortcut fold the shape does not take); the packed operands P, M,
 * wbits and wnz are not arguments and count as valid.  Launches nothing, calls no HIP function and reads through no
 * pointer of *e: those are only compared with NULL (and checked for alignment), so any non-null value describes "given".
 * *out is written only on BNN_HIP_OK.                                                                               */
int bnn_hip_bconv2d_route(const bnn_hip_conv_desc* d, const bnn_hip_epilogue* e, bnn_hip_conv_route* out);
/* HOST: the same for bnn_hip_bconv2d_dot(d, ...).                                                                    */
int bnn_hip_bconv2d_dot_route(const bnn_hip_conv_desc* d, bnn_hip_conv_route* out);

/* Same traversal, raw integer result: dot[n,o,y,x] (int32) — the bit-exact target
 * of the popcount path against the emulated-integer oracle.                        */
int bnn_hip_bconv2d_dot(const bnn_hip_conv_desc* d,
                        const uint64_t* P, const uint64_t* M,
                        const uint32_t* wbits, const uint32_t* wnz,
                        int32_t* dot, void* stream);

/* ---- Grouped and depthwise binary convolutions (additive entry points of ABI 15): bnn.layers.Conv2d / Conv1d built
 * with groups = G > 1 (bnn/layers/conv.py:90-97 passes `groups` to conv2d; the BATS cells' SepConv / DilConv,
 * bnn/models/layers/bats_ops.py:108-173, and the BATS ImageNet stem, bnn/models/bats.py:165,170).
 * Notation: C input channels, O output channels, Cg = C / G, Og = O / G; output channel o reads input channels
 * [(o / Og) Cg, (o / Og + 1) Cg).  Output block ob (32 channels o0 = 32 ob .. o1 = min(O, o0 + 32) - 1) reads the groups
 * g_lo = o0 / Og .. g_hi = o1 / Og, i.e. the 32-bit activation words
 *     w_lo(ob) = (g_lo Cg) / 32  ..  w_hi(ob) = ((g_hi + 1) Cg - 1) / 32.
 * Windowed block-diagonal weight layout: S = max over ob of (w_hi - w_lo + 1) words per tap, and
 *     wbits[ob][tap][s][j], wnz[ob][tap][s][j]   (uint32; j = o % 32 innermost: one (tap, word) of a block is 32
 *                                                consecutive words, a scalar-cache stream)
 * word s covers the absolute input channels 32 (w_lo(ob) + s) + b.  wbits bit b: sign(W) == +1; wnz bit b: W != 0 AND
 * the channel belongs to output channel o's group.  Pad output channels, window words past w_hi and words past the
 * activation planes are all zero in wnz.  The dot is the zero-aware form of bnn_hip_bconv2d:
 *     dot = popcount((P | M) & Z) - 2 popcount(disagree(W, M, P) & Z)
 * Depthwise (Cg = Og = 1) has S = 1.  bnn_hip_wlayout fields for this layout: cw32 = cwc = S (words per tap), nchunk = 1,
 * taps = KH KW, o_pad = O rounded up to 32, n_words = o_pad taps S, reserved = 0.
 *
 * HOST: the layout of a [O, C/groups, KH, KW] weight; C and O multiples of groups.                                      */
int bnn_hip_grouped_weight_layout(int O, int C, int groups, int KH, int KW, bnn_hip_wlayout* out);
/* XNORWeightBinarizer of a grouped weight w [O, Cg, KH, KW] (fp32 contiguous) into that layout.  center / compute_alpha
 * reduce over Cg and Cg KH KW as the reference does (bnn/ops.py:116-140): alpha[o_pad] holds the same bits as
 * bnn_hip_pack_weight_f32 of the same [O, Cg, KH, KW] tensor; *zero_flag as there.                                      */
int bnn_hip_pack_weight_grouped_f32(const float* w, int O, int Cg, int groups, int KH, int KW, int center,
                                    int compute_alpha, uint32_t* wbits, uint32_t* wnz, float* alpha,
                                    int32_t* zero_flag, void* stream);
/* The grouped convolution on bnn_hip_pack_act_f32 planes of all C = d->C input channels (d->O outputs, d->flags
 * ignored: the group mask makes every launch zero-aware).  out: float32 [N,O,Ho,Wo],
 *     out[n,o,y,x] = fmaf(alpha[o], dot, bias ? bias[o] : 0) * (post_scale ? post_scale[o] : 1)
 * alpha == NULL: `out` is an int32 [N,O,Ho,Wo] tensor and receives the integer dot (bias and post_scale must be NULL).
 * groups == 1 gives the bits of bnn_hip_bconv2d with BNN_HIP_FLAG_WEIGHT_ZEROS.  Same size limits and alignments as
 * bnn_hip_bconv2d (wnz is required, 16-byte aligned).                                                                   */
int bnn_hip_bconv2d_grouped(const bnn_hip_conv_desc* d, int groups, const uint64_t* P, const uint64_t* M,
                            const uint32_t* wbits, const uint32_t* wnz, const float* alpha, const float* bias,
                            const float* post_scale, float* out, void* stream);
/* The same convolution with the epilogue of a BATS cell operation (bnn/models/layers/bats_ops.py:108-173:
 * y = [x +] channel_shuffle(PReLU(conv(.)), 4)) in the one launch.  Per output channel o and pixel:
 *     v  = fmaf(alpha[o], dot, bias ? bias[o] : 0) * (post_scale ? post_scale[o] : 1)      the bits of bnn_hip_bconv2d_grouped
 *     v  = prelu ? (v >= 0 ? v : prelu[o] * v) : v                                         prelu: O floats
 *     o' = shuffle_groups > 1 ? (o % (O / shuffle_groups)) * shuffle_groups + o / (O / shuffle_groups) : o
 *     out[n,o',y,x] = residual ? residual[n,o',y,x] + v : v                                residual: float32 [N,O,Ho,Wo]
 * The product with the slope and the add of the residual are two separately rounded fp32 operations.
 * Everything bnn_hip_bconv2d_grouped requires, and: alpha != NULL (no raw-dot form); shuffle_groups >= 1 and
 * O % shuffle_groups == 0; residual, when given, 4-byte aligned and not overlapping `out` (no in-place skip).
 * prelu == NULL, shuffle_groups == 1, residual == NULL: the bits of bnn_hip_bconv2d_grouped.                             */
int bnn_hip_bconv2d_grouped_fused(const bnn_hip_conv_desc* d, int groups, const uint64_t* P, const uint64_t* M,
                                  const uint32_t* wbits, const uint32_t* wnz, const float* alpha, const float* bias,
                                  const float* post_scale, const float* prelu, int shuffle_groups,
                                  const float* residual, float* out, void* stream);

/* ---- The gradients of a grouped convolution in a training step (additive entry points of ABI 15;
 * csrc/grad_grouped.hip).  Both read the bit planes of bnn_hip_pack_act_ste_f32 over all C input channels, never the
 * fp32 input; plain fp32 arithmetic, no atomics: two runs on the same input give the same bits.
 *   input gradient   gx[n,c,y,x] = T bit ? sum_{o in group(c)} sum_{ky,kx} g[n,o,qy,qx] what[o, c mod Cg, ky, kx] : +0.0
 *                    qy = (y + pad_h - dil_h ky) / stride_h where that division is exact and 0 <= qy < Ho (x likewise);
 *                    what: float32 [O, Cg, KH, KW] (bnn_hip_xnor_weight_forward_f32 of the layer's weight); every
 *                    element of gx [N,C,H,W] is written.  T = |x| < 1: |x| == 1 is masked (bnn/ops.py:68-73).
 *   weight gradient  partial[s,o,cg,ky,kx] = sum_{n in split s} sum_{y,x} g[n,o,y,x] sign(x)[n, (o / Og) Cg + cg,
 *                    stride_h y + dil_h ky - pad_h, stride_w x + dil_w kx - pad_w]   (taps outside the image add nothing)
 *                    partial: float32 [splits, O, Cg, KH, KW]; split s holds the images [s N / splits, (s + 1) N / splits);
 *                    the caller adds the slabs (bnn_hip_xnor_weight_backward_f32 does, in slab order).
 * Covered: groups >= 2 dividing C and O, Cg <= 32, KH, KW <= 7, stride_h == stride_w in {1, 2}; any Og, width, dilation
 * and padding bnn_hip_bconv2d_grouped accepts; g and gx below 2^30 elements.  groups == 1 is BNN_HIP_ERR_UNSUPPORTED (the
 * dense layers have bnn_hip_bconv_grad_*); groups <= 0 or not dividing C and O, null or misaligned pointers (planes 8,
 * fp32 tensors 4 bytes) and splits outside 1 .. N are BNN_HIP_ERR_INVALID_ARG.  d->flags is ignored.
 * HOST: _supported returns 1 / 0; _weight_splits the library's choice of `splits` (1 .. min(N, 64)), 0 when unsupported. */
int bnn_hip_bconv_grouped_grad_supported(const bnn_hip_conv_desc* d, int groups);
int bnn_hip_bconv_grouped_grad_weight_splits(const bnn_hip_conv_desc* d, int groups);
int bnn_hip_bconv_grouped_grad_input_f32(const bnn_hip_conv_desc* d, int groups, const float* g, const float* what,
                                         const uint64_t* T, float* gx, void* stream);
int bnn_hip_bconv_grouped_grad_weight_f32(const bnn_hip_conv_desc* d, int groups, const float* g, const uint64_t* P,
                                          const uint64_t* M, float* partial, int splits, void* stream);

/* ---- A whole BATS cell (bnn/models/bats.py:9-83) as fused launches: additive entry points of ABI 15. ----
 * A channel-slice view of a contiguous fp32 NCHW tensor: channels [c_offset, c_offset + C) of [N, c_total, H, W] that
 * starts at p (C, N, H, W come from the call).  c_total == 0: the tensor is exactly the C channels used (c_offset must
 * be 0).  p is 4-byte aligned.                                                                                          */
typedef struct bnn_hip_f32_view {
  const float* p;
  int32_t c_offset;
  int32_t c_total;
} bnn_hip_f32_view;

/* K BatchNorm + sign() plane sets from ONE read of x (a cell state that feeds K operations, each with its own
 * BatchNorm): scale / shift are [K][C], 1 <= K <= 4; P / M are [K][N][ceil(C/64)][H][W] uint64.  Plane set k holds the
 * bits of bnn_hip_bn_act_pack_f32 on a contiguous copy of the view with scale[k] / shift[k] (both required here).      */
int bnn_hip_bn_act_pack_multi_f32(const bnn_hip_f32_view* x, int N, int C, int H, int W, int K, const float* scale,
                                  const float* shift, int relu, uint64_t* P, uint64_t* M, void* stream);
/* The binarisation inside FactorizedReduce (bats_ops.py:204-206): H and W even, one affine (or none: both NULL).
 * P / M are [2][N][ceil(C/64)][H/2][W/2]: phase 0 holds the pixels (2i, 2j), phase 1 the pixels (2i+1, 2j+1) — the bits
 * of bnn_hip_bn_act_pack_f32 on x[:, :, ::2, ::2] and on x[:, :, 1::2, 1::2] — from one pass over x.                    */
int bnn_hip_bn_act_pack_s2_f32(const bnn_hip_f32_view* x, int N, int C, int H, int W, const float* bn_scale,
                               const float* bn_shift, int relu, uint64_t* P, uint64_t* M, void* stream);
/* bnn_hip_bconv2d_grouped_fused as one term of a cell node  s = op1(h1) + op2(h2)  that stores into its slice of the
 * cell's concatenated output.  With v and o' as there:
 *     out[n, out_c_offset + o', y, x] = (residual ? residual[n,o',y,x] + v : v) + (addend ? addend[n,o',y,x] : 0)
 * three separately rounded fp32 operations (a missing operand is skipped, not added as zero).  `out` is channels
 * [out_c_offset, out_c_offset + O) of a [N, out_c_total, Ho, Wo] tensor that starts at `out` (out_c_total == 0: exactly
 * the O channels); residual / addend are views of O channels at the output resolution, each with a c_total of its own.
 * `out` must not alias an operand.  Two views are disjoint when their whole tensors do not overlap, or when they have
 * the same base pointer and c_total and their channel intervals are disjoint (a node reads one slice of the cell
 * output and writes another).  Every tensor involved stays below 2^30 elements.                                        */
int bnn_hip_bconv2d_grouped_node(const bnn_hip_conv_desc* d, int groups, const uint64_t* P, const uint64_t* M,
                                 const uint32_t* wbits, const uint32_t* wnz, const float* alpha, const float* bias,
                                 const float* post_scale, const float* prelu, int shuffle_groups,
                                 const bnn_hip_f32_view* residual, const bnn_hip_f32_view* addend, float* out,
                                 int out_c_offset, int out_c_total, void* stream);

/* ---- The BATS FactorizedConv ('conv_7x1_1x7', bnn/models/layers/bats_ops.py:55-75) in one launch: additive entry points
 * of ABI 16 (csrc/fconv.hip). ----
 *     y = [x +] channel_shuffle(PReLU(conv_Kx1(sign(BatchNorm(PReLU(conv_1xK(sign(BatchNorm(x)))))))), 4)
 * Two dense binary convolutions over C channels: [C,C,1,K] with stride (1, s) and padding (0, K/2), then [C,C,K,1] with
 * stride (s, 1) and padding (K/2, 0).  With Wm = (W-1)/s + 1, Ho = (H-1)/s + 1, Wo = Wm, every float operation rounded on
 * its own:
 *     dot1[n,m,y,xm] = zero-aware XNOR dot over (c, kx) of planes[n,c,y, s*xm + kx - K/2] and w1[m,c,0,kx]   (outside the image: 0)
 *     v = fmaf(alpha1[m], dot1, bias1 ? bias1[m] : 0);  v *= post_scale1[m] (if given);  v = v >= 0 ? v : prelu1[m]*v (if given)
 *     p = fmaf(v, mid_scale[m], mid_shift[m]);          t[n,m,y,xm] = (p > 0) - (p < 0)        (NaN, +-0 -> 0: the planes' predicate)
 *     dot2[n,o,yo,xo] = zero-aware dot over (m, ky) of t[n,m, s*yo + ky - K/2, xo] and w2[o,m,ky,0]   (rows outside the image: 0)
 *     v = fmaf(alpha2[o], dot2, bias2 ? bias2[o] : 0);  v *= post_scale2[o] (if given);  v = v >= 0 ? v : prelu2[o]*v (if given)
 *     o' = (o % (C/sg)) * sg + o / (C/sg)     (sg = shuffle_groups; 1: o' = o)
 *     out[n,o',yo,xo] = residual ? residual[n,o',yo,xo] + v : v
 * The bits of: bnn_hip_bconv2d_fused of the 1 x K layer (prelu, pack_scale / pack_shift = mid_scale / mid_shift, planes
 * only), bnn_hip_bconv2d_fused of the K x 1 layer (prelu), then shuffle and add as separate fp32 passes.  t is kept in LDS
 * as two bit planes: it is never written to global memory, and no fp32 intermediate exists.
 * P / M: bnn_hip_bn_act_pack_f32 planes [N, ceil(C/64), H, W]; w1bits / w1nz and w2bits / w2nz: bnn_hip_pack_weight_f32 of
 * the two weights (wnz may be NULL unless BNN_HIP_FLAG_WEIGHT_ZEROS is set in d->flags: then both masks are honoured);
 * s1 / s2: the per-channel constants of the two stages (alpha [o_pad] from the weight pack, the rest [C] or NULL);
 * mid_scale / mid_shift: the folded BatchNorm between the convolutions, [C]; residual, out: float32 [N, C, Ho, Wo], not
 * overlapping.  Planes and weight words 16-byte aligned, fp32 tensors 4.
 * Covered (bnn_hip_fconv_supported, HOST: 1 / 0): K in {1, 3, 5, 7}, stride in {1, 2}, and
 * 2 * ceil(C/64) * K * Wm * 8 bytes (K rows of t) within the 64 KB of LDS a workgroup takes: a workgroup computes a band
 * of output rows of one image — the whole image where 2 * ceil(C/64) * (s*(Ho-1) + K) * Wm * 8 bytes fit — and the
 * s*(rows-1) + K rows of t under it.  Anything else: BNN_HIP_ERR_UNSUPPORTED (the composition above is the fallback).
 * Null or misaligned pointers, non-positive sizes, shuffle_groups < 1 or not dividing C: BNN_HIP_ERR_INVALID_ARG; planes
 * of 2^29 words or an fp32 tensor of 2^30 elements and more: BNN_HIP_ERR_TOO_LARGE (split the batch).                  */
typedef struct bnn_hip_fconv_desc {
  int32_t N, C, H, W;   /* input [N,C,H,W]                                       */
  int32_t K;            /* kernel extent of both convolutions                    */
  int32_t stride;       /* (1, s) then (s, 1)                                    */
  int32_t flags;        /* BNN_HIP_FLAG_WEIGHT_ZEROS                             */
  int32_t reserved;     /* 0                                                     */
} bnn_hip_fconv_desc;
typedef struct bnn_hip_fconv_stage {
  const float* alpha;      /* [o_pad]                                            */
  const float* bias;       /* [C] or NULL                                        */
  const float* post_scale; /* [C] or NULL                                        */
  const float* prelu;      /* [C] or NULL                                        */
} bnn_hip_fconv_stage;
int bnn_hip_fconv_supported(const bnn_hip_fconv_desc* d);
int bnn_hip_fconv_fused(const bnn_hip_fconv_desc* d, const uint64_t* P, const uint64_t* M, const uint32_t* w1bits,
                        const uint32_t* w1nz, const bnn_hip_fconv_stage* s1, const uint32_t* w2bits, const uint32_t* w2nz,
                        const bnn_hip_fconv_stage* s2, const float* mid_scale, const float* mid_shift, int shuffle_groups,
                        const float* residual, float* out, void* stream);

/* ---- The real-valued stem of a BATS CIFAR network with the binarisation of its consumers (additive, ABI 15). ----
 * Conv2d(3, O, 3, stride 1, padding 1, no bias) -> folded BatchNorm -> ReLU (bnn/models/bats.py:118-122), and K plane
 * sets of the result, one per ReLUConvBN that reads it (bats_ops.py:78-105), in one launch:
 *     acc = 0;  over (c, kh, kw) in that order:  acc = fmaf(x[n,c,y+kh-1,x+kw-1], w[o,c,kh,kw], acc)   (padding: x = 0)
 *     v   = fmaxf(fmaf(acc, bn_scale[o], bn_shift[o]), 0)
 *     plane set k = the bits of bnn_hip_bn_act_pack_multi_f32 on v with pack_scale[k][o] / pack_shift[k][o], relu = 0
 * x: [N,3,H,W]; w: [O,3,3,3]; pack_scale / pack_shift: [K][O], 1 <= K <= 4; P / M: [K][N][ceil(O/64)][H][W] uint64
 * (8-byte aligned).  y: fp32 [N,O,H,W] receives v, or NULL: v is not written.  N*O*H*W and N*3*H*W stay below 2^31
 * (BNN_HIP_ERR_TOO_LARGE: split the batch).                                                                            */
int bnn_hip_stem3x3_bn_relu_pack_f32(const float* x, const float* w, const float* bn_scale, const float* bn_shift,
                                     const float* pack_scale, const float* pack_shift, int N, int O, int H, int W, int K,
                                     uint64_t* P, uint64_t* M, float* y, void* stream);

/* ---- The two real-valued stems of a BATS ImageNet network, one launch each (additive, ABI 15). ----
 * bnn/models/bats.py:161-172.  With H1 = (H + 1) / 2, H2 = (H1 + 1) / 2 (W alike), Cig = (input channels) / G and
 * Cog = (output channels) / G per group, g = o / Cog; every convolution is 3x3, stride 2, padding 1, without bias, and a
 * tap outside its input contributes nothing:
 *
 * bnn_hip_stem_s2x2_f32 — stem0: Conv2d(3, C1) -> BatchNorm -> ReLU -> Conv2d(C1, C, groups G) -> BatchNorm [-> ReLU]
 *     acc1 = 0;  over (ci, kh, kw) in that order:  acc1 = fmaf(x[n,ci,2p+kh-1,2q+kw-1], w1[c,ci,kh,kw], acc1)
 *     y1[n,c,p,q] = fmaxf(fmaf(acc1, s1[c], t1[c]), 0)                                   on the H1 x W1 map
 *     acc2 = 0;  over (j, kh, kw) in that order:   acc2 = fmaf(y1[n,g*Cig+j,2p+kh-1,2q+kw-1], w2[o,j,kh,kw], acc2)
 *     y[n,o,p,q]  = fmaf(acc2, s2[o], t2[o]), then fmaxf(., 0) when relu_out               on the H2 x W2 map
 *   A tap of the second convolution outside the H1 x W1 map is padding (zero), not the max(t1, 0) the first convolution
 *   would produce there.  y1 is never written to memory.  x: [N,3,H,W]; w1: [C1,3,3,3]; s1 / t1: [C1]; w2: [C,C1/G,3,3];
 *   s2 / t2: [C]; y: [N,C,H2,W2].  G divides C1 and C (else INVALID_ARG); C1 / G <= BNN_HIP_STEM_S2X2_MAX_GROUP_CHANNELS and
 *   G <= 65535 (else UNSUPPORTED); N*3*H*W and N*C*H2*W2 stay below 2^31 (TOO_LARGE: split the batch).
 *
 * bnn_hip_gconv3x3s2_bn_pack_f32 — stem1: [ReLU ->] Conv2d(C, O, groups G) -> BatchNorm, and the sign planes of K consumers
 *     x' = relu_in ? fmaxf(x, 0) : x
 *     acc = 0;  over (j, kh, kw) in that order:  acc = fmaf(x'[n,g*Cig+j,2p+kh-1,2q+kw-1], w[o,j,kh,kw], acc)
 *     v   = fmaf(acc, bn_scale[o], bn_shift[o])                                           on the H1 x W1 map
 *     plane set k = the bits of bnn_hip_bn_act_pack_multi_f32 on v with pack_scale[k][o] / pack_shift[k][o], relu = 0
 *   x: [N,C,H,W]; w: [O,C/G,3,3]; pack_scale / pack_shift: [K][O], 0 <= K <= 4; P / M: [K][N][ceil(O/64)][H1][W1] uint64
 *   (8-byte aligned; unused when K == 0).  y: fp32 [N,O,H1,W1] receives v, or NULL (only when K >= 1): v is not written.
 *   G divides C and O (else INVALID_ARG); C / G <= BNN_HIP_GCONV3X3S2_MAX_GROUP_CHANNELS and ceil(O / 64) <= 65535 (else
 *   UNSUPPORTED); N*C*H*W and N*O*H1*W1 stay below 2^31 (TOO_LARGE).
 * Both kernels work on BNN_HIP_STEM_S2_TILE_H x BNN_HIP_STEM_S2_TILE_W tiles of output pixels; any H, W >= 1 is covered. */
#define BNN_HIP_STEM_S2_TILE_H 4
#define BNN_HIP_STEM_S2_TILE_W 16
#define BNN_HIP_STEM_S2X2_MAX_GROUP_CHANNELS 32
#define BNN_HIP_GCONV3X3S2_MAX_GROUP_CHANNELS 40
int bnn_hip_stem_s2x2_f32(const float* x, const float* w1, const float* s1, const float* t1, const float* w2,
                          const float* s2, const float* t2, int N, int C1, int C, int G, int H, int W, int relu_out,
                          float* y, void* stream);
int bnn_hip_gconv3x3s2_bn_pack_f32(const float* x, const float* w, const float* bn_scale, const float* bn_shift,
                                   const float* pack_scale, const float* pack_shift, int N, int C, int O, int G, int H,
                                   int W, int relu_in, int K, uint64_t* P, uint64_t* M, float* y, void* stream);

/* Binary fully-connected layer: x packed as [B][ceil(F/64)] planes (pack_act with
 * H=W=1, i.e. [B][ceil(F/64)] words), weight packed with KH=KW=1.  out: float32 [B,O].                         */
int bnn_hip_blinear(int B, int F, int O,
                    const uint64_t* P, const uint64_t* M,
                    const uint32_t* wbits, const uint32_t* wnz, int weight_zeros,
                    const float* alpha, const float* bias, const float* post_scale,
                    float* out, void* stream);

/* ---- Linear as GEMM-shaped kernels (additive, ABI 16): bnn.layers.Linear.forward (bnn/layers/linear.py:22-27) from the
 * FLOAT input in one launch, and its two gradients under the straight-through estimator (bnn/ops.py:68-73).  Leading
 * dimensions are flattened by the caller: x is row-major [M, F].  The weight is the 1x1 pack of bnn_hip_pack_weight_f32
 * (O, F, 1, 1).  Sizes: M, F, O > 0; M * F and M * O below 2^30 per launch (BNN_HIP_ERR_TOO_LARGE: split M); more than
 * 65535 * 256 features or 65535 * 64 output channels: BNN_HIP_ERR_UNSUPPORTED.
 *
 *   bnn_hip_blinear_direct          out[m,o] = fmaf(alpha[o], dot(sign(x[m,:]), sign(Wc[o,:])), bias[o]) [* post_scale[o]]:
 *                                   the bits of bnn_hip_bconv2d_direct / bnn_hip_blinear on the same operands.  x: fp32
 *                                   (4-byte aligned), fp16 or bf16 (2-byte aligned), x_dtype = BNN_HIP_DTYPE_*; wbits / wnz
 *                                   16-byte aligned, wnz may be NULL unless weight_zeros; bias / post_scale may be NULL;
 *                                   out fp32 [M,O].  P, Mn, T: all NULL, or all three 8-byte aligned [M][ceil(F/64)]
 *                                   words that receive x > 0, x < 0 and |x| < 1 — the planes of bnn_hip_pack_act_ste_f32
 *                                   with H = W = 1, pad bits of the last word 0 — from the same pass over x.
 *                                   lds_words: 32-bit words per row that one LDS pass over F holds (rounded down to the
 *                                   pack's chunk, at least one chunk); 0 = the default (128).  Same bits for any value.
 *   bnn_hip_blinear_grad_input_f32  gx[m,f] = 1[|x[m,f]| < 1] * sum_o g[m,o] alpha[o] sign(Wc)[o,f]; g fp32 [M,O], alpha
 *                                   [O], wbits AND wnz of the forward's pack (16-byte aligned), T the mask plane of
 *                                   the forward (8-byte aligned), gx fp32 [M,F].  g' = alpha g is rounded once in fp32 and
 *                                   split into three bf16 terms; v_mfma_f32_16x16x32_bf16, fp32 accumulation.
 *   bnn_hip_blinear_grad_weight_f32 partial[s,o,f] = sum over the rows m of split s of g[m,o] sign(x)[m,f] from the P / Mn
 *                                   planes (8-byte aligned); partial fp32 [splits,O,F].  Split s holds rows
 *                                   [s * per, min(M, (s+1) * per)), per = ceil(M / splits); a `splits` outside 1..M or
 *                                   with ceil(M / per) != splits is BNN_HIP_ERR_INVALID_ARG (the rule of
 *                                   bnn_hip_bconv_grad_weight_f32).  bnn_hip_blinear_grad_weight_splits returns the default
 *                                   (a valid one), or BNN_HIP_ERR_INVALID_ARG for sizes the kernels reject.  The slabs go to
 *                                   bnn_hip_xnor_weight_backward_f32 as they are.                                          */
int bnn_hip_blinear_direct(int M, int F, int O, const void* x, int x_dtype, const uint32_t* wbits, const uint32_t* wnz,
                           int weight_zeros, const float* alpha, const float* bias, const float* post_scale, float* out,
                           uint64_t* P, uint64_t* Mn, uint64_t* T, int lds_words, void* stream);
int bnn_hip_blinear_grad_input_f32(const float* g, const float* alpha, const uint32_t* wbits, const uint32_t* wnz,
                                   const uint64_t* T, float* gx, int M, int O, int F, void* stream);
int bnn_hip_blinear_grad_weight_splits(int M, int O, int F);
int bnn_hip_blinear_grad_weight_f32(const float* g, const uint64_t* P, const uint64_t* Mn, float* partial, int splits, int M,
                                    int O, int F, void* stream);

/* ---- Linear with binary activations and REAL weights (additive entry points of ABI 16, no struct or signature changed):
 * the fully-connected layer of step 0 of the two-stage recipe, bnn/layers/linear.py:22-27 with weight: nn.Identity, which
 * the reference evaluates as F.linear(sign(x), W, b) * alpha in fp32.  One launch from the fp32 row-major input:
 *
 *   bnn_hip_slinear_f32   out[m,o] = (sum_f s(x[m,f]) * W[o,f] + bias[o]) * post_scale[o]
 *
 * s(x) and the arithmetic are those of bnn_hip_sconv2d_f32: +1 / -1 / 0 for x > 0 / x < 0 / anything else, the weight
 * split into three bf16 terms, three v_mfma_f32_16x16x32_bf16 per product, fp32 accumulation, then * 2^-kexp[o], + bias[o],
 * * post_scale[o] in that order.  Leading dimensions are flattened by the caller.
 * x: float32 [M,F] row-major (4-byte aligned: any F); packed: bnn_hip_sconv2d_pack_weight_f32(W.view(O,F,1,1), O, F, 1),
 * 16-byte aligned; bias, post_scale: float32 [O], each may be NULL (no add / no multiply); out: float32 [M,O].
 * P, Mn, T: all NULL, or all three 8-byte aligned [M][ceil(F/64)] words that receive x > 0, x < 0 and |x| < 1 — the planes
 * of bnn_hip_pack_act_ste_f32 with H = W = 1, pad bits of the last word 0 — from the same pass over x (a mix of NULL and
 * non-NULL: BNN_HIP_ERR_INVALID_ARG).  Sizes: M, F, O > 0 (BNN_HIP_ERR_INVALID_ARG); M * F and M * O below 2^30 per launch
 * (BNN_HIP_ERR_TOO_LARGE: split M).
 *
 *   bnn_hip_ste_mask_f32  gx[m,f] = T bit (m,f) ? gx[m,f] : +0.0f   in place: the hard-tanh straight-through mask on an
 *                         input gradient [M,F] (4-byte aligned) from the mask plane T [M][ceil(F/64)] (8-byte aligned);
 *                         M, F > 0, M * F below 2^30.                                                                  */
int bnn_hip_slinear_f32(int M, int F, int O, const float* x, const void* packed, const float* bias, const float* post_scale,
                        float* out, uint64_t* P, uint64_t* Mn, uint64_t* T, void* stream);
int bnn_hip_ste_mask_f32(float* gx, const uint64_t* T, int M, int F, void* stream);

/* ---- The LAYER in one launch (ABI 10): bnn.layers.Conv2d.forward (bnn/layers/conv.py:90-97) from the float
 * activation tensor to the float output, sign(x) (bnn/ops.py:63-66,151-152) computed ON THE FLY inside the
 * convolution kernel: a workgroup binarises its band of the input (whole images, or a run of output rows of one
 * image with its halo) straight into LDS as two bit planes and convolves it from there — no packed copy of the
 * activations in HBM, no workspace, the input is read once.  Same integers, same float epilogue, same bits as
 * bnn_hip_pack_act_f32 + bnn_hip_bconv2d.
 *   x: [N,C,H,W] contiguous, x_dtype = BNN_HIP_DTYPE_F32 (4-byte aligned), BNN_HIP_DTYPE_F16 or BNN_HIP_DTYPE_BF16
 *      (2-byte aligned; a 16-bit model or autocast: the planes are those of the exactly widened values);
 *      N*C*H*W < 2^30 elements per launch.
 *   out: fp32 [N,O,Ho,Wo], 4-byte aligned — or, with BNN_HIP_FLAG_OUT_F16 / BNN_HIP_FLAG_OUT_BF16 in d->flags, a tensor
 *      of that 16-bit type, 2-byte aligned, rounded inside the kernel (see the flags).
 *   plan: NULL = bnn_hip_bconv2d_direct_plan()'s choice.  A caller's plan (tests, tuning) supplies
 *      images_per_band / rows_per_band / waves / blocks_per_unit / pack_ahead / fine_head / fine_tail /
 *      producers;
 *      lds_bytes and n_bands are outputs.
 * Returns BNN_HIP_ERR_UNSUPPORTED when not even one output row of one image with its halo fits into the 160 KiB
 * of LDS of a CU (or an index factor leaves the 24-bit multiplies of the tiled kernels): use
 * bnn_hip_pack_act_f32 + bnn_hip_bconv2d (what bnn_hip_bconv2d_f32 does by itself) for those.                   */
#define BNN_HIP_DTYPE_F32 0
#define BNN_HIP_DTYPE_F16 1
#define BNN_HIP_DTYPE_BF16 2
typedef struct bnn_hip_fly_plan {
  int32_t images_per_band;  /* whole images per workgroup (>= 1); > 1 only with rows_per_band == Ho            */
  int32_t rows_per_band;    /* output rows per workgroup: Ho = whole images                                     */
  int32_t waves;            /* wavefronts per workgroup, 1..16                                                  */
  int32_t blocks_per_unit;  /* 32-channel output blocks per (coarse) work unit = per load of the field: 1, 2 or 4 */
  int32_t pack_ahead;       /* pixel groups (64 pixels) the binarisation is kept in front of the convolution;
                               < 0 = the planner's default                                                      */
  int32_t fine_head;        /* pixel groups at the start / end of a band that are split into single-pass units    */
  int32_t fine_tail;        /* (8 output channels of one block each); < 0 = the planner's default                 */
  int32_t producers;        /* wavefronts per workgroup that binarise the band front to back before they join the
                               convolution (0: every wave packs what it needs itself); < 0 = the planner's default */
  int32_t lds_bytes;        /* out: dynamic LDS per workgroup                                                   */
  int32_t n_bands;          /* out: workgroups of the launch                                                    */
} bnn_hip_fly_plan;
/* HOST: the plan bnn_hip_bconv2d_direct(plan = NULL) uses for this geometry. */
int bnn_hip_bconv2d_direct_plan(const bnn_hip_conv_desc* d, bnn_hip_fly_plan* plan);
int bnn_hip_bconv2d_direct(const bnn_hip_conv_desc* d, const void* x, int x_dtype,
                           const uint32_t* wbits, const uint32_t* wnz,
                           const float* alpha, const float* bias, const float* post_scale,
                           float* out, const bnn_hip_fly_plan* plan, void* stream);

/* ---- The hierarchical block in one launch (ABI 15): bnn.models.layers.HBlock.forward
 * (bnn/models/layers/hierarchical_block.py:38-60) behind its first BatchNorm + activation:
 *     o1 = conv1(sign(act1(bn1(x))));  o2 = conv2(sign(act2(bn2(o1))));  o3 = conv3(sign(act3(bn3(o2))))
 *     y  = cat(o1, o2, o3) + residual
 * three 3x3 / stride 1 / padding 1 binary convolutions (C_in -> C/2 -> C/4 -> C/4, C = `planes`) with ReLU
 * activations: every sign plane between them is non-negative (P plane only) and stays in LDS; a workgroup owns whole
 * images or a band of rows of one image with its halo (csrc/hblock.hip).  Bit-identical to three bnn_hip_bconv2d_fused
 * launches with BNN_HIP_EPI_RES_AFTER_ACT | PACK_BEFORE_RES | PACK_RELU.
 *   in_P:     the block's input planes, sign(act1(bn1(x))): [N, ceil(C_in/64), H, W] uint64, P plane (bnn_hip_bn_act_pack_f32
 *             with relu = 1, or the out_P of the previous block's launch)
 *   weights:  bnn_hip_hblock_pack_weights() of the three standard weight packs (no zero weights; bias-free convolutions)
 *   consts:   fp32, offsets from bnn_hip_hblock_layout_of(): alpha of conv1 / conv2 / conv3 | folded bn2 scale, shift |
 *             folded bn3 scale, shift | the NEXT block's folded bn1 scale, shift over all C channels (read only when out_P != NULL)
 *   residual: fp32 [N, C, H, W] (the block input, or its shortcut branch);  out: fp32 [N, C, H, W], must not alias residual
 *   out_P:    NULL, or [N, C/64, H, W] uint64: sign(relu(fmaf(y, next_a, next_b))) — the next block's in_P
 * planes % 64 == 0; C_in <= 32 or C_in % 64 == 0; N * planes < 2^23; N * planes * H * W < 2^30.                     */
/* flags bit of bnn_hip_hblock_desc: the SMALL-image form of the kernel (csrc/hblock_cl.hip: 14 x 14 and 7 x 7 images, planes a
 * multiple of 256, C_in a multiple of 64): a wave's lanes are 64 output channels instead of 64 pixels — no idle lanes on 196- or
 * 49-pixel images, taps in the left / right padding not computed.  `weights` must then come from
 * bnn_hip_hblock_pack_weights_cl (same size, another order); consts and results are the same, bit for bit.        */
#define BNN_HIP_HBLOCK_CHANNEL_LANES 128
typedef struct bnn_hip_hblock_desc {
  int32_t N, C_in, H, W;
  int32_t planes;
  int32_t flags;            /* BNN_HIP_FLAG_THROUGHPUT: other work shares the GPU — whole-image regions preferred;
                               BNN_HIP_HBLOCK_CHANNEL_LANES (below)                                                   */
  int32_t rows_per_band;    /* 0 = the planner's choice; else rows of one image per workgroup                         */
  int32_t images_per_band;  /* 0 = the planner's choice; > 1 only with rows_per_band == 0 or H                         */
  int32_t waves;            /* 0 = 16; wavefronts per workgroup, 1..16                                                */
  int32_t reserved;
} bnn_hip_hblock_desc;
/* Alignment, all three hblock entry points (bnn_hip_hblock_forward, _pool_forward, _shortcut_forward): `consts` 32 bytes (the
 * kernels read it eight floats at a time; the layout's offsets keep every piece on such a boundary), `weights` 64 bytes, the
 * uint64 planes 8 bytes, the fp32 tensors 4 bytes — except with BNN_HIP_HBLOCK_CHANNEL_LANES on 14 x 14 images, where
 * `residual` and `out` are accessed two pixels at a time and must be 8-byte aligned.  A misaligned pointer is refused with
 * BNN_HIP_ERR_INVALID_ARG before any launch.                                                                          */
typedef struct bnn_hip_hblock_layout {
  int64_t weight_words;     /* uint32 words of the weight buffer (64-byte aligned)                                    */
  int64_t w_off[3];         /* word offset of conv1 / conv2 / conv3 in it                                             */
  int64_t const_floats;     /* floats of the constants buffer                                                         */
  int64_t alpha_off[3];     /* float offsets: alpha[O_k] of conv k                                                    */
  int64_t pack_a_off[2], pack_b_off[2];  /* folded bn2 (C/2 values each) and bn3 (C/4)                                */
  int64_t next_a_off, next_b_off;        /* the next block's folded bn1 (C values each)                               */
} bnn_hip_hblock_layout;
/* HOST: 1 when bnn_hip_hblock_forward covers this geometry on the current device, else 0. */
int bnn_hip_hblock_supported(const bnn_hip_hblock_desc* d);
/* HOST: buffer sizes and offsets for a block of this shape. */
int bnn_hip_hblock_layout_of(int C_in, int planes, bnn_hip_hblock_layout* out);
/* wbits1..3: bnn_hip_pack_weight_f32 packs of [C/2, C_in, 3, 3], [C/4, C/2, 3, 3], [C/4, C/4, 3, 3]. */
int bnn_hip_hblock_pack_weights(int C_in, int planes, const uint32_t* wbits1, const uint32_t* wbits2,
                                const uint32_t* wbits3, uint32_t* weights, void* stream);
int bnn_hip_hblock_pack_weights_cl(int C_in, int planes, const uint32_t* wbits1, const uint32_t* wbits2,
                                   const uint32_t* wbits3, uint32_t* weights, void* stream);
int bnn_hip_hblock_forward(const bnn_hip_hblock_desc* d, const uint64_t* in_P, const uint32_t* weights,
                           const float* consts, const float* residual, float* out, uint64_t* out_P, void* stream);

/* The last block of a stage in front of `AvgPool2d(2, 2)` and a block with a shortcut convolution (ABI 15;
 * bnn/models/resnet.py: the stages of the hierarchical-block network, hierarchical_block.py:30-39): the block's output is
 * only ever pooled and binarised — by the next block's bn1 -> ReLU and by its shortcut's BatchNorm — so this launch writes
 * those planes at half resolution and NO fp32 tensor:
 *     t      = AvgPool2d(2, 2)(y)                     (((y00 + y01) + y10) + y11) / 4, as ATen sums a window
 *     out_P1 = fmaf(t, a1[c], b1[c]) > 0              (the minus plane of a ReLU'd tensor is zero: not written)
 *     out_P2 = fmaf(t, a2[c], b2[c]) > 0,  out_M2 = ... < 0
 * pool_consts = [a1/4 | b1 | a2/4 | b2 | -a2/4 | -b2 | 0 | 0], `planes` floats each, 32-byte aligned (the four lanes of a
 * window each test one plane's bit as fmaf(window sum, a, b) > 0: the caller checks that a/4 is exact, i.e. that a is not
 * within two binades of the smallest normal).  C_in == planes, even H and W, the widths of
 * bnn_hip_hblock_pool_supported; the planes are [N, planes / 64, H / 2, W / 2].  Same bits as bnn_hip_hblock_forward +
 * bnn_hip_avgpool2_bn_pack2_f32.  */
int bnn_hip_hblock_pool_supported(const bnn_hip_hblock_desc* d);
int bnn_hip_hblock_pool_forward(const bnn_hip_hblock_desc* d, const uint64_t* in_P, const uint32_t* weights,
                                const float* consts, const float* pool_consts, const float* residual, uint64_t* out_P1,
                                uint64_t* out_P2, uint64_t* out_M2, void* stream);

/* The FIRST block of a stage with its shortcut convolution inside the launch (ABI 15; hierarchical_block.py:30-36: the
 * shortcut of a block that changes width is BatchNorm -> sign -> binary conv1x1 of the block's input).  Instead of a residual
 * tensor the launch takes the two sign planes of that binarisation (sc_P / sc_M: [N, C_in / 64, H, W], what
 * bnn_hip_hblock_pool_forward or bnn_hip_avgpool2_bn_pack2_f32 wrote), the 1 x 1 weights as [planes][C_in / 32] words
 * (bnn_hip_hblock_pack_shortcut_weights of the standard pack; no zero weights, no bias) and their alpha [planes], and
 * computes  shortcut = fmaf(alpha[c], dot, 0)  per pass — the integer and the one rounding of bnn_hip_bconv2d — so the
 * shortcut launch and its fp32 tensor disappear.  planes == 2 * C_in, C_in in {64, 128} — with
 * BNN_HIP_HBLOCK_CHANNEL_LANES (14 x 14 / 7 x 7 images, weights of bnn_hip_hblock_pack_weights_cl) C_in in {128, 256};
 * out_P is required (a next block in the stage); same bits as bnn_hip_bconv2d + bnn_hip_hblock_forward.  */
int bnn_hip_hblock_shortcut_supported(const bnn_hip_hblock_desc* d);
int bnn_hip_hblock_pack_shortcut_weights(int C_in, int planes, const uint32_t* wbits, uint32_t* weights, void* stream);
int bnn_hip_hblock_shortcut_forward(const bnn_hip_hblock_desc* d, const uint64_t* in_P, const uint32_t* weights,
                                    const float* consts, const uint64_t* sc_P, const uint64_t* sc_M,
                                    const uint32_t* sc_weights, const float* sc_alpha, float* out, uint64_t* out_P,
                                    void* stream);

/* fp32 NCHW in -> fp32 NCHW out.  ONE launch (bnn_hip_bconv2d_direct) wherever that path applies:
 * bnn_hip_conv_workspace_bytes(d) is then 0 and `workspace` may be NULL.  For the remaining geometries (see above)
 * it is pack_act + conv through `workspace` (bnn_hip_conv_workspace_bytes(d) bytes, 16-byte aligned).          */
size_t bnn_hip_conv_workspace_bytes(const bnn_hip_conv_desc* d);
int bnn_hip_bconv2d_f32(const bnn_hip_conv_desc* d, const float* x,
                        const uint32_t* wbits, const uint32_t* wnz,
                        const float* alpha, const float* bias, const float* post_scale,
                        float* out, void* workspace, void* stream);

/* XNORWeightBinarizer.forward under autograd (bnn/ops.py:129-140 with the STE of bnn/ops.py:68-73), value and backward
 * as one kernel each (torch: ~14 small kernels per layer and step).  w, what, dwhat, dw: fp32 [O, C, KH, KW].
 *   forward :  what = sign(Wc) * alpha[o],  Wc = w - mean over C (center),  alpha = mean |Wc| (compute_alpha) or 1;
 *              alpha (may be NULL) receives alpha[O] (fp64 sums in a fixed order; bnn_hip_pack_weight_f32's alpha to the
 *              rounding of that sum).
 *   backward:  dw from dwhat = dL/dwhat:  dWc = dwhat * alpha * 1[|Wc| < 1] + sign(Wc) * sum(dwhat * sign(Wc)) / (C KH KW),
 *              dw = dWc - mean over C of dWc when centred.  dwhat: `splits` >= 1 slabs [splits][O][C][KH][KW] that are
 *              added here in slab order (ABI 13: the split-K partial sums of bnn_hip_bconv_grad_weight_f32 go in as they
 *              are — no separate reduction pass); splits == 1: the gradient itself.                                    */
int bnn_hip_xnor_weight_forward_f32(const float* w, int O, int C, int KH, int KW, int center, int compute_alpha,
                                    float* what, float* alpha, void* stream);
int bnn_hip_xnor_weight_backward_f32(const float* w, const float* dwhat, int splits, int O, int C, int KH, int KW,
                                     int center, int compute_alpha, float* dw, void* stream);

/* ABI 14 — what bnn_hip_bconv_grad_input_f32 needs of the weights, straight from W in ONE launch: the fragments and alpha of
 * bnn_hip_grad_pack_weight_f32(What) for What = XNORWeightBinarizer(W) (bnn/ops.py:129-140) — the same bytes as
 * bnn_hip_xnor_weight_forward_f32 followed by bnn_hip_grad_pack_weight_f32 (three launches), without the fp32 What.
 * w: float32 [O,C,k,k], k = 3 or 1; packed: bnn_hip_grad_weight_pack_bytes(O, C, k) bytes, 16-byte aligned (written
 * completely: no clearing needed); alpha: float32 [O].                                                                  */
int bnn_hip_xnor_grad_pack_weight_f32(const float* w, int O, int C, int ksize, int center, int compute_alpha, void* packed,
                                      float* alpha, void* stream);

/* Training-mode BatchNorm2d fused with what follows it in the reference's residual blocks:
 *     y = relu?( batch_norm_train(x) (+ residual) )          bnn/models/layers/res_block.py:40-56, resnet.py:150-153
 * x, y, residual: fp32 [N, C, HW] (NCHW with HW = H * W).  forward: per-channel batch statistics (fp64 accumulation,
 * deterministic), y, save_mean / save_invstd [C] for the backward, and — when running_mean / running_var are given —
 * their momentum update (unbiased variance), exactly torch.nn.BatchNorm2d's training semantics to fp32 rounding.
 * backward: g = gy * 1[y > 0] when `y` is given (a fused ReLU; pass NULL otherwise); dgamma = sum g * xhat, dbeta = sum g,
 * dx = gamma * invstd * (g - dbeta / m - xhat * dgamma / m), and dres = g (the residual branch's gradient) when dres
 * is given.  gamma / beta may be NULL (1 / 0).  `workspace`: bnn_hip_bn_train_workspace_bytes(N, C, HW) bytes,
 * 8-byte aligned, not shared between concurrent calls.  Three launches each, no synchronisation.                     */
size_t bnn_hip_bn_train_workspace_bytes(int N, int C, int HW);
int bnn_hip_bn_train_forward_f32(const float* x, int N, int C, int HW, const float* gamma, const float* beta,
                                 const float* residual, int relu, float eps, float momentum, float* running_mean,
                                 float* running_var, float* y, float* save_mean, float* save_invstd, void* workspace,
                                 void* stream);
int bnn_hip_bn_train_backward_f32(const float* gy, const float* y, const float* x, const float* save_mean,
                                  const float* save_invstd, const float* gamma, int N, int C, int HW, float* dx,
                                  float* dres, float* dgamma, float* dbeta, void* workspace, void* stream);

/* The same backward with an addend:  dx = gamma * invstd * (g - dbeta / m - xhat * dgamma / m) + addend.  The backward
 * of y = x + f(batch_norm_train(x)) passes the skip's gradient (gy of the whole operation) as `addend`, fp32 [N, C, HW],
 * and needs no add pass of its own.  dgamma / dbeta: the bits of bnn_hip_bn_train_backward_f32.  addend == NULL: that
 * entry point itself (dres NULL), bit for bit.  No dres here.  Same workspace.                                       */
int bnn_hip_bn_train_backward_add_f32(const float* gy, const float* y, const float* x, const float* save_mean,
                                      const float* save_invstd, const float* gamma, const float* addend, int N, int C,
                                      int HW, float* dx, float* dgamma, float* dbeta, void* workspace, void* stream);

/* Training-mode BatchNorm2d in front of a binary convolution (the BATS cell operations, bnn/models/layers/bats_ops.py:
 * 78-173: BatchNorm2d -> binary Conv2d): the statistics and running-statistics update of bnn_hip_bn_train_forward_f32
 * (same kernels: save_mean, save_invstd and the running buffers get the same bits), then the three bit planes of
 * bnn_hip_bn_act_pack_ste_f32 with scale = gamma * invstd, shift = beta - mean * scale — the normalised tensor is never
 * written.  scale / shift: fp32 [C], outputs (what the planes were made with).  gamma / beta may be NULL.  Workspace:
 * bnn_hip_bn_train_workspace_bytes(N, C, H * W).  Three launches, no synchronisation.                                */
int bnn_hip_bn_train_pack_ste_f32(const float* x, int N, int C, int H, int W, const float* gamma, const float* beta,
                                  float eps, float momentum, float* running_mean, float* running_var, uint64_t* P,
                                  uint64_t* M, uint64_t* T, float* save_mean, float* save_invstd, float* scale, float* shift,
                                  void* workspace, void* stream);

/* Training-mode BatchNorm2d in front of the two 1x1 stride-2 convolutions of FactorizedReduce (bnn/models/layers/
 * bats_ops.py:190-209).  forward: the statistics and running-statistics update of bnn_hip_bn_train_pack_ste_f32 (same
 * launchers: save_mean, save_invstd and the running buffers get the same bits — the statistics are over ALL of x), then the
 * planes of bnn_hip_bn_act_pack_ste_s2_f32 with the scale / shift it returns.  Workspace: bnn_hip_bn_train_workspace_bytes(
 * N, C, H * W).  Three launches.
 * backward: the gradient with respect to u arrives on the lattices only — g0[n, c, i, j] at pixel (2i, 2j), g1 at
 * (2i+1, 2j+1), fp32 [N, C, H/2, W/2] each — and is zero elsewhere: dbeta = sum g, dgamma = sum g * xhat over the
 * lattice pixels, dx = gamma * invstd * (g - dbeta / m - xhat * dgamma / m) at EVERY pixel of [N, C, H, W], m = N * H * W.
 * x is read for the sums at the lattice pixels only; dx is written exactly once per element (no clearing pass).  Sums in
 * double through per-(channel, image split) partials added in a fixed order: no atomics, the same bits on every run.
 * x, dx: 8-byte aligned (rows are moved as float2, or float4 where W % 4 == 0 and they are 16-byte aligned); gamma,
 * dgamma, dbeta may be NULL.  H and W even.  Same workspace.  Three launches, no synchronisation.                      */
int bnn_hip_bn_train_pack_ste_s2_f32(const float* x, int N, int C, int H, int W, const float* gamma, const float* beta,
                                     float eps, float momentum, float* running_mean, float* running_var, uint64_t* P,
                                     uint64_t* M, uint64_t* T, float* save_mean, float* save_invstd, float* scale,
                                     float* shift, void* workspace, void* stream);
int bnn_hip_bn_train_backward_s2_f32(const float* g0, const float* g1, const float* x, const float* save_mean,
                                     const float* save_invstd, const float* gamma, int N, int C, int H, int W, float* dx,
                                     float* dgamma, float* dbeta, void* workspace, void* stream);

/* Backward of  y = channel_shuffle(PReLU(z), shuffle_groups)  (the tail of a BATS cell operation; the forward is the
 * epilogue of bnn_hip_bconv2d_grouped_fused / bnn_hip_bconv2d_fused).  gy: fp32 [N, O, HW] in the OUTPUT's (shuffled)
 * channel order; z, gz: fp32 [N, O, HW] in the convolution's order; slope: slope_count (1 or O) floats:
 *     gz[n,o,:] = z > 0 ? g : slope[o] * g      g = gy[n, (o % (O / sg)) * sg + o / (O / sg), :]     (z == +-0: slope branch)
 *     dslope[o] = sum over n, pixels with !(z > 0) of g * z          (slope_count == 1: one value, summed over o as well)
 * torch.nn.PReLU's convention.  The sums are accumulated in double through per-(channel, image split) partials added in a
 * fixed order: no atomics, the same bits on every run.  gz may be z (in place), not gy.  workspace:
 * bnn_hip_prelu_shuffle_backward_workspace_bytes(N, O, HW) bytes, 8-byte aligned.  Two launches.                      */
size_t bnn_hip_prelu_shuffle_backward_workspace_bytes(int N, int O, int HW);
int bnn_hip_prelu_shuffle_backward_f32(const float* gy, const float* z, const float* slope, int slope_count, int N, int O,
                                       int HW, int shuffle_groups, float* gz, float* dslope, void* workspace,
                                       size_t workspace_bytes, void* stream);

/* Eval-mode BatchNorm2d with folded constants, fused with what follows it in the reference's residual blocks:
 *     y = relu?( fmaf(x, scale[c], shift[c]) (+ residual) )     bnn/models/layers/res_block.py:40-56 under .eval()
 * x, y, residual: fp32 [N, C, HW]; scale, shift: fp32 [C] (scale = weight / sqrt(running_var + eps), shift = bias -
 * running_mean * scale, rounded as the caller wishes — the host side rounds them as ATen's CPU kernel does).  The same
 * float operations in the same order as the BN / residual / ReLU epilogue of bnn_hip_bconv2d_fused, so a network run
 * layer by layer and the fused executor agree bit for bit.  ReLU keeps NaN (torch.relu).  One launch.  y must not
 * alias x or residual.  (ABI 13)                                                                                      */
int bnn_hip_bn_act_f32(const float* x, int N, int C, int HW, const float* scale, const float* shift, const float* residual,
                       int relu, float* y, void* stream);

/* The stem tail in training mode:  maxpool3x3/2/1( relu( batch_norm_train(x) ) )   (bnn/models/resnet.py:150-153) without
 * ever writing the normalised tensor: `pooled` [N, C, Hp, Wp] (Hp = (H - 1) / 2 + 1) and ONE BYTE per pooled output,
 * `code` = 3 * dy + dx of the winning window position, are all the forward leaves behind (the library: the fp32
 * BatchNorm output, the ReLU output and int64 pooling indices).  The backward routes gy through the codes inside the
 * BatchNorm reductions (a winner of value 0 passes nothing: ReLU).  Workspace: bnn_hip_bn_train_workspace_bytes(N, C,
 * H * W).  Same statistics semantics as bnn_hip_bn_train_forward_f32.                                                   */
int bnn_hip_bn_relu_maxpool_train_forward_f32(const float* x, int N, int C, int H, int W, const float* gamma,
                                              const float* beta, float eps, float momentum, float* running_mean,
                                              float* running_var, float* pooled, uint8_t* code, float* save_mean,
                                              float* save_invstd, void* workspace, void* stream);
int bnn_hip_bn_relu_maxpool_train_backward_f32(const float* gy, const float* pooled, const uint8_t* code, const float* x,
                                               const float* save_mean, const float* save_invstd, const float* gamma,
                                               int N, int C, int H, int W, float* dx, float* dgamma, float* dbeta,
                                               void* workspace, void* stream);

/* Roofline calibration: runs a register-only instruction stream on every CU at full
 * occupancy and reports the sustained 32-bit lane-ops/s.  mode: 0 = v_bitop3_b32 +
 * v_bcnt_u32_b32 (the hot loop's pair), 1 = v_xor_b32 + v_bcnt_u32_b32, 2 = bcnt only,
 * 3 = bitop3 only, 4 = xor only, 5 = v_fma_f32 only, 6 = v_add_u32 only, 7 = v_and_b32 with
 * VGPR-only operands, 8 = that + bcnt, 9 = v_xor_b32 VGPR-only, 10 = v_and_b32 (scalar operand) + bcnt.
 * Synchronous (hipEvents on `stream`, temporary hipMalloc); not part of the inference path. */
int bnn_hip_probe_int_alu(int mode, int iters, double* lane_ops_per_s, double* elapsed_ms,
                          void* stream);

/* The engine (shader) clock at this moment, MHz: one wave reads the shader-clock counter (s_memtime) and the
 * constant-rate counter (s_memrealtime) around `spin_iters` dependent ALU steps (10000 ~ 20 us).  Issued on `stream`
 * right behind a timed region it reports the clock those kernels ran at (DVFS moves on a millisecond scale) — the
 * figure bench.py prints next to every sustained number.  Synchronous; not part of the inference path.            */
int bnn_hip_probe_clock(int spin_iters, double* shader_mhz, double* elapsed_us, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BNN_HIP_H_ */

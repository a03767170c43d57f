// capi_fuzz.hip — argument fuzz of the C-ABI's validators (csrc/capi.hip) under AddressSanitizer + UBSan, HOST ONLY.
//
// Built by `make -C binary-networks-pytorch_amd/csrc fuzz` (hipcc --cuda-host-only -fsanitize=address,undefined): capi.hip
// is compiled as it is, the kernels' launchers (bnn::launch_*) are replaced by the stubs below, which never touch a
// pointer and instead CHECK what the kernels rely on — the contract capi.hip has to enforce before it launches:
//   * every tensor of a conv launch below 2^30 fp32 elements / 2^29 plane words, stem and one-launch-layer tensors
//     below the 32-bit buffer-descriptor limit, alignments, consistent weight layout, positive geometry.
// The driver throws edge-value integers and null / misaligned / plausible pointers at every entry point: no call may
// crash, overflow a signed integer, read out of bounds, or reach a launcher with arguments that break the contract.
// Test infrastructure (tests/test_native_cpu.py runs it); nothing here ships in libbnn_hip.so.
#include <cinttypes>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../binary-networks-pytorch_amd/csrc/bnn_dev.h"

namespace {
unsigned long long g_reached = 0, g_calls = 0;
uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint64_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }

[[noreturn]] void broken(const char* what) {
  std::fprintf(stderr, "CONTRACT BROKEN: %s\n", what);
  std::abort();
}
#define REQUIRE(c) do { if (!(c)) broken(#c); } while (0)
bool al(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
constexpr long long kConvElems = (1LL << 30) - 1, kPlaneWords = (1LL << 29) - 1, kDesc = 0xFFFFFE00LL;
}  // namespace

namespace bnn {
int choose_cwc(int cw32, int KH, int KW) {  // same rule as csrc/bconv.hip
  if (KH == 3 && KW == 3) return (cw32 % 4 == 0) ? 4 : 2;
  if (KH == 1 && KW == 1) return cw32 % 16 == 0 ? 16 : cw32 % 8 == 0 ? 8 : cw32 % 4 == 0 ? 4 : 2;
  return 2;
}
static void check_convp(const ConvP& p) {
  REQUIRE(p.N > 0 && p.C > 0 && p.H > 0 && p.Wd > 0 && p.O > 0 && p.KH > 0 && p.KW > 0 && p.Ho > 0 && p.Wo > 0);
  REQUIRE(p.sh > 0 && p.sw > 0 && p.ph >= 0 && p.pw >= 0 && p.dh > 0 && p.dw > 0);
  REQUIRE(p.cw32 == 2 * ((p.C + 63) / 64) && p.cwc > 0 && p.cwc * p.nchunk == p.cw32);
  REQUIRE((long long)p.N * p.Ho * p.Wo == p.npix);
  const long long ctot = p.c_tot > 0 ? p.c_tot : p.O;
  REQUIRE(p.c_off >= 0 && p.c_off + p.O <= ctot);
  REQUIRE((long long)p.N * ctot * p.Ho * p.Wo <= kConvElems);
  REQUIRE((long long)p.N * p.Ho * p.Wo * ((p.O + 63) / 64) <= kPlaneWords);
}
int launch_bconv(const ConvP& p, int flags, hipStream_t, bnn_hip_conv_route* route, bool dry) {
  ++g_reached;
  REQUIRE(dry == (route != nullptr));  // the entry points launch without a route; the queries ask for one and launch nothing
  if (route) { std::memset(route, 0, sizeof(*route)); route->site = BNN_HIP_ROUTE_SITES - 1; route->waves = 1; }
  check_convp(p);
  REQUIRE((long long)p.N * p.H * p.Wd * ((p.C + 63) / 64) <= kPlaneWords);
  REQUIRE(p.P && p.M && p.W && al(p.P, 16) && al(p.M, 16) && al(p.W, 16));
  REQUIRE(p.out || (p.outP && p.outM));
  REQUIRE(p.raw || p.alpha);
  REQUIRE((p.bn_a == nullptr) == (p.bn_b == nullptr) && (p.outP == nullptr) == (p.outM == nullptr));
  REQUIRE((p.pack_a == nullptr) == (p.pack_b == nullptr));
  REQUIRE(!(flags & BNN_HIP_FLAG_WEIGHT_ZEROS) || p.Z);
  REQUIRE(!p.outP || (al(p.outP, 8) && al(p.outM, 8)));
  REQUIRE(!p.ds_P || (p.ds_W && p.ds_alpha && p.ds_a && p.ds_b && !p.res && p.ds_C > 0 && al(p.ds_P, 8) && al(p.ds_W, 16)));
  return BNN_HIP_OK;
}
bool ds_fold_applies(const ConvP& p, int flags) { return p.KH == 3 && p.KW == 3 && (flags & BNN_HIP_FLAG_ACT_NONNEG); }
// the int8 matrix-core convolution (csrc/bconv_mfma.hip)
size_t weight_i8_bytes(int O, int C, int KH, int KW) {
  return (O > 0 && C > 0 && KH == 3 && KW == 3 && O % 64 == 0 && C % 64 == 0) ? (size_t)O * (size_t)C * 9 : 0;
}
int launch_pack_weight_i8(const uint32_t* wbits, const uint32_t* wnz, const bnn_hip_wlayout& L, int O, void* w8, hipStream_t) {
  ++g_reached;
  REQUIRE(wbits && wnz && w8 && al(wbits, 16) && al(wnz, 16) && al(w8, 16));
  REQUIRE(O > 0 && O % 64 == 0 && L.taps == 9 && L.cw32 > 0 && L.cw32 % 2 == 0 && L.cwc * L.nchunk == L.cw32 && L.o_pad == O);
  return BNN_HIP_OK;
}
bool mfma_conv_applies(const ConvP& p, int) {
  check_convp(p);
  return p.KH == 3 && p.KW == 3 && p.C % 64 == 0 && p.O % 64 == 0 && !p.ds_P && !p.prelu && p.c_tot == p.O;
}
size_t weight_f4_bytes(int O, int C, int KH, int KW) {
  return (weight_i8_bytes(O, C, KH, KW) != 0 && C % 128 == 0) ? (size_t)O * (size_t)C * 9 / 2 : 0;
}
int launch_pack_weight_f4(const uint32_t* wbits, const uint32_t* wnz, const bnn_hip_wlayout& L, int O, void* w4, hipStream_t) {
  ++g_reached;
  REQUIRE(wbits && wnz && w4 && al(wbits, 16) && al(wnz, 16) && al(w4, 16));
  REQUIRE(O > 0 && O % 64 == 0 && (L.taps == 9 || L.taps == 1) && L.cw32 > 0 && L.cw32 % 4 == 0 && L.cwc * L.nchunk == L.cw32 && L.o_pad == O);
  return BNN_HIP_OK;
}
bool mfma4_conv_applies(const ConvP& p, int flags) { return p.C % 128 == 0 && mfma_conv_applies(p, flags); }
int launch_bconv_mfma(const ConvP& p, int flags, const void* w8, hipStream_t, bool f4) {
  ++g_reached;
  check_convp(p);
  REQUIRE(f4 ? mfma4_conv_applies(p, flags) : mfma_conv_applies(p, flags));
  REQUIRE((long long)p.N * p.H * p.Wd * ((p.C + 63) / 64) <= kPlaneWords);
  REQUIRE(p.P && p.M && w8 && al(p.P, 16) && al(p.M, 16) && al(w8, 16) && p.alpha);
  REQUIRE(p.out || (p.outP && p.outM));
  REQUIRE((p.bn_a == nullptr) == (p.bn_b == nullptr) && (p.outP == nullptr) == (p.outM == nullptr));
  REQUIRE(!p.outP || (al(p.outP, 8) && al(p.outM, 8)));
  REQUIRE(!p.out || al(p.out, 4));
  return BNN_HIP_OK;
}
// the 1x1 convolution on the FP4 matrix cores (csrc/bconv1x1_mfma.hip)
size_t weight1x1_f4_bytes(int O, int C) { return (O > 0 && C > 0 && O % 64 == 0 && C % 128 == 0) ? (size_t)O * (size_t)C / 2 : 0; }
bool mfma1x1_applies(const ConvP& p, int flags) {
  check_convp(p);
  return p.KH == 1 && p.KW == 1 && p.sh == 1 && p.sw == 1 && p.ph == 0 && p.pw == 0 && p.dh == 1 && p.dw == 1 &&
         weight1x1_f4_bytes(p.O, p.C) != 0 && !p.ds_P && p.c_off == 0 && p.c_tot == p.O &&
         !(flags & BNN_HIP_FLAG_FORCE_GENERIC);
}
int launch_bconv1x1_mfma(const ConvP& p, int flags, const void* w4, hipStream_t) {
  ++g_reached;
  check_convp(p);
  REQUIRE(mfma1x1_applies(p, flags));
  REQUIRE((long long)p.N * p.H * p.Wd * ((p.C + 63) / 64) <= kPlaneWords);
  REQUIRE(p.P && p.M && w4 && al(p.P, 16) && al(p.M, 16) && al(w4, 16) && p.alpha);
  REQUIRE(p.out || (p.outP && p.outM));
  REQUIRE((p.bn_a == nullptr) == (p.bn_b == nullptr) && (p.outP == nullptr) == (p.outM == nullptr));
  REQUIRE((p.pack_a == nullptr) == (p.pack_b == nullptr));
  REQUIRE(!p.outP || (al(p.outP, 8) && al(p.outM, 8)));
  REQUIRE(!p.out || al(p.out, 4));
  return BNN_HIP_OK;
}
// the same with the shortcut convolution folded in
size_t shortcut_weight_i8_bytes(int O, int C) {
  return (O > 0 && O % 64 == 0 && (C == 64 || C == 128 || C == 256)) ? (size_t)O * (size_t)C : 0;
}
int launch_pack_shortcut_weight_i8(const uint32_t* wbits, int O, int C, void* w8, hipStream_t) {
  ++g_reached;
  REQUIRE(wbits && w8 && al(wbits, 16) && al(w8, 16) && shortcut_weight_i8_bytes(O, C) != 0);
  return BNN_HIP_OK;
}
bool mfma_fold_applies(const ConvP& p, int flags) {
  check_convp(p);
  return p.KH == 3 && p.KW == 3 && p.C % 64 == 0 && p.O % 64 == 0 && p.ds_P && !p.res && !p.prelu && p.c_tot == p.O &&
         (flags & BNN_HIP_FLAG_ACT_NONNEG) && shortcut_weight_i8_bytes(p.O, p.ds_C) != 0;
}
bool mfma4_fold_applies(const ConvP& p, int flags) { return p.C % 128 == 0 && mfma_fold_applies(p, flags); }
int launch_bconv_mfma_fold(const ConvP& p, int flags, const void* w8, const void* sc_w8, hipStream_t, bool f4) {
  ++g_reached;
  check_convp(p);
  REQUIRE(f4 ? mfma4_fold_applies(p, flags) : mfma_fold_applies(p, flags));
  REQUIRE((long long)p.N * p.H * p.Wd * ((p.C + 63) / 64) <= kPlaneWords);
  REQUIRE(p.P && p.M && w8 && sc_w8 && al(p.P, 16) && al(p.M, 16) && al(w8, 16) && al(sc_w8, 16) && p.alpha);
  REQUIRE(p.ds_P && al(p.ds_P, 8) && p.ds_alpha && p.ds_a && p.ds_b);
  REQUIRE(p.ds_inW == 0 || ((p.ds_inH + 1) / 2 == p.Ho && (p.ds_inW + 1) / 2 == p.Wo));
  REQUIRE(!p.outP || (al(p.outP, 8) && al(p.outM, 8)));
  REQUIRE(!p.out || al(p.out, 4));
  return BNN_HIP_OK;
}
bool fly_supported(const ConvP& p) { return p.KH * p.KW <= 49; }
int fly_default_plan(const ConvP& p, int, bnn_hip_fly_plan* plan) {
  check_convp(p);
  std::memset(plan, 0, sizeof(*plan));
  return fly_supported(p) ? BNN_HIP_OK : BNN_HIP_ERR_UNSUPPORTED;
}
int launch_bconv_fly(const ConvP& p, const void* x, int dtype, int flags, const bnn_hip_fly_plan*, hipStream_t) {
  ++g_reached;
  check_convp(p);
  REQUIRE(dtype == BNN_HIP_DTYPE_F32 || dtype == BNN_HIP_DTYPE_F16 || dtype == BNN_HIP_DTYPE_BF16);
  const bool half = dtype != BNN_HIP_DTYPE_F32;
  REQUIRE(p.out16 == 0 || p.out16 == BNN_HIP_DTYPE_F16 || p.out16 == BNN_HIP_DTYPE_BF16);
  REQUIRE(x && p.W && p.alpha && p.out && al(x, half ? 2 : 4) && al(p.W, 16) && al(p.out, p.out16 ? 2 : 4));
  REQUIRE((long long)p.N * p.C * p.H * p.Wd * (half ? 2 : 4) <= kDesc);
  REQUIRE(!(flags & (BNN_HIP_FLAG_OUT_F16 | BNN_HIP_FLAG_OUT_BF16)));   // (they travel as p.out16)
  REQUIRE(!(flags & BNN_HIP_FLAG_WEIGHT_ZEROS) || p.Z);
  return BNN_HIP_OK;
}
static void check_planes(const void* x, int N, int C, int H, int W, const void* P, const void* M, int xal) {
  REQUIRE(x && P && M && N > 0 && C > 0 && H > 0 && W > 0 && al(x, xal) && al(P, 8) && al(M, 8));
  REQUIRE((long long)N * H * W <= (1LL << 31) - 1 && (C + 63) / 64 <= 65535);
}
int launch_pack_act(const float* x, int N, int C, int H, int W, uint64_t* P, uint64_t* M, hipStream_t) {
  ++g_reached; check_planes(x, N, C, H, W, P, M, 4); return BNN_HIP_OK;
}
int launch_pack_act_f16(const void* x, int N, int C, int H, int W, uint64_t* P, uint64_t* M, hipStream_t) {
  ++g_reached; check_planes(x, N, C, H, W, P, M, 2); return BNN_HIP_OK;
}
int launch_pack_act_bf16(const void* x, int N, int C, int H, int W, uint64_t* P, uint64_t* M, hipStream_t) {
  ++g_reached; check_planes(x, N, C, H, W, P, M, 2); return BNN_HIP_OK;
}
int launch_bn_act_pack(const float* x, int N, int C, int H, int W, const float* a, const float* b, int, uint64_t* P,
                       uint64_t* M, hipStream_t) {
  ++g_reached; check_planes(x, N, C, H, W, P, M, 4); REQUIRE((a == nullptr) == (b == nullptr)); return BNN_HIP_OK;
}
static void check_view_planes(const float* x, int c_off, int c_tot, int N, int C, int H, int W, const void* P, const void* M) {
  check_planes(x, N, C, H, W, P, M, 4);
  REQUIRE(c_off >= 0 && c_tot > 0 && (long long)c_off + C <= c_tot);
}
int launch_bn_act_pack_multi(const float* x, int c_off, int c_tot, int N, int C, int H, int W, int K, const float* a,
                             const float* b, int, uint64_t* P, uint64_t* M, hipStream_t) {
  ++g_reached; check_view_planes(x, c_off, c_tot, N, C, H, W, P, M); REQUIRE(K >= 1 && K <= 4 && a && b); return BNN_HIP_OK;
}
int launch_bn_act_pack_s2(const float* x, int c_off, int c_tot, int N, int C, int H, int W, const float* a, const float* b, int,
                          uint64_t* P, uint64_t* M, hipStream_t) {
  ++g_reached; check_view_planes(x, c_off, c_tot, N, C, H, W, P, M);
  REQUIRE(H % 2 == 0 && W % 2 == 0 && (a == nullptr) == (b == nullptr)); return BNN_HIP_OK;
}
int launch_stem3x3_bn_relu_pack(const float* x, const float* w, const float* s, const float* t, const float* a, const float* b,
                                int N, int O, int H, int W, int K, uint64_t* P, uint64_t* M, float* y, hipStream_t) {
  ++g_reached; check_planes(x, N, O, H, W, P, M, 4);
  REQUIRE(w && s && t && a && b && K >= 1 && K <= 4 && (!y || al(y, 4)));
  REQUIRE((long long)N * O * H * W <= (1LL << 31) - 1 && 3LL * N * H * W <= (1LL << 31) - 1);
  return BNN_HIP_OK;
}
// csrc/bats_stem_in.hip: the groups divide the channels, a group's input channels fit the LDS tile, the groups / plane
// words fit grid.y, every tensor stays below 2^31 elements, and the planes exist exactly when K >= 1
int launch_stem_s2x2(const float* x, const float* w1, const float* s1, const float* t1, const float* w2, const float* s2,
                     const float* t2, int N, int C1, int C, int G, int H, int W, int relu_out, float* y, hipStream_t) {
  ++g_reached;
  REQUIRE(x && w1 && s1 && t1 && w2 && s2 && t2 && y && al(x, 4) && al(w1, 4) && al(w2, 4) && al(y, 4));
  REQUIRE(N > 0 && C1 > 0 && C > 0 && G > 0 && H > 0 && W > 0 && C1 % G == 0 && C % G == 0 && (relu_out == 0 || relu_out == 1));
  REQUIRE(C1 / G <= BNN_HIP_STEM_S2X2_MAX_GROUP_CHANNELS && G <= 65535);
  const long long H2 = ((long long)H + 3) / 4, W2 = ((long long)W + 3) / 4;      // ceil(ceil(H / 2) / 2)
  REQUIRE(3LL * N * H * W <= (1LL << 31) - 1 && (long long)N * C * H2 * W2 <= (1LL << 31) - 1);
  return BNN_HIP_OK;
}
int launch_gconv3x3s2_bn_pack(const float* x, const float* w, const float* s, const float* t, const float* a, const float* b,
                              int N, int C, int O, int G, int H, int W, int relu_in, int K, uint64_t* P, uint64_t* M, float* y,
                              hipStream_t) {
  ++g_reached;
  REQUIRE(x && w && s && t && al(x, 4) && al(w, 4) && (!y || al(y, 4)) && K >= 0 && K <= 4 && (relu_in == 0 || relu_in == 1));
  REQUIRE(K == 0 ? (y && !a && !b && !P && !M) : (a && b && P && M && al(P, 8) && al(M, 8)));
  REQUIRE(N > 0 && C > 0 && O > 0 && G > 0 && H > 0 && W > 0 && C % G == 0 && O % G == 0);
  REQUIRE(C / G <= BNN_HIP_GCONV3X3S2_MAX_GROUP_CHANNELS && (O + 63) / 64 <= 65535);
  const long long Ho = ((long long)H + 1) / 2, Wo = ((long long)W + 1) / 2;
  REQUIRE((long long)N * C * H * W <= (1LL << 31) - 1 && (long long)N * O * Ho * Wo <= (1LL << 31) - 1);
  return BNN_HIP_OK;
}
int launch_avgpool_pack(const float* x, int N, int C, int H, int W, int k, uint64_t* P, uint64_t* M, hipStream_t) {
  ++g_reached; REQUIRE(x && P && M && N > 0 && C > 0 && H > 0 && W > 0 && k > 0 && al(P, 8) && al(M, 8)); return BNN_HIP_OK;
}
int launch_avgpool2_bn_pack2(const float* x, int N, int C, int H, int W, const float* a1, const float* b1, int, uint64_t* P1,
                             uint64_t* M1, const float* a2, const float* b2, int, uint64_t* P2, uint64_t* M2, float* out,
                             hipStream_t) {
  ++g_reached;
  REQUIRE(x && a1 && b1 && P1 && M1 && N > 0 && C > 0 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0 && al(x, 8));
  REQUIRE((a2 == nullptr) == (b2 == nullptr) && (!a2 || (P2 && M2 && al(P2, 8) && al(M2, 8))) && al(P1, 8) && al(M1, 8));
  REQUIRE((long long)N * C * H * W <= (1LL << 31) - 1 && (!out || al(out, 4)));
  return BNN_HIP_OK;
}
// csrc/hblock.hip: the shape rule and the launch contract of the one-launch hierarchical block
static bool stub_hb_shape(int C_in, int planes) {
  if (C_in <= 0 || C_in > (1 << 20) || planes < 64 || planes % 64 || planes > 4096) return false;
  const int cin[3] = {C_in, planes / 2, planes / 4};
  for (int k = 0; k < 3; ++k) {
    const int cw = (cin[k] + 31) / 32;
    if (cw == 3 || (cw > 4 && cw % 4)) return false;
  }
  const int cw0 = (C_in + 31) / 32;
  return cw0 == 1 ? C_in <= 32 : cw0 % 2 == 0;
}
bool hblock_supported(const bnn_hip_hblock_desc* d) {
  REQUIRE(d && d->N > 0 && d->C_in > 0 && d->H > 0 && d->W > 0 && d->planes > 0 && d->waves >= 0 && d->waves <= 16);
  REQUIRE((long long)d->N * d->planes < (1LL << 23) && (long long)d->H * d->W < (1LL << 23));
  return stub_hb_shape(d->C_in, d->planes) && (long long)(d->H + 6) * (d->W + 2) * ((d->C_in + 31) / 32) * 4 < 160 * 1024;
}
int hblock_layout(int C_in, int planes, bnn_hip_hblock_layout* L) {
  REQUIRE(L && C_in > 0 && planes > 0);
  if (!stub_hb_shape(C_in, planes)) return BNN_HIP_ERR_UNSUPPORTED;
  L->weight_words = 9LL * ((C_in + 31) / 32) * (planes / 2) + 9LL * ((planes / 2 + 31) / 32) * (planes / 4) +
                    9LL * ((planes / 4 + 31) / 32) * (planes / 4);
  L->const_floats = 4LL * planes;
  return BNN_HIP_OK;
}
bool hblock_cl_ds_supported(const bnn_hip_hblock_desc* d) {
  return d->planes == 2 * d->C_in && (d->C_in == 128 || d->C_in == 256) && d->H == d->W && (d->H == 7 || d->H == 14);
}
int launch_hblock_cl_ds(const bnn_hip_hblock_desc* d, const uint64_t* inP, const uint32_t* W, const float* Kc, const uint64_t* p,
                        const uint64_t* m, const uint32_t* w, const float* a, float* out, uint64_t* outP, hipStream_t) {
  ++g_reached;
  REQUIRE(d && inP && W && Kc && p && m && w && a && out && outP && al(w, 32) && al(a, 32) && al(outP, 8) && al(Kc, 32));
  REQUIRE(d->N > 0 && d->planes == 2 * d->C_in && d->H == d->W && (d->W != 14 || al(out, 8)));
  return BNN_HIP_OK;
}
bool hblock_ds_supported(const bnn_hip_hblock_desc* d) {
  return d->planes == 2 * d->C_in && (d->C_in == 64 || d->C_in == 128) && (long long)d->H * d->W <= 4096;
}
int launch_hblock_ds(const bnn_hip_hblock_desc* d, const uint64_t* inP, const uint32_t* W, const float* Kc, const uint64_t* p,
                     const uint64_t* m, const uint32_t* w, const float* a, float* out, uint64_t* outP, hipStream_t) {
  ++g_reached;
  REQUIRE(d && inP && W && Kc && p && m && w && a && out && outP && al(w, 32) && al(a, 32) && al(outP, 8) && al(p, 8) && al(m, 8) &&
          al(Kc, 32));
  REQUIRE(d->N > 0 && d->H > 0 && d->W > 0 && d->planes == 2 * d->C_in);
  return BNN_HIP_OK;
}
int launch_hblock_ds_pack_weights(int C_in, int planes, const uint32_t* w, uint32_t* dst, hipStream_t) {
  ++g_reached;
  REQUIRE(w && dst && C_in > 0 && planes > 0 && al(dst, 32));
  return (C_in % 64 || C_in > 4096 || planes > 4096) ? BNN_HIP_ERR_UNSUPPORTED : BNN_HIP_OK;
}
bool hblock_pool_supported(const bnn_hip_hblock_desc* d) {
  return d->C_in == d->planes && (d->planes == 64 || d->planes == 128 || d->planes == 256) && d->H % 2 == 0 && d->W % 2 == 0 &&
         d->rows_per_band % 2 == 0 && (long long)d->H * d->W <= 4096;
}
int launch_hblock_pool(const bnn_hip_hblock_desc* d, const uint64_t* inP, const uint32_t* W, const float* Kc, const float* Kp,
                       const float* res, uint64_t* o1, uint64_t* o2, uint64_t* o3, hipStream_t) {
  ++g_reached;
  REQUIRE(d && inP && W && Kc && Kp && res && o1 && o2 && o3 && al(Kc, 32) && al(Kp, 32) && al(o1, 8) && al(o2, 8) && al(o3, 8));
  REQUIRE(d->N > 0 && d->H > 0 && d->W > 0 && d->H % 2 == 0 && d->W % 2 == 0 && d->C_in == d->planes);
  return BNN_HIP_OK;
}
int launch_hblock_pack_weights(int C_in, int planes, const uint32_t* const w[3], uint32_t* dst, hipStream_t) {
  ++g_reached; REQUIRE(C_in > 0 && planes > 0 && w[0] && w[1] && w[2] && dst && al(dst, 64));
  return stub_hb_shape(C_in, planes) ? BNN_HIP_OK : BNN_HIP_ERR_UNSUPPORTED;
}
int launch_hblock(const bnn_hip_hblock_desc* d, const uint64_t* inP, const uint32_t* W, const float* Kc, const float* res,
                  float* out, uint64_t* outP, hipStream_t) {
  ++g_reached;
  REQUIRE(d && inP && W && Kc && res && out && res != out && al(inP, 8) && al(W, 64) && al(Kc, 32) && (!outP || al(outP, 8)));
  REQUIRE(stub_hb_shape(d->C_in, d->planes) && (long long)d->N * d->planes * d->H * d->W <= kConvElems);
  REQUIRE((long long)d->N * ((d->C_in + 63) / 64) * d->H * d->W <= kPlaneWords);
  return BNN_HIP_OK;
}
bool hblock_cl_supported(const bnn_hip_hblock_desc* d) {
  REQUIRE(d && d->N > 0 && d->C_in > 0 && d->planes > 0);
  return stub_hb_shape(d->C_in, d->planes) && d->planes % 256 == 0 && d->C_in % 64 == 0 && d->H == d->W && (d->H == 7 || d->H == 14);
}
int launch_hblock_cl_pack_weights(int C_in, int planes, const uint32_t* const w[3], uint32_t* dst, hipStream_t) {
  ++g_reached; REQUIRE(C_in > 0 && planes > 0 && w[0] && w[1] && w[2] && dst && al(dst, 64));
  return stub_hb_shape(C_in, planes) && planes % 256 == 0 ? BNN_HIP_OK : BNN_HIP_ERR_UNSUPPORTED;
}
int launch_hblock_cl(const bnn_hip_hblock_desc* d, const uint64_t* inP, const uint32_t* W, const float* Kc, const float* res,
                     float* out, uint64_t* outP, hipStream_t) {
  ++g_reached;
  REQUIRE(d && inP && W && Kc && res && out && res != out && al(inP, 8) && al(W, 64) && al(Kc, 32) && (!outP || al(outP, 8)));
  REQUIRE(d->planes % 256 == 0 && d->H == d->W && (d->H == 7 || d->H == 14) && (d->W != 14 || (al(res, 8) && al(out, 8))));
  return BNN_HIP_OK;
}
int launch_orpool_packed(const uint64_t* P, int N, int C, int H, int W, int k, uint64_t* oP, uint64_t* oM, hipStream_t) {
  ++g_reached; REQUIRE(P && oP && oM && N > 0 && C > 0 && H > 0 && W > 0 && k > 0 && al(P, 8) && al(oP, 8) && al(oM, 8));
  return BNN_HIP_OK;
}
int launch_bn_relu_maxpool_pack(const float* x, int N, int C, int H, int W, const float* a, const float* b, int, int k,
                                int stride, int pad, float* out, uint64_t* P, uint64_t* M, hipStream_t) {
  ++g_reached;
  REQUIRE(x && N > 0 && C > 0 && H > 0 && W > 0 && k > 0 && stride > 0 && pad >= 0 && (out || P));
  REQUIRE((P == nullptr) == (M == nullptr) && (a == nullptr) == (b == nullptr) && 2 * pad <= k);
  return BNN_HIP_OK;
}
int launch_stem(const float* x, const float* w, const float* a, const float* b, int N, int H, int W, int flags, float* out,
                uint64_t* P, uint64_t* M, hipStream_t) {
  ++g_reached;
  REQUIRE(x && w && a && b && N > 0 && H > 0 && W > 0 && (out || P) && (P == nullptr) == (M == nullptr));
  REQUIRE(!(flags & ~(BNN_HIP_STEM_EXACT_FP32 | BNN_HIP_STEM_FP16)));
  const long long hc = (H - 1) / 2 + 1, wc = (W - 1) / 2 + 1, hp = (hc - 1) / 2 + 1, wp = (wc - 1) / 2 + 1;
  REQUIRE((long long)N * 3 * H * W * 4 <= kDesc && (long long)N * 64 * hp * wp * 4 <= kDesc);
  REQUIRE(!P || (al(P, 8) && al(M, 8)));
  return BNN_HIP_OK;
}
int launch_stem_rows_aff(const float* x, const float* w, const float* a, const float* b, const float* pa, const float* pb,
                         int N, int H, int W, int, float*, uint64_t* P, uint64_t* M, hipStream_t) {
  ++g_reached;
  REQUIRE(x && w && a && b && pa && pb && P && M && N > 0 && H > 0 && W > 0 && al(P, 8) && al(M, 8));
  const long long hc = (H - 1) / 2 + 1, wc = (W - 1) / 2 + 1, hp = (hc - 1) / 2 + 1, wp = (wc - 1) / 2 + 1;
  REQUIRE((long long)N * 3 * H * W * 4 <= kDesc && (long long)N * 64 * hp * wp * 4 <= kDesc);
  return BNN_HIP_OK;
}
int launch_stem_conv(const float* x, const float* w, int N, int H, int W, int, float* out, hipStream_t) {
  ++g_reached;
  REQUIRE(x && w && out && N > 0 && H > 0 && W > 0);
  const long long hc = (H - 1) / 2 + 1, wc = (W - 1) / 2 + 1;
  REQUIRE((long long)N * 3 * H * W * 4 <= kDesc && (long long)N * 64 * hc * wc * 4 <= kDesc);
  return BNN_HIP_OK;
}
// the stub mirrors the product's support rule and slab arithmetic (csrc/stem_wgrad.hip) with a fixed workgroup count
static size_t stub_wgrad_lds(int W) {
  const int wc = (W - 1) / 2 + 1, need = 2 * ((wc + 15) / 16 * 16) + 8;
  int s = (need + 63) / 64 * 64 + 32;
  if (s - 64 >= need) s -= 64;
  return (size_t)3 * 13 * s * 4;
}
bool stem_wgrad_supported(int H, int W) { return H > 0 && W > 0 && stub_wgrad_lds(W) <= 64 * 1024; }
size_t stem_wgrad_workspace_bytes(int N, int H, int W) {
  if (N <= 0 || !stem_wgrad_supported(H, W)) return 0;
  const long long bands = (long long)N * (((H - 1) / 2 + 1 + 3) / 4);
  return (size_t)std::min<long long>(bands, 768) * 64 * 176 * 4;
}
int launch_stem_wgrad(const float* x, const float* dy, int N, int H, int W, float* work, float* dw, hipStream_t) {
  ++g_reached;
  REQUIRE(x && dy && work && dw && N > 0 && stem_wgrad_supported(H, W));
  const long long hc = (H - 1) / 2 + 1, wc = (W - 1) / 2 + 1;
  REQUIRE((long long)N * 3 * H * W <= 0x7fffffffLL && (long long)N * 64 * hc * wc <= 0x7fffffffLL);
  return BNN_HIP_OK;
}
int launch_avgpool2x2_bwd(const float* gy, int N, int C, int Ho, int Wo, float* gx, hipStream_t) {
  ++g_reached;
  REQUIRE(gy && gx && N > 0 && C > 0 && Ho > 0 && Wo > 0 && (long long)N * C * Ho * Wo * 4 <= 0x7fffffffLL);
  return BNN_HIP_OK;
}
int launch_avgpool_fc(const float* x, const float* wt, const float*, float* out, int N, int C, int HW, int O, hipStream_t) {
  ++g_reached; REQUIRE(x && wt && out && N > 0 && C > 0 && HW > 0 && O > 0); return BNN_HIP_OK;
}
size_t avgpool_fc_workspace_bytes(int N, int C) {
  REQUIRE(N > 0 && C > 0);
  const unsigned long long e = (((unsigned long long)N + 15) / 16) * (unsigned long long)C;
  return e > (1ull << 56) ? ~(size_t)0 : (size_t)(e * 64);
}
bool avgpool_fc_ws_supported(int C, int HW) { REQUIRE(C > 0 && HW > 0); return (size_t)C * 64 <= 160 * 1024 - 1024; }
int launch_avgpool_fc_ws(const float* x, const float* wt, const float*, float* out, float* ws, int N, int C, int HW, int O,
                         hipStream_t) {
  ++g_reached; REQUIRE(x && wt && out && ws && al(ws, 16) && N > 0 && C > 0 && HW > 0 && O > 0 && (size_t)C * 64 <= 160 * 1024 - 1024);
  return BNN_HIP_OK;
}
size_t grad_weight_pack_bytes(int O, int C, int ks) { REQUIRE(O > 0 && C > 0 && (ks == 1 || ks == 3)); return 16; }
int launch_grad_pack_weight(const float* w, int O, int C, int ks, void* packed, float* alpha, hipStream_t) {
  ++g_reached; REQUIRE(w && packed && alpha && O > 0 && C > 0 && (ks == 1 || ks == 3) && al(packed, 16)); return BNN_HIP_OK;
}
static void check_grad(int N, int O, int C, int H, int W, int ks, int stride) {
  REQUIRE(N > 0 && O > 0 && C > 0 && H > 0 && W > 0 && W <= 64 && (ks == 1 || ks == 3) && (stride == 1 || stride == 2));
  REQUIRE((long long)N * O * H * W <= (1LL << 31) - 1 && (long long)N * C * H * W <= (1LL << 31) - 1);
}
int launch_dgrad(const float* g, const float* alpha, const void* packed, const void* x, int planes, float* gx, int N, int O,
                 int C, int H, int W, int ks, int stride, hipStream_t) {
  ++g_reached; REQUIRE(g && alpha && packed && x && gx && al(x, planes ? 8 : 4)); check_grad(N, O, C, H, W, ks, stride);
  return BNN_HIP_OK;
}
static void check_sconv_w(int O, int C, int ks) {
  REQUIRE(O > 0 && C > 0 && (ks == 1 || ks == 3));
  REQUIRE(((long long)C + 31) / 32 * ks * ks * (((long long)O + 15) / 16) * 3 * 64 * 8 <= (1LL << 31) - 1);
}
size_t sconv_weight_pack_bytes(int O, int C, int ks) { check_sconv_w(O, C, ks); return 16; }
int launch_sconv_pack_weight(const float* w, int O, int C, int ks, void* packed, hipStream_t) {
  ++g_reached; REQUIRE(w && packed && al(packed, 16) && al(w, 4)); check_sconv_w(O, C, ks); return BNN_HIP_OK;
}
int launch_sconv(const float* x, const void* packed, const float* bias, const float* scale, float* y, int N, int O, int C,
                 int H, int W, int ks, int stride, hipStream_t) {
  ++g_reached; REQUIRE(x && packed && y && al(packed, 16) && al(x, 4) && al(y, 4) && al(bias, 4) && al(scale, 4));
  check_grad(N, O, C, H, W, ks, stride); check_sconv_w(O, C, ks);
  REQUIRE(ks == 3 || stride == 1);
  REQUIRE((long long)N * C * H * W * 4 <= kDesc && (long long)N * O * ((H - 1) / stride + 1) * ((W - 1) / stride + 1) * 4 <= kDesc);
  return BNN_HIP_OK;
}
int launch_pack_ste(const float* x, int N, int C, int H, int W, uint64_t* P, uint64_t* M, uint64_t* T, hipStream_t) {
  ++g_reached; check_planes(x, N, C, H, W, P, M, 4); REQUIRE(T && al(T, 8)); return BNN_HIP_OK;
}
int launch_bn_pack_ste(const float* x, int N, int C, int H, int W, const float* a, const float* b, uint64_t* P, uint64_t* M,
                       uint64_t* T, hipStream_t) {
  ++g_reached; check_planes(x, N, C, H, W, P, M, 4); REQUIRE(T && al(T, 8) && (a == nullptr) == (b == nullptr) && al(a, 4) && al(b, 4));
  return BNN_HIP_OK;
}
int launch_bn_pack_ste_s2(const float* x, int N, int C, int H, int W, const float* a, const float* b, uint64_t* P, uint64_t* M,
                          uint64_t* T, hipStream_t) {
  ++g_reached; check_planes(x, N, C, H, W, P, M, 4);
  REQUIRE(H % 2 == 0 && W % 2 == 0 && T && al(T, 8) && (a == nullptr) == (b == nullptr) && al(a, 4) && al(b, 4));
  return BNN_HIP_OK;
}
int grad_wgrad_splits(int N, int O, int C, int ks) { REQUIRE(N > 0 && O > 0 && C > 0 && (ks == 1 || ks == 3)); return 1; }
int launch_wgrad(const float* g, const void* x, const void* x2, int planes, float* part, int, int N, int O, int C, int H,
                 int W, int ks, int stride, hipStream_t) {
  ++g_reached; REQUIRE(g && x && part && (!planes || (x2 && al(x, 8) && al(x2, 8)))); check_grad(N, O, C, H, W, ks, stride);
  return BNN_HIP_OK;
}
static void check_linear(int M, int F, int O) {
  REQUIRE(M > 0 && F > 0 && O > 0 && (long long)M * F <= (1LL << 30) - 1 && (long long)M * O <= (1LL << 30) - 1);
  REQUIRE(((long long)O + 31) / 32 * 32 * (2 * (((long long)F + 63) / 64)) <= (1LL << 31) - 1);
}
int launch_blinear_fwd(const void* x, int x_dtype, const uint32_t* wb, const uint32_t* wz, int zeros, const float* alpha,
                       const float* bias, const float* scale, float* out, uint64_t* P, uint64_t* Mn, uint64_t* T, int M, int F,
                       int O, int lds_words, hipStream_t) {
  ++g_reached; check_linear(M, F, O);
  REQUIRE(x_dtype == BNN_HIP_DTYPE_F32 || x_dtype == BNN_HIP_DTYPE_F16 || x_dtype == BNN_HIP_DTYPE_BF16);
  REQUIRE(x && wb && alpha && out && al(x, x_dtype != BNN_HIP_DTYPE_F32 ? 2 : 4) && al(wb, 16) && al(wz, 16) && (!zeros || wz) && al(bias, 4) &&
          al(scale, 4) && al(out, 4) && lds_words >= 0);
  REQUIRE((P == nullptr) == (Mn == nullptr) && (P == nullptr) == (T == nullptr) && al(P, 8) && al(Mn, 8) && al(T, 8));
  return BNN_HIP_OK;
}
int launch_blinear_dgrad(const float* g, const float* alpha, const uint32_t* wb, const uint32_t* wz, const uint64_t* T,
                         float* gx, int M, int O, int F, hipStream_t) {
  ++g_reached; check_linear(M, F, O);
  REQUIRE(g && alpha && wb && wz && T && gx && al(wb, 16) && al(wz, 16) && al(T, 8) && al(g, 4) && al(gx, 4));
  return BNN_HIP_OK;
}
int blinear_wgrad_splits(int M, int O, int F) { check_linear(M, F, O); return 1; }
int launch_blinear_wgrad(const float* g, const uint64_t* P, const uint64_t* Mn, float* part, int splits, int M, int O, int F,
                         hipStream_t) {
  ++g_reached; check_linear(M, F, O);
  REQUIRE(g && P && Mn && part && al(P, 8) && al(Mn, 8) && al(g, 4) && al(part, 4));
  REQUIRE(splits >= 1 && splits <= M && (M + (M + splits - 1) / splits - 1) / ((M + splits - 1) / splits) == splits);
  return BNN_HIP_OK;
}
int slinear_block_channels(int O) { REQUIRE(O > 0); return O > 64 ? 128 : 64; }
int launch_slinear(const float* x, const void* packed, const float* bias, const float* scale, float* out, uint64_t* P,
                   uint64_t* Mn, uint64_t* T, int M, int F, int O, hipStream_t) {
  ++g_reached; check_linear(M, F, O); check_sconv_w(O, F, 1);
  REQUIRE(x && packed && out && al(packed, 16) && al(x, 4) && al(out, 4) && al(bias, 4) && al(scale, 4));
  REQUIRE((P == nullptr) == (Mn == nullptr) && (P == nullptr) == (T == nullptr) && al(P, 8) && al(Mn, 8) && al(T, 8));
  return BNN_HIP_OK;
}
int launch_ste_mask(float* gx, const uint64_t* T, int M, int F, hipStream_t) {
  ++g_reached; REQUIRE(gx && T && al(gx, 4) && al(T, 8) && M > 0 && F > 0 && (long long)M * F <= (1LL << 30) - 1);
  return BNN_HIP_OK;
}
int launch_pack_weight(const float* w, int O, int C, int KH, int KW, int, int, const bnn_hip_wlayout& L, uint32_t* wb,
                       uint32_t* wz, float* alpha, int32_t* flag, hipStream_t) {
  ++g_reached;
  REQUIRE(w && wb && wz && alpha && flag && O > 0 && C > 0 && KH > 0 && KW > 0);
  REQUIRE(L.cw32 == 2 * ((C + 63) / 64) && L.cwc * L.nchunk == L.cw32 && L.o_pad >= O && L.o_pad % 32 == 0);
  REQUIRE(L.n_words == (int64_t)L.o_pad * KH * KW * L.cw32);
  return BNN_HIP_OK;
}
int launch_sign_thresholds(const float* alpha, const float*, const float*, const float* a, const float* b, int O, int kmax,
                           int32_t* thr, hipStream_t) {
  ++g_reached; REQUIRE(alpha && thr && O > 0 && kmax > 0 && kmax < (1 << 20) && (a == nullptr) == (b == nullptr) && al(thr, 4));
  return BNN_HIP_OK;
}
int launch_xnor_grad_pack(const float* w, int O, int C, int ks, int, int, void* packed, float* alpha, hipStream_t) {
  ++g_reached; REQUIRE(w && packed && alpha && O > 0 && C > 0 && (ks == 1 || ks == 3)); return BNN_HIP_OK;
}
int launch_xnor_what(const float* w, int O, int C, int taps, int, int, float* what, float*, hipStream_t) {
  ++g_reached; REQUIRE(w && what && O > 0 && C > 0 && taps > 0 && taps <= 1024 && (long long)O * C * taps <= (1LL << 31) - 1);
  return BNN_HIP_OK;
}
int launch_xnor_weight_bwd(const float* w, const float* g, int splits, int O, int C, int taps, int, int, float* dw, hipStream_t) {
  ++g_reached; REQUIRE(w && g && dw && splits > 0 && O > 0 && C > 0 && taps > 0 && taps <= 1024 && (long long)O * C * taps <= (1LL << 31) - 1 &&
                       (long long)O * C * taps * splits <= 4 * ((1LL << 31) - 1));
  return BNN_HIP_OK;
}
int bn_train_splits(int N, int C, int) { int s = (1024 + C - 1) / C; s = s > 64 ? 64 : s; s = s > N ? N : s; return s < 1 ? 1 : s; }
static void check_bn_args(int N, int C, int HW) {
  REQUIRE(N > 0 && C > 0 && HW > 0 && (long long)N * C * HW <= 4 * ((1LL << 31) - 1));
}
int launch_bn_stats(const float* x, int N, int C, int HW, int S, double* partial, hipStream_t) {
  ++g_reached; check_bn_args(N, C, HW); REQUIRE(x && partial && S >= 1 && S <= N && al(partial, 8)); return BNN_HIP_OK;
}
int launch_bn_act(const float* x, const float* scale, const float* shift, const float* res, int, float* y, int N, int C,
                  int HW, hipStream_t) {
  ++g_reached; check_bn_args(N, C, HW);
  REQUIRE(x && scale && shift && y && al(x, 4) && al(y, 4) && al(scale, 4) && al(shift, 4) && al(res, 4));
  return BNN_HIP_OK;
}
int launch_bn_apply(const float* x, const double* partial, int S, const float*, const float*, const float*, int, float* y,
                    int N, int C, int HW, float eps, float, float* rm, float* rv, float* mo, float* io, float* work,
                    hipStream_t) {
  ++g_reached; check_bn_args(N, C, HW);
  REQUIRE(x && partial && y && mo && io && work && S >= 1 && eps >= 0.0f && (rm == nullptr) == (rv == nullptr) && al(work, 4));
  return BNN_HIP_OK;
}
int launch_bn_bwd_reduce(const float* gy, const float*, const float* x, const float* m, const float* is, int N, int C, int HW,
                         int S, double* partial, hipStream_t) {
  ++g_reached; check_bn_args(N, C, HW); REQUIRE(gy && x && m && is && partial && S >= 1); return BNN_HIP_OK;
}
int launch_bn_bwd_dx(const float* gy, const float*, const float* x, const float* m, const float* is, const float*,
                     const double* partial, int S, float* dx, float*, float*, float*, int N, int C, int HW, float* work,
                     hipStream_t) {
  ++g_reached; check_bn_args(N, C, HW); REQUIRE(gy && x && m && is && partial && dx && work && S >= 1); return BNN_HIP_OK;
}
int launch_bn_finalize(const double* partial, int S, const float*, const float*, int N, int C, int HW, float eps, float,
                       float* rm, float* rv, float* mo, float* io, float* sc, float* sh, hipStream_t) {
  ++g_reached; check_bn_args(N, C, HW);
  REQUIRE(partial && mo && io && sc && sh && S >= 1 && S <= N && eps >= 0.0f && (rm == nullptr) == (rv == nullptr));
  return BNN_HIP_OK;
}
int launch_bn_bwd_dx_add(const float* gy, const float* y, const float* x, const float* m, const float* is, const float*,
                         const double* partial, int S, const float* addend, float* dx, float*, float*, int N, int C, int HW,
                         float* work, hipStream_t) {
  ++g_reached; check_bn_args(N, C, HW);
  REQUIRE(gy && x && m && is && partial && addend && dx && work && S >= 1 && al(addend, 4) && al(dx, 4) && al(y, 4));
  return BNN_HIP_OK;
}
// csrc/bn_train.hip, FactorizedReduce: rows of x and dx move as float2 at least, so even H / W and 8-byte bases
int launch_bn_bwd_s2(const float* g0, const float* g1, const float* x, const float* m, const float* is, const float*, int N,
                     int C, int H, int W, int S, double* partial, float* work, float* dx, float*, float*, hipStream_t) {
  ++g_reached; REQUIRE(H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0 && (long long)H * W <= 0x7fffffffLL); check_bn_args(N, C, H * W);
  REQUIRE(g0 && g1 && x && m && is && partial && work && dx && S >= 1 && S <= N && (long long)N * H * W <= (1LL << 31) - 1);
  REQUIRE(al(g0, 4) && al(g1, 4) && al(x, 8) && al(dx, 8) && al(partial, 8));
  return BNN_HIP_OK;
}
int launch_prelu_shuffle_bwd(const float* gy, const float* z, const float* slope, int count, int N, int O, int HW, int sg,
                             int S, float* gz, float* dslope, double* partial, hipStream_t) {
  ++g_reached; check_bn_args(N, O, HW);
  REQUIRE(gy && z && slope && gz && dslope && partial && gz != gy && (count == 1 || count == O) && sg >= 1 && O % sg == 0);
  REQUIRE(S == bn_train_splits(N, O, HW) && (long long)N * HW <= (1LL << 31) - 1 && al(partial, 8) && al(gy, 4) && al(z, 4) && al(gz, 4));
  return BNN_HIP_OK;
}
int launch_bn_relu_pool_fwd(const float* x, const double* partial, int S, const float*, const float*, float* p, unsigned char* code,
                            int N, int C, int H, int W, float eps, float, float* rm, float* rv, float* mo, float* io, float* work,
                            hipStream_t) {
  ++g_reached; REQUIRE(H > 0 && W > 0 && (long long)H * W <= 0x7fffffffLL); check_bn_args(N, C, H * W);
  REQUIRE(x && partial && p && code && mo && io && work && S >= 1 && eps >= 0.0f && (rm == nullptr) == (rv == nullptr));
  return BNN_HIP_OK;
}
int launch_bn_relu_pool_bwd(const float* gy, const float* p, const unsigned char* code, const float* x, const float* m,
                            const float* is, const float*, int N, int C, int H, int W, int S, double* partial, float* work,
                            float* dx, float*, float*, hipStream_t) {
  ++g_reached; REQUIRE(H > 0 && W > 0 && (long long)H * W <= 0x7fffffffLL); check_bn_args(N, C, H * W);
  REQUIRE(gy && p && code && x && m && is && partial && work && dx && S >= 1);
  return BNN_HIP_OK;
}
// grouped convolutions (csrc/bconv_grouped.hip, pack_weight.hip): the windowed weight layout must hold every block's window
static void check_group_windows(long long O, long long C, long long G, long long S, long long cw32) {
  REQUIRE(G >= 1 && C % G == 0 && O % G == 0 && S >= 1);
  const long long Cg = C / G, Og = O / G, nb = (O + 31) / 32;
  for (int k = 0; k < 40; ++k) {   // the first blocks, the last ones and random ones
    const long long ob = k < 16 ? k : k < 24 ? nb - 1 - (k - 16) : (long long)(rnd() % (uint64_t)nb);
    if (ob < 0 || ob >= nb) continue;
    const long long o0 = 32 * ob, o1 = (O < o0 + 32 ? O : o0 + 32) - 1;
    const long long w_lo = (o0 / Og) * Cg / 32, w_hi = ((o1 / Og + 1) * Cg - 1) / 32;
    REQUIRE(w_lo >= 0 && w_lo <= w_hi && w_hi - w_lo + 1 <= S);
    if (cw32 > 0) REQUIRE(w_hi < cw32);  // the kernel reads words w_lo .. min(w_lo + S, cw32) - 1
  }
}
int launch_pack_weight_grouped(const float* w, int O, int Cg, int groups, int, int, const bnn_hip_wlayout& L,
                               uint32_t* wb, uint32_t* wz, float* alpha, int32_t* flag, hipStream_t) {
  ++g_reached;
  REQUIRE(w && wb && wz && alpha && flag && O > 0 && Cg > 0 && groups > 0 && O % groups == 0);
  REQUIRE(L.cw32 >= 1 && L.cwc == L.cw32 && L.nchunk == 1 && L.o_pad >= O && L.o_pad % 32 == 0 && L.taps > 0);
  REQUIRE(L.n_words == (int64_t)L.o_pad * L.taps * L.cw32 && L.n_words <= (1LL << 31) - 1);
  REQUIRE((long long)O * Cg * L.taps <= (1LL << 31) - 1);
  check_group_windows(O, (long long)Cg * groups, groups, L.cw32, 0);
  return BNN_HIP_OK;
}
int launch_bconv_grouped(const ConvP& p, int groups, int S, hipStream_t) {
  ++g_reached;
  check_convp(p);
  REQUIRE((long long)p.N * p.H * p.Wd * ((p.C + 63) / 64) <= kPlaneWords);
  REQUIRE(p.P && p.M && p.W && p.Z && p.out && al(p.P, 16) && al(p.M, 16) && al(p.W, 16) && al(p.Z, 16) && al(p.out, 4));
  REQUIRE(p.raw ? (!p.alpha && !p.bias && !p.scale) : p.alpha != nullptr);
  REQUIRE(!p.outP && !p.outM && !p.res && !p.bn_a && !p.ds_P);
  REQUIRE((long long)((p.O + 31) / 32 * 32) * p.KH * p.KW * S <= (1LL << 31) - 1);
  check_group_windows(p.O, p.C, groups, S, p.cw32);
  return BNN_HIP_OK;
}
int launch_bconv_grouped_cell(const ConvP& p, int groups, int S, int shuffle_groups, hipStream_t) {
  ++g_reached;
  check_convp(p);
  REQUIRE((long long)p.N * p.H * p.Wd * ((p.C + 63) / 64) <= kPlaneWords);
  REQUIRE(p.P && p.M && p.W && p.Z && p.out && al(p.P, 16) && al(p.M, 16) && al(p.W, 16) && al(p.Z, 16) && al(p.out, 4));
  REQUIRE(!p.raw && p.alpha != nullptr);                                    // no raw-dot form
  REQUIRE(shuffle_groups >= 1 && p.O % shuffle_groups == 0);               // o -> o' stays inside [0, O)
  if (p.res) {   // 4-byte aligned and disjoint from the output tensor
    const uintptr_t r = reinterpret_cast<uintptr_t>(p.res), o = reinterpret_cast<uintptr_t>(p.out);
    const uintptr_t bytes = (uintptr_t)p.N * p.O * p.Ho * p.Wo * 4;
    REQUIRE(al(p.res, 4) && (r >= o + bytes || o >= r + bytes));
  }
  REQUIRE(p.c_off == 0 && p.c_tot == p.O);                                 // residual and output are [N, O, Ho, Wo]
  REQUIRE(!p.outP && !p.outM && !p.bn_a && !p.ds_P && !p.relu);
  REQUIRE((long long)((p.O + 31) / 32 * 32) * p.KH * p.KW * S <= (1LL << 31) - 1);
  check_group_windows(p.O, p.C, groups, S, p.cw32);
  return BNN_HIP_OK;
}
// one term of a cell node: the three views stay inside the 32-bit byte offsets, and `out` shares no element with an operand
int launch_bconv_grouped_node(const ConvP& p, int groups, int S, int shuffle_groups, const float* add, int ct_res, int ct_add,
                              hipStream_t) {
  ++g_reached;
  check_convp(p);
  REQUIRE((long long)p.N * p.H * p.Wd * ((p.C + 63) / 64) <= kPlaneWords);
  REQUIRE(p.P && p.M && p.W && p.Z && p.out && al(p.P, 16) && al(p.M, 16) && al(p.W, 16) && al(p.Z, 16) && al(p.out, 4));
  REQUIRE(!p.raw && p.alpha != nullptr);
  REQUIRE(shuffle_groups >= 1 && p.O % shuffle_groups == 0);
  const long long hw = (long long)p.Ho * p.Wo;
  const uintptr_t o = reinterpret_cast<uintptr_t>(p.out), obytes = (uintptr_t)p.N * p.c_tot * hw * 4;
  const float* opnd[2] = {p.res, add};
  const int ct[2] = {ct_res, ct_add};
  for (int i = 0; i < 2; ++i) {
    if (!opnd[i]) continue;
    REQUIRE(al(opnd[i], 4) && ct[i] >= p.O && (long long)p.N * ct[i] * hw <= kConvElems);
    // the launcher receives channel 0 of the slice: either its image-0 run lies outside the output tensor, or inside it
    // (one tensor, another channel interval) and then clear of the output window of every image
    const uintptr_t a = reinterpret_cast<uintptr_t>(opnd[i]), run = (uintptr_t)p.O * hw * 4;
    if (!(a + (uintptr_t)p.N * ct[i] * hw * 4 <= o || a >= o + obytes)) {
      REQUIRE(ct[i] == p.c_tot && a >= o && (a - o) % (hw * 4) == 0);
      const uintptr_t c0 = (a - o) / (hw * 4);                   // the operand's first channel in the shared tensor
      REQUIRE(c0 + p.O <= (uintptr_t)p.c_tot && (c0 + p.O <= (uintptr_t)p.c_off || c0 >= (uintptr_t)(p.c_off + p.O)));
      (void)run;
    }
  }
  REQUIRE(!p.outP && !p.outM && !p.bn_a && !p.ds_P && !p.relu);
  REQUIRE((long long)((p.O + 31) / 32 * 32) * p.KH * p.KW * S <= (1LL << 31) - 1);
  check_group_windows(p.O, p.C, groups, S, p.cw32);
  return BNN_HIP_OK;
}
// gradients of a grouped convolution (csrc/grad_grouped.hip): the geometry capi.hip's check_grouped_grad states
static void check_grouped_grad(const GroupedGradP& q) {
  REQUIRE(q.N > 0 && q.C > 0 && q.H > 0 && q.W > 0 && q.O > 0 && q.Ho > 0 && q.Wo > 0 && q.KH > 0 && q.KW > 0);
  REQUIRE(q.G >= 2 && q.C % q.G == 0 && q.O % q.G == 0 && q.C / q.G <= 32 && q.KH <= 7 && q.KW <= 7);
  REQUIRE((q.stride == 1 || q.stride == 2) && q.ph >= 0 && q.pw >= 0 && q.dh > 0 && q.dw > 0);
  REQUIRE((long long)q.N * q.O * q.Ho * q.Wo <= kConvElems && (long long)q.N * q.C * q.H * q.W <= kConvElems);
  REQUIRE((long long)q.N * q.H * q.W * ((q.C + 63) / 64) <= kPlaneWords);
  REQUIRE((long long)q.O * (q.C / q.G) * q.KH * q.KW <= (1LL << 31) - 1);
}
int grouped_wgrad_splits(int N, int O, int G, int taps) {
  REQUIRE(N > 0 && O > 0 && G >= 2 && O % G == 0 && taps > 0 && taps <= 49);
  return N < 3 ? N : 3;
}
int launch_grouped_dgrad(const GroupedGradP& q, const float* g, const float* what, const uint64_t* T, float* gx, hipStream_t) {
  ++g_reached; check_grouped_grad(q);
  REQUIRE(g && what && T && gx && al(g, 4) && al(what, 4) && al(T, 8) && al(gx, 4));
  return BNN_HIP_OK;
}
int launch_grouped_wgrad(const GroupedGradP& q, const float* g, const uint64_t* P, const uint64_t* M, float* part, int splits,
                         hipStream_t) {
  ++g_reached; check_grouped_grad(q);
  REQUIRE(g && P && M && part && al(g, 4) && al(P, 8) && al(M, 8) && al(part, 4) && splits >= 1 && splits <= q.N && splits <= 65535);
  return BNN_HIP_OK;
}
// the FactorizedConv launch (csrc/fconv.hip): a geometry the stub's own statement of the kernel's coverage accepts, every
// tensor inside the 32-bit byte offsets, the two fp32 tensors disjoint
bool fconv_supported(int C, int H, int W, int K, int stride) {
  if (C <= 0 || H <= 0 || W <= 0 || K < 1 || K > 7 || K % 2 == 0 || (stride != 1 && stride != 2)) return false;
  return 2LL * ((C + 63) / 64) * K * ((W - 1) / stride + 1) * 8 <= 64 * 1024;
}
int launch_fconv(const FconvP& p, hipStream_t) {
  ++g_reached;
  REQUIRE(p.N > 0 && fconv_supported(p.C, p.H, p.W, p.K, p.stride));
  const long long Ho = (p.H - 1) / p.stride + 1, Wo = (p.W - 1) / p.stride + 1;
  REQUIRE((long long)p.N * p.H * p.W * ((p.C + 63) / 64) <= kPlaneWords && (long long)p.N * p.C * Ho * Wo <= kConvElems);
  REQUIRE(p.P && p.M && p.W1 && p.W2 && p.out && al(p.P, 16) && al(p.M, 16) && al(p.W1, 16) && al(p.W2, 16) && al(p.out, 4));
  REQUIRE(p.wz ? (p.Z1 && p.Z2 && al(p.Z1, 16) && al(p.Z2, 16)) : (!p.Z1 && !p.Z2));
  REQUIRE(p.s1.alpha && p.s2.alpha && p.mid_a && p.mid_b && al(p.s1.alpha, 4) && al(p.s2.alpha, 4) && al(p.mid_a, 4) && al(p.mid_b, 4));
  for (const bnn_hip_fconv_stage* st : {&p.s1, &p.s2}) REQUIRE(al(st->bias, 4) && al(st->post_scale, 4) && al(st->prelu, 4));
  REQUIRE(p.shuffle_groups >= 1 && p.C % p.shuffle_groups == 0);
  if (p.res) {
    const uintptr_t r = reinterpret_cast<uintptr_t>(p.res), o = reinterpret_cast<uintptr_t>(p.out);
    const uintptr_t bytes = (uintptr_t)((long long)p.N * p.C * Ho * Wo) * 4;
    REQUIRE(al(p.res, 4) && (r >= o + bytes || o >= r + bytes));
  }
  return BNN_HIP_OK;
}
int launch_probe_int_alu(int mode, int iters, double* r, double*, hipStream_t) { REQUIRE(iters > 0 && r); (void)mode; return BNN_HIP_OK; }
int launch_probe_clock(int it, double* mhz, double*, hipStream_t) { REQUIRE(it > 0 && mhz); return BNN_HIP_OK; }
}  // namespace bnn

namespace {
const int kInts[] = {INT_MIN, -65536, -1, 0, 1, 2, 3, 7, 8, 31, 32, 33, 63, 64, 65, 127, 128, 129, 224, 255, 256, 1000, 4096,
                     65535, 65536, (1 << 20), (1 << 23), (1 << 24) - 1, (1 << 24), (1 << 28), (1 << 30) - 1, (1 << 30), INT_MAX};
const int kSmall[] = {1, 1, 1, 2, 3, 3, 4, 7, 8, 14, 16, 28, 56, 64, 112, 128, 224, 256, 512};
int pick_int() {
  const uint64_t r = rnd();
  if (r % 4 == 0) return kInts[(r >> 8) % (sizeof(kInts) / sizeof(int))];
  if (r % 4 == 1) return (int)(r >> 33) % 3000 - 10;
  return kSmall[(r >> 8) % (sizeof(kSmall) / sizeof(int))];       // mostly plausible: reach the launchers
}
template <class T>
T* pick_ptr() {
  static const uintptr_t kPtrs[] = {0, 0x10000, 0x10000, 0x10000, 0x10001, 0x10002, 0x10004, 0x10008, 0x7fff0000fff0ull};
  return reinterpret_cast<T*>(kPtrs[rnd() % (sizeof(kPtrs) / sizeof(uintptr_t))]);
}
bnn_hip_conv_desc pick_desc() {
  bnn_hip_conv_desc d;
  int* f = reinterpret_cast<int*>(&d);
  for (size_t i = 0; i < sizeof(d) / sizeof(int); ++i) f[i] = pick_int();
  if (rnd() % 2) { d.KH = d.KW = (rnd() % 2) ? 3 : 1; d.stride_h = d.stride_w = 1 + (int)(rnd() % 2); d.dil_h = d.dil_w = 1;
                   d.pad_h = d.pad_w = d.KH / 2; }
  d.flags = (int)(rnd() % 128);
  return d;
}
// a group count for C / O: mostly one that divides them (the BATS shapes, depthwise), sometimes anything
int pick_groups(int C, int O) {
  const uint64_t r = rnd() % 8;
  if (r == 0) return pick_int();
  if (r == 1) return C;
  const int g[] = {1, 2, 3, 4, 12, 16};
  const int v = g[rnd() % 6];
  return (C > 0 && O > 0 && C % v == 0 && O % v == 0) ? v : 1;
}
// a channel-slice view of C channels: mostly a valid window, sometimes anything; bases far apart or shared
bnn_hip_f32_view pick_view(int C) {
  static const uintptr_t kBases[] = {0, 0x10000, 0x10000, 0x10002, 0x40000000, 0x7fff0000fff0ull};
  bnn_hip_f32_view v;
  v.p = reinterpret_cast<const float*>(kBases[rnd() % (sizeof(kBases) / sizeof(uintptr_t))]);
  const uint64_t r = rnd() % 8;
  if (r == 0) { v.c_offset = pick_int(); v.c_total = pick_int(); }
  else if (r == 1) { v.c_offset = 0; v.c_total = 0; }
  else { v.c_offset = (int)(rnd() % 3) * (C > 0 && C < (1 << 20) ? C : 1); v.c_total = v.c_offset + (C > 0 && C < (1 << 20) ? C : 1) * (int)(1 + rnd() % 3); }
  return v;
}
bool status_ok(int st) { return st <= 0 && st >= -5; }
}  // namespace

int main(int argc, char** argv) {
  const long iters = argc > 1 ? std::atol(argv[1]) : 200000;
  if (argc > 2) g_rng ^= (uint64_t)std::atoll(argv[2]) * 0xD1342543DE82EF95ull + 1;
  void* stream = nullptr;
  uint64_t digest = 0xCBF29CE484222325ull;
  for (long it = 0; it < iters; ++it) {
    ++g_calls;
    int st = 0;
    switch (rnd() % 64) {
      case 0: { bnn_hip_conv_desc d = pick_desc();
        st = bnn_hip_bconv2d(rnd() % 16 ? &d : nullptr, pick_ptr<uint64_t>(), pick_ptr<uint64_t>(), pick_ptr<uint32_t>(),
                             pick_ptr<uint32_t>(), pick_ptr<float>(), pick_ptr<float>(), pick_ptr<float>(), pick_ptr<float>(), stream);
        break; }
      case 1: { bnn_hip_conv_desc d = pick_desc(); bnn_hip_epilogue e; std::memset(&e, 0, sizeof(e));
        e.alpha = pick_ptr<float>(); e.bias = pick_ptr<float>(); e.post_scale = pick_ptr<float>(); e.bn_scale = pick_ptr<float>();
        e.bn_shift = pick_ptr<float>(); e.residual = pick_ptr<float>(); e.prelu = pick_ptr<float>(); e.relu = pick_int();
        e.flags = (int)(rnd() % 8); e.out_f32 = pick_ptr<float>(); e.out_P = pick_ptr<uint64_t>(); e.out_M = pick_ptr<uint64_t>();
        e.pack_scale = pick_ptr<float>(); e.pack_shift = pick_ptr<float>(); e.out_c_offset = pick_int(); e.out_c_total = pick_int();
        e.sign_thresholds = pick_ptr<int32_t>();
        if (rnd() % 3 == 0) { e.sc_P = pick_ptr<uint64_t>(); e.sc_wbits = pick_ptr<uint32_t>(); e.sc_alpha = pick_ptr<float>();
                              e.sc_bn_scale = pick_ptr<float>(); e.sc_bn_shift = pick_ptr<float>(); e.sc_C = pick_int(); }
        st = bnn_hip_bconv2d_fused(&d, pick_ptr<uint64_t>(), pick_ptr<uint64_t>(), pick_ptr<uint32_t>(), pick_ptr<uint32_t>(),
                                   rnd() % 16 ? &e : nullptr, stream);
        break; }
      case 2: { bnn_hip_conv_desc d = pick_desc();
        st = bnn_hip_bconv2d_dot(&d, pick_ptr<uint64_t>(), pick_ptr<uint64_t>(), pick_ptr<uint32_t>(), pick_ptr<uint32_t>(),
                                 pick_ptr<int32_t>(), stream);
        break; }
      case 3: { bnn_hip_conv_desc d = pick_desc(); bnn_hip_fly_plan plan; std::memset(&plan, 0, sizeof(plan));
        st = bnn_hip_bconv2d_direct(&d, pick_ptr<float>(), (int)(rnd() % 3), pick_ptr<uint32_t>(), pick_ptr<uint32_t>(),
                                    pick_ptr<float>(), pick_ptr<float>(), pick_ptr<float>(), pick_ptr<float>(),
                                    rnd() % 2 ? &plan : nullptr, stream);
        break; }
      case 4: { bnn_hip_conv_desc d = pick_desc(); bnn_hip_fly_plan plan;
        st = bnn_hip_bconv2d_direct_plan(rnd() % 16 ? &d : nullptr, rnd() % 16 ? &plan : nullptr);
        break; }
      case 5: { bnn_hip_conv_desc d = pick_desc();
        const size_t ws = bnn_hip_conv_workspace_bytes(&d);
        if (ws > (size_t)1 << 40) broken("workspace size overflow");
        st = bnn_hip_bconv2d_f32(&d, pick_ptr<float>(), pick_ptr<uint32_t>(), pick_ptr<uint32_t>(), pick_ptr<float>(),
                                 pick_ptr<float>(), pick_ptr<float>(), pick_ptr<float>(), pick_ptr<char>(), stream);
        break; }
      case 6: st = bnn_hip_pack_act_f32(pick_ptr<float>(), pick_int(), pick_int(), pick_int(), pick_int(), pick_ptr<uint64_t>(),
                                        pick_ptr<uint64_t>(), stream); break;
      case 7: st = bnn_hip_pack_act_f16(pick_ptr<char>(), pick_int(), pick_int(), pick_int(), pick_int(), pick_ptr<uint64_t>(),
                                        pick_ptr<uint64_t>(), stream); break;
      case 8: st = bnn_hip_bn_act_pack_f32(pick_ptr<float>(), pick_int(), pick_int(), pick_int(), pick_int(), pick_ptr<float>(),
                                           pick_ptr<float>(), pick_int(), pick_ptr<uint64_t>(), pick_ptr<uint64_t>(), stream); break;
      case 9: st = bnn_hip_avgpool_pack_f32(pick_ptr<float>(), pick_int(), pick_int(), pick_int(), pick_int(), pick_int(),
                                            pick_ptr<uint64_t>(), pick_ptr<uint64_t>(), stream); break;
      case 10: st = bnn_hip_orpool_packed(pick_ptr<uint64_t>(), pick_int(), pick_int(), pick_int(), pick_int(), pick_int(),
                                          pick_ptr<uint64_t>(), pick_ptr<uint64_t>(), stream); break;
      case 11: st = bnn_hip_bn_relu_maxpool_pack_f32(pick_ptr<float>(), pick_int(), pick_int(), pick_int(), pick_int(),
                                                     pick_ptr<float>(), pick_ptr<float>(), pick_int(), pick_int(), pick_int(),
                                                     pick_int(), pick_ptr<float>(), pick_ptr<uint64_t>(), pick_ptr<uint64_t>(), stream); break;
      case 12: st = bnn_hip_stem7x7_bn_relu_pool_pack_f32(pick_ptr<float>(), pick_ptr<float>(), pick_ptr<float>(), pick_ptr<float>(),
                                                          pick_int(), pick_int(), pick_int(), (int)(rnd() % 16), pick_ptr<float>(),
                                                          pick_ptr<uint64_t>(), pick_ptr<uint64_t>(), stream); break;
      case 13: st = bnn_hip_avgpool_fc_f32(pick_ptr<float>(), pick_int(), pick_int(), pick_int(), pick_ptr<float>(), pick_ptr<float>(),
                                           pick_int(), pick_ptr<float>(), stream); break;
      case 14: { bnn_hip_wlayout L;
        st = bnn_hip_weight_layout(pick_int(), pick_int(), pick_int(), pick_int(), rnd() % 16 ? &L : nullptr);
        if (st == BNN_HIP_OK && (L.n_words <= 0 || L.cwc * L.nchunk != L.cw32)) broken("weight layout");
        break; }
      case 15: st = bnn_hip_pack_weight_f32(pick_ptr<float>(), pick_int(), pick_int(), pick_int(), pick_int(), pick_int(), pick_int(),
                                            pick_ptr<uint32_t>(), pick_ptr<uint32_t>(), pick_ptr<float>(), pick_ptr<int32_t>(), stream); break;
      case 16: st = bnn_hip_bconv_grad_input_f32(pick_ptr<float>(), pick_ptr<float>(), pick_ptr<char>(), pick_ptr<float>(),
                                                 pick_ptr<float>(), pick_int(), pick_int(), pick_int(), pick_int(), pick_int(),
                                                 (int)(rnd() % 5), (int)(rnd() % 4), stream); break;
      case 17: st = bnn_hip_bconv_grad_weight_f32(pick_ptr<float>(), pick_ptr<float>(), pick_ptr<float>(), pick_int(), pick_int(),
                                                  pick_int(), pick_int(), pick_int(), pick_int(), (int)(rnd() % 5), (int)(rnd() % 4), stream); break;
      case 18: st = bnn_hip_sign_thresholds_f32(pick_ptr<float>(), pick_ptr<float>(), pick_ptr<float>(), pick_ptr<float>(),
                                                pick_ptr<float>(), pick_int(), pick_int(), pick_ptr<int32_t>(), stream); break;
      case 19: st = bnn_hip_pack_act_ste_f32(pick_ptr<float>(), pick_int(), pick_int(), pick_int(), pick_int(), pick_ptr<uint64_t>(),
                                             pick_ptr<uint64_t>(), pick_ptr<uint64_t>(), stream); break;
      case 20: st = bnn_hip_bconv_grad_input_packed_f32(pick_ptr<float>(), pick_ptr<float>(), pick_ptr<char>(), pick_ptr<uint64_t>(),
                                                        pick_ptr<float>(), pick_int(), pick_int(), pick_int(), pick_int(), pick_int(),
                                                        (int)(rnd() % 5), (int)(rnd() % 4), stream); break;
      case 21: st = bnn_hip_bconv_grad_weight_packed_f32(pick_ptr<float>(), pick_ptr<uint64_t>(), pick_ptr<uint64_t>(), pick_ptr<float>(),
                                                         pick_int(), pick_int(), pick_int(), pick_int(), pick_int(), pick_int(),
                                                         (int)(rnd() % 5), (int)(rnd() % 4), stream); break;
      case 22: { const int N = pick_int(), C = pick_int(), HW = pick_int();
        if (bnn_hip_bn_train_workspace_bytes(N, C, HW) > ((size_t)1 << 40)) broken("bn workspace size");
        st = bnn_hip_bn_train_forward_f32(pick_ptr<float>(), N, C, HW, pick_ptr<float>(), pick_ptr<float>(), pick_ptr<float>(),
                                          pick_int(), (float)(pick_int() % 3) * 1e-5f, 0.1f, pick_ptr<float>(), pick_ptr<float>(),
                                          pick_ptr<float>(), pick_ptr<float>(), pick_ptr<float>(), pick_ptr<double>(), stream);
        break; }
      case 23: st = bnn_hip_bn_train_backward_f32(pick_ptr<float>(), pick_ptr<float>(), pick_ptr<float>(), pick_ptr<float>(),
                                                  pick_ptr<float>(), pick_ptr<float>(), pick_int(), pick_int(), pick_int(),
                                                  pick_ptr<float>(), pick_ptr<float>(), pick_ptr<float>(), pick_ptr<float>(),
                                                  pick_ptr<double>(), stream); break;
      case 24: st = bnn_hip_bn_relu_maxpool_train_forward_f32(pick_ptr<float>(), pick_int(), pick_int(), pick_int(), pick_int(),
                                                              pick_ptr<float>(), pick_ptr<float>(), 1e-5f, 0.1f, pick_ptr<float>(),
                                                              pick_ptr<float>(), pick_ptr<float>(), pick_ptr<uint8_t>(),
                                                              pick_ptr<float>(), pick_ptr<float>(), pick_ptr<double>(), stream); break;
      case 25: st = bnn_hip_bn_relu_maxpool_train_backward_f32(pick_ptr<float>(), pick_ptr<float>(), pick_ptr<uint8_t>(),
                                                               pick_ptr<float>(), pick_ptr<float>(), pick_ptr<float>(),
                                                               pick_ptr<float>(), pick_int(), pick_int(), pick_int(), pick_int(),
                                                               pick_ptr<float>(), pick_ptr<float>(), pick_ptr<float>(),
                                                               pick_ptr<double>(), stream); break;
      case 26: st = bnn_hip_xnor_weight_forward_f32(pick_ptr<float>(), pick_int(), pick_int(), pick_int(), pick_int(), pick_int(),
                                                    pick_int(), pick_ptr<float>(), pick_ptr<float>(), stream); break;
      case 27: st = bnn_hip_xnor_weight_backward_f32(pick_ptr<float>(), pick_ptr<float>(), pick_int(), pick_int(), pick_int(), pick_int(),
                                                     pick_int(), pick_int(), pick_int(), pick_ptr<float>(), stream); break;
      case 28: st = bnn_hip_bn_act_f32(pick_ptr<float>(), pick_int(), pick_int(), pick_int(), pick_ptr<float>(), pick_ptr<float>(),
                                       pick_ptr<float>(), pick_int(), pick_ptr<float>(), stream); break;
      case 29: { const int n = pick_int(), c = pick_int();
        const size_t need = bnn_hip_avgpool_fc_workspace_bytes(n, c);
        st = bnn_hip_avgpool_fc_ws_f32(pick_ptr<float>(), n, c, pick_int(), pick_ptr<float>(), pick_ptr<float>(), pick_int(),
                                       pick_ptr<float>(), pick_ptr<float>(), rnd() % 4 ? need : (size_t)(rnd() % 4096), stream);
        break; }
      case 30: st = bnn_hip_stem7x7_conv_f32(pick_ptr<float>(), pick_ptr<float>(), pick_int(), pick_int(), pick_int(),
                                             (int)(rnd() % 8), pick_ptr<float>(), stream); break;
      case 31: { const int n = pick_int(), h = pick_int(), w = pick_int();
        const size_t need = bnn_hip_stem7x7_wgrad_workspace_bytes(n, h, w);
        st = bnn_hip_stem7x7_wgrad_f32(pick_ptr<float>(), pick_ptr<float>(), n, h, w, pick_ptr<float>(),
                                       rnd() % 4 ? need : (size_t)(rnd() % 4096), pick_ptr<float>(), stream);
        break; }
      case 32: st = bnn_hip_avgpool2x2_backward_f32(pick_ptr<float>(), pick_int(), pick_int(), pick_int(), pick_int(),
                                                    pick_ptr<float>(), stream); break;
      case 34: st = bnn_hip_avgpool2_bn_pack2_f32(pick_ptr<float>(), pick_int(), pick_int(), pick_int(), pick_int(), pick_ptr<float>(),
                                                  pick_ptr<float>(), pick_int(), pick_ptr<uint64_t>(), pick_ptr<uint64_t>(),
                                                  pick_ptr<float>(), pick_ptr<float>(), pick_int(), pick_ptr<uint64_t>(),
                                                  pick_ptr<uint64_t>(), pick_ptr<float>(), stream); break;
      case 35: { bnn_hip_hblock_desc d; int* f = reinterpret_cast<int*>(&d);
        for (size_t i = 0; i < sizeof(d) / sizeof(int); ++i) f[i] = pick_int();
        if (rnd() % 2) { d.planes = 64 << (rnd() % 4); d.C_in = rnd() % 2 ? d.planes : d.planes / 2; d.flags = (int)(rnd() % 2) * 64 + (int)(rnd() % 2) * 128; if (rnd() % 2) d.H = d.W = (rnd() % 2) ? 7 : 14;
                         d.rows_per_band = d.images_per_band = d.waves = 0; }
        (void)bnn_hip_hblock_supported(rnd() % 16 ? &d : nullptr);
        st = bnn_hip_hblock_forward(rnd() % 16 ? &d : nullptr, pick_ptr<uint64_t>(), pick_ptr<uint32_t>(), pick_ptr<float>(),
                                    pick_ptr<float>(), pick_ptr<float>(), pick_ptr<uint64_t>(), stream);
        break; }
      case 36: { bnn_hip_hblock_layout L;
        st = bnn_hip_hblock_layout_of(pick_int(), pick_int(), rnd() % 16 ? &L : nullptr);
        if (st == BNN_HIP_OK && (L.weight_words <= 0 || L.const_floats <= 0)) broken("hblock layout");
        break; }
      case 38: st = bnn_hip_hblock_pack_weights_cl(pick_int(), pick_int(), pick_ptr<uint32_t>(), pick_ptr<uint32_t>(), pick_ptr<uint32_t>(),
                                                   pick_ptr<uint32_t>(), stream); break;
      case 39: st = bnn_hip_stem7x7_bn_relu_pool_pack_affine_f32(pick_ptr<float>(), pick_ptr<float>(), pick_ptr<float>(), pick_ptr<float>(),
                                                                pick_ptr<float>(), pick_ptr<float>(), pick_int(), pick_int(), pick_int(),
                                                                pick_int() & 3, pick_ptr<float>(), pick_ptr<uint64_t>(),
                                                                pick_ptr<uint64_t>(), stream); break;
      case 40: { bnn_hip_hblock_desc d; int* f = reinterpret_cast<int*>(&d);
        for (size_t i = 0; i < sizeof(d) / sizeof(int); ++i) f[i] = pick_int();
        if (rnd() % 2) { d.planes = d.C_in = 64 << (rnd() % 3); d.flags = (int)(rnd() % 2) * 64; d.H = d.W = 2 * (1 + (int)(rnd() % 28));
                         d.rows_per_band = d.images_per_band = d.waves = 0; }
        (void)bnn_hip_hblock_pool_supported(rnd() % 16 ? &d : nullptr);
        st = bnn_hip_hblock_pool_forward(rnd() % 16 ? &d : nullptr, pick_ptr<uint64_t>(), pick_ptr<uint32_t>(), pick_ptr<float>(),
                                         pick_ptr<float>(), pick_ptr<float>(), pick_ptr<uint64_t>(), pick_ptr<uint64_t>(),
                                         pick_ptr<uint64_t>(), stream);
        break; }
      case 41: { bnn_hip_hblock_desc d; int* f = reinterpret_cast<int*>(&d);
        for (size_t i = 0; i < sizeof(d) / sizeof(int); ++i) f[i] = pick_int();
        if (rnd() % 2) { d.C_in = 64 << (rnd() % 3); d.planes = 2 * d.C_in; d.flags = (int)(rnd() % 2) * 64 + (int)(rnd() % 2) * 128; d.H = d.W = (rnd() % 2) ? (rnd() % 2 ? 7 : 14) : 1 + (int)(rnd() % 56);
                         d.rows_per_band = d.images_per_band = d.waves = 0; }
        (void)bnn_hip_hblock_shortcut_supported(rnd() % 16 ? &d : nullptr);
        st = bnn_hip_hblock_shortcut_forward(rnd() % 16 ? &d : nullptr, pick_ptr<uint64_t>(), pick_ptr<uint32_t>(), pick_ptr<float>(),
                                             pick_ptr<uint64_t>(), pick_ptr<uint64_t>(), pick_ptr<uint32_t>(), pick_ptr<float>(),
                                             pick_ptr<float>(), pick_ptr<uint64_t>(), stream);
        break; }
      case 42: st = bnn_hip_hblock_pack_shortcut_weights(pick_int(), pick_int(), pick_ptr<uint32_t>(), pick_ptr<uint32_t>(), stream); break;
      case 37: st = bnn_hip_hblock_pack_weights(pick_int(), pick_int(), pick_ptr<uint32_t>(), pick_ptr<uint32_t>(), pick_ptr<uint32_t>(),
                                                pick_ptr<uint32_t>(), stream); break;
      case 33: st = bnn_hip_xnor_grad_pack_weight_f32(pick_ptr<float>(), pick_int(), pick_int(), pick_int(), pick_int(), pick_int(),
                                                      pick_ptr<float>(), pick_ptr<float>(), stream); break;
      case 44: { bnn_hip_wlayout L; const int O = pick_int(), C = pick_int(), G = pick_groups(C, O);
        st = bnn_hip_grouped_weight_layout(O, C, G, pick_int(), pick_int(), rnd() % 16 ? &L : nullptr);
        if (st == BNN_HIP_OK && (L.cw32 < 1 || L.nchunk != 1 || L.n_words != (int64_t)L.o_pad * L.taps * L.cw32))
          broken("grouped weight layout");
        if (st == BNN_HIP_OK) bnn::check_group_windows(O, C, G, L.cw32, 2 * ((C + 63LL) / 64));
        break; }
      case 45: { const int O = pick_int(), Cg = pick_int(), G = rnd() % 4 ? pick_groups(O, O) : pick_int();
        st = bnn_hip_pack_weight_grouped_f32(pick_ptr<float>(), O, Cg, G, pick_int(), pick_int(), pick_int(), pick_int(),
                                             pick_ptr<uint32_t>(), pick_ptr<uint32_t>(), pick_ptr<float>(),
                                             pick_ptr<int32_t>(), stream);
        break; }
      case 46: { bnn_hip_conv_desc d = pick_desc();
        if (rnd() % 2) { d.O = d.C; }   // depthwise / BATS-like: C == O
        const bool raw = rnd() % 4 == 0;
        st = bnn_hip_bconv2d_grouped(rnd() % 16 ? &d : nullptr, pick_groups(d.C, d.O), pick_ptr<uint64_t>(),
                                     pick_ptr<uint64_t>(), pick_ptr<uint32_t>(), pick_ptr<uint32_t>(),
                                     raw ? nullptr : pick_ptr<float>(), raw ? nullptr : pick_ptr<float>(),
                                     raw ? nullptr : pick_ptr<float>(), pick_ptr<float>(), stream);
        break; }
      case 47: { bnn_hip_conv_desc d = pick_desc();
        if (rnd() % 2) { d.O = d.C; }
        const int sgs[] = {1, 1, 2, 4, 12};
        const int sg = rnd() % 8 ? sgs[rnd() % 5] : pick_int();
        float* out = pick_ptr<float>();
        const float* res = rnd() % 3 == 0 ? nullptr : rnd() % 4 == 0 ? out : pick_ptr<float>();
        st = bnn_hip_bconv2d_grouped_fused(rnd() % 16 ? &d : nullptr, pick_groups(d.C, d.O), pick_ptr<uint64_t>(),
                                           pick_ptr<uint64_t>(), pick_ptr<uint32_t>(), pick_ptr<uint32_t>(),
                                           pick_ptr<float>(), pick_ptr<float>(), pick_ptr<float>(), pick_ptr<float>(), sg,
                                           res, out, stream);
        break; }
      case 48: { const int C = pick_int(); const bnn_hip_f32_view x = pick_view(C);
        st = bnn_hip_bn_act_pack_multi_f32(rnd() % 16 ? &x : nullptr, pick_int(), C, pick_int(), pick_int(),
                                           rnd() % 4 ? 1 + (int)(rnd() % 4) : pick_int(), pick_ptr<float>(), pick_ptr<float>(),
                                           pick_int(), pick_ptr<uint64_t>(), pick_ptr<uint64_t>(), stream);
        break; }
      case 49: { const int C = pick_int(); const bnn_hip_f32_view x = pick_view(C);
        const int H = rnd() % 4 ? 2 * (int)(1 + rnd() % 16) : pick_int(), W = rnd() % 4 ? 2 * (int)(1 + rnd() % 16) : pick_int();
        st = bnn_hip_bn_act_pack_s2_f32(rnd() % 16 ? &x : nullptr, pick_int(), C, H, W, pick_ptr<float>(), pick_ptr<float>(),
                                        pick_int(), pick_ptr<uint64_t>(), pick_ptr<uint64_t>(), stream);
        break; }
      case 50: { bnn_hip_conv_desc d = pick_desc();
        if (rnd() % 2) { d.O = d.C; }
        const int sgs[] = {1, 1, 2, 4, 12};
        const int sg = rnd() % 8 ? sgs[rnd() % 5] : pick_int();
        // the views: often slices of ONE tensor (the cell output), disjoint or overlapping; else anything
        bnn_hip_f32_view out = pick_view(d.O), res = pick_view(d.O), add = pick_view(d.O);
        if (rnd() % 2) { res.p = out.p; res.c_total = out.c_total; }
        if (rnd() % 2) { add.p = out.p; add.c_total = out.c_total; }
        st = bnn_hip_bconv2d_grouped_node(rnd() % 16 ? &d : nullptr, pick_groups(d.C, d.O), pick_ptr<uint64_t>(),
                                          pick_ptr<uint64_t>(), pick_ptr<uint32_t>(), pick_ptr<uint32_t>(), pick_ptr<float>(),
                                          pick_ptr<float>(), pick_ptr<float>(), pick_ptr<float>(), sg,
                                          rnd() % 3 ? &res : nullptr, rnd() % 3 ? &add : nullptr, const_cast<float*>(out.p),
                                          out.c_offset, out.c_total, stream);
        break; }
      case 51: { bnn_hip_conv_desc d = pick_desc();
        if (rnd() % 2) { d.O = d.C; }
        const int G = pick_groups(d.C, d.O);
        const bnn_hip_conv_desc* dp = rnd() % 16 ? &d : nullptr;
        const int ok = bnn_hip_bconv_grouped_grad_supported(dp, G);
        if (ok != 0 && ok != 1) broken("grouped grad supported");
        st = bnn_hip_bconv_grouped_grad_input_f32(dp, G, pick_ptr<float>(), pick_ptr<float>(),
                                                  pick_ptr<uint64_t>(), pick_ptr<float>(), stream);
        if (st == BNN_HIP_OK && !ok) broken("grouped input gradient launched on an unsupported geometry");
        break; }
      case 52: { bnn_hip_conv_desc d = pick_desc();
        if (rnd() % 2) { d.O = d.C; }
        const int G = pick_groups(d.C, d.O);
        const bnn_hip_conv_desc* dp = rnd() % 16 ? &d : nullptr;
        const int sp = bnn_hip_bconv_grouped_grad_weight_splits(dp, G);
        if (sp < 0 || (sp > 0 && sp > d.N) || (sp > 0) != (bnn_hip_bconv_grouped_grad_supported(dp, G) == 1)) broken("grouped grad splits");
        st = bnn_hip_bconv_grouped_grad_weight_f32(dp, G, pick_ptr<float>(), pick_ptr<uint64_t>(),
                                                   pick_ptr<uint64_t>(), pick_ptr<float>(), rnd() % 4 ? sp : pick_int(), stream);
        break; }
      case 53: st = bnn_hip_stem3x3_bn_relu_pack_f32(pick_ptr<float>(), pick_ptr<float>(), pick_ptr<float>(), pick_ptr<float>(),
                                                     pick_ptr<float>(), pick_ptr<float>(), pick_int(), pick_int(), pick_int(),
                                                     pick_int(), rnd() % 4 ? 1 + (int)(rnd() % 4) : pick_int(),
                                                     pick_ptr<uint64_t>(), pick_ptr<uint64_t>(), pick_ptr<float>(), stream);
        break;
      case 54: { const int C1 = pick_int(), C = (rnd() % 2 && C1 > 0 && C1 < (1 << 20)) ? 2 * C1 : pick_int();
        st = bnn_hip_stem_s2x2_f32(pick_ptr<float>(), pick_ptr<float>(), pick_ptr<float>(), pick_ptr<float>(), pick_ptr<float>(),
                                   pick_ptr<float>(), pick_ptr<float>(), pick_int(), C1, C, pick_groups(C1, C), pick_int(),
                                   pick_int(), (int)(rnd() % 3), pick_ptr<float>(), stream);
        break; }
      case 55: { const int C = pick_int(), O = rnd() % 2 ? C : pick_int();
        st = bnn_hip_gconv3x3s2_bn_pack_f32(pick_ptr<float>(), pick_ptr<float>(), pick_ptr<float>(), pick_ptr<float>(),
                                            pick_ptr<float>(), pick_ptr<float>(), pick_int(), C, O, pick_groups(C, O), pick_int(),
                                            pick_int(), (int)(rnd() % 3), rnd() % 4 ? (int)(rnd() % 5) : pick_int(),
                                            pick_ptr<uint64_t>(), pick_ptr<uint64_t>(), pick_ptr<float>(), stream);
        break; }
      case 56: st = bnn_hip_bn_act_pack_ste_f32(pick_ptr<float>(), pick_int(), pick_int(), pick_int(), pick_int(), pick_ptr<float>(),
                                                pick_ptr<float>(), pick_ptr<uint64_t>(), pick_ptr<uint64_t>(), pick_ptr<uint64_t>(),
                                                stream); break;
      case 57: st = bnn_hip_bn_train_pack_ste_f32(pick_ptr<float>(), pick_int(), pick_int(), pick_int(), pick_int(), pick_ptr<float>(),
                                                  pick_ptr<float>(), (float)(pick_int() % 3) * 1e-5f, 0.1f, pick_ptr<float>(),
                                                  pick_ptr<float>(), pick_ptr<uint64_t>(), pick_ptr<uint64_t>(), pick_ptr<uint64_t>(),
                                                  pick_ptr<float>(), pick_ptr<float>(), pick_ptr<float>(), pick_ptr<float>(),
                                                  pick_ptr<double>(), stream); break;
      case 58: st = bnn_hip_bn_train_backward_add_f32(pick_ptr<float>(), pick_ptr<float>(), pick_ptr<float>(), pick_ptr<float>(),
                                                      pick_ptr<float>(), pick_ptr<float>(), pick_ptr<float>(), pick_int(), pick_int(),
                                                      pick_int(), pick_ptr<float>(), pick_ptr<float>(), pick_ptr<float>(),
                                                      pick_ptr<double>(), stream); break;
      case 59: { const int N = pick_int(), O = pick_int(), HW = pick_int();
        const int sgs[] = {1, 1, 2, 4, 12};
        const int sg = rnd() % 8 ? sgs[rnd() % 5] : pick_int();
        const size_t need = bnn_hip_prelu_shuffle_backward_workspace_bytes(N, O, HW);
        if (need > ((size_t)1 << 40)) broken("prelu backward workspace size");
        float* gz = pick_ptr<float>();
        st = bnn_hip_prelu_shuffle_backward_f32(rnd() % 8 ? pick_ptr<float>() : gz, rnd() % 4 ? pick_ptr<float>() : gz,
                                                pick_ptr<float>(), rnd() % 3 ? (rnd() % 2 ? 1 : O) : pick_int(), N, O, HW, sg, gz,
                                                pick_ptr<float>(), pick_ptr<double>(),
                                                rnd() % 4 ? need : (size_t)(rnd() % 4096), stream);
        break; }
      case 60: { const int H = rnd() % 4 ? 2 * (int)(1 + rnd() % 16) : pick_int(), W = rnd() % 4 ? 2 * (int)(1 + rnd() % 16) : pick_int();
        st = bnn_hip_bn_act_pack_ste_s2_f32(pick_ptr<float>(), pick_int(), pick_int(), H, W, pick_ptr<float>(), pick_ptr<float>(),
                                            pick_ptr<uint64_t>(), pick_ptr<uint64_t>(), pick_ptr<uint64_t>(), stream);
        break; }
      case 61: { const int H = rnd() % 4 ? 2 * (int)(1 + rnd() % 16) : pick_int(), W = rnd() % 4 ? 2 * (int)(1 + rnd() % 16) : pick_int();
        st = bnn_hip_bn_train_pack_ste_s2_f32(pick_ptr<float>(), pick_int(), pick_int(), H, W, pick_ptr<float>(), pick_ptr<float>(),
                                              (float)(pick_int() % 3) * 1e-5f, 0.1f, pick_ptr<float>(), pick_ptr<float>(),
                                              pick_ptr<uint64_t>(), pick_ptr<uint64_t>(), pick_ptr<uint64_t>(), pick_ptr<float>(),
                                              pick_ptr<float>(), pick_ptr<float>(), pick_ptr<float>(), pick_ptr<double>(), stream);
        break; }
      case 62: { const int H = rnd() % 4 ? 2 * (int)(1 + rnd() % 16) : pick_int(), W = rnd() % 4 ? 2 * (int)(1 + rnd() % 16) : pick_int();
        st = bnn_hip_bn_train_backward_s2_f32(pick_ptr<float>(), pick_ptr<float>(), pick_ptr<float>(), pick_ptr<float>(),
                                              pick_ptr<float>(), pick_ptr<float>(), pick_int(), pick_int(), H, W, pick_ptr<float>(),
                                              pick_ptr<float>(), pick_ptr<float>(), pick_ptr<double>(), stream);
        break; }
      default: { bnn_hip_conv_desc d = pick_desc();
        (void)bnn_hip_shortcut_fold_supported(rnd() % 16 ? &d : nullptr, pick_int());
        { // the FactorizedConv entry points: mostly a plausible geometry, sometimes anything
          bnn_hip_fconv_desc fd;
          fd.N = pick_int(); fd.C = pick_int(); fd.H = pick_int(); fd.W = pick_int(); fd.K = pick_int(); fd.stride = pick_int();
          fd.flags = (int)(rnd() % 4); fd.reserved = 0;
          if (rnd() % 2) { fd.K = 1 + 2 * (int)(rnd() % 4); fd.stride = 1 + (int)(rnd() % 2); }
          if (rnd() % 2) { fd.C = 16 * (1 + (int)(rnd() % 16)); }
          const int sup = bnn_hip_fconv_supported(rnd() % 16 ? &fd : nullptr);
          if (sup != 0 && sup != 1) broken("fconv_supported");
          bnn_hip_fconv_stage s1{pick_ptr<float>(), pick_ptr<float>(), pick_ptr<float>(), pick_ptr<float>()};
          bnn_hip_fconv_stage s2{pick_ptr<float>(), pick_ptr<float>(), pick_ptr<float>(), pick_ptr<float>()};
          const int sgs[] = {1, 1, 2, 4};
          float* fout = pick_ptr<float>();
          const float* fres = rnd() % 3 == 0 ? nullptr : rnd() % 4 == 0 ? fout : reinterpret_cast<const float*>(0x7fff0000fff0ull);
          const int sf = bnn_hip_fconv_fused(rnd() % 16 ? &fd : nullptr, pick_ptr<uint64_t>(), pick_ptr<uint64_t>(),
                                             pick_ptr<uint32_t>(), pick_ptr<uint32_t>(), rnd() % 16 ? &s1 : nullptr,
                                             pick_ptr<uint32_t>(), pick_ptr<uint32_t>(), rnd() % 16 ? &s2 : nullptr,
                                             pick_ptr<float>(), pick_ptr<float>(), rnd() % 8 ? sgs[rnd() % 4] : pick_int(), fres,
                                             fout, stream);
          if (!status_ok(sf)) broken("fconv status");
        }
        { // the route queries: the validator of bnn_hip_bconv2d_fused / _dot on a descriptor and an epilogue alone
          bnn_hip_epilogue e; std::memset(&e, 0, sizeof(e));
          e.alpha = pick_ptr<float>(); e.bn_scale = pick_ptr<float>(); e.bn_shift = pick_ptr<float>(); e.residual = pick_ptr<float>();
          e.relu = pick_int(); e.flags = (int)(rnd() % 8); e.out_f32 = pick_ptr<float>(); e.out_P = pick_ptr<uint64_t>();
          e.out_M = pick_ptr<uint64_t>(); e.out_c_offset = pick_int(); e.out_c_total = pick_int();
          e.sign_thresholds = pick_ptr<int32_t>();
          if (rnd() % 3 == 0) { e.sc_P = pick_ptr<uint64_t>(); e.sc_wbits = pick_ptr<uint32_t>(); e.sc_alpha = pick_ptr<float>();
                                e.sc_bn_scale = pick_ptr<float>(); e.sc_bn_shift = pick_ptr<float>(); e.sc_C = pick_int(); }
          bnn_hip_conv_route r; std::memset(&r, 0x5A, sizeof(r));
          const int sr = bnn_hip_bconv2d_route(rnd() % 16 ? &d : nullptr, rnd() % 4 ? &e : nullptr, rnd() % 16 ? &r : nullptr);
          if (!status_ok(sr)) broken("route status");
          if (sr == BNN_HIP_OK && (r.site < 0 || r.site >= BNN_HIP_ROUTE_SITES || r.waves <= 0)) broken("route of an accepted call");
          const int sd = bnn_hip_bconv2d_dot_route(rnd() % 16 ? &d : nullptr, rnd() % 16 ? &r : nullptr);
          if (!status_ok(sd)) broken("dot route status");
          digest = (digest ^ (uint64_t)(uint32_t)sr ^ ((uint64_t)(uint32_t)sd << 32)) * 0x100000001B3ull;
          // the int8 matrix-core convolution on the same descriptor and epilogue (csrc/bconv_mfma.hip)
          if (rnd() % 2) { d.KH = d.KW = 3; d.pad_h = d.pad_w = d.dil_h = d.dil_w = 1; d.stride_h = d.stride_w = 1 + (int)(rnd() % 2); }
          if (rnd() % 2) { d.C = 64 * (1 + (int)(rnd() % 8)); d.O = 64 * (1 + (int)(rnd() % 8)); }
          const bnn_hip_conv_desc* dp = rnd() % 16 ? &d : nullptr;
          const bnn_hip_epilogue* ep = rnd() % 16 ? &e : nullptr;
          const int sup = bnn_hip_bconv2d_mfma_supported(dp, ep);
          if (sup != 0 && sup != 1) broken("mfma supported");
          const int sm = bnn_hip_bconv2d_mfma_fused(dp, pick_ptr<uint64_t>(), pick_ptr<uint64_t>(), pick_ptr<char>(), ep, stream);
          if (!status_ok(sm) || (sm == BNN_HIP_OK && !sup)) broken("mfma conv launched where the query said no");
          if (bnn_hip_weight_i8_bytes(d.O, d.C, d.KH, d.KW) > ((size_t)1 << 62)) broken("int8 weight pack size");
          const int sp8 = bnn_hip_pack_weight_i8(pick_ptr<uint32_t>(), pick_ptr<uint32_t>(), d.O, d.C, d.KH, d.KW, pick_ptr<char>(), stream);
          if (!status_ok(sp8)) broken("int8 weight pack status");
          digest = (digest ^ (uint64_t)(uint32_t)sm ^ ((uint64_t)(uint32_t)sp8 << 32) ^ (uint64_t)sup) * 0x100000001B3ull;
          // and its folded-shortcut form
          const int fsup = bnn_hip_bconv2d_mfma_fold_supported(dp, ep);
          if (fsup != 0 && fsup != 1) broken("mfma fold supported");
          const int sf = bnn_hip_bconv2d_mfma_fold_fused(dp, pick_ptr<uint64_t>(), pick_ptr<uint64_t>(), pick_ptr<char>(),
                                                         pick_ptr<char>(), ep, stream);
          if (!status_ok(sf) || (sf == BNN_HIP_OK && !fsup)) broken("mfma fold launched where the query said no");
          const int sc_c = rnd() % 4 ? 64 << (rnd() % 3) : pick_int();
          if (bnn_hip_shortcut_weight_i8_bytes(d.O, sc_c) > ((size_t)1 << 62)) broken("int8 shortcut pack size");
          const int sps = bnn_hip_pack_shortcut_weight_i8(pick_ptr<uint32_t>(), d.O, sc_c, pick_ptr<char>(), stream);
          if (!status_ok(sps)) broken("int8 shortcut pack status");
          digest = (digest ^ (uint64_t)(uint32_t)sf ^ ((uint64_t)(uint32_t)sps << 32) ^ (uint64_t)fsup) * 0x100000001B3ull;
          // the FP4 forms of both: never wider than their int8 twins
          const int sup4 = bnn_hip_bconv2d_mfma4_supported(dp, ep), fsup4 = bnn_hip_bconv2d_mfma4_fold_supported(dp, ep);
          if ((sup4 != 0 && sup4 != 1) || (sup4 && !sup) || (fsup4 != 0 && fsup4 != 1) || (fsup4 && !fsup))
            broken("mfma4 supported");
          if ((sup4 || fsup4) && d.C % 128 != 0) broken("mfma4 took half a 128-channel group");
          const int sm4 = bnn_hip_bconv2d_mfma4_fused(dp, pick_ptr<uint64_t>(), pick_ptr<uint64_t>(), pick_ptr<char>(), ep, stream);
          if (!status_ok(sm4) || (sm4 == BNN_HIP_OK && !sup4)) broken("mfma4 conv launched where the query said no");
          const int sf4 = bnn_hip_bconv2d_mfma4_fold_fused(dp, pick_ptr<uint64_t>(), pick_ptr<uint64_t>(), pick_ptr<char>(),
                                                           pick_ptr<char>(), ep, stream);
          if (!status_ok(sf4) || (sf4 == BNN_HIP_OK && !fsup4)) broken("mfma4 fold launched where the query said no");
          const size_t b4 = bnn_hip_weight_f4_bytes(d.O, d.C, d.KH, d.KW);
          if (b4 != 0 && 2 * b4 != bnn_hip_weight_i8_bytes(d.O, d.C, d.KH, d.KW)) broken("FP4 weight pack size");
          const int sp4 = bnn_hip_pack_weight_f4(pick_ptr<uint32_t>(), pick_ptr<uint32_t>(), d.O, d.C, d.KH, d.KW, pick_ptr<char>(), stream);
          if (!status_ok(sp4)) broken("FP4 weight pack status");
          digest = (digest ^ (uint64_t)(uint32_t)sm4 ^ ((uint64_t)(uint32_t)sf4 << 32) ^ (uint64_t)(sup4 + 2 * fsup4 + 4 * sp4)) * 0x100000001B3ull;
          // the 1x1 form: a query and a launch that agree, a pack only where there is a size for it.  (Its picks replay
          // the generator from here: every other call of a run sees the arguments it saw before this block existed.)
          const uint64_t rng_here = g_rng;
          const int sup1 = bnn_hip_bconv1x1_mfma4_supported(dp, ep);
          if (sup1 != 0 && sup1 != 1) broken("mfma 1x1 supported");
          if (sup1 && (d.KH != 1 || d.KW != 1 || d.C % 128 != 0 || d.O % 64 != 0 || sup || fsup)) broken("mfma 1x1 took another shape");
          const int sm1 = bnn_hip_bconv1x1_mfma4_fused(dp, pick_ptr<uint64_t>(), pick_ptr<uint64_t>(), pick_ptr<char>(), ep, stream);
          if (!status_ok(sm1) || (sm1 == BNN_HIP_OK && !sup1)) broken("mfma 1x1 launched where the query said no");
          const size_t b1 = bnn_hip_weight1x1_f4_bytes(d.O, d.C);
          if (b1 != 0 && (2 * b1 != (size_t)d.O * (size_t)d.C || b4 != 0 && 9 * b1 != b4)) broken("FP4 1x1 weight pack size");
          const int sp1 = bnn_hip_pack_weight1x1_f4(pick_ptr<uint32_t>(), pick_ptr<uint32_t>(), d.O, d.C, d.KH, d.KW, pick_ptr<char>(), stream);
          if (!status_ok(sp1) || (sp1 == BNN_HIP_OK && (b1 == 0 || d.KH != 1 || d.KW != 1))) broken("FP4 1x1 weight pack status");
          digest = (digest ^ (uint64_t)(uint32_t)sm1 ^ ((uint64_t)(uint32_t)sp1 << 32) ^ (uint64_t)sup1) * 0x100000001B3ull;
          g_rng = rng_here;
        }
        st = bnn_hip_blinear(pick_int(), pick_int(), pick_int(), pick_ptr<uint64_t>(), pick_ptr<uint64_t>(), pick_ptr<uint32_t>(),
                             pick_ptr<uint32_t>(), pick_int(), pick_ptr<float>(), pick_ptr<float>(), pick_ptr<float>(),
                             pick_ptr<float>(), stream);
        { // the convolution with real weights (csrc/sconv.hip)
          const int O = pick_int(), C = pick_int(), ks = (int)(rnd() % 5);
          if (bnn_hip_sconv2d_weight_pack_bytes(O, C, ks) > ((size_t)1 << 40)) broken("sconv weight pack size");
          const int s1 = bnn_hip_sconv2d_pack_weight_f32(pick_ptr<float>(), O, C, ks, pick_ptr<char>(), stream);
          const int s2 = bnn_hip_sconv2d_f32(pick_ptr<float>(), pick_ptr<char>(), pick_ptr<float>(), pick_ptr<float>(),
                                             pick_ptr<float>(), pick_int(), pick_int(), pick_int(), pick_int(), pick_int(),
                                             (int)(rnd() % 5), (int)(rnd() % 4), stream);
          if (!status_ok(s1) || !status_ok(s2)) broken("sconv status");
          digest = (digest ^ (uint64_t)(uint32_t)s1 ^ ((uint64_t)(uint32_t)s2 << 32)) * 0x100000001B3ull;
        }
        { // the GEMM-shaped Linear entry points (csrc/blinear.hip)
          const int s1 = bnn_hip_blinear_direct(pick_int(), pick_int(), pick_int(), pick_ptr<float>(), (int)(rnd() % 3),
                                                pick_ptr<uint32_t>(), pick_ptr<uint32_t>(), pick_int(), pick_ptr<float>(),
                                                pick_ptr<float>(), pick_ptr<float>(), pick_ptr<float>(), pick_ptr<uint64_t>(),
                                                pick_ptr<uint64_t>(), pick_ptr<uint64_t>(), rnd() % 4 ? (int)(rnd() % 200) : pick_int(),
                                                stream);
          const int s2 = bnn_hip_blinear_grad_input_f32(pick_ptr<float>(), pick_ptr<float>(), pick_ptr<uint32_t>(),
                                                        pick_ptr<uint32_t>(), pick_ptr<uint64_t>(), pick_ptr<float>(), pick_int(),
                                                        pick_int(), pick_int(), stream);
          const int M = pick_int(), O = pick_int(), F = pick_int();
          const int sp = bnn_hip_blinear_grad_weight_splits(M, O, F);
          if (sp != BNN_HIP_ERR_INVALID_ARG && (sp < 1 || sp > M)) broken("default split of the Linear weight gradient");
          const int s3 = bnn_hip_blinear_grad_weight_f32(pick_ptr<float>(), pick_ptr<uint64_t>(), pick_ptr<uint64_t>(),
                                                         pick_ptr<float>(), rnd() % 2 ? sp : pick_int(), M, O, F, stream);
          if (!status_ok(s1) || !status_ok(s2) || !status_ok(s3)) broken("blinear status");
          digest = (digest ^ (uint64_t)(uint32_t)s1 ^ ((uint64_t)(uint32_t)s2 << 16) ^ ((uint64_t)(uint32_t)s3 << 32)) * 0x100000001B3ull;
        }
        { // the Linear with real weights and the mask kernel (csrc/slinear.hip)
          const int s1 = bnn_hip_slinear_f32(pick_int(), pick_int(), pick_int(), pick_ptr<float>(), pick_ptr<char>(),
                                             pick_ptr<float>(), pick_ptr<float>(), pick_ptr<float>(), pick_ptr<uint64_t>(),
                                             pick_ptr<uint64_t>(), pick_ptr<uint64_t>(), stream);
          const int s2 = bnn_hip_ste_mask_f32(pick_ptr<float>(), pick_ptr<uint64_t>(), pick_int(), pick_int(), stream);
          if (!status_ok(s1) || !status_ok(s2)) broken("slinear status");
          digest = (digest ^ (uint64_t)(uint32_t)s1 ^ ((uint64_t)(uint32_t)s2 << 32)) * 0x100000001B3ull;
        }
        break; }
    }
    if (!status_ok(st)) { std::fprintf(stderr, "unknown status %d\n", st); return 2; }
    digest = (digest ^ (uint64_t)(uint32_t)st) * 0x100000001B3ull;   // FNV-1a over the statuses, in call order
  }
  std::printf("CAPI_FUZZ_OK calls=%llu reached_launchers=%llu status_digest=%016" PRIx64 " launches=%" PRIu64 "\n", g_calls,
              g_reached, digest, bnn_hip_launch_count());
  return g_reached > g_calls / 200 ? 0 : 3;     // the fuzz must actually get past the validators often enough
}

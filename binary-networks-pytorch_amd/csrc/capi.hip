// capi.hip — the extern "C" boundary declared in include/bnn_hip.h.
// Argument validation, geometry, workspace carving and launch bookkeeping live here;
// kernels live in pack_act.hip / pack_weight.hip / bconv.hip.
#include <dlfcn.h>

#include <atomic>
#include <cstdlib>
#include <cstring>

#include "bnn_dev.h"

namespace {

std::atomic<uint64_t> g_launches{0};

// roctx ranges around every launching entry point (the reference's users profile with named ranges):
// off unless BNN_HIP_ROCTX=1 is in the environment when the first entry point runs.  The marker library is dlopen'ed —
// libbnn_hip.so has no link-time dependency on a profiler — and a box without it silently runs without ranges.
// rocprofv3 --marker-trace shows one range per C-ABI call, named after it.
struct Roctx {
  int (*push)(const char*) = nullptr;
  int (*pop)() = nullptr;
  Roctx() {
    const char* e = std::getenv("BNN_HIP_ROCTX");
    if (!e || e[0] != '1') return;
    for (const char* name : {"librocprofiler-sdk-roctx.so", "librocprofiler-sdk-roctx.so.1", "libroctx64.so", "libroctx64.so.4"}) {
      if (void* h = dlopen(name, RTLD_NOW | RTLD_GLOBAL)) {
        push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
        pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
        if (push && pop) return;
        push = nullptr; pop = nullptr;
      }
    }
  }
};
const Roctx& roctx() { static const Roctx r; return r; }
struct Range {
  bool on;
  explicit Range(const char* name) : on(roctx().push != nullptr) { if (on) roctx().push(name); }
  ~Range() { if (on) roctx().pop(); }
  Range(const Range&) = delete;
  Range& operator=(const Range&) = delete;
};
#define BNN_RANGE() Range bnn_range_(__func__)

inline bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

constexpr long long kMaxElems = (1LL << 31) - 1;
// the convolution kernels address every tensor as uniform base + 32-bit BYTE offset per lane: fp32 / int32 tensors
// of one launch stay below 2^30 elements, packed planes (uint64 per 64 channels per pixel) below 2^29 words
constexpr long long kMaxConvElems = (1LL << 30) - 1;
constexpr long long kMaxPlaneWords = (1LL << 29) - 1;
// tensors addressed through a sized 32-bit buffer descriptor (stem input / output, one-launch layer input): the
// out-of-range marker offsets the kernels use for dead lanes (0xFFFFFFF0 + small immediates) must stay out of range
constexpr long long kMaxDescBytes = 0xFFFFFE00LL;

// Size arithmetic on caller-supplied 32-bit integers: products of up to five of them.  Computed in 64 bits with
// saturation (all factors are checked positive first), so that a hostile descriptor cannot wrap a limit check
// (found by tools/fuzz/capi_fuzz.hip under UBSan: N * H * W * words overflowed `long long` for N = H = W = 2^24).
constexpr long long kSat = 1LL << 62;
inline long long mulc(long long a, long long b) { return (a <= 0 || b <= 0) ? 0 : (a > kSat / b ? kSat : a * b); }
inline long long mulc(long long a, long long b, long long c) { return mulc(mulc(a, b), c); }
inline long long mulc(long long a, long long b, long long c, long long d) { return mulc(mulc(a, b, c), d); }

// output extent of a convolution dimension, or 0 when it is empty / does not fit an int
int out_dim(int in, int k, int s, int p, int d) {
  const long long span = (long long)in + 2LL * p - (long long)d * (k - 1) - 1;
  if (span < 0) return 0;
  const long long o = span / s + 1;
  return o > 0x7fffffffLL ? 0 : (int)o;
}

int check_desc(const bnn_hip_conv_desc* d, int* Ho, int* Wo) {
  if (!d) return BNN_HIP_ERR_INVALID_ARG;
  if (d->N <= 0 || d->C <= 0 || d->H <= 0 || d->W <= 0 || d->O <= 0 || d->KH <= 0 || d->KW <= 0)
    return BNN_HIP_ERR_INVALID_ARG;
  if (d->stride_h <= 0 || d->stride_w <= 0 || d->pad_h < 0 || d->pad_w < 0 || d->dil_h <= 0 ||
      d->dil_w <= 0)
    return BNN_HIP_ERR_INVALID_ARG;
  // the 16-bit output store exists in the one-launch layer alone (bnn_hip_bconv2d_direct takes the bits out of the
  // descriptor it validates): every other entry point rejects them here
  if (d->flags & (BNN_HIP_FLAG_OUT_F16 | BNN_HIP_FLAG_OUT_BF16)) return BNN_HIP_ERR_INVALID_ARG;
  const int ho = out_dim(d->H, d->KH, d->stride_h, d->pad_h, d->dil_h);
  const int wo = out_dim(d->W, d->KW, d->stride_w, d->pad_w, d->dil_w);
  if (ho <= 0 || wo <= 0) return BNN_HIP_ERR_INVALID_ARG;
  if (mulc(d->N, d->H, d->W, ((long long)d->C + 63) / 64) > kMaxPlaneWords) return BNN_HIP_ERR_TOO_LARGE;
  if (mulc(d->N, ho, wo, ((long long)d->O + 63) / 64) > kMaxPlaneWords) return BNN_HIP_ERR_TOO_LARGE;
  if (mulc(d->N, d->O, ho, wo) > kMaxConvElems) return BNN_HIP_ERR_TOO_LARGE;
  // weight words of the layer (o_pad x taps x cw32) and the receptive field must be addressable too
  if (mulc(((long long)d->O + 31) / 32 * 32, d->KH, d->KW, 2 * (((long long)d->C + 63) / 64)) > kMaxElems)
    return BNN_HIP_ERR_TOO_LARGE;
  *Ho = ho;
  *Wo = wo;
  return BNN_HIP_OK;
}

// Geometry part of a ConvP from a descriptor that passed check_desc (which proved the dense weight layout in range)
// and the output extents it returned.  A caller that set no output-channel window (c_tot == 0) gets the whole output.
void fill_geometry(const bnn_hip_conv_desc* d, int Ho, int Wo, bnn::ConvP* p) {
  bnn_hip_wlayout L;
  bnn_hip_weight_layout(d->O, d->C, d->KH, d->KW, &L);
  p->N = d->N; p->H = d->H; p->Wd = d->W; p->Ho = Ho; p->Wo = Wo; p->O = d->O; p->C = d->C;
  p->KH = d->KH; p->KW = d->KW; p->sh = d->stride_h; p->sw = d->stride_w;
  p->ph = d->pad_h; p->pw = d->pad_w; p->dh = d->dil_h; p->dw = d->dil_w;
  p->cw32 = L.cw32; p->cwc = L.cwc; p->nchunk = L.nchunk;
  p->npix = d->N * Ho * Wo;
  if (p->c_tot == 0) { p->c_off = 0; p->c_tot = d->O; }
}

// The validator of every dense conv entry point (and of the route query): fills the geometry and operand part of `p`.
int check_conv(const bnn_hip_conv_desc* d, const uint64_t* P, const uint64_t* M, const uint32_t* wbits,
               const uint32_t* wnz, bnn::ConvP* pp) {
  bnn::ConvP& p = *pp;
  int Ho = 0, Wo = 0;
  const int st = check_desc(d, &Ho, &Wo);
  if (st != BNN_HIP_OK) return st;
  fill_geometry(d, Ho, Wo, &p);
  if (!P || !M || !wbits) return BNN_HIP_ERR_INVALID_ARG;
  if (!p.out && !(p.outP && p.outM)) return BNN_HIP_ERR_INVALID_ARG;
  if (!p.raw && !p.alpha) return BNN_HIP_ERR_INVALID_ARG;
  if ((p.bn_a == nullptr) != (p.bn_b == nullptr)) return BNN_HIP_ERR_INVALID_ARG;
  if ((p.outP == nullptr) != (p.outM == nullptr)) return BNN_HIP_ERR_INVALID_ARG;
  if ((p.pack_a == nullptr) != (p.pack_b == nullptr)) return BNN_HIP_ERR_INVALID_ARG;
  if (p.c_off < 0 || p.c_tot <= 0 || (long long)p.c_off + d->O > p.c_tot) return BNN_HIP_ERR_INVALID_ARG;
  if (mulc(d->N, p.c_tot, Ho, Wo) > kMaxConvElems) return BNN_HIP_ERR_TOO_LARGE;
  if ((d->flags & BNN_HIP_FLAG_WEIGHT_ZEROS) && !wnz) return BNN_HIP_ERR_INVALID_ARG;
  if (!aligned(P, 16) || !aligned(M, 16) || !aligned(wbits, 16)) return BNN_HIP_ERR_INVALID_ARG;
  if (p.outP && (!aligned(p.outP, 8) || !aligned(p.outM, 8))) return BNN_HIP_ERR_INVALID_ARG;
  p.P = reinterpret_cast<const uint32_t*>(P);
  p.M = reinterpret_cast<const uint32_t*>(M);
  p.W = wbits;
  p.Z = wnz;
  if (p.ds_P) {  // folded shortcut convolution (bnn_hip_epilogue sc_*)
    if (!p.ds_W || !p.ds_alpha || !p.ds_a || !p.ds_b || p.res || p.ds_C <= 0) return BNN_HIP_ERR_INVALID_ARG;
    if (!aligned(p.ds_P, 8) || !aligned(p.ds_W, 16)) return BNN_HIP_ERR_INVALID_ARG;
    if (!bnn::ds_fold_applies(p, d->flags)) return BNN_HIP_ERR_UNSUPPORTED;
    if (p.ds_inW > 0 && ((p.ds_inH + 1) / 2 != Ho || (p.ds_inW + 1) / 2 != Wo)) return BNN_HIP_ERR_INVALID_ARG;
    if (p.ds_inW > 0 && mulc(d->N, ((long long)p.ds_C + 63) / 64, p.ds_inH, p.ds_inW) > kMaxPlaneWords) return BNN_HIP_ERR_TOO_LARGE;
  }
  return BNN_HIP_OK;
}

// Shared tail of every conv entry point: validates, fills the geometry part of `p` and launches.
int run_conv(const bnn_hip_conv_desc* d, const uint64_t* P, const uint64_t* M, const uint32_t* wbits,
             const uint32_t* wnz, bnn::ConvP p, void* stream) {
  const int st = check_conv(d, P, M, wbits, wnz, &p);
  if (st != BNN_HIP_OK) return st;
  g_launches.fetch_add(1, std::memory_order_relaxed);
  Range range(p.raw ? "bnn_hip_bconv2d_dot" : p.ds_P ? "bnn_hip_bconv2d_fused+shortcut"
              : (p.bn_a || p.res || p.outP || p.relu || p.prelu) ? "bnn_hip_bconv2d_fused" : "bnn_hip_bconv2d");
  return bnn::launch_bconv(p, d->flags, static_cast<hipStream_t>(stream));
}

// Shared tail of the route queries: the same validator, then the launch ladder as a dry run.  The packed operands are
// not part of a query: an aligned host word stands in for them (never read — nothing is launched).
int route_conv(const bnn_hip_conv_desc* d, bnn::ConvP p, bnn_hip_conv_route* out) {
  alignas(16) static const uint64_t operand[2] = {0, 0};
  if (!out) return BNN_HIP_ERR_INVALID_ARG;
  const uint32_t* const w = reinterpret_cast<const uint32_t*>(operand);
  const int st = check_conv(d, operand, operand, w, w, &p);
  if (st != BNN_HIP_OK) return st;
  return bnn::launch_bconv(p, d->flags, nullptr, out, /*dry=*/true);
}

// Grouped convolutions (include/bnn_hip.h, bnn_hip_grouped_weight_layout): S = the most 32-bit activation words one
// 32-channel output block reads per tap.  Not a loop over every block (O may be ~2^30): block windows repeat.
//   Og < 32:  shifting a whole block by T blocks with 32 T = m Og, m = lcm(32 / gcd(32, Cg), 32 / gcd(32, Og)) <= 32,
//             moves both of its group bounds by m and its window by m Cg, a multiple of 32 channels: the same word count.
//             T = m Og / 32 < 32, so the first 33 blocks and the (possibly partial) last one cover every window.
//   Og >= 32: a block spans one group g or straddles g | g+1 (when (g+1) Og is not a multiple of 32).  Those windows
//             depend on g only through g Cg mod 32 and (g+1) Og mod 32 (period <= 32); a lone group's window is inside
//             the window of some block, so counting every one of them never exceeds the true maximum.
inline long long window_words(long long a, long long len) { return (a + len - 1) / 32 - a / 32 + 1; }
long long grouped_words_per_tap(long long O, long long C, long long G) {
  const long long Cg = C / G, Og = O / G, nb = (O + 31) / 32;
  long long S = 0;
  auto block = [&](long long ob) {
    const long long o0 = 32 * ob, o1 = (O < o0 + 32 ? O : o0 + 32) - 1;
    const long long glo = o0 / Og, ghi = o1 / Og;
    const long long w = window_words(glo * Cg, (ghi - glo + 1) * Cg);
    if (w > S) S = w;
  };
  if (Og < 32) {
    for (long long ob = 0; ob < nb && ob < 33; ++ob) block(ob);
    block(nb - 1);
  } else {
    for (long long g = 0; g < G && g < 64; ++g) {
      long long w = window_words(g * Cg, Cg);
      if (g + 1 < G && ((g + 1) * Og) % 32 != 0) w = window_words(g * Cg, 2 * Cg);
      if (w > S) S = w;
    }
  }
  return S;
}

bnn::ConvP empty_convp() {
  bnn::ConvP p;
  std::memset(&p, 0, sizeof(p));
  return p;
}

// The epilogue part of a ConvP from a bnn_hip_epilogue (bnn_hip_bconv2d_fused and its route query).
int epilogue_convp(const bnn_hip_epilogue* e, bnn::ConvP* pp) {
  if (!e) return BNN_HIP_ERR_INVALID_ARG;
  bnn::ConvP& p = *pp;
  p.alpha = e->alpha; p.bias = e->bias; p.scale = e->post_scale;
  p.bn_a = e->bn_scale; p.bn_b = e->bn_shift; p.res = e->residual; p.prelu = e->prelu;
  p.relu = e->relu != 0;
  p.out = e->out_f32;
  p.outP = reinterpret_cast<uint32_t*>(e->out_P);
  p.outM = reinterpret_cast<uint32_t*>(e->out_M);
  p.pack_a = e->pack_scale; p.pack_b = e->pack_shift;
  p.thr = e->sign_thresholds;
  if (p.thr && !aligned(p.thr, 4)) return BNN_HIP_ERR_INVALID_ARG;
  p.eflags = e->flags;
  p.c_off = e->out_c_offset; p.c_tot = e->out_c_total;
  if (e->sc_P || e->sc_wbits || e->sc_alpha || e->sc_bn_scale || e->sc_bn_shift) {
    if (!e->sc_P) return BNN_HIP_ERR_INVALID_ARG;
    p.ds_P = reinterpret_cast<const uint32_t*>(e->sc_P);
    p.ds_W = e->sc_wbits; p.ds_alpha = e->sc_alpha; p.ds_a = e->sc_bn_scale; p.ds_b = e->sc_bn_shift;
    p.ds_C = e->sc_C;
    if (e->sc_in_hw != 0) {      // un-pooled shortcut plane: (H << 16) | W of it; the kernel ORs the 2 x 2 windows
      p.ds_inH = (int)((uint32_t)e->sc_in_hw >> 16);
      p.ds_inW = (int)((uint32_t)e->sc_in_hw & 0xFFFFu);
      if (p.ds_inH <= 0 || p.ds_inW <= 0) return BNN_HIP_ERR_INVALID_ARG;
    }
  }
  return BNN_HIP_OK;
}

// A weight layout of `words` 32-bit words per output channel and tap, read in chunks of `cwc` words (which divides it).
int fill_layout(long long O, int KH, int KW, long long words, int cwc, bnn_hip_wlayout* out) {
  const long long o_pad = (O + BNN_HIP_OCB - 1) / BNN_HIP_OCB * BNN_HIP_OCB, taps = mulc(KH, KW);
  // the packed weight (one bit per weight) addresses words with 31-bit indices; taps and the padded channel count
  // are ints of the layout struct
  if (taps > 0x7fffffffLL || o_pad > 0x7fffffffLL || mulc(o_pad, taps, words) > kMaxElems) return BNN_HIP_ERR_TOO_LARGE;
  out->cw32 = (int32_t)words;
  out->cwc = cwc;
  out->nchunk = out->cw32 / cwc;
  out->taps = (int32_t)taps;
  out->o_pad = (int32_t)o_pad;
  out->reserved = 0;
  out->n_words = o_pad * taps * words;
  return BNN_HIP_OK;
}

// Entry contract of the plane-packing kernels (pack_act.hip, pack_ste.hip): fp32 or fp16 NCHW in (`x_align` = its
// element size), 8-byte plane words out, pixels indexed in 32 bits, one grid row per 64-channel word.
int check_pack(const void* x, size_t x_align, int N, int C, int H, int W, const uint64_t* P, const uint64_t* M) {
  if (!x || !P || !M || N <= 0 || C <= 0 || H <= 0 || W <= 0) return BNN_HIP_ERR_INVALID_ARG;
  if (mulc(N, H, W) > kMaxElems) return BNN_HIP_ERR_TOO_LARGE;
  if (((long long)C + 63) / 64 > 65535) return BNN_HIP_ERR_UNSUPPORTED;  // grid.y limit
  if (!aligned(P, 8) || !aligned(M, 8) || !aligned(x, x_align)) return BNN_HIP_ERR_INVALID_ARG;
  return BNN_HIP_OK;
}

// The two pixel lattices (2i, 2j) and (2i+1, 2j+1) of FactorizedReduce cover an image only when H and W are even.
int check_lattice(int H, int W) { return (H % 2 != 0 || W % 2 != 0) ? BNN_HIP_ERR_INVALID_ARG : BNN_HIP_OK; }

// A channel-slice view (bnn_hip_f32_view) of C channels: pointer, window, and the whole [N, c_total, H, W] tensor within
// `max_elems`.  *c_off / *c_tot receive the window with c_total == 0 resolved to C.
int check_view(const bnn_hip_f32_view* v, int N, int C, long long hw, long long max_elems, int* c_off, int* c_tot) {
  if (!v || !v->p || !aligned(v->p, 4) || v->c_offset < 0 || v->c_total < 0) return BNN_HIP_ERR_INVALID_ARG;
  const int tot = v->c_total == 0 ? C : v->c_total;
  if ((v->c_total == 0 && v->c_offset != 0) || (long long)v->c_offset + C > tot) return BNN_HIP_ERR_INVALID_ARG;
  if (mulc(N, tot, hw) > max_elems) return BNN_HIP_ERR_TOO_LARGE;
  *c_off = v->c_offset; *c_tot = tot;
  return BNN_HIP_OK;
}

// Whether the channel slices [ao, ao + C) of a [N, at, hw] tensor at `a` and [bo, bo + C) of a [N, bt, hw] tensor at `b`
// may share an element.  Disjoint: the whole tensors do not overlap, or they are ONE tensor (same base, same c_total)
// and the channel intervals are disjoint.  Anything else (two bases inside one allocation) counts as overlapping.
bool views_may_overlap(const void* a, int ao, int at, const void* b, int bo, int bt, int N, int C, long long hw) {
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  const uintptr_t na = (uintptr_t)mulc(N, at, hw) * 4, nb = (uintptr_t)mulc(N, bt, hw) * 4;
  if (pa + na <= pb || pb + nb <= pa) return false;
  if (pa == pb && at == bt) return ao < bo + C && bo < ao + C;
  return true;
}

// Output extent of the stem's convolution (7x7 / 2 / 3) along one dimension; of its MaxPool 3 / 2 / 1 too: apply twice.
inline long long stem_out(long long v) { return (v - 1) / 2 + 1; }
// The stem kernels address x and out through 32-bit buffer descriptors (range-checked loads are the zero padding,
// out-of-range stores are dropped): the input and the [N, 64, ho, wo] output of a launch stay below 2^32 - 512 bytes
// (4 GiB: ~7100 images of 224 x 224 in, ~5300 out) — larger batches are split by the caller (hipops.stem7x7 does)
bool stem_fits_descriptors(int N, int H, int W, long long ho, long long wo) {
  return mulc(N, 12, H, W) <= kMaxDescBytes && mulc(N, 256, ho, wo) <= kMaxDescBytes;
}
// The stem's weight gradient indexes x and dy [N, 64, hc, wc] by element, in 31 bits.
bool stem_wgrad_fits(int N, int H, int W) {
  return mulc(N, 3, H, W) <= kMaxElems && mulc(N, 64, stem_out(H), stem_out(W)) <= kMaxElems;
}

// H * W of an image as the int the BatchNorm entry points take, or 0 (which they reject) when it does not fit one
int checked_hw(int H, int W) { return (int)(mulc(H, W) > 0x7fffffffLL ? 0 : (long long)H * W); }

// Workspace of the training BatchNorm entry points (csrc/bn_train.hip) for (N, C, HW) that passed check_bn, carved
// from the caller's 8-byte aligned `base` when there is one: [C][splits][2] doubles of partial sums, rounded up to
// 256 bytes, then 3 C floats of per-channel coefficients.
struct BnWorkspace { int splits; size_t bytes; double* partial; float* work; };
BnWorkspace bn_workspace(int N, int C, int HW, void* base) {
  const int S = bnn::bn_train_splits(N, C, HW);
  const size_t partial_bytes = align_up((size_t)C * S * 2 * sizeof(double), 256);
  char* const b = static_cast<char*>(base);
  return {S, partial_bytes + (size_t)3 * C * sizeof(float), reinterpret_cast<double*>(b),
          b ? reinterpret_cast<float*>(b + partial_bytes) : nullptr};
}

// Entry contract of the grouped convolution kernels (csrc/bconv_grouped.hip), shared by bnn_hip_bconv2d_grouped and
// bnn_hip_bconv2d_grouped_fused: fills `p` (operands, epilogue constants, geometry) and *S, the words per tap of the
// windowed weight layout.  alpha == NULL asks for the raw dot and excludes the other epilogue constants.
int check_grouped(const bnn_hip_conv_desc* d, int groups, const uint64_t* P, const uint64_t* M, const uint32_t* wbits,
                  const uint32_t* wnz, const float* alpha, const float* bias, const float* post_scale, float* out,
                  bnn::ConvP* p, int* S) {
  int Ho = 0, Wo = 0;
  const int st = check_desc(d, &Ho, &Wo);
  if (st != BNN_HIP_OK) return st;
  if (groups <= 0 || d->C % groups != 0 || d->O % groups != 0) return BNN_HIP_ERR_INVALID_ARG;
  if (!P || !M || !wbits || !wnz || !out) return BNN_HIP_ERR_INVALID_ARG;
  if (!alpha && (bias || post_scale)) return BNN_HIP_ERR_INVALID_ARG;  // raw dot: no epilogue constants
  if (!aligned(P, 16) || !aligned(M, 16) || !aligned(wbits, 16) || !aligned(wnz, 16) || !aligned(out, 4))
    return BNN_HIP_ERR_INVALID_ARG;
  bnn_hip_wlayout G;
  const int sg = bnn_hip_grouped_weight_layout(d->O, d->C, groups, d->KH, d->KW, &G);
  if (sg != BNN_HIP_OK) return sg;
  p->alpha = alpha; p->bias = bias; p->scale = post_scale; p->out = out; p->raw = alpha == nullptr;
  p->P = reinterpret_cast<const uint32_t*>(P);
  p->M = reinterpret_cast<const uint32_t*>(M);
  p->W = wbits;
  p->Z = wnz;
  fill_geometry(d, Ho, Wo, p);            // cw32: the activation words per pixel, as for a dense weight
  p->cwc = p->cw32; p->nchunk = 1;        // (one chunk: the grouped kernel walks its window, not chunks)
  *S = G.cw32;
  return BNN_HIP_OK;
}

// Sizes of a FactorizedConv descriptor (csrc/fconv.hip): positive extents, a stride, and every tensor of the launch
// inside the convolution kernels' 32-bit byte offsets.  What the kernel covers beyond that is bnn::fconv_supported().
int check_fconv_desc(const bnn_hip_fconv_desc* d) {
  if (d->N <= 0 || d->C <= 0 || d->H <= 0 || d->W <= 0 || d->K <= 0 || d->stride <= 0) return BNN_HIP_ERR_INVALID_ARG;
  const long long cw64 = ((long long)d->C + 63) / 64;
  const long long Ho = ((long long)d->H - 1) / d->stride + 1, Wo = ((long long)d->W - 1) / d->stride + 1;
  if (mulc(d->N, d->H, d->W, cw64) > kMaxPlaneWords) return BNN_HIP_ERR_TOO_LARGE;
  if (mulc(d->N, d->C, Ho, Wo) > kMaxConvElems) return BNN_HIP_ERR_TOO_LARGE;
  if (mulc(((long long)d->C + 31) / 32 * 32, d->K, 2 * cw64) > kMaxElems) return BNN_HIP_ERR_TOO_LARGE;
  return BNN_HIP_OK;
}

}  // namespace

extern "C" {

int bnn_hip_abi_version(void) { return BNN_HIP_ABI_VERSION; }

const char* bnn_hip_status_string(int status) {
  switch (status) {
    case BNN_HIP_OK: return "ok";
    case BNN_HIP_ERR_INVALID_ARG: return "invalid argument (null/misaligned pointer or non-positive size)";
    case BNN_HIP_ERR_UNSUPPORTED: return "unsupported shape";
    case BNN_HIP_ERR_LAUNCH: return "HIP kernel launch failed";
    case BNN_HIP_ERR_TOO_LARGE: return "tensor exceeds 2^31-1 elements per launch; split the batch";
    case BNN_HIP_ERR_NO_DEVICE: return "no usable HIP device";
    default: return "unknown status";
  }
}

uint64_t bnn_hip_launch_count(void) { return g_launches.load(std::memory_order_relaxed); }

int bnn_hip_device_info(int device, bnn_hip_devinfo* out) {
  if (!out) return BNN_HIP_ERR_INVALID_ARG;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return BNN_HIP_ERR_NO_DEVICE;
  std::memset(out, 0, sizeof(*out));
  std::strncpy(out->name, prop.name, sizeof(out->name) - 1);
  std::strncpy(out->arch, prop.gcnArchName, sizeof(out->arch) - 1);
  out->compute_units = prop.multiProcessorCount;
  out->clock_khz = prop.clockRate;
  out->mem_clock_khz = prop.memoryClockRate;
  out->mem_bus_bits = prop.memoryBusWidth;
  out->wavefront = prop.warpSize;
  out->lds_bytes_per_block = (int32_t)prop.sharedMemPerBlock;
  out->total_mem_bytes = (int64_t)prop.totalGlobalMem;
  out->l2_bytes = prop.l2CacheSize;
  return BNN_HIP_OK;
}

int bnn_hip_act_words(int C) { return C > 0 ? (int)(((long long)C + 63) / 64) : BNN_HIP_ERR_INVALID_ARG; }

int bnn_hip_weight_layout(int O, int C, int KH, int KW, bnn_hip_wlayout* out) {
  if (!out || O <= 0 || C <= 0 || KH <= 0 || KW <= 0) return BNN_HIP_ERR_INVALID_ARG;
  const int cw32 = (int)(2 * (((long long)C + 63) / 64));
  return fill_layout(O, KH, KW, cw32, bnn::choose_cwc(cw32, KH, KW), out);
}

int bnn_hip_pack_act_f32(const float* x, int N, int C, int H, int W, uint64_t* P, uint64_t* M,
                         void* stream) {
  const int st = check_pack(x, 4, N, C, H, W, P, M);
  if (st != BNN_HIP_OK) return st;
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_pack_act(x, N, C, H, W, P, M, static_cast<hipStream_t>(stream));
}

int bnn_hip_pack_act_f16(const void* x, int N, int C, int H, int W, uint64_t* P, uint64_t* M,
                         void* stream) {
  const int st = check_pack(x, 2, N, C, H, W, P, M);
  if (st != BNN_HIP_OK) return st;
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_pack_act_f16(x, N, C, H, W, P, M, static_cast<hipStream_t>(stream));
}

int bnn_hip_pack_act_bf16(const void* x, int N, int C, int H, int W, uint64_t* P, uint64_t* M,
                          void* stream) {
  const int st = check_pack(x, 2, N, C, H, W, P, M);
  if (st != BNN_HIP_OK) return st;
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_pack_act_bf16(x, N, C, H, W, P, M, static_cast<hipStream_t>(stream));
}

int bnn_hip_bn_act_pack_f32(const float* x, int N, int C, int H, int W, const float* bn_scale,
                            const float* bn_shift, int relu, uint64_t* P, uint64_t* M, void* stream) {
  if ((bn_scale == nullptr) != (bn_shift == nullptr)) return BNN_HIP_ERR_INVALID_ARG;
  const int st = check_pack(x, 4, N, C, H, W, P, M);
  if (st != BNN_HIP_OK) return st;
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_bn_act_pack(x, N, C, H, W, bn_scale, bn_shift, relu, P, M,
                                 static_cast<hipStream_t>(stream));
}

int bnn_hip_bn_act_pack_multi_f32(const bnn_hip_f32_view* x, int N, int C, int H, int W, int K, const float* scale,
                                  const float* shift, int relu, uint64_t* P, uint64_t* M, void* stream) {
  if (!x || K < 1 || K > 4 || !scale || !shift) return BNN_HIP_ERR_INVALID_ARG;
  const int st = check_pack(x->p, 4, N, C, H, W, P, M);
  if (st != BNN_HIP_OK) return st;
  int c_off = 0, c_tot = 0;
  const int sv = check_view(x, N, C, mulc(H, W), kSat, &c_off, &c_tot);   // (the kernel indexes x in 64 bits)
  if (sv != BNN_HIP_OK) return sv;
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_bn_act_pack_multi(x->p, c_off, c_tot, N, C, H, W, K, scale, shift, relu, P, M,
                                       static_cast<hipStream_t>(stream));
}

int bnn_hip_bn_act_pack_s2_f32(const bnn_hip_f32_view* x, int N, int C, int H, int W, const float* bn_scale,
                               const float* bn_shift, int relu, uint64_t* P, uint64_t* M, void* stream) {
  if (!x || (bn_scale == nullptr) != (bn_shift == nullptr)) return BNN_HIP_ERR_INVALID_ARG;
  const int st = check_pack(x->p, 4, N, C, H, W, P, M);
  if (st != BNN_HIP_OK) return st;
  if (check_lattice(H, W) != BNN_HIP_OK) return BNN_HIP_ERR_INVALID_ARG;
  int c_off = 0, c_tot = 0;
  const int sv = check_view(x, N, C, mulc(H, W), kSat, &c_off, &c_tot);
  if (sv != BNN_HIP_OK) return sv;
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_bn_act_pack_s2(x->p, c_off, c_tot, N, C, H, W, bn_scale, bn_shift, relu, P, M,
                                    static_cast<hipStream_t>(stream));
}

int bnn_hip_stem3x3_bn_relu_pack_f32(const float* x, const float* w, const float* bn_scale, const float* bn_shift,
                                     const float* pack_scale, const float* pack_shift, int N, int O, int H, int W, int K,
                                     uint64_t* P, uint64_t* M, float* y, void* stream) {
  if (!w || !bn_scale || !bn_shift || !pack_scale || !pack_shift || K < 1 || K > 4) return BNN_HIP_ERR_INVALID_ARG;
  const int st = check_pack(x, 4, N, O, H, W, P, M);     // (the planes are those of the O output channels)
  if (st != BNN_HIP_OK) return st;
  if (mulc(N, O, H, W) > kMaxElems || mulc(N, 3, H, W) > kMaxElems) return BNN_HIP_ERR_TOO_LARGE;
  if (!aligned(w, 4) || !aligned(bn_scale, 4) || !aligned(bn_shift, 4) || !aligned(pack_scale, 4) ||
      !aligned(pack_shift, 4) || (y && !aligned(y, 4)))
    return BNN_HIP_ERR_INVALID_ARG;
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_stem3x3_bn_relu_pack(x, w, bn_scale, bn_shift, pack_scale, pack_shift, N, O, H, W, K, P, M, y,
                                          static_cast<hipStream_t>(stream));
}

int bnn_hip_stem_s2x2_f32(const float* x, const float* w1, const float* s1, const float* t1, const float* w2,
                          const float* s2, const float* t2, int N, int C1, int C, int G, int H, int W, int relu_out,
                          float* y, void* stream) {
  if (!x || !w1 || !s1 || !t1 || !w2 || !s2 || !t2 || !y) return BNN_HIP_ERR_INVALID_ARG;
  if (N <= 0 || C1 <= 0 || C <= 0 || G <= 0 || H <= 0 || W <= 0) return BNN_HIP_ERR_INVALID_ARG;
  if (C1 % G != 0 || C % G != 0) return BNN_HIP_ERR_INVALID_ARG;
  if (!aligned(x, 4) || !aligned(w1, 4) || !aligned(s1, 4) || !aligned(t1, 4) || !aligned(w2, 4) || !aligned(s2, 4) ||
      !aligned(t2, 4) || !aligned(y, 4))
    return BNN_HIP_ERR_INVALID_ARG;
  const int H2 = out_dim(out_dim(H, 3, 2, 1, 1), 3, 2, 1, 1), W2 = out_dim(out_dim(W, 3, 2, 1, 1), 3, 2, 1, 1);
  if (mulc(N, 3, H, W) > kMaxElems || mulc(N, C, H2, W2) > kMaxElems || mulc(C, C1 / G, 9) > kMaxElems ||
      mulc(C1, 27) > kMaxElems)
    return BNN_HIP_ERR_TOO_LARGE;
  if (C1 / G > BNN_HIP_STEM_S2X2_MAX_GROUP_CHANNELS || G > 65535) return BNN_HIP_ERR_UNSUPPORTED;   // LDS tile, grid.y
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_stem_s2x2(x, w1, s1, t1, w2, s2, t2, N, C1, C, G, H, W, relu_out != 0, y,
                               static_cast<hipStream_t>(stream));
}

int bnn_hip_gconv3x3s2_bn_pack_f32(const float* x, const float* w, const float* bn_scale, const float* bn_shift,
                                   const float* pack_scale, const float* pack_shift, int N, int C, int O, int G, int H,
                                   int W, int relu_in, int K, uint64_t* P, uint64_t* M, float* y, void* stream) {
  if (!x || !w || !bn_scale || !bn_shift || K < 0 || K > 4) return BNN_HIP_ERR_INVALID_ARG;
  if (K == 0 ? !y : (!pack_scale || !pack_shift || !P || !M)) return BNN_HIP_ERR_INVALID_ARG;
  if (N <= 0 || C <= 0 || O <= 0 || G <= 0 || H <= 0 || W <= 0) return BNN_HIP_ERR_INVALID_ARG;
  if (C % G != 0 || O % G != 0) return BNN_HIP_ERR_INVALID_ARG;
  if (!aligned(x, 4) || !aligned(w, 4) || !aligned(bn_scale, 4) || !aligned(bn_shift, 4) || (y && !aligned(y, 4)))
    return BNN_HIP_ERR_INVALID_ARG;
  if (K > 0 && (!aligned(pack_scale, 4) || !aligned(pack_shift, 4) || !aligned(P, 8) || !aligned(M, 8)))
    return BNN_HIP_ERR_INVALID_ARG;
  const int Ho = out_dim(H, 3, 2, 1, 1), Wo = out_dim(W, 3, 2, 1, 1);
  if (mulc(N, C, H, W) > kMaxElems || mulc(N, O, Ho, Wo) > kMaxElems || mulc(O, C / G, 9) > kMaxElems)
    return BNN_HIP_ERR_TOO_LARGE;
  if (C / G > BNN_HIP_GCONV3X3S2_MAX_GROUP_CHANNELS || ((long long)O + 63) / 64 > 65535)   // LDS tile, grid.y
    return BNN_HIP_ERR_UNSUPPORTED;
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_gconv3x3s2_bn_pack(x, w, bn_scale, bn_shift, K ? pack_scale : nullptr, K ? pack_shift : nullptr, N, C, O,
                                        G, H, W, relu_in != 0, K, K ? P : nullptr, K ? M : nullptr, y,
                                        static_cast<hipStream_t>(stream));
}

int bnn_hip_avgpool_pack_f32(const float* x, int N, int C, int H, int W, int k, uint64_t* P,
                             uint64_t* M, void* stream) {
  if (!x || !P || !M || N <= 0 || C <= 0 || H <= 0 || W <= 0 || k <= 0) return BNN_HIP_ERR_INVALID_ARG;
  if (mulc(N, H, W) > kMaxElems) return BNN_HIP_ERR_TOO_LARGE;
  if (2 * (((long long)C + 63) / 64) > 65535) return BNN_HIP_ERR_UNSUPPORTED;
  if (!aligned(P, 8) || !aligned(M, 8)) return BNN_HIP_ERR_INVALID_ARG;
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_avgpool_pack(x, N, C, H, W, k, P, M, static_cast<hipStream_t>(stream));
}

int bnn_hip_avgpool2_bn_pack2_f32(const float* x, int N, int C, int H, int W, const float* a1, const float* b1, int relu1,
                                  uint64_t* P1, uint64_t* M1, const float* a2, const float* b2, int relu2, uint64_t* P2,
                                  uint64_t* M2, float* out_f32, void* stream) {
  if (!x || !a1 || !b1 || !P1 || !M1 || N <= 0 || C <= 0 || H <= 0 || W <= 0) return BNN_HIP_ERR_INVALID_ARG;
  if (H % 2 || W % 2) return BNN_HIP_ERR_UNSUPPORTED;
  if ((a2 == nullptr) != (b2 == nullptr) || (a2 && (!P2 || !M2))) return BNN_HIP_ERR_INVALID_ARG;
  if (mulc(N, C, H, W) > kMaxElems) return BNN_HIP_ERR_TOO_LARGE;
  if (2 * (((long long)C + 63) / 64) > 65535) return BNN_HIP_ERR_UNSUPPORTED;
  if (!aligned(x, 8) || !aligned(P1, 8) || !aligned(M1, 8) || (a2 && (!aligned(P2, 8) || !aligned(M2, 8))) ||
      (out_f32 && !aligned(out_f32, 4)))
    return BNN_HIP_ERR_INVALID_ARG;
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_avgpool2_bn_pack2(x, N, C, H, W, a1, b1, relu1, P1, M1, a2, b2, relu2, P2, M2, out_f32,
                                       static_cast<hipStream_t>(stream));
}

int bnn_hip_orpool_packed(const uint64_t* P, int N, int C, int H, int W, int k, uint64_t* out_P,
                          uint64_t* out_M, void* stream) {
  if (!P || !out_P || !out_M || N <= 0 || C <= 0 || H <= 0 || W <= 0 || k <= 0) return BNN_HIP_ERR_INVALID_ARG;
  if (mulc(N, ((long long)C + 63) / 64, H, W) > kMaxElems) return BNN_HIP_ERR_TOO_LARGE;
  if (!aligned(P, 8) || !aligned(out_P, 8) || !aligned(out_M, 8)) return BNN_HIP_ERR_INVALID_ARG;
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_orpool_packed(P, N, C, H, W, k, out_P, out_M, static_cast<hipStream_t>(stream));
}

int bnn_hip_bn_relu_maxpool_pack_f32(const float* x, int N, int C, int H, int W,
                                     const float* bn_scale, const float* bn_shift, int relu, int k,
                                     int stride, int pad, float* out_f32, uint64_t* P, uint64_t* M,
                                     void* stream) {
  if (!x || N <= 0 || C <= 0 || H <= 0 || W <= 0 || k <= 0 || stride <= 0 || pad < 0)
    return BNN_HIP_ERR_INVALID_ARG;
  if (!out_f32 && !P) return BNN_HIP_ERR_INVALID_ARG;
  if ((P == nullptr) != (M == nullptr)) return BNN_HIP_ERR_INVALID_ARG;
  if ((bn_scale == nullptr) != (bn_shift == nullptr)) return BNN_HIP_ERR_INVALID_ARG;
  if (2LL * pad > k || (long long)H + 2LL * pad < k || (long long)W + 2LL * pad < k) return BNN_HIP_ERR_INVALID_ARG;
  if (mulc(N, C, H, W) > 4 * kMaxElems) return BNN_HIP_ERR_TOO_LARGE;
  if (P && (!aligned(P, 8) || !aligned(M, 8))) return BNN_HIP_ERR_INVALID_ARG;
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_bn_relu_maxpool_pack(x, N, C, H, W, bn_scale, bn_shift, relu, k, stride, pad,
                                          out_f32, P, M, static_cast<hipStream_t>(stream));
}

int bnn_hip_stem7x7_bn_relu_pool_pack_f32(const float* x, const float* w, const float* bn_scale,
                                          const float* bn_shift, int N, int H, int W, int flags,
                                          float* out_f32, uint64_t* P, uint64_t* M, void* stream) {
  if (!x || !w || !bn_scale || !bn_shift || N <= 0 || H <= 0 || W <= 0) return BNN_HIP_ERR_INVALID_ARG;
  if (!out_f32 && !P) return BNN_HIP_ERR_INVALID_ARG;
  if (flags & ~(BNN_HIP_STEM_EXACT_FP32 | BNN_HIP_STEM_FP16)) return BNN_HIP_ERR_INVALID_ARG;
  if ((flags & BNN_HIP_STEM_EXACT_FP32) && (flags & BNN_HIP_STEM_FP16)) return BNN_HIP_ERR_INVALID_ARG;
  if ((P == nullptr) != (M == nullptr)) return BNN_HIP_ERR_INVALID_ARG;
  if (P && (!aligned(P, 8) || !aligned(M, 8))) return BNN_HIP_ERR_INVALID_ARG;
  if (!stem_fits_descriptors(N, H, W, stem_out(stem_out(H)), stem_out(stem_out(W)))) return BNN_HIP_ERR_TOO_LARGE;
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_stem(x, w, bn_scale, bn_shift, N, H, W, flags, out_f32, P, M,
                          static_cast<hipStream_t>(stream));
}

int bnn_hip_stem7x7_bn_relu_pool_pack_affine_f32(const float* x, const float* w, const float* bn_scale,
                                                 const float* bn_shift, const float* pack_scale, const float* pack_shift,
                                                 int N, int H, int W, int flags, float* out_f32, uint64_t* P, uint64_t* M,
                                                 void* stream) {
  if (!x || !w || !bn_scale || !bn_shift || !pack_scale || !pack_shift || !P || !M || N <= 0 || H <= 0 || W <= 0)
    return BNN_HIP_ERR_INVALID_ARG;
  if (flags & ~BNN_HIP_STEM_FP16) return BNN_HIP_ERR_INVALID_ARG;   // (the exact-fp32 stem has no such variant)
  if (!aligned(P, 8) || !aligned(M, 8)) return BNN_HIP_ERR_INVALID_ARG;
  if (!stem_fits_descriptors(N, H, W, stem_out(stem_out(H)), stem_out(stem_out(W)))) return BNN_HIP_ERR_TOO_LARGE;
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_stem_rows_aff(x, w, bn_scale, bn_shift, pack_scale, pack_shift, N, H, W, (flags & BNN_HIP_STEM_FP16) != 0,
                                   out_f32, P, M, static_cast<hipStream_t>(stream));
}

int bnn_hip_stem7x7_conv_f32(const float* x, const float* w, int N, int H, int W, int flags, float* out,
                             void* stream) {
  if (!x || !w || !out || N <= 0 || H <= 0 || W <= 0) return BNN_HIP_ERR_INVALID_ARG;
  if (flags & ~BNN_HIP_STEM_FP16) return BNN_HIP_ERR_INVALID_ARG;
  if (!aligned(x, 4) || !aligned(w, 4) || !aligned(out, 4)) return BNN_HIP_ERR_INVALID_ARG;
  if (!stem_fits_descriptors(N, H, W, stem_out(H), stem_out(W))) return BNN_HIP_ERR_TOO_LARGE;   // (no pooling here)
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_stem_conv(x, w, N, H, W, (flags & BNN_HIP_STEM_FP16) != 0, out, static_cast<hipStream_t>(stream));
}

int bnn_hip_avgpool2x2_backward_f32(const float* gy, int N, int C, int Ho, int Wo, float* gx, void* stream) {
  if (!gy || !gx || N <= 0 || C <= 0 || Ho <= 0 || Wo <= 0) return BNN_HIP_ERR_INVALID_ARG;
  if (!aligned(gy, 4) || !aligned(gx, 4)) return BNN_HIP_ERR_INVALID_ARG;
  if (mulc(N, C, Ho, Wo) > kMaxElems / 4) return BNN_HIP_ERR_TOO_LARGE;   // gx holds four times as many elements
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_avgpool2x2_bwd(gy, N, C, Ho, Wo, gx, static_cast<hipStream_t>(stream));
}

size_t bnn_hip_stem7x7_wgrad_workspace_bytes(int N, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0 || !stem_wgrad_fits(N, H, W)) return 0;
  return bnn::stem_wgrad_workspace_bytes(N, H, W);
}

int bnn_hip_stem7x7_wgrad_f32(const float* x, const float* dy, int N, int H, int W, float* workspace,
                              size_t workspace_bytes, float* dw, void* stream) {
  if (!x || !dy || !dw || !workspace || N <= 0 || H <= 0 || W <= 0) return BNN_HIP_ERR_INVALID_ARG;
  if (!aligned(x, 4) || !aligned(dy, 4) || !aligned(dw, 4) || !aligned(workspace, 4)) return BNN_HIP_ERR_INVALID_ARG;
  if (!stem_wgrad_fits(N, H, W)) return BNN_HIP_ERR_TOO_LARGE;
  if (!bnn::stem_wgrad_supported(H, W)) return BNN_HIP_ERR_UNSUPPORTED;
  if (workspace_bytes < bnn::stem_wgrad_workspace_bytes(N, H, W)) return BNN_HIP_ERR_INVALID_ARG;
  g_launches.fetch_add(2, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_stem_wgrad(x, dy, N, H, W, workspace, dw, static_cast<hipStream_t>(stream));
}

// What both forms of the head (avgpool + fc, csrc/tail.hip) ask of x [N, C, HW], w_t [C, O] and out [N, O].
static int check_head(const float* x, int N, int C, int HW, const float* w_t, int O, const float* out) {
  if (!x || !w_t || !out || N <= 0 || C <= 0 || HW <= 0 || O <= 0) return BNN_HIP_ERR_INVALID_ARG;
  if (!aligned(x, 4) || !aligned(w_t, 4) || !aligned(out, 4)) return BNN_HIP_ERR_INVALID_ARG;
  if (mulc(N, C, HW) > 4 * kMaxElems || mulc(N, O) > kMaxElems) return BNN_HIP_ERR_TOO_LARGE;
  return BNN_HIP_OK;
}

int bnn_hip_avgpool_fc_f32(const float* x, int N, int C, int HW, const float* w_t, const float* bias, int O,
                           float* out, void* stream) {
  const int st = check_head(x, N, C, HW, w_t, O, out);
  if (st != BNN_HIP_OK) return st;
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_avgpool_fc(x, w_t, bias, out, N, C, HW, O, static_cast<hipStream_t>(stream));
}

size_t bnn_hip_avgpool_fc_workspace_bytes(int N, int C) {
  if (N <= 0 || C <= 0) return 0;
  return bnn::avgpool_fc_workspace_bytes(N, C);
}

int bnn_hip_avgpool_fc_ws_f32(const float* x, int N, int C, int HW, const float* w_t, const float* bias, int O,
                              float* out, void* workspace, size_t workspace_bytes, void* stream) {
  const int st = check_head(x, N, C, HW, w_t, O, out);
  if (st != BNN_HIP_OK) return st;
  const bool two = bnn::avgpool_fc_ws_supported(C, HW);  // else the one-kernel form, which needs no workspace
  if (two && (!workspace || !aligned(workspace, 16) || workspace_bytes < bnn::avgpool_fc_workspace_bytes(N, C)))
    return BNN_HIP_ERR_INVALID_ARG;
  g_launches.fetch_add(two ? 2 : 1, std::memory_order_relaxed);
  BNN_RANGE();
  if (!two) return bnn::launch_avgpool_fc(x, w_t, bias, out, N, C, HW, O, static_cast<hipStream_t>(stream));
  return bnn::launch_avgpool_fc_ws(x, w_t, bias, out, static_cast<float*>(workspace), N, C, HW, O,
                                   static_cast<hipStream_t>(stream));
}

static bool grad_ks_ok(int ksize) { return ksize == 1 || ksize == 3; }

size_t bnn_hip_grad_weight_pack_bytes(int O, int C, int ksize) {
  return (O > 0 && C > 0 && grad_ks_ok(ksize)) ? bnn::grad_weight_pack_bytes(O, C, ksize) : 0;
}

int bnn_hip_grad_pack_weight_f32(const float* w_hat, int O, int C, int ksize, void* packed, float* alpha,
                                 void* stream) {
  if (!w_hat || !packed || !alpha || O <= 0 || C <= 0) return BNN_HIP_ERR_INVALID_ARG;
  if (!grad_ks_ok(ksize)) return BNN_HIP_ERR_UNSUPPORTED;
  if (!aligned(packed, 16)) return BNN_HIP_ERR_INVALID_ARG;
  g_launches.fetch_add(2, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_grad_pack_weight(w_hat, O, C, ksize, packed, alpha, static_cast<hipStream_t>(stream));
}

static int check_grad_shape(int N, int O, int C, int H, int W, int ksize, int stride) {
  if (N <= 0 || O <= 0 || C <= 0 || H <= 0 || W <= 0) return BNN_HIP_ERR_INVALID_ARG;
  if (!grad_ks_ok(ksize) || (stride != 1 && stride != 2) || (ksize == 1 && stride != 1)) return BNN_HIP_ERR_UNSUPPORTED;
  if (W > 64) return BNN_HIP_ERR_UNSUPPORTED;
  if (mulc(N, O, H, W) > kMaxElems || mulc(N, C, H, W) > kMaxElems) return BNN_HIP_ERR_TOO_LARGE;
  return BNN_HIP_OK;
}

int bnn_hip_bconv_grad_input_f32(const float* g, const float* alpha, const void* packed, const float* x, float* gx,
                                 int N, int O, int C, int H, int W, int ksize, int stride, void* stream) {
  if (!g || !alpha || !packed || !x || !gx) return BNN_HIP_ERR_INVALID_ARG;
  const int st = check_grad_shape(N, O, C, H, W, ksize, stride);
  if (st != BNN_HIP_OK) return st;
  if (!aligned(packed, 16) || !aligned(x, 4) || !aligned(g, 4) || !aligned(gx, 4)) return BNN_HIP_ERR_INVALID_ARG;
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_dgrad(g, alpha, packed, x, 0, gx, N, O, C, H, W, ksize, stride, static_cast<hipStream_t>(stream));
}

int bnn_hip_bconv_grad_input_packed_f32(const float* g, const float* alpha, const void* packed, const uint64_t* T,
                                        float* gx, int N, int O, int C, int H, int W, int ksize, int stride,
                                        void* stream) {
  if (!g || !alpha || !packed || !T || !gx) return BNN_HIP_ERR_INVALID_ARG;
  const int st = check_grad_shape(N, O, C, H, W, ksize, stride);
  if (st != BNN_HIP_OK) return st;
  if (!aligned(packed, 16) || !aligned(T, 8) || !aligned(g, 4) || !aligned(gx, 4)) return BNN_HIP_ERR_INVALID_ARG;
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_dgrad(g, alpha, packed, T, 1, gx, N, O, C, H, W, ksize, stride, static_cast<hipStream_t>(stream));
}

// Entry contract of the real-weight convolution (csrc/sconv.hip): the geometry of check_grad_shape (3x3 / stride 1 or 2
// and 1x1 / stride 1, input rows of at most 64 pixels), and x [N,C,H,W] and y [N,O,Ho,Wo] inside the 32-bit range of a
// sized buffer descriptor (kMaxDescBytes).
static int check_sconv_shape(int N, int O, int C, int H, int W, int ksize, int stride) {
  const int st = check_grad_shape(N, O, C, H, W, ksize, stride);
  if (st != BNN_HIP_OK) return st;
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  if (mulc(mulc(N, C, H, W), 4) > kMaxDescBytes || mulc(mulc(N, O, Ho, Wo), 4) > kMaxDescBytes) return BNN_HIP_ERR_TOO_LARGE;
  return BNN_HIP_OK;
}

// fragments of the packed weight stay addressable by a 32-bit element index (as the other weight layouts)
static int check_sconv_weight(int O, int C, int ksize) {
  if (O <= 0 || C <= 0) return BNN_HIP_ERR_INVALID_ARG;
  if (!grad_ks_ok(ksize)) return BNN_HIP_ERR_UNSUPPORTED;
  if (mulc(((long long)C + 31) / 32, ksize * ksize, ((long long)O + 15) / 16, 3 * 64 * 8) > kMaxElems) return BNN_HIP_ERR_TOO_LARGE;
  return BNN_HIP_OK;
}

size_t bnn_hip_sconv2d_weight_pack_bytes(int O, int C, int ksize) {
  return check_sconv_weight(O, C, ksize) == BNN_HIP_OK ? bnn::sconv_weight_pack_bytes(O, C, ksize) : 0;
}

int bnn_hip_sconv2d_pack_weight_f32(const float* w, int O, int C, int ksize, void* packed, void* stream) {
  if (!w || !packed) return BNN_HIP_ERR_INVALID_ARG;
  const int st = check_sconv_weight(O, C, ksize);
  if (st != BNN_HIP_OK) return st;
  if (!aligned(packed, 16) || !aligned(w, 4)) return BNN_HIP_ERR_INVALID_ARG;
  g_launches.fetch_add(2, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_sconv_pack_weight(w, O, C, ksize, packed, static_cast<hipStream_t>(stream));
}

int bnn_hip_sconv2d_f32(const float* x, const void* packed, const float* bias, const float* post_scale, float* y, int N,
                        int O, int C, int H, int W, int ksize, int stride, void* stream) {
  if (!x || !packed || !y) return BNN_HIP_ERR_INVALID_ARG;
  int st = check_sconv_shape(N, O, C, H, W, ksize, stride);
  if (st == BNN_HIP_OK) st = check_sconv_weight(O, C, ksize);
  if (st != BNN_HIP_OK) return st;
  if (!aligned(packed, 16) || !aligned(x, 4) || !aligned(y, 4) || !aligned(bias, 4) || !aligned(post_scale, 4))
    return BNN_HIP_ERR_INVALID_ARG;
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_sconv(x, packed, bias, post_scale, y, N, O, C, H, W, ksize, stride, static_cast<hipStream_t>(stream));
}

int bnn_hip_pack_act_ste_f32(const float* x, int N, int C, int H, int W, uint64_t* P, uint64_t* M, uint64_t* T,
                             void* stream) {
  if (!T) return BNN_HIP_ERR_INVALID_ARG;
  const int st = check_pack(x, 4, N, C, H, W, P, M);
  if (st != BNN_HIP_OK) return st;
  if (!aligned(T, 8)) return BNN_HIP_ERR_INVALID_ARG;
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_pack_ste(x, N, C, H, W, P, M, T, static_cast<hipStream_t>(stream));
}

int bnn_hip_bn_act_pack_ste_f32(const float* x, int N, int C, int H, int W, const float* bn_scale, const float* bn_shift,
                                uint64_t* P, uint64_t* M, uint64_t* T, void* stream) {
  if (!T || (bn_scale == nullptr) != (bn_shift == nullptr)) return BNN_HIP_ERR_INVALID_ARG;
  const int st = check_pack(x, 4, N, C, H, W, P, M);
  if (st != BNN_HIP_OK) return st;
  if (!aligned(T, 8) || !aligned(bn_scale, 4) || !aligned(bn_shift, 4)) return BNN_HIP_ERR_INVALID_ARG;
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_bn_pack_ste(x, N, C, H, W, bn_scale, bn_shift, P, M, T, static_cast<hipStream_t>(stream));
}

int bnn_hip_bn_act_pack_ste_s2_f32(const float* x, int N, int C, int H, int W, const float* bn_scale, const float* bn_shift,
                                   uint64_t* P, uint64_t* M, uint64_t* T, void* stream) {
  if (!T || (bn_scale == nullptr) != (bn_shift == nullptr)) return BNN_HIP_ERR_INVALID_ARG;
  const int st = check_pack(x, 4, N, C, H, W, P, M);
  if (st != BNN_HIP_OK) return st;
  if (check_lattice(H, W) != BNN_HIP_OK) return BNN_HIP_ERR_INVALID_ARG;
  if (!aligned(T, 8) || !aligned(bn_scale, 4) || !aligned(bn_shift, 4)) return BNN_HIP_ERR_INVALID_ARG;
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_bn_pack_ste_s2(x, N, C, H, W, bn_scale, bn_shift, P, M, T, static_cast<hipStream_t>(stream));
}

int bnn_hip_bconv_grad_weight_splits(int N, int O, int C, int ksize) {
  return (N > 0 && O > 0 && C > 0 && grad_ks_ok(ksize)) ? bnn::grad_wgrad_splits(N, O, C, ksize)
                                                         : BNN_HIP_ERR_INVALID_ARG;
}

int bnn_hip_bconv_grad_weight_f32(const float* g, const float* x, float* partial, int splits, int N, int O, int C,
                                  int H, int W, int ksize, int stride, void* stream) {
  if (!g || !x || !partial || !aligned(g, 4) || !aligned(x, 4) || !aligned(partial, 4)) return BNN_HIP_ERR_INVALID_ARG;
  const int st = check_grad_shape(N, O, C, H, W, ksize, stride);
  if (st != BNN_HIP_OK) return st;
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_wgrad(g, x, nullptr, 0, partial, splits, N, O, C, H, W, ksize, stride,
                           static_cast<hipStream_t>(stream));
}

int bnn_hip_bconv_grad_weight_packed_f32(const float* g, const uint64_t* P, const uint64_t* M, float* partial, int splits,
                                         int N, int O, int C, int H, int W, int ksize, int stride, void* stream) {
  if (!g || !P || !M || !partial || !aligned(P, 8) || !aligned(M, 8) || !aligned(g, 4) || !aligned(partial, 4))
    return BNN_HIP_ERR_INVALID_ARG;
  const int st = check_grad_shape(N, O, C, H, W, ksize, stride);
  if (st != BNN_HIP_OK) return st;
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_wgrad(g, P, M, 1, partial, splits, N, O, C, H, W, ksize, stride, static_cast<hipStream_t>(stream));
}

// Entry contract of the grouped gradient kernels (csrc/grad_grouped.hip), and the ONE statement of what they cover:
// groups >= 2 dividing C and O, Cg <= 32 (a thread per channel of the group inside a wave), KH, KW <= 7 (the What tile of
// 32 output channels fits the LDS), one stride of 1 or 2 for both dimensions; any Og, width, dilation and padding the
// forward accepts.  g [N,O,Ho,Wo], gx [N,C,H,W] and the weight stay inside the 2^30-element addressing of a launch.
static int check_grouped_grad(const bnn_hip_conv_desc* d, int groups, bnn::GroupedGradP* q) {
  int Ho = 0, Wo = 0;
  const int st = check_desc(d, &Ho, &Wo);
  if (st != BNN_HIP_OK) return st;
  if (groups <= 0 || d->C % groups != 0 || d->O % groups != 0) return BNN_HIP_ERR_INVALID_ARG;
  if (groups == 1) return BNN_HIP_ERR_UNSUPPORTED;   // the dense layers have their own kernels (csrc/grad.hip)
  if (mulc(d->N, d->C, d->H, d->W) > kMaxConvElems) return BNN_HIP_ERR_TOO_LARGE;
  if (mulc(d->O, d->C / groups, d->KH, d->KW) > kMaxElems) return BNN_HIP_ERR_TOO_LARGE;
  if (d->C / groups > 32 || d->KH > 7 || d->KW > 7) return BNN_HIP_ERR_UNSUPPORTED;
  if (d->stride_h != d->stride_w || d->stride_h > 2) return BNN_HIP_ERR_UNSUPPORTED;
  *q = bnn::GroupedGradP{d->N, d->C, d->H, d->W, d->O, Ho, Wo, d->KH, d->KW, d->stride_h, d->pad_h, d->pad_w,
                         d->dil_h, d->dil_w, groups};
  return BNN_HIP_OK;
}

int bnn_hip_bconv_grouped_grad_supported(const bnn_hip_conv_desc* d, int groups) {
  bnn::GroupedGradP q;
  return check_grouped_grad(d, groups, &q) == BNN_HIP_OK ? 1 : 0;
}

int bnn_hip_bconv_grouped_grad_weight_splits(const bnn_hip_conv_desc* d, int groups) {
  bnn::GroupedGradP q;
  if (check_grouped_grad(d, groups, &q) != BNN_HIP_OK) return 0;
  return bnn::grouped_wgrad_splits(q.N, q.O, q.G, q.KH * q.KW);
}

int bnn_hip_bconv_grouped_grad_input_f32(const bnn_hip_conv_desc* d, int groups, const float* g, const float* what,
                                         const uint64_t* T, float* gx, void* stream) {
  if (!g || !what || !T || !gx || !aligned(g, 4) || !aligned(what, 4) || !aligned(T, 8) || !aligned(gx, 4))
    return BNN_HIP_ERR_INVALID_ARG;
  bnn::GroupedGradP q;
  const int st = check_grouped_grad(d, groups, &q);
  if (st != BNN_HIP_OK) return st;
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_grouped_dgrad(q, g, what, T, gx, static_cast<hipStream_t>(stream));
}

int bnn_hip_bconv_grouped_grad_weight_f32(const bnn_hip_conv_desc* d, int groups, const float* g, const uint64_t* P,
                                          const uint64_t* M, float* partial, int splits, void* stream) {
  if (!g || !P || !M || !partial || !aligned(g, 4) || !aligned(P, 8) || !aligned(M, 8) || !aligned(partial, 4))
    return BNN_HIP_ERR_INVALID_ARG;
  bnn::GroupedGradP q;
  const int st = check_grouped_grad(d, groups, &q);
  if (st != BNN_HIP_OK) return st;
  if (splits < 1 || splits > q.N) return BNN_HIP_ERR_INVALID_ARG;     // (every split holds at least one image)
  if (splits > 65535) return BNN_HIP_ERR_UNSUPPORTED;                 // (one grid row per split)
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_grouped_wgrad(q, g, P, M, partial, splits, static_cast<hipStream_t>(stream));
}

int bnn_hip_pack_weight_f32(const float* w, int O, int C, int KH, int KW, int center,
                            int compute_alpha, uint32_t* wbits, uint32_t* wnz, float* alpha,
                            int32_t* zero_flag, void* stream) {
  if (!w || !wbits || !wnz || !alpha || !zero_flag) return BNN_HIP_ERR_INVALID_ARG;
  bnn_hip_wlayout L;
  const int st = bnn_hip_weight_layout(O, C, KH, KW, &L);
  if (st != BNN_HIP_OK) return st;
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_pack_weight(w, O, C, KH, KW, center, compute_alpha, L, wbits, wnz, alpha,
                                 zero_flag, static_cast<hipStream_t>(stream));
}

int bnn_hip_bconv2d(const bnn_hip_conv_desc* d, const uint64_t* P, const uint64_t* M,
                    const uint32_t* wbits, const uint32_t* wnz, const float* alpha,
                    const float* bias, const float* post_scale, float* out, void* stream) {
  bnn::ConvP p = empty_convp();
  p.alpha = alpha; p.bias = bias; p.scale = post_scale; p.out = out;
  return run_conv(d, P, M, wbits, wnz, p, stream);
}

int bnn_hip_grouped_weight_layout(int O, int C, int groups, int KH, int KW, bnn_hip_wlayout* out) {
  if (!out || O <= 0 || C <= 0 || groups <= 0 || KH <= 0 || KW <= 0) return BNN_HIP_ERR_INVALID_ARG;
  if (C % groups != 0 || O % groups != 0) return BNN_HIP_ERR_INVALID_ARG;
  const long long S = grouped_words_per_tap(O, C, groups);   // (at most C / 32 + 2: an int)
  return fill_layout(O, KH, KW, S, (int)S, out);               // one chunk: the grouped kernel walks its window
}

int bnn_hip_pack_weight_grouped_f32(const float* w, int O, int Cg, int groups, int KH, int KW, int center,
                                    int compute_alpha, uint32_t* wbits, uint32_t* wnz, float* alpha,
                                    int32_t* zero_flag, void* stream) {
  if (!w || !wbits || !wnz || !alpha || !zero_flag || Cg <= 0 || groups <= 0) return BNN_HIP_ERR_INVALID_ARG;
  if ((long long)Cg * groups > 0x7fffffffLL) return BNN_HIP_ERR_TOO_LARGE;
  bnn_hip_wlayout L;
  const int st = bnn_hip_grouped_weight_layout(O, Cg * groups, groups, KH, KW, &L);
  if (st != BNN_HIP_OK) return st;
  // the fp32 weight itself is read with 64-bit offsets, but its size must be a valid tensor
  if (mulc(O, Cg, L.taps) > kMaxElems) return BNN_HIP_ERR_TOO_LARGE;
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_pack_weight_grouped(w, O, Cg, groups, center, compute_alpha, L, wbits, wnz, alpha, zero_flag,
                                         static_cast<hipStream_t>(stream));
}

int bnn_hip_bconv2d_grouped(const bnn_hip_conv_desc* d, int groups, const uint64_t* P, const uint64_t* M,
                            const uint32_t* wbits, const uint32_t* wnz, const float* alpha, const float* bias,
                            const float* post_scale, float* out, void* stream) {
  bnn::ConvP p = empty_convp();
  int S = 0;
  const int st = check_grouped(d, groups, P, M, wbits, wnz, alpha, bias, post_scale, out, &p, &S);
  if (st != BNN_HIP_OK) return st;
  g_launches.fetch_add(1, std::memory_order_relaxed);
  Range range(p.raw ? "bnn_hip_bconv2d_grouped_dot" : "bnn_hip_bconv2d_grouped");
  return bnn::launch_bconv_grouped(p, groups, S, static_cast<hipStream_t>(stream));
}

int bnn_hip_bconv2d_grouped_fused(const bnn_hip_conv_desc* d, int groups, const uint64_t* P, const uint64_t* M,
                                  const uint32_t* wbits, const uint32_t* wnz, const float* alpha, const float* bias,
                                  const float* post_scale, const float* prelu, int shuffle_groups,
                                  const float* residual, float* out, void* stream) {
  bnn::ConvP p = empty_convp();
  int S = 0;
  const int st = check_grouped(d, groups, P, M, wbits, wnz, alpha, bias, post_scale, out, &p, &S);
  if (st != BNN_HIP_OK) return st;
  if (!alpha) return BNN_HIP_ERR_INVALID_ARG;  // the epilogue works on the float value: no raw-dot form
  if (shuffle_groups < 1 || d->O % shuffle_groups != 0) return BNN_HIP_ERR_INVALID_ARG;
  // the kernel reads the residual and writes its output through independent (__restrict__) pointers, and the shuffle
  // makes a wave's stores land on other planes than its loads: the two [N,O,Ho,Wo] tensors must not overlap
  if (residual) {
    const uintptr_t r = reinterpret_cast<uintptr_t>(residual), o = reinterpret_cast<uintptr_t>(out);
    const uintptr_t bytes = (uintptr_t)mulc(d->N, d->O, p.Ho, p.Wo) * 4;   // (check_desc: below 2^32)
    if (!aligned(residual, 4) || (r < o + bytes && o < r + bytes)) return BNN_HIP_ERR_INVALID_ARG;
  }
  p.prelu = prelu; p.res = residual;
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_bconv_grouped_cell(p, groups, S, shuffle_groups, static_cast<hipStream_t>(stream));
}

int bnn_hip_fconv_supported(const bnn_hip_fconv_desc* d) {
  return (d && check_fconv_desc(d) == BNN_HIP_OK && bnn::fconv_supported(d->C, d->H, d->W, d->K, d->stride)) ? 1 : 0;
}

int bnn_hip_fconv_fused(const bnn_hip_fconv_desc* d, const uint64_t* P, const uint64_t* M, const uint32_t* w1bits,
                        const uint32_t* w1nz, const bnn_hip_fconv_stage* s1, const uint32_t* w2bits, const uint32_t* w2nz,
                        const bnn_hip_fconv_stage* s2, const float* mid_scale, const float* mid_shift, int shuffle_groups,
                        const float* residual, float* out, void* stream) {
  if (!d) return BNN_HIP_ERR_INVALID_ARG;
  const int st = check_fconv_desc(d);
  if (st != BNN_HIP_OK) return st;
  if (!P || !M || !w1bits || !w2bits || !s1 || !s2 || !s1->alpha || !s2->alpha || !mid_scale || !mid_shift || !out)
    return BNN_HIP_ERR_INVALID_ARG;
  const bool wz = (d->flags & BNN_HIP_FLAG_WEIGHT_ZEROS) != 0;
  if (wz && (!w1nz || !w2nz)) return BNN_HIP_ERR_INVALID_ARG;
  if (!aligned(P, 16) || !aligned(M, 16) || !aligned(w1bits, 16) || !aligned(w2bits, 16) || !aligned(s1->alpha, 4) ||
      !aligned(s2->alpha, 4) || !aligned(out, 4) || !aligned(mid_scale, 4) || !aligned(mid_shift, 4))
    return BNN_HIP_ERR_INVALID_ARG;
  if (wz && (!aligned(w1nz, 16) || !aligned(w2nz, 16))) return BNN_HIP_ERR_INVALID_ARG;
  for (const bnn_hip_fconv_stage* s : {s1, s2})
    if (!aligned(s->bias, 4) || !aligned(s->post_scale, 4) || !aligned(s->prelu, 4)) return BNN_HIP_ERR_INVALID_ARG;
  if (shuffle_groups < 1 || d->C % shuffle_groups != 0) return BNN_HIP_ERR_INVALID_ARG;
  if (residual) {  // read and written through independent pointers, on other planes under the shuffle: no overlap
    const int Ho = (d->H - 1) / d->stride + 1, Wo = (d->W - 1) / d->stride + 1;
    const uintptr_t r = reinterpret_cast<uintptr_t>(residual), o = reinterpret_cast<uintptr_t>(out);
    const uintptr_t bytes = (uintptr_t)mulc(d->N, d->C, Ho, Wo) * 4;   // (check_fconv_desc: below 2^32)
    if (!aligned(residual, 4) || (r < o + bytes && o < r + bytes)) return BNN_HIP_ERR_INVALID_ARG;
  }
  if (!bnn::fconv_supported(d->C, d->H, d->W, d->K, d->stride)) return BNN_HIP_ERR_UNSUPPORTED;
  bnn::FconvP p{};
  p.P = P; p.M = M; p.W1 = w1bits; p.Z1 = wz ? w1nz : nullptr; p.W2 = w2bits; p.Z2 = wz ? w2nz : nullptr;
  p.s1 = *s1; p.s2 = *s2; p.mid_a = mid_scale; p.mid_b = mid_shift; p.res = residual; p.out = out;
  p.N = d->N; p.C = d->C; p.H = d->H; p.W = d->W; p.K = d->K; p.stride = d->stride; p.shuffle_groups = shuffle_groups;
  p.wz = wz;
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_fconv(p, static_cast<hipStream_t>(stream));
}

int bnn_hip_bconv2d_grouped_node(const bnn_hip_conv_desc* d, int groups, const uint64_t* P, const uint64_t* M,
                                 const uint32_t* wbits, const uint32_t* wnz, const float* alpha, const float* bias,
                                 const float* post_scale, const float* prelu, int shuffle_groups,
                                 const bnn_hip_f32_view* residual, const bnn_hip_f32_view* addend, float* out,
                                 int out_c_offset, int out_c_total, void* stream) {
  bnn::ConvP p = empty_convp();
  int S = 0;
  const int st = check_grouped(d, groups, P, M, wbits, wnz, alpha, bias, post_scale, out, &p, &S);
  if (st != BNN_HIP_OK) return st;
  if (!alpha) return BNN_HIP_ERR_INVALID_ARG;  // the epilogue works on the float value: no raw-dot form
  if (shuffle_groups < 1 || d->O % shuffle_groups != 0) return BNN_HIP_ERR_INVALID_ARG;
  const long long hw = mulc(p.Ho, p.Wo);
  const bnn_hip_f32_view ov = {out, out_c_offset, out_c_total};
  const int so = check_view(&ov, d->N, d->O, hw, kMaxConvElems, &p.c_off, &p.c_tot);
  if (so != BNN_HIP_OK) return so;
  // the operands: per-lane byte offsets of 32 bits like the output's, and no element shared with it (the kernel reads
  // them through independent __restrict__ pointers, and the shuffle makes a wave store other planes than it loads)
  const float* opnd[2] = {nullptr, nullptr};
  int ct[2] = {d->O, d->O};
  const bnn_hip_f32_view* views[2] = {residual, addend};
  for (int i = 0; i < 2; ++i) {
    if (!views[i]) continue;
    int off = 0;
    const int sv = check_view(views[i], d->N, d->O, hw, kMaxConvElems, &off, &ct[i]);
    if (sv != BNN_HIP_OK) return sv;
    if (views_may_overlap(out, p.c_off, p.c_tot, views[i]->p, off, ct[i], d->N, d->O, hw)) return BNN_HIP_ERR_INVALID_ARG;
    opnd[i] = views[i]->p + (size_t)off * (size_t)hw;
  }
  p.prelu = prelu; p.res = opnd[0];
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_bconv_grouped_node(p, groups, S, shuffle_groups, opnd[1], ct[0], ct[1],
                                        static_cast<hipStream_t>(stream));
}

int bnn_hip_bconv2d_fused(const bnn_hip_conv_desc* d, const uint64_t* P, const uint64_t* M,
                          const uint32_t* wbits, const uint32_t* wnz, const bnn_hip_epilogue* e,
                          void* stream) {
  bnn::ConvP p = empty_convp();
  const int st = epilogue_convp(e, &p);
  if (st != BNN_HIP_OK) return st;
  return run_conv(d, P, M, wbits, wnz, p, stream);
}

int bnn_hip_bconv2d_route(const bnn_hip_conv_desc* d, const bnn_hip_epilogue* e, bnn_hip_conv_route* out) {
  bnn::ConvP p = empty_convp();
  if (e) {
    const int st = epilogue_convp(e, &p);
    if (st != BNN_HIP_OK) return st;
  } else {  // bnn_hip_bconv2d: alpha -> fp32 (any non-null values: only compared with null)
    p.alpha = reinterpret_cast<const float*>(&p);
    p.out = &p;
  }
  return route_conv(d, p, out);
}

int bnn_hip_bconv2d_dot_route(const bnn_hip_conv_desc* d, bnn_hip_conv_route* out) {
  bnn::ConvP p = empty_convp();
  p.raw = true; p.out = &p;
  return route_conv(d, p, out);
}

int bnn_hip_shortcut_fold_supported(const bnn_hip_conv_desc* d, int sc_C) {
  int Ho = 0, Wo = 0;
  if (check_desc(d, &Ho, &Wo) != BNN_HIP_OK) return 0;
  bnn::ConvP p = empty_convp();
  fill_geometry(d, Ho, Wo, &p);
  // the epilogue the fold belongs to: BatchNorm + shortcut + ReLU -> fp32 + sign planes (any non-null pointers)
  const float* f = reinterpret_cast<const float*>(&p);
  p.alpha = f; p.bn_a = f; p.bn_b = f; p.relu = true; p.out = &p;
  p.outP = reinterpret_cast<uint32_t*>(&p); p.outM = reinterpret_cast<uint32_t*>(&p);
  p.ds_C = sc_C;
  return bnn::ds_fold_applies(p, d->flags) ? 1 : 0;
}

// ---- the dense 3x3 convolution on the int8 matrix cores (csrc/bconv_mfma.hip) ----
size_t bnn_hip_weight_i8_bytes(int O, int C, int KH, int KW) { return bnn::weight_i8_bytes(O, C, KH, KW); }

int bnn_hip_pack_weight_i8(const uint32_t* wbits, const uint32_t* wnz, int O, int C, int KH, int KW, void* w8,
                           void* stream) {
  if (!wbits || !wnz || !w8) return BNN_HIP_ERR_INVALID_ARG;
  bnn_hip_wlayout L;
  const int st = bnn_hip_weight_layout(O, C, KH, KW, &L);
  if (st != BNN_HIP_OK) return st;
  if (bnn::weight_i8_bytes(O, C, KH, KW) == 0) return BNN_HIP_ERR_UNSUPPORTED;
  if (!aligned(wbits, 16) || !aligned(wnz, 16) || !aligned(w8, 16)) return BNN_HIP_ERR_INVALID_ARG;
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_pack_weight_i8(wbits, wnz, L, O, w8, static_cast<hipStream_t>(stream));
}

// The int8, the FP4 and the 1x1 FP4 entry points share their validation.
namespace {
// form: the kernel a call is for — the 3x3 kernel in its int8 or its FP4 form (bconv_mfma.hip), or the 1x1 FP4 kernel
// (bconv1x1_mfma.hip).  Only the admission rule and the launcher differ.
enum { kMfmaI8 = 0, kMfmaF4 = 1, kMfma1x1F4 = 2 };
bool mfma_applies(const bnn::ConvP& p, int flags, int form) {
  return form == kMfma1x1F4 ? bnn::mfma1x1_applies(p, flags)
         : form == kMfmaF4  ? bnn::mfma4_conv_applies(p, flags)
                            : bnn::mfma_conv_applies(p, flags);
}

int mfma_supported(const bnn_hip_conv_desc* d, const bnn_hip_epilogue* e, int form) {
  alignas(16) static const uint64_t operand[2] = {0, 0};  // stands in for the packed operands (never read)
  bnn::ConvP p = empty_convp();
  if (epilogue_convp(e, &p) != BNN_HIP_OK) return 0;
  const uint32_t* const w = reinterpret_cast<const uint32_t*>(operand);
  if (check_conv(d, operand, operand, w, w, &p) != BNN_HIP_OK) return 0;
  if (p.out && !aligned(p.out, 4)) return 0;
  return mfma_applies(p, d->flags, form) ? 1 : 0;
}

int mfma_fused(const bnn_hip_conv_desc* d, const uint64_t* P, const uint64_t* M, const void* w8,
               const bnn_hip_epilogue* e, void* stream, int form) {
  bnn::ConvP p = empty_convp();
  int st = epilogue_convp(e, &p);
  if (st != BNN_HIP_OK) return st;
  if (!w8 || !aligned(w8, 16)) return BNN_HIP_ERR_INVALID_ARG;
  // (the int8 pack stands in for wbits / wnz in the shared validator: non-null and 16-byte aligned like them)
  st = check_conv(d, P, M, static_cast<const uint32_t*>(w8), static_cast<const uint32_t*>(w8), &p);
  if (st != BNN_HIP_OK) return st;
  if (p.out && !aligned(p.out, 4)) return BNN_HIP_ERR_INVALID_ARG;
  if (!mfma_applies(p, d->flags, form)) return BNN_HIP_ERR_UNSUPPORTED;
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  if (form == kMfma1x1F4) return bnn::launch_bconv1x1_mfma(p, d->flags, w8, static_cast<hipStream_t>(stream));
  return bnn::launch_bconv_mfma(p, d->flags, w8, static_cast<hipStream_t>(stream), form == kMfmaF4);
}
}  // namespace

int bnn_hip_bconv2d_mfma_supported(const bnn_hip_conv_desc* d, const bnn_hip_epilogue* e) {
  return mfma_supported(d, e, kMfmaI8);
}

int bnn_hip_bconv2d_mfma_fused(const bnn_hip_conv_desc* d, const uint64_t* P, const uint64_t* M, const void* w8,
                               const bnn_hip_epilogue* e, void* stream) {
  return mfma_fused(d, P, M, w8, e, stream, kMfmaI8);
}

// ---- the FP4 form (bnn_hip_pack_weight_f4's pack in place of the int8 one) ----
size_t bnn_hip_weight_f4_bytes(int O, int C, int KH, int KW) { return bnn::weight_f4_bytes(O, C, KH, KW); }

int bnn_hip_pack_weight_f4(const uint32_t* wbits, const uint32_t* wnz, int O, int C, int KH, int KW, void* w4,
                           void* stream) {
  if (!wbits || !wnz || !w4) return BNN_HIP_ERR_INVALID_ARG;
  bnn_hip_wlayout L;
  const int st = bnn_hip_weight_layout(O, C, KH, KW, &L);
  if (st != BNN_HIP_OK) return st;
  if (bnn::weight_f4_bytes(O, C, KH, KW) == 0) return BNN_HIP_ERR_UNSUPPORTED;
  if (!aligned(wbits, 16) || !aligned(wnz, 16) || !aligned(w4, 16)) return BNN_HIP_ERR_INVALID_ARG;
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_pack_weight_f4(wbits, wnz, L, O, w4, static_cast<hipStream_t>(stream));
}

int bnn_hip_bconv2d_mfma4_supported(const bnn_hip_conv_desc* d, const bnn_hip_epilogue* e) {
  return mfma_supported(d, e, kMfmaF4);
}

int bnn_hip_bconv2d_mfma4_fused(const bnn_hip_conv_desc* d, const uint64_t* P, const uint64_t* M, const void* w4,
                                const bnn_hip_epilogue* e, void* stream) {
  return mfma_fused(d, P, M, w4, e, stream, kMfmaF4);
}

// ---- the 1x1 convolution on the FP4 matrix cores (csrc/bconv1x1_mfma.hip) ----
size_t bnn_hip_weight1x1_f4_bytes(int O, int C) { return bnn::weight1x1_f4_bytes(O, C); }

int bnn_hip_pack_weight1x1_f4(const uint32_t* wbits, const uint32_t* wnz, int O, int C, int KH, int KW, void* w4,
                              void* stream) {
  if (!wbits || !wnz || !w4) return BNN_HIP_ERR_INVALID_ARG;
  bnn_hip_wlayout L;
  const int st = bnn_hip_weight_layout(O, C, KH, KW, &L);
  if (st != BNN_HIP_OK) return st;
  if (KH != 1 || KW != 1 || bnn::weight1x1_f4_bytes(O, C) == 0) return BNN_HIP_ERR_UNSUPPORTED;
  if (!aligned(wbits, 16) || !aligned(wnz, 16) || !aligned(w4, 16)) return BNN_HIP_ERR_INVALID_ARG;
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_pack_weight_f4(wbits, wnz, L, O, w4, static_cast<hipStream_t>(stream));  // (the 3x3 pack's, one tap)
}

int bnn_hip_bconv1x1_mfma4_supported(const bnn_hip_conv_desc* d, const bnn_hip_epilogue* e) {
  return mfma_supported(d, e, kMfma1x1F4);
}

int bnn_hip_bconv1x1_mfma4_fused(const bnn_hip_conv_desc* d, const uint64_t* P, const uint64_t* M, const void* w4,
                                 const bnn_hip_epilogue* e, void* stream) {
  return mfma_fused(d, P, M, w4, e, stream, kMfma1x1F4);
}

// ---- the same with the shortcut convolution folded in ----
size_t bnn_hip_shortcut_weight_i8_bytes(int O, int C) { return bnn::shortcut_weight_i8_bytes(O, C); }

int bnn_hip_pack_shortcut_weight_i8(const uint32_t* wbits, int O, int C, void* sc_w8, void* stream) {
  if (!wbits || !sc_w8 || O <= 0 || C <= 0) return BNN_HIP_ERR_INVALID_ARG;
  if (bnn::shortcut_weight_i8_bytes(O, C) == 0) return BNN_HIP_ERR_UNSUPPORTED;
  if (!aligned(wbits, 16) || !aligned(sc_w8, 16)) return BNN_HIP_ERR_INVALID_ARG;
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_pack_shortcut_weight_i8(wbits, O, C, sc_w8, static_cast<hipStream_t>(stream));
}

namespace {
int mfma_fold_supported(const bnn_hip_conv_desc* d, const bnn_hip_epilogue* e, bool f4) {
  alignas(16) static const uint64_t operand[2] = {0, 0};  // stands in for the packed operands (never read)
  bnn::ConvP p = empty_convp();
  if (epilogue_convp(e, &p) != BNN_HIP_OK || !p.ds_P) return 0;
  const uint32_t* const w = reinterpret_cast<const uint32_t*>(operand);
  p.ds_W = w;  // (the shortcut's int8 pack stands in for sc_wbits in the shared validator)
  if (check_conv(d, operand, operand, w, w, &p) != BNN_HIP_OK) return 0;
  if (p.out && !aligned(p.out, 4)) return 0;
  return (f4 ? bnn::mfma4_fold_applies(p, d->flags) : bnn::mfma_fold_applies(p, d->flags)) ? 1 : 0;
}

int mfma_fold_fused(const bnn_hip_conv_desc* d, const uint64_t* P, const uint64_t* M, const void* w8, const void* sc_w8,
                    const bnn_hip_epilogue* e, void* stream, bool f4) {
  bnn::ConvP p = empty_convp();
  int st = epilogue_convp(e, &p);
  if (st != BNN_HIP_OK) return st;
  if (!w8 || !aligned(w8, 16) || !sc_w8 || !aligned(sc_w8, 16)) return BNN_HIP_ERR_INVALID_ARG;
  if (!p.ds_P) return BNN_HIP_ERR_UNSUPPORTED;
  p.ds_W = static_cast<const uint32_t*>(sc_w8);  // (stands in for sc_wbits in the shared validator, like w8 for wbits)
  st = check_conv(d, P, M, static_cast<const uint32_t*>(w8), static_cast<const uint32_t*>(w8), &p);
  if (st != BNN_HIP_OK) return st;
  if (p.out && !aligned(p.out, 4)) return BNN_HIP_ERR_INVALID_ARG;
  if (!(f4 ? bnn::mfma4_fold_applies(p, d->flags) : bnn::mfma_fold_applies(p, d->flags))) return BNN_HIP_ERR_UNSUPPORTED;
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_bconv_mfma_fold(p, d->flags, w8, sc_w8, static_cast<hipStream_t>(stream), f4);
}
}  // namespace

int bnn_hip_bconv2d_mfma_fold_supported(const bnn_hip_conv_desc* d, const bnn_hip_epilogue* e) {
  return mfma_fold_supported(d, e, false);
}

int bnn_hip_bconv2d_mfma_fold_fused(const bnn_hip_conv_desc* d, const uint64_t* P, const uint64_t* M, const void* w8,
                                    const void* sc_w8, const bnn_hip_epilogue* e, void* stream) {
  return mfma_fold_fused(d, P, M, w8, sc_w8, e, stream, false);
}

// (the shortcut's weight stays the int8 pack: bnn_hip_pack_shortcut_weight_i8)
int bnn_hip_bconv2d_mfma4_fold_supported(const bnn_hip_conv_desc* d, const bnn_hip_epilogue* e) {
  return mfma_fold_supported(d, e, true);
}

int bnn_hip_bconv2d_mfma4_fold_fused(const bnn_hip_conv_desc* d, const uint64_t* P, const uint64_t* M, const void* w4,
                                     const void* sc_w8, const bnn_hip_epilogue* e, void* stream) {
  return mfma_fold_fused(d, P, M, w4, sc_w8, e, stream, true);
}

int bnn_hip_sign_thresholds_f32(const float* alpha, const float* bias, const float* post_scale, const float* bn_scale,
                                const float* bn_shift, int O, int kmax, int32_t* thresholds, void* stream) {
  // (kmax < 2^20: the two-instruction form of the test biases its counts by 2^20 > kmax / 2, bconv_core.h kMidtBias)
  if (!alpha || !thresholds || O <= 0 || kmax <= 0 || kmax >= (1 << 20)) return BNN_HIP_ERR_INVALID_ARG;
  if ((bn_scale == nullptr) != (bn_shift == nullptr)) return BNN_HIP_ERR_INVALID_ARG;
  if (!aligned(thresholds, 4)) return BNN_HIP_ERR_INVALID_ARG;
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_sign_thresholds(alpha, bias, post_scale, bn_scale, bn_shift, O, kmax, thresholds,
                                     static_cast<hipStream_t>(stream));
}

int bnn_hip_bconv2d_dot(const bnn_hip_conv_desc* d, const uint64_t* P, const uint64_t* M,
                        const uint32_t* wbits, const uint32_t* wnz, int32_t* dot, void* stream) {
  bnn::ConvP p = empty_convp();
  p.raw = true; p.out = dot;
  return run_conv(d, P, M, wbits, wnz, p, stream);
}

int bnn_hip_blinear(int B, int F, int O, const uint64_t* P, const uint64_t* M, const uint32_t* wbits,
                    const uint32_t* wnz, int weight_zeros, const float* alpha, const float* bias,
                    const float* post_scale, float* out, void* stream) {
  bnn_hip_conv_desc d;
  std::memset(&d, 0, sizeof(d));
  d.N = B; d.C = F; d.H = 1; d.W = 1; d.O = O; d.KH = 1; d.KW = 1;
  d.stride_h = d.stride_w = 1; d.dil_h = d.dil_w = 1;
  d.flags = weight_zeros ? BNN_HIP_FLAG_WEIGHT_ZEROS : 0;
  return bnn_hip_bconv2d(&d, P, M, wbits, wnz, alpha, bias, post_scale, out, stream);
}

// Entry contract of the GEMM-shaped Linear kernels (csrc/blinear.hip): positive sizes, M * F and M * O below 2^30 per launch
// (the caller splits M), a weight whose 1x1 pack layout exists.
static int check_linear(int M, int F, int O) {
  if (M <= 0 || F <= 0 || O <= 0) return BNN_HIP_ERR_INVALID_ARG;
  if (mulc(M, F) > kMaxConvElems || mulc(M, O) > kMaxConvElems) return BNN_HIP_ERR_TOO_LARGE;
  bnn_hip_wlayout L;
  return bnn_hip_weight_layout(O, F, 1, 1, &L);
}

int bnn_hip_blinear_direct(int M, int F, int O, const void* x, int x_dtype, const uint32_t* wbits, const uint32_t* wnz,
                           int weight_zeros, const float* alpha, const float* bias, const float* post_scale, float* out,
                           uint64_t* P, uint64_t* Mn, uint64_t* T, int lds_words, void* stream) {
  if (!x || !wbits || !alpha || !out || lds_words < 0) return BNN_HIP_ERR_INVALID_ARG;
  if (x_dtype != BNN_HIP_DTYPE_F32 && x_dtype != BNN_HIP_DTYPE_F16 && x_dtype != BNN_HIP_DTYPE_BF16)
    return BNN_HIP_ERR_INVALID_ARG;
  if (weight_zeros && !wnz) return BNN_HIP_ERR_INVALID_ARG;
  if ((P == nullptr) != (Mn == nullptr) || (P == nullptr) != (T == nullptr)) return BNN_HIP_ERR_INVALID_ARG;
  if (!aligned(x, x_dtype == BNN_HIP_DTYPE_F32 ? 4 : 2) || !aligned(wbits, 16) || !aligned(wnz, 16) || !aligned(alpha, 4) ||
      !aligned(bias, 4) || !aligned(post_scale, 4) || !aligned(out, 4) || !aligned(P, 8) || !aligned(Mn, 8) || !aligned(T, 8))
    return BNN_HIP_ERR_INVALID_ARG;
  const int st = check_linear(M, F, O);
  if (st != BNN_HIP_OK) return st;
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_blinear_fwd(x, x_dtype, wbits, wnz, weight_zeros != 0, alpha, bias, post_scale, out,
                                 P, Mn, T, M, F, O, lds_words, static_cast<hipStream_t>(stream));
}

int bnn_hip_blinear_grad_input_f32(const float* g, const float* alpha, const uint32_t* wbits, const uint32_t* wnz,
                                   const uint64_t* T, float* gx, int M, int O, int F, void* stream) {
  if (!g || !alpha || !wbits || !wnz || !T || !gx) return BNN_HIP_ERR_INVALID_ARG;
  if (!aligned(g, 4) || !aligned(alpha, 4) || !aligned(wbits, 16) || !aligned(wnz, 16) || !aligned(T, 8) || !aligned(gx, 4))
    return BNN_HIP_ERR_INVALID_ARG;
  const int st = check_linear(M, F, O);
  if (st != BNN_HIP_OK) return st;
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_blinear_dgrad(g, alpha, wbits, wnz, T, gx, M, O, F, static_cast<hipStream_t>(stream));
}

int bnn_hip_blinear_grad_weight_splits(int M, int O, int F) {
  return check_linear(M, F, O) == BNN_HIP_OK ? bnn::blinear_wgrad_splits(M, O, F) : BNN_HIP_ERR_INVALID_ARG;
}

int bnn_hip_blinear_grad_weight_f32(const float* g, const uint64_t* P, const uint64_t* Mn, float* partial, int splits, int M,
                                    int O, int F, void* stream) {
  if (!g || !P || !Mn || !partial || !aligned(g, 4) || !aligned(P, 8) || !aligned(Mn, 8) || !aligned(partial, 4))
    return BNN_HIP_ERR_INVALID_ARG;
  const int st = check_linear(M, F, O);
  if (st != BNN_HIP_OK) return st;
  // the rule of bnn_hip_bconv_grad_weight_f32, checked here (a host-side decision): every split holds ceil(M / splits) rows,
  // the last one what is left, none is empty
  if (splits < 1 || splits > M) return BNN_HIP_ERR_INVALID_ARG;
  const int per = (M + splits - 1) / splits;
  if ((M + per - 1) / per != splits) return BNN_HIP_ERR_INVALID_ARG;
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_blinear_wgrad(g, P, Mn, partial, splits, M, O, F, static_cast<hipStream_t>(stream));
}

// Linear with binary activations and real weights (csrc/slinear.hip): the sizes of check_linear, the weight that of
// check_sconv_weight with ksize = 1.
int bnn_hip_slinear_f32(int M, int F, int O, const float* x, const void* packed, const float* bias, const float* post_scale,
                        float* out, uint64_t* P, uint64_t* Mn, uint64_t* T, void* stream) {
  if (!x || !packed || !out) return BNN_HIP_ERR_INVALID_ARG;
  if ((P == nullptr) != (Mn == nullptr) || (P == nullptr) != (T == nullptr)) return BNN_HIP_ERR_INVALID_ARG;
  int st = check_linear(M, F, O);
  if (st == BNN_HIP_OK) st = check_sconv_weight(O, F, 1);
  if (st != BNN_HIP_OK) return st;
  if (!aligned(packed, 16) || !aligned(x, 4) || !aligned(out, 4) || !aligned(bias, 4) || !aligned(post_scale, 4) ||
      !aligned(P, 8) || !aligned(Mn, 8) || !aligned(T, 8))
    return BNN_HIP_ERR_INVALID_ARG;
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_slinear(x, packed, bias, post_scale, out, P, Mn, T, M, F, O, static_cast<hipStream_t>(stream));
}

int bnn_hip_ste_mask_f32(float* gx, const uint64_t* T, int M, int F, void* stream) {
  if (!gx || !T) return BNN_HIP_ERR_INVALID_ARG;
  if (M <= 0 || F <= 0) return BNN_HIP_ERR_INVALID_ARG;
  if (mulc(M, F) > kMaxConvElems) return BNN_HIP_ERR_TOO_LARGE;
  if (!aligned(gx, 4) || !aligned(T, 8)) return BNN_HIP_ERR_INVALID_ARG;
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_ste_mask(gx, T, M, F, static_cast<hipStream_t>(stream));
}

// Geometry part of a ConvP for the one-launch layer (no packed operands).
static int fly_convp(const bnn_hip_conv_desc* d, bnn::ConvP* out) {
  int Ho = 0, Wo = 0;
  const int st = check_desc(d, &Ho, &Wo);
  if (st != BNN_HIP_OK) return st;
  if (mulc(d->N, d->C, d->H, d->W) > kMaxConvElems) return BNN_HIP_ERR_TOO_LARGE;
  // the kernel reads x through a sized buffer descriptor and marks dead lanes with offset 0xFFFFFFF0 (+ soffset): a
  // tensor within a few elements of 2^32 bytes would bring the marker in range.  UNSUPPORTED, not TOO_LARGE: the
  // two-launch form (pack_act + conv) of the same layer has no such limit and callers fall back to it
  if (mulc(d->N, d->C, d->H, d->W) * 4 > kMaxDescBytes) return BNN_HIP_ERR_UNSUPPORTED;
  *out = empty_convp();
  fill_geometry(d, Ho, Wo, out);
  return BNN_HIP_OK;
}

int bnn_hip_bconv2d_direct_plan(const bnn_hip_conv_desc* d, bnn_hip_fly_plan* plan) {
  if (!plan) return BNN_HIP_ERR_INVALID_ARG;
  bnn::ConvP p;
  const int st = fly_convp(d, &p);
  if (st != BNN_HIP_OK) return st;
  return bnn::fly_default_plan(p, d->flags, plan);
}

int bnn_hip_bconv2d_direct(const bnn_hip_conv_desc* d, const void* x, int x_dtype, const uint32_t* wbits,
                           const uint32_t* wnz, const float* alpha, const float* bias, const float* post_scale,
                           float* out, const bnn_hip_fly_plan* plan, void* stream) {
  if (!d || !x || !wbits || !alpha || !out) return BNN_HIP_ERR_INVALID_ARG;
  if (x_dtype != BNN_HIP_DTYPE_F32 && x_dtype != BNN_HIP_DTYPE_F16 && x_dtype != BNN_HIP_DTYPE_BF16)
    return BNN_HIP_ERR_INVALID_ARG;
  // the output type travels in the descriptor's flags; the shared validator sees the descriptor without them
  const int out_bits = d->flags & (BNN_HIP_FLAG_OUT_F16 | BNN_HIP_FLAG_OUT_BF16);
  if (out_bits == (BNN_HIP_FLAG_OUT_F16 | BNN_HIP_FLAG_OUT_BF16)) return BNN_HIP_ERR_INVALID_ARG;
  bnn_hip_conv_desc plain = *d;
  plain.flags &= ~(BNN_HIP_FLAG_OUT_F16 | BNN_HIP_FLAG_OUT_BF16);
  d = &plain;
  if (!aligned(x, x_dtype == BNN_HIP_DTYPE_F32 ? 4 : 2) || !aligned(wbits, 16) || !aligned(out, out_bits ? 2 : 4))
    return BNN_HIP_ERR_INVALID_ARG;
  if ((d->flags & BNN_HIP_FLAG_WEIGHT_ZEROS) && !wnz) return BNN_HIP_ERR_INVALID_ARG;
  bnn::ConvP p;
  const int st = fly_convp(d, &p);
  if (st != BNN_HIP_OK) return st;
  p.out16 = out_bits == BNN_HIP_FLAG_OUT_F16 ? BNN_HIP_DTYPE_F16 : out_bits == BNN_HIP_FLAG_OUT_BF16 ? BNN_HIP_DTYPE_BF16 : 0;
  p.W = wbits; p.Z = wnz; p.alpha = alpha; p.bias = bias; p.scale = post_scale; p.out = out;
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_bconv_fly(p, x, x_dtype, d->flags, plan, static_cast<hipStream_t>(stream));
}

static bool direct_applies(const bnn_hip_conv_desc* d) {
  bnn::ConvP p;
  return fly_convp(d, &p) == BNN_HIP_OK && bnn::fly_supported(p);
}

// Workspace of the two-launch form of bnn_hip_bconv2d_f32: the P plane, then the M plane, each rounded up to 256 bytes.
static size_t conv_plane_bytes(const bnn_hip_conv_desc* d) {
  const size_t npix = (size_t)d->N * d->H * d->W;
  return align_up(npix * ((d->C + 63) / 64) * sizeof(uint64_t), 256);
}

size_t bnn_hip_conv_workspace_bytes(const bnn_hip_conv_desc* d) {
  int Ho = 0, Wo = 0;
  if (check_desc(d, &Ho, &Wo) != BNN_HIP_OK) return 0;   // (bnn_hip_bconv2d_f32 rejects such a descriptor itself)
  if (direct_applies(d)) return 0;
  return 2 * conv_plane_bytes(d);
}

int bnn_hip_bconv2d_f32(const bnn_hip_conv_desc* d, const float* x, const uint32_t* wbits,
                        const uint32_t* wnz, const float* alpha, const float* bias,
                        const float* post_scale, float* out, void* workspace, void* stream) {
  if (!d || !x) return BNN_HIP_ERR_INVALID_ARG;
  if (direct_applies(d))
    return bnn_hip_bconv2d_direct(d, x, BNN_HIP_DTYPE_F32, wbits, wnz, alpha, bias, post_scale, out, nullptr, stream);
  if (!workspace || !aligned(workspace, 16)) return BNN_HIP_ERR_INVALID_ARG;
  int Ho, Wo;
  int st = check_desc(d, &Ho, &Wo);
  if (st != BNN_HIP_OK) return st;
  char* ws = static_cast<char*>(workspace);
  uint64_t* P = reinterpret_cast<uint64_t*>(ws);
  uint64_t* M = reinterpret_cast<uint64_t*>(ws + conv_plane_bytes(d));
  st = bnn_hip_pack_act_f32(x, d->N, d->C, d->H, d->W, P, M, stream);
  if (st != BNN_HIP_OK) return st;
  return bnn_hip_bconv2d(d, P, M, wbits, wnz, alpha, bias, post_scale, out, stream);
}

int bnn_hip_probe_int_alu(int mode, int iters, double* lane_ops_per_s, double* elapsed_ms,
                          void* stream) {
  if (iters <= 0 || !lane_ops_per_s) return BNN_HIP_ERR_INVALID_ARG;
  return bnn::launch_probe_int_alu(mode, iters, lane_ops_per_s, elapsed_ms,
                                   static_cast<hipStream_t>(stream));
}

// ---- XNORWeightBinarizer under autograd: csrc/xnor_train.hip
int bnn_hip_xnor_weight_forward_f32(const float* w, int O, int C, int KH, int KW, int center, int compute_alpha,
                                    float* what, float* alpha, void* stream) {
  if (!w || !what || O <= 0 || C <= 0 || KH <= 0 || KW <= 0) return BNN_HIP_ERR_INVALID_ARG;
  if (mulc(KH, KW) > 1024) return BNN_HIP_ERR_UNSUPPORTED;
  if (mulc(O, C, KH, KW) > kMaxElems) return BNN_HIP_ERR_TOO_LARGE;
  if (!aligned(w, 4) || !aligned(what, 4)) return BNN_HIP_ERR_INVALID_ARG;
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_xnor_what(w, O, C, KH * KW, center != 0, compute_alpha != 0, what, alpha, static_cast<hipStream_t>(stream));
}

int bnn_hip_xnor_grad_pack_weight_f32(const float* w, int O, int C, int ksize, int center, int compute_alpha, void* packed,
                                      float* alpha, void* stream) {
  if (!w || !packed || !alpha || O <= 0 || C <= 0) return BNN_HIP_ERR_INVALID_ARG;
  if (!grad_ks_ok(ksize)) return BNN_HIP_ERR_UNSUPPORTED;
  if (mulc(O, C, ksize, ksize) > kMaxElems) return BNN_HIP_ERR_TOO_LARGE;
  if (!aligned(w, 4) || !aligned(packed, 16) || !aligned(alpha, 4)) return BNN_HIP_ERR_INVALID_ARG;
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_xnor_grad_pack(w, O, C, ksize, center != 0, compute_alpha != 0, packed, alpha,
                                    static_cast<hipStream_t>(stream));
}

int bnn_hip_xnor_weight_backward_f32(const float* w, const float* dwhat, int splits, int O, int C, int KH, int KW,
                                     int center, int compute_alpha, float* dw, void* stream) {
  if (!w || !dwhat || !dw || O <= 0 || C <= 0 || KH <= 0 || KW <= 0 || splits <= 0) return BNN_HIP_ERR_INVALID_ARG;
  if (mulc(KH, KW) > 1024) return BNN_HIP_ERR_UNSUPPORTED;
  if (mulc(O, C, KH, KW) > kMaxElems || mulc(mulc(O, C, KH, KW), splits) > 4 * kMaxElems) return BNN_HIP_ERR_TOO_LARGE;
  if (!aligned(w, 4) || !aligned(dwhat, 4) || !aligned(dw, 4)) return BNN_HIP_ERR_INVALID_ARG;
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_xnor_weight_bwd(w, dwhat, splits, O, C, KH * KW, center != 0, compute_alpha != 0, dw,
                                     static_cast<hipStream_t>(stream));
}

// ---- training-mode BatchNorm (+ residual) (+ ReLU): csrc/bn_train.hip
static int check_bn(int N, int C, int HW) {
  if (N <= 0 || C <= 0 || HW <= 0) return BNN_HIP_ERR_INVALID_ARG;
  if (mulc(N, C, HW) > 4 * kMaxElems || mulc(N, HW) > kMaxElems || C > (1 << 20)) return BNN_HIP_ERR_TOO_LARGE;
  return BNN_HIP_OK;
}

size_t bnn_hip_bn_train_workspace_bytes(int N, int C, int HW) {
  return check_bn(N, C, HW) == BNN_HIP_OK ? bn_workspace(N, C, HW, nullptr).bytes : 0;
}

int bnn_hip_bn_train_forward_f32(const float* x, int N, int C, int HW, const float* gamma, const float* beta,
                                 const float* residual, int relu, float eps, float momentum, float* running_mean,
                                 float* running_var, float* y, float* save_mean, float* save_invstd, void* workspace,
                                 void* stream) {
  if (!x || !y || !save_mean || !save_invstd || !workspace) return BNN_HIP_ERR_INVALID_ARG;
  const int st = check_bn(N, C, HW);
  if (st != BNN_HIP_OK) return st;
  if ((running_mean == nullptr) != (running_var == nullptr) || !(eps >= 0.0f)) return BNN_HIP_ERR_INVALID_ARG;
  if (!aligned(x, 4) || !aligned(y, 4) || (residual && !aligned(residual, 4)) || !aligned(workspace, 8))
    return BNN_HIP_ERR_INVALID_ARG;
  const BnWorkspace ws = bn_workspace(N, C, HW, workspace);
  g_launches.fetch_add(3, std::memory_order_relaxed);
  BNN_RANGE();
  const int st2 = bnn::launch_bn_stats(x, N, C, HW, ws.splits, ws.partial, static_cast<hipStream_t>(stream));
  if (st2 != BNN_HIP_OK) return st2;
  return bnn::launch_bn_apply(x, ws.partial, ws.splits, gamma, beta, residual, relu, y, N, C, HW, eps, momentum, running_mean,
                              running_var, save_mean, save_invstd, ws.work, static_cast<hipStream_t>(stream));
}

int bnn_hip_bn_train_pack_ste_f32(const float* x, int N, int C, int H, int W, const float* gamma, const float* beta,
                                  float eps, float momentum, float* running_mean, float* running_var, uint64_t* P,
                                  uint64_t* M, uint64_t* T, float* save_mean, float* save_invstd, float* scale, float* shift,
                                  void* workspace, void* stream) {
  if (!T || !save_mean || !save_invstd || !scale || !shift || !workspace) return BNN_HIP_ERR_INVALID_ARG;
  const int stp = check_pack(x, 4, N, C, H, W, P, M);
  if (stp != BNN_HIP_OK) return stp;
  const int HW = checked_hw(H, W);
  const int st = check_bn(N, C, HW);
  if (st != BNN_HIP_OK) return st;
  if ((running_mean == nullptr) != (running_var == nullptr) || !(eps >= 0.0f)) return BNN_HIP_ERR_INVALID_ARG;
  if (!aligned(T, 8) || !aligned(scale, 4) || !aligned(shift, 4) || !aligned(save_mean, 4) || !aligned(save_invstd, 4) ||
      !aligned(workspace, 8))
    return BNN_HIP_ERR_INVALID_ARG;
  const BnWorkspace ws = bn_workspace(N, C, HW, workspace);
  g_launches.fetch_add(3, std::memory_order_relaxed);
  BNN_RANGE();
  hipStream_t s = static_cast<hipStream_t>(stream);
  int st2 = bnn::launch_bn_stats(x, N, C, HW, ws.splits, ws.partial, s);
  if (st2 != BNN_HIP_OK) return st2;
  st2 = bnn::launch_bn_finalize(ws.partial, ws.splits, gamma, beta, N, C, HW, eps, momentum, running_mean, running_var,
                                save_mean, save_invstd, scale, shift, s);
  if (st2 != BNN_HIP_OK) return st2;
  return bnn::launch_bn_pack_ste(x, N, C, H, W, scale, shift, P, M, T, s);
}

int bnn_hip_bn_train_pack_ste_s2_f32(const float* x, int N, int C, int H, int W, const float* gamma, const float* beta,
                                     float eps, float momentum, float* running_mean, float* running_var, uint64_t* P,
                                     uint64_t* M, uint64_t* T, float* save_mean, float* save_invstd, float* scale,
                                     float* shift, void* workspace, void* stream) {
  if (!T || !save_mean || !save_invstd || !scale || !shift || !workspace) return BNN_HIP_ERR_INVALID_ARG;
  const int stp = check_pack(x, 4, N, C, H, W, P, M);
  if (stp != BNN_HIP_OK) return stp;
  if (check_lattice(H, W) != BNN_HIP_OK) return BNN_HIP_ERR_INVALID_ARG;
  const int HW = checked_hw(H, W);
  const int st = check_bn(N, C, HW);
  if (st != BNN_HIP_OK) return st;
  if ((running_mean == nullptr) != (running_var == nullptr) || !(eps >= 0.0f)) return BNN_HIP_ERR_INVALID_ARG;
  if (!aligned(T, 8) || !aligned(scale, 4) || !aligned(shift, 4) || !aligned(save_mean, 4) || !aligned(save_invstd, 4) ||
      !aligned(workspace, 8))
    return BNN_HIP_ERR_INVALID_ARG;
  const BnWorkspace ws = bn_workspace(N, C, HW, workspace);
  g_launches.fetch_add(3, std::memory_order_relaxed);
  BNN_RANGE();
  hipStream_t s = static_cast<hipStream_t>(stream);
  int st2 = bnn::launch_bn_stats(x, N, C, HW, ws.splits, ws.partial, s);
  if (st2 != BNN_HIP_OK) return st2;
  st2 = bnn::launch_bn_finalize(ws.partial, ws.splits, gamma, beta, N, C, HW, eps, momentum, running_mean, running_var,
                                save_mean, save_invstd, scale, shift, s);
  if (st2 != BNN_HIP_OK) return st2;
  return bnn::launch_bn_pack_ste_s2(x, N, C, H, W, scale, shift, P, M, T, s);
}

int bnn_hip_bn_act_f32(const float* x, int N, int C, int HW, const float* scale, const float* shift, const float* residual,
                       int relu, float* y, void* stream) {
  if (!x || !y || !scale || !shift) return BNN_HIP_ERR_INVALID_ARG;
  const int st = check_bn(N, C, HW);
  if (st != BNN_HIP_OK) return st;
  if (!aligned(x, 4) || !aligned(y, 4) || !aligned(scale, 4) || !aligned(shift, 4) || (residual && !aligned(residual, 4)))
    return BNN_HIP_ERR_INVALID_ARG;
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_bn_act(x, scale, shift, residual, relu, y, N, C, HW, static_cast<hipStream_t>(stream));
}

int bnn_hip_bn_train_backward_f32(const float* gy, const float* y, const float* x, const float* save_mean,
                                  const float* save_invstd, const float* gamma, int N, int C, int HW, float* dx,
                                  float* dres, float* dgamma, float* dbeta, void* workspace, void* stream) {
  if (!gy || !x || !save_mean || !save_invstd || !dx || !workspace) return BNN_HIP_ERR_INVALID_ARG;
  const int st = check_bn(N, C, HW);
  if (st != BNN_HIP_OK) return st;
  if (!aligned(gy, 4) || !aligned(x, 4) || !aligned(dx, 4) || (y && !aligned(y, 4)) || (dres && !aligned(dres, 4)) ||
      !aligned(workspace, 8))
    return BNN_HIP_ERR_INVALID_ARG;
  const BnWorkspace ws = bn_workspace(N, C, HW, workspace);
  g_launches.fetch_add(3, std::memory_order_relaxed);
  BNN_RANGE();
  const int st2 = bnn::launch_bn_bwd_reduce(gy, y, x, save_mean, save_invstd, N, C, HW, ws.splits, ws.partial,
                                            static_cast<hipStream_t>(stream));
  if (st2 != BNN_HIP_OK) return st2;
  return bnn::launch_bn_bwd_dx(gy, y, x, save_mean, save_invstd, gamma, ws.partial, ws.splits, dx, dres, dgamma, dbeta, N, C,
                               HW, ws.work, static_cast<hipStream_t>(stream));
}

int bnn_hip_bn_train_backward_add_f32(const float* gy, const float* y, const float* x, const float* save_mean,
                                      const float* save_invstd, const float* gamma, const float* addend, int N, int C,
                                      int HW, float* dx, float* dgamma, float* dbeta, void* workspace, void* stream) {
  if (!addend)    // no skip: the existing backward, bit for bit
    return bnn_hip_bn_train_backward_f32(gy, y, x, save_mean, save_invstd, gamma, N, C, HW, dx, nullptr, dgamma, dbeta,
                                         workspace, stream);
  if (!gy || !x || !save_mean || !save_invstd || !dx || !workspace) return BNN_HIP_ERR_INVALID_ARG;
  const int st = check_bn(N, C, HW);
  if (st != BNN_HIP_OK) return st;
  if (!aligned(gy, 4) || !aligned(x, 4) || !aligned(dx, 4) || (y && !aligned(y, 4)) || !aligned(addend, 4) ||
      !aligned(workspace, 8))
    return BNN_HIP_ERR_INVALID_ARG;
  const BnWorkspace ws = bn_workspace(N, C, HW, workspace);
  g_launches.fetch_add(3, std::memory_order_relaxed);
  BNN_RANGE();
  const int st2 = bnn::launch_bn_bwd_reduce(gy, y, x, save_mean, save_invstd, N, C, HW, ws.splits, ws.partial,
                                            static_cast<hipStream_t>(stream));
  if (st2 != BNN_HIP_OK) return st2;
  return bnn::launch_bn_bwd_dx_add(gy, y, x, save_mean, save_invstd, gamma, ws.partial, ws.splits, addend, dx, dgamma, dbeta,
                                   N, C, HW, ws.work, static_cast<hipStream_t>(stream));
}

int bnn_hip_bn_train_backward_s2_f32(const float* g0, const float* g1, const float* x, const float* save_mean,
                                     const float* save_invstd, const float* gamma, int N, int C, int H, int W, float* dx,
                                     float* dgamma, float* dbeta, void* workspace, void* stream) {
  if (!g0 || !g1 || !x || !save_mean || !save_invstd || !dx || !workspace || H <= 0 || W <= 0) return BNN_HIP_ERR_INVALID_ARG;
  if (check_lattice(H, W) != BNN_HIP_OK) return BNN_HIP_ERR_INVALID_ARG;
  const int HW = checked_hw(H, W);
  const int st = check_bn(N, C, HW);
  if (st != BNN_HIP_OK) return st;
  // (x and dx are read and written as rows of float2 at least: W is even, so 8-byte bases keep every row aligned)
  if (!aligned(g0, 4) || !aligned(g1, 4) || !aligned(x, 8) || !aligned(dx, 8) || !aligned(workspace, 8))
    return BNN_HIP_ERR_INVALID_ARG;
  const BnWorkspace ws = bn_workspace(N, C, HW, workspace);
  g_launches.fetch_add(3, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_bn_bwd_s2(g0, g1, x, save_mean, save_invstd, gamma, N, C, H, W, ws.splits, ws.partial, ws.work, dx,
                               dgamma, dbeta, static_cast<hipStream_t>(stream));
}

// ---- backward of channel_shuffle(PReLU(z), shuffle_groups): csrc/prelu_bwd.hip
size_t bnn_hip_prelu_shuffle_backward_workspace_bytes(int N, int O, int HW) {
  return check_bn(N, O, HW) == BNN_HIP_OK ? (size_t)O * bnn::bn_train_splits(N, O, HW) * sizeof(double) : 0;
}

int bnn_hip_prelu_shuffle_backward_f32(const float* gy, const float* z, const float* slope, int slope_count, int N, int O,
                                       int HW, int shuffle_groups, float* gz, float* dslope, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  if (!gy || !z || !slope || !gz || !dslope || !workspace) return BNN_HIP_ERR_INVALID_ARG;
  const int st = check_bn(N, O, HW);
  if (st != BNN_HIP_OK) return st;
  if ((slope_count != 1 && slope_count != O) || shuffle_groups <= 0 || O % shuffle_groups != 0) return BNN_HIP_ERR_INVALID_ARG;
  if (gz == gy) return BNN_HIP_ERR_INVALID_ARG;   // (gz may be z: same index read and written by one thread; gy is read shuffled)
  if (!aligned(gy, 4) || !aligned(z, 4) || !aligned(slope, 4) || !aligned(gz, 4) || !aligned(dslope, 4) || !aligned(workspace, 8))
    return BNN_HIP_ERR_INVALID_ARG;
  const int splits = bnn::bn_train_splits(N, O, HW);
  if (workspace_bytes < (size_t)O * splits * sizeof(double)) return BNN_HIP_ERR_INVALID_ARG;
  g_launches.fetch_add(2, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_prelu_shuffle_bwd(gy, z, slope, slope_count, N, O, HW, shuffle_groups, splits, gz, dslope,
                                       static_cast<double*>(workspace), static_cast<hipStream_t>(stream));
}

int bnn_hip_bn_relu_maxpool_train_forward_f32(const float* x, int N, int C, int H, int W, const float* gamma,
                                              const float* beta, float eps, float momentum, float* running_mean,
                                              float* running_var, float* pooled, uint8_t* code, float* save_mean,
                                              float* save_invstd, void* workspace, void* stream) {
  if (!x || !pooled || !code || !save_mean || !save_invstd || !workspace || H <= 0 || W <= 0) return BNN_HIP_ERR_INVALID_ARG;
  const int HW = checked_hw(H, W);
  const int st = check_bn(N, C, HW);
  if (st != BNN_HIP_OK) return st;
  if ((running_mean == nullptr) != (running_var == nullptr) || !(eps >= 0.0f)) return BNN_HIP_ERR_INVALID_ARG;
  if (!aligned(x, 4) || !aligned(pooled, 4) || !aligned(workspace, 8)) return BNN_HIP_ERR_INVALID_ARG;
  const BnWorkspace ws = bn_workspace(N, C, HW, workspace);
  g_launches.fetch_add(3, std::memory_order_relaxed);
  BNN_RANGE();
  const int st2 = bnn::launch_bn_stats(x, N, C, HW, ws.splits, ws.partial, static_cast<hipStream_t>(stream));
  if (st2 != BNN_HIP_OK) return st2;
  return bnn::launch_bn_relu_pool_fwd(x, ws.partial, ws.splits, gamma, beta, pooled, code, N, C, H, W, eps, momentum,
                                      running_mean, running_var, save_mean, save_invstd, ws.work,
                                      static_cast<hipStream_t>(stream));
}

int bnn_hip_bn_relu_maxpool_train_backward_f32(const float* gy, const float* pooled, const uint8_t* code, const float* x,
                                               const float* save_mean, const float* save_invstd, const float* gamma,
                                               int N, int C, int H, int W, float* dx, float* dgamma, float* dbeta,
                                               void* workspace, void* stream) {
  if (!gy || !pooled || !code || !x || !save_mean || !save_invstd || !dx || !workspace || H <= 0 || W <= 0)
    return BNN_HIP_ERR_INVALID_ARG;
  const int HW = checked_hw(H, W);
  const int st = check_bn(N, C, HW);
  if (st != BNN_HIP_OK) return st;
  if (!aligned(gy, 4) || !aligned(pooled, 4) || !aligned(x, 4) || !aligned(dx, 4) || !aligned(workspace, 8))
    return BNN_HIP_ERR_INVALID_ARG;
  const BnWorkspace ws = bn_workspace(N, C, HW, workspace);
  g_launches.fetch_add(3, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_bn_relu_pool_bwd(gy, pooled, code, x, save_mean, save_invstd, gamma, N, C, H, W, ws.splits, ws.partial,
                                      ws.work, dx, dgamma, dbeta, static_cast<hipStream_t>(stream));
}

// ---- the hierarchical block in one launch (csrc/hblock.hip) ----
static int check_hblock(const bnn_hip_hblock_desc* d) {
  if (!d) return BNN_HIP_ERR_INVALID_ARG;
  if (d->N <= 0 || d->C_in <= 0 || d->H <= 0 || d->W <= 0 || d->planes <= 0) return BNN_HIP_ERR_INVALID_ARG;
  if (d->rows_per_band < 0 || d->images_per_band < 0 || d->waves < 0 || d->waves > 16) return BNN_HIP_ERR_INVALID_ARG;
  if (d->flags & ~(BNN_HIP_FLAG_THROUGHPUT | BNN_HIP_HBLOCK_CHANNEL_LANES)) return BNN_HIP_ERR_INVALID_ARG;
  // the kernel's index arithmetic: 24-bit multiplies, 32-bit byte offsets into the fp32 tensors
  const long long lim = 1ll << 23;
  if (mulc(d->N, d->planes) >= lim || mulc(d->H, d->W) >= lim || mulc(d->H + 8, d->W + 2) >= lim) return BNN_HIP_ERR_TOO_LARGE;
  if (mulc(d->N, d->planes, d->H, d->W) > kMaxConvElems) return BNN_HIP_ERR_TOO_LARGE;
  if (mulc(d->N, ((long long)d->C_in + 63) / 64, d->H, d->W) > kMaxPlaneWords) return BNN_HIP_ERR_TOO_LARGE;
  return BNN_HIP_OK;
}

// Whether the form of a kernel the descriptor selects (channel lanes: lanes = output channels, else pixels) covers it.
using hblock_rule = bool (*)(const bnn_hip_hblock_desc*);
static bool hblock_form_supported(const bnn_hip_hblock_desc* d, hblock_rule channel_lanes, hblock_rule pixel_lanes) {
  return (d->flags & BNN_HIP_HBLOCK_CHANNEL_LANES) ? channel_lanes(d) : pixel_lanes(d);
}
// the channel-lane kernels move two pixels per access of an fp32 tensor on 14-wide rows
static bool hblock_fp32_aligned(const bnn_hip_hblock_desc* d, const float* t) {
  return !(d->flags & BNN_HIP_HBLOCK_CHANNEL_LANES) || d->W != 14 || aligned(t, 8);
}
// the operands every forward entry point takes: input planes, the dense weights, the constants buffer
static bool hblock_operands_ok(const uint64_t* in_P, const uint32_t* weights, const float* consts) {
  return in_P && weights && consts && aligned(in_P, 8) && aligned(weights, 64) && aligned(consts, 32);
}
// bnn_hip_hblock_pack_weights and _pack_weights_cl: the three standard packs in, one 64-byte aligned buffer out
static int check_hblock_pack(int C_in, int planes, const uint32_t* const w[3], const uint32_t* weights) {
  if (!w[0] || !w[1] || !w[2] || !weights || C_in <= 0 || planes <= 0) return BNN_HIP_ERR_INVALID_ARG;
  if (!aligned(w[0], 4) || !aligned(w[1], 4) || !aligned(w[2], 4) || !aligned(weights, 64)) return BNN_HIP_ERR_INVALID_ARG;
  return BNN_HIP_OK;
}

int bnn_hip_hblock_supported(const bnn_hip_hblock_desc* d) {
  if (check_hblock(d) != BNN_HIP_OK) return 0;
  return hblock_form_supported(d, bnn::hblock_cl_supported, bnn::hblock_supported) ? 1 : 0;
}

int bnn_hip_hblock_layout_of(int C_in, int planes, bnn_hip_hblock_layout* out) {
  if (!out || C_in <= 0 || planes <= 0) return BNN_HIP_ERR_INVALID_ARG;
  std::memset(out, 0, sizeof(*out));
  return bnn::hblock_layout(C_in, planes, out);
}

int bnn_hip_hblock_pack_weights(int C_in, int planes, const uint32_t* wbits1, const uint32_t* wbits2,
                                const uint32_t* wbits3, uint32_t* weights, void* stream) {
  const uint32_t* const w[3] = {wbits1, wbits2, wbits3};
  const int st = check_hblock_pack(C_in, planes, w, weights);
  if (st != BNN_HIP_OK) return st;
  g_launches.fetch_add(3, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_hblock_pack_weights(C_in, planes, w, weights, static_cast<hipStream_t>(stream));
}

int bnn_hip_hblock_pack_weights_cl(int C_in, int planes, const uint32_t* wbits1, const uint32_t* wbits2,
                                   const uint32_t* wbits3, uint32_t* weights, void* stream) {
  const uint32_t* const w[3] = {wbits1, wbits2, wbits3};
  const int st = check_hblock_pack(C_in, planes, w, weights);
  if (st != BNN_HIP_OK) return st;
  g_launches.fetch_add(3, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_hblock_cl_pack_weights(C_in, planes, w, weights, static_cast<hipStream_t>(stream));
}

int bnn_hip_hblock_forward(const bnn_hip_hblock_desc* d, const uint64_t* in_P, const uint32_t* weights,
                           const float* consts, const float* residual, float* out, uint64_t* out_P, void* stream) {
  const int st = check_hblock(d);
  if (st != BNN_HIP_OK) return st;
  if (!hblock_operands_ok(in_P, weights, consts) || !residual || !out || residual == out) return BNN_HIP_ERR_INVALID_ARG;
  if (!aligned(residual, 4) || !aligned(out, 4) || (out_P && !aligned(out_P, 8))) return BNN_HIP_ERR_INVALID_ARG;
  if (!hblock_form_supported(d, bnn::hblock_cl_supported, bnn::hblock_supported)) return BNN_HIP_ERR_UNSUPPORTED;
  if (!hblock_fp32_aligned(d, residual) || !hblock_fp32_aligned(d, out)) return BNN_HIP_ERR_INVALID_ARG;
  const bool cl = (d->flags & BNN_HIP_HBLOCK_CHANNEL_LANES) != 0;
  g_launches.fetch_add(1, std::memory_order_relaxed);
  Range range(cl ? "bnn_hip_hblock_forward(channel lanes)" : __func__);
  return (cl ? bnn::launch_hblock_cl : bnn::launch_hblock)(d, in_P, weights, consts, residual, out, out_P,
                                                           static_cast<hipStream_t>(stream));
}

int bnn_hip_hblock_pool_supported(const bnn_hip_hblock_desc* d) {
  if (check_hblock(d) != BNN_HIP_OK || (d->flags & BNN_HIP_HBLOCK_CHANNEL_LANES)) return 0;
  return bnn::hblock_pool_supported(d) ? 1 : 0;
}

int bnn_hip_hblock_pool_forward(const bnn_hip_hblock_desc* d, const uint64_t* in_P, const uint32_t* weights,
                                const float* consts, const float* pool_consts, const float* residual, uint64_t* out_P1,
                                uint64_t* out_P2, uint64_t* out_M2, void* stream) {
  const int st = check_hblock(d);
  if (st != BNN_HIP_OK) return st;
  if (d->flags & BNN_HIP_HBLOCK_CHANNEL_LANES) return BNN_HIP_ERR_INVALID_ARG;
  if (!hblock_operands_ok(in_P, weights, consts) || !pool_consts || !residual || !out_P1 || !out_P2 || !out_M2)
    return BNN_HIP_ERR_INVALID_ARG;
  if (!aligned(pool_consts, 32) || !aligned(residual, 4) || !aligned(out_P1, 8) || !aligned(out_P2, 8) || !aligned(out_M2, 8))
    return BNN_HIP_ERR_INVALID_ARG;
  if (!bnn::hblock_pool_supported(d)) return BNN_HIP_ERR_UNSUPPORTED;
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_hblock_pool(d, in_P, weights, consts, pool_consts, residual, out_P1, out_P2, out_M2,
                                 static_cast<hipStream_t>(stream));
}

int bnn_hip_hblock_shortcut_supported(const bnn_hip_hblock_desc* d) {
  if (check_hblock(d) != BNN_HIP_OK) return 0;
  return hblock_form_supported(d, bnn::hblock_cl_ds_supported, bnn::hblock_ds_supported) ? 1 : 0;
}

int bnn_hip_hblock_pack_shortcut_weights(int C_in, int planes, const uint32_t* wbits, uint32_t* weights, void* stream) {
  if (!wbits || !weights || C_in <= 0 || planes <= 0) return BNN_HIP_ERR_INVALID_ARG;
  if (!aligned(wbits, 4) || !aligned(weights, 32)) return BNN_HIP_ERR_INVALID_ARG;
  g_launches.fetch_add(1, std::memory_order_relaxed);
  BNN_RANGE();
  return bnn::launch_hblock_ds_pack_weights(C_in, planes, wbits, weights, static_cast<hipStream_t>(stream));
}

int bnn_hip_hblock_shortcut_forward(const bnn_hip_hblock_desc* d, const uint64_t* in_P, const uint32_t* weights,
                                    const float* consts, const uint64_t* sc_P, const uint64_t* sc_M,
                                    const uint32_t* sc_weights, const float* sc_alpha, float* out, uint64_t* out_P,
                                    void* stream) {
  const int st = check_hblock(d);
  if (st != BNN_HIP_OK) return st;
  if (!hblock_operands_ok(in_P, weights, consts) || !sc_P || !sc_M || !sc_weights || !sc_alpha || !out || !out_P)
    return BNN_HIP_ERR_INVALID_ARG;
  if (!aligned(sc_P, 8) || !aligned(sc_M, 8) || !aligned(sc_weights, 32) || !aligned(sc_alpha, 32) || !aligned(out, 4) ||
      !aligned(out_P, 8))
    return BNN_HIP_ERR_INVALID_ARG;
  if (!hblock_form_supported(d, bnn::hblock_cl_ds_supported, bnn::hblock_ds_supported)) return BNN_HIP_ERR_UNSUPPORTED;
  if (!hblock_fp32_aligned(d, out)) return BNN_HIP_ERR_INVALID_ARG;
  const bool cl = (d->flags & BNN_HIP_HBLOCK_CHANNEL_LANES) != 0;   // (weights: then those of bnn_hip_hblock_pack_weights_cl)
  g_launches.fetch_add(1, std::memory_order_relaxed);
  Range range(cl ? "bnn_hip_hblock_shortcut_forward(channel lanes)" : __func__);
  return (cl ? bnn::launch_hblock_cl_ds : bnn::launch_hblock_ds)(d, in_P, weights, consts, sc_P, sc_M, sc_weights, sc_alpha,
                                                                 out, out_P, static_cast<hipStream_t>(stream));
}

int bnn_hip_probe_clock(int spin_iters, double* shader_mhz, double* elapsed_us, void* stream) {
  if (spin_iters <= 0 || spin_iters > (1 << 24) || !shader_mhz) return BNN_HIP_ERR_INVALID_ARG;
  return bnn::launch_probe_clock(spin_iters, shader_mhz, elapsed_us, static_cast<hipStream_t>(stream));
}

}  // extern "C"

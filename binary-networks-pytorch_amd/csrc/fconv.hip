// fconv.hip — the BATS FactorizedConv (bnn/models/layers/bats_ops.py:55-75, 'conv_7x1_1x7') in ONE launch.
//
//     y = [x +] channel_shuffle(PReLU(conv_Kx1(sign(BatchNorm(PReLU(conv_1xK(sign(BatchNorm(x)))))))), 4)
//
// Two DENSE binary convolutions, 1 x K with stride (1, s) and K x 1 with stride (s, 1), and between them only
// sign(BatchNorm(PReLU(.))) — one bit pair per element.  The launch reads the planes of sign(BatchNorm(x))
// (bnn_hip_bn_act_pack_f32) and the two weight packs of bnn_hip_pack_weight_f32, and writes the fp32 result; the
// intermediate tensor t lives in LDS as two bit planes and never reaches global memory, as a float or otherwise.
// The arithmetic is stated in include/bnn_hip.h (bnn_hip_fconv_fused); every float operation is the one the
// per-layer launches do (bconv_core.h: epilogue), so the result equals their composition bit for bit.
//
// Work decomposition: a workgroup takes a band of `R` output rows of one image (the whole image where its planes fit
// the LDS budget).  Phase 1 computes the s (rows - 1) + K rows of t the band reads, halo included; rows outside the
// image are all-zero planes, written and never computed (the K x 1 convolution's zero padding is applied AFTER sign():
// bnn/layers/conv.py:91-92), not the sign of a padded dot.  After one barrier phase 2 runs the second convolution from
// LDS.  In both phases lanes are pixels (64 consecutive pixels of the band: loads and stores of one channel are
// contiguous), a wave takes one (64-pixel tile, 32-channel block) item at a time, and the weights are a wave-uniform
// stream through the scalar cache (s_load_dwordx16), as in bconv_core.h.  The sign bits of a 32-channel block are
// collected into one word per lane and stored as one half of the pixel's 64-channel word, as the hierarchical-block
// kernels do; phase 2 reads whole 64-bit words (ds_read_b64).  No atomics: two runs give the same bits.
//
// Weight layout (include/bnn_hip.h): wbits[ob][chunk][j][tap][cwc].  For a 1 x K / K x 1 weight with K > 1 cwc is 2,
// i.e. chunk = the 64-channel word g, and the 32 x K x 2 words of one (ob, g) are contiguous: 4 K blocks of 16.
// K == 1 (two 1 x 1 convolutions) has the wider chunks of the 1 x 1 layout: its two words per channel are fetched
// one channel at a time.
//
// LDS: 2 planes x ceil(C/64) words x mid_rows x Wm pixels x 8 bytes; kFcLdsBudget bounds it (no opt-in to more than
// the default 64 KB of dynamic LDS is needed).  fconv_supported() says what fits.
#include <algorithm>

#include "bconv_core.h"

namespace bnn {

namespace {

constexpr int kFcLdsBudget = 64 * 1024;
constexpr int kFcMaxWaves = 16;

extern __shared__ __attribute__((aligned(16))) unsigned char fc_smem[];

struct FcGeo {
  int N, C, H, W;     // input planes [N, cw64, H, W]
  int s;              // stride
  int Wm, Ho;         // t is [N, C, H, Wm]; the output [N, C, Ho, Wm]
  int cw64, nob;      // 64-channel words per pixel, 32-channel blocks that hold a channel
  int R, bands;       // output rows per band, bands per image
  int plane;          // LDS words of one (plane, g): mid rows of a full band x Wm
  int sg, cpg;        // shuffle groups, C / sg
  int cwc, nchunk;    // weight layout (K == 1 only: cwc may exceed 2)
};

__device__ __forceinline__ int fc_uniform(int v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_readfirstlane(v);
#else
  return v;
#endif
}

// The zero-aware XNOR dots of one 64-channel word g of a lane's K taps (pw / mw: word f = 2 tap + half) with the 32
// output channels of block ob: acc[j] += disagreeing non-zero positions; WZ: nzw[j] += non-zero products.
template <int K, bool WZ>
__device__ __forceinline__ void fc_dots(const uint32_t* __restrict__ W, const uint32_t* __restrict__ Z, const FcGeo& g,
                                        const int ob, const int gw, const uint32_t (&pw)[2 * K],
                                        const uint32_t (&mw)[2 * K], int (&acc)[kOCB], int (&nzw)[kOCB]) {
  if constexpr (K == 1) {
    // word 2 gw of the pixel lies in chunk (2 gw) / cwc at position (2 gw) % cwc (cwc even)
    const int ch = (2 * gw) / g.cwc, c0 = 2 * gw - ch * g.cwc;
    const size_t base = ((size_t)(ob * g.nchunk + ch) * kOCB) * g.cwc + c0;
    static_for<kOCB>([&](auto jc) {
      constexpr int j = decltype(jc)::value;
      uint32_t w[2], z[2] = {~0u, ~0u};
      load_words<2>(W, base + (size_t)j * g.cwc, w);
      if constexpr (WZ) load_words<2>(Z, base + (size_t)j * g.cwc, z);
#pragma unroll
      for (int f = 0; f < 2; ++f) {
        uint32_t d = disagree(w[f], mw[f], pw[f]);
        if constexpr (WZ) {
          d &= z[f];
          nzw[j] = popc_acc((pw[f] | mw[f]) & z[f], nzw[j]);
        }
        acc[j] = popc_acc(d, acc[j]);
      }
    });
  } else {
    const size_t base = (size_t)(ob * g.cw64 + gw) * (kOCB * 2 * K);
    const uint32_t* __restrict__ wrun = W + base;
    const uint32_t* __restrict__ zrun = Z + (WZ ? base : 0);
    static_for<4 * K>([&](auto bc) {
      constexpr int b = decltype(bc)::value;
      WStream<16> wv, zv;
      load_wblock<16>(wrun + 16 * b, wv);
      if constexpr (WZ) load_wblock<16>(zrun + 16 * b, zv);
      static_for<16>([&](auto ec) {
        constexpr int e = 16 * b + decltype(ec)::value;
        constexpr int j = e / (2 * K), f = e % (2 * K);
        uint32_t d = disagree(wv.v[e - 16 * b], mw[f], pw[f]);
        if constexpr (WZ) {
          d &= zv.v[e - 16 * b];
          nzw[j] = popc_acc((pw[f] | mw[f]) & zv.v[e - 16 * b], nzw[j]);
        }
        acc[j] = popc_acc(d, acc[j]);
      });
    });
  }
}

// v = fmaf(alpha[o], dot, bias[o]) [* post_scale[o]];  v = v >= 0 ? v : prelu[o] * v: the operations of bconv_core.h's
// epilogue, each rounded on its own.
__device__ __forceinline__ float fc_value(const bnn_hip_fconv_stage& st, const int o, const int dot) {
#pragma clang fp contract(off)
  float v = fmaf(st.alpha[o], (float)dot, st.bias ? st.bias[o] : 0.0f);
  if (st.post_scale) v *= st.post_scale[o];
  if (st.prelu) {
    const float neg = st.prelu[o] * v;
    v = (v >= 0.0f) ? v : neg;
  }
  return v;
}

template <int K, bool WZ>
__global__ __launch_bounds__(kFcMaxWaves* kWave) void fconv_kernel(
    const uint64_t* __restrict__ P, const uint64_t* __restrict__ M, const uint32_t* __restrict__ W1,
    const uint32_t* __restrict__ Z1, const uint32_t* __restrict__ W2, const uint32_t* __restrict__ Z2,
    const bnn_hip_fconv_stage s1, const bnn_hip_fconv_stage s2, const float* __restrict__ mid_a,
    const float* __restrict__ mid_b, const float* __restrict__ res, float* __restrict__ out, const FcGeo g) {
  uint64_t* const tP = reinterpret_cast<uint64_t*>(fc_smem);  // [cw64][plane]
  uint64_t* const tM = tP + (size_t)g.cw64 * g.plane;
  const int lane = (int)threadIdx.x & (kWave - 1);
  const int wave = fc_uniform((int)threadIdx.x >> 6);
  const int nwaves = (int)blockDim.x >> 6;
  const int n = (int)blockIdx.x / g.bands, band = (int)blockIdx.x - n * g.bands;
  const int yo0 = band * g.R;
  const int rows = min(g.R, g.Ho - yo0);       // output rows of this band
  const int mrows = g.s * (rows - 1) + K;      // rows of t it reads
  const int y0 = g.s * yo0 - K / 2;            // image row of t's row 0 (may be negative: zero planes)

  // ---- phase 1: t = sign(BN2(PReLU(conv_1xK(planes)))) of the band's rows, into LDS
  {
    // rows [r_lo, r_hi) of the band's t lie inside the image (never empty); the others are zero planes, written here
    // and never computed
    const int r_lo = max(0, -y0), r_hi = min(mrows, g.H - y0);
    {
      const int zr = mrows - (r_hi - r_lo), per_g = zr * g.Wm;
      for (int i = (int)threadIdx.x; i < g.cw64 * per_g; i += (int)blockDim.x) {
        const int gw = i / per_g, c = i - gw * per_g;
        const int zrow = c / g.Wm, xm = c - zrow * g.Wm;
        const int r = zrow < r_lo ? zrow : r_hi + (zrow - r_lo);
        const int cell = gw * g.plane + r * g.Wm + xm;
        tP[cell] = 0ull;
        tM[cell] = 0ull;
      }
    }
    const int npix = (r_hi - r_lo) * g.Wm;
    const int tiles = (npix + kWave - 1) / kWave;
    const int nhalf = 2 * g.cw64;  // 32-bit halves of a pixel's words: the blocks past the last channel are zero
    const int items = tiles * nhalf;
    for (int item = wave; item < items; item += nwaves) {
      const int tile = item / nhalf, ob = item - tile * nhalf;
      const int pix = tile * kWave + lane;
      const bool live = pix < npix;
      const int pc = live ? pix : npix - 1;
      const int r = pc / g.Wm, xm = pc - r * g.Wm;
      const int y = y0 + r_lo + r;  // inside the image
      uint32_t pb = 0u, mb = 0u;
      if (ob < g.nob) {  // wave-uniform
        int acc[kOCB], nzw[kOCB];
#pragma unroll
        for (int j = 0; j < kOCB; ++j) { acc[j] = 0; nzw[j] = 0; }
        int nz = 0;
        for (int gw = 0; gw < g.cw64; ++gw) {
          uint32_t pw[2 * K], mw[2 * K];
          const int rowbase = ((n * g.cw64 + gw) * g.H + y) * g.W;  // words: below 2^29 (capi.hip)
#pragma unroll
          for (int t = 0; t < K; ++t) {
            const int ix = g.s * xm + t - K / 2;
            const bool ok = (unsigned)ix < (unsigned)g.W;  // taps in the zero padding contribute P = M = 0
            const unsigned boff = (unsigned)(rowbase + (ok ? ix : 0)) * 8u;
            const uint64_t pv = ld_off(P, boff), mv = ld_off(M, boff);
            pw[2 * t] = ok ? (uint32_t)pv : 0u;
            pw[2 * t + 1] = ok ? (uint32_t)(pv >> 32) : 0u;
            mw[2 * t] = ok ? (uint32_t)mv : 0u;
            mw[2 * t + 1] = ok ? (uint32_t)(mv >> 32) : 0u;
          }
          if constexpr (!WZ) {
#pragma unroll
            for (int f = 0; f < 2 * K; ++f) nz = popc_acc(pw[f] | mw[f], nz);
          }
          fc_dots<K, WZ>(W1, Z1, g, ob, gw, pw, mw, acc, nzw);
        }
        const int o0 = ob * kOCB;
        static_for<kOCB>([&](auto jc) {
#pragma clang fp contract(off)
          constexpr int j = decltype(jc)::value;
          const int o = o0 + j;
          if (o < g.C) {  // wave-uniform; pad channels keep 0 in both planes
            const float v = fc_value(s1, o, (WZ ? nzw[j] : nz) - 2 * acc[j]);
            const float p = fmaf(v, mid_a[o], mid_b[o]);
            pb |= (is_pos(p) ? 1u : 0u) << j;
            mb |= (is_neg(p) ? 1u : 0u) << j;
          }
        });
      }
      if (live) {
        const unsigned cell = (unsigned)(ob >> 1) * (unsigned)g.plane + (unsigned)(r_lo * g.Wm + pix);
        reinterpret_cast<uint32_t*>(tP)[cell * 2u + (unsigned)(ob & 1)] = pb;
        reinterpret_cast<uint32_t*>(tM)[cell * 2u + (unsigned)(ob & 1)] = mb;
      }
    }
  }
  __syncthreads();

  // ---- phase 2: the K x 1 convolution of t from LDS, PReLU, shuffle, skip, fp32 store
  {
    const int npix = rows * g.Wm;
    const int tiles = (npix + kWave - 1) / kWave;
    const int items = tiles * g.nob;
    const int hw = g.Ho * g.Wm;
    for (int item = wave; item < items; item += nwaves) {
      const int tile = item / g.nob, ob = item - tile * g.nob;
      const int pix = tile * kWave + lane;
      const int pc = min(pix, npix - 1);
      const int ry = pc / g.Wm, xo = pc - ry * g.Wm;
      int acc[kOCB], nzw[kOCB];
#pragma unroll
      for (int j = 0; j < kOCB; ++j) { acc[j] = 0; nzw[j] = 0; }
      int nz = 0;
      for (int gw = 0; gw < g.cw64; ++gw) {
        uint32_t pw[2 * K], mw[2 * K];
        const int cell0 = gw * g.plane + g.s * ry * g.Wm + xo;  // every tap's row is inside the band's rows of t
#pragma unroll
        for (int t = 0; t < K; ++t) {
          const uint64_t pv = tP[cell0 + t * g.Wm], mv = tM[cell0 + t * g.Wm];
          pw[2 * t] = (uint32_t)pv;
          pw[2 * t + 1] = (uint32_t)(pv >> 32);
          mw[2 * t] = (uint32_t)mv;
          mw[2 * t + 1] = (uint32_t)(mv >> 32);
        }
        if constexpr (!WZ) {
#pragma unroll
          for (int f = 0; f < 2 * K; ++f) nz = popc_acc(pw[f] | mw[f], nz);
        }
        fc_dots<K, WZ>(W2, Z2, g, ob, gw, pw, mw, acc, nzw);
      }
      const int o0 = ob * kOCB;
      // o -> o' = (o % cpg) sg + o / cpg on the scalar unit: (q, r) of the block's first channel, then r counts up
      int q = o0 / g.cpg, rr = o0 - q * g.cpg;
      const unsigned lane_off = (unsigned)(n * g.C * hw + yo0 * g.Wm + pc) * 4u;  // BYTES; N C Ho Wo < 2^30 (capi.hip)
      static_for<kOCB>([&](auto jc) {
#pragma clang fp contract(off)
        constexpr int j = decltype(jc)::value;
        const int o = o0 + j;
        if (o < g.C) {  // wave-uniform
          float v = fc_value(s2, o, (WZ ? nzw[j] : nz) - 2 * acc[j]);
          const unsigned choff = (unsigned)(rr * g.sg + q) * (unsigned)hw * 4u;
          // (lanes past the band's last pixel were clamped to it: they store the same value to the same place)
          if (res) v = ld_off(reinterpret_cast<const float*>(reinterpret_cast<const char*>(res) + choff), lane_off) + v;
          st_off(reinterpret_cast<float*>(reinterpret_cast<char*>(out) + choff), lane_off, v);
          if (++rr == g.cpg) { rr = 0; ++q; }
        }
      });
    }
  }
}

// The band plan of a geometry: rows per band (the whole image where its planes of t fit the budget, else the most rows
// that do), LDS bytes, waves per workgroup.  false: not even one output row fits.
bool fc_plan(int C, int H, int W, int K, int s, FcGeo* g, size_t* lds, int* waves) {
  const int Wm = (W - 1) / s + 1, Ho = (H - 1) / s + 1;
  const long long cw64 = ((long long)C + 63) / 64;
  const long long row_bytes = 2 * cw64 * Wm * 8;  // one row of t, both planes
  if (row_bytes * K > kFcLdsBudget) return false;
  long long R = (kFcLdsBudget / row_bytes - K) / s + 1;  // s (R - 1) + K rows fit
  if (R > Ho) R = Ho;
  const int bands = (int)((Ho + R - 1) / R);
  R = (Ho + bands - 1) / bands;  // the same number of bands, evenly filled
  const int mid_rows = (int)(s * (R - 1) + K);
  if (g) {
    g->C = C; g->H = H; g->W = W; g->s = s; g->Wm = Wm; g->Ho = Ho;
    g->cw64 = (int)cw64; g->nob = (C + kOCB - 1) / kOCB;
    g->R = (int)R; g->bands = bands; g->plane = mid_rows * Wm;
  }
  if (lds) *lds = (size_t)(row_bytes * mid_rows);
  if (waves) {
    const long long items1 = ((long long)mid_rows * Wm + kWave - 1) / kWave * 2 * cw64;
    const long long items2 = (R * Wm + kWave - 1) / kWave * ((C + kOCB - 1) / kOCB);
    *waves = (int)std::min<long long>(kFcMaxWaves, std::max(items1, items2));
  }
  return true;
}

template <int K>
int fc_launch(const FconvP& p, const FcGeo& g, size_t lds, int waves, hipStream_t s) {
  const dim3 grid((unsigned)(p.N * g.bands)), block((unsigned)(waves * kWave));
  if (p.wz)
    hipLaunchKernelGGL((fconv_kernel<K, true>), grid, block, lds, s, p.P, p.M, p.W1, p.Z1, p.W2, p.Z2, p.s1, p.s2, p.mid_a,
                       p.mid_b, p.res, p.out, g);
  else
    hipLaunchKernelGGL((fconv_kernel<K, false>), grid, block, lds, s, p.P, p.M, p.W1, p.Z1, p.W2, p.Z2, p.s1, p.s2, p.mid_a,
                       p.mid_b, p.res, p.out, g);
  return hipGetLastError() == hipSuccess ? BNN_HIP_OK : BNN_HIP_ERR_LAUNCH;
}

}  // namespace

// What the kernel covers: K odd and at most 7, stride 1 or 2, and K rows of t within the LDS budget.  (Sizes and
// pointers are capi.hip's business.)
bool fconv_supported(int C, int H, int W, int K, int stride) {
  if (C <= 0 || H <= 0 || W <= 0 || K < 1 || K > 7 || K % 2 == 0 || (stride != 1 && stride != 2)) return false;
  return fc_plan(C, H, W, K, stride, nullptr, nullptr, nullptr);
}

// capi.hip has checked sizes (planes below 2^29 words, the fp32 tensors below 2^30 elements), pointers, alignments,
// shuffle_groups >= 1 dividing C, and fconv_supported().
int launch_fconv(const FconvP& p, hipStream_t s) {
  FcGeo g{};
  size_t lds = 0;
  int waves = 1;
  if (!fc_plan(p.C, p.H, p.W, p.K, p.stride, &g, &lds, &waves)) return BNN_HIP_ERR_UNSUPPORTED;
  g.N = p.N;
  g.sg = p.shuffle_groups;
  g.cpg = p.C / p.shuffle_groups;
  g.cwc = choose_cwc(2 * g.cw64, 1, p.K);
  g.nchunk = 2 * g.cw64 / g.cwc;
  switch (p.K) {
    case 1: return fc_launch<1>(p, g, lds, waves, s);
    case 3: return fc_launch<3>(p, g, lds, waves, s);
    case 5: return fc_launch<5>(p, g, lds, waves, s);
    case 7: return fc_launch<7>(p, g, lds, waves, s);
    default: return BNN_HIP_ERR_UNSUPPORTED;
  }
}

}  // namespace bnn

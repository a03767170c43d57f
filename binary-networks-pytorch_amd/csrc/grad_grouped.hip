// grad_grouped.hip — the two gradients of a GROUPED binary convolution in a training step, from the saved bit planes.
//
// Reference: the backward of bnn/layers/conv.py:90-97 with groups = G > 1 (the BATS cells' SepConv / DilConv,
// bnn/models/layers/bats_ops.py:108-173; depthwise layers) and the straight-through estimator of bnn/ops.py:63-73.
// Notation as in include/bnn_hip.h: Cg = C / G, Og = O / G, output channel o reads input channels of group o / Og.
//
//   input gradient    gx[n,c,y,x]         = T[n,c,y,x] ? sum_{o in group(c)} sum_{ky,kx} g[n,o,qy,qx] What[o, c mod Cg, ky, kx] : +0
//                                            qy = (y + pad - dil ky) / stride where that division is exact and 0 <= qy < Ho
//   weight gradient   part[s,o,cg,ky,kx]  = sum_{n in split s} sum_{y,x} g[n,o,y,x] sign(x)[n, (o / Og) Cg + cg, stride y + dil ky - pad, ..]
//
// Neither reads the fp32 input: T (|x| < 1) masks the input gradient, P / M (x > 0, x < 0) are sign(x) — the three
// planes of bnn_hip_pack_act_ste_f32.  Plain fp32 VALU: a group's reduction (Og KH KW terms; pixels) and its 1..32
// channels fill no MFMA tile, and g keeps its full fp32 precision without the three-way bf16 split of grad.hip.
// No atomics: every output element is written by one thread, sums run in a fixed order — two runs give the same bits.
// What capi.hip's check_grouped_grad lets through: Cg <= 32, KH, KW <= 7, one stride of 1 or 2, any width, dilation,
// padding and Og; g and gx below 2^30 elements.
#include "bnn_dev.h"

namespace bnn {

namespace {

constexpr int kOChunk = 32;   // output channels of a group whose What tile is staged in LDS at a time (dgrad)

// ---- input gradient: a workgroup = 256 pixels of one image x CT input channels of one group.  Lanes run along the
// image row (g loads and gx stores coalesced); the group's weights are wave-uniform: staged in LDS as
// [tap][o][CT] and read back as one broadcast vector per (tap, o).
template <int CT>
__global__ __launch_bounds__(256) void grouped_dgrad_kernel(const float* __restrict__ g, const float* __restrict__ what,
                                                            const uint64_t* __restrict__ T, float* __restrict__ gx,
                                                            GroupedGradP q, int ctiles, int ptiles) {
  extern __shared__ float4 dgrad_lds[];
  float* wl = reinterpret_cast<float*>(dgrad_lds);
  struct alignas(CT >= 4 ? 16 : 4 * CT) WV { float v[CT]; };
  unsigned b = blockIdx.x;
  const int tile = (int)(b % (unsigned)ptiles); b /= (unsigned)ptiles;
  const int c0 = (int)(b % (unsigned)ctiles) * CT; b /= (unsigned)ctiles;
  const int grp = (int)(b % (unsigned)q.G), n = (int)(b / (unsigned)q.G);
  const int Cg = q.C / q.G, Og = q.O / q.G, taps = q.KH * q.KW, HW = q.H * q.W, HoWo = q.Ho * q.Wo;
  const int p = tile * 256 + (int)threadIdx.x;
  const bool live = p < HW;
  const int y = live ? p / q.W : 0, x = live ? p - y * q.W : 0;
  const int sl = q.stride - 1;   // stride 1 or 2: the division is a shift
  const float* gb = g + ((size_t)n * q.O + (size_t)grp * Og) * HoWo;
  float acc[CT];
#pragma unroll
  for (int j = 0; j < CT; ++j) acc[j] = 0.0f;
  for (int o_base = 0; o_base < Og; o_base += kOChunk) {
    const int ob = Og - o_base < kOChunk ? Og - o_base : kOChunk;
    __syncthreads();   // (the previous chunk's tile has been read)
    for (int i = (int)threadIdx.x; i < taps * ob * CT; i += 256) {
      const int j = i % CT, o = (i / CT) % ob, t = i / (CT * ob);
      const int c = c0 + j < Cg ? c0 + j : Cg - 1;   // channels past the group: a copy nobody stores
      wl[i] = what[(((size_t)grp * Og + o_base + o) * Cg + c) * taps + t];
    }
    __syncthreads();
    if (live) {
      for (int ky = 0; ky < q.KH; ++ky) {
        const int ty = y + q.ph - q.dh * ky, qy = ty >> sl;
        if (ty < 0 || (qy << sl) != ty || qy >= q.Ho) continue;
        for (int kx = 0; kx < q.KW; ++kx) {
          const int tx = x + q.pw - q.dw * kx, qx = tx >> sl;
          if (tx < 0 || (qx << sl) != tx || qx >= q.Wo) continue;
          const float* gp = gb + (size_t)o_base * HoWo + (size_t)qy * q.Wo + qx;
          const WV* wv = reinterpret_cast<const WV*>(wl + (size_t)(ky * q.KW + kx) * ob * CT);
          for (int o = 0; o < ob; ++o) {
            const float gv = gp[(size_t)o * HoWo];
            const WV w = wv[o];
#pragma unroll
            for (int j = 0; j < CT; ++j) acc[j] = fmaf(gv, w.v[j], acc[j]);
          }
        }
      }
    }
  }
  if (!live) return;
  const int cw64 = (q.C + 63) / 64;
#pragma unroll
  for (int j = 0; j < CT; ++j) {
    if (c0 + j >= Cg) break;
    const int c = grp * Cg + c0 + j;
    const uint64_t tw = T[((size_t)n * cw64 + (c >> 6)) * HW + p];
    gx[((size_t)n * q.C + c) * HW + p] = ((tw >> (c & 63)) & 1ull) ? acc[j] : 0.0f;   // hard-tanh STE (bnn/ops.py:68-73)
  }
}

// ---- weight gradient: a workgroup = (group, OT output channels, TT taps, one split of the batch).  A thread owns one
// input channel cg of the group (its lane index modulo CGP = Cg rounded up to a power of two) and every (256 / CGP)-th
// output pixel of the split: per pixel it loads OT values of g, and per tap ONE 32-bit word of each sign plane, whose
// bit cg becomes the fp32 sign shared by the OT products.  The OT x TT accumulators of the threads with the same cg are
// added by a butterfly inside the wave and in wave order through LDS.
template <int OT, int TT>
__global__ __launch_bounds__(256) void grouped_wgrad_kernel(const float* __restrict__ g, const uint32_t* __restrict__ P,
                                                            const uint32_t* __restrict__ M, float* __restrict__ part,
                                                            GroupedGradP q, int otiles, int cgp_log2) {
  __shared__ float red[4][OT * TT][32];
  const int grp = (int)blockIdx.x / otiles, o0 = ((int)blockIdx.x % otiles) * OT;
  const int split = (int)blockIdx.y, splits = (int)gridDim.y, t0 = (int)blockIdx.z * TT;
  const int Cg = q.C / q.G, Og = q.O / q.G, taps = q.KH * q.KW, HW = q.H * q.W, HoWo = q.Ho * q.Wo;
  const int CGP = 1 << cgp_log2, PS = 256 >> cgp_log2;          // pixel slots of the workgroup
  const int tid = (int)threadIdx.x, cg = tid & (CGP - 1), slot = tid >> cgp_log2;
  const int c = grp * Cg + (cg < Cg ? cg : Cg - 1);             // (idle lanes of a padded group repeat its last channel)
  const int cw64 = (q.C + 63) / 64, bit = c & 31;
  const size_t word0 = (size_t)(c >> 6) * HW * 2 + ((c >> 5) & 1);   // 32-bit index of the lane's plane word at pixel 0 of image 0
  const int n0 = (int)((long long)split * q.N / splits), n1 = (int)((long long)(split + 1) * q.N / splits);
  const int npix = (n1 - n0) * HoWo;

  int dyo[TT], dxo[TT];   // input offset of each tap: dil k - pad
#pragma unroll
  for (int tt = 0; tt < TT; ++tt) {
    const int t = t0 + tt < taps ? t0 + tt : taps - 1;          // taps past the kernel: a copy nobody stores
    dyo[tt] = q.dh * (t / q.KW) - q.ph;
    dxo[tt] = q.dw * (t % q.KW) - q.pw;
  }
  size_t gofs[OT];        // element offset of each output channel's plane in image 0
#pragma unroll
  for (int j = 0; j < OT; ++j) gofs[j] = (size_t)(grp * Og + (o0 + j < Og ? o0 + j : Og - 1)) * HoWo;

  float acc[OT][TT];
#pragma unroll
  for (int j = 0; j < OT; ++j)
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) acc[j][tt] = 0.0f;

  // this thread's pixels: slot, slot + PS, ... as (image, row, column), advanced without a division
  int n = n0 + slot / HoWo, r = slot % HoWo, y = r / q.Wo, x = r % q.Wo;
  const int dn = PS / HoWo, dr = PS % HoWo, dy = dr / q.Wo, dx = dr % q.Wo;
  for (int pix = slot; pix < npix; pix += PS) {
    const float* gn = g + (size_t)n * q.O * HoWo + (size_t)y * q.Wo + x;
    float gv[OT];
#pragma unroll
    for (int j = 0; j < OT; ++j) gv[j] = gn[gofs[j]];
    const size_t wn = (size_t)n * cw64 * HW * 2 + word0;
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) {
      const int iy = y * q.stride + dyo[tt], ix = x * q.stride + dxo[tt];
      const bool in = (unsigned)iy < (unsigned)q.H && (unsigned)ix < (unsigned)q.W;   // taps outside the image add nothing
      const size_t wi = wn + (in ? ((size_t)iy * q.W + ix) * 2 : 0);
      const uint32_t pw = P[wi], mw = M[wi];
      const float s = in ? (float)((int)((pw >> bit) & 1u) - (int)((mw >> bit) & 1u)) : 0.0f;
#pragma unroll
      for (int j = 0; j < OT; ++j) acc[j][tt] = fmaf(gv[j], s, acc[j][tt]);
    }
    x += dx; if (x >= q.Wo) { x -= q.Wo; ++y; }
    y += dy; if (y >= q.Ho) { y -= q.Ho; ++n; }
    n += dn;
  }

  const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
  for (int j = 0; j < OT; ++j)
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) {
      float v = acc[j][tt];
      for (int off = 32; off >= CGP; off >>= 1) v += __shfl_xor(v, off);
      if (lane < CGP) red[wave][j * TT + tt][lane] = v;
    }
  __syncthreads();
  for (int i = tid; i < (OT * TT) << cgp_log2; i += 256) {
    const int a = i >> cgp_log2, ci = i & (CGP - 1), j = a / TT, tt = a % TT;
    if (o0 + j >= Og || t0 + tt >= taps || ci >= Cg) continue;
    const float v = ((red[0][a][ci] + red[1][a][ci]) + red[2][a][ci]) + red[3][a][ci];
    part[(((size_t)split * q.O + grp * Og + o0 + j) * Cg + ci) * taps + t0 + tt] = v;
  }
}

// channels per thread of the input gradient: the tile of 8 / 4 / 2 / 1 that wastes the fewest lanes on Cg (ties: wider)
int dgrad_tile(int Cg) {
  int best = 1, waste = 0;
  for (int ct = 2; ct <= 8; ct *= 2) {
    const int w = (Cg + ct - 1) / ct * ct - Cg;
    if (w <= waste) { best = ct; waste = w; }
  }
  return best;
}
int wgrad_otile(int Og) { return Og >= 8 ? 8 : Og >= 4 ? 4 : Og >= 2 ? 2 : 1; }
int wgrad_ttile(int taps) { return taps == 1 ? 1 : taps <= 4 ? 4 : 9; }   // taps per workgroup: 1x1; up to 2x2 / 1x4; 3x3 and chunks of larger kernels

}  // namespace

int grouped_wgrad_splits(int N, int O, int G, int taps) {
  const int Og = O / G, ot = wgrad_otile(Og), tt = wgrad_ttile(taps);
  const long long base = (long long)G * ((Og + ot - 1) / ot) * ((taps + tt - 1) / tt);   // workgroups per split
  long long s = (1024 + base - 1) / base;                                                // ~4 per compute unit
  s = s > 64 ? 64 : s;
  s = s > N ? N : s;
  return (int)(s < 1 ? 1 : s);
}

int launch_grouped_dgrad(const GroupedGradP& q, const float* g, const float* what, const uint64_t* T, float* gx,
                         hipStream_t s) {
  const int Cg = q.C / q.G, Og = q.O / q.G, ct = dgrad_tile(Cg);
  const int ctiles = (Cg + ct - 1) / ct, ptiles = (q.H * q.W + 255) / 256;
  const long long blocks = (long long)q.N * q.G * ctiles * ptiles;     // <= N C H W < 2^31
  const size_t lds = (size_t)q.KH * q.KW * (Og < kOChunk ? Og : kOChunk) * ct * sizeof(float);   // <= 49 * 32 * 8 * 4 B
  if (blocks > 0x7fffffffLL || lds > 64 * 1024) return BNN_HIP_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)blocks), block(256);
  switch (ct) {
    case 8: hipLaunchKernelGGL(grouped_dgrad_kernel<8>, grid, block, lds, s, g, what, T, gx, q, ctiles, ptiles); break;
    case 4: hipLaunchKernelGGL(grouped_dgrad_kernel<4>, grid, block, lds, s, g, what, T, gx, q, ctiles, ptiles); break;
    case 2: hipLaunchKernelGGL(grouped_dgrad_kernel<2>, grid, block, lds, s, g, what, T, gx, q, ctiles, ptiles); break;
    default: hipLaunchKernelGGL(grouped_dgrad_kernel<1>, grid, block, lds, s, g, what, T, gx, q, ctiles, ptiles); break;
  }
  return hipGetLastError() == hipSuccess ? BNN_HIP_OK : BNN_HIP_ERR_LAUNCH;
}

template <int TT>
static void launch_wgrad_tt(int ot, dim3 grid, hipStream_t s, const float* g, const uint32_t* P, const uint32_t* M,
                            float* part, const GroupedGradP& q, int otiles, int cgp_log2) {
  const dim3 block(256);
  switch (ot) {
    case 8: hipLaunchKernelGGL((grouped_wgrad_kernel<8, TT>), grid, block, 0, s, g, P, M, part, q, otiles, cgp_log2); break;
    case 4: hipLaunchKernelGGL((grouped_wgrad_kernel<4, TT>), grid, block, 0, s, g, P, M, part, q, otiles, cgp_log2); break;
    case 2: hipLaunchKernelGGL((grouped_wgrad_kernel<2, TT>), grid, block, 0, s, g, P, M, part, q, otiles, cgp_log2); break;
    default: hipLaunchKernelGGL((grouped_wgrad_kernel<1, TT>), grid, block, 0, s, g, P, M, part, q, otiles, cgp_log2); break;
  }
}

int launch_grouped_wgrad(const GroupedGradP& q, const float* g, const uint64_t* P, const uint64_t* M, float* part,
                         int splits, hipStream_t s) {
  const int Cg = q.C / q.G, Og = q.O / q.G, taps = q.KH * q.KW;
  const int ot = wgrad_otile(Og), tt = wgrad_ttile(taps), otiles = (Og + ot - 1) / ot, tchunks = (taps + tt - 1) / tt;
  int cgp_log2 = 0;
  while ((1 << cgp_log2) < Cg) ++cgp_log2;
  if (cgp_log2 > 5 || splits < 1 || splits > 65535 || tchunks > 65535) return BNN_HIP_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)(q.G * otiles), (unsigned)splits, (unsigned)tchunks);
  const uint32_t* P32 = reinterpret_cast<const uint32_t*>(P);
  const uint32_t* M32 = reinterpret_cast<const uint32_t*>(M);
  if (tt == 1) launch_wgrad_tt<1>(ot, grid, s, g, P32, M32, part, q, otiles, cgp_log2);
  else if (tt == 4) launch_wgrad_tt<4>(ot, grid, s, g, P32, M32, part, q, otiles, cgp_log2);
  else launch_wgrad_tt<9>(ot, grid, s, g, P32, M32, part, q, otiles, cgp_log2);
  return hipGetLastError() == hipSuccess ? BNN_HIP_OK : BNN_HIP_ERR_LAUNCH;
}

}  // namespace bnn

// bconv_grouped.hip — grouped and depthwise binary convolutions (groups > 1) on the gfx950 integer ALU.
//
// Replaces bnn/layers/conv.py:90-97 for a layer built with groups = G: output channel o reads only the Cg = C / G input
// channels of its group o / Og (Og = O / G) — the BATS cells' SepConv / DilConv (bnn/models/layers/bats_ops.py:108-173,
// Conv2d(groups=12)) and the BATS ImageNet stem (bnn/models/bats.py:165,170, groups = C / 20).
//
// Weights: the windowed block-diagonal layout of include/bnn_hip.h (bnn_hip_grouped_weight_layout).  The 32 output
// channels of block ob read S consecutive 32-bit activation words per tap from w_lo(ob) = ((32 ob / Og) Cg) / 32 on; the
// group mask is folded into the non-zero mask Z, so the dot is exactly the zero-aware form of bconv.hip:
//     N   = (P | M) & Z_j                 non-zero products of channel j
//     D   = N & ~(W_j ^ M)                disagreeing positions (one v_bitop3_b32, disagree_nz(): a non-zero activation
//                                         disagrees with the weight iff its minus bit equals the weight's plus bit)
//     dot = popcount(N) - 2 popcount(D)   = popcount((P|M)&Z) - 2 popcount(disagree(W, M, P) & Z)
// Four vector instructions per word and output channel (v_and, v_bitop3, two v_bcnt); W_j and Z_j are wave-uniform and
// come through the scalar cache (two s_load_dwordx16 per plane and (tap, word)), the activation words are per-lane loads.
//
// Work decomposition: lane = output pixel (flattened over N, Ho, Wo; stores coalesced per channel), one wave = 64 pixels
// x one 32-channel block, as in bconv.hip's generic kernel.  These layers are small in K (Cg KH KW = 72 .. 400 on the
// BATS shapes): the fp32 output store, not the integer ALU, bounds most of them (tools/bench_grouped.py).
#include "bconv_core.h"

namespace bnn {

// D = n & ~(w ^ m) in ONE v_bitop3_b32 (truth table 0x90: src0 set and src1 == src2), with the weight word w as the
// scalar operand.  Written out because hipcc, seeing n = (p | m) & z, re-associates the plain expression into
// bitop3(z, xnor(w, m), p | m): three instructions per word and channel instead of one.
__device__ __forceinline__ uint32_t disagree_nz(uint32_t n, uint32_t w, uint32_t m) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint32_t r;
  asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x90" : "=v"(r) : "v"(n), "s"(w), "v"(m));
  return r;
#else
  return n & ~(w ^ m);
#endif
}

// The integer part of one wave: the dot products of its 64 pixels with the 32 output channels of block `ob`.
// FAST: 24-bit index multiplies (decode_pixel<true>), when small_indices() holds.
template <bool FAST>
__device__ __forceinline__ void grouped_dots(const uint32_t* __restrict__ P, const uint32_t* __restrict__ M,
                                             const uint32_t* __restrict__ W, const uint32_t* __restrict__ Z,
                                             const Geo& g, const Pix& px, const int ob, const int Cg, const int Og,
                                             const int S, int (&dotv)[kOCB]) {
  const int taps = g.KH * g.KW;
  const int w_lo = (ob * kOCB) / Og * Cg / 32;
  const int nw = min(S, g.cw32 - w_lo);  // window words that exist in the planes (the rest has Z == 0): never >= cw32
  const int plane = g.H * g.Wd;
  const uint32_t* __restrict__ wblk = W + (size_t)ob * taps * S * kOCB;
  const uint32_t* __restrict__ zblk = Z + (size_t)ob * taps * S * kOCB;

  int nzc[kOCB], dis[kOCB];
#pragma unroll
  for (int j = 0; j < kOCB; ++j) { nzc[j] = 0; dis[j] = 0; }
  const int iy0 = px.oy * g.sh - g.ph, ix0 = px.ox * g.sw - g.pw;
  for (int t = 0; t < taps; ++t) {
    const int ky = t / g.KW, kx = t - ky * g.KW;
    const int iy = iy0 + ky * g.dh, ix = ix0 + kx * g.dw;
    // taps in the zero padding (applied after sign(): conv.py:91-92) read pixel 0 and contribute P = M = 0
    const bool ok = (unsigned)iy < (unsigned)g.H && (unsigned)ix < (unsigned)g.Wd;
    const int pix = ok ? iy * g.Wd + ix : 0;
    for (int s = 0; s < nw; ++s) {
      const int w = w_lo + s;
      // word w of the pixel: plane (w >> 1), half (w & 1); BYTES below 2^32 (capi.hip keeps the planes < 2^29 words)
      const unsigned boff = ((px.in_base + (unsigned)((w >> 1) * plane + pix)) * 2u + (unsigned)(w & 1)) * 4u;
      const uint32_t pw = ld_off(P, boff), mw = ld_off(M, boff);
      const uint32_t p = ok ? pw : 0u, m = ok ? mw : 0u;
      const uint32_t pm = p | m;
      WStream<kOCB> wv, zv;
      const size_t woff = ((size_t)t * S + s) * kOCB;
      load_wblock<kOCB>(wblk + woff, wv);
      load_wblock<kOCB>(zblk + woff, zv);
      static_for<kOCB>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        const uint32_t n = pm & zv.v[j];
        nzc[j] = popc_acc(n, nzc[j]);
        dis[j] = popc_acc(disagree_nz(n, wv.v[j], m), dis[j]);
      });
    }
  }
#pragma unroll
  for (int j = 0; j < kOCB; ++j) dotv[j] = nzc[j] - 2 * dis[j];
}

template <bool FAST>
__global__ __launch_bounds__(64) void bconv_grouped_kernel(
    const uint32_t* __restrict__ P, const uint32_t* __restrict__ M, const uint32_t* __restrict__ W,
    const uint32_t* __restrict__ Z, BNN_EPI_PARAMS, const Geo g, const int Cg, const int Og, const int S) {
  BNN_EPI_INIT;
  // 1-D grid, block-major: consecutive workgroups walk the pixel tiles of one 32-channel block (the same weight words)
  const int ob = (int)(blockIdx.x / (unsigned)g.tiles);
  const int tile = (int)blockIdx.x - ob * g.tiles;
  const Pix px = decode_pixel<FAST>(g, tile * kWave + threadIdx.x);
  int dotv[kOCB];
  grouped_dots<FAST>(P, M, W, Z, g, px, ob, Cg, Og, S, dotv);
  uint32_t pbits = 0u, mbits = 0u;
  float resv[kOCB];  // (no residual in this epilogue)
  // the float operations of the other kernels: fmaf(alpha, dot, bias) [* post_scale] (or the int32 dot: EF_RAW).  A whole
  // block takes the straight-line form (no per-lane / per-channel guards; lanes past the last pixel were clamped to it
  // and store the same value to the same place).
  if ((ob + 1) * kOCB <= g.O) epilogue<kOCB, EP_PLAIN, true>(g, px, ob * kOCB, dotv, resv, epi, pbits, mbits);
  else epilogue<kOCB, EP_PLAIN>(g, px, ob * kOCB, dotv, resv, epi, pbits, mbits);
}

// Epilogue of a BATS cell operation (bnn/models/layers/bats_ops.py:108-173: y = [x +] channel_shuffle(PReLU(conv), 4)):
//     v  = fmaf(alpha[o], dot, bias[o]) [* post_scale[o]]            the EP_PLAIN operations, the same bits
//     v  = v >= 0 ? v : prelu[o] * v                                  (EF_PRELU; the form of bconv_core.h's epilogue)
//     o' = (o % (O / sg)) * sg + o / (O / sg)                         channel_shuffle(., sg) as a store index
//     out[n, o', y, x] = res[n, o', y, x] + v                         (EF_RES)
// The shuffle moves whole channel planes: a store instruction still writes 64 consecutive pixels of ONE plane, only the
// wave-uniform plane offset (the buffer instruction's scalar operand) changes.  o -> o' runs on the scalar unit, without a
// division per channel: (q, r) = (o / cpg, o % cpg) of the block's first channel, then r counts up and carries into q.
// The product with the slope and the add of the residual are two roundings, as in torch: never contracted into an fma.
// FULL (all 32 channels exist): the straight-line form of epilogue<.., FULL> — the residual loads of a batch of channels
// are issued first and queue up, each channel then waits for its own (`s_waitcnt vmcnt(n)` counts down) while the stores
// queue behind them.
// PRELU / RES are compile-time there: as run-time flags every channel's slope load, select and residual became a branch
// region of its own with an `s_waitcnt vmcnt(0)` at each join.  The partial last block keeps run-time flags and guards.
//
// A cell NODE (bnn_hip_bconv2d_grouped_node; bnn/models/bats.py:61-74: s = op1(h1) + op2(h2)) adds a second operand
// and lets every fp32 tensor be a channel slice of a wider one:
//     out[n, c_off + o', y, x] = (res[n, o', y, x] + v) + add[n, o', y, x]      three roundings
// NodeViews carries what differs from `out`: e.res / nv.add point at channel 0 of their slices, and their per-lane bases
// are n c_total hw + r with THEIR c_total.  VIEWS = false is the cell operation's epilogue as it was (res shares out's
// layout, no addend): the same instructions.
struct NodeViews {
  const float* add;
  unsigned res_lane, add_lane;  // BYTES
};
template <bool FULL, bool PRELU = false, bool RES = false, bool VIEWS = false, bool ADD = false>
__device__ __forceinline__ void cell_epilogue(const Geo& g, const Pix& px, const int o0, const int (&dot)[kOCB],
                                              const EpiArgs& e, const int sg, const int cpg,
                                              const NodeViews nv = NodeViews{}) {
#pragma clang fp contract(off)
  using f2 = __attribute__((ext_vector_type(2))) float;
  const int hw = g.Ho * g.Wo;
  const unsigned lane_off = px.out_base * 4u;  // BYTES; host keeps N*c_tot*hw < 2^30
  const int f = g.flags;
  const bool hb = (f & EF_BIAS) != 0, hs = (f & EF_SCALE) != 0;
  // the operands' own slices start at their channel 0: plane o' of them is choff[] less out's window offset
  const unsigned res_lane = VIEWS ? nv.res_lane : lane_off, win = VIEWS ? (unsigned)g.c_off * (unsigned)hw * 4u : 0u;
  unsigned choff[kOCB];  // byte offset of plane o' (wave-uniform)
  {
    int q = o0 / cpg, r = o0 - q * cpg;
#pragma unroll
    for (int j = 0; j < kOCB; ++j) {
      choff[j] = (unsigned)(r * sg + q + g.c_off) * (unsigned)hw * 4u;
      if (++r == cpg) { r = 0; ++q; }
    }
  }
  if constexpr (FULL) {
    // (the residual loads go out kResBatch channels at a time: all 32 at once cost 30 more VGPRs, a wave per SIMD less)
    // (with both operands, 8 + 8: the same number of loads in flight)
    constexpr int kResBatch = (RES && ADD) ? 8 : 16;
#pragma unroll
    for (int j0 = 0; j0 < kOCB; j0 += kResBatch) {
      [[maybe_unused]] float resv[kResBatch], addv[kResBatch];
      if constexpr (RES) {
#pragma unroll
        for (int j = 0; j < kResBatch; ++j) resv[j] = buf_ld(make_rsrc(e.res), res_lane, choff[j0 + j] - win);
      }
      if constexpr (ADD) {
#pragma unroll
        for (int j = 0; j < kResBatch; ++j) addv[j] = buf_ld(make_rsrc(nv.add), nv.add_lane, choff[j0 + j] - win);
      }
#pragma unroll
      for (int j = j0; j < j0 + kResBatch; j += 2) {
        const int o = o0 + j;
        f2 y = __builtin_elementwise_fma(f2{e.alpha[o], e.alpha[o + 1]}, f2{(float)dot[j], (float)dot[j + 1]},
                                         hb ? f2{e.bias[o], e.bias[o + 1]} : f2{0.0f, 0.0f});
        if (hs) y *= f2{e.scale[o], e.scale[o + 1]};
        float y0 = y.x, y1 = y.y;
        if constexpr (PRELU) {
          const float a0 = e.prelu[o], a1 = e.prelu[o + 1];  // (read outside the select: no branch per channel)
          const float n0 = a0 * y0, n1 = a1 * y1;
          y0 = (y0 >= 0.0f) ? y0 : n0;
          y1 = (y1 >= 0.0f) ? y1 : n1;
        }
        if constexpr (RES) { y0 = resv[j - j0] + y0; y1 = resv[j - j0 + 1] + y1; }
        if constexpr (ADD) { y0 = y0 + addv[j - j0]; y1 = y1 + addv[j - j0 + 1]; }
        buf_st(make_rsrc(e.out), lane_off, choff[j], y0);
        buf_st(make_rsrc(e.out), lane_off, choff[j + 1], y1);
      }
    }
  } else {  // channels past O (the pad channels of the weight layout) and dead lanes do not store
    const bool hp = (f & EF_PRELU) != 0, hr = (f & EF_RES) != 0;
    float* outf = static_cast<float*>(e.out);
#pragma unroll
    for (int j = 0; j < kOCB; ++j) {
      const int o = o0 + j;
      if (o < g.O && px.live) {
        float y = fmaf(e.alpha[o], (float)dot[j], hb ? e.bias[o] : 0.0f);
        if (hs) y *= e.scale[o];
        if (hp) y = (y >= 0.0f) ? y : e.prelu[o] * y;
        if (hr) y = ld_off(reinterpret_cast<const float*>(reinterpret_cast<const char*>(e.res) + (choff[j] - win)), res_lane) + y;
        if constexpr (VIEWS) {
          if (nv.add) y = y + ld_off(reinterpret_cast<const float*>(reinterpret_cast<const char*>(nv.add) + (choff[j] - win)), nv.add_lane);
        }
        st_off(reinterpret_cast<float*>(reinterpret_cast<char*>(outf) + choff[j]), lane_off, y);
      }
    }
  }
}

// The grouped convolution with the cell-operation epilogue: the main loop of bconv_grouped_kernel, one launch for
// conv + PReLU + channel_shuffle + skip.  sg: shuffle groups (>= 1, divides O), cpg = O / sg.
template <bool FAST>
__global__ __launch_bounds__(64) void bconv_grouped_cell_kernel(
    const uint32_t* __restrict__ P, const uint32_t* __restrict__ M, const uint32_t* __restrict__ W,
    const uint32_t* __restrict__ Z, BNN_EPI_PARAMS, const Geo g, const int Cg, const int Og, const int S, const int sg,
    const int cpg) {
  BNN_EPI_INIT;
  const int ob = (int)(blockIdx.x / (unsigned)g.tiles);
  const int tile = (int)blockIdx.x - ob * g.tiles;
  const Pix px = decode_pixel<FAST>(g, tile * kWave + threadIdx.x);
  int dotv[kOCB];
  grouped_dots<FAST>(P, M, W, Z, g, px, ob, Cg, Og, S, dotv);
  const int o0 = ob * kOCB;
  if (o0 + kOCB > g.O) return cell_epilogue<false>(g, px, o0, dotv, epi, sg, cpg);
  const bool hp = (g.flags & EF_PRELU) != 0, hr = (g.flags & EF_RES) != 0;
  if (hp && hr) cell_epilogue<true, true, true>(g, px, o0, dotv, epi, sg, cpg);
  else if (hp) cell_epilogue<true, true, false>(g, px, o0, dotv, epi, sg, cpg);
  else if (hr) cell_epilogue<true, false, true>(g, px, o0, dotv, epi, sg, cpg);
  else cell_epilogue<true, false, false>(g, px, o0, dotv, epi, sg, cpg);
}

// The grouped convolution as one term of a cell node: the same main loop, the epilogue above with VIEWS.  res / add point
// at the first element of their channel slices (capi.hip), ct_res / ct_add are the channel counts of the tensors around
// them.  PRELU / RES / ADD are compile-time for whole blocks: eight straight-line epilogues, one taken per launch.
template <bool FAST>
__global__ __launch_bounds__(64) void bconv_grouped_node_kernel(
    const uint32_t* __restrict__ P, const uint32_t* __restrict__ M, const uint32_t* __restrict__ W,
    const uint32_t* __restrict__ Z, BNN_EPI_PARAMS, const float* __restrict__ add, const Geo g, const int Cg,
    const int Og, const int S, const int sg, const int cpg, const int ct_res, const int ct_add) {
  BNN_EPI_INIT;
  const int ob = (int)(blockIdx.x / (unsigned)g.tiles);
  const int tile = (int)blockIdx.x - ob * g.tiles;
  const Pix px = decode_pixel<FAST>(g, tile * kWave + threadIdx.x);
  int dotv[kOCB];
  grouped_dots<FAST>(P, M, W, Z, g, px, ob, Cg, Og, S, dotv);
  const int o0 = ob * kOCB, hw = g.Ho * g.Wo;
  NodeViews nv;
  nv.add = add;
  nv.res_lane = (unsigned)(imul<FAST>(imul<FAST>(px.n, ct_res), hw) + px.r) * 4u;
  nv.add_lane = (unsigned)(imul<FAST>(imul<FAST>(px.n, ct_add), hw) + px.r) * 4u;
  if (o0 + kOCB > g.O) return cell_epilogue<false, false, false, true>(g, px, o0, dotv, epi, sg, cpg, nv);
  const int v = ((g.flags & EF_PRELU) ? 4 : 0) | ((g.flags & EF_RES) ? 2 : 0) | (add ? 1 : 0);
  switch (v) {
    case 0: return cell_epilogue<true, false, false, true, false>(g, px, o0, dotv, epi, sg, cpg, nv);
    case 1: return cell_epilogue<true, false, false, true, true>(g, px, o0, dotv, epi, sg, cpg, nv);
    case 2: return cell_epilogue<true, false, true, true, false>(g, px, o0, dotv, epi, sg, cpg, nv);
    case 3: return cell_epilogue<true, false, true, true, true>(g, px, o0, dotv, epi, sg, cpg, nv);
    case 4: return cell_epilogue<true, true, false, true, false>(g, px, o0, dotv, epi, sg, cpg, nv);
    case 5: return cell_epilogue<true, true, false, true, true>(g, px, o0, dotv, epi, sg, cpg, nv);
    case 6: return cell_epilogue<true, true, true, true, false>(g, px, o0, dotv, epi, sg, cpg, nv);
    default: return cell_epilogue<true, true, true, true, true>(g, px, o0, dotv, epi, sg, cpg, nv);
  }
}

// p: geometry of the whole convolution (p.C = all input channels, p.cw32 = their words per pixel); S: words per tap of the
// weight layout (bnn_hip_grouped_weight_layout).  capi.hip has checked sizes, alignments and C % groups == O % groups == 0.
int launch_bconv_grouped(const ConvP& p, int groups, int S, hipStream_t s) {
  const Geo g = make_geo(p);
  const unsigned nb = (unsigned)((p.O + kOCB - 1) / kOCB);
  const dim3 grid((unsigned)g.tiles * nb);
  const int Cg = p.C / groups, Og = p.O / groups;
  if (small_indices(p))
    hipLaunchKernelGGL((bconv_grouped_kernel<true>), grid, dim3(kWave), 0, s, p.P, p.M, p.W, p.Z, BNN_EPI_ACTUALS, g,
                       Cg, Og, S);
  else
    hipLaunchKernelGGL((bconv_grouped_kernel<false>), grid, dim3(kWave), 0, s, p.P, p.M, p.W, p.Z, BNN_EPI_ACTUALS, g,
                       Cg, Og, S);
  return hipGetLastError() == hipSuccess ? BNN_HIP_OK : BNN_HIP_ERR_LAUNCH;
}

// The same launch with the cell-operation epilogue (p.prelu, p.res optional; p.alpha set): capi.hip has checked, beyond
// the above, shuffle_groups >= 1 and O % shuffle_groups == 0, and that p.res does not alias p.out.
int launch_bconv_grouped_cell(const ConvP& p, int groups, int S, int shuffle_groups, hipStream_t s) {
  const Geo g = make_geo(p);
  const unsigned nb = (unsigned)((p.O + kOCB - 1) / kOCB);
  const dim3 grid((unsigned)g.tiles * nb);
  const int Cg = p.C / groups, Og = p.O / groups, cpg = p.O / shuffle_groups;
  if (small_indices(p))
    hipLaunchKernelGGL((bconv_grouped_cell_kernel<true>), grid, dim3(kWave), 0, s, p.P, p.M, p.W, p.Z, BNN_EPI_ACTUALS,
                       g, Cg, Og, S, shuffle_groups, cpg);
  else
    hipLaunchKernelGGL((bconv_grouped_cell_kernel<false>), grid, dim3(kWave), 0, s, p.P, p.M, p.W, p.Z, BNN_EPI_ACTUALS,
                       g, Cg, Og, S, shuffle_groups, cpg);
  return hipGetLastError() == hipSuccess ? BNN_HIP_OK : BNN_HIP_ERR_LAUNCH;
}

// The node launch: p.c_off / p.c_tot window `out`; p.res and `add` (either may be null) point at channel 0 of their
// slices of [N, ct_res, Ho, Wo] / [N, ct_add, Ho, Wo] tensors.  capi.hip has checked everything launch_bconv_grouped_cell
// needs, the three views' sizes, and that `out` overlaps neither operand.
int launch_bconv_grouped_node(const ConvP& p, int groups, int S, int shuffle_groups, const float* add, int ct_res,
                              int ct_add, hipStream_t s) {
  const Geo g = make_geo(p);
  const unsigned nb = (unsigned)((p.O + kOCB - 1) / kOCB);
  const dim3 grid((unsigned)g.tiles * nb);
  const int Cg = p.C / groups, Og = p.O / groups, cpg = p.O / shuffle_groups;
  const long long lim = 1ll << 23;  // (decode_pixel<true>'s products, for the operands' image strides too)
  if (small_indices(p) && (long long)p.N * ct_res < lim && (long long)p.N * ct_add < lim)
    hipLaunchKernelGGL((bconv_grouped_node_kernel<true>), grid, dim3(kWave), 0, s, p.P, p.M, p.W, p.Z, BNN_EPI_ACTUALS,
                       add, g, Cg, Og, S, shuffle_groups, cpg, ct_res, ct_add);
  else
    hipLaunchKernelGGL((bconv_grouped_node_kernel<false>), grid, dim3(kWave), 0, s, p.P, p.M, p.W, p.Z, BNN_EPI_ACTUALS,
                       add, g, Cg, Og, S, shuffle_groups, cpg, ct_res, ct_add);
  return hipGetLastError() == hipSuccess ? BNN_HIP_OK : BNN_HIP_ERR_LAUNCH;
}

}  // namespace bnn

// prelu_bwd.hip — backward of  channel_shuffle(PReLU(z), sg)  of a BATS cell operation in a training step
// (bnn/models/layers/bats_ops.py:108-173: y = [x +] channel_shuffle(PReLU(conv(.)), 4); ReLUConvBN: sg = 1).
//
// The forward (csrc/bconv_grouped.hip, launch_bconv_grouped_cell) applies PReLU and the shuffle in the convolution's
// epilogue and keeps no z; the backward recomputes z with the un-fused launch and runs this pass over it:
//     o' = (o % (O / sg)) * sg + o / (O / sg)                 where the forward stored channel o
//     g  = gy[n, o', :]                                       the incoming gradient, in the output's (shuffled) order
//     gz[n, o, :] = z > 0 ? g : slope[o] * g                  torch's convention: z == +-0 and NaN take the slope branch
//     dslope[o]   = sum over n, pixels with !(z > 0) of g * z
// torch evaluates this as a .contiguous() copy for the shuffle, PReLU's backward and its reduction: several passes over
// gy and z.  Here: one pass (2 reads, 1 write) whose blocks leave per-(channel, image split) partial sums in double,
// and a second tiny kernel that adds them in a fixed order — no atomics, the same bits on every run (the
// scheme of bn_stats_kernel / bn_finalize_kernel in bn_train.hip, whose split rule is shared).  HBM-bound; float4 along
// the contiguous HW axis of an (image, channel) row.  gz may be z itself (each element is read before it is written,
// by the same thread).
#include "bnn_dev.h"

namespace bnn {

namespace plb {
constexpr int NT = 256;
}

template <int VEC>
__global__ __launch_bounds__(plb::NT) void prelu_shuffle_bwd_kernel(const float* __restrict__ gy, const float* z,
                                                                    const float* __restrict__ slope, int slope_stride,
                                                                    int N, int O, int HW, int sg, int cpg, int per,
                                                                    float* gz, double* __restrict__ partial) {
  __shared__ double sw[plb::NT / 64];
  const int o = blockIdx.x, s = blockIdx.y, S = gridDim.y;
  const int os = (o % cpg) * sg + o / cpg;           // where the forward stored channel o
  const int n0 = s * per, n1 = min(N, n0 + per);
  const int upr = HW / VEC;
  const int total = (n1 - n0) * upr;
  const float a = slope[o * slope_stride];
  double acc = 0.0;
  for (int idx = threadIdx.x; idx < total; idx += plb::NT) {
    const int dn = idx / upr, u = idx - dn * upr;
    const size_t iz = ((size_t)(n0 + dn) * O + o) * HW + (size_t)u * VEC;
    const size_t ig = ((size_t)(n0 + dn) * O + os) * HW + (size_t)u * VEC;
    if constexpr (VEC == 4) {
      const float4 g = *reinterpret_cast<const float4*>(gy + ig);
      const float4 zv = *reinterpret_cast<const float4*>(z + iz);
      float4 d;
      d.x = zv.x > 0.f ? g.x : a * g.x; d.y = zv.y > 0.f ? g.y : a * g.y;
      d.z = zv.z > 0.f ? g.z : a * g.z; d.w = zv.w > 0.f ? g.w : a * g.w;
      *reinterpret_cast<float4*>(gz + iz) = d;
      acc += (zv.x > 0.f ? 0.0 : (double)g.x * zv.x) + (zv.y > 0.f ? 0.0 : (double)g.y * zv.y) +
             (zv.z > 0.f ? 0.0 : (double)g.z * zv.z) + (zv.w > 0.f ? 0.0 : (double)g.w * zv.w);
    } else {
      const float g = gy[ig], zv = z[iz];
      gz[iz] = zv > 0.f ? g : a * g;
      acc += zv > 0.f ? 0.0 : (double)g * zv;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) sw[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < plb::NT / 64; ++w) t += sw[w];     // fixed order: deterministic
    partial[(size_t)o * S + s] = t;
  }
}

// dslope from the partial sums, one workgroup.  count == O: thread per channel (strided), splits added in index order.
// count == 1 (a one-parameter PReLU): the channel sums are added over channels too — per thread in channel order, then
// the 256 thread sums in thread order.
__global__ __launch_bounds__(plb::NT) void prelu_slope_finalize_kernel(const double* __restrict__ partial, int S, int O,
                                                                       int single, float* __restrict__ dslope) {
  __shared__ double st[plb::NT];
  double mine = 0.0;
  for (int o = threadIdx.x; o < O; o += plb::NT) {
    double t = 0.0;
    for (int s = 0; s < S; ++s) t += partial[(size_t)o * S + s];
    if (!single) dslope[o] = (float)t;
    mine += t;
  }
  if (!single) return;
  st[threadIdx.x] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int i = 0; i < plb::NT; ++i) t += st[i];
    dslope[0] = (float)t;
  }
}

// capi.hip has checked: positive sizes, N * HW and the tensor inside the BatchNorm entry points' limits (check_bn),
// slope_count in {1, O}, sg >= 1 dividing O, gz not gy, `partial` O * splits doubles with splits = bn_train_splits(N, O, HW).
int launch_prelu_shuffle_bwd(const float* gy, const float* z, const float* slope, int slope_count, int N, int O, int HW,
                             int sg, int splits, float* gz, float* dslope, double* partial, hipStream_t s) {
  auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  const int per = (N + splits - 1) / splits;
  const dim3 grid((unsigned)O, (unsigned)splits);
  const int stride = slope_count == 1 ? 0 : 1, cpg = O / sg;
  if (HW % 4 == 0 && al16(gy) && al16(z) && al16(gz))
    hipLaunchKernelGGL(prelu_shuffle_bwd_kernel<4>, grid, dim3(plb::NT), 0, s, gy, z, slope, stride, N, O, HW, sg, cpg, per, gz,
                       partial);
  else
    hipLaunchKernelGGL(prelu_shuffle_bwd_kernel<1>, grid, dim3(plb::NT), 0, s, gy, z, slope, stride, N, O, HW, sg, cpg, per, gz,
                       partial);
  hipLaunchKernelGGL(prelu_slope_finalize_kernel, dim3(1), dim3(plb::NT), 0, s, partial, splits, O, slope_count == 1 ? 1 : 0,
                     dslope);
  return hipGetLastError() == hipSuccess ? BNN_HIP_OK : BNN_HIP_ERR_LAUNCH;
}

}  // namespace bnn

// Fixed-order reduction of the weight-gradient slabs.
#pragma once
#include "ssip_common.h"

namespace {

// WGRAD slab reduction:  dW[k][c][r][s] (torchvision KCRS, fp32) =
//   (accumulate ? dW : 0) + sum_split slab[split][k][(r*Sp + s)*Cp + c]
// A thread owns one 16-B vector (4 consecutive columns) in one of G split
// groups (G a power of two, chosen so the grid has ~1024 workgroups); a
// group sums its contiguous split range in order, then the G partials are
// combined in fixed order through LDS: bitwise reproducible.
__global__ void __launch_bounds__(256) wgrad_reduce_kernel(const float* __restrict__ slab, int splits, int K,
                                                           int Ng, int C, int R, int S, int Cp, int Sp,
                                                           float* __restrict__ dw, int accumulate, int lg) {
  typedef __attribute__((ext_vector_type(4))) float f4;
  __shared__ f4 red[256];
  const int G = 1 << lg, V = 256 >> lg;
  const int v = threadIdx.x & (V - 1), grp = threadIdx.x >> (8 - lg);
  const long total4 = (long)K * Ng / 4;
  const long idx4 = (long)blockIdx.x * V + v;
  const long sstride4 = total4;
  const int per = (splits + G - 1) / G;
  const int s0 = grp * per;
  const int s1 = min(splits, s0 + per);
  f4 acc = {0.f, 0.f, 0.f, 0.f};
  if (idx4 < total4) {
    const f4* p = reinterpret_cast<const f4*>(slab) + idx4;
    int sp = s0;
    for (; sp + 4 <= s1; sp += 4) {
      const f4 a0 = p[(long)sp * sstride4], a1 = p[(long)(sp + 1) * sstride4];
      const f4 a2 = p[(long)(sp + 2) * sstride4], a3 = p[(long)(sp + 3) * sstride4];
      acc += a0;
      acc += a1;
      acc += a2;
      acc += a3;
    }
    for (; sp < s1; ++sp) acc += p[(long)sp * sstride4];
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  if (grp == 0 && idx4 < total4) {
    f4 t = red[v];
    for (int g = 1; g < G; ++g) t += red[g * V + v];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const long idx = idx4 * 4 + e;
      const int col = (int)(idx % Ng);
      const int k = (int)(idx / Ng);
      const int c = col % Cp;
      const int rs = col / Cp;
      const int s = rs % Sp;
      const int r = rs / Sp;
      if (c < C && s < S) {
        const long o = (((long)k * C + c) * R + r) * S + s;
        dw[o] = accumulate ? dw[o] + t[e] : t[e];
      }
    }
  }
}

// The same reduction with coalesced KCRS stores, for few splits over many
// output rows (C % 64 == 0, no channel / tap padding): one workgroup per
// (k, 64-channel block) sums the block's R*S segments of 64 columns (16-B
// vectors, splits in order) into LDS as [c][rs] and writes dW[k][c0 ..
// c0+63][r][s] -- 64 R S contiguous floats -- as 16-B vectors.  (The kernel
// above stores 4-B values R*S floats apart, a partial line per lane.)
constexpr int WGR_T_MAXRS = 9;

__global__ void __launch_bounds__(256) wgrad_reduce_t_kernel(const float* __restrict__ slab, int splits, int K,
                                                             int Ng, int C, int RS, float* __restrict__ dw,
                                                             int accumulate) {
  typedef __attribute__((ext_vector_type(4))) float f4;
  __shared__ float tile[64 * WGR_T_MAXRS];
  const int cblocks = C >> 6;
  const int k = blockIdx.x / cblocks, c0 = (blockIdx.x - k * cblocks) << 6;
  const long sstride4 = (long)K * Ng / 4;
  for (int u = threadIdx.x; u < RS * 16; u += blockDim.x) {
    const int rs = u >> 4, cv = u & 15;
    const f4* p = reinterpret_cast<const f4*>(slab) + ((long)k * Ng + (long)rs * C + c0 + cv * 4) / 4;
    f4 acc = {0.f, 0.f, 0.f, 0.f};
    int sp = 0;
    for (; sp + 4 <= splits; sp += 4) {
      const f4 a0 = p[(long)sp * sstride4], a1 = p[(long)(sp + 1) * sstride4];
      const f4 a2 = p[(long)(sp + 2) * sstride4], a3 = p[(long)(sp + 3) * sstride4];
      acc += a0;
      acc += a1;
      acc += a2;
      acc += a3;
    }
    for (; sp < splits; ++sp) acc += p[(long)sp * sstride4];
#pragma unroll
    for (int e = 0; e < 4; ++e) tile[(cv * 4 + e) * RS + rs] = acc[e];
  }
  __syncthreads();
  f4* o = reinterpret_cast<f4*>(dw + ((long)k * C + c0) * RS);
  for (int i = threadIdx.x; i < 16 * RS; i += blockDim.x) {
    f4 t = {tile[4 * i], tile[4 * i + 1], tile[4 * i + 2], tile[4 * i + 3]};
    if (accumulate) t += o[i];
    o[i] = t;
  }
}

}  // namespace

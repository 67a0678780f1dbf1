// Layout A of the pairwise kernels (analytics.hip, tsne.hip): a workgroup of
// NT threads owns RA = 64 rows and walks the columns in tiles of 64; lane =
// column, each wave holds 16 rows.  Squared distances are the direct
// difference sum_c (x_c - y_c)^2, fp32, one fma per feature in feature order,
// over LDS-staged chunks of DC features.
#pragma once
#include "ssip_common.h"

namespace {

constexpr int DC = 32;        // features per LDS chunk
constexpr int NT = 256;       // threads per workgroup (4 waves)
constexpr int RA = 64;        // layout A: rows per workgroup (16 per wave)
constexpr int XR_LD = 68;     // layout A: row-tile leading dimension ([DC][RA] transposed, 16-B aligned rows)
constexpr int XC_LD = DC + 1; // +1 pad: lane-per-row reads hit 32 distinct banks

// ---------------------------------------------------------------------------
// layout A
// ---------------------------------------------------------------------------
// A 64 x DC tile is 8 elements per thread: element q of thread tid is (point
// idx >> 5, feature idx & 31) with idx = tid + q * NT.  Tiles are fetched into
// registers one step ahead of their use, so the global latency overlaps the
// previous tile's arithmetic.
constexpr int TQ = 64 * DC / NT;
__device__ __forceinline__ void fetch_tile_a(float (&v)[TQ], const float* __restrict__ X, int p0, int N, int d, int c0,
                                             int tid) {
#pragma unroll
  for (int q = 0; q < TQ; ++q) {
    const int idx = tid + q * NT;
    const int p = p0 + (idx >> 5), c = c0 + (idx & (DC - 1));
    v[q] = (p < N && c < d) ? X[(long)p * d + c] : 0.f;
  }
}
// xr[c][r] = X[row0 + r][c0 + c] (zero outside the matrix)
__device__ __forceinline__ void put_rows_a(float* xr, const float (&v)[TQ], int tid) {
#pragma unroll
  for (int q = 0; q < TQ; ++q) {
    const int idx = tid + q * NT;
    xr[(idx & (DC - 1)) * XR_LD + (idx >> 5)] = v[q];
  }
}
// xc[j][c] = X[col0 + j][c0 + c] (zero outside the matrix)
__device__ __forceinline__ void put_cols_a(float* xc, const float (&v)[TQ], int tid) {
#pragma unroll
  for (int q = 0; q < TQ; ++q) {
    const int idx = tid + q * NT;
    xc[(idx >> 5) * XC_LD + (idx & (DC - 1))] = v[q];
  }
}
// acc[u] += sum_c (x[row w*16+u][c] - x[col lane][c])^2 over one chunk
__device__ __forceinline__ void accumulate_a(float (&acc)[16], const float* xr, const float* xc, int w, int lane) {
#pragma unroll 4
  for (int cc = 0; cc < DC; ++cc) {
    const float cv = xc[lane * XC_LD + cc];
    const f32x4* rp = reinterpret_cast<const f32x4*>(xr + cc * XR_LD + w * 16);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 rv = rp[q];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float df = rv[e] - cv;
        acc[q * 4 + e] = fmaf(df, df, acc[q * 4 + e]);
      }
    }
  }
}

}  // namespace

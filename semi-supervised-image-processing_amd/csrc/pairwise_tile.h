// Layout A of the pairwise kernels (analytics.hip, tsne.hip): a workgroup of
// NT threads owns RA = 64 rows and walks the columns in tiles of 64; lane =
// column, each wave holds 16 rows.  Squared distances are the direct
// difference sum_c (x_c - y_c)^2, fp32, one fma per feature in feature order,
// over LDS-staged chunks of DC features.  walk_columns_a is the one walk; its
// users say what happens to a finished 64 x 64 tile of squared distances.
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

// The column walk of the workgroup's rows row0 .. row0 + 63: on_tile(jt, acc)
// is called once per column tile jt, in increasing jt, with acc[u] = d2(row
// row0 + w * 16 + u, column jt * 64 + lane) (zero-padded outside the matrix,
// so the caller masks rows and columns >= N).  Tiles are staged in steps of
// one feature chunk; every thread of the workgroup must call this, once.
template <class OnTile>
__device__ __forceinline__ void walk_columns_a(int N, int d, const float* __restrict__ X, int row0, OnTile on_tile) {
  __shared__ __attribute__((aligned(16))) float xr[DC * XR_LD];
  __shared__ float xc[64 * XC_LD];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int nch = (d + DC - 1) / DC, ntile = (N + 63) / 64;

  float pre_r[TQ], pre_c[TQ];
  fetch_tile_a(pre_r, X, row0, N, d, 0, tid);
  fetch_tile_a(pre_c, X, 0, N, d, 0, tid);
  float acc[16];
  const int steps = ntile * nch;
  for (int it = 0; it < steps; ++it) {
    const int jt = it / nch, ch = it - jt * nch;
    // a single-chunk row tile stays resident for the whole column walk
    if (nch > 1 || it == 0) put_rows_a(xr, pre_r, tid);
    put_cols_a(xc, pre_c, tid);
    __syncthreads();
    if (it + 1 < steps) {  // next step's tiles, in flight during the arithmetic below
      const int jn = (it + 1) / nch, cn = (it + 1) - jn * nch;
      if (nch > 1) fetch_tile_a(pre_r, X, row0, N, d, cn * DC, tid);
      fetch_tile_a(pre_c, X, jn * 64, N, d, cn * DC, tid);
    }
    if (ch == 0) {
#pragma unroll
      for (int u = 0; u < 16; ++u) acc[u] = 0.f;
    }
    accumulate_a(acc, xr, xc, w, lane);
    __syncthreads();  // the next step overwrites the tiles
    if (ch == nch - 1) on_tile(jt, acc);
  }
}

// ---------------------------------------------------------------------------
// selection across a wave
// ---------------------------------------------------------------------------
typedef unsigned long long u64;
// fminf / fmaxf, not <: of a NaN distance and a number both give the number
__device__ __forceinline__ float key_min(float a, float b) { return fminf(a, b); }
__device__ __forceinline__ float key_max(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ u64 key_min(u64 a, u64 b) { return b < a ? b : a; }
__device__ __forceinline__ u64 key_max(u64 a, u64 b) { return b > a ? b : a; }

// ascending bitonic sort of one key per lane across the wave
template <class T>
__device__ __forceinline__ T wave_sort(T v, int lane) {
#pragma unroll
  for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      const T p = __shfl_xor(v, j, 64);
      const bool up = (lane & k) == 0;
      const bool lo = (lane & j) == 0;
      v = (lo == up) ? key_min(v, p) : key_max(v, p);
    }
  }
  return v;
}
// best: ascending 64 smallest so far; cand: 64 new keys.  Returns the
// ascending 64 smallest of the union.
template <class T>
__device__ __forceinline__ T wave_merge_smallest(T best, T cand, int lane) {
  const T s = wave_sort(cand, lane);
  T m = key_min(best, __shfl(s, 63 - lane, 64));  // bitonic, holds the 64 smallest
#pragma unroll
  for (int j = 32; j > 0; j >>= 1) {
    const T p = __shfl_xor(m, j, 64);
    m = (lane & j) == 0 ? key_min(m, p) : key_max(m, p);
  }
  return m;
}

// The walk with a selection: every row keeps its 64 smallest keys ascending,
// one per lane of its wave, and a column tile is merged in only when one of
// its keys is below the row's current kk-th (1 <= kk <= 64).  Key supplies
// the element type T, the sentinel worst() that orders after every real key,
// and make(d2, j), the key of column j.  store(i, key) is then called for
// every row i < N of the wave (a wave-uniform condition) with lane l holding
// the row's l-th smallest key.
template <class Key, class Store>
__device__ __forceinline__ void select_smallest_a(int N, int d, int kk, const float* __restrict__ X, Store store) {
  typedef typename Key::T T;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int row0 = blockIdx.x * RA;
  T best[16];
#pragma unroll
  for (int u = 0; u < 16; ++u) best[u] = Key::worst();
  walk_columns_a(N, d, X, row0, [&](int jt, const float(&acc)[16]) {
    const int j = jt * 64 + lane;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const T cand = j < N ? Key::make(acc[u], j) : Key::worst();
      const T thr = __shfl(best[u], kk - 1, 64);
      if (__any(cand < thr)) best[u] = wave_merge_smallest(best[u], cand, lane);  // wave-uniform branch
    }
  });
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    const int i = row0 + w * 16 + u;
    if (i < N) store(i, best[u]);
  }
}

}  // namespace

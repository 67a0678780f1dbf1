// Embedding analytics on the PCA cluster space: K-Means (Lloyd assign /
// update), the DBSCAN eps-neighbourhood graph, DBSCAN label propagation
// without a stored graph (degree / walk / hook), the k-th neighbour distance
// and the per-cluster distance sums behind the silhouette score.  These stand
// in for the sklearn calls the reference makes at src/clustering.py:330-438
// (KMeans.fit_predict, DBSCAN.fit_predict, silhouette_score,
// NearestNeighbors.kneighbors).  The exact k nearest neighbours that the
// native UMAP (umap.hip) starts from are a pairwise primitive too and live
// here (ssip_knn).
//
// Points are fp32, row-major [N][d], 1 <= d <= 512.
//
// Every squared distance is the direct difference sum_c (x_c - y_c)^2,
// accumulated in fp32 with one fma per feature in feature order, over
// LDS-staged chunks of DC features.  The Gram form |x|^2 + |y|^2 - 2 x.y is
// deliberately not used: every consumer here thresholds a distance or takes
// an argmin that is compared with an fp64 oracle, the feature dimension is
// small (5-60 for the PCA cluster space), and the Gram form's cancellation
// error near d2 = 0 (self pairs, duplicates, eps thresholds) would buy
// nothing.  The direct form also gives d2(i, j) == d2(j, i) and d2(i, i) == 0
// bit for bit, so the eps graph is symmetric by construction.
//
// No atomics, with one exception: the DBSCAN hook takes an integer atomicMin
// on the label array.  A minimum of integers does not depend on the order of
// arrival, so that output is as reproducible as the rest; there are no
// floating-point atomics.  Every other reduction runs in a fixed order, so all
// outputs are bit-reproducible from run to run.  Two thread layouts:
//   A (eps graph and degree, DBSCAN walk, k-th distance, exact kNN; the t-SNE
//     distances of tsne.hip):
//     a workgroup owns RA = 64 rows and walks all columns in tiles of 64
//     (pairwise_tile.h); lane = column, each wave holds 16 rows, so one wave
//     ballot is 64 columns of one row = two bitmap words.  The k-th distance
//     and the kNN are one selection body over two key types.
//   B (assign, cluster sums): a workgroup owns RB = 256 rows, thread = row,
//     and walks the columns (centres / points in label order) in tiles of 16;
//     everything that depends on the column is uniform across the workgroup.
#include "ssip_common.h"
#include "pairwise_tile.h"

#include <math.h>

namespace {

constexpr int RB = 256;       // layout B: rows per workgroup
constexpr int CT = 16;        // layout B: columns per tile
constexpr int KMAX = 64;      // centres
constexpr int UPD_NT = 1024;  // update: one workgroup

constexpr int KNN_MAX_N = 1 << 20;
constexpr int KNN_MAX_K = 64;
constexpr int DBSCAN_MAX_N = 1 << 20;
constexpr int DBSCAN_MAX_M = 4;  // min_samples configurations of one walk

// ---------------------------------------------------------------------------
// layout A (the walk and the selection are pairwise_tile.h's)
// ---------------------------------------------------------------------------
// degree and (BITMAP) adjacency bitmap of d2 <= eps2
template <bool BITMAP>
__global__ __launch_bounds__(NT) void pairwise_eps_kernel(int N, int d, const float* __restrict__ X, float eps2,
                                                          int* __restrict__ degree, uint32_t* __restrict__ bitmap) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int row0 = blockIdx.x * RA;
  const int W = (N + 31) / 32;
  int deg[16];
#pragma unroll
  for (int u = 0; u < 16; ++u) deg[u] = 0;
  walk_columns_a(N, d, X, row0, [&](int jt, const float(&acc)[16]) {
    const int j = jt * 64 + lane;
    unsigned long long mine = 0;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int i = row0 + w * 16 + u;
      const unsigned long long m = __ballot(j < N && i < N && acc[u] <= eps2);
      deg[u] += __popcll(m);
      if ((lane >> 1) == u) mine = m;
    }
    if constexpr (BITMAP) {
      // lanes 0..31 store the wave's 16 rows x 2 words
      const int i = row0 + w * 16 + (lane >> 1), wi = jt * 2 + (lane & 1);
      if (lane < 32 && i < N && wi < W)
        bitmap[(long)i * W + wi] = (uint32_t)((lane & 1) ? (mine >> 32) : (mine & 0xffffffffull));
    }
  });
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    const int i = row0 + w * 16 + u;
    if (lane == u && i < N) degree[i] = deg[u];
  }
}

// One DBSCAN label walk for M min_samples configurations over one tile of
// d2: nbr_min[m][i] = min of labels[m][j] over the columns j that are core in
// configuration m (degree[j] >= min_samples[m]) and have d2(i, j) <= eps2, N
// when there is none.  The predicate is pairwise_eps_kernel's, so the pair set
// is the bitmap's bit for bit.  lane = column: the lane fetches its column's
// degree and M labels once per tile and keeps a running minimum per (m, row);
// the 64 lanes of a row are reduced once, after the walk.  A label outside
// 0..N-1 counts as N.
template <int M>
__global__ __launch_bounds__(NT) void dbscan_walk_kernel(int N, int d, const float* __restrict__ X, float eps2,
                                                         const int* __restrict__ degree,
                                                         const int* __restrict__ min_samples,
                                                         const int* __restrict__ labels, int* __restrict__ nbr_min) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int row0 = blockIdx.x * RA;
  int ms[M];
#pragma unroll
  for (int m = 0; m < M; ++m) ms[m] = min_samples[m];
  int mn[M][16];
#pragma unroll
  for (int m = 0; m < M; ++m)
#pragma unroll
    for (int u = 0; u < 16; ++u) mn[m][u] = N;
  walk_columns_a(N, d, X, row0, [&](int jt, const float(&acc)[16]) {
    const int j = jt * 64 + lane;
    const int dj = j < N ? degree[j] : 0;
    int cl[M];
#pragma unroll
    for (int m = 0; m < M; ++m) cl[m] = j < N ? labels[(long)m * N + j] : N;
    unsigned hits = 0;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int i = row0 + w * 16 + u;
      hits |= (unsigned)(j < N && i < N && acc[u] <= eps2) << u;
    }
    if (!__any(hits != 0)) return;  // wave-uniform: no pair of this tile is within eps
#pragma unroll
    for (int m = 0; m < M; ++m) {
      if (dj < ms[m] || (unsigned)cl[m] >= (unsigned)N) cl[m] = N;
#pragma unroll
      for (int u = 0; u < 16; ++u) mn[m][u] = min(mn[m][u], ((hits >> u) & 1u) ? cl[m] : N);
    }
  });
#pragma unroll
  for (int m = 0; m < M; ++m) {
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      int v = mn[m][u];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
      const int i = row0 + w * 16 + u;
      if (lane == u && i < N) nbr_min[(long)m * N + i] = v;
    }
  }
}

// The hook of one DBSCAN round, thread = (configuration m, row i) = idx / N,
// idx % N.  copy: out = in, changed = 0.  min: every core row i hooks its
// neighbourhood minimum onto itself and onto its current label's row.  jump:
// dst[i] = src[src[i]] on core rows (Jacobi: src is read only, dst written
// only); the last jump reports a difference from the round's input labels.  A
// label or minimum outside 0..N-1 is never used as an index.
constexpr int HOOK_NT = 256;
__global__ __launch_bounds__(HOOK_NT) void dbscan_hook_copy_kernel(int N, int M, const int* __restrict__ in,
                                                                   int* __restrict__ out, int* __restrict__ changed) {
  const int idx = blockIdx.x * HOOK_NT + threadIdx.x;
  if (idx < M * N) out[idx] = in[idx];
  if (idx < M) changed[idx] = 0;
}
__global__ __launch_bounds__(HOOK_NT) void dbscan_hook_min_kernel(int N, int M, const int* __restrict__ degree,
                                                                  const int* __restrict__ min_samples,
                                                                  const int* __restrict__ in,
                                                                  const int* __restrict__ nbr_min, int* out) {
  const int idx = blockIdx.x * HOOK_NT + threadIdx.x;
  if (idx >= M * N) return;
  const int m = idx / N, i = idx - m * N;
  if (degree[i] < min_samples[m]) return;
  const int nm = nbr_min[idx], l = in[idx];
  if ((unsigned)nm >= (unsigned)N) return;
  if ((unsigned)l < (unsigned)N) atomicMin(&out[m * N + l], nm);
  atomicMin(&out[idx], nm);
}
template <bool LAST>
__global__ __launch_bounds__(HOOK_NT) void dbscan_hook_jump_kernel(int N, int M, const int* __restrict__ degree,
                                                                   const int* __restrict__ min_samples,
                                                                   const int* __restrict__ src, int* __restrict__ dst,
                                                                   const int* __restrict__ in,
                                                                   int* __restrict__ changed) {
  const int idx = blockIdx.x * HOOK_NT + threadIdx.x;
  if (idx >= M * N) return;
  const int m = idx / N, i = idx - m * N;
  int v = src[idx];
  if (degree[i] >= min_samples[m] && (unsigned)v < (unsigned)N) v = src[m * N + v];
  dst[idx] = v;
  if (LAST && v != in[idx]) changed[m] = 1;  // every writer stores the same value
}

// k-th distance: the key is the squared distance alone
struct DistKey {
  typedef float T;
  static __device__ T worst() { return INFINITY; }
  static __device__ T make(float d2, int) { return d2; }
};
// kNN: the bits of the squared distance above the column index.  d2 >= 0, so
// keys order by distance and then by index, and no two keys are equal; hence
// the first k' keys of a k result are the k' result.
struct DistIndexKey {
  typedef u64 T;
  static __device__ T worst() { return ~0ull; }
  static __device__ T make(float d2, int j) { return ((u64)__float_as_uint(d2) << 32) | (u64)(uint32_t)j; }
};

__global__ __launch_bounds__(NT) void pairwise_kth_kernel(int N, int d, int kk, const float* __restrict__ X,
                                                          float* __restrict__ kth) {
  const int lane = threadIdx.x & 63;
  select_smallest_a<DistKey>(N, d, kk, X, [&](int i, float key) {
    if (lane == kk - 1) kth[i] = sqrtf(key);
  });
}

// k <= N, so the first k keys of every row are real candidates
__global__ __launch_bounds__(NT) void knn_kernel(int N, int d, int kk, const float* __restrict__ X,
                                                 float* __restrict__ d2out, int32_t* __restrict__ idxout) {
  const int lane = threadIdx.x & 63;
  select_smallest_a<DistIndexKey>(N, d, kk, X, [&](int i, u64 key) {
    if (lane < kk) {
      d2out[(long)i * kk + lane] = __uint_as_float((uint32_t)(key >> 32));
      idxout[(long)i * kk + lane] = (int32_t)(uint32_t)(key & 0xffffffffull);
    }
  });
}

// ---------------------------------------------------------------------------
// layout B
// ---------------------------------------------------------------------------
// xs[r][c] = X[row0 + r][c0 + c] (zero outside the matrix)
__device__ __forceinline__ void stage_rows_b(float* xs, const float* __restrict__ X, long row0, long N, int d, int c0,
                                             int tid) {
  for (int idx = tid; idx < RB * DC; idx += NT) {
    const int r = idx >> 5, cc = idx & (DC - 1);
    const long row = row0 + r;
    const int c = c0 + cc;
    xs[r * XC_LD + cc] = (row < N && c < d) ? X[row * d + c] : 0.f;
  }
}
// ys[c][u] = Y[col_s[u]][c0 + c] (zero for col_s[u] < 0 or outside d)
__device__ __forceinline__ void stage_cols_b(float* ys, const float* __restrict__ Y, const int* col_s, int d, int c0,
                                             int tid) {
  for (int idx = tid; idx < CT * DC; idx += NT) {
    const int u = idx >> 5, cc = idx & (DC - 1);
    const int col = col_s[u], c = c0 + cc;
    ys[cc * CT + u] = (col >= 0 && c < d) ? Y[(long)col * d + c] : 0.f;
  }
}
__device__ __forceinline__ void accumulate_b(float (&acc)[CT], const float* xs, const float* ys, int tid) {
#pragma unroll 4
  for (int cc = 0; cc < DC; ++cc) {
    const float xv = xs[tid * XC_LD + cc];
    const f32x4* yp = reinterpret_cast<const f32x4*>(ys + cc * CT);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 yv = yp[q];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float df = xv - yv[e];
        acc[q * 4 + e] = fmaf(df, df, acc[q * 4 + e]);
      }
    }
  }
}

// Workspace of the Lloyd iteration, G = ceil(N / RB) workgroups.
struct KmeansWs {
  double* inertia;  // [G]
  int* changed;     // [G]
  int* counts;      // [G][K]
  float* sums;      // [G][K][d]
};
inline long kmeans_groups(long N) { return (N + RB - 1) / RB; }
inline long kmeans_ws_bytes(long N, int d, int K) {
  const long G = kmeans_groups(N);
  long b = G * 8 + G * 4 + G * K * 4;
  b = (b + 15) / 16 * 16;
  return b + G * K * d * 4;
}
inline KmeansWs kmeans_ws(void* base, long N, int d, int K) {
  const long G = kmeans_groups(N);
  char* p = static_cast<char*>(base);
  KmeansWs ws;
  ws.inertia = reinterpret_cast<double*>(p);
  ws.changed = reinterpret_cast<int*>(p + G * 8);
  ws.counts = reinterpret_cast<int*>(p + G * 8 + G * 4);
  const long b = (G * 8 + G * 4 + G * K * 4 + 15) / 16 * 16;
  ws.sums = reinterpret_cast<float*>(p + b);
  return ws;
}

__global__ __launch_bounds__(NT) void kmeans_assign_kernel(long N, int d, int K, const float* __restrict__ X,
                                                           const float* __restrict__ C, const int* __restrict__ prev,
                                                           int* __restrict__ labels, float* __restrict__ mind2,
                                                           KmeansWs ws) {
  __shared__ float xs[RB * XC_LD];
  __shared__ __attribute__((aligned(16))) float ys[DC * CT];
  __shared__ int col_s[CT];
  __shared__ int lab_s[RB];
  __shared__ float red_f[NT / 64];
  __shared__ int red_i[NT / 64];
  const int tid = threadIdx.x;
  const long row0 = (long)blockIdx.x * RB, row = row0 + tid;
  const bool valid = row < N;
  const int nch = (d + DC - 1) / DC;

  float best = INFINITY;
  int bi = 0;
  for (int kt = 0; kt * CT < K; ++kt) {
    __syncthreads();
    if (tid < CT) col_s[tid] = kt * CT + tid < K ? kt * CT + tid : -1;
    __syncthreads();
    float acc[CT];
#pragma unroll
    for (int u = 0; u < CT; ++u) acc[u] = 0.f;
    for (int ch = 0; ch < nch; ++ch) {
      if (nch > 1 || kt == 0) stage_rows_b(xs, X, row0, N, d, ch * DC, tid);
      stage_cols_b(ys, C, col_s, d, ch * DC, tid);
      __syncthreads();
      accumulate_b(acc, xs, ys, tid);
      __syncthreads();
    }
    // strict <, centres in increasing index: a tie keeps the lowest index (numpy.argmin)
#pragma unroll
    for (int u = 0; u < CT; ++u) {
      const int k = kt * CT + u;
      if (k < K && acc[u] < best) {
        best = acc[u];
        bi = k;
      }
    }
  }
  int chg = 0;
  if (valid) {
    labels[row] = bi;
    mind2[row] = best;
    chg = prev == nullptr || prev[row] != bi;
  }
  lab_s[tid] = valid ? bi : -1;

  // inertia and changed-label partials of this workgroup (butterfly within a
  // wave, then the four waves in order)
  const float ws_f = wave_sum(valid ? best : 0.f);
  int ws_i = chg;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ws_i += __shfl_xor(ws_i, o, 64);
  if ((tid & 63) == 0) {
    red_f[tid >> 6] = ws_f;
    red_i[tid >> 6] = ws_i;
  }
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    int c = 0;
    for (int q = 0; q < NT / 64; ++q) {
      s += (double)red_f[q];
      c += red_i[q];
    }
    ws.inertia[blockIdx.x] = s;
    ws.changed[blockIdx.x] = c;
  }
  if (tid < K) {
    int c = 0;
    for (int r = 0; r < RB; ++r) c += lab_s[r] == tid;
    ws.counts[(long)blockIdx.x * K + tid] = c;
  }

  // per-cluster sums of this workgroup's points, rows in order.  Thread
  // (c = feature of the chunk, g = tid / 32) owns clusters g, g + 8, ...
  const int c = tid & (DC - 1), g = tid >> 5;
  for (int ch = 0; ch < nch; ++ch) {
    if (nch > 1) {
      __syncthreads();
      stage_rows_b(xs, X, row0, N, d, ch * DC, tid);
      __syncthreads();
    }
    float a[KMAX / 8];
#pragma unroll
    for (int m = 0; m < KMAX / 8; ++m) a[m] = 0.f;
    for (int r = 0; r < RB; ++r) {
      const int l = lab_s[r];
      if (l >= 0 && (l & 7) == g) {
        const float x = xs[r * XC_LD + c];
        const int mm = l >> 3;
#pragma unroll
        for (int m = 0; m < KMAX / 8; ++m) a[m] += (m == mm) ? x : 0.f;
      }
    }
#pragma unroll
    for (int m = 0; m < KMAX / 8; ++m) {
      const int k = g + 8 * m;
      if (k < K && ch * DC + c < d) ws.sums[((long)blockIdx.x * K + k) * d + ch * DC + c] = a[m];
    }
  }
}

// One workgroup: reduce the G partials in index order (fp64), new centres,
// counts and the scalars {sum |delta centre|^2, inertia, changed labels,
// empty clusters}.
__global__ __launch_bounds__(UPD_NT) void kmeans_update_kernel(long G, int d, int K, KmeansWs ws,
                                                               const float* __restrict__ C, float* __restrict__ Cn,
                                                               int* __restrict__ counts, double* __restrict__ scalars) {
  __shared__ int cnt_s[KMAX];
  __shared__ double red[3][UPD_NT];
  const int tid = threadIdx.x;
  if (tid < K) {
    int c = 0;
    for (long g = 0; g < G; ++g) c += ws.counts[g * K + tid];
    cnt_s[tid] = c;
    counts[tid] = c;
  }
  __syncthreads();
  double shift = 0.0, inertia = 0.0, changed = 0.0;
  for (int slot = tid; slot < K * d; slot += UPD_NT) {
    const int k = slot / d;
    double s = 0.0;
    for (long g = 0; g < G; ++g) s += (double)ws.sums[g * K * d + slot];
    const float old = C[slot];
    const float nw = cnt_s[k] > 0 ? (float)(s / (double)cnt_s[k]) : old;  // an empty cluster keeps its centre
    Cn[slot] = nw;
    const double df = (double)nw - (double)old;
    shift += df * df;
  }
  for (long g = tid; g < G; g += UPD_NT) {
    inertia += ws.inertia[g];
    changed += (double)ws.changed[g];
  }
  red[0][tid] = shift;
  red[1][tid] = inertia;
  red[2][tid] = changed;
  __syncthreads();
  for (int s = UPD_NT / 2; s > 0; s >>= 1) {
    if (tid < s) {
#pragma unroll
      for (int q = 0; q < 3; ++q) red[q][tid] += red[q][tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    int empty = 0;
    for (int k = 0; k < K; ++k) empty += cnt_s[k] == 0;
    scalars[0] = red[0][0];
    scalars[1] = red[1][0];
    scalars[2] = red[2][0];
    scalars[3] = (double)empty;
  }
}

// sums[row][label] = sum of distances from the row to that cluster's members.
// Columns come in label order, so each (row, label) slot is stored exactly
// once, when the label of the walk changes (uniform across the workgroup).
// Columns are staged SC = 64 at a time (four tiles of CT), which amortises the
// order -> labels -> X chain of dependent loads and the barriers; the indices
// of the next stage are fetched during the arithmetic of the current one.
constexpr int SC = 64;
__global__ __launch_bounds__(NT) void cluster_sums_kernel(int N, int d, int K, const float* __restrict__ X,
                                                          const int* __restrict__ labels, const int* __restrict__ order,
                                                          float* __restrict__ sums) {
  __shared__ float xs[RB * XC_LD];
  __shared__ __attribute__((aligned(16))) float ys[SC / CT][DC * CT];
  __shared__ int col_s[SC];
  __shared__ int lab_s[SC];
  const int tid = threadIdx.x;
  const long row0 = (long)blockIdx.x * RB, row = row0 + tid;
  const int nch = (d + DC - 1) / DC;
  float run = 0.f;
  int cur = -1;

  // (column, label) of stage position tid; -1 / -1 when it is not a member of any cluster
  auto fetch_index = [&](int j, int& col, int& l) {
    col = j < N ? order[j] : -1;
    if (col < 0 || col >= N) col = -1;
    l = col >= 0 ? labels[col] : -1;
    if (l < 0 || l >= K) {
      l = -1;
      col = -1;
    }
  };
  int ncol = -1, nlab = -1;
  if (tid < SC) fetch_index(tid, ncol, nlab);

  for (int j0 = 0; j0 < N; j0 += SC) {
    __syncthreads();
    if (tid < SC) {
      col_s[tid] = ncol;
      lab_s[tid] = nlab;
    }
    __syncthreads();
    if (tid < SC) fetch_index(j0 + SC + tid, ncol, nlab);
    float acc[SC];
#pragma unroll
    for (int u = 0; u < SC; ++u) acc[u] = 0.f;
    for (int ch = 0; ch < nch; ++ch) {
      if (nch > 1 || j0 == 0) stage_rows_b(xs, X, row0, N, d, ch * DC, tid);
#pragma unroll
      for (int t = 0; t < SC / CT; ++t) stage_cols_b(ys[t], X, col_s + t * CT, d, ch * DC, tid);
      __syncthreads();
#pragma unroll
      for (int t = 0; t < SC / CT; ++t) {
        float a[CT];
#pragma unroll
        for (int u = 0; u < CT; ++u) a[u] = acc[t * CT + u];
        accumulate_b(a, xs, ys[t], tid);
#pragma unroll
        for (int u = 0; u < CT; ++u) acc[t * CT + u] = a[u];
      }
      __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < SC; ++u) {
      const int l = lab_s[u];
      if (l != cur) {
        if (cur >= 0 && row < N) sums[row * K + cur] = run;
        run = 0.f;
        cur = l;
      }
      if (l >= 0) run += sqrtf(acc[u]);
    }
  }
  if (cur >= 0 && row < N) sums[row * K + cur] = run;
}

// true when two int32 [M][N] arrays share a byte
inline bool dbscan_overlap(const void* p, const void* q, long N, int M) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  const uintptr_t bytes = (uintptr_t)N * M * sizeof(int32_t);
  return a < b + bytes && b < a + bytes;
}

}  // namespace

extern "C" {

int64_t ssip_kmeans_workspace_bytes(int64_t N, int d, int K) {
  SSIP_REQUIRE(N >= 1 && d >= 1 && d <= 512 && K >= 2 && K <= KMAX, SSIP_ERR_ARG,
               "ssip_kmeans_workspace_bytes: need N >= 1, 1 <= d <= 512, 2 <= K <= 64 (N=%ld d=%d K=%d)", (long)N, d,
               K);
  return kmeans_ws_bytes(N, d, K);
}

int ssip_kmeans_assign(int64_t N, int d, int K, const float* X, const float* centres, const int32_t* prev_labels,
                       int32_t* labels, float* mind2, void* workspace, int64_t workspace_bytes, void* stream) {
  if (int rc = check_points("ssip_kmeans_assign", N, d, X)) return rc;
  SSIP_REQUIRE(K >= 2 && K <= KMAX, SSIP_ERR_ARG, "ssip_kmeans_assign: K = %d outside 2..64", K);
  SSIP_REQUIRE(centres && labels && mind2 && workspace, SSIP_ERR_ARG, "ssip_kmeans_assign: null pointer");
  if (int rc = check_workspace("ssip_kmeans_assign", workspace, workspace_bytes, kmeans_ws_bytes(N, d, K))) return rc;
  const long G = kmeans_groups(N);
  SSIP_REQUIRE(G <= 0x7fffffffL, SSIP_ERR_ARG, "ssip_kmeans_assign: N = %ld too large", (long)N);
  SSIP_KLAUNCH(kmeans_assign_kernel, dim3((unsigned)G), dim3(NT), 0, (hipStream_t)stream, (long)N, d, K, X, centres,
               prev_labels, labels, mind2, kmeans_ws(workspace, N, d, K));
  return ssip::check_launch("ssip_kmeans_assign");
}

int ssip_kmeans_update(int64_t N, int d, int K, const void* workspace, int64_t workspace_bytes, const float* centres,
                       float* new_centres, int32_t* counts, double* scalars, void* stream) {
  SSIP_REQUIRE(N >= 1 && d >= 1 && d <= 512 && K >= 2 && K <= KMAX, SSIP_ERR_ARG,
               "ssip_kmeans_update: need N >= 1, 1 <= d <= 512, 2 <= K <= 64 (N=%ld d=%d K=%d)", (long)N, d, K);
  SSIP_REQUIRE(workspace && centres && new_centres && counts && scalars, SSIP_ERR_ARG,
               "ssip_kmeans_update: null pointer");
  // the alignment is the one ssip_kmeans_assign demands of the same buffer
  if (int rc = check_workspace("ssip_kmeans_update", workspace, workspace_bytes, kmeans_ws_bytes(N, d, K))) return rc;
  SSIP_KLAUNCH(kmeans_update_kernel, dim3(1), dim3(UPD_NT), 0, (hipStream_t)stream, kmeans_groups(N), d, K,
               kmeans_ws(const_cast<void*>(workspace), N, d, K), centres, new_centres, counts, scalars);
  return ssip::check_launch("ssip_kmeans_update");
}

int ssip_pairwise_eps(int N, int d, const float* X, float eps, int32_t* degree, uint32_t* bitmap, void* stream) {
  if (int rc = check_points("ssip_pairwise_eps", N, d, X)) return rc;
  SSIP_REQUIRE(N <= 65536, SSIP_ERR_ARG,
               "ssip_pairwise_eps: N = %d above 65536 (the adjacency bitmap would exceed 512 MB)", N);
  SSIP_REQUIRE(eps >= 0.f, SSIP_ERR_ARG, "ssip_pairwise_eps: eps = %g must be >= 0", (double)eps);
  SSIP_REQUIRE(degree && bitmap, SSIP_ERR_ARG, "ssip_pairwise_eps: null pointer");
  SSIP_KLAUNCH(pairwise_eps_kernel<true>, dim3((N + RA - 1) / RA), dim3(NT), 0, (hipStream_t)stream, N, d, X, eps * eps,
               degree, bitmap);
  return ssip::check_launch("ssip_pairwise_eps");
}

int ssip_pairwise_degree(int N, int d, const float* X, float eps, int32_t* degree, void* stream) {
  if (int rc = check_points("ssip_pairwise_degree", N, d, X)) return rc;
  SSIP_REQUIRE(N <= DBSCAN_MAX_N, SSIP_ERR_ARG, "ssip_pairwise_degree: N = %d above %d", N, DBSCAN_MAX_N);
  SSIP_REQUIRE(eps >= 0.f, SSIP_ERR_ARG, "ssip_pairwise_degree: eps = %g must be >= 0", (double)eps);
  SSIP_REQUIRE(degree != nullptr, SSIP_ERR_ARG, "ssip_pairwise_degree: null pointer");
  SSIP_KLAUNCH(pairwise_eps_kernel<false>, dim3((N + RA - 1) / RA), dim3(NT), 0, (hipStream_t)stream, N, d, X,
               eps * eps, degree, (uint32_t*)nullptr);
  return ssip::check_launch("ssip_pairwise_degree");
}

int ssip_dbscan_walk(int N, int d, const float* X, float eps, int M, const int32_t* degree, const int32_t* min_samples,
                     const int32_t* labels, int32_t* nbr_min, void* stream) {
  if (int rc = check_points("ssip_dbscan_walk", N, d, X)) return rc;
  SSIP_REQUIRE(N <= DBSCAN_MAX_N, SSIP_ERR_ARG, "ssip_dbscan_walk: N = %d above %d", N, DBSCAN_MAX_N);
  SSIP_REQUIRE(eps >= 0.f, SSIP_ERR_ARG, "ssip_dbscan_walk: eps = %g must be >= 0", (double)eps);
  SSIP_REQUIRE(M >= 1 && M <= DBSCAN_MAX_M, SSIP_ERR_ARG, "ssip_dbscan_walk: M = %d outside 1..%d", M, DBSCAN_MAX_M);
  SSIP_REQUIRE(degree && min_samples && labels && nbr_min, SSIP_ERR_ARG, "ssip_dbscan_walk: null pointer");
  SSIP_REQUIRE(!dbscan_overlap(labels, nbr_min, N, M), SSIP_ERR_ARG,
               "ssip_dbscan_walk: nbr_min must not alias labels");
  auto kernel = dbscan_walk_kernel<1>;  // one instance per M: the minima live in registers
  if (M == 2) kernel = dbscan_walk_kernel<2>;
  if (M == 3) kernel = dbscan_walk_kernel<3>;
  if (M == 4) kernel = dbscan_walk_kernel<4>;
  SSIP_KLAUNCH(kernel, dim3((N + RA - 1) / RA), dim3(NT), 0, (hipStream_t)stream, N, d, X, eps * eps, degree,
               min_samples, labels, nbr_min);
  return ssip::check_launch("ssip_dbscan_walk");
}

int ssip_dbscan_hook(int N, int M, const int32_t* degree, const int32_t* min_samples, const int32_t* labels_in,
                     const int32_t* nbr_min, int32_t* labels_out, int32_t* scratch, int32_t* changed, void* stream) {
  SSIP_REQUIRE(N >= 1 && N <= DBSCAN_MAX_N, SSIP_ERR_ARG, "ssip_dbscan_hook: N = %d outside 1..%d", N, DBSCAN_MAX_N);
  SSIP_REQUIRE(M >= 1 && M <= DBSCAN_MAX_M, SSIP_ERR_ARG, "ssip_dbscan_hook: M = %d outside 1..%d", M, DBSCAN_MAX_M);
  SSIP_REQUIRE(degree && min_samples && labels_in && nbr_min && labels_out && scratch && changed, SSIP_ERR_ARG,
               "ssip_dbscan_hook: null pointer");
  SSIP_REQUIRE(!dbscan_overlap(labels_in, labels_out, N, M) && !dbscan_overlap(labels_in, scratch, N, M) &&
                   !dbscan_overlap(labels_out, scratch, N, M) && !dbscan_overlap(nbr_min, labels_out, N, M) &&
                   !dbscan_overlap(nbr_min, scratch, N, M),
               SSIP_ERR_ARG,
               "ssip_dbscan_hook: labels_out and scratch must not alias labels_in, nbr_min or each other");
  // ceil(log2 N) jumps (at least one, which carries the comparison) halve
  // every chain of decreasing labels down to its root.  They alternate
  // between two buffers, started so that the last one writes labels_out.
  int jumps = 0;
  while ((1L << jumps) < N) ++jumps;
  if (jumps < 1) jumps = 1;
  int* a = (jumps % 2 == 0) ? labels_out : scratch;
  int* b = (jumps % 2 == 0) ? scratch : labels_out;
  const dim3 grid((M * N + HOOK_NT - 1) / HOOK_NT), block(HOOK_NT);
  const hipStream_t st = (hipStream_t)stream;
  SSIP_KLAUNCH(dbscan_hook_copy_kernel, grid, block, 0, st, N, M, labels_in, a, changed);
  SSIP_KLAUNCH(dbscan_hook_min_kernel, grid, block, 0, st, N, M, degree, min_samples, labels_in, nbr_min, a);
  for (int k = 0; k < jumps; ++k) {
    const int* src = (k % 2 == 0) ? a : b;
    int* dst = (k % 2 == 0) ? b : a;
    if (k == jumps - 1)
      SSIP_KLAUNCH(dbscan_hook_jump_kernel<true>, grid, block, 0, st, N, M, degree, min_samples, src, dst, labels_in,
                   changed);
    else
      SSIP_KLAUNCH(dbscan_hook_jump_kernel<false>, grid, block, 0, st, N, M, degree, min_samples, src, dst, labels_in,
                   changed);
  }
  return ssip::check_launch("ssip_dbscan_hook");
}

int ssip_pairwise_kth(int N, int d, int k, const float* X, float* kth, void* stream) {
  if (int rc = check_points("ssip_pairwise_kth", N, d, X)) return rc;
  SSIP_REQUIRE(k >= 1 && k <= 64, SSIP_ERR_ARG, "ssip_pairwise_kth: k = %d outside 1..64", k);
  SSIP_REQUIRE(k <= N, SSIP_ERR_ARG, "ssip_pairwise_kth: k = %d neighbours asked of N = %d points", k, N);
  SSIP_REQUIRE(kth != nullptr, SSIP_ERR_ARG, "ssip_pairwise_kth: null pointer");
  SSIP_KLAUNCH(pairwise_kth_kernel, dim3((N + RA - 1) / RA), dim3(NT), 0, (hipStream_t)stream, N, d, k, X, kth);
  return ssip::check_launch("ssip_pairwise_kth");
}

int ssip_knn(int N, int d, int k, const float* X, float* d2, int32_t* idx, void* stream) {
  SSIP_REQUIRE(N >= 2 && N <= KNN_MAX_N, SSIP_ERR_ARG, "ssip_knn: N = %d outside 2..%d", N, KNN_MAX_N);
  if (int rc = check_points("ssip_knn", N, d, X)) return rc;
  SSIP_REQUIRE(k >= 2 && k <= KNN_MAX_K, SSIP_ERR_ARG, "ssip_knn: k = %d outside 2..%d", k, KNN_MAX_K);
  SSIP_REQUIRE(k <= N, SSIP_ERR_ARG, "ssip_knn: k = %d neighbours asked of N = %d points", k, N);
  SSIP_REQUIRE(d2 && idx, SSIP_ERR_ARG, "ssip_knn: null pointer");
  SSIP_KLAUNCH(knn_kernel, dim3((N + RA - 1) / RA), dim3(NT), 0, (hipStream_t)stream, N, d, k, X, d2, idx);
  return ssip::check_launch("ssip_knn");
}

int ssip_pairwise_cluster_sums(int N, int d, int K, const float* X, const int32_t* labels, const int32_t* order,
                               float* sums, void* stream) {
  if (int rc = check_points("ssip_pairwise_cluster_sums", N, d, X)) return rc;
  SSIP_REQUIRE(K >= 1 && K <= 256, SSIP_ERR_ARG, "ssip_pairwise_cluster_sums: K = %d outside 1..256", K);
  SSIP_REQUIRE(labels && order && sums, SSIP_ERR_ARG, "ssip_pairwise_cluster_sums: null pointer");
  // a cluster without members keeps a zero column
  if (hipMemsetAsync(sums, 0, (size_t)N * K * sizeof(float), (hipStream_t)stream) != hipSuccess) {
    ssip::set_error("ssip_pairwise_cluster_sums: hipMemsetAsync failed");
    return SSIP_ERR_LAUNCH;
  }
  SSIP_KLAUNCH(cluster_sums_kernel, dim3((N + RB - 1) / RB), dim3(NT), 0, (hipStream_t)stream, N, d, K, X, labels,
               order, sums);
  return ssip::check_launch("ssip_pairwise_cluster_sums");
}

}  // extern "C"

// Native UMAP (reference src/clustering.py:279-306, which calls umap.UMAP):
// the two device stages of ssip.analytics.umap_fit that follow the exact kNN
// (ssip_knn, a pairwise kernel of analytics.hip).  The algorithm is
// umap-learn's (nearest neighbours -> smooth_knn_dist -> membership strengths
// -> optimize_layout_euclidean); the graph symmetrisation, the a / b curve
// fit, the schedule and the initial layout are O(N k) host work.
//
// Everything is fp32 unless said otherwise.  No atomics; every reduction runs
// in a fixed order, so all outputs are bit-reproducible from run to run.
//
//   fuzzy:  one wave per row, lane = neighbour column.  rho by a wave minimum,
//           sigma by umap's bisection with exp and the sums in fp64.  The mean
//           of all distances (the sigma floor of rows with rho = 0) is reduced
//           per row, then over the rows by one workgroup in index order.
//   epoch:  one wave per vertex, lanes stride over its CSR row.  Epochs are
//           Jacobi-ordered (read y_in, write y_out), so no vertex sees a
//           half-updated neighbour and the result does not depend on the
//           order the waves run in.  A lane owns the schedule state of the
//           edges it visits; the forces and the per-vertex sum (the lanes'
//           running sums through a fixed butterfly) are fp64, then one plain
//           8-byte store of the fp32 position.
#include "ssip_common.h"

#include <math.h>

namespace {

constexpr int UMAP_MAX_N = 1 << 20;
constexpr int KNN_MAX_K = 64;       // columns of a kNN result (ssip_knn)
constexpr int NT = 256;             // threads per workgroup: four rows / vertices, one per wave
constexpr int FIN_NT = 256;         // global mean: one workgroup
constexpr int BISECT_STEPS = 64;    // umap's n_iter
constexpr int MAX_NEG = 65536;      // draws of one edge in one epoch (eps >= 1 gives n_neg <= 5 n)

// ---------------------------------------------------------------------------
// smooth_knn_dist + membership strengths
// ---------------------------------------------------------------------------
struct UmapWs {
  double* rowsum;  // [N] sum of the row's k distances
  double* total;   // [1] sum of rowsum in index order
};
inline long umap_ws_bytes(long N) { return (N + 1) * 8 + 8; }
inline UmapWs umap_ws(void* base, long N) {
  UmapWs ws;
  ws.rowsum = static_cast<double*>(base);
  ws.total = ws.rowsum + N;
  return ws;
}

// the distance umap sees: sqrt of the kNN squared distance, rounded to fp32
// once (the fp64 root of an fp32 value rounds to the correctly rounded fp32 root)
__device__ __forceinline__ float knn_dist(float d2) { return (float)sqrt((double)d2); }

// wave = row, lane = column
__global__ __launch_bounds__(NT) void umap_rowsum_kernel(int N, int k, int ld, const float* __restrict__ d2,
                                                         double* __restrict__ rowsum) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
  if (i >= N) return;  // wave-uniform
  const double v = lane < k ? (double)knn_dist(d2[(long)i * ld + lane]) : 0.0;
  const double s = wave_sum_d(v);
  if (lane == 0) rowsum[i] = s;
}

// One workgroup: total = sum of rowsum, thread-strided, then wave butterfly,
// then the waves in order
__global__ __launch_bounds__(FIN_NT) void umap_total_kernel(int N, const double* __restrict__ rowsum,
                                                            double* __restrict__ total) {
  __shared__ double slot[FIN_NT / 64];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int q = tid; q < N; q += FIN_NT) s += rowsum[q];
  s = block_sum_d(s, slot, tid);
  if (tid == 0) *total = s;
}

__global__ __launch_bounds__(NT) void umap_fuzzy_kernel(int N, int k, int ld, const float* __restrict__ d2,
                                                        const int32_t* __restrict__ idx, UmapWs ws,
                                                        float* __restrict__ rho_out, float* __restrict__ sigma_out,
                                                        float* __restrict__ memb) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
  if (i >= N) return;  // wave-uniform
  const bool in = lane < k;
  const float dist = in ? knn_dist(d2[(long)i * ld + lane]) : 0.f;

  float m = (in && dist > 0.f) ? dist : INFINITY;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fminf(m, __shfl_xor(m, o, 64));
  const float rho = m == INFINITY ? 0.f : m;

  const double target = log2((double)k);
  const double dd = (double)dist - (double)rho;
  const bool counted = in && lane >= 1;
  double lo = 0.0, hi = INFINITY, mid = 1.0;
  for (int l = 0; l < BISECT_STEPS; ++l) {
    const double term = counted ? (dd > 0.0 ? exp(-dd / mid) : 1.0) : 0.0;
    const double psum = wave_sum_d(term);  // the same bits in every lane
    if (fabs(psum - target) < 1e-5) break;
    if (psum > target) {
      hi = mid;
      mid = (lo + hi) / 2.0;
    } else {
      lo = mid;
      mid = hi == INFINITY ? mid * 2.0 : (lo + hi) / 2.0;
    }
  }
  const double mean = rho > 0.f ? ws.rowsum[i] / (double)k : *ws.total / ((double)N * (double)k);
  if (mid < 1e-3 * mean) mid = 1e-3 * mean;

  if (in) {
    float v;
    if (idx[(long)i * ld + lane] == i)
      v = 0.f;
    else if (dd <= 0.0 || mid == 0.0)
      v = 1.f;
    else
      v = (float)exp(-dd / mid);
    memb[(long)i * k + lane] = v;
  }
  if (lane == 0) {
    rho_out[i] = rho;
    sigma_out[i] = (float)mid;
  }
}

// ---------------------------------------------------------------------------
// layout epoch
// ---------------------------------------------------------------------------
// The schedule of one firing edge: next_sample += eps; n_neg = int((n -
// next_neg) / epn); next_neg += n_neg * epn.  Contraction is off: every
// operation is rounded to fp32 on its own, as numpy rounds them, so an fma
// must not replace the multiply and the add.
__device__ __forceinline__ int umap_schedule(float nf, float eps, float epn, float& next_sample, float& next_neg) {
#pragma clang fp contract(off)
  next_sample = next_sample + eps;
  const float ahead = nf - next_neg;
  const float q = ahead / epn;
  int m = (int)q;
  m = m < 0 ? 0 : (m > MAX_NEG ? MAX_NEG : m);
  const float adv = (float)m * epn;
  next_neg = next_neg + adv;
  return m;
}

__device__ __forceinline__ double clip4(double v) { return fmin(fmax(v, -4.0), 4.0); }

// Positions and the schedule state are fp32; the forces and their sum are
// fp64.  The map is sensitive (a repulsion near contact has a slope in the
// hundreds per unit of distance), so a rounding error of fp32 forces grows
// about tenfold per epoch, and a hub's fp32 sum of a hundred clipped terms
// starts it off well above the rounding of the positions themselves.
__global__ __launch_bounds__(NT) void umap_epoch_kernel(int N, const int32_t* __restrict__ row_ptr,
                                                        const int32_t* __restrict__ col,
                                                        const float* __restrict__ eps, const float* __restrict__ epn,
                                                        float* __restrict__ next_sample,
                                                        float* __restrict__ next_neg, const float* __restrict__ y_in,
                                                        float* __restrict__ y_out, float a32, float b32, float gamma,
                                                        float alpha, int n, uint32_t seed) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
  if (i >= N) return;  // wave-uniform
  const double yix = (double)y_in[2 * (long)i], yiy = (double)y_in[2 * (long)i + 1];
  const int e0 = row_ptr[i], e1 = row_ptr[i + 1];
  const float nf = (float)n;
  const double a = (double)a32, b = (double)b32;
  const double attr_scale = -2.0 * a * b, rep_scale = 2.0 * (double)gamma * b;

  double fx = 0.0, fy = 0.0;
  for (int e = e0 + lane; e < e1; e += 64) {
    float ns = next_sample[e];
    if (!(ns <= nf)) continue;
    const int j = col[e];
    if ((unsigned)j >= (unsigned)N) continue;  // never read outside y_in
    {
      const double dx = yix - (double)y_in[2 * (long)j], dy = yiy - (double)y_in[2 * (long)j + 1];
      const double d2 = dx * dx + dy * dy;
      if (d2 > 0.0) {
        const double pb = pow(d2, b);
        const double c = attr_scale * (pb / d2) / (a * pb + 1.0);
        fx += 2.0 * clip4(c * dx);
        fy += 2.0 * clip4(c * dy);
      }
    }
    float nn = next_neg[e];
    const int n_neg = umap_schedule(nf, eps[e], epn[e], ns, nn);
    next_sample[e] = ns;
    next_neg[e] = nn;
    for (int p = 0; p < n_neg; ++p) {
      const int k = (int)(ssip_umap_hash(seed, (uint32_t)n, (uint32_t)e, (uint32_t)p) % (uint32_t)N);
      if (k == i) continue;
      const double dx = yix - (double)y_in[2 * (long)k], dy = yiy - (double)y_in[2 * (long)k + 1];
      const double d2 = dx * dx + dy * dy;
      if (d2 > 0.0) {
        const double pb = pow(d2, b);
        const double c = rep_scale / ((0.001 + d2) * (a * pb + 1.0));
        fx += clip4(c * dx);
        fy += clip4(c * dy);
      }
    }
  }
  fx = wave_sum_d(fx);
  fy = wave_sum_d(fy);
  if (lane == 0) {
    float2 o;
    o.x = (float)(yix + (double)alpha * fx);
    o.y = (float)(yiy + (double)alpha * fy);
    *reinterpret_cast<float2*>(y_out + 2 * (long)i) = o;
  }
}

}  // namespace

extern "C" {

int64_t ssip_umap_workspace_bytes(int64_t N) {
  SSIP_REQUIRE(N >= 2 && N <= UMAP_MAX_N, SSIP_ERR_ARG, "ssip_umap_workspace_bytes: N = %ld outside 2..%d", (long)N,
               UMAP_MAX_N);
  return umap_ws_bytes(N);
}

int ssip_umap_fuzzy(int N, int k, int ld, const float* d2, const int32_t* idx, float* rho, float* sigma, float* memb,
                    void* workspace, int64_t workspace_bytes, void* stream) {
  SSIP_REQUIRE(N >= 2 && N <= UMAP_MAX_N, SSIP_ERR_ARG, "ssip_umap_fuzzy: N = %d outside 2..%d", N, UMAP_MAX_N);
  SSIP_REQUIRE(k >= 2 && k <= KNN_MAX_K && k <= N, SSIP_ERR_ARG, "ssip_umap_fuzzy: k = %d outside 2..min(%d, N = %d)",
               k, KNN_MAX_K, N);
  SSIP_REQUIRE(ld >= k, SSIP_ERR_ARG, "ssip_umap_fuzzy: leading dimension %d below k = %d", ld, k);
  SSIP_REQUIRE(d2 && idx && rho && sigma && memb, SSIP_ERR_ARG, "ssip_umap_fuzzy: null pointer");
  if (int rc = check_workspace("ssip_umap_fuzzy", workspace, workspace_bytes, umap_ws_bytes(N))) return rc;
  const UmapWs ws = umap_ws(workspace, N);
  const dim3 grid((N + NT / 64 - 1) / (NT / 64));
  SSIP_KLAUNCH(umap_rowsum_kernel, grid, dim3(NT), 0, (hipStream_t)stream, N, k, ld, d2, ws.rowsum);
  SSIP_KLAUNCH(umap_total_kernel, dim3(1), dim3(FIN_NT), 0, (hipStream_t)stream, N, ws.rowsum, ws.total);
  SSIP_KLAUNCH(umap_fuzzy_kernel, grid, dim3(NT), 0, (hipStream_t)stream, N, k, ld, d2, idx, ws, rho, sigma, memb);
  return ssip::check_launch("ssip_umap_fuzzy");
}

int ssip_umap_epoch(int N, const int32_t* row_ptr, const int32_t* col, const float* eps, const float* epn,
                    float* next_sample, float* next_neg, const float* y_in, float* y_out, float a, float b,
                    float gamma, float alpha, int n, uint32_t seed, void* stream) {
  SSIP_REQUIRE(N >= 2 && N <= UMAP_MAX_N, SSIP_ERR_ARG, "ssip_umap_epoch: N = %d outside 2..%d", N, UMAP_MAX_N);
  SSIP_REQUIRE(row_ptr && col && eps && epn && next_sample && next_neg && y_in && y_out, SSIP_ERR_ARG,
               "ssip_umap_epoch: null pointer");
  SSIP_REQUIRE(y_in != y_out, SSIP_ERR_ARG, "ssip_umap_epoch: y_out must not alias y_in (epochs are Jacobi-ordered)");
  SSIP_REQUIRE(n >= 0 && n < (1 << 24), SSIP_ERR_ARG, "ssip_umap_epoch: epoch %d outside 0..2^24 - 1", n);
  SSIP_REQUIRE(a > 0.f && b > 0.f, SSIP_ERR_ARG, "ssip_umap_epoch: a = %g, b = %g must be > 0", (double)a, (double)b);
  SSIP_KLAUNCH(umap_epoch_kernel, dim3((N + NT / 64 - 1) / (NT / 64)), dim3(NT), 0, (hipStream_t)stream, N, row_ptr,
               col, eps, epn, next_sample, next_neg, y_in, y_out, a, b, gamma, alpha, n, seed);
  return ssip::check_launch("ssip_umap_epoch");
}

}  // extern "C"

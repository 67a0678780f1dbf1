// Exact t-SNE on the PCA space (reference src/clustering.py:251-276, which
// calls sklearn.manifold.TSNE): the joint probabilities P of the input points
// and, per iteration, the gradient of KL(P || Q) over all N^2 pairs plus
// sklearn's momentum / gains step.  The objective is the one
// sklearn.manifold._t_sne._kl_divergence evaluates (method="exact"); the
// Barnes-Hut method approximates it.
//
// Everything is fp32 unless said otherwise.  The only N^2 operand is P
// ([N][N] row-major, N <= TSNE_MAX_N = 32768: 4 GB); the 2-D embedding Y is
// [N][2].  No atomics; every reduction runs in a fixed order, so all outputs
// are bit-reproducible from run to run.
//
//   cond_p:  squared distances in layout A of analytics.hip (pairwise_tile.h,
//            direct difference, feature order) written into P, then one
//            workgroup per row runs sklearn's bisection on beta with the exp
//            and the entropy sums in fp64 (a row whose every exp(-d2) is zero
//            at beta = 1 halves its way down exactly as sklearn's does).
//   joint_p: 64 x 64 tile pairs (bi <= bj) symmetrise P in place, the
//            transposed tile read through LDS; the total is reduced per tile
//            pair, then over the tile pairs in fp64; a third pass divides.
//   grad:    layout A's thread mapping over P: a workgroup owns 32 rows (8 per
//            wave) and one of S column splits, lane = column, so every P read
//            is 256 contiguous bytes per row.  Six partial sums per (split, row).
//   update:  per-row sum of the partials in split order, Z and the KL sum in
//            fp64, then grad = 4 (exaggeration attr - rep / Z) and the step.
#include "ssip_common.h"
#include "pairwise_tile.h"

#include <math.h>

namespace {

constexpr int TSNE_MAX_N = 32768;  // 4 GB of P
constexpr int TSNE_MAX_SPLITS = 64;
constexpr int TT = 64;             // joint_p tile
constexpr int TT_LD = TT + 1;      // +1 pad: the transposed read walks a column
constexpr int RU = 256;            // reduce / apply: rows per workgroup (thread = row)
constexpr int FIN_NT = 256;        // finish: one workgroup
constexpr int BISECT_STEPS = 100;  // sklearn's n_steps
constexpr int GW = 8;              // grad: rows per wave
constexpr int RG = 4 * GW;         // grad: rows per workgroup
constexpr int NQ = 6;              // partial sums per row: attr x, y, rep x, y, z, kl

// column splits of the gradient pass: enough workgroups to fill the chip at
// small N, whole 64-column tiles per split.  A function of N alone.
struct Splits {
  int tiles_per_split, splits;
};
inline Splits grad_splits(int N) {
  const int ntile = (N + 63) / 64, rowblocks = (N + RG - 1) / RG;
  int want = (1024 + rowblocks - 1) / rowblocks;
  want = want < 1 ? 1 : (want > TSNE_MAX_SPLITS ? TSNE_MAX_SPLITS : want);
  if (want > ntile) want = ntile;
  Splits s;
  s.tiles_per_split = (ntile + want - 1) / want;
  s.splits = (ntile + s.tiles_per_split - 1) / s.tiles_per_split;
  return s;
}

// Workspace: fp64 scalars first, then the per-row arrays, then the region
// shared by the tile-pair sums of joint_p and the split partials of grad.
struct TsneWs {
  double* rowpart;   // [G][2]  per row block of RU: sum z, sum kl
  double* gradpart;  // [G][2]  per row block of RU: sum grad^2, sum (gains grad)^2
  double* sigma;     // [1]     joint_p: total of the symmetrised matrix
  float* red;        // [NQ][N] partials summed over the splits
  float* grad;       // [N][2]
  float* part;       // [S][NQ][N] (grad) / double [T][T] (joint_p)
};
inline long tsne_groups(long N) { return (N + RU - 1) / RU; }
inline long tsne_head_bytes(long N) { return ((4 * tsne_groups(N) + 1) * 8 + 15) / 16 * 16; }
inline long tsne_ws_bytes(long N) {
  const long T = (N + TT - 1) / TT;
  const long part = (long)grad_splits((int)N).splits * NQ * N * 4, tiles = T * T * 8;
  return tsne_head_bytes(N) + (NQ + 2) * N * 4 + 16 + (part > tiles ? part : tiles);
}
inline TsneWs tsne_ws(void* base, long N) {
  const long G = tsne_groups(N);
  char* p = static_cast<char*>(base);
  TsneWs ws;
  ws.rowpart = reinterpret_cast<double*>(p);
  ws.gradpart = ws.rowpart + 2 * G;
  ws.sigma = ws.gradpart + 2 * G;
  p += tsne_head_bytes(N);
  ws.red = reinterpret_cast<float*>(p);
  ws.grad = ws.red + NQ * N;
  ws.part = reinterpret_cast<float*>(p + ((NQ + 2) * N * 4 + 15) / 16 * 16);
  return ws;
}

// ---------------------------------------------------------------------------
// conditional P
// ---------------------------------------------------------------------------
// P[i][j] = |x_i - x_j|^2
__global__ __launch_bounds__(NT) void tsne_d2_kernel(int N, int d, const float* __restrict__ X, float* __restrict__ P) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int row0 = blockIdx.x * RA;
  walk_columns_a(N, d, X, row0, [&](int jt, const float(&acc)[16]) {
    const int j = jt * 64 + lane;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int i = row0 + w * 16 + u;
      if (i < N && j < N) P[(long)i * N + j] = acc[u];
    }
  });
}

// One workgroup per row: sklearn's _binary_search_perplexity over the row of
// squared distances held in P, which the row of p(j|i) then replaces.
__global__ __launch_bounds__(NT) void tsne_bisect_kernel(int N, double log_perplexity, float* __restrict__ P,
                                                         double* __restrict__ beta_out) {
  __shared__ double slot[2][2][NT / 64];
  const int tid = threadIdx.x;
  const int i = blockIdx.x;
  float* row = P + (long)i * N;
  const double tiny = (double)1e-8f, tol = (double)1e-5f;  // sklearn keeps both as C floats

  double beta = 1.0, beta_min = -INFINITY, beta_max = INFINITY;
  double beta_used = 1.0, sum_used = 1.0;
  for (int l = 0; l < BISECT_STEPS; ++l) {
    double s0 = 0.0, s1 = 0.0;
    for (int j = tid; j < N; j += NT) {
      if (j == i) continue;
      const double dd = (double)row[j];
      const double e = exp(-dd * beta);
      s0 += e;
      s1 += dd * e;
    }
    // two barriers per step; the slots alternate so a step never overwrites
    // what a slower wave still reads
    s0 = block_sum_d(s0, slot[l & 1][0], tid);
    s1 = block_sum_d(s1, slot[l & 1][1], tid);
    if (s0 == 0.0) s0 = tiny;
    beta_used = beta;
    sum_used = s0;
    const double diff = log(s0) + beta * (s1 / s0) - log_perplexity;
    if (fabs(diff) <= tol) break;
    if (diff > 0.0) {
      beta_min = beta;
      beta = beta_max == INFINITY ? beta * 2.0 : (beta + beta_max) / 2.0;
    } else {
      beta_max = beta;
      beta = beta_min == -INFINITY ? beta / 2.0 : (beta + beta_min) / 2.0;
    }
  }
  for (int j = tid; j < N; j += NT) row[j] = j == i ? 0.f : (float)(exp(-(double)row[j] * beta_used) / sum_used);
  if (tid == 0) beta_out[i] = beta_used;
}

// ---------------------------------------------------------------------------
// joint P
// ---------------------------------------------------------------------------
// Tile pair (bi, bj), bi <= bj: both tiles become p(j|i) + p(i|j); the sum is
// formed once per pair of entries and stored to both, so the matrix is
// symmetric bit for bit.  tilesum[bi][bj] = the pair's share of the total.
__global__ __launch_bounds__(NT) void tsne_symmetrise_kernel(int N, float* __restrict__ P, double* __restrict__ tilesum) {
  __shared__ float a[TT * TT_LD];
  __shared__ float b[TT * TT_LD];
  __shared__ double slot[NT / 64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int bi = blockIdx.y, bj = blockIdx.x, T = gridDim.x;
  if (bj < bi) {
    if (tid == 0) tilesum[(long)bi * T + bj] = 0.0;
    return;
  }
  const bool diag = bi == bj;
  // a[r][c] = P[bi*64 + r][bj*64 + c], b[r][c] = P[bj*64 + r][bi*64 + c]; lane = c
  for (int r = w; r < TT; r += NT / 64) {
    const int ia = bi * TT + r, ja = bj * TT + lane;
    a[r * TT_LD + lane] = (ia < N && ja < N) ? P[(long)ia * N + ja] : 0.f;
    if (!diag) {
      const int ib = bj * TT + r, jb = bi * TT + lane;
      b[r * TT_LD + lane] = (ib < N && jb < N) ? P[(long)ib * N + jb] : 0.f;
    }
  }
  __syncthreads();
  const float* t = diag ? a : b;
  float acc = 0.f;
  for (int r = w; r < TT; r += NT / 64) {
    const int ia = bi * TT + r, ja = bj * TT + lane;
    // IEEE addition commutes, so on the diagonal tile entry (r, c) and entry
    // (c, r) get the same bits
    const float s = a[r * TT_LD + lane] + t[lane * TT_LD + r];
    if (ia < N && ja < N) {
      P[(long)ia * N + ja] = s;
      acc += s;
    }
    if (!diag) {
      const int ib = bj * TT + r, jb = bi * TT + lane;
      const float s2 = a[lane * TT_LD + r] + b[r * TT_LD + lane];  // = entry (lane, r) of the pair above
      if (ib < N && jb < N) {
        P[(long)ib * N + jb] = s2;
        acc += s2;
      }
    }
  }
  const double total = block_sum_d((double)acc, slot, tid);
  if (tid == 0) tilesum[(long)bi * T + bj] = total;
}

// One workgroup: sigma = sum of the T * T tile sums in index order (fp64)
__global__ __launch_bounds__(FIN_NT) void tsne_sigma_kernel(long count, const double* __restrict__ tilesum,
                                                            double* __restrict__ sigma) {
  __shared__ double slot[FIN_NT / 64];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (long q = tid; q < count; q += FIN_NT) s += tilesum[q];
  s = block_sum_d(s, slot, tid);
  if (tid == 0) *sigma = s;
}

__global__ __launch_bounds__(NT) void tsne_normalise_kernel(long count, float* __restrict__ P,
                                                            const double* __restrict__ sigma) {
  const double s = *sigma > 0.0 ? *sigma : 1.0;
  const long base = (long)blockIdx.x * (NT * 8) + threadIdx.x;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const long idx = base + q * NT;
    if (idx < count) P[idx] = (float)((double)P[idx] / s);
  }
}

// ---------------------------------------------------------------------------
// gradient
// ---------------------------------------------------------------------------
// Workgroup (x = row block of RG = 32, GW = 8 rows per wave, y = column split).  part[s][q][i] for the six
// sums of row i over the split's columns: lanes stride the columns, then a
// wave butterfly.
template <bool ERR>
__global__ __launch_bounds__(NT) void tsne_grad_kernel(int N, int tiles_per_split, const float* __restrict__ P,
                                                       const float* __restrict__ Y, float* __restrict__ part) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int rowbase = blockIdx.x * RG + w * GW;
  const int ntile = (N + 63) / 64;
  const int t0 = blockIdx.y * tiles_per_split;
  const int t1 = min(ntile, t0 + tiles_per_split);

  float yix[GW], yiy[GW];
#pragma unroll
  for (int u = 0; u < GW; ++u) {
    const int i = min(rowbase + u, N - 1);  // rows past N are computed on a copy of the last row and not stored
    yix[u] = Y[2 * (long)i];
    yiy[u] = Y[2 * (long)i + 1];
  }
  float ax[GW], ay[GW], rx[GW], ry[GW], zz[GW], kl[GW];
#pragma unroll
  for (int u = 0; u < GW; ++u) ax[u] = ay[u] = rx[u] = ry[u] = zz[u] = kl[u] = 0.f;

  for (int t = t0; t < t1; ++t) {
    const int j = t * 64 + lane;
    const bool jin = j < N;
    float yjx = 0.f, yjy = 0.f;
    if (jin) {
      yjx = Y[2 * (long)j];
      yjy = Y[2 * (long)j + 1];
    }
    float p[GW];
#pragma unroll
    for (int u = 0; u < GW; ++u) {
      const int i = rowbase + u;
      p[u] = (jin && i < N) ? P[(long)i * N + j] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < GW; ++u) {
      const int i = rowbase + u;
      const bool pair = jin && j != i;
      const float dx = yix[u] - yjx, dy = yiy[u] - yjy;
      const float q = fmaf(dy, dy, fmaf(dx, dx, 1.f));
      const float wgt = pair ? 1.f / q : 0.f;
      const float pw = p[u] * wgt, w2 = wgt * wgt;
      ax[u] = fmaf(pw, dx, ax[u]);
      ay[u] = fmaf(pw, dy, ay[u]);
      rx[u] = fmaf(w2, dx, rx[u]);
      ry[u] = fmaf(w2, dy, ry[u]);
      zz[u] += wgt;
      // sum P log P - sum P log w = sum P (log P + log(1 + |y_i - y_j|^2))
      if (ERR) kl[u] += (pair && p[u] > 0.f) ? p[u] * (logf(p[u]) + logf(q)) : 0.f;
    }
  }
  const long s = blockIdx.y;
#pragma unroll
  for (int u = 0; u < GW; ++u) {
    const float v0 = wave_sum(ax[u]), v1 = wave_sum(ay[u]), v2 = wave_sum(rx[u]), v3 = wave_sum(ry[u]);
    const float v4 = wave_sum(zz[u]), v5 = ERR ? wave_sum(kl[u]) : 0.f;
    const int i = rowbase + u;
    if (lane == u && i < N) {
      float* o = part + s * NQ * N + i;
      o[0] = v0;
      o[(long)N] = v1;
      o[2L * N] = v2;
      o[3L * N] = v3;
      o[4L * N] = v4;
      o[5L * N] = v5;
    }
  }
}

// ---------------------------------------------------------------------------
// update
// ---------------------------------------------------------------------------
// thread = row: red[q][i] = sum over the splits, in split order; per workgroup
// the fp64 sums of z and kl over its rows
__global__ __launch_bounds__(RU) void tsne_reduce_kernel(int N, int S, TsneWs ws) {
  __shared__ double slot[2][RU / 64];
  const int tid = threadIdx.x;
  const int i = blockIdx.x * RU + tid;
  float v[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) v[q] = 0.f;
  if (i < N) {
    for (int s = 0; s < S; ++s) {
#pragma unroll
      for (int q = 0; q < NQ; ++q) v[q] += ws.part[((long)s * NQ + q) * N + i];
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) ws.red[(long)q * N + i] = v[q];
  }
  const double z = block_sum_d((double)v[4], slot[0], tid);
  const double k = block_sum_d((double)v[5], slot[1], tid);
  if (tid == 0) {
    ws.rowpart[2 * blockIdx.x] = z;
    ws.rowpart[2 * blockIdx.x + 1] = k;
  }
}

// sklearn's _gradient_descent step on one coordinate; returns gains * grad.
// Contraction is off: every product and sum is rounded to fp32 on its own, as
// numpy rounds them, so an fma must not replace a multiply and an add.
__device__ __forceinline__ float sklearn_step(float grad, float momentum, float learning_rate, float& update,
                                              float& gain, float& y) {
#pragma clang fp contract(off)
  const float prod = update * grad;
  gain = prod < 0.f ? gain + 0.2f : gain * 0.8f;
  gain = fmaxf(gain, 0.01f);
  const float sg = grad * gain;
  const float keep = momentum * update;
  const float move = learning_rate * sg;
  update = keep - move;
  y = y + update;
  return sg;
}

// thread = row.  Every workgroup sums the G row-block values of z in index
// order (fp64), so all of them hold the same Z.  The step is sklearn's
// _gradient_descent, each operation rounded to fp32 on its own (no
// contraction) so that it equals the numpy expression in float32 bit for bit.
__global__ __launch_bounds__(RU) void tsne_apply_kernel(int N, int G, float exaggeration, float momentum,
                                                        float learning_rate, TsneWs ws, float* __restrict__ Y,
                                                        float* __restrict__ update, float* __restrict__ gains) {
  __shared__ double slot[2][RU / 64];
  const int tid = threadIdx.x;
  const int i = blockIdx.x * RU + tid;
  double Z = 0.0;
  for (int g = 0; g < G; ++g) Z += ws.rowpart[2 * g];
  double g2 = 0.0, gg2 = 0.0;
  if (i < N) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const double attr = (double)ws.red[(long)c * N + i], rep = (double)ws.red[(long)(2 + c) * N + i];
      const float grad = (float)(4.0 * ((double)exaggeration * attr - rep / Z));
      ws.grad[2 * (long)i + c] = grad;
      float u = update[2 * (long)i + c], gn = gains[2 * (long)i + c], y = Y[2 * (long)i + c];
      const float sg = sklearn_step(grad, momentum, learning_rate, u, gn, y);
      gains[2 * (long)i + c] = gn;
      update[2 * (long)i + c] = u;
      Y[2 * (long)i + c] = y;
      g2 += (double)grad * (double)grad;
      gg2 += (double)sg * (double)sg;
    }
  }
  g2 = block_sum_d(g2, slot[0], tid);
  gg2 = block_sum_d(gg2, slot[1], tid);
  if (tid == 0) {
    ws.gradpart[2 * blockIdx.x] = g2;
    ws.gradpart[2 * blockIdx.x + 1] = gg2;
  }
}

// One workgroup: scalars = {Z, KL, |grad|, |gains * grad|}
__global__ __launch_bounds__(FIN_NT) void tsne_finish_kernel(int G, TsneWs ws, double* __restrict__ scalars) {
  __shared__ double v[4];
  const int tid = threadIdx.x;
  // G <= 128 row blocks: thread q sums quantity q in index order, so Z here is
  // the Z tsne_apply_kernel divided by
  if (tid < 4) {
    const double* src = tid < 2 ? ws.rowpart + tid : ws.gradpart + (tid - 2);
    double s = 0.0;
    for (int g = 0; g < G; ++g) s += src[2 * g];
    v[tid] = s;
  }
  __syncthreads();
  if (tid == 0) {
    scalars[0] = v[0];
    scalars[1] = v[1] + log(v[0]);
    scalars[2] = sqrt(v[2]);
    scalars[3] = sqrt(v[3]);
  }
}

int check_tsne(const char* what, long N, const void* workspace, long workspace_bytes) {
  SSIP_REQUIRE(N >= 2 && N <= TSNE_MAX_N, SSIP_ERR_ARG, "%s: N = %ld outside 2..%d (P is N^2 floats)", what, N,
               TSNE_MAX_N);
  return check_workspace(what, workspace, workspace_bytes, tsne_ws_bytes(N));
}

}  // namespace

extern "C" {

int64_t ssip_tsne_workspace_bytes(int64_t N) {
  SSIP_REQUIRE(N >= 2 && N <= TSNE_MAX_N, SSIP_ERR_ARG, "ssip_tsne_workspace_bytes: N = %ld outside 2..%d", (long)N,
               TSNE_MAX_N);
  return tsne_ws_bytes(N);
}

int ssip_tsne_cond_p(int N, int d, const float* X, float perplexity, float* P, double* beta, void* stream) {
  SSIP_REQUIRE(N >= 2 && N <= TSNE_MAX_N, SSIP_ERR_ARG, "ssip_tsne_cond_p: N = %d outside 2..%d", N, TSNE_MAX_N);
  if (int rc = check_points("ssip_tsne_cond_p", N, d, X)) return rc;
  SSIP_REQUIRE(perplexity > 0.f, SSIP_ERR_ARG, "ssip_tsne_cond_p: perplexity = %g must be > 0", (double)perplexity);
  SSIP_REQUIRE(P && beta, SSIP_ERR_ARG, "ssip_tsne_cond_p: null pointer");
  SSIP_KLAUNCH(tsne_d2_kernel, dim3((N + RA - 1) / RA), dim3(NT), 0, (hipStream_t)stream, N, d, X, P);
  SSIP_KLAUNCH(tsne_bisect_kernel, dim3(N), dim3(NT), 0, (hipStream_t)stream, N, log((double)perplexity), P, beta);
  return ssip::check_launch("ssip_tsne_cond_p");
}

int ssip_tsne_joint_p(int N, float* P, void* workspace, int64_t workspace_bytes, void* stream) {
  if (int rc = check_tsne("ssip_tsne_joint_p", N, workspace, workspace_bytes)) return rc;
  SSIP_REQUIRE(P != nullptr, SSIP_ERR_ARG, "ssip_tsne_joint_p: null pointer");
  const TsneWs ws = tsne_ws(workspace, N);
  const int T = (N + TT - 1) / TT;
  double* tilesum = reinterpret_cast<double*>(ws.part);
  const long count = (long)N * N;
  SSIP_KLAUNCH(tsne_symmetrise_kernel, dim3(T, T), dim3(NT), 0, (hipStream_t)stream, N, P, tilesum);
  SSIP_KLAUNCH(tsne_sigma_kernel, dim3(1), dim3(FIN_NT), 0, (hipStream_t)stream, (long)T * T, tilesum, ws.sigma);
  SSIP_KLAUNCH(tsne_normalise_kernel, dim3((unsigned)((count + NT * 8 - 1) / (NT * 8))), dim3(NT), 0,
               (hipStream_t)stream, count, P, ws.sigma);
  return ssip::check_launch("ssip_tsne_joint_p");
}

int ssip_tsne_grad(int N, const float* P, const float* Y, int compute_error, void* workspace, int64_t workspace_bytes,
                   void* stream) {
  if (int rc = check_tsne("ssip_tsne_grad", N, workspace, workspace_bytes)) return rc;
  SSIP_REQUIRE(P && Y, SSIP_ERR_ARG, "ssip_tsne_grad: null pointer");
  const TsneWs ws = tsne_ws(workspace, N);
  const Splits sp = grad_splits(N);
  const dim3 grid((N + RG - 1) / RG, sp.splits);
  if (compute_error)
    SSIP_KLAUNCH(tsne_grad_kernel<true>, grid, dim3(NT), 0, (hipStream_t)stream, N, sp.tiles_per_split, P, Y, ws.part);
  else
    SSIP_KLAUNCH(tsne_grad_kernel<false>, grid, dim3(NT), 0, (hipStream_t)stream, N, sp.tiles_per_split, P, Y,
                 ws.part);
  return ssip::check_launch("ssip_tsne_grad");
}

int ssip_tsne_update(int N, void* workspace, int64_t workspace_bytes, float* Y, float* update, float* gains,
                     float exaggeration, float momentum, float learning_rate, double* scalars, void* stream) {
  if (int rc = check_tsne("ssip_tsne_update", N, workspace, workspace_bytes)) return rc;
  SSIP_REQUIRE(Y && update && gains && scalars, SSIP_ERR_ARG, "ssip_tsne_update: null pointer");
  const TsneWs ws = tsne_ws(workspace, N);
  const int G = (int)tsne_groups(N);
  SSIP_KLAUNCH(tsne_reduce_kernel, dim3(G), dim3(RU), 0, (hipStream_t)stream, N, grad_splits(N).splits, ws);
  SSIP_KLAUNCH(tsne_apply_kernel, dim3(G), dim3(RU), 0, (hipStream_t)stream, N, G, exaggeration, momentum,
               learning_rate, ws, Y, update, gains);
  SSIP_KLAUNCH(tsne_finish_kernel, dim3(1), dim3(FIN_NT), 0, (hipStream_t)stream, G, ws, scalars);
  return ssip::check_launch("ssip_tsne_update");
}

}  // extern "C"

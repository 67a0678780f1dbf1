#pragma once
#include "conv_tile.h"

namespace {

// ---------------------------------------------------------------------------
// The stem conv (7x7 / stride 2 over the pre-padded 4-channel image, pad 0,
// S padded to 8) in the same persistent, LDS-resident form.  A tile is
// STEM_TR = 2 output rows; their 9 input rows (2 p0 .. 2 p0 + 8) are one
// contiguous run of the NHWC4 image, DMA'd linearly into a double buffer.
// Output pixel (j, q), filter row r reads the 8 pixels 2q .. 2q+7 of input
// row 2j + r: 64 contiguous bytes = one 32-deep MFMA k-step (s = 7 carries a
// zero weight), so a tile is 7 k-steps with no barrier.  GEMM rows are the
// output rows padded to STEM_QP = 128 (q >= Q discarded).  The weight panel
// (64 filters x 7 rows x 32) stays resident.  Epilogue as conv_halo_kernel:
// 16-bit stores from the accumulators, per-wave BN records [K][G][4][3].
// The k-order differs from conv_glds_kernel's C4 path (which pairs two filter
// rows per 64-deep step), so outputs agree to fp32 rounding, not bitwise.
// ---------------------------------------------------------------------------
struct StemArgs {
  const __bf16* X;    // [N][H][W][4]   pre-padded image
  const __bf16* Wt;   // [Ncols][7][8][4]
  __bf16* out;        // [N][P][Q][Ncols]
  float* partial;     // BN records (nullable)
  uint32_t x_bytes, w_bytes, o_bytes;
  int N, H, W, P, Q, Ncols, tiles, units;
};

constexpr int STEM_QP = 128, STEM_TR = 2, STEM_XROWS = 2 * STEM_TR + 5;
constexpr int STEM_XBUF = 17 * 1024;  // 9 rows x W x 8 B, W <= 240

// The STEM_XROWS input rows of the tile at output row p0 of image n (one
// contiguous run of the NHWC4 image) DMA'd linearly into Xs, 1-KiB pieces
// dealt to NWV waves.  FIXED: every wave issues ceil(STEM_XBUF / NWV KiB)
// pieces whatever W is -- past the buffer its previous one again (same bytes
// to the same place) -- so a counted vmcnt can retire them; a tile that is
// not `live` issues zero-fill.
template <int NWV, bool FIXED>
__device__ __forceinline__ void stem_issue_x(__amdgpu_buffer_rsrc_t rsX, int n, int p0, int H, int W, bool live,
                                             int wave, int lane, char* Xs) {
  const int xrun = STEM_XROWS * (W * 8);  // bytes of a tile's input rows
  const uint32_t base = (uint32_t)((((long)n * H + 2 * p0) * W) * 8);
  auto piece = [&](int i) {
    const int b = i * 1024 + lane * 16;
    blds16(rsX, live && b < xrun ? base + (uint32_t)b : SSIP_OOB, Xs + i * 1024);
  };
  if constexpr (FIXED) {
#pragma unroll
    for (int k = 0; k < (STEM_XBUF / 1024 + NWV - 1) / NWV; ++k)
      piece(wave + NWV * k - (wave + NWV * k < STEM_XBUF / 1024 ? 0 : NWV));
  } else {
    const int nxi = (xrun + 1023) >> 10;  // 1-KiB DMA wave-instructions
    for (int i = wave; i < nxi; i += NWV) piece(i);
  }
}

template <int WMW, int WNW>
__global__ void __launch_bounds__(64 * WMW * WNW, (WMW * WNW) / 2) conv_stem_halo_kernel(const StemArgs a) {
  typedef __bf16 T;
  constexpr int NW = WMW * WNW, NT = 64 * NW;
  constexpr int BM = STEM_TR * STEM_QP, BN = 64;
  constexpr int WTM = BM / WMW, WTN = BN / WNW, FM = WTM / 16, FN = WTN / 16;
  constexpr int B_BYTES = 7 * BN * 64;  // [r][col][32 k], 16-B slot s at s ^ 2((col >> 3) & 1)
  static_assert(FM >= 1 && FN >= 1, "bad stem wave tile");
  __shared__ __attribute__((aligned(16))) char smem[B_BYTES + 2 * STEM_XBUF];
  char* const Bs = smem;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WNW, wn = wave % WNW;
  const int G = gridDim.x, g = blockIdx.x;
  const int u0 = (int)((long)g * a.units / G), u1 = (int)((long)(g + 1) * a.units / G);
  const __amdgpu_buffer_rsrc_t rsX = make_rsrc(a.X, a.x_bytes), rsW = make_rsrc(a.Wt, a.w_bytes);
  const __amdgpu_buffer_rsrc_t rsO = make_rsrc(a.out, a.o_bytes);
  const int xpitch = a.W * 8;                  // one input row (4 channels bf16)

  auto issue_x = [&](int tile, char* Xs) {
    const auto [n, p0] = tile_row(tile, STEM_TR, a.P);
    stem_issue_x<NW, false>(rsX, n, p0, a.H, a.W, true, wave, lane, Xs);
  };
  auto issue_w = [&](int jn) {
    // 7 x 64 x 64 B = 28 KiB: instruction i covers rows r = i / 4, cols 16 (i % 4) .. +16
    for (int i = wave; i < 28; i += NW) {
      const int r = i >> 2, col = ((i & 3) << 4) + (lane >> 2);
      const int sl = (lane & 3) ^ (((col >> 3) & 1) << 1);
      const uint32_t off = (uint32_t)(((((long)jn * 64 + col) * 7 + r) * 32 + sl * 8) * 2);
      blds16(rsW, off, Bs + i * 1024);
    }
  };

  const int kq = lane >> 4;
  const int rbase = wm * WTM + kq * 4, cbase = wn * WTN + (lane & 15);
  // A fragment bases: GEMM row m = j * QP + q reads input row 2j + r, pixel 2q + 2kq
  int abase[FM];
#pragma unroll
  for (int i = 0; i < FM; ++i) {
    const int m = wm * WTM + i * 16 + (lane & 15);
    const int j = m / STEM_QP, q = m - j * STEM_QP;
    abase[i] = q < a.Q ? 2 * j * xpitch + (2 * q + 2 * kq) * 8 : 0;
  }
  int boff[FN];
#pragma unroll
  for (int jj = 0; jj < FN; ++jj) {
    const int col = wn * WTN + jj * 16 + (lane & 15);
    boff[jj] = col * 64 + ((kq ^ (((col >> 3) & 1) << 1)) << 4);
  }
  uint32_t rowoff[FM][4];
  const uint32_t vmask = lane_out_rows(rowoff, rbase, cbase, STEM_QP, BM, a.Q, a.Ncols);
  const int wrows = count_out_rows(wm * WTM, WTM, STEM_QP, BM, a.Q);

  if (a.partial) bn_records_zero<3>(a.partial, a.Ncols, G, g, tid, NT);
  WaveStats<FM, FN> ws;
  ws.reset();

  if (u0 < u1) {
    const int jn = u0 / a.tiles;
    issue_w(jn);
    issue_x(u0 - jn * a.tiles, smem + B_BYTES);
  }
  bool first = true;
  for (int u = u0; u < u1; ++u) {
    const int jn = u / a.tiles, tile = u - jn * a.tiles;
    char* const Xs = smem + B_BYTES + ((u - u0) & 1) * STEM_XBUF;
    char* const Xn = smem + B_BYTES + ((u - u0 + 1) & 1) * STEM_XBUF;
    if (first) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    first = false;
    halo_lds_barrier();
    const int un = u + 1;
    const bool more = un < u1;
    const int jn_next = more ? un / a.tiles : jn;
    const bool prefetch = more && jn_next == jn;
    if (prefetch) issue_x(un - jn * a.tiles, Xn);

    f32x4 acc[FM][FN];
    zero_acc(acc);
    Frag<T> fa[2][FM], fb[2][FN];
    auto load_step = [&](int r, Frag<T>(&ra)[FM], Frag<T>(&rb)[FN]) {
#pragma unroll
      for (int i = 0; i < FM; ++i) ra[i].v = *reinterpret_cast<const bf16x8*>(Xs + abase[i] + r * xpitch);
#pragma unroll
      for (int jj = 0; jj < FN; ++jj)
        rb[jj].v = *reinterpret_cast<const bf16x8*>(Bs + r * (BN * 64) + boff[jj]);
    };
    load_step(0, fa[0], fb[0]);
#pragma unroll
    for (int r = 0; r < 7; ++r) {
      if (r + 1 < 7) load_step(r + 1, fa[(r + 1) & 1], fb[(r + 1) & 1]);
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int jj = 0; jj < FN; ++jj) mma(acc[i][jj], fa[r & 1][i], fb[r & 1][jj]);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    if (a.partial && wrows > 0) {
      // per-lane shifted sums over the fp32 accumulators of the valid rows;
      // merged across the wave (and written) when the panel or range ends
      ws.tile(acc, vmask);
      if (!prefetch) ws.flush(a.partial, jn * BN + cbase, G, g, wm, lane);
    }
    const uint32_t obase = (uint32_t)(((long)tile * STEM_TR * a.Q * a.Ncols + jn * BN) * 2);
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int jj = 0; jj < FN; ++jj)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(short, from_f32<T>(acc[i][jj][e])), rsO,
                                                obase + rowoff[i][e] + jj * 32, 0, 0);
    if (more && !prefetch) {
      halo_lds_barrier();
      issue_w(jn_next);
      issue_x(un - jn_next * a.tiles, Xn);
      first = true;
    }
  }
}

// ---------------------------------------------------------------------------
// WGRAD of the stem conv (7x7 / stride 2 over the pre-padded NHWC4 image):
//   dW[k][(r, s, c)] = sum_m dy[m][k] * x[2p + r][2q + s][c]
// Per tile of STEM_TR output rows (GEMM rows m = j * QP + q, dy zero for
// q >= Q) a persistent workgroup stages the 9 contiguous input rows (as
// conv_stem_halo_kernel) and the tile's dy rows (m-major MTile image), both
// double-buffered, and keeps the 64 x 224 fp32 result in registers across
// its tiles.  The x operand of column block (r, 16 of the 32 (s, c)) for
// row m is the 64-B run at input row 2j + r, pixel 2q: transposed fragment
// reads with per-lane row addresses (overlapping runs).  One fp32 slab per
// workgroup, summed by wgrad_reduce_kernel.
// ---------------------------------------------------------------------------
struct StemWgArgs {
  const __bf16* X;   // [N][H][W][4]
  const __bf16* DY;  // [N][P][Q][64]
  float* slab;       // [G][64][224]
  uint32_t x_bytes, dy_bytes;
  int N, H, W, P, Q, tiles;
};

constexpr int SWG_DBUF = 32 * 1024;  // 256 dy rows x 128 B

__global__ void __launch_bounds__(512, 2) conv_stem_wgrad_kernel(const StemWgArgs a) {
  typedef __bf16 T;
  constexpr int NW = 8, NB = 14;  // 224 / 16 column blocks
  __shared__ __attribute__((aligned(16))) char smem[2 * (STEM_XBUF + SWG_DBUF)];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;  // k rows 32 wm .. +31; column blocks wn, wn + 4, ...
  const int G = gridDim.x, g = blockIdx.x;
  const int u0 = (int)((long)g * a.tiles / G), u1 = (int)((long)(g + 1) * a.tiles / G);
  const __amdgpu_buffer_rsrc_t rsX = make_rsrc(a.X, a.x_bytes), rsD = make_rsrc(a.DY, a.dy_bytes);
  const int xpitch = a.W * 8;

  auto issue = [&](int tile, char* Xs, char* Ds) {
    const auto [n, p0] = tile_row(tile, STEM_TR, a.P);
    stem_issue_x<NW, false>(rsX, n, p0, a.H, a.W, true, wave, lane, Xs);
    for (int i = wave; i < SWG_DBUF / 1024; i += NW) {
      const int m = i * 8 + (lane >> 3);
      const int j = m / STEM_QP, q = m - j * STEM_QP;
      const int ch = (lane & 7) ^ mt64_chunk_xor(m);  // MTile<64> swizzle
      const bool ok = q < a.Q;
      const uint32_t off = (uint32_t)(((((long)n * a.P + p0 + j) * a.Q + q) * 64 + ch * 8) * 2);
      blds16(rsD, ok ? off : SSIP_OOB, Ds + i * 1024);
    }
  };

  const int nbw = wn < NB - 12 ? 4 : 3;  // column blocks of this wave: wn + 4 b, b < nbw
  f32x4 acc[2][4];
  zero_acc(acc);
  // x fragment addressing: lane (g, q, p) reads rows m = row0 + 8 g + q (+4),
  // columns 4p .. 4p+3 of its block; row m's run starts at (2j + r) xpitch + 16 q_m
  const int lg = lane >> 4, lq = (lane & 15) >> 2, lp = lane & 3;

  if (u0 < u1) issue(u0, smem, smem + STEM_XBUF);
  bool first = true;
  for (int u = u0; u < u1; ++u) {
    char* const Xs = smem + ((u - u0) & 1) * (STEM_XBUF + SWG_DBUF);
    char* const Ds = Xs + STEM_XBUF;
    char* const Xn = smem + ((u - u0 + 1) & 1) * (STEM_XBUF + SWG_DBUF);
    if (first) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    first = false;
    halo_lds_barrier();
    if (u + 1 < u1) issue(u + 1, Xn, Xn + STEM_XBUF);
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      Frag<T> fa[2], fb[4];
#pragma unroll
      for (int x = 0; x < 2; ++x) read_tfrag(fa[x], Ds, 32 * ks, (2 * wm + x) * 16, lane);
      // the lane's two rows (lo: +0, hi: +4) of this k-step
      const int m_lo = 32 * ks + 8 * lg + lq, m_hi = m_lo + 4;
      const int jl = m_lo / STEM_QP, ql = m_lo - jl * STEM_QP;
      const int jh = m_hi / STEM_QP, qh = m_hi - jh * STEM_QP;
      const int base_lo = 2 * jl * xpitch + (ql < a.Q ? ql : 0) * 16;  // rows past Q meet dy = 0
      const int base_hi = 2 * jh * xpitch + (qh < a.Q ? qh : 0) * 16;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        if (b < nbw) {
          const int nb = wn + 4 * b, r = nb >> 1, cofs = ((nb & 1) * 16 + 4 * lp) * 2;
          read_tfrag_at(fb[b], Xs + base_lo + r * xpitch + cofs, Xs + base_hi + r * xpitch + cofs);
        }
      }
#pragma unroll
      for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int b = 0; b < 4; ++b)
          if (b < nbw) mma(acc[x][b], fa[x], fb[b]);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  float* sl = a.slab + (long)g * 64 * 224;
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int b = 0; b < 4; ++b)
      if (b < nbw) store_slab_frag(sl, 224, (2 * wm + x) * 16, (wn + 4 * b) * 16, acc[x][b], lane);
}

// ---------------------------------------------------------------------------
// Stem backward tail fused: the BN(+ReLU, through the 3x3/2/1 max-pool)
// backward apply pass and the stem wgrad in one persistent kernel, so the
// full-resolution dy never goes through HBM.  Per tile of 2 conv-output
// rows (h0 = 2T, 2T+1) a workgroup DMAs (double-buffered) the 9 input rows,
// the 2 pre-BN rows y, and pooled rows T, T+1 of dpool and the argmax bytes;
// then forms dy = A*d + B*y + C in LDS (d = the argmax-gathered pooled
// gradient masked by relu(fma(y, scale, shift)) > 0, exactly as
// stem_pool_bn_bwd_apply_kernel) as an m-major MTile image over the 224
// output pixels, and runs conv_stem_wgrad_kernel's MFMA loop on it.
// ---------------------------------------------------------------------------
struct StemBwArgs {
  const __bf16* X;      // [N][H][W][4]   pre-padded image
  const __bf16* Y;      // [N][P][Q][64]  pre-BN stem conv output
  const __bf16* DP;     // [N][P2][Q2][64] pooled gradient
  const uint8_t* IX;    // [N][P2][Q2][64] argmax bytes
  const float* scale;   // BN affine (ReLU mask)
  const float* shift;
  const float* coef;    // [3][64] from the BN-backward finalize
  float* slab;          // [G][64][224]
  uint32_t x_bytes, y_bytes, dp_bytes, ix_bytes;
  int N, H, W, P, Q, P2, Q2, tiles;
};

constexpr int SBW_Y = 28 * 1024, SBW_DP = 14 * 1024, SBW_IX = 7 * 1024;
constexpr int SBW_IN = STEM_XBUF + SBW_Y + SBW_DP + SBW_IX;  // one input buffer (66 KiB)

// The two halves of the work are specialised (tools/time_stem_bw.py on
// round 2's form, where every wave ran both behind a barrier -- r3-variants
// branch: DMA + sync alone 133 us, the dy pass +72, the MFMAs +74, and the
// two did not overlap): waves 0-7 form dy (two per SIMD,
// 4 channels x one 2x2 block per thread), waves 8-11 multiply (one per SIMD,
// all 64 k x 3-4 column blocks).  A tile's 224 GEMM rows are cut into half A (output columns
// 0-63 of both rows: 128 rows, 4 k-steps) and half B (columns 64-111: 96
// rows, 3 k-steps), GEMM row = 16 columns x 2 rows per 32-row chunk (the
// 2x2 pixel blocks of 8 pooled windows).  Phase (u, A): the dy waves form
// (u, B) while the MFMA waves run (u, A); phase (u, B): the dy waves form
// (u+1, A) while the MFMA waves run (u, B); one barrier per phase, each half
// in its own slot, so on every SIMD one wave's VALU work runs beside its
// partner's MFMAs.  The input regions are refilled as soon as their last
// reader is done, two phases ahead of their next reader: x of tile u+1 at
// (u, A) (x of u-1 was last read at (u-1, B)); y, the pooled gradient and
// the argmax of tile u+2 at (u, B) (those of u were last read at (u, A)).
// The dy waves issue every LDS-DMA, a fixed count per wave per region, and
// retire each region with a counted vmcnt before the barrier ahead of its
// first reader.  Same dy formula and (p, q)-ascending window order as above;
// the MFMA k-order within a tile differs (column chunks), so results agree
// to fp32 rounding.
constexpr int SBW2_SA = 128 * 128, SBW2_SB = 96 * 128;  // dy slots of half A / B

__global__ void __launch_bounds__(768, 1) conv_stem_bwd_wgrad2_kernel(const StemBwArgs a) {
  typedef __bf16 T;
  typedef __attribute__((ext_vector_type(4))) __bf16 v4bf;
  constexpr int NB = 14;
  constexpr int NVW = 8;  // dy waves (2 per SIMD); waves 8-11 run the MFMAs
  static_assert(STEM_XBUF / 1024 >= NVW && (SBW_Y + SBW_DP + SBW_IX) / 1024 >= NVW, "padding re-issues block i - NVW");
  static_assert(2 * SBW_IN + SBW2_SA + SBW2_SB <= 160 * 1024, "LDS");
  __shared__ __attribute__((aligned(16))) char smem[2 * SBW_IN + SBW2_SA + SBW2_SB];
  char* const SA = smem + 2 * SBW_IN;
  char* const SB = SA + SBW2_SA;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool vw = wave < NVW;
  const int G = gridDim.x, g = blockIdx.x;
  const int u0 = (int)((long)g * a.tiles / G), u1 = (int)((long)(g + 1) * a.tiles / G);
  const __amdgpu_buffer_rsrc_t rsX = make_rsrc(a.X, a.x_bytes), rsY = make_rsrc(a.Y, a.y_bytes);
  const __amdgpu_buffer_rsrc_t rsP = make_rsrc(a.DP, a.dp_bytes), rsI = make_rsrc(a.IX, a.ix_bytes);
  const int xpitch = a.W * 8;
  const int yrun = 2 * a.Q * 128, prow = a.Q2 * 128, irow = a.Q2 * 64;
  auto buf = [&](int tile) { return smem + ((tile - u0) & 1) * SBW_IN; };

  // x rows of a tile (ceil(STEM_XBUF / NVW KiB) instructions per dy wave; a
  // tile past the range issues zero-fill so every wave's count is fixed)
  auto issue_x = [&](int tile) {
    const auto [n, h0] = tile_row(tile, STEM_TR, a.P);
    stem_issue_x<NVW, true>(rsX, n, h0, a.H, a.W, tile < u1, wave, lane, buf(tile));
  };
  // y (whole 1-KiB runs), pooled gradient rows and argmax rows of a tile
  auto issue_ypi = [&](int tile) {
    char* B = buf(tile);
    const bool ok = tile < u1;
    const auto [n, h0] = tile_row(tile, STEM_TR, a.P);
    const int T0 = h0 >> 1;
    const uint32_t yb = (uint32_t)((((long)n * a.P + h0) * a.Q) * 128);
    const int prows = (T0 + 1 < a.P2) ? 2 : 1;
    const uint32_t pb = (uint32_t)((((long)n * a.P2 + T0) * a.Q2) * 128);
    const uint32_t ib = (uint32_t)((((long)n * a.P2 + T0) * a.Q2) * 64);
    constexpr int NY = SBW_Y / 1024, NP = SBW_DP / 1024, NI = SBW_IX / 1024;
#pragma unroll
    for (int k = 0; k < (NY + NP + NI + NVW - 1) / NVW; ++k) {
      // past the regions: the wave's previous block again (same bytes to the same place)
      const int i = wave + NVW * k - (wave + NVW * k < NY + NP + NI ? 0 : NVW);
      const int b = (i < NY ? i : (i < NY + NP ? i - NY : i - NY - NP)) * 1024 + lane * 16;
      if (i < NY) {
        blds16(rsY, ok && b < yrun ? yb + (uint32_t)b : SSIP_OOB, B + STEM_XBUF + i * 1024);
      } else if (i < NY + NP) {
        blds16(rsP, ok && b < prows * prow ? pb + (uint32_t)b : SSIP_OOB, B + STEM_XBUF + i * 1024);
      } else {
        blds16(rsI, ok && b < prows * irow ? ib + (uint32_t)b : SSIP_OOB, B + STEM_XBUF + i * 1024);
      }
    }
  };
  constexpr int CX = (STEM_XBUF / 1024 + NVW - 1) / NVW;
  constexpr int CY = ((SBW_Y + SBW_DP + SBW_IX) / 1024 + NVW - 1) / NVW;

  // ---- dy waves: thread = (block lb, 4-channel quad c4) of a half
  const int lb = tid >> 4, c4 = tid & 15, ch0 = c4 * 4;
  float sc[4], sh[4], ca[4], cb[4], ck[4];
  if (vw) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      sc[e] = a.scale[ch0 + e];
      sh[e] = a.shift[ch0 + e];
      ca[e] = a.coef[ch0 + e];
      cb[e] = a.coef[64 + ch0 + e];
      ck[e] = a.coef[128 + ch0 + e];
    }
  }
  // half h of tile `tile` into slot D (GEMM row of pixel (j, q) = chunk * 32 + j * 16 + q % 16,
  // chunk = (q - q0) / 16 with q0 the half's first column)
  auto produce = [&](int tile, int h, char* D) {
    const int nblk = h == 0 ? 32 : 24;
    if (lb >= nblk) return;
    const int T0 = tile_row(tile, STEM_TR, a.P).p0 >> 1;
    const char* B = buf(tile);
    const char* Ys = B + STEM_XBUF;
    const char* Ps = Ys + SBW_Y;
    const char* Is = Ps + SBW_DP;
    const int l = (h == 0 ? 0 : 32) + lb;  // pooled window column: output columns 2l, 2l+1
    const bool q1 = l + 1 < a.Q2, p1 = T0 + 1 < a.P2;
    const uint32_t NOHIT = ~0u;  // no argmax byte is 255
    uint32_t k00, k01 = NOHIT, k10 = NOHIT, k11 = NOHIT;
    v4bf g00, g01, g10, g11;
    const v4bf z4 = (v4bf){(__bf16)0.f, (__bf16)0.f, (__bf16)0.f, (__bf16)0.f};
    k00 = *reinterpret_cast<const uint32_t*>(Is + l * 64 + ch0);
    g00 = *reinterpret_cast<const v4bf*>(Ps + l * 128 + ch0 * 2);
    g01 = g10 = g11 = z4;
    if (q1) {
      k01 = *reinterpret_cast<const uint32_t*>(Is + (l + 1) * 64 + ch0);
      g01 = *reinterpret_cast<const v4bf*>(Ps + (l + 1) * 128 + ch0 * 2);
    }
    if (p1) {
      k10 = *reinterpret_cast<const uint32_t*>(Is + (a.Q2 + l) * 64 + ch0);
      g10 = *reinterpret_cast<const v4bf*>(Ps + (a.Q2 + l) * 128 + ch0 * 2);
      if (q1) {
        k11 = *reinterpret_cast<const uint32_t*>(Is + (a.Q2 + l + 1) * 64 + ch0);
        g11 = *reinterpret_cast<const v4bf*>(Ps + (a.Q2 + l + 1) * 128 + ch0 * 2);
      }
    }
    float dz[4][4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int b00 = (int)((k00 >> (8 * e)) & 0xff), b01 = (int)((k01 >> (8 * e)) & 0xff);
      const int b10 = (int)((k10 >> (8 * e)) & 0xff), b11 = (int)((k11 >> (8 * e)) & 0xff);
      const float v00 = (float)g00[e], v01 = (float)g01[e], v10 = (float)g10[e], v11 = (float)g11[e];
      float d;
      d = 0.f; if (b00 == 4) d += v00;
      dz[0][e] = d;
      d = 0.f; if (b00 == 5) d += v00; if (b01 == 3) d += v01;
      dz[1][e] = d;
      d = 0.f; if (b00 == 7) d += v00; if (b10 == 1) d += v10;
      dz[2][e] = d;
      d = 0.f; if (b00 == 8) d += v00; if (b01 == 6) d += v01; if (b10 == 2) d += v10; if (b11 == 0) d += v11;
      dz[3][e] = d;
    }
    const int q0 = h == 0 ? 0 : 64;
#pragma unroll
    for (int px = 0; px < 4; ++px) {
      const int q = 2 * l + (px & 1), j = px >> 1;
      const int m = j * a.Q + q;                                      // pixel within the tile
      const int r = ((q - q0) >> 4) * 32 + j * 16 + ((q - q0) & 15);  // GEMM row within the half
      const v4bf yy = *reinterpret_cast<const v4bf*>(Ys + m * 128 + ch0 * 2);
      v4bf o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float yv = (float)yy[e];
        const float t = __builtin_fmaf(yv, sc[e], sh[e]);
        const float d = (t > 0.f ? t : 0.f) > 0.f ? dz[px][e] : 0.f;
        o[e] = (__bf16)(ca[e] * d + cb[e] * yv + ck[e]);
      }
      *reinterpret_cast<v4bf*>(D + r * 128 + (((c4 >> 1) ^ mt64_chunk_xor(r)) << 4) + (c4 & 1) * 8) = o;
    }
  };

  // ---- MFMA waves: wave mw = wave - NVW owns column blocks mw + 4 b (b < nbw) x all 64 k
  const int mw = wave - NVW;
  const int nbw = mw < NB - 12 ? 4 : 3;
  const int lg = lane >> 4, lq = (lane & 15) >> 2, lp = lane & 3;
  auto consume = [&](f32x4 (&acc)[4][4], int tile, int h, const char* D) {
    const char* Xs = buf(tile);
    const int nks = h == 0 ? 4 : 3, q0 = h == 0 ? 0 : 64;
    for (int ks = 0; ks < nks; ++ks) {
      Frag<T> fa[4], fb[4];
#pragma unroll
      for (int x = 0; x < 4; ++x) read_tfrag(fa[x], D, 32 * ks, x * 16, lane);
      // the lane's rows (lo, hi = lo + 4) of this chunk: output row >> 4, column q0 + 16 ks + (row & 15)
      const int m_lo = 8 * lg + lq, m_hi = m_lo + 4;
      const int base_lo = 2 * (m_lo >> 4) * xpitch + (q0 + 16 * ks + (m_lo & 15)) * 16;
      const int base_hi = 2 * (m_hi >> 4) * xpitch + (q0 + 16 * ks + (m_hi & 15)) * 16;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        if (b < nbw) {
          const int nb = mw + 4 * b, r = nb >> 1, cofs = ((nb & 1) * 16 + 4 * lp) * 2;
          read_tfrag_at(fb[b], Xs + base_lo + r * xpitch + cofs, Xs + base_hi + r * xpitch + cofs);
        }
      }
#pragma unroll
      for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int b = 0; b < 4; ++b)
          if (b < nbw) mma(acc[x][b], fa[x], fb[b]);
    }
  };

  // the two roles run separate loops (so neither holds the other's registers)
  // with the same barrier sequence: 2 in the prologue, 2 per tile
  if (vw) {
    if (u0 < u1) {
      // prologue: inputs of the first tile (+ y / pooled / argmax of the second), its half A
      issue_ypi(u0);
      issue_x(u0);
      issue_ypi(u0 + 1);
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(CY) : "memory");
      halo_lds_barrier();
      produce(u0, 0, SA);
      halo_lds_barrier();
    }
    for (int u = u0; u < u1; ++u) {
      // phase (u, A): dy (u, B) beside the MFMAs of (u, A); x of u+1 into its buffer
      issue_x(u + 1);
      produce(u, 1, SB);
      // y / pooled / argmax of u+1 (issued at (u-1, B)) land before the barrier
      // ahead of phase (u, B), whose dy waves form (u+1, A); younger: x of u+1
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(CX) : "memory");
      halo_lds_barrier();
      // phase (u, B): dy (u+1, A) beside the MFMAs of (u, B); y / pooled / argmax of u+2
      issue_ypi(u + 2);
      if (u + 1 < u1) produce(u + 1, 0, SA);
      // x of u+1 (issued at (u, A)) lands before the barrier ahead of (u+1, A);
      // younger: this phase's y / pooled / argmax of u+2
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(CY) : "memory");
      halo_lds_barrier();
    }
    // the zero-fill issues past the range land before the LDS is released
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  } else {
    f32x4 acc[4][4];
    zero_acc(acc);
    if (u0 < u1) {
      halo_lds_barrier();
      halo_lds_barrier();
    }
    for (int u = u0; u < u1; ++u) {
      consume(acc, u, 0, SA);
      halo_lds_barrier();
      consume(acc, u, 1, SB);
      halo_lds_barrier();
    }
    float* sl = a.slab + (long)g * 64 * 224;
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
      for (int b = 0; b < 4; ++b)
        if (b < nbw) store_slab_frag(sl, 224, x * 16, (mw + 4 * b) * 16, acc[x][b], lane);
  }
}

}  // namespace

#pragma once
#include "conv_tile.h"

namespace {

// ---------------------------------------------------------------------------
// Halo-resident 3x3 / stride 1 / pad 1 convolution over 64 reduction
// channels: every forward conv of ResNet layer1 and every stride-1 DGRAD
// whose reduction is 64 channels (the same conv of dy with the taps flipped).
//
// The implicit-GEMM kernel above gathers the A operand once per tap (each
// input pixel crosses L2 -> LDS nine times) and pays a barrier per k-step.
// Here a persistent workgroup (one per CU) keeps the whole 64-column weight
// panel (9 taps x 64 x 64 bf16 = 72 KiB) resident in LDS and stages, per
// tile of TR whole output rows (TR*W <= 256 pixels of one image), the
// (TR+2) x (W+2) zero-haloed input rows once.  Tap (r, s) of output pixel
// (j, q) is LDS pixel (j + r)(W+2) + q + s, a uniform offset from tap (0, 0),
// so the nine taps are nine shifted fragment reads of one LDS image and the
// 18 MFMA k-steps of a tile run with no barrier.  The input rows are double
// buffered: tile u+1's rows are DMA'd while tile u computes, and tile u's
// epilogue stages its output through its own (then idle) buffer.  The wait
// for the next rows is a counted vmcnt that leaves the epilogue's stores in
// flight (vector-memory ops retire in issue order; the epilogue issues a
// fixed number of them per thread through buffer ops, rows past the tile
// going to an out-of-range offset).  LDS pixels use ktile_off's 16-B slot
// swizzle (conflict-free ds_read_b128 over 16 consecutive pixels).  Each
// MFMA k-step is one weight tap's 64 channels, in tap order, exactly as in
// conv_glds_kernel: the outputs are the same bits.
//
// FWD epilogue: bf16 y plus the BatchNorm statistics of the workgroup's
// tiles merged in fixed order (Chan) into one {count, sum, M2} record per
// (channel, workgroup): [Ncols][G][3].  DGRAD epilogue: dx (+ add, which may
// alias dx).
// ---------------------------------------------------------------------------

struct HaloArgs {
  const __bf16* X;    // [N][H][W][64]   (FWD: x, DGRAD: dy)
  const __bf16* Wt;   // [Ncols][9][64]  (FWD: w_krsc, DGRAD: w_crsk)
  __bf16* out;        // [N][H][W][Ncols]
  const __bf16* add;  // DGRAD residual gradient / FWD residual (nullable, may alias out)
  float* partial;     // FWD BN records (nullable)
  const float* bias;  // FWD per-channel bias (folded eval BN), nullable
  int relu;           // FWD ReLU after bias and residual
  uint32_t x_bytes, w_bytes, o_bytes;
  int N, H, W, Ncols, TR, tiles, units, flip;
  // DGRAD BN-backward post-op (conv_halo_kernel<..., BNPOST>, ssip_conv_dgrad_bn):
  // out = (dgrad + add) * relu_mask, and per-(channel, workgroup, wave row)
  // sums {out, out * (y - mean) * invstd} into partial [Ncols][G][HALO_WMW][2].
  // Mask: bit c & 7 of pbits[pixel * Ncols / 8 + c / 8], or (pbits null)
  // fma(y, mscale, mshift) > 0.
  const __bf16* py;
  const uint8_t* pbits;
  const float *pmean, *pinvstd, *pmscale, *pmshift;
  uint32_t bits_bytes;
  // INBN (FWD): the input is y of the BN+ReLU below; x = relu(fma(y, in_scale,
  // in_shift)) is formed in LDS (ssip_conv_fwd_bnrelu_in)
  const float *in_scale, *in_shift;
  __bf16* zout;  // INBN (nullable): the transformed input's own tile rows written out (the wgrad's x)
};

constexpr int HALO_XBUF = 44 * 1024;  // one input-row buffer: (TR + 2) * (W + 2) <= 352 pixels

// X-row LDS image: pixel px's 128-B row, 16-B slot s at s ^ 2((px >> 1) & 3).
// Fragment reads start at any pixel (tap shifts); with this swizzle the 16
// lanes of every ds_read_b128 lane group ({0-3,12-15,20-27}, ...: rows
// r0..r0+15 across two k-slots) hit 16 distinct 16-B bank slots for every r0
// (ktile_off's swizzle is conflict-free only for r0 = 0 mod 16).
__device__ __forceinline__ int xtile_off(int px, int slot) { return px * 128 + ((slot ^ (((px >> 1) & 3) << 1)) << 4); }

// conv_halo_kernel's DGRAD epilogue with the BN-backward reduction of the
// BN+ReLU below fused in (ssip_conv_dgrad_bn): per row-fragment i, the
// residual-gradient add, y and the mask bytes of the lane's 4 x FN elements
// are loaded together, then d = relu_mask ? bf16(bf16(acc) + add) : 0 is
// stored and summed (d, d * (y - mean) * invstd) into the lane's columns.
// Padded-grid rows (vmask clear) store nothing and add nothing.
template <int FM, int FN, int BATCH, bool YONLY>
__device__ __forceinline__ void halo_bnpost_epilogue(const HaloArgs& a, const f32x4 (&acc)[FM][FN],
                                                     __amdgpu_buffer_rsrc_t rsO, __amdgpu_buffer_rsrc_t rsA,
                                                     __amdgpu_buffer_rsrc_t rsY, __amdgpu_buffer_rsrc_t rsM, int tile,
                                                     int rows, int col0, const uint32_t (&rowoff)[FM][4],
                                                     uint32_t vmask, int cbase, float (&bsd)[FN], float (&bsx)[FN],
                                                     const short (*pre_y)[FN][4] = nullptr) {
  typedef __bf16 T;
  static_assert(FM % BATCH == 0, "row-group batches");
  const uint32_t obase = (uint32_t)(((long)tile * rows * a.Ncols + col0) * 2);
  float mu[FN], is[FN], msc[FN], msh[FN];
  const bool bits = !YONLY && a.pbits != nullptr;  // YONLY: no add, mask from the BN affine
  const bool has_add = !YONLY && a.add != nullptr;
#pragma unroll
  for (int jj = 0; jj < FN; ++jj) {
    const int c = col0 + cbase + jj * 16;
    mu[jj] = a.pmean[c];
    is[jj] = a.pinvstd[c];
    msc[jj] = bits ? 0.f : a.pmscale[c];
    msh[jj] = bits ? 0.f : a.pmshift[c];
  }
  const int cbit = cbase & 7;  // column c's bit in its mask byte (jj * 16 keeps c & 7)
  // the operands of BATCH row groups per round trip (all FM in one where the
  // registers allow: each batch is a dependent HBM round trip per tile)
#pragma unroll
  for (int i0 = 0; i0 < FM; i0 += BATCH) {
    short ra[BATCH][FN][4], ry[BATCH][FN][4];
    uint32_t rm[BATCH][FN][4];
#pragma unroll
    for (int b = 0; b < BATCH; ++b)
#pragma unroll
      for (int jj = 0; jj < FN; ++jj)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int i = i0 + b;
          const uint32_t off = obase + rowoff[i][e] + jj * 32;
          const bool valid = (vmask >> (i * 4 + e)) & 1u;
          ry[b][jj][e] = pre_y ? pre_y[i][jj][e] : __builtin_amdgcn_raw_buffer_load_b16(rsY, off, 0, 0);
          ra[b][jj][e] = has_add ? __builtin_amdgcn_raw_buffer_load_b16(rsA, off, 0, 0) : (short)0;
          rm[b][jj][e] =
              bits ? (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(rsM, valid ? off >> 4 : SSIP_OOB, 0, 0) : 0u;
        }
#pragma unroll
    for (int b = 0; b < BATCH; ++b)
#pragma unroll
      for (int jj = 0; jj < FN; ++jj)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int i = i0 + b;
          const uint32_t off = obase + rowoff[i][e] + jj * 32;
          const bool valid = (vmask >> (i * 4 + e)) & 1u;
          const float yv = to_f32(__builtin_bit_cast(T, ry[b][jj][e]));
          float t = to_f32(from_f32<T>(acc[i][jj][e]));
          if (has_add) t += to_f32(__builtin_bit_cast(T, ra[b][jj][e]));
          const bool keep = bits ? ((rm[b][jj][e] >> cbit) & 1u) != 0u : __builtin_fmaf(yv, msc[jj], msh[jj]) > 0.f;
          const T o = from_f32<T>(keep ? t : 0.f);
          __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(short, o), rsO, off, 0, 0);
          const float dq = valid ? to_f32(o) : 0.f;
          bsd[jj] += dq;
          bsx[jj] += dq * ((yv - mu[jj]) * is[jj]);
        }
  }
}

// BNPOST: 0 = none; 1 = the BN-backward post-op with no residual add and the
// mask from the BN affine (y is the only extra operand: one load batch per
// tile); 2 = any other post-op operand set (one load batch per row group:
// the registers hold no more without spilling)
template <int WMW, int WNW, bool FOLD = false, int BNPOST = 0, bool ADD = false, bool INBN = false>
__global__ void __launch_bounds__(64 * WMW * WNW, (WMW * WNW) / 4) conv_halo_kernel(const HaloArgs a) {
  typedef __bf16 T;
  constexpr int NW = WMW * WNW, NT = 64 * NW;
  constexpr int BM = 256, BN = 64;
  constexpr int WTM = BM / WMW, WTN = BN / WNW, FM = WTM / 16, FN = WTN / 16;
  constexpr int B_BYTES = 9 * BN * 128;
  static_assert(FM >= 1 && FN >= 1 && (NW == 4 || NW == 8 || NW == 16) && WMW <= HALO_WMW, "bad halo wave tile");
  static_assert(B_BYTES + 2 * HALO_XBUF <= 160 * 1024, "LDS");
  __shared__ __attribute__((aligned(16))) char smem[B_BYTES + 2 * HALO_XBUF];
  char* const Bs = smem;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WNW, wn = wave % WNW;
  const int G = gridDim.x, g = blockIdx.x;
  const int u0 = (int)((long)g * a.units / G), u1 = (int)((long)(g + 1) * a.units / G);
  const __amdgpu_buffer_rsrc_t rsX = make_rsrc(a.X, a.x_bytes), rsW = make_rsrc(a.Wt, a.w_bytes);
  const __amdgpu_buffer_rsrc_t rsO = make_rsrc(a.out, a.o_bytes), rsA = make_rsrc(a.add, a.o_bytes);
  const __amdgpu_buffer_rsrc_t rsZ = make_rsrc(a.zout, a.zout ? a.x_bytes : 0);
  typedef __attribute__((ext_vector_type(4))) unsigned int hv4u;
  const int Wp = a.W + 2;
  const int npx = (a.TR + 2) * Wp;
  const int nxi = (npx + 7) >> 3;  // X DMA wave-instructions per tile (8 pixels each)
  const int rows = a.TR * a.W;     // output pixels per tile
  const int mrows = a.TR * Wp;     // GEMM rows per tile: the padded grid (q = W, W+1 are discarded)

  // one 1-KiB LDS-DMA piece (8 pixels) of tile (n, p0)'s input rows
  auto issue_x_piece = [&](int n, int p0, int i, char* Xs) {
    const int px = i * 8 + (lane >> 3);
    const int sr = px / Wp, sc = px - sr * Wp;
    const int pin = p0 - 1 + sr, win = sc - 1;
    const int ch = (lane & 7) ^ (((px >> 1) & 3) << 1);  // xtile_off's swizzle
    const bool ok = px < npx && pin >= 0 && pin < a.H && win >= 0 && win < a.W;
    const uint32_t off = (uint32_t)(((((long)n * a.H + pin) * a.W + win) * 64 + ch * 8) * 2);
    blds16(rsX, ok ? off : SSIP_OOB, Xs + i * 1024);
  };
  auto issue_x = [&](int tile, char* Xs) {
    const auto [n, p0] = tile_row(tile, a.TR, a.H);
    for (int i = wave; i < nxi; i += NW) issue_x_piece(n, p0, i, Xs);
  };
  constexpr int XPW = (HALO_XBUF / 1024 + NW - 1) / NW;  // most pieces per wave and tile
  // INBN: this wave's pieces of `tile` (landed: after its vmcnt(0)) become
  // relu(bn(y)) in place; halo and out-of-image pixels stay zero.  Every
  // wave transforms only what it DMA'd, so the next barrier publishes it.
  // A lane's LDS chunk is (lane & 7) ^ xtile swizzle of px = 8 i + lane / 8,
  // i.e. ((px >> 1) & 3) = (lane >> 4) & 3 for every piece i: the lane's
  // eight channels, and so its scale / shift, are fixed for the whole kernel
  // (loaded once here; per piece they were a dependent L2 round trip each)
  float isc[8], ish[8];
  if constexpr (INBN) {
    const int c0 = ((lane & 7) ^ (((lane >> 4) & 3) << 1)) * 8;
    load_f8(isc, a.in_scale + c0);
    load_f8(ish, a.in_shift + c0);
  }
  auto xform_x = [&](int tile, char* Xs, bool zst) {
    const int R0 = tile * a.TR;
    const int n = R0 / a.H, p0 = R0 - n * a.H;
    for (int i = wave; i < nxi; i += NW) {
      const int px = i * 8 + (lane >> 3);
      const int sr = px / Wp, sc = px - sr * Wp;
      const int pin = p0 - 1 + sr, win = sc - 1;
      const bool ok = px < npx && pin >= 0 && pin < a.H && win >= 0 && win < a.W;
      if (ok) {
        char* const q = Xs + i * 1024 + lane * 16;
        bnrelu_chunk(q, isc, ish);
        if (zst && sr >= 1 && sr <= a.TR) {
          const int ch = (lane & 7) ^ (((px >> 1) & 3) << 1);
          const uint32_t off = (uint32_t)(((((long)n * a.H + pin) * a.W + win) * 64 + ch * 8) * 2);
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(hv4u, *reinterpret_cast<const bf16x8*>(q)),
                                                 rsZ, off, 0, 0);
        }
      }
    }
  };
  // INBN register staging of the next tile's pieces (XLAG + 1 slots)
  constexpr int XLAG = 2;
  bf16x8 xr[XLAG + 1];
  bool xok[XLAG + 1];
  uint32_t xzo[XLAG + 1];  // z_out offset of the piece (SSIP_OOB: halo row, padding or no z_out)
  auto xreg_load = [&](int n, int p0, int i, int slot, bool zst_tile) {
    const int px = i * 8 + (lane >> 3);
    const int sr = px / Wp, sc = px - sr * Wp;
    const int pin = p0 - 1 + sr, win = sc - 1;
    const int ch = (lane & 7) ^ (((px >> 1) & 3) << 1);  // xtile_off's swizzle
    const bool ok = px < npx && pin >= 0 && pin < a.H && win >= 0 && win < a.W;
    const uint32_t off = (uint32_t)(((((long)n * a.H + pin) * a.W + win) * 64 + ch * 8) * 2);
    xr[slot] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rsX, ok ? off : SSIP_OOB, 0, 0));
    xok[slot] = ok;
    xzo[slot] = (ok && zst_tile && sr >= 1 && sr <= a.TR) ? off : SSIP_OOB;
  };
  auto xreg_store = [&](int i, int slot, char* Xs) {
    bf16x8 v = xr[slot];
    if (xok[slot]) v = bnrelu8(v, isc, ish);
    *reinterpret_cast<bf16x8*>(Xs + i * 1024 + lane * 16) = v;
    if (a.zout) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(hv4u, v), rsZ, xzo[slot], 0, 0);
  };
  auto issue_w = [&](int jn) {
    for (int i = wave; i < 72; i += NW) {
      const int tw = i >> 3, col = ((i & 7) << 3) + (lane >> 3);
      const int ch = (lane & 7) ^ ((col >> 1) & 7);
      const uint32_t off = (uint32_t)(((((long)jn * 64 + col) * 9 + tw) * 64 + ch * 8) * 2);
      blds16(rsW, off, Bs + i * 1024);
    }
  };

  // per-lane fragment bases: A rows (LDS pixel of tap (0, 0)), B columns
  int pxb[FM];
#pragma unroll
  for (int i = 0; i < FM; ++i) {
    const int m = wm * WTM + i * 16 + (lane & 15);
    pxb[i] = m < mrows ? m : 0;  // row m of the padded grid reads LDS pixel m + tap offset
  }
  const int kq = lane >> 4;
  // A-fragment LDS offsets of the first 32-channel half, per row group and
  // k-step tap (DGRAD: flipped), fixed for all tiles: 9 FM registers.  The
  // second half is the same pixel at slot ^ 4, i.e. offset ^ 64 (xtile_off's
  // swizzle only XORs the slot, and the buffer bases are multiples of 128):
  // one v_xor per read instead of 9 FM more hoisted offsets.
  uint32_t offA[FM][9];
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const int tt = a.flip ? 8 - t : t;
    const int toff = (tt / 3) * Wp + (tt % 3);
#pragma unroll
    for (int i = 0; i < FM; ++i) offA[i][t] = (uint32_t)xtile_off(pxb[i] + toff, kq);
  }
  int boff[FN][2];
#pragma unroll
  for (int jj = 0; jj < FN; ++jj)
#pragma unroll
    for (int kh = 0; kh < 2; ++kh) boff[jj][kh] = ktile_off(wn * WTN + jj * 16 + (lane & 15), 4 * kh + kq);

  // BN records [Ncols][G][WMW][3]: one per (channel, workgroup, wave row);
  // zero this workgroup's, then lanes < 16 of each wave keep the running
  // {n, mean, M2} of their FN columns over the wave's rows of every tile
  constexpr int RV = BNPOST ? 2 : 3;  // floats per record
  if (a.partial) bn_records_zero<RV>(a.partial, a.Ncols, G, g, tid, NT);
  // BNPOST: this lane's running sums {d, d * xhat} of its FN columns
  float bsd[FN], bsx[FN];
#pragma unroll
  for (int jj = 0; jj < FN; ++jj) bsd[jj] = bsx[jj] = 0.f;
  const __amdgpu_buffer_rsrc_t rsY = make_rsrc(a.py, BNPOST ? a.o_bytes : 0);
  const __amdgpu_buffer_rsrc_t rsM = make_rsrc(a.pbits, BNPOST ? a.bits_bytes : 0);
  WaveStats<FM, FN> ws;
  ws.reset();
  // this lane's output rows (rbase + 16 i + e): byte offset within a tile's
  // output block and validity (q < W of the padded grid), fixed for all tiles
  const int rbase = wm * WTM + kq * 4, cbase = wn * WTN + (lane & 15);
  uint32_t rowoff[FM][4];
  const uint32_t vmask = lane_out_rows(rowoff, rbase, cbase, Wp, mrows, a.W, a.Ncols);
  const int wrows = count_out_rows(wm * WTM, WTM, Wp, mrows, a.W);  // valid rows of this wave in a tile (uniform)

  if (u0 < u1) {
    const int jn = u0 / a.tiles;
    issue_w(jn);
    issue_x(u0 - jn * a.tiles, smem + B_BYTES);
  }
  const bool stats = a.partial && wrows > 0;
  constexpr bool has_add = ADD;  // BNPOST == 0: out += add (BNPOST reads a.add itself)
  // The epilogue of one row group i of a finished tile: BN statistics over the
  // fp32 accumulators of its valid rows, then 16-bit stores straight from the
  // accumulators (lane: 4 rows x 1 column per fragment; padded-grid rows go to
  // an out-of-range offset), with the residual (ra, loaded beforehand) and the
  // folded eval BN bias / ReLU applied.  Round 5 measured the stores at 3 us
  // of a 78 us layer-1 forward and a transposed tile with 16-B row stores at
  // 93 us (profiles/r5_halo_lab.txt): the 32-B pieces do not bound the kernel.
  auto epi_rows = [&](const f32x4 (&ac)[FM][FN], int i, int etile, int ejn, const short (&ra)[FM][FN][4]) {
    if (stats) ws.rows(ac, vmask, i);
    const uint32_t obase = (uint32_t)(((long)etile * rows * a.Ncols + ejn * BN) * 2);
    const float lo = (FOLD && a.relu) ? 0.f : -__builtin_huge_valf();
#pragma unroll
    for (int jj = 0; jj < FN; ++jj) {
      const float bcol = FOLD ? a.bias[ejn * BN + cbase + jj * 16] : 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const uint32_t off = obase + rowoff[i][e] + jj * 32;
        float t = FOLD ? ac[i][jj][e] + bcol : ac[i][jj][e];
        if (has_add) t = to_f32(from_f32<T>(t)) + to_f32(__builtin_bit_cast(T, ra[i][jj][e]));
        const T o = from_f32<T>(FOLD ? fmaxf(t, lo) : t);
        __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(short, o), rsO, off, 0, 0);
      }
    }
  };
  auto epi_load = [&](int etile, int ejn, short (&ra)[FM][FN][4]) {
    const uint32_t obase = (uint32_t)(((long)etile * rows * a.Ncols + ejn * BN) * 2);
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int jj = 0; jj < FN; ++jj)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          ra[i][jj][e] = __builtin_amdgcn_raw_buffer_load_b16(rsA, obase + rowoff[i][e] + jj * 32, 0, 0);
  };

  // One barrier per tile: after it every wave has finished the previous
  // tile's fragment reads (so that buffer may take the next rows) and has
  // seen its own share of this tile's rows land (the vmcnt(0) each wave
  // issues after its MFMAs, by which time the prefetch has had the whole
  // MFMA phase).  The epilogue writes straight from the accumulators with
  // 16-bit buffer stores and needs no LDS, so a wave that finishes its MFMAs
  // early runs its epilogue while the other waves still compute, and its
  // stores stay in flight into the next tile.  (Round 5 deferred each tile's
  // epilogue into the next tile's MFMAs, one row group per 4 k-steps: the 32
  // accumulators it keeps push the kernel past 256 VGPRs into spills, 132 vs
  // 82 us; profiles/r5_halo_lab.txt.)
  short rap[FM][FN][4];
  bool first = true;
  for (int u = u0; u < u1; ++u) {
    const int jn = u / a.tiles, tile = u - jn * a.tiles;
    char* const Xs = smem + B_BYTES + ((u - u0) & 1) * HALO_XBUF;
    char* const Xn = smem + B_BYTES + ((u - u0 + 1) & 1) * HALO_XBUF;
    if (first) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if constexpr (INBN) xform_x(tile, Xs, a.zout != nullptr && jn == 0);
    }
    first = false;
    halo_lds_barrier();
    const int un = u + 1;
    const bool more = un < u1;
    const int jn_next = more ? un / a.tiles : jn;
    const bool prefetch = more && jn_next == jn;
    // this tile's epilogue operands (the residual; BNPOST 1: y) are requested
    // now and land during the MFMAs: loaded after them, each tile paid a
    // dependent HBM round trip before its stores
    if constexpr (BNPOST == 0 && has_add) epi_load(tile, jn, rap);
    if constexpr (BNPOST == 1) {
      const uint32_t ob = (uint32_t)(((long)tile * rows * a.Ncols + jn * BN) * 2);  // the epilogue's obase
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int jj = 0; jj < FN; ++jj)
#pragma unroll
          for (int e = 0; e < 4; ++e)
            rap[i][jj][e] = __builtin_amdgcn_raw_buffer_load_b16(rsY, ob + rowoff[i][e] + jj * 32, 0, 0);
    }
    // the next tile's rows go to tile u-1's buffer (every wave is past its
    // reads): one piece per wave after every other k-step's MFMAs, so the
    // DMA issue (~60-185 cycles a piece) runs beside the matrix pipe instead
    // of ahead of it with the partner wave's in the same place
    const auto [nn, np0] = tile_row(un - jn * a.tiles, a.TR, a.H);

    f32x4 acc[FM][FN];
    zero_acc(acc);
    // 18 k-steps (weight tap t, 32-channel half kh) in weight-tap order, as
    // conv_glds_kernel; DGRAD's tap t reads dy at the flipped shift 8 - t.
    // Fragments are read one k-step ahead (register double buffer) so the
    // LDS latency hides behind the previous step's MFMAs.
    Frag<T> fa[2][FM], fb[2][FN];
    const uint32_t xbase = (uint32_t)(Xs - smem);
    uint32_t m64 = 64;  // opaque per tile: keeps offA ^ 64 from being hoisted into 9 FM more registers
    asm volatile("" : "+s"(m64));
    uint32_t xa[FM];
    auto load_step = [&](int st, Frag<T>(&ra)[FM], Frag<T>(&rb)[FN]) {
      const int t = st >> 1, kh = st & 1;
      const char* bt = Bs + t * (BN * 128);
#pragma unroll
      for (int i = 0; i < FM; ++i) {
        xa[i] = kh ? xa[i] ^ m64 : xbase + offA[i][t];
        ra[i].v = *reinterpret_cast<const bf16x8*>(smem + xa[i]);
      }
#pragma unroll
      for (int jj = 0; jj < FN; ++jj) rb[jj].v = *reinterpret_cast<const bf16x8*>(bt + boff[jj][kh]);
    };
    load_step(0, fa[0], fb[0]);
#pragma unroll
    for (int st = 0; st < 18; ++st) {
      if (st + 1 < 18) load_step(st + 1, fa[(st + 1) & 1], fb[(st + 1) & 1]);
      // step st + 1's fragment reads go out before step st's MFMAs: with the
      // k-loop one basic block the scheduler otherwise sinks each read to just
      // before its first use (lgkmcnt(0) ahead of most MFMAs)
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int jj = 0; jj < FN; ++jj)
          mma(acc[i][jj], fa[st & 1][i], fb[st & 1][jj]);
      if (st % 2 == 0 && st / 2 < XPW) {
        const int i = wave + (st / 2) * NW;
        if constexpr (INBN) {
          // INBN: the piece comes through registers -- a buffer load now, the
          // BN+ReLU and one LDS store XLAG pieces later (by then it has
          // landed) -- so the transform needs no LDS read-modify-write pass and
          // its VALU work sits between k-steps beside the partner wave's MFMAs
          // (issued unconditionally -- an unneeded piece reads the OOB zero --
          // so the compiler can count the loads in flight: vmcnt(XLAG) before
          // a store instead of vmcnt(0))
          xreg_load(nn, np0, i, (st / 2) % (XLAG + 1), a.zout != nullptr && jn == 0);
        } else {
          if (prefetch && i < nxi) issue_x_piece(nn, np0, i, Xn);
        }
      }
      if constexpr (INBN) {
        if (st % 2 == 0 && st / 2 >= XLAG && st / 2 - XLAG < XPW) {
          const int k = st / 2 - XLAG, i = wave + k * NW;
          if (prefetch && i < nxi) xreg_store(i, k % (XLAG + 1), Xn);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    // the next tile's rows (issued among the MFMAs) and this wave's older
    // stores retire here; nothing younger is in flight
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if constexpr (INBN) {
      // pieces staged too late for the k-loop's stores (XPW + XLAG > 9)
#pragma unroll
      for (int k = 9 - XLAG; k < XPW; ++k) {
        const int i = wave + k * NW;
        if (prefetch && k >= 0 && i < nxi) xreg_store(i, k % (XLAG + 1), Xn);
      }
    }

    // ---- epilogue
    if constexpr (BNPOST) {
      halo_bnpost_epilogue<FM, FN, BNPOST == 1 ? FM : 1, BNPOST == 1>(
          a, acc, rsO, rsA, rsY, rsM, tile, rows, jn * BN, rowoff, vmask, cbase, bsd, bsx,
          BNPOST == 1 ? rap : nullptr);
      if (!prefetch) {
        // panel / range end: the wave's column sums -> records [c][g][wm]
#pragma unroll
        for (int jj = 0; jj < FN; ++jj)
#pragma unroll
          for (int off = 16; off <= 32; off <<= 1) {
            bsd[jj] += __shfl_xor(bsd[jj], off, 64);
            bsx[jj] += __shfl_xor(bsx[jj], off, 64);
          }
        if (lane < 16) {
#pragma unroll
          for (int jj = 0; jj < FN; ++jj) {
            float* rec = bn_record(a.partial, jn * BN + cbase + jj * 16, G, g, wm, 2);
            rec[0] = bsd[jj];
            rec[1] = bsx[jj];
          }
        }
#pragma unroll
        for (int jj = 0; jj < FN; ++jj) bsd[jj] = bsx[jj] = 0.f;
      }
    } else {
#pragma unroll
      for (int i = 0; i < FM; ++i) epi_rows(acc, i, tile, jn, rap);
      if (stats && !prefetch) ws.flush(a.partial, jn * BN + cbase, G, g, wm, lane);
    }
    if (more && !prefetch) {
      // panel change: new weights and the next tile's rows, loaded once every
      // wave is past this tile's MFMAs
      halo_lds_barrier();
      issue_w(jn_next);
      issue_x(un - jn_next * a.tiles, Xn);
      first = true;
    }
  }
}

// ---------------------------------------------------------------------------
// WGRAD of the same 3x3 / stride 1 / pad 1 convs with C = K = 64 (layer1):
//   dW[k][(t, c)] = sum_m dy[m][k] * x_pad[m + toff(t)][c]
// over the padded-grid rows m = j (W+2) + q of each tile (dy is zero at
// q >= W).  A persistent workgroup (one per CU) stages per tile the input
// rows (as conv_halo_kernel, with the m-major MTile swizzle) and the tile's
// dy rows, both double-buffered, and keeps the whole 64 x 576 fp32 result in
// registers across its tiles (waves: 2 k-halves x 4 quarters of the 36
// (tap, 16-channel) column blocks); the nine taps are shifted transposed
// fragment reads of the one input image.  At the end each workgroup writes
// its partial dW as one fp32 slab; wgrad_reduce_kernel sums the slabs in
// fixed order (deterministic).
// ---------------------------------------------------------------------------
struct HaloWgArgs {
  const __bf16* X;   // [N][H][W][64]
  const __bf16* DY;  // [N][H][W][64]
  float* slab;       // [G][64][576]
  uint32_t x_bytes;
  int N, H, W, TR, tiles;
  // INBN: X is y of the BN+ReLU below; relu(fma(y, in_scale, in_shift)) is
  // formed in LDS (ssip_conv_wgrad_bnrelu_in)
  const float *in_scale, *in_shift;
};

constexpr int HWG_XBUF = 48 * 1024;  // 384 input-image rows x 128 B
constexpr int HWG_DBUF = 32 * 1024;  // 256 dy rows x 128 B

template <bool INBN = false>
__global__ void __launch_bounds__(512, 2) conv_halo_wgrad_kernel(const HaloWgArgs a) {
  typedef __bf16 T;
  constexpr int NW = 8;
  // the two tile buffers as two objects: the tile loop runs unrolled by two,
  // so the compiler sees that this tile's fragment reads and the next tile's
  // LDS-DMA never alias (one array: a vmcnt(0) wait for the DMA ahead of every
  // read that followed it)
  __shared__ __attribute__((aligned(16))) char smem0[HWG_XBUF + HWG_DBUF];
  __shared__ __attribute__((aligned(16))) char smem1[HWG_XBUF + HWG_DBUF];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;  // k rows 32 wm .. +31; column blocks 9 wn .. 9 wn + 8
  const int G = gridDim.x, g = blockIdx.x;
  const int u0 = (int)((long)g * a.tiles / G), u1 = (int)((long)(g + 1) * a.tiles / G);
  const __amdgpu_buffer_rsrc_t rsX = make_rsrc(a.X, a.x_bytes), rsD = make_rsrc(a.DY, a.x_bytes);
  const int Wp = a.W + 2;
  const int npx = (a.TR + 2) * Wp, mrows = a.TR * Wp;

  // LDS-DMA pieces of a tile: all 48 of the input image's (the k-loop reads
  // rows up to 255 + 2 Wp + 2: dy is zero at m >= mrows, but 0 x garbage in
  // an unfilled row is NaN), then all 32 of dy's
  constexpr int nxp = HWG_XBUF / 1024, npieces = nxp + HWG_DBUF / 1024;
  auto issue_piece = [&](int n, int p0, int i, char* Xs, char* Ds) {
    if (i < nxp) {  // input image: 8 rows per instruction
      const int px = i * 8 + (lane >> 3);
      const int sr = px / Wp, sc = px - sr * Wp;
      const int pin = p0 - 1 + sr, win = sc - 1;
      const int ch = (lane & 7) ^ mt64_chunk_xor(px);  // MTile<64>
      const bool ok = px < npx && pin >= 0 && pin < a.H && win >= 0 && win < a.W;
      const uint32_t off = (uint32_t)(((((long)n * a.H + pin) * a.W + win) * 64 + ch * 8) * 2);
      blds16(rsX, ok ? off : SSIP_OOB, Xs + i * 1024);
    } else {  // dy rows of the padded grid
      const int m = (i - nxp) * 8 + (lane >> 3);
      const int j = m / Wp, q = m - j * Wp;
      const int ch = (lane & 7) ^ mt64_chunk_xor(m);
      const bool ok = m < mrows && q < a.W;
      const uint32_t off = (uint32_t)(((((long)n * a.H + p0 + j) * a.W + q) * 64 + ch * 8) * 2);
      blds16(rsD, ok ? off : SSIP_OOB, Ds + (i - nxp) * 1024);
    }
  };
  auto issue = [&](int tile, char* Xs, char* Ds) {
    const int R0 = tile * a.TR;
    const int n = R0 / a.H, p0 = R0 - n * a.H;
    for (int i = wave; i < npieces; i += NW) issue_piece(n, p0, i, Xs, Ds);
  };
  // INBN: this wave's input-image pieces of `tile` (landed) become
  // relu(bn(y)) in place; padding and out-of-image pixels stay zero
  // (a lane's chunk, (lane & 7) ^ mt64_chunk_xor(8 i + lane / 8), depends on i
  // only through i & 1 = wave & 1: one scale / shift load per call, not per piece)
  auto xform_x = [&](int tile, char* Xs) {
    const int R0 = tile * a.TR;
    const int n = R0 / a.H, p0 = R0 - n * a.H;
    (void)n;
    float isc[8], ish[8];
    const int c0 = ((lane & 7) ^ mt64_chunk_xor(wave * 8 + (lane >> 3))) * 8;
    load_f8(isc, a.in_scale + c0);
    load_f8(ish, a.in_shift + c0);
    for (int i = wave; i < nxp; i += NW) {
      const int px = i * 8 + (lane >> 3);
      const int sr = px / Wp, sc = px - sr * Wp;
      const int pin = p0 - 1 + sr, win = sc - 1;
      const bool ok = px < npx && pin >= 0 && pin < a.H && win >= 0 && win < a.W;
      if (ok) bnrelu_chunk(Xs + i * 1024 + lane * 16, isc, ish);
    }
  };
  // This wave's pieces of every tile -- i = wave + 8 k: k < 6 input image, k >= 6
  // dy -- as tile-independent byte offsets from the tile's first pixel, with
  // the input piece's row (0 .. TR + 1) in bits 0-2 and bit 3 set where the
  // piece lane is always out of range; only the input rows above / below the
  // image depend on the tile.  The k-loop issues them two per k-step, beside
  // the MFMAs, without the division of issue_piece.
  static_assert(nxp == 6 * NW && npieces == 10 * NW, "piece map");
  int pc[10];
#pragma unroll
  for (int k = 0; k < 10; ++k) {
    if (k < 6) {
      const int px = (wave + NW * k) * 8 + (lane >> 3);
      const int sr = px / Wp, sc = px - sr * Wp, win = sc - 1;
      const int ch = (lane & 7) ^ mt64_chunk_xor(px);
      const bool ok = px < npx && win >= 0 && win < a.W;
      pc[k] = ((((sr - 1) * a.W + win) * 64 + ch * 8) * 2) | (sr & 7) | (ok ? 0 : 8);
    } else {
      const int m = (wave + NW * (k - 6)) * 8 + (lane >> 3);
      const int j = m / Wp, q = m - j * Wp;
      const int ch = (lane & 7) ^ mt64_chunk_xor(m);
      const bool ok = m < mrows && q < a.W;
      pc[k] = (((j * a.W + q) * 64 + ch * 8) * 2) | (ok ? 0 : 8);
    }
  }
  auto issue_pc = [&](int k, int base, int p0, char* Xs, char* Ds) {
    const int v = pc[k];
    bool ok = (v & 8) == 0;
    if (k < 6) {
      const int pin = p0 - 1 + (v & 7);
      ok = ok && pin >= 0 && pin < a.H;
    }
    const uint32_t off = (uint32_t)(base + (v & ~15));
    if (k < 6)
      blds16(rsX, ok ? off : SSIP_OOB, Xs + (wave + NW * k) * 1024);
    else
      blds16(rsD, ok ? off : SSIP_OOB, Ds + (wave + NW * (k - 6)) * 1024);
  };

  // (zeroing and slab write-out stay spelled out here, not zero_acc / store_slab_frag: with those and a
  // shared form of issue_piece this kernel measured 122.1 us against 118.9 (range 116.3-120.6), bench layer 1)
  f32x4 acc[2][9];
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int b = 0; b < 9; ++b) acc[x][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
  // column block b of this wave: tap t = (9 wn + b) / 4, channels 16 ((9 wn + b) % 4) ..
  // Per-lane LDS byte offsets of the transposed fragment reads at k-step 0
  // (read_tfrag's rows r0 and r0 + 4): a k-step adds 32 rows = 4096 B and
  // leaves row bits 1 and 3 -- the swizzle's -- unchanged.
  int xo[9][2], dof[2][2];
  {
    const int tg = lane >> 4, ti = lane & 15, tq = ti >> 2, tp = ti & 3;
#pragma unroll
    for (int b = 0; b < 9; ++b) {
      const int nb = 9 * wn + b, t = nb >> 2;
      const int toff = (t / 3) * Wp + (t % 3), ccol = (nb & 3) * 16;
      xo[b][0] = MTile<__bf16, 64>::off(toff + 8 * tg + tq, ccol + 4 * tp);
      xo[b][1] = MTile<__bf16, 64>::off(toff + 8 * tg + tq + 4, ccol + 4 * tp);
    }
#pragma unroll
    for (int x = 0; x < 2; ++x) {
      dof[x][0] = MTile<__bf16, 64>::off(8 * tg + tq, (2 * wm + x) * 16 + 4 * tp);
      dof[x][1] = MTile<__bf16, 64>::off(8 * tg + tq + 4, (2 * wm + x) * 16 + 4 * tp);
    }
  }

  if (u0 < u1) issue(u0, smem0, smem0 + HWG_XBUF);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if constexpr (INBN) {
    if (u0 < u1) xform_x(u0, smem0);
  }
  auto run_tile = [&](int u, char* const Xs, char* const Xn) {
    char* const Ds = Xs + HWG_XBUF;
    halo_lds_barrier();
    // the next tile's pieces: two per wave after each of k-steps 0-4's MFMAs
    // (beside the matrix pipe instead of ahead of it, where both waves of a
    // SIMD issued theirs at once)
    const bool nxt = u + 1 < u1;
    const auto [nn, np0] = tile_row(u + 1, a.TR, a.H);
    const int nbase = (nn * a.H + np0) * a.W * 128;
    Frag<T> fa[2][2], fb[2][9];
    auto load_step = [&](int ks, Frag<T>(&ra)[2], Frag<T>(&rb)[9]) {
#pragma unroll
      for (int x = 0; x < 2; ++x) read_tfrag_at(ra[x], Ds + 4096 * ks + dof[x][0], Ds + 4096 * ks + dof[x][1]);
#pragma unroll
      for (int b = 0; b < 9; ++b) read_tfrag_at(rb[b], Xs + 4096 * ks + xo[b][0], Xs + 4096 * ks + xo[b][1]);
    };
    load_step(0, fa[0], fb[0]);
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      if (ks + 1 < 8) load_step(ks + 1, fa[(ks + 1) & 1], fb[(ks + 1) & 1]);
#pragma unroll
      for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int b = 0; b < 9; ++b) mma(acc[x][b], fa[ks & 1][x], fb[ks & 1][b]);
      if (ks < 5 && nxt) {
        issue_pc(2 * ks, nbase, np0, Xn, Xn + HWG_XBUF);
        issue_pc(2 * ks + 1, nbase, np0, Xn, Xn + HWG_XBUF);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the next tile's rows land before the barrier
    if constexpr (INBN) {
      if (nxt) xform_x(u + 1, Xn);
    }
  };
  for (int u = u0; u < u1; u += 2) {
    run_tile(u, smem0, smem1);
    if (u + 1 < u1) run_tile(u + 1, smem1, smem0);
  }
  // this workgroup's partial dW: slab[g][k][(t, c)]
  float* sl = a.slab + (long)g * 64 * 576;
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int b = 0; b < 9; ++b)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int k = (2 * wm + x) * 16 + 4 * (lane >> 4) + e;
        const int col = (9 * wn + b) * 16 + (lane & 15);
        sl[(long)k * 576 + col] = acc[x][b][e];
      }
}

}  // namespace

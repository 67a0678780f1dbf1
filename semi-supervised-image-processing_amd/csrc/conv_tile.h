// Conv device code shared by every kernel family: the kernel argument struct of the
// implicit-GEMM kernels, LDS tile layouts, MFMA fragments and their reads, global -> LDS
// staging primitives, barriers, and the per-wave BatchNorm statistics.
#pragma once
#include "ssip_common.h"

namespace {

enum { MODE_FWD = 0, MODE_DGRAD = 1, MODE_WGRAD = 2 };

struct FastDiv {  // n / d for 0 <= n < 2^31, 1 <= d < 2^31 (round-up multiplier)
  uint32_t d, mul, shr;
};
static FastDiv make_fastdiv(uint32_t d) {
  FastDiv f;
  f.d = d;
  if (d <= 1) { f.mul = 0; f.shr = 0; return f; }
  uint32_t l = 0;
  while ((1ull << l) < d) ++l;            // l = ceil(log2 d) >= 1
  const uint64_t p = 31 + l;
  f.mul = (uint32_t)(((1ull << p) + d - 1) / d);  // < 2^32
  f.shr = (uint32_t)(p - 32);
  return f;
}
__device__ __forceinline__ uint32_t fdiv(uint32_t n, const FastDiv& f) {
  return f.mul ? (__umulhi(n, f.mul) >> f.shr) : n;
}

struct PhaseInfo {
  int M, tiles_m, ksteps;     // rows (N * Hph * Wph), M-tiles, k-steps of this phase
  int r0, s0, nr, ns, bh, bw;  // first tap, tap counts, dy offsets
  int ph, pw, Wph;
  FastDiv div_hw, div_w;       // / (Hph * Wph), / Wph
};

struct ConvArgs {
  int N, H, W, C, K, R, S, stride, pad, P, Q;
  int M;        // GEMM rows (FWD: N*P*Q, DGRAD: N*H*W, WGRAD: K)
  int Ng;       // GEMM cols (FWD: K, DGRAD: C, WGRAD: R*S*C)
  int Kg;       // reduction length (FWD: R*S*C, DGRAD: R*S*K)
  int Mred;     // WGRAD: N*P*Q
  int ksteps;   // k steps per block (WGRAD: per split)
  int tiles_n;
  FastDiv div_pq, div_q, div_hw, div_w;
  const void* A;
  const void* B;
  void* out;
  const void* add;     // DGRAD: residual-gradient add; FWD: residual (ssip_conv_fwd_bias)
  float* partial;
  const float* bias;   // FWD: per-output-channel bias (a folded eval-mode BatchNorm), nullable
  int relu;            // FWD: ReLU on the output (after bias and residual)
  // DGRAD post-op (BN backward of the layer that produced this conv's input):
  // out = (dgrad + add) * relu_mask; per-(channel, tile) sums of out and
  // out * (py - pmean) * pinvstd into partial [Ng][tiles_m][2].  The ReLU
  // mask: pmask > 0 (z), else bit n & 7 of pbits[m * Ng / 8 + n / 8], else
  // fma(py, pmscale, pmshift) > 0 (the forward's sign for a BN+ReLU with no
  // residual).  Active when pmean != nullptr.
  const void* pmask;
  const uint8_t* pbits;
  const float* pmscale;
  const float* pmshift;
  const void* py;
  const float* pmean;
  const float* pinvstd;
  // DGRAD stride-2 phase split (LDS-DMA kernel): blockIdx.y = phase
  // (ph, pw) = output rows h = 2i+ph, columns w = 2j+pw; only the taps
  // r = r0 + 2*ri, s = s0 + 2*si reach them, at dy row p = i + bh - ri.
  int phased;
  PhaseInfo phase[4];
  // phase order (2 bits each, heaviest first): workgroup t of an XCD's
  // contiguous run takes phase (phase_order >> 2*(t & 3)) & 3 of tile t >> 2,
  // so every XCD gets the same mix of long and short phases
  int phase_order;
  // DGRAD of a stride-2 3x3 conv fused with its block's 1x1 / stride-2
  // downsample (ssip_conv_dgrad_ds): phase (0, 0) -- the only one the
  // downsample reaches, at the same dy pixel as its single tap -- runs
  // ds_from own k-steps, then K/64 more over dY_ds (A2) and W_ds [C][K] (B2)
  const void* A2;
  const void* B2;
  uint32_t a2_bytes, b2_bytes;
  int ds_from;
  int xcd_remap;  // 1: XCD-aware workgroup -> tile order (LDS-DMA kernel)
  int stagger;  // LDS-DMA ring: waves NW/2.. run each k-step's second MFMA half after the next barrier (SSIP_STAGGER)
  // INBN (LDS-DMA ring, FWD's A / WGRAD's B operand): the conv input is
  // relu(fma(y, in_scale[c], in_shift[c])) of the layer below, formed in place
  // in the ring after each wave's own pieces land (ssip_conv_*_bnrelu_in)
  const float* in_scale;
  const float* in_shift;
  // INBN FWD of a 1x1 / stride-1 conv (nullable): the n-tile-0 workgroups
  // also store each transformed piece to zout (same layout as A), so the
  // weight gradient takes relu(bn(y)) as a plain input
  void* zout;
  // FWD of a 3x3 / stride-s conv fused with its block's 1x1 / stride-s
  // downsample (ssip_conv_fwd_ds): workgroups >= fwd_tiles1 compute the
  // downsample's tiles -- its input pixel is the conv's tap (1, 1) pixel, so
  // they run only that tap's C/64 k-steps, with W_ds [K][C] as B -- into
  // out_ds / partial_ds.  0: no downsample.
  int fwd_tiles1;
  const void* Bds;
  void* out_ds;
  float* partial_ds;
  uint32_t bds_bytes;
  int stat_tiles_m;  // BN record tiles per channel when the grid is not tiles_m x tiles_n (0: from the grid)
  uint32_t a_bytes, b_bytes;  // operand extents (LDS-DMA kernel buffer resources)
  // WGRAD x-gather walk: a 64-row k-step advances each row's output pixel
  // (n, p, q) by (dn, dp, dq); its input byte offset by k0, plus e1 when q
  // wraps into the next row and e2 when p wraps into the next image
  int wg_dn, wg_dp, wg_dq, wg_k0, wg_e1, wg_e2;
};

template <typename T> struct Traits;
template <> struct Traits<__bf16> { static constexpr int BK = 64; };
template <> struct Traits<float> { static constexpr int BK = 32; };

// ---------------------------------------------------------------------------
// LDS addressing
// ---------------------------------------------------------------------------
// FWD/DGRAD tiles: [rows][128 B] (8 x 16-B slots).  slot' = slot ^ ((row>>1)&7)
// makes every 16-lane group of a ds_read_b128 fragment read (rows l&15,
// slot 4h + (l>>4) for bf16; slots 2(l>>4)+{0,1} for f32) hit 16 distinct
// 16-B bank slots.
__device__ __forceinline__ int ktile_off(int row, int slot) { return row * 128 + ((slot ^ ((row >> 1) & 7)) << 4); }

// WGRAD tiles: [BK m-rows][COLS elems], cols contiguous (as in HBM).
template <typename T, int COLS> struct MTile;
// 16-B chunk XOR of row `row` in a 64-column (128-B row) MTile: a transposed
// fragment read (read_mfrag / read_tfrag) touches rows r0 + {0..3, 8..11} in
// one 32-lane half, and two rows of equal parity share the 32 banks of one
// 128-B half-line -- so the four equal-parity rows need four different 32-B
// column groups for every r0.  Row bits 1 and 3 pick the group (the former
// row & 3 selector repeated every 8 rows: rows r and r + 8 collided, a 2-way
// conflict on every read, SQ_LDS_BANK_CONFLICT = 0.50 of the active LDS
// cycles of conv_halo_wgrad_kernel).
__device__ __forceinline__ int mt64_chunk_xor(int row) { return (((row >> 1) & 1) | (((row >> 3) & 1) << 1)) << 1; }

template <int COLS> struct MTile<__bf16, COLS> {
  static constexpr int ROW_BYTES = COLS * 2;
  static constexpr int UNITS = COLS / 4;  // 8-byte units per row
  __device__ static __forceinline__ int swz(int row) {
    if constexpr (COLS == 64) return mt64_chunk_xor(row) << 1;
    int h = (row & 3) | (((row >> 3) & 1) << 2);
    return (h * 4) & (UNITS - 1) & ~3;
  }
  __device__ static __forceinline__ int off(int row, int col) {  // col multiple of 4
    return row * ROW_BYTES + ((((col >> 2) ^ swz(row))) << 3);
  }
};
template <int COLS> struct MTile<float, COLS> {
  static constexpr int ROW_BYTES = COLS * 4 + 16;
  __device__ static __forceinline__ int off(int row, int col) { return row * ROW_BYTES + col * 4; }
};

// ---------------------------------------------------------------------------
// fragments and MFMA
// ---------------------------------------------------------------------------
template <typename T> struct Frag;
template <> struct Frag<__bf16> { bf16x8 v; };
template <> struct Frag<float> { float v[8]; };

__device__ __forceinline__ void mma(f32x4& acc, const Frag<__bf16>& a, const Frag<__bf16>& b) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.v, b.v, acc, 0, 0, 0);
}
__device__ __forceinline__ void mma(f32x4& acc, const Frag<float>& a, const Frag<float>& b) {
#pragma unroll
  for (int e = 0; e < 8; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.v[e], b.v[e], acc, 0, 0, 0);
}

// k-contiguous fragment for 32-deep sub-step h: lane holds row (l&15), k = 32h + 8(l>>4) .. +7
__device__ __forceinline__ void read_kfrag(Frag<__bf16>& f, const char* base, int row, int kq, int h) {
  f.v = *reinterpret_cast<const bf16x8*>(base + ktile_off(row, 4 * h + kq));
}
__device__ __forceinline__ void read_kfrag(Frag<float>& f, const char* base, int row, int kq, int) {
  const f32x4 lo = *reinterpret_cast<const f32x4*>(base + ktile_off(row, 2 * kq));
  const f32x4 hi = *reinterpret_cast<const f32x4*>(base + ktile_off(row, 2 * kq + 1));
  f.v[0] = lo[0]; f.v[1] = lo[1]; f.v[2] = lo[2]; f.v[3] = lo[3];
  f.v[4] = hi[0]; f.v[5] = hi[1]; f.v[6] = hi[2]; f.v[7] = hi[3];
}

// m-major fragment (WGRAD) for sub-step h: lane l gets column col0 + (l&15),
// m = 32h + 8(l>>4) .. +7
// The read pair of a transposed bf16 fragment (ds_read_b64_tr_b16): a0, a1 are
// the lane's addresses in m-rows r0 and r0 + 4 of an m-major image
__device__ __forceinline__ void read_tfrag_at(Frag<__bf16>& f, const char* a0, const char* a1) {
  typedef __attribute__((ext_vector_type(4))) __bf16 v4bf;
  v4bf lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) v4bf*)(a0));
  v4bf hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) v4bf*)(a1));
  f.v = (bf16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}
template <int COLS>
__device__ __forceinline__ void read_mfrag(Frag<__bf16>& f, const char* base, int col0, int lane, int h) {
  const int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3;
  const int r0 = 32 * h + 8 * g + q;
  read_tfrag_at(f, base + MTile<__bf16, COLS>::off(r0, col0 + 4 * p),
                base + MTile<__bf16, COLS>::off(r0 + 4, col0 + 4 * p));
}
template <int COLS>
__device__ __forceinline__ void read_mfrag(Frag<float>& f, const char* base, int col0, int lane, int h) {
  const int g = lane >> 4, col = col0 + (lane & 15);
#pragma unroll
  for (int j = 0; j < 8; ++j)
    f.v[j] = *reinterpret_cast<const float*>(base + MTile<float, COLS>::off(32 * h + 8 * g + j, col));
}

template <typename T>
__device__ __forceinline__ void load_v8(Vec8<T>& d, const T* p, bool ok) {
  if (ok) d.load(p); else d.zero();
}
// two padded pixels of 4 channels each (stem layout)
template <typename T>
__device__ __forceinline__ void load_2px(Vec8<T>& d, const T* p0, bool ok0, const T* p1, bool ok1);
template <>
__device__ __forceinline__ void load_2px<__bf16>(Vec8<__bf16>& d, const __bf16* p0, bool ok0, const __bf16* p1, bool ok1) {
  typedef __attribute__((ext_vector_type(2))) int i2;
  i2 a = ok0 ? *reinterpret_cast<const i2*>(p0) : (i2){0, 0};
  i2 b = ok1 ? *reinterpret_cast<const i2*>(p1) : (i2){0, 0};
  d.v = (i32x4){a[0], a[1], b[0], b[1]};
}
template <>
__device__ __forceinline__ void load_2px<float>(Vec8<float>& d, const float* p0, bool ok0, const float* p1, bool ok1) {
  d.v0 = ok0 ? *reinterpret_cast<const i32x4*>(p0) : (i32x4){0, 0, 0, 0};
  d.v1 = ok1 ? *reinterpret_cast<const i32x4*>(p1) : (i32x4){0, 0, 0, 0};
}

// 8-element chunk kc (0..KC-1) of a k-tile row
__device__ __forceinline__ void store_kchunk(char* base, int row, int kc, const Vec8<__bf16>& v) {
  *reinterpret_cast<i32x4*>(base + ktile_off(row, kc)) = v.v;
}
__device__ __forceinline__ void store_kchunk(char* base, int row, int kc, const Vec8<float>& v) {
  *reinterpret_cast<i32x4*>(base + ktile_off(row, 2 * kc)) = v.v0;
  *reinterpret_cast<i32x4*>(base + ktile_off(row, 2 * kc + 1)) = v.v1;
}
template <int COLS>
__device__ __forceinline__ void store_mchunk(char* base, int row, int col, const Vec8<__bf16>& v) {
  *reinterpret_cast<i32x4*>(base + MTile<__bf16, COLS>::off(row, col)) = v.v;
}
template <int COLS>
__device__ __forceinline__ void store_mchunk(char* base, int row, int col, const Vec8<float>& v) {
  *reinterpret_cast<i32x4*>(base + MTile<float, COLS>::off(row, col)) = v.v0;
  *reinterpret_cast<i32x4*>(base + MTile<float, COLS>::off(row, col + 4)) = v.v1;
}

// transposed (m-major) fragment of a [rows][64] bf16 MTile image: lane l gets
// column col0 + (l & 15), rows row0 + 8 (l >> 4) .. +7
__device__ __forceinline__ void read_tfrag(Frag<__bf16>& f, const char* base, int row0, int col0, int lane) {
  const int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3;
  const int r0 = row0 + 8 * g + q;
  read_tfrag_at(f, base + MTile<__bf16, 64>::off(r0, col0 + 4 * p),
                base + MTile<__bf16, 64>::off(r0 + 4, col0 + 4 * p));
}

// 16x16 accumulator fragment -> fp32 slab rows k0 + 4 (l >> 4) + e, column col0 + (l & 15)
__device__ __forceinline__ void store_slab_frag(float* slab, int pitch, int k0, int col0, const f32x4& acc, int lane) {
#pragma unroll
  for (int e = 0; e < 4; ++e) slab[(long)(k0 + 4 * (lane >> 4) + e) * pitch + col0 + (lane & 15)] = acc[e];
}

template <int A, int B>
__device__ __forceinline__ void zero_acc(f32x4 (&acc)[A][B]) {
#pragma unroll
  for (int i = 0; i < A; ++i)
#pragma unroll
    for (int j = 0; j < B; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
}

// Tile `tile` of TR whole rows, images H rows high: its image and first row
struct TileRow { int n, p0; };
__device__ __forceinline__ TileRow tile_row(int tile, int TR, int H) {
  const int R0 = tile * TR;
  const int n = R0 / H;
  return {n, R0 - n * H};
}

__device__ __attribute__((aligned(16))) int g_zero16[4];


__device__ __forceinline__ void glds16(const void* src, char* lds_block) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                   (__attribute__((address_space(3))) void*)lds_block, 16, 0, 0);
}

// Buffer-resource LDS-DMA: a raw buffer over the whole operand, per-lane
// 32-bit byte offsets.  An offset past the extent reads zeros (the padding /
// out-of-tile taps), so a gather step costs a mask test and one add per lane
// instead of 64-bit address arithmetic and a select against a zero page.
constexpr uint32_t SSIP_OOB = 0xFFFFFFF0u;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base, uint32_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ void blds16(__amdgpu_buffer_rsrc_t r, uint32_t voff, char* lds_block) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void*)lds_block, 16, voff, 0, 0, 0);
}

// relu(fma(v, scale, shift)) over the 8 channels c0 .. c0 + 7 of one LDS
// chunk, in place -- bn_apply_kernel's arithmetic exactly, so a conv over the
// transformed tile equals the conv of the materialised BN+ReLU output
__device__ __forceinline__ bf16x8 bnrelu8(bf16x8 v, const float (&sc)[8], const float (&sh)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float t = __builtin_fmaf((float)v[j], sc[j], sh[j]);
    t = t > 0.f ? t : 0.f;
    v[j] = (__bf16)t;
  }
  return v;
}
__device__ __forceinline__ void bnrelu_chunk(char* p, const float (&sc)[8], const float (&sh)[8]) {
  bf16x8 v = *reinterpret_cast<bf16x8*>(p);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float t = __builtin_fmaf((float)v[j], sc[j], sh[j]);
    t = t > 0.f ? t : 0.f;
    v[j] = (__bf16)t;
  }
  *reinterpret_cast<bf16x8*>(p) = v;
}

template <int N>
__device__ __forceinline__ void wait_vm_barrier() {
  asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(N) : "memory");
}
// the same with every LDS read of this wave retired first: with the stagger a
// lagging wave's second-half fragments are read before the barrier but used
// after it, and nothing else keeps those reads ahead of the next refill of
// their ring slot, which other waves issue right after the barrier
template <int N>
__device__ __forceinline__ void wait_vm_lgkm_barrier() {
  asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(N) : "memory");
}

// LDS-only workgroup barrier: __syncthreads() would also drain vmcnt, i.e.
// wait for the next tile's rows in flight and this tile's output stores
__device__ __forceinline__ void halo_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// ---------------------------------------------------------------------------
// tile bookkeeping of the persistent (halo / stem) kernels: a tile is whole
// output rows, its GEMM rows m = j * pitch + q the rows padded to `pitch`
// pixels, of which q < Q are output pixels and m < mrows belong to the tile
// ---------------------------------------------------------------------------
// This lane's output rows (rbase + 16 i + e): byte offset within a tile's
// [rows][Q][Ncols] bf16 output block at column cbase, and the validity mask
// (returned; bit 4 i + e), fixed for all tiles.  Discarded rows get an offset
// that stays out of range with + jj * 32 added.
template <int FM>
__device__ __forceinline__ uint32_t lane_out_rows(uint32_t (&rowoff)[FM][4], int rbase, int cbase, int pitch,
                                                  int mrows, int Q, int Ncols) {
  uint32_t vmask = 0;
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int m = rbase + i * 16 + e;
      const int j = m / pitch, q = m - j * pitch;
      const bool v = m < mrows && q < Q;
      rowoff[i][e] = v ? (uint32_t)(((j * Q + q) * Ncols + cbase) * 2) : 0x80000000u;
      vmask |= (v ? 1u : 0u) << (i * 4 + e);
    }
  return vmask;
}
// valid rows among GEMM rows r0 .. r0 + n - 1 (a wave's: uniform)
__device__ __forceinline__ int count_out_rows(int r0, int n, int pitch, int mrows, int Q) {
  int rows = 0;
  for (int r = r0; r < r0 + n; ++r) rows += (r < mrows && r % pitch < Q) ? 1 : 0;
  return rows;
}

// BN records per (channel, workgroup) of the halo / stem forwards: the wave rows of every
// conv_halo_kernel instantiation, or more
constexpr int HALO_WMW = 8;
// record (channel c, workgroup g of G, wave row wm) of [c][G][HALO_WMW][RV]
__device__ __forceinline__ float* bn_record(float* partial, int c, int G, int g, int wm, int RV) {
  return partial + ((long)c * G * HALO_WMW + (long)g * HALO_WMW + wm) * RV;
}
// zero workgroup g's records of every channel
template <int RV>
__device__ __forceinline__ void bn_records_zero(float* partial, int Ncols, int G, int g, int tid, int NT) {
  for (int c = tid; c < Ncols * HALO_WMW; c += NT) {
    float* rec = bn_record(partial, c / HALO_WMW, G, g, c % HALO_WMW, RV);
#pragma unroll
    for (int v = 0; v < RV; ++v) rec[v] = 0.f;
  }
}

// BatchNorm statistics of a wave's output rows over the tiles of a
// persistent workgroup: per lane (one column, the rows (l >> 4) * 4 + e of
// each 16x16 fragment) a count and sums shifted by the lane's first value;
// wave_merge turns them into {n, mean, M2} per column and combines the four
// lane groups in fixed order (Chan).  Deterministic.
template <int FM, int FN>
struct WaveStats {
  float n, k[FN], s1[FN], s2[FN];
  __device__ __forceinline__ void reset() {
    n = 0.f;
#pragma unroll
    for (int jj = 0; jj < FN; ++jj) k[jj] = s1[jj] = s2[jj] = 0.f;
  }
  __device__ __forceinline__ void tile(const f32x4 (&acc)[FM][FN], uint32_t vmask) {
    if (n == 0.f)
#pragma unroll
      for (int jj = 0; jj < FN; ++jj) k[jj] = acc[0][jj][0];
#pragma unroll
    for (int jj = 0; jj < FN; ++jj)
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float d = ((vmask >> (i * 4 + e)) & 1) ? acc[i][jj][e] - k[jj] : 0.f;
          s1[jj] += d;
          s2[jj] = __builtin_fmaf(d, d, s2[jj]);
        }
    n += (float)__builtin_popcount(vmask);
  }
  // tile() one row group at a time (i = 0 first): the same sums in the same order
  __device__ __forceinline__ void rows(const f32x4 (&acc)[FM][FN], uint32_t vmask, int i) {
    if (i == 0) {
      if (n == 0.f)
#pragma unroll
        for (int jj = 0; jj < FN; ++jj) k[jj] = acc[0][jj][0];
      n += (float)__builtin_popcount(vmask);
    }
#pragma unroll
    for (int jj = 0; jj < FN; ++jj)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float d = ((vmask >> (i * 4 + e)) & 1) ? acc[i][jj][e] - k[jj] : 0.f;
        s1[jj] += d;
        s2[jj] = __builtin_fmaf(d, d, s2[jj]);
      }
  }
  __device__ __forceinline__ void wave_merge(float& nw, float (&mean)[FN], float (&m2)[FN]) const {
    nw = n;
#pragma unroll
    for (int jj = 0; jj < FN; ++jj) {
      mean[jj] = n > 0.f ? k[jj] + s1[jj] / n : 0.f;
      m2[jj] = n > 0.f ? fmaxf(s2[jj] - s1[jj] * s1[jj] / n, 0.f) : 0.f;
    }
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {
      const float nb = __shfl_xor(nw, off, 64);
      const float nn = nw + nb;
#pragma unroll
      for (int jj = 0; jj < FN; ++jj) {
        const float mb = __shfl_xor(mean[jj], off, 64), qb = __shfl_xor(m2[jj], off, 64);
        // combine in a fixed order (lower lane group first) so every lane gets the same bits
        const bool lo = (threadIdx.x & off) == 0;
        const float na_ = lo ? nw : nb, ma = lo ? mean[jj] : mb, qa = lo ? m2[jj] : qb;
        const float nb_ = lo ? nb : nw, mb_ = lo ? mb : mean[jj], qb_ = lo ? qb : m2[jj];
        const float d = mb_ - ma;
        mean[jj] = nn > 0.f ? ma + d * (nb_ / nn) : 0.f;
        m2[jj] = nn > 0.f ? qa + qb_ + d * d * (na_ * nb_ / nn) : 0.f;
      }
      nw = nn;
    }
  }
  // panel / range end: the wave's sums -> records [c][g][wm] of its columns
  // c0 + 16 jj (lanes < 16 write), and start over
  __device__ __forceinline__ void flush(float* partial, int c0, int G, int g, int wm, int lane) {
    float nw, mean[FN], m2[FN];
    wave_merge(nw, mean, m2);
    if (lane < 16) {
#pragma unroll
      for (int jj = 0; jj < FN; ++jj) {
        float* rec = bn_record(partial, c0 + jj * 16, G, g, wm, 3);
        rec[0] = nw;
        rec[1] = mean[jj] * nw;
        rec[2] = m2[jj];
      }
    }
    reset();
  }
};

}  // namespace

#pragma once
#include "conv_epilogue.h"

namespace {

// ---------------------------------------------------------------------------
// bf16 fast path: LDS-DMA (global_load_lds_dwordx4) 3-stage ring.
// Each wave-instruction moves 64 x 16 B = 1 KiB straight into LDS (no VGPR
// staging, no ds_write); the XOR swizzle is applied to the per-lane SOURCE
// chunk so the LDS image is the same one the register-staged kernel builds.
// Padded / out-of-range taps read a 16-byte zero block.  Prefetch distance
// 2: the loop waits with a counted vmcnt (one stage left in flight) and a
// raw s_barrier, never vmcnt(0) until the last step.
// ---------------------------------------------------------------------------

// Waves per SIMD the LDS budget allows; asking the compiler for that many
// keeps the register count from costing a resident workgroup.
constexpr int glds_min_waves(int bm, int bn, int nw, int nstage, bool wg) {
  const int stage = wg ? 64 * (bm + bn) * 2 : (bm + bn) * 128;
  const int blocks = 163840 / (nstage * stage);
  const int w = blocks * nw / 4;
  return w < 1 ? 1 : (w > 8 ? 8 : w);
}

// C4: the stem conv on a pre-padded 4-channel image (pad 0, S padded to 8,
// even W): a 16-B chunk is a pixel pair (s, s+1) of one filter row, so a
// 64-deep k-step covers filter rows 2ks and 2ks+1; k >= R*S*4 reads zeros.
// POST: DGRAD with the BN-backward epilogue (ssip_conv_dgrad_bn); its
// operand registers are only allocated in that instantiation.
// (Round 3's timing ablations of this k-loop, its 5- and 8-phase ping-pong
// schedules and the persistent row-balanced halo kernel conv_hb -- all
// measured no faster in the step -- live on the r3-variants branch.)
// INBN: FWD / WGRAD over relu(bn(y)) of the layer below (ConvArgs::in_scale),
// the transform applied to each wave's own landed pieces before the k-step's
// barrier (2-stage ring; input channels <= GLDS_INBN_C).
constexpr int GLDS_INBN_C = 512;
template <int MODE, int BM, int BN, int WMW, int WNW, int NSTAGE, bool C4 = false, bool POST = false,
          bool FOLD = false, bool INBN = false>
__global__ void __launch_bounds__(64 * WMW * WNW, glds_min_waves(BM, BN, WMW * WNW, NSTAGE, MODE == 2))
    conv_glds_kernel(const ConvArgs a) {
  typedef __bf16 T;
  constexpr int NW = WMW * WNW, BK = 64;
  constexpr int WTM = BM / WMW, WTN = BN / WNW;
  constexpr int FM = WTM / 16, FN = WTN / 16;
  constexpr bool WG = (MODE == MODE_WGRAD);
  constexpr int A_BYTES = WG ? BK * BM * 2 : BM * 128;
  constexpr int B_BYTES = WG ? BK * BN * 2 : BN * 128;
  constexpr int STAGE = A_BYTES + B_BYTES;
  static_assert(NSTAGE == 2 || NSTAGE == 3, "2 or 3 LDS stages");
  constexpr int NBUF = NSTAGE;
  constexpr int IA = A_BYTES / 1024, IB = B_BYTES / 1024;
  constexpr int LA = IA / NW, LB = IB / NW;
  constexpr int L = LA + LB;
  static_assert(IA % NW == 0 && IB % NW == 0 && LA >= 1 && LB >= 1, "bad glds tile");
  static_assert(FM >= 1 && FN >= 1, "bad wave tile");
  constexpr int EPI = WG ? 0 : BM * (BN * 2 + 16);
  constexpr int SMEM = (NBUF * STAGE > EPI) ? NBUF * STAGE : EPI;
  static_assert(!INBN || (NSTAGE == 2 && !C4 && !POST && !FOLD && MODE != MODE_DGRAD), "INBN: FWD / WGRAD, 2 stages");
  __shared__ __attribute__((aligned(16))) char smem[SMEM + (INBN ? 2 * GLDS_INBN_C * 4 : 0)];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WNW, wn = wave % WNW;
  // XCD-aware order: the hardware deals workgroups round-robin to the 8 XCDs
  // (each with its own L2); remap so every XCD owns a contiguous run of
  // tiles (same split/phase, neighbouring M-tiles sharing im2col rows and the
  // whole weight panel) instead of every 8th tile.
  int bx, by;
  bool ds = false;  // FWD: a fused downsample tile (ConvArgs::fwd_tiles1)
  {
    const int nb = gridDim.x * gridDim.y;
    const int lin = blockIdx.x + blockIdx.y * gridDim.x;
    const int xcd = lin & 7, q = nb >> 3, r = nb & 7;
    const int t = a.xcd_remap ? xcd * q + min(xcd, r) + (lin >> 3) : lin;
    if (MODE == MODE_DGRAD && a.phased) {  // gridDim.y == 4: all phases of a tile together, heaviest first
      bx = t >> 2;
      by = (a.phase_order >> (2 * (t & 3))) & 3;
    } else {
      bx = t % gridDim.x;
      by = t / gridDim.x;
    }
    if (MODE == MODE_FWD && a.fwd_tiles1 > 0) {
      // fused downsample: the conv's tiles first in dispatch order, then the
      // short downsample tiles (they fill the last round), each group remapped
      // XCD-contiguously on its own
      ds = lin >= a.fwd_tiles1;
      const int base = ds ? a.fwd_tiles1 : 0, cnt = ds ? nb - a.fwd_tiles1 : a.fwd_tiles1;
      const int l = lin - base, x8 = l & 7, q8 = cnt >> 3, r8 = cnt & 7;
      bx = a.xcd_remap ? x8 * q8 + min(x8, r8) + (l >> 3) : l;
      by = 0;
    }
  }
  const int tn = bx % a.tiles_n;
  const int tm = bx / a.tiles_n;
  const int m0 = tm * BM, n0 = tn * BN;
  const T* __restrict__ Ag = static_cast<const T*>(a.A);
  const T* __restrict__ Bg = static_cast<const T*>(a.B);
  // stride-2 DGRAD phase (uniform per workgroup); surplus M-tiles of the
  // shorter phases leave before touching memory or a barrier
  // (field-wise constant-index selects: a dynamic index into the kernel
  // argument struct, or a pointer into a copy, lands it in scratch)
  const bool phased = (MODE == MODE_DGRAD) && a.phased;
  const int f = phased ? by : 0;
#define SSIP_PSEL(fld) \
  (f == 0 ? a.phase[0].fld : f == 1 ? a.phase[1].fld : f == 2 ? a.phase[2].fld : a.phase[3].fld)
  RowMap rmap;
  rmap.phased = phased;
  rmap.H = a.H;
  rmap.W = a.W;
  int ph_nr = a.R, ph_ns = a.S, ph_r0 = 0, ph_s0 = 0, ph_bh = 0, ph_bw = 0,
      ph_ksteps = (MODE == MODE_FWD && ds) ? a.C / 64 : a.ksteps;
  if (phased) {
    if (tm >= SSIP_PSEL(tiles_m)) return;
    // a phase no tap reaches (1x1 stride-2 dgrad: 3 of 4) adds nothing: with
    // the residual gradient accumulated in place there is nothing to write
    if (!POST && SSIP_PSEL(ksteps) == 0 && a.add == a.out) return;
    rmap.M = SSIP_PSEL(M);
    rmap.ph = SSIP_PSEL(ph);
    rmap.pw = SSIP_PSEL(pw);
    rmap.Wph = SSIP_PSEL(Wph);
    rmap.div_hw.d = SSIP_PSEL(div_hw.d);
    rmap.div_hw.mul = SSIP_PSEL(div_hw.mul);
    rmap.div_hw.shr = SSIP_PSEL(div_hw.shr);
    rmap.div_w.d = SSIP_PSEL(div_w.d);
    rmap.div_w.mul = SSIP_PSEL(div_w.mul);
    rmap.div_w.shr = SSIP_PSEL(div_w.shr);
    ph_nr = SSIP_PSEL(nr);
    ph_ns = SSIP_PSEL(ns);
    ph_r0 = SSIP_PSEL(r0);
    ph_s0 = SSIP_PSEL(s0);
    ph_bh = SSIP_PSEL(bh);
    ph_bw = SSIP_PSEL(bw);
    ph_ksteps = SSIP_PSEL(ksteps);
  } else {
    rmap.M = a.M;
  }
#undef SSIP_PSEL
  const int Mrows = rmap.M;

  // ---------------- per-lane source state ----------------
  // FWD/DGRAD: instruction j = wave + NW*t covers k-tile rows 8j..8j+7;
  //   lane -> row 8j + lane/8, LDS slot lane%8 holds logical chunk (lane%8) ^ ((row>>1)&7)
  // WGRAD: rows of CPR = cols/8 chunks; instruction j covers 64/CPR rows.
  int a_base[LA], a_h[LA], a_w[LA], a_c[LA];
  bool a_ok[LA];
  const T* b_ptr[LB];
  int b_r[LB], b_s[LB], b_c[LB], b_row[LB];
  bool b_ok[LB];
  int kr = 0, ks_ = 0, kcb = 0;
  if (MODE == MODE_FWD && ds) { kr = 1; ks_ = 1; }  // the downsample's pixel is the conv's tap (1, 1)
  const int Cred = (MODE == MODE_FWD) ? a.C : a.K;
  long mstart = 0, mend = 0;

  if constexpr (!WG) {
#pragma unroll
    for (int t = 0; t < LA; ++t) {
      const int row = 8 * (wave + NW * t) + (lane >> 3);
      a_c[t] = (lane & 7) ^ ((row >> 1) & 7);
      const int m = m0 + row;
      a_ok[t] = m < Mrows;
      const int mm = a_ok[t] ? m : 0;
      if constexpr (MODE == MODE_FWD) {
        const int n = fdiv(mm, a.div_pq);
        const int rem = mm - n * a.P * a.Q;
        const int p = fdiv(rem, a.div_q);
        const int q = rem - p * a.Q;
        a_base[t] = n * a.H * a.W;
        a_h[t] = p * a.stride - a.pad;
        a_w[t] = q * a.stride - a.pad;
      } else if (phased) {
        const int n = fdiv(mm, rmap.div_hw);
        const int rem = mm - n * (int)rmap.div_hw.d;
        const int i = fdiv(rem, rmap.div_w);
        const int j = rem - i * rmap.Wph;
        a_base[t] = n * a.P * a.Q;
        a_h[t] = i + ph_bh;  // dy row for tap ri: a_h - ri
        a_w[t] = j + ph_bw;
      } else {
        const int n = fdiv(mm, a.div_hw);
        const int rem = mm - n * a.H * a.W;
        const int h = fdiv(rem, a.div_w);
        const int w = rem - h * a.W;
        a_base[t] = n * a.P * a.Q;
        a_h[t] = h + a.pad;
        a_w[t] = w + a.pad;
      }
    }
#pragma unroll
    for (int t = 0; t < LB; ++t) {
      const int row = 8 * (wave + NW * t) + (lane >> 3);
      const int c = (lane & 7) ^ ((row >> 1) & 7);
      const int n = n0 + row;
      b_ok[t] = n < a.Ng;
      b_c[t] = c;
      b_ptr[t] = Bg + (long)(b_ok[t] ? n : 0) * a.Kg + c * 8;
    }
  } else {
    mstart = (long)by * a.ksteps * BK;
    mend = mstart + (long)a.ksteps * BK;
    if (mend > a.Mred) mend = a.Mred;
    constexpr int CPA = BM / 8, RPA = 64 / CPA;
    constexpr int CPB = BN / 8, RPB = 64 / CPB;
#pragma unroll
    for (int t = 0; t < LA; ++t) {
      const int row = RPA * (wave + NW * t) + lane / CPA;
      const int lc = (lane % CPA) ^ (MTile<T, BM>::swz(row) >> 1);
      a_h[t] = row;                       // m-row within the k-step
      a_c[t] = m0 + lc * 8;               // output-channel column
      a_ok[t] = a_c[t] < a.K;
    }
#pragma unroll
    for (int t = 0; t < LB; ++t) {
      const int row = RPB * (wave + NW * t) + lane / CPB;
      const int lc = (lane % CPB) ^ (MTile<T, BN>::swz(row) >> 1);
      const int col = n0 + lc * 8;
      b_row[t] = row;
      b_ok[t] = col < a.Ng;
      const int cc = b_ok[t] ? col : 0;
      const int rs = cc / a.C;
      b_c[t] = cc - rs * a.C;
      b_r[t] = rs / a.S;
      b_s[t] = rs - b_r[t] * a.S;
    }
  }

  // buffer-resource state (FWD except the stem, DGRAD stride 1 / phase-split,
  // WGRAD's dY operand): byte offset of the lane's chunk at tap 0 and the
  // taps (bit r*S + s) whose source pixel lies inside the image.
  constexpr bool BUF_A = !C4;
  uint32_t a_off[LA], a_msk[LA], b_off[LB];
  __amdgpu_buffer_rsrc_t rsA = make_rsrc(Ag, a.a_bytes),
                         rsB = (MODE == MODE_FWD && ds) ? make_rsrc(a.Bds, a.bds_bytes) : make_rsrc(Bg, a.b_bytes);
  const int b_stride = (MODE == MODE_FWD && ds) ? a.C : a.Kg;  // B row length (W_ds: [K][C])
  const bool dsx = (MODE == MODE_DGRAD) && phased && f == 0 && a.A2 != nullptr;
  if constexpr (!WG && BUF_A) {
    const int nr = phased ? ph_nr : a.R, ns = phased ? ph_ns : a.S;
#pragma unroll
    for (int t = 0; t < LA; ++t) {
      // valid taps: rows [lr, hr) x columns [ls, hs) of the (nr x ns) filter
      int lr, hr, ls, hs;
      long pix;
      if constexpr (MODE == MODE_FWD) {  // input pixel (a_h + r, a_w + s)
        lr = max(0, -a_h[t]); hr = min(nr, a.H - a_h[t]);
        ls = max(0, -a_w[t]); hs = min(ns, a.W - a_w[t]);
        pix = (long)a_base[t] + (long)a_h[t] * a.W + a_w[t];
        a_off[t] = (uint32_t)((pix * a.C + a_c[t] * 8) * 2);
      } else {  // dY pixel (a_h - r, a_w - s)
        lr = max(0, a_h[t] - a.P + 1); hr = min(nr, a_h[t] + 1);
        ls = max(0, a_w[t] - a.Q + 1); hs = min(ns, a_w[t] + 1);
        pix = (long)a_base[t] + (long)a_h[t] * a.Q + a_w[t];
        a_off[t] = (uint32_t)((pix * a.K + a_c[t] * 8) * 2);
      }
      const uint32_t cbits = hs > ls ? ((1u << hs) - 1u) & ~((1u << ls) - 1u) : 0u;
      uint32_t msk = 0;
      for (int r = 0; r < nr; ++r) msk |= (r >= lr && r < hr) ? cbits << (r * ns) : 0u;
      a_msk[t] = a_ok[t] ? msk : 0u;
    }
#pragma unroll
    for (int t = 0; t < LB; ++t) {
      const int row = 8 * (wave + NW * t) + (lane >> 3);
      b_off[t] = b_ok[t] ? (uint32_t)(((long)(n0 + row) * b_stride + b_c[t] * 8) * 2) : 0xF0000000u;
    }
  } else if constexpr (WG) {
#pragma unroll
    for (int t = 0; t < LA; ++t) a_off[t] = (uint32_t)(((mstart + a_h[t]) * a.K + a_c[t]) * 2);
  }
  // WGRAD x gather: per slot the output pixel (p, q) of its row, the byte
  // offset of its tap's input pixel (+ channel chunk), and the p / q ranges
  // for which that tap lies inside the image (fixed: the slot's tap is fixed)
  int w_p[LB], w_q[LB], w_plo[LB], w_pn[LB], w_qlo[LB], w_qn[LB];
  uint32_t w_pix[LB];
  if constexpr (WG) {
#pragma unroll
    for (int t = 0; t < LB; ++t) {
      const int m = (int)min(mstart + b_row[t], (long)a.Mred - 1);
      const int n = fdiv(m, a.div_pq);
      const int rem = m - n * a.P * a.Q;
      const int pp = fdiv(rem, a.div_q);
      const int qq = rem - pp * a.Q;
      w_p[t] = pp;
      w_q[t] = qq;
      const int hin = pp * a.stride - a.pad + b_r[t], win = qq * a.stride - a.pad + b_s[t];
      w_pix[t] = (uint32_t)(((((long)n * a.H + hin) * a.W + win) * a.C + b_c[t]) * 2);
      // hin = p*stride - pad + r in [0, H)  <=>  p in [plo, plo + pn)
      const int r0 = a.pad - b_r[t], s0 = a.pad - b_s[t];
      const int plo = r0 > 0 ? (r0 + a.stride - 1) / a.stride : 0;
      const int phi = min(a.P, (a.H - 1 + r0) >= 0 ? (a.H - 1 + r0) / a.stride + 1 : 0);
      const int qlo = s0 > 0 ? (s0 + a.stride - 1) / a.stride : 0;
      const int qhi = min(a.Q, (a.W - 1 + s0) >= 0 ? (a.W - 1 + s0) / a.stride + 1 : 0);
      w_plo[t] = plo;
      w_pn[t] = b_ok[t] ? max(0, phi - plo) : 0;
      w_qlo[t] = qlo;
      w_qn[t] = max(0, qhi - qlo);
    }
  }

  // INBN: per ring stage, which of this wave's pieces read real input (bit t;
  // padding taps, rows past the grid and split tails stay zero) and, FWD, the
  // channel offset of the k-step
  uint32_t inb_v0 = 0, inb_v1 = 0;
  int inb_k0 = 0, inb_k1 = 0;
  auto issue = [&](int ks, int stage) {
    char* As = smem + stage * STAGE;
    char* Bs = As + A_BYTES;
    uint32_t inb_v = 0;
    if constexpr (MODE == MODE_FWD && C4) {
#pragma unroll
      for (int t = 0; t < LA; ++t) {
        const int k = ks * BK + a_c[t] * 8;
        const int hin = a_h[t] + 2 * ks + (a_c[t] >> 2), win = a_w[t] + 2 * (a_c[t] & 3);
        const bool ok = a_ok[t] && k < a.Kg && hin >= 0 && hin < a.H && win >= 0 && win + 1 < a.W;
        const T* src = ok ? Ag + ((long)(a_base[t] + hin * a.W + win)) * 4
                          : reinterpret_cast<const T*>(g_zero16);
        glds16(src, As + (wave + NW * t) * 1024);
      }
    } else if constexpr (MODE == MODE_FWD) {
      const int tp = kr * a.S + ks_;
      const uint32_t toff = (uint32_t)(((kr * a.W + ks_) * a.C + kcb) * 2);
#pragma unroll
      for (int t = 0; t < LA; ++t) {
        const bool ok = (a_msk[t] >> tp) & 1u;
        blds16(rsA, ok ? a_off[t] + toff : SSIP_OOB, As + (wave + NW * t) * 1024);
        if constexpr (INBN) inb_v |= (ok ? 1u : 0u) << t;
      }
      if constexpr (INBN) {
        if (stage == 0) { inb_v0 = inb_v; inb_k0 = kcb; } else { inb_v1 = inb_v; inb_k1 = kcb; }
      }
    } else if constexpr (MODE == MODE_DGRAD) {
      if (dsx && ks == a.ds_from) {
        // switch to the fused downsample: its dY_ds pixel is this phase's tap-0
        // pixel (same a_off / mask bit 0), its weights are [C][K]
        rsA = make_rsrc(a.A2, a.a2_bytes);
        rsB = make_rsrc(a.B2, a.b2_bytes);
#pragma unroll
        for (int t = 0; t < LB; ++t) {
          const int row = 8 * (wave + NW * t) + (lane >> 3);
          b_off[t] = b_ok[t] ? (uint32_t)(((long)(n0 + row) * a.K + b_c[t] * 8) * 2) : 0xF0000000u;
        }
        kr = 0; ks_ = 0; kcb = 0; ph_r0 = 0; ph_s0 = 0; ph_ns = 1;
      }
      const int tp = kr * ph_ns + ks_;
      const uint32_t toff = (uint32_t)((kcb - (kr * a.Q + ks_) * a.K) * 2);
#pragma unroll
      for (int t = 0; t < LA; ++t) {
        const bool ok = (a_msk[t] >> tp) & 1u;
        blds16(rsA, ok ? a_off[t] + toff : SSIP_OOB, As + (wave + NW * t) * 1024);
      }
    }
    if constexpr (!WG) {
#pragma unroll
      for (int t = 0; t < LB; ++t) {
        int koff = ks * BK;
        if constexpr (MODE == MODE_DGRAD) {
          if (phased) koff = ((ph_r0 + 2 * kr) * a.S + ph_s0 + 2 * ks_) * a.K + kcb;
        }
        if constexpr (BUF_A) {
          blds16(rsB, b_off[t] + (uint32_t)(koff * 2), Bs + (wave + NW * t) * 1024);
        } else {
          bool ok = b_ok[t];
          if constexpr (C4) ok = ok && ks * BK + b_c[t] * 8 < a.Kg;
          const T* src = ok ? b_ptr[t] + koff : reinterpret_cast<const T*>(g_zero16);
          glds16(src, Bs + (wave + NW * t) * 1024);
        }
      }
    } else {
      const int mlim = (int)(mend - mstart) - ks * BK;  // rows of this k-step inside the split
      const uint32_t moff = (uint32_t)(ks * BK * a.K * 2);
#pragma unroll
      for (int t = 0; t < LA; ++t) {
        const bool ok = a_ok[t] && a_h[t] < mlim;
        blds16(rsA, ok ? a_off[t] + moff : SSIP_OOB, As + (wave + NW * t) * 1024);
      }
#pragma unroll
      for (int t = 0; t < LB; ++t) {
        const bool ok = b_row[t] < mlim && (uint32_t)(w_p[t] - w_plo[t]) < (uint32_t)w_pn[t] &&
                        (uint32_t)(w_q[t] - w_qlo[t]) < (uint32_t)w_qn[t];
        blds16(rsB, ok ? w_pix[t] : SSIP_OOB, Bs + (wave + NW * t) * 1024);
        if constexpr (INBN) inb_v |= (ok ? 1u : 0u) << t;
        // advance the slot's row by the 64 rows of a k-step
        int q = w_q[t] + a.wg_dq;
        const bool c1 = q >= a.Q;
        q = c1 ? q - a.Q : q;
        int pp = w_p[t] + a.wg_dp + (c1 ? 1 : 0);
        const bool c2 = pp >= a.P;
        pp = c2 ? pp - a.P : pp;
        w_q[t] = q;
        w_p[t] = pp;
        w_pix[t] += (uint32_t)(a.wg_k0 + (c1 ? a.wg_e1 : 0) + (c2 ? a.wg_e2 : 0));
      }
      if constexpr (INBN) {
        if (stage == 0) inb_v0 = inb_v; else inb_v1 = inb_v;
      }
    }
    if constexpr (!WG) {
      kcb += BK;
      if (kcb >= Cred) {
        kcb = 0;
        if (++ks_ >= ph_ns) { ks_ = 0; ++kr; }
      }
    }
  };

  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  int nsteps = ph_ksteps;
  if constexpr (WG) {
    const long rem = mend - mstart;
    nsteps = rem > 0 ? (int)((rem + BK - 1) / BK) : 0;
  }
  // NSTAGE-deep ring, NSTAGE-1 k-steps in flight.  Step ks: retire stage ks
  // with a counted vmcnt (the later in-flight steps stay outstanding across
  // the raw barrier), then refill the slot every wave finished reading in
  // step ks-1.
  // fused-BN epilogue operands: issued first, landed long before the epilogue
  BnPostRegs<T, BM, BN, 64 * WMW * WNW> post;
  if constexpr (MODE == MODE_DGRAD && POST) post.load(a, m0, n0);
  float* const inb_sc = reinterpret_cast<float*>(smem + SMEM);
  float* const inb_sh = inb_sc + GLDS_INBN_C;
  // INBN FWD z_out (1x1 / stride 1: a piece's byte offset at tap 0 + the
  // k-step's channel offset is its input offset, so z has A's layout); only
  // the n-tile-0 workgroups store (every n-tile reads the same pieces)
  const bool zst = INBN && MODE == MODE_FWD && a.zout != nullptr && tn == 0;
  const __amdgpu_buffer_rsrc_t rsZ = make_rsrc(zst ? a.zout : nullptr, zst ? a.a_bytes : 0);
  if constexpr (INBN) {
    for (int c = tid; c < a.C; c += 64 * NW) {
      inb_sc[c] = a.in_scale[c];
      inb_sh[c] = a.in_shift[c];
    }
    __syncthreads();
  }
  // INBN: this wave's landed pieces of `stage` become relu(fma(y, scale, shift))
  // in place (bn_apply_kernel's arithmetic: fp32 fma, ReLU, one bf16 rounding),
  // so the k-step's fragment reads see the conv input itself
  auto inbn_xform = [&](int stage) {
    if constexpr (INBN) {
      const uint32_t vb = stage == 0 ? inb_v0 : inb_v1;
      char* const base = smem + stage * STAGE + (WG ? A_BYTES : 0);
      constexpr int LP = WG ? LB : LA;
#pragma unroll
      for (int t = 0; t < LP; ++t) {
        if ((vb >> t) & 1u) {
          int c0;
          if constexpr (WG) c0 = b_c[t];
          else c0 = (stage == 0 ? inb_k0 : inb_k1) + a_c[t] * 8;
          const f32x4 s0 = *reinterpret_cast<const f32x4*>(inb_sc + c0);
          const f32x4 s1 = *reinterpret_cast<const f32x4*>(inb_sc + c0 + 4);
          const f32x4 h0 = *reinterpret_cast<const f32x4*>(inb_sh + c0);
          const f32x4 h1 = *reinterpret_cast<const f32x4*>(inb_sh + c0 + 4);
          const float sc8[8] = {s0[0], s0[1], s0[2], s0[3], s1[0], s1[1], s1[2], s1[3]};
          const float sh8[8] = {h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
          bnrelu_chunk(base + (wave + NW * t) * 1024 + lane * 16, sc8, sh8);
          if constexpr (!WG) {
            if (zst) {
              typedef __attribute__((ext_vector_type(4))) unsigned int zv4u;
              const zv4u v = *reinterpret_cast<const zv4u*>(base + (wave + NW * t) * 1024 + lane * 16);
              __builtin_amdgcn_raw_buffer_store_b128(
                  v, rsZ, a_off[t] + (uint32_t)((stage == 0 ? inb_k0 : inb_k1) * 2), 0, 0);
            }
          }
        }
      }
    }
  };
  if (nsteps > 0) issue(0, 0);
  if (NSTAGE == 3 && nsteps > 1) issue(1, 1);
  int stage = 0;
  Frag<T> fa[2][FM], fb[2][FN];
  // Stagger (MI355X_MICROARCH "two waves per SIMD" item 9): waves w and
  // w + NW/2 share a SIMD and run this loop in lockstep -- both issue their
  // LDS-DMA pieces and fragment reads right after the barrier with the SIMD's
  // matrix pipe idle, then both multiply (round 3's ablation: the DMA and MFMA
  // phases add).  The second half of the workgroup runs each k-step's second
  // MFMA half after the next barrier instead, from fragments it already holds
  // in registers, so its matrix work fills the interval in which its partner
  // issues the ring refill and reads.  LDS is untouched by the deferred half;
  // the accumulation order h0(ks), h1(ks), h0(ks+1), ... is unchanged, so the
  // results are the same bits.
  const bool lag = a.stagger != 0 && wave >= NW / 2;
  for (int ks = 0; ks < nsteps; ++ks) {
    bool deferred = lag && ks > 0;
    if constexpr (INBN) {
      // own pieces landed -> transform them -> publish (LDS writes, barrier);
      // the lagging half's deferred MFMAs (registers only) go first, beside
      // the leading half's transform
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (deferred) {
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
          for (int j = 0; j < FN; ++j) mma(acc[i][j], fa[1][i], fb[1][j]);
        deferred = false;
      }
      inbn_xform(stage);
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    } else if (a.stagger) {
      if (NSTAGE == 3 && ks + 1 < nsteps) wait_vm_lgkm_barrier<L>(); else wait_vm_lgkm_barrier<0>();
    } else if (NSTAGE == 3 && ks + 1 < nsteps) {
      wait_vm_barrier<L>();
    } else {
      wait_vm_barrier<0>();
    }
    if (deferred) {
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) mma(acc[i][j], fa[1][i], fb[1][j]);
    }
    const bool refill = ks + NSTAGE - 1 < nsteps;
    if (refill) issue(ks + NSTAGE - 1, stage == 0 ? NSTAGE - 1 : stage - 1);
    const char* As = smem + stage * STAGE;
    const char* Bs = As + A_BYTES;
    // both k-halves' fragments are requested before the first MFMA, so the
    // second half's LDS reads overlap the first half's matrix work
    // (wave tiles of more than 8 fragments read one k-half at a time)
    constexpr bool BOTH = FM + FN <= 8;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (!BOTH && h == 1) break;
      if constexpr (!WG) {
#pragma unroll
        for (int i = 0; i < FM; ++i) read_kfrag(fa[h][i], As, wm * WTM + i * 16 + (lane & 15), lane >> 4, h);
#pragma unroll
        for (int j = 0; j < FN; ++j) read_kfrag(fb[h][j], Bs, wn * WTN + j * 16 + (lane & 15), lane >> 4, h);
      } else {
#pragma unroll
        for (int i = 0; i < FM; ++i) read_mfrag<BM>(fa[h][i], As, wm * WTM + i * 16, lane, h);
#pragma unroll
        for (int j = 0; j < FN; ++j) read_mfrag<BN>(fb[h][j], Bs, wn * WTN + j * 16, lane, h);
      }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (!BOTH && h == 1) {
        if constexpr (!WG) {
#pragma unroll
          for (int i = 0; i < FM; ++i) read_kfrag(fa[1][i], As, wm * WTM + i * 16 + (lane & 15), lane >> 4, 1);
#pragma unroll
          for (int j = 0; j < FN; ++j) read_kfrag(fb[1][j], Bs, wn * WTN + j * 16 + (lane & 15), lane >> 4, 1);
        } else {
#pragma unroll
          for (int i = 0; i < FM; ++i) read_mfrag<BM>(fa[1][i], As, wm * WTM + i * 16, lane, 1);
#pragma unroll
          for (int j = 0; j < FN; ++j) read_mfrag<BN>(fb[1][j], Bs, wn * WTN + j * 16, lane, 1);
        }
      }
      if (h == 1 && lag) break;  // deferred past the next barrier
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) mma(acc[i][j], fa[h][i], fb[h][j]);
    }
    stage = stage == NSTAGE - 1 ? 0 : stage + 1;
  }
  if (lag && nsteps > 0) {
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j) mma(acc[i][j], fa[1][i], fb[1][j]);
  }
  __syncthreads();
  if constexpr (MODE == MODE_DGRAD && POST)
    conv_epilogue<MODE, T, BM, BN, WMW, WNW>(a, acc, smem, m0, n0, tm, post, rmap, by);
  else
    conv_epilogue_impl<MODE, T, BM, BN, WMW, WNW, FM, FN, false, FOLD>(
        a, acc, smem, m0, n0, tm, post, false, rmap, by, (MODE == MODE_FWD && ds) ? a.out_ds : nullptr,
        (MODE == MODE_FWD && ds) ? a.partial_ds : nullptr);
}

}  // namespace

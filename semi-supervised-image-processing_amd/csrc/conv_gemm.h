// Register-staged implicit-GEMM kernel: every dtype, tile and mode.
#pragma once
#include "conv_epilogue.h"

namespace {

// ---------------------------------------------------------------------------
// the kernel
// ---------------------------------------------------------------------------
template <int MODE, typename T, int BM, int BN, int WMW, int WNW, bool CONV1>
__global__ void __launch_bounds__(64 * WMW * WNW) conv_gemm_kernel(const ConvArgs a) {
  constexpr int NT = 64 * WMW * WNW;
  constexpr int BK = Traits<T>::BK;
  constexpr int KC = BK / 8;                 // 8-element chunks per k-tile row
  constexpr int NSUB = BK / 32;              // 32-deep MFMA sub-steps per k step
  constexpr int WTM = BM / WMW, WTN = BN / WNW;
  constexpr int FM = WTM / 16, FN = WTN / 16;
  constexpr bool WG = (MODE == MODE_WGRAD);
  typedef Smem<MODE, T, BM, BN> SM;
  constexpr int ITA = WG ? (BK * BM / 8) / NT : (BM * KC) / NT;
  constexpr int ITB = WG ? (BK * BN / 8) / NT : (BN * KC) / NT;
  static_assert(ITA >= 1 && ITB >= 1 && FM >= 1 && FN >= 1, "tile too small");
  static_assert(!WG || ((BK * BM / 8) % NT == 0 && (BK * BN / 8) % NT == 0), "bad WGRAD tile");
  __shared__ __attribute__((aligned(16))) char smem[SM::BYTES];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WNW, wn = wave % WNW;

  const int tn = blockIdx.x % a.tiles_n;
  const int tm = blockIdx.x / a.tiles_n;
  const int m0 = tm * BM, n0 = tn * BN;

  const T* __restrict__ Ag = static_cast<const T*>(a.A);
  const T* __restrict__ Bg = static_cast<const T*>(a.B);

  // ---------------- per-thread loader state ----------------
  // FWD/DGRAD: chunk id = tid + it*NT -> (row = id / KC, kc = id % KC); KC | NT so kc is fixed per thread
  // WGRAD A: [BK m][BM cols]: ml = id / (BM/8), col chunk = id % (BM/8) (fixed per thread)
  // WGRAD B: [BK m][BN cols]: ml = id / (BN/8), col chunk = id % (BN/8) (fixed per thread)
  int a_base[ITA], a_h[ITA], a_w[ITA];
  bool a_ok[ITA];
  int b_r = 0, b_s = 0, b_c = 0;
  bool b_colok = true;
  const int kc = tid % KC;

  // uniform k-step counters (FWD/DGRAD):  k = ((r*S)+s)*Cred + cb
  int kr = 0, ks_ = 0, kcb = 0;
  const int Cred = (MODE == MODE_FWD) ? a.C : a.K;

  long mstart = 0, mend = 0;
  if constexpr (!WG) {
#pragma unroll
    for (int it = 0; it < ITA; ++it) {
      const int row = (tid + it * NT) / KC;
      const int m = m0 + row;
      a_ok[it] = m < a.M;
      const int mm = a_ok[it] ? m : 0;
      if constexpr (MODE == MODE_FWD) {
        const int n = fdiv(mm, a.div_pq);
        const int rem = mm - n * a.P * a.Q;
        const int p = fdiv(rem, a.div_q);
        const int q = rem - p * a.Q;
        a_base[it] = n * a.H * a.W;
        a_h[it] = p * a.stride - a.pad;
        a_w[it] = q * a.stride - a.pad;
      } else {
        const int n = fdiv(mm, a.div_hw);
        const int rem = mm - n * a.H * a.W;
        const int h = fdiv(rem, a.div_w);
        const int w = rem - h * a.W;
        a_base[it] = n * a.P * a.Q;
        a_h[it] = h + a.pad;
        a_w[it] = w + a.pad;
      }
    }
  } else {
    mstart = (long)blockIdx.y * a.ksteps * BK;
    mend = mstart + (long)a.ksteps * BK;
    if (mend > a.Mred) mend = a.Mred;
    const int nc = tid % (BN / 8);
    const int col = n0 + nc * 8;
    b_colok = col < a.Ng;
    const int cc = b_colok ? col : 0;
    if constexpr (CONV1) {
      b_r = cc / (a.S * a.C);
      const int rem = cc - b_r * a.S * a.C;
      b_s = rem / a.C;
      b_c = 0;
    } else {
      const int rs = cc / a.C;
      b_c = cc - rs * a.C;
      b_r = rs / a.S;
      b_s = rs - b_r * a.S;
    }
  }

  Vec8<T> ra[ITA], rb[ITB];

  auto load_tiles = [&](int ks) {
    if constexpr (MODE == MODE_FWD) {
#pragma unroll
      for (int it = 0; it < ITA; ++it) {
        if constexpr (CONV1) {
          // k = ks*BK + kc*8: filter row r = k / 32, pixel pair s = (k % 32) / 4, 4 channels each
          const int k = ks * BK + kc * 8;
          const int r = k >> 5;
          const int s0 = (k & 31) >> 2;
          const int hin = a_h[it] + r;
          const int w0 = a_w[it] + s0;
          const bool rowok = a_ok[it] && r < a.R && hin >= 0 && hin < a.H;
          const bool ok0 = rowok && w0 >= 0 && w0 < a.W;
          const bool ok1 = rowok && (w0 + 1) >= 0 && (w0 + 1) < a.W;
          const T* p0 = Ag + ((long)(a_base[it] + hin * a.W + w0)) * 4;
          load_2px<T>(ra[it], p0, ok0, p0 + 4, ok1);
        } else {
          const int hin = a_h[it] + kr, win = a_w[it] + ks_;
          const bool ok = a_ok[it] && hin >= 0 && hin < a.H && win >= 0 && win < a.W;
          const T* p = Ag + ((long)(a_base[it] + hin * a.W + win)) * a.C + kcb + kc * 8;
          load_v8<T>(ra[it], p, ok);
        }
      }
    } else if constexpr (MODE == MODE_DGRAD) {
#pragma unroll
      for (int it = 0; it < ITA; ++it) {
        const int hp = a_h[it] - kr, wp = a_w[it] - ks_;
        int p = hp, q = wp;
        bool ok = a_ok[it] && hp >= 0 && wp >= 0;
        if (a.stride != 1) {
          ok = ok && ((hp | wp) & (a.stride - 1)) == 0;  // stride is a power of two (host-checked)
          p = hp >> (a.stride >> 1);
          q = wp >> (a.stride >> 1);
        }
        ok = ok && p < a.P && q < a.Q;
        const T* ptr = Ag + ((long)(a_base[it] + p * a.Q + q)) * a.K + kcb + kc * 8;
        load_v8<T>(ra[it], ptr, ok);
      }
    }
    if constexpr (!WG) {
#pragma unroll
      for (int it = 0; it < ITB; ++it) {
        const int row = (tid + it * NT) / KC;
        const int n = n0 + row;
        const int k = ks * BK + kc * 8;
        const bool ok = n < a.Ng && k < a.Kg;
        const T* p = Bg + (long)(ok ? n : 0) * a.Kg + (ok ? k : 0);
        load_v8<T>(rb[it], p, ok);
      }
    } else {
#pragma unroll
      for (int it = 0; it < ITA; ++it) {
        const int id = tid + it * NT;
        const int ml = id / (BM / 8), cch = id % (BM / 8);
        const long m = mstart + (long)ks * BK + ml;
        const int k = m0 + cch * 8;
        const bool ok = m < mend && k < a.K;
        const T* p = Ag + (ok ? m : 0) * (long)a.K + (ok ? k : 0);
        load_v8<T>(ra[it], p, ok);
      }
#pragma unroll
      for (int it = 0; it < ITB; ++it) {
        const int id = tid + it * NT;
        const int ml = id / (BN / 8);
        const long m = mstart + (long)ks * BK + ml;
        const bool mok = m < mend && b_colok;
        const int mm = mok ? (int)m : 0;
        const int n = fdiv(mm, a.div_pq);
        const int rem = mm - n * a.P * a.Q;
        const int p = fdiv(rem, a.div_q);
        const int q = rem - p * a.Q;
        const int hin = p * a.stride - a.pad + b_r;
        if constexpr (CONV1) {
          const int w0 = q * a.stride - a.pad + b_s;
          const bool rowok = mok && hin >= 0 && hin < a.H;
          const bool ok0 = rowok && w0 >= 0 && w0 < a.W;
          const bool ok1 = rowok && (w0 + 1) >= 0 && (w0 + 1) < a.W;
          const T* p0 = Bg + ((long)((n * a.H + hin) * a.W + w0)) * 4;
          load_2px<T>(rb[it], p0, ok0, p0 + 4, ok1);
        } else {
          const int win = q * a.stride - a.pad + b_s;
          const bool ok = mok && hin >= 0 && hin < a.H && win >= 0 && win < a.W;
          const T* ptr = Bg + ((long)((n * a.H + hin) * a.W + win)) * a.C + b_c;
          load_v8<T>(rb[it], ptr, ok);
        }
      }
    }
  };

  auto advance_k = [&]() {  // uniform (r, s, cb) counters for FWD/DGRAD
    if constexpr (!WG && !CONV1) {
      kcb += BK;
      if (kcb >= Cred) {
        kcb = 0;
        if (++ks_ >= a.S) { ks_ = 0; ++kr; }
      }
    }
  };

  auto store_tiles = [&](int buf) {
    char* As = smem + buf * SM::STAGE;
    char* Bs = As + SM::A_BYTES;
    if constexpr (!WG) {
#pragma unroll
      for (int it = 0; it < ITA; ++it) store_kchunk(As, (tid + it * NT) / KC, kc, ra[it]);
#pragma unroll
      for (int it = 0; it < ITB; ++it) store_kchunk(Bs, (tid + it * NT) / KC, kc, rb[it]);
    } else {
#pragma unroll
      for (int it = 0; it < ITA; ++it) {
        const int id = tid + it * NT;
        store_mchunk<BM>(As, id / (BM / 8), (id % (BM / 8)) * 8, ra[it]);
      }
#pragma unroll
      for (int it = 0; it < ITB; ++it) {
        const int id = tid + it * NT;
        store_mchunk<BN>(Bs, id / (BN / 8), (id % (BN / 8)) * 8, rb[it]);
      }
    }
  };

  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  int nsteps = a.ksteps;
  if constexpr (WG) {
    const long rem = mend - mstart;
    nsteps = rem > 0 ? (int)((rem + BK - 1) / BK) : 0;
  }

  if (nsteps > 0) {
    load_tiles(0);
    advance_k();
    store_tiles(0);
    __syncthreads();
  }
  for (int ks = 0; ks < nsteps; ++ks) {
    const int cur = ks & 1;
    if (ks + 1 < nsteps) {
      load_tiles(ks + 1);
      advance_k();
    }
    const char* As = smem + cur * SM::STAGE;
    const char* Bs = As + SM::A_BYTES;
#pragma unroll
    for (int h = 0; h < NSUB; ++h) {
      Frag<T> fa[FM], fb[FN];
      if constexpr (!WG) {
#pragma unroll
        for (int i = 0; i < FM; ++i) read_kfrag(fa[i], As, wm * WTM + i * 16 + (lane & 15), lane >> 4, h);
#pragma unroll
        for (int j = 0; j < FN; ++j) read_kfrag(fb[j], Bs, wn * WTN + j * 16 + (lane & 15), lane >> 4, h);
      } else {
#pragma unroll
        for (int i = 0; i < FM; ++i) read_mfrag<BM>(fa[i], As, wm * WTM + i * 16, lane, h);
#pragma unroll
        for (int j = 0; j < FN; ++j) read_mfrag<BN>(fb[j], Bs, wn * WTN + j * 16, lane, h);
      }
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) mma(acc[i][j], fa[i], fb[j]);
    }
    if (ks + 1 < nsteps) store_tiles(cur ^ 1);
    __syncthreads();
  }

  conv_epilogue<MODE, T, BM, BN, WMW, WNW>(a, acc, smem, m0, n0, tm);
}

}  // namespace

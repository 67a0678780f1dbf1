// Epilogue of the implicit-GEMM kernels (conv_gemm_kernel, conv_glds_kernel).
#pragma once
#include "conv_tile.h"

namespace {

template <int MODE, typename T, int BM, int BN>
struct Smem {
  static constexpr int BK = Traits<T>::BK;
  static constexpr bool WG = (MODE == MODE_WGRAD);
  static constexpr int A_BYTES = WG ? BK * MTile<T, BM>::ROW_BYTES : BM * 128;
  static constexpr int B_BYTES = WG ? BK * MTile<T, BN>::ROW_BYTES : BN * 128;
  static constexpr int STAGE = A_BYTES + B_BYTES;
  static constexpr int EPI = WG ? 0 : BM * (BN * (int)sizeof(T) + 16);
  static constexpr int BYTES = (2 * STAGE > EPI) ? 2 * STAGE : EPI;
};

// ---------------------------------------------------------------------------
// shared epilogue: WGRAD -> fp32 slab; FWD/DGRAD -> LDS-staged 16-B stores
// (+ residual-gradient add for DGRAD, + BN partial statistics for FWD)
// ---------------------------------------------------------------------------
// DGRAD epilogue with the BatchNorm-backward reduction fused in (the tile is
// already staged in LDS as T).  Each thread owns one 8-channel chunk (NT is a
// multiple of BN/8), so its sums stay in registers; the NT/(BN/8) partial
// sums per chunk are combined in fixed order through LDS.
// The epilogue operands of the fused BN backward (mask z, pre-BN y and the
// residual-gradient add) for the rows this thread stores; the LDS-DMA kernel
// loads them before its main loop so the epilogue never waits on HBM.
template <typename T, int BM, int BN, int NT>
struct BnPostRegs {
  static constexpr int CPR = BN / 8;
  static constexpr int RPI = NT / CPR;  // rows per pass
  static constexpr int ROWS = BM / RPI;
  static_assert(NT % CPR == 0 && BM % RPI == 0, "thread count must cover whole rows");
  Vec8<T> z[ROWS], y[ROWS], add[ROWS];
  uint32_t mb[ROWS];  // mask byte (pbits) of the thread's 8-channel chunk

  __device__ __forceinline__ void load(const ConvArgs& a, int m0, int n0) {
    const int tid = threadIdx.x;
    const int ch = tid % CPR, rsub = tid / CPR;
    const int n = n0 + ch * 8;
    if (n >= a.Ng) return;
    const T* Zm = static_cast<const T*>(a.pmask);
    const T* Yp = static_cast<const T*>(a.py);
    const T* Add = static_cast<const T*>(a.add);
#pragma unroll
    for (int k = 0; k < ROWS; ++k) {
      const int m = m0 + rsub + k * RPI;
      if (m < a.M) {
        const long off = (long)m * a.Ng + n;
        if (Zm) z[k].load(Zm + off);
        else if (a.pbits) mb[k] = a.pbits[off >> 3];
        y[k].load(Yp + off);
        if (Add) add[k].load(Add + off);
      }
    }
  }
};

template <typename T, int BM, int BN, int NT>
__device__ __forceinline__ void dgrad_bn_post(const ConvArgs& a, char* smem, int m0, int n0, int tm,
                                              const BnPostRegs<T, BM, BN, NT>& pr) {
  constexpr int CPR = BN / 8;
  constexpr int RPI = NT / CPR;  // rows per pass
  constexpr int ROWS = BM / RPI;
  constexpr int EROW = BN * (int)sizeof(T) + 16;
  const int tid = threadIdx.x;
  const int ch = tid % CPR, rsub = tid / CPR;
  const int n = n0 + ch * 8;
  T* Out = static_cast<T*>(a.out);
  const bool has_add = a.add != nullptr;
  float sd[8], sx[8], mu[8], is[8], msc[8], msh[8];
  const bool nok = n < a.Ng;
  const int mode = a.pmask ? 0 : (a.pbits ? 1 : 2);  // mask source (ConvArgs)
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    sd[j] = 0.f;
    sx[j] = 0.f;
    mu[j] = nok ? a.pmean[n + j] : 0.f;
    is[j] = nok ? a.pinvstd[n + j] : 0.f;
    msc[j] = (nok && mode == 2) ? a.pmscale[n + j] : 0.f;
    msh[j] = (nok && mode == 2) ? a.pmshift[n + j] : 0.f;
  }
  if (nok) {
#pragma unroll
    for (int k = 0; k < ROWS; ++k) {
      const int row = rsub + k * RPI;
      const int m = m0 + row;
      if (m >= a.M) break;
      Vec8<T> v;
      const char* src = smem + row * EROW + ch * 8 * (int)sizeof(T);
      if constexpr (sizeof(T) == 2) {
        v.v = *reinterpret_cast<const i32x4*>(src);
      } else {
        reinterpret_cast<Vec8<float>&>(v).v0 = reinterpret_cast<const i32x4*>(src)[0];
        reinterpret_cast<Vec8<float>&>(v).v1 = reinterpret_cast<const i32x4*>(src)[1];
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float d = v.get(j);
        if (has_add) d += pr.add[k].get(j);
        const bool keep = mode == 0 ? pr.z[k].get(j) > 0.f
                                    : (mode == 1 ? ((pr.mb[k] >> j) & 1u) != 0u
                                                 : __builtin_fmaf(pr.y[k].get(j), msc[j], msh[j]) > 0.f);
        d = keep ? d : 0.f;
        v.set(j, d);
        const float dq = v.get(j);  // the stored (rounded) value feeds the sums
        sd[j] += dq;
        sx[j] += dq * ((pr.y[k].get(j) - mu[j]) * is[j]);
      }
      v.store(Out + (long)m * a.Ng + n);
    }
  }
  // lanes l, l+CPR, ... of a wave share a chunk: butterfly over the lane
  // bits above log2(CPR), then combine the waves in fixed order via LDS.
  static_assert(CPR == 8 || CPR == 16 || CPR == 32, "chunk count per row");
#pragma unroll
  for (int o = CPR; o < 64; o <<= 1) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      sd[j] += __shfl_xor(sd[j], o, 64);
      sx[j] += __shfl_xor(sx[j], o, 64);
    }
  }
  __syncthreads();
  constexpr int NW = NT / 64;
  float* red = reinterpret_cast<float*>(smem);  // [NW][CPR][16]
  const int lane = tid & 63, wave = tid >> 6;
  if (lane < CPR) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      red[(wave * CPR + lane) * 16 + j] = sd[j];
      red[(wave * CPR + lane) * 16 + 8 + j] = sx[j];
    }
  }
  __syncthreads();
  if (tid < CPR * 16) {
    const int c8 = tid >> 4, v = tid & 15;  // chunk, value (0-7 sum d, 8-15 sum d*xhat)
    const int nn = n0 + c8 * 8;
    if (nn < a.Ng) {
      float t = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) t += red[(w * CPR + c8) * 16 + v];
      const int tiles_m = (a.M + BM - 1) / BM;  // [Ng][tiles_m][2]: each channel's records contiguous
      a.partial[((long)(nn + (v & 7)) * tiles_m + tm) * 2 + (v >> 3)] = t;
    }
  }
}

// GEMM row -> output row (identity, or the phase's strided rows of dx)
struct RowMap {
  int M;
  bool phased;  // false: identity
  int H, W, ph, pw, Wph;
  FastDiv div_hw, div_w;
  __device__ __forceinline__ long row(int m) const {
    if (!phased) return m;
    const int n = fdiv(m, div_hw);
    const int rem = m - n * (int)div_hw.d;
    const int i = fdiv(rem, div_w);
    const int j = rem - i * Wph;
    return ((long)n * H + 2 * i + ph) * W + 2 * j + pw;
  }
};

template <int MODE, typename T, int BM, int BN, int WMW, int WNW, int FM, int FN, bool ALLOW_POST = true,
          bool FOLD = false>
__device__ __forceinline__ void conv_epilogue_impl(const ConvArgs& a, f32x4 (&acc)[FM][FN], char* smem, int m0,
                                                   int n0, int tm, const BnPostRegs<T, BM, BN, 64 * WMW * WNW>& pre,
                                                   bool pre_loaded, const RowMap& rmap, int split,
                                                   void* out_alt = nullptr, float* partial_alt = nullptr) {
  constexpr int NT = 64 * WMW * WNW;
  constexpr int WTM = BM / WMW, WTN = BN / WNW;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WNW, wn = wave % WNW;
  const int rbase = wm * WTM + (lane >> 4) * 4;
  const int cbase = wn * WTN + (lane & 15);
  if constexpr (MODE == MODE_WGRAD) {
    float* slab = static_cast<float*>(a.out) + (long)split * a.M * a.Ng;
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        const int n = n0 + cbase + j * 16;
        if (n >= a.Ng) continue;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int m = m0 + rbase + i * 16 + e;
          if (m < a.M) slab[(long)m * a.Ng + n] = acc[i][j][e];
        }
      }
    return;
  }

  // stage the tile through LDS (main loop finished: the staging buffers are free)
  constexpr int EROW = BN * (int)sizeof(T) + 16;  // padded row (bytes)
  {
    float bcol[FN];
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int n = n0 + cbase + j * 16;
      bcol[j] = (FOLD && n < a.Ng) ? a.bias[n] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int row = rbase + i * 16 + e;
          const int col = cbase + j * 16;
          *reinterpret_cast<T*>(smem + row * EROW + col * (int)sizeof(T)) =
              from_f32<T>(FOLD ? acc[i][j][e] + bcol[j] : acc[i][j][e]);
        }
  }
  __syncthreads();
  if constexpr (MODE == MODE_DGRAD && ALLOW_POST) {
    if (a.pmean != nullptr) {
      if (pre_loaded) {
        dgrad_bn_post<T, BM, BN, NT>(a, smem, m0, n0, tm, pre);
      } else {
        BnPostRegs<T, BM, BN, NT> pr;
        pr.load(a, m0, n0);
        dgrad_bn_post<T, BM, BN, NT>(a, smem, m0, n0, tm, pr);
      }
      return;
    }
  }
  {
    // each thread moves 8-element chunks: BN/8 chunks per row
    constexpr int CPR = BN / 8;
    T* Out = static_cast<T*>(out_alt ? out_alt : a.out);   // may alias Add (in-place residual-gradient add)
    const T* Add = static_cast<const T*>(a.add);
    for (int id = tid; id < BM * CPR; id += NT) {
      const int row = id / CPR, ch = id % CPR;
      const int m = m0 + row, n = n0 + ch * 8;
      if (m >= rmap.M || n >= a.Ng) continue;
      const long orow = rmap.row(m);
      Vec8<T> v;
      const char* src = smem + row * EROW + ch * 8 * (int)sizeof(T);
      if constexpr (sizeof(T) == 2) {
        v.v = *reinterpret_cast<const i32x4*>(src);
      } else {
        reinterpret_cast<Vec8<float>&>(v).v0 = reinterpret_cast<const i32x4*>(src)[0];
        reinterpret_cast<Vec8<float>&>(v).v1 = reinterpret_cast<const i32x4*>(src)[1];
      }
      if constexpr (MODE == MODE_DGRAD) {
        if (Add) {
          // the unrounded accumulator would be better; the LDS copy is already in T
          Vec8<T> r;
          r.load(Add + orow * a.Ng + n);
#pragma unroll
          for (int j = 0; j < 8; ++j) v.set(j, v.get(j) + r.get(j));
        }
      }
      if constexpr (MODE == MODE_FWD && FOLD) {  // folded eval BN: + residual, ReLU (bias already in)
        {
          Vec8<T> r;
          if (Add) r.load(Add + orow * a.Ng + n);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            float t = v.get(j);
            if (Add) t += r.get(j);
            if (a.relu) t = t > 0.f ? t : 0.f;
            v.set(j, t);
          }
        }
      }
      v.store(Out + orow * a.Ng + n);
    }
  }

  if constexpr (MODE == MODE_FWD) {
    float* const partial = partial_alt ? partial_alt : a.partial;
    if (partial == nullptr) return;
    __syncthreads();
    // BatchNorm partial statistics over this tile's valid rows (from fp32 accumulators).
    float* red = reinterpret_cast<float*>(smem);  // [WMW][BN]
    float* mean_t = red + WMW * BN;               // [BN]
    const int cnt = min(BM, a.M - m0);
    float s[FN];
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      float t = 0.f;
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int row = rbase + i * 16 + e;
          t += (row < cnt) ? acc[i][j][e] : 0.f;
        }
      t += __shfl_xor(t, 16, 64);
      t += __shfl_xor(t, 32, 64);
      s[j] = t;
    }
    if (lane < 16) {
#pragma unroll
      for (int j = 0; j < FN; ++j) red[wm * BN + cbase + j * 16] = s[j];
    }
    __syncthreads();
    for (int c = tid; c < BN; c += NT) {
      float t = 0.f;
#pragma unroll
      for (int w = 0; w < WMW; ++w) t += red[w * BN + c];
      mean_t[c] = t / (float)cnt;
    }
    __syncthreads();
    float q2[FN];
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const float mu = mean_t[cbase + j * 16];
      float t = 0.f;
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int row = rbase + i * 16 + e;
          const float d = acc[i][j][e] - mu;
          t += (row < cnt) ? d * d : 0.f;
        }
      t += __shfl_xor(t, 16, 64);
      t += __shfl_xor(t, 32, 64);
      q2[j] = t;
    }
    __syncthreads();
    if (lane < 16) {
#pragma unroll
      for (int j = 0; j < FN; ++j) red[wm * BN + cbase + j * 16] = q2[j];
    }
    __syncthreads();
    const int tiles_m = a.stat_tiles_m > 0 ? a.stat_tiles_m : (int)(gridDim.x / a.tiles_n);
    for (int c = tid; c < BN; c += NT) {
      const int n = n0 + c;
      if (n < a.Ng) {
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < WMW; ++w) t += red[w * BN + c];
        float* rec = partial + ((long)n * tiles_m + tm) * 3;  // [C][tiles][3]
        rec[0] = (float)cnt;
        rec[1] = mean_t[c] * (float)cnt;
        rec[2] = t;
      }
    }
  }
}

template <int MODE, typename T, int BM, int BN, int WMW, int WNW, int FM, int FN>
__device__ __forceinline__ void conv_epilogue(const ConvArgs& a, f32x4 (&acc)[FM][FN], char* smem, int m0, int n0,
                                              int tm) {
  BnPostRegs<T, BM, BN, 64 * WMW * WNW> none;
  RowMap rmap;
  rmap.M = a.M;
  rmap.phased = false;
  if (MODE == MODE_FWD && a.bias != nullptr)  // ssip_conv_fwd_bias on the register-staged kernel
    conv_epilogue_impl<MODE, T, BM, BN, WMW, WNW, FM, FN, true, true>(a, acc, smem, m0, n0, tm, none, false, rmap,
                                                                      (int)blockIdx.y);
  else
    conv_epilogue_impl<MODE, T, BM, BN, WMW, WNW, FM, FN>(a, acc, smem, m0, n0, tm, none, false, rmap,
                                                          (int)blockIdx.y);
}

template <int MODE, typename T, int BM, int BN, int WMW, int WNW, int FM, int FN>
__device__ __forceinline__ void conv_epilogue(const ConvArgs& a, f32x4 (&acc)[FM][FN], char* smem, int m0, int n0,
                                              int tm, const BnPostRegs<T, BM, BN, 64 * WMW * WNW>& pre,
                                              const RowMap& rmap, int split) {
  conv_epilogue_impl<MODE, T, BM, BN, WMW, WNW, FM, FN>(a, acc, smem, m0, n0, tm, pre, true, rmap, split);
}

}  // namespace

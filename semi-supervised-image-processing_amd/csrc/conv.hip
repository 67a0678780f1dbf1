// Implicit-GEMM convolution for gfx950 (CDNA4), NHWC activations.
//
// Replaces the torchvision/MIOpen convolutions that ResNet-18 runs inside
// `model(inputs)` / `loss.backward()` in the reference hot loop
// (reference: src/training/common.py:380-382; model built at :299-304).
//
// Three GEMM views of one conv (M x N x K, all fp32-accumulated on MFMA):
//   FWD   : Y[m=(n,p,q)][k]        = sum_{(r,s,c)} X[n,p*st-pd+r,q*st-pd+s,c] * W[k][r][s][c]
//   DGRAD : dX[m=(n,h,w)][c]       = sum_{(r,s,k)} dY[n,(h+pd-r)/st,(w+pd-s)/st,k] * WT[c][r][s][k]
//   WGRAD : dW[k][(r,s,c)]         = sum_{m=(n,p,q)} dY[m][k] * X[n,p*st-pd+r,q*st-pd+s,c]
//
// Block = WMW x WNW waves (64-wide), tile BM x BN, k-step BK = 128 bytes of
// reduction per row (64 bf16 / 32 f32).  FWD/DGRAD stage A/B as
// [rows][128 B] k-contiguous LDS tiles (16-B slot XOR swizzle, conflict-free
// ds_read_b128 fragment reads); WGRAD stages both operands m-major
// ([BK][cols], as they lie in HBM) and reads fragments with
// ds_read_b64_tr_b16 (bf16) — no register transposes.  Global->LDS staging
// is register double-buffered (issue k+1 loads before the MFMAs of k, write
// them to the other LDS buffer after), one barrier per k-step.
// bf16: v_mfma_f32_16x16x32_bf16; f32 parity path: v_mfma_f32_16x16x4_f32 on
// the same tiles.  Epilogue goes through LDS so global stores (and the
// residual-gradient add of DGRAD) are 16-B per lane, row-contiguous.
//
// FWD also emits per-(channel, M-tile) BatchNorm partial statistics
// {count, sum, M2-about-tile-mean} from the fp32 accumulators so the BN
// batch statistics need no extra pass over Y.  WGRAD is split over the m
// reduction into fp32 slabs that a second kernel sums in fixed order
// (bitwise reproducible, no atomics).
//
// The kernels live in one header per family (conv_tile.h: what they share;
// conv_epilogue.h, conv_gemm.h, conv_glds.h: the implicit GEMM; conv_halo.h,
// conv_stem.h: the persistent layer-1 / stem kernels; conv_wgrad_reduce.h),
// all in this file's anonymous namespace.  This file is the host side.
#include <algorithm>
#include <cstdio>
#include "ssip_common.h"
#include "fin_split.h"
#include "conv_gemm.h"
#include "conv_glds.h"
#include "conv_halo.h"
#include "conv_stem.h"
#include "conv_wgrad_reduce.h"

namespace {

// ---------------------------------------------------------------------------
// host-side planning
//
// Every extern "C" entry point has one shape: read the knobs once
// (conv_knobs), route the call (route_fwd / route_dgrad / route_wgrad: the
// one place that orders the kernel families), validate pointers and
// workspace, fill the operands, launch.  The size queries and the name query
// read the same route objects, so they cannot disagree with a launch.
// ---------------------------------------------------------------------------
struct Plan {
  int mode;
  int bm, bn, wmw, wnw;
  int stages;  // 2/3: LDS-DMA ring kernel (bf16); 0: register-staged kernel
  bool conv1;
  bool stem_glds;  // conv1 on a pre-padded image (pad 0, even W): LDS-DMA capable
  ConvArgs args;
  dim3 grid;
  int splits;
};

static bool desc_ok(const ssip_conv_desc* d) {
  return d && d->N > 0 && d->H > 0 && d->W > 0 && d->C > 0 && d->K > 0 && d->R > 0 && d->S > 0 &&
         d->stride > 0 && d->pad >= 0 && d->P > 0 && d->Q > 0;
}

static void fill_common(ConvArgs& a, const ssip_conv_desc* d) {
  memset(&a, 0, sizeof(a));
  a.N = d->N; a.H = d->H; a.W = d->W; a.C = d->C; a.K = d->K; a.R = d->R; a.S = d->S;
  a.stride = d->stride; a.pad = d->pad; a.P = d->P; a.Q = d->Q;
  a.div_pq = make_fastdiv((uint32_t)(d->P * d->Q));
  a.div_q = make_fastdiv((uint32_t)d->Q);
  a.div_hw = make_fastdiv((uint32_t)(d->H * d->W));
  a.div_w = make_fastdiv((uint32_t)d->W);
}

static void pick_tile(int M, int Ng, int elem_bytes, Plan& pl) {
  // bf16: 256-row tiles (8 waves) when the grid still fills the chip twice over
  const int bn = (Ng % 128 == 0) ? 128 : 64;
  const long blocks256 = (long)ceil_div(M, 256) * ceil_div(Ng, bn);
  if (elem_bytes == 2 && blocks256 >= 512) {
    pl.bm = 256; pl.bn = bn; pl.wmw = 4; pl.wnw = 2;
  } else {
    pl.bm = 128; pl.bn = bn; pl.wmw = 2; pl.wnw = 2;
  }
}

static int elem_bytes_of(int dtype) { return dtype == SSIP_BF16 ? 2 : 4; }

static int device_cus() {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0, v = 0;
    cus = (hipGetDevice(&dev) == hipSuccess &&
           hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0)
              ? v
              : 256;
  }
  return cus;
}

// The tuning knobs of this file, read from the environment once per extern "C"
// call (tests and labs flip them in one process) and handed down: this file's
// only environment reads.
// ssip/ops.py keys its plan cache on these names (tests/test_cpu_conv_knobs.py).
struct ConvKnobs {
  bool halo;           // SSIP_HALO (0: off): the halo / stem kernels where they apply
  const char* force;   // SSIP_CONV_FORCE="<f|d|w>,bm,bn,waves_m,waves_n,stages" (apply_force), or null
  int stagger;         // SSIP_STAGGER: pass mask (stagger_for)
  bool wgrad_big;      // SSIP_WGRAD_BIG (0: the full-grid tiles for a wgrad with a budget)
  int wgrad_blocks;    // SSIP_WGRAD_BLOCKS: target workgroup count of a wgrad (0: unset)
  int bnrelu_glds;     // SSIP_BNRELU_GLDS: bit 0 the 1x1, bit 1 the 3x3 BN+ReLU-in ring form (glds_inbn_plan)
  long bnrelu_minm;    // SSIP_BNRELU_GLDS_MINM: fewest rows for the 1x1 form
  bool no_fwd_dsfuse;  // SSIP_NO_FWD_DSFUSE: conv + downsample forwards as two launches
  // the halo / stem kernels may take pass 'f' / 'd' / 'w': not switched off, and
  // no SSIP_CONV_FORCE for that pass (it selects the implicit-GEMM kernels)
  bool halo_for(char pass) const { return halo && !(force && force[0] == pass); }
};

static ConvKnobs conv_knobs() {
  ConvKnobs k;
  const char* e = getenv("SSIP_HALO");
  k.halo = !(e && e[0] == '0');
  k.force = getenv("SSIP_CONV_FORCE");
  e = getenv("SSIP_STAGGER");
  k.stagger = e ? atoi(e) : 7;
  e = getenv("SSIP_WGRAD_BIG");
  k.wgrad_big = !e || atoi(e) != 0;
  e = getenv("SSIP_WGRAD_BLOCKS");
  k.wgrad_blocks = (e && e[0]) ? std::max(1, atoi(e)) : 0;
  e = getenv("SSIP_BNRELU_GLDS");
  k.bnrelu_glds = e ? atoi(e) : 1;
  e = getenv("SSIP_BNRELU_GLDS_MINM");
  k.bnrelu_minm = e ? atol(e) : 262144l;
  k.no_fwd_dsfuse = getenv("SSIP_NO_FWD_DSFUSE") != nullptr;
  return k;
}

// ---- kernel instances: one table and one lookup per implicit-GEMM family
typedef void (*ConvKernel)(const ConvArgs);
static const char* const MODE_NAME[3] = {"fwd", "dgrad", "wgrad"};

// LDS-DMA ring kernel configurations (bm, bn, waves_m, waves_n, stages):
// the ones choose_glds() selects (round 3's wider tuning sets are on the
// r3-variants branch, with tools/tune_conv.py's lists)
#define SSIP_GLDS_FD(X, M, F) \
  X(M, F, 128, 128, 4, 2, 2) X(M, F, 128, 64, 4, 2, 2) X(M, F, 256, 256, 4, 2, 2) X(M, F, 128, 128, 4, 4, 3)
// (the first two: the full-grid tiles; the other two: the side-stream budget's)
#define SSIP_GLDS_WG(X, M, F) \
  X(M, F, 128, 128, 4, 2, 2) X(M, F, 64, 128, 2, 4, 2) X(M, F, 128, 256, 2, 4, 2) X(M, F, 256, 256, 4, 2, 2)
// the fused BN-backward epilogue (DGRAD) and the folded eval BN epilogue (FWD): the default tiles only
#define SSIP_GLDS_POST(X, M, F) X(M, F, 128, 128, 4, 2, 2) X(M, F, 128, 64, 4, 2, 2)
#define SSIP_GLDS_FOLD(X, M, F) SSIP_GLDS_FD(X, M, F)
#define SSIP_GLDS_STEM(X, M, F) X(M, F, 128, 64, 4, 2, 2)
// the LDS-DMA ring configurations with the BN+ReLU-in operand transform
#define SSIP_GLDS_INBN_FD(X, M, F) X(M, F, 128, 128, 4, 2, 2) X(M, F, 128, 64, 4, 2, 2) X(M, F, 256, 256, 4, 2, 2)
#define SSIP_GLDS_INBN_WG(X, M, F) X(M, F, 128, 128, 4, 2, 2)

enum GldsForm { GLDS_PLAIN, GLDS_STEM, GLDS_POST, GLDS_FOLD, GLDS_INBN };
// per form: check_launch's name, and the "no <what> kernel for <tile>" of a tile without an instance
static const struct { const char *check, *what; } GLDS_FORMS[] = {
    {"conv_glds", "LDS-DMA conv"},          {"conv_glds_stem", "LDS-DMA stem"},    {"conv_glds_bnpost", "fused-BN dgrad"},
    {"conv_glds_fold", "folded-BN conv"},   {"conv_glds_inbn", "BN+ReLU-in conv"}};

struct GldsRow {
  int mode, form, bm, bn, wmw, wnw, stages;
  ConvKernel fn;
};
#define SSIP_GLDS_ROW(M, F, BM_, BN_, WM_, WN_, ST_)                                                         \
  {M, F, BM_, BN_, WM_, WN_, ST_,                                                                            \
   conv_glds_kernel<M, BM_, BN_, WM_, WN_, ST_, F == GLDS_STEM, F == GLDS_POST, F == GLDS_FOLD, F == GLDS_INBN>},
static const GldsRow GLDS_TABLE[] = {
    SSIP_GLDS_FD(SSIP_GLDS_ROW, MODE_FWD, GLDS_PLAIN) SSIP_GLDS_FD(SSIP_GLDS_ROW, MODE_DGRAD, GLDS_PLAIN)
    SSIP_GLDS_WG(SSIP_GLDS_ROW, MODE_WGRAD, GLDS_PLAIN) SSIP_GLDS_STEM(SSIP_GLDS_ROW, MODE_FWD, GLDS_STEM)
    SSIP_GLDS_POST(SSIP_GLDS_ROW, MODE_DGRAD, GLDS_POST) SSIP_GLDS_FOLD(SSIP_GLDS_ROW, MODE_FWD, GLDS_FOLD)
    SSIP_GLDS_INBN_FD(SSIP_GLDS_ROW, MODE_FWD, GLDS_INBN) SSIP_GLDS_INBN_WG(SSIP_GLDS_ROW, MODE_WGRAD, GLDS_INBN)};
#undef SSIP_GLDS_ROW

static const GldsRow* glds_find(int mode, int form, int bm, int bn, int wmw, int wnw, int stages) {
  for (const GldsRow& r : GLDS_TABLE)
    if (r.mode == mode && r.form == form && bm == r.bm && bn == r.bn && wmw == r.wmw && wnw == r.wnw &&
        stages == r.stages)
      return &r;
  return nullptr;
}

// Register-staged kernel instances: 4 waves over 128 (WGRAD: also 64) rows
// for both dtypes, 8 waves over 256 rows for a bf16 FWD / DGRAD (pick_tile);
// conv1: the C = 4 stem (no DGRAD)
#define SSIP_GEMM_128(X, M, T, C1) X(M, T, 128, 128, 2, 2, C1) X(M, T, 128, 64, 2, 2, C1)
#define SSIP_GEMM_256(X, M, C1) X(M, __bf16, 256, 128, 4, 2, C1) X(M, __bf16, 256, 64, 4, 2, C1)
#define SSIP_GEMM_WG(X, T, C1) SSIP_GEMM_128(X, MODE_WGRAD, T, C1) X(MODE_WGRAD, T, 64, 128, 2, 2, C1)

struct GemmRow {
  int mode, elem_bytes, bm, bn, wmw, wnw;
  bool conv1;
  ConvKernel fn;
};
#define SSIP_GEMM_ROW(M, T, BM_, BN_, WM_, WN_, C1) \
  {M, (int)sizeof(T), BM_, BN_, WM_, WN_, C1, conv_gemm_kernel<M, T, BM_, BN_, WM_, WN_, C1>},
static const GemmRow GEMM_TABLE[] = {
    SSIP_GEMM_128(SSIP_GEMM_ROW, MODE_FWD, __bf16, false) SSIP_GEMM_128(SSIP_GEMM_ROW, MODE_FWD, __bf16, true)
    SSIP_GEMM_128(SSIP_GEMM_ROW, MODE_FWD, float, false) SSIP_GEMM_128(SSIP_GEMM_ROW, MODE_FWD, float, true)
    SSIP_GEMM_256(SSIP_GEMM_ROW, MODE_FWD, false) SSIP_GEMM_256(SSIP_GEMM_ROW, MODE_FWD, true)
    SSIP_GEMM_128(SSIP_GEMM_ROW, MODE_DGRAD, __bf16, false) SSIP_GEMM_128(SSIP_GEMM_ROW, MODE_DGRAD, float, false)
    SSIP_GEMM_256(SSIP_GEMM_ROW, MODE_DGRAD, false)
    SSIP_GEMM_WG(SSIP_GEMM_ROW, __bf16, false) SSIP_GEMM_WG(SSIP_GEMM_ROW, __bf16, true)
    SSIP_GEMM_WG(SSIP_GEMM_ROW, float, false) SSIP_GEMM_WG(SSIP_GEMM_ROW, float, true)};
#undef SSIP_GEMM_ROW

static const GemmRow* gemm_find(int mode, int elem_bytes, int bm, int bn, int wmw, int wnw, bool conv1) {
  for (const GemmRow& r : GEMM_TABLE)
    if (r.mode == mode && r.elem_bytes == elem_bytes && bm == r.bm && bn == r.bn && wmw == r.wmw && wnw == r.wnw &&
        conv1 == r.conv1)
      return &r;
  return nullptr;
}

// A wgrad with a budget (on the side stream) takes 8-wave 256x256 tiles, and
// 8-wave 128x256 tiles where 128 <= K < 256, on WGRAD_BIG_CUS percent of the
// budget's CUs, the rest of the chip left to the main stream; SSIP_WGRAD_BIG=0
// keeps the full-grid tiles.  Round 6, with the stagger (tools/gpu_r6_{i,j,k}.sh,
// alternated runs on one box each, ms/step): on 62 % of the CUs 5.937 vs 6.013
// (4 + 4; 56 % 5.969, 70 % 5.979, 80 % 6.083), 5.933 vs 6.018 on another box;
// the 256x256 tiles alone at 62 % 5.985, on every CU 5.98 vs 5.87
// (profiles/r6_wgrad_big_ab.txt).  Measured and removed: 16-wave 256-column
// tiles -- round 5: faster alone, slower in the step (6.34 vs 6.19 ms), a
// 16-wave workgroup holding every register of its CU keeps the main stream's
// dgrad / BN chain off it.
constexpr int WGRAD_BIG_CUS = 62;

// Default LDS-DMA configuration for a bf16 GEMM view (M x Ng, reduction Kg).
// Chosen from tools/tune_conv.py over the ResNet-18 train-step shapes
// (profiles/r1_conv_tune.txt): two LDS stages and 8-16 waves per workgroup
// beat deeper rings at one workgroup per CU on every shape; 2-3 workgroups
// per CU hide each other's barriers and epilogues.
static void choose_glds(int mode, const ConvArgs& a, Plan& pl) {
  pl.stages = 2;
  if (mode == MODE_WGRAD) {
    // 8 waves of 32x64 (profiles/r2_wgrad_tiles.txt: 3-6 % over 16 waves of 32x32,
    // whose fragment reads load the LDS as much as the MFMAs)
    if (a.M % 128 == 0) { pl.bm = 128; pl.bn = 128; pl.wmw = 4; pl.wnw = 2; }
    else { pl.bm = 64; pl.bn = 128; pl.wmw = 2; pl.wnw = 4; }
    return;
  }
  pl.bm = 128; pl.wmw = 4; pl.wnw = 2;
  pl.bn = (a.Ng % 128 == 0) ? 128 : 64;
  // 256x256 tiles (8 waves of 64x128) where a forward or stride-1 dgrad still
  // has >= 160 of them (ResNet-18 layer3: fwd 62.7 vs 69.1 us,
  // profiles/r1_conv_tune.txt; dgrad 62.4 vs 67.8 us, profiles/r3_tune_fd.txt)
  if ((mode == MODE_FWD || (mode == MODE_DGRAD && a.stride == 1)) && a.Ng % 256 == 0 &&
      (long)ceil_div(a.M, 256) * (a.Ng / 256) >= 160) {
    pl.bm = 256; pl.bn = 256;
  } else if (mode == MODE_FWD && a.Ng % 128 == 0 && (long)ceil_div(a.M, 128) * (a.Ng / 128) <= device_cus()) {
    // at most one 128x128 tile per CU (the weak forward's layer4 at batch 128:
    // 196 tiles): one workgroup of 16 waves (32x32 wave tiles) and a 3-deep
    // ring per CU instead of 8 waves that leave every second slot empty
    // (l4.3x3 42.4 vs 50.2 us, l4.3x3s2 24.1 vs 26.7, profiles/r2_tune_fwd_b128.txt)
    pl.wnw = 4; pl.stages = 3;
  }
}

// Tuning override: SSIP_CONV_FORCE="<f|d|w>,bm,bn,waves_m,waves_n,stages"
// (stages 0 = register-staged kernel) applies to the named pass only.
static int apply_force(const ConvKnobs& k, int mode, int elem_bytes, Plan& pl) {
  const char* e = k.force;
  if (!e || !e[0]) return SSIP_OK;
  if (e[0] != MODE_NAME[mode][0] || (pl.conv1 && !pl.stem_glds)) return SSIP_OK;
  int bm, bn, wm, wn, st;
  SSIP_REQUIRE(sscanf(e + 1, ",%d,%d,%d,%d,%d", &bm, &bn, &wm, &wn, &st) == 5, SSIP_ERR_ARG,
               "bad SSIP_CONV_FORCE '%s'", e);
  if (st > 0) {
    const int form = (mode == MODE_FWD && pl.conv1) ? GLDS_STEM : GLDS_PLAIN;
    SSIP_REQUIRE(elem_bytes == 2 && glds_find(mode, form, bm, bn, wm, wn, st), SSIP_ERR_ARG,
                 "SSIP_CONV_FORCE: no LDS-DMA kernel %s", e);
  } else {
    // not a gemm_find: this accepts a 64x64 wgrad tile, which GEMM_TABLE does not
    // hold (the launch then reports "no wgrad kernel for tile 64x64"); every
    // other answer is the table's
    const bool ok = mode == MODE_WGRAD ? (wm == 2 && wn == 2 && (bm == 128 || bm == 64))
                                       : ((bm == 256 && wm == 4 && wn == 2 && elem_bytes == 2) ||
                                          (bm == 128 && wm == 2 && wn == 2));
    SSIP_REQUIRE(ok && (bn == 128 || bn == 64), SSIP_ERR_ARG, "SSIP_CONV_FORCE: no register-staged kernel %s", e);
  }
  pl.bm = bm; pl.bn = bn; pl.wmw = wm; pl.wnw = wn; pl.stages = st;
  return SSIP_OK;
}

// SSIP_STAGGER: a bit mask over the passes whose LDS-DMA ring kernels run the stagger
// (conv_glds_kernel: waves NW/2.. one MFMA half behind), 1 fwd, 2 dgrad,
// 4 wgrad; 0 off; default 7 (round 6, tools/stagger_lab.py, batch 256, same
// bits: the layer 2-4 launches -3.8 % in sum, the 256x256 layer-3 fwd /
// dgrad -11 to -13 %, the side stream's one-workgroup-per-CU wgrads -4 to
// -6 %; step 6.076 -> 6.045 ms, 3 + 3 alternated runs,
// profiles/r6_stagger_lab.txt).
static int stagger_for(const ConvKnobs& k, int mode, const Plan& pl) {
  if (pl.stages <= 0 || pl.conv1) return 0;
  return (k.stagger >> mode) & 1;
}

static int plan_conv(const ConvKnobs& k, int mode, const ssip_conv_desc* d, int elem_bytes, Plan& pl,
                     int wg_budget = 0, bool allow_big = true) {
  SSIP_REQUIRE(desc_ok(d), SSIP_ERR_ARG, "bad conv descriptor");
  pl.mode = mode;
  pl.conv1 = (d->C == 4);
  // the padded stem stores S = 8 columns for a real 7-wide filter
  const int s_real = pl.conv1 ? d->S - 1 : d->S;
  SSIP_REQUIRE(d->P == (d->H + 2 * d->pad - d->R) / d->stride + 1 && d->Q == (d->W + 2 * d->pad - s_real) / d->stride + 1,
               SSIP_ERR_ARG, "P/Q inconsistent with H/W/R/S/stride/pad");
  const int BK = elem_bytes == 2 ? 64 : 32;
  SSIP_REQUIRE(pl.conv1 ? (d->S == 8) : (d->C % BK == 0), SSIP_ERR_ARG,
               "conv input channels must be a multiple of %d (or 4 with S padded to 8); got C=%d S=%d", BK, d->C,
               d->S);
  SSIP_REQUIRE(d->K % BK == 0, SSIP_ERR_ARG, "conv output channels must be a multiple of %d; got K=%d", BK, d->K);
  const long NPQ = (long)d->N * d->P * d->Q, NHW = (long)d->N * d->H * d->W;
  SSIP_REQUIRE(NPQ < (1l << 31) && NHW * d->C < (1l << 31) && NPQ * d->K < (1l << 31), SSIP_ERR_ARG,
               "tensor too large for 32-bit indexing");
  ConvArgs& a = pl.args;
  fill_common(a, d);
  pl.splits = 1;
  if (mode == MODE_FWD) {
    a.M = (int)NPQ; a.Ng = d->K; a.Kg = d->R * d->S * d->C;
    a.ksteps = ceil_div(a.Kg, BK);
    pick_tile(a.M, a.Ng, elem_bytes, pl);
  } else if (mode == MODE_DGRAD) {
    SSIP_REQUIRE(!pl.conv1, SSIP_ERR_ARG, "dgrad of the C=4 stem conv is not supported (input needs no grad)");
    SSIP_REQUIRE(d->stride == 1 || d->stride == 2 || d->stride == 4, SSIP_ERR_ARG, "dgrad stride must be 1, 2 or 4");
    a.M = (int)NHW; a.Ng = d->C; a.Kg = d->R * d->S * d->K;
    a.ksteps = a.Kg / BK;
    pick_tile(a.M, a.Ng, elem_bytes, pl);
  } else {
    a.M = d->K; a.Ng = d->R * d->S * d->C; a.Kg = 0;
    a.Mred = (int)NPQ;
    pl.wmw = 2; pl.wnw = 2;
    pl.bm = (d->K % 128 == 0) ? 128 : 64;
    pl.bn = 128;
    if (a.Ng % 128 != 0 && a.Ng % 64 == 0 && pl.bm == 128) pl.bn = 64;
  }
  pl.stages = 0;
  pl.stem_glds = pl.conv1 && d->pad == 0 && d->W % 2 == 0 && d->S == 8;
  if (elem_bytes == 2 && (!pl.conv1 || pl.stem_glds)) choose_glds(mode, a, pl);
  // a wgrad sharing the chip at one workgroup per CU (ssip_conv_wgrad_budget):
  // 8-wave 128x128 workgroups alone on a CU wait on their own barriers and
  // LDS-DMA (18 % MFMA busy, 59 % of wave cycles parked); 16-wave
  // workgroups of 256 columns hide that and halve the DMA bytes per FLOP
  // (tools/wgrad_lab.py at the 256-workgroup budget, profiles/r5_wgrad_lab.txt:
  // l2.3x3 110.9 -> 89.1 us with 128x256, l3.3x3 109.9 -> 73.9 and l4.3x3
  // 101.4 -> 75.4 with 256x256) -- but not in the step (WGRAD_BIG_CUS)
  // (round 5 also measured 8-wave 128x256 tiles at the budget -- two waves
  // per SIMD, 96 KiB of LDS, so not the whole CU: 517.6 -> 461.1 us over the
  // six layer 2-4 wgrads, but the step 6.14 -> 6.43 ms, 4 + 4 runs)
  if (mode == MODE_WGRAD && wg_budget > 0 && pl.stages > 0 && !pl.conv1 && allow_big && k.wgrad_big) {
    // (the 1x1 downsample wgrads, Ng <= 256, keep their many-tile grids)
    if (a.M % 256 == 0 && a.Ng % 256 == 0 && a.Ng >= 512) {
      // the 8-wave 256x256 tile (with the stagger: l3 / l4 3x3 wgrads at the
      // budget 98 -> 73 us, profiles/r6_tile_lab.txt)
      pl.bm = 256; pl.bn = 256; pl.wmw = 4; pl.wnw = 2;
    } else if (a.M % 128 == 0 && a.Ng >= 512) {
      pl.bm = 128; pl.bn = 256; pl.wmw = 2; pl.wnw = 4;  // 8 waves, 96 KiB of LDS; a partial last tile where Ng % 256 != 0
    }
    // on WGRAD_BIG_CUS percent of the budget's CUs, the rest left to the
    // main stream (measured: profiles/r6_tile_lab.txt)
    if (pl.bn == 256) wg_budget = std::max(1, wg_budget * WGRAD_BIG_CUS / 100);
  }
  if (int rc = apply_force(k, mode, elem_bytes, pl)) return rc;
  if (mode == MODE_WGRAD) {
    const int tiles = ceil_div(a.M, pl.bm) * ceil_div(a.Ng, pl.bn);
    const int total_ks = ceil_div(a.Mred, BK);
    // split count: every split is one more fp32 slab written here and read by
    // the reduce; the grid should end on a full wave of resident workgroups
    // (a launch of 540 workgroups on 512 slots runs two waves for 5 % more
    // work).  Cost in k-step times: waves * k-steps per split + the slab
    // round trip (~0.27 k-step per MiB, tools/tune_wgrad_splits.py);
    // slab <= 64 MiB, >= 16 k-steps per split.
    const long slab_split = (long)a.M * a.Ng * 4;
    const int cap_bytes = (int)std::max<long>(1, (64l << 20) / slab_split);
    const int max_splits = std::max(1, std::min(cap_bytes, total_ks / 16));
    int splits = 1;
    if (k.wgrad_blocks > 0) {  // tuning override: target workgroup count
      splits = std::min(max_splits, ceil_div(k.wgrad_blocks, tiles));
    } else if (pl.stages > 0 && wg_budget > 0) {
      // a wgrad sharing the chip (ssip_conv_wgrad_budget): ResNet-18 train
      // step with the side-stream wgrads at one workgroup per CU, two A/Bs of
      // 3 + 3 alternated runs: 6.341 vs 6.369 and 6.431 vs 6.490 ms/step
      // (the main stream's BN-backward passes wait less for wgrad workgroups
      // to retire, and half the split slabs move through HBM)
      // a kernel that fits one workgroup per CU (LDS > 80 KiB): at most
      // `budget` workgroups (one more would run a second round on its CU);
      // the 2-per-CU tiles round up (an extra workgroup shares a CU)
      const int lds = std::max(2, pl.stages) * 64 * (pl.bm + pl.bn) * 2;
      splits = std::min(max_splits, lds > 81920 ? std::max(1, wg_budget / tiles) : ceil_div(wg_budget, tiles));
    } else if (pl.stages > 0) {
      const int nt = 64 * pl.wmw * pl.wnw;
      const int nbuf = std::max(2, pl.stages);
      const int lds = nbuf * 64 * (pl.bm + pl.bn) * 2;
      const int per_cu = std::max(1, std::min(2048 / nt, 163840 / lds));
      const long slots = (long)device_cus() * per_cu;
      double best = 1e30;
      for (int s = 1; s <= max_splits; ++s) {
        const long waves = ((long)tiles * s + slots - 1) / slots;
        const double cost = (double)waves * ceil_div(total_ks, s) + 0.27 * s * (double)slab_split / (1 << 20);
        if (cost < best - 1e-9) { best = cost; splits = s; }
      }
    } else {
      splits = std::min(max_splits, ceil_div(1024, tiles));
    }
    if (splits < 1) splits = 1;
    a.ksteps = ceil_div(total_ks, splits);
    splits = ceil_div(total_ks, a.ksteps);
    pl.splits = splits;
  }
  a.tiles_n = ceil_div(a.Ng, pl.bn);
  const int tiles_m = ceil_div(a.M, pl.bm);
  pl.grid = dim3(tiles_m * a.tiles_n, pl.splits, 1);
  a.xcd_remap = 1;
  a.stagger = stagger_for(k, mode, pl);
  return SSIP_OK;
}

// the ring kernel's form follows from the operands the entry point has set
static int glds_form(const Plan& pl) {
  const ConvArgs& a = pl.args;
  if (pl.mode != MODE_DGRAD && a.in_scale != nullptr) return GLDS_INBN;
  if (pl.mode == MODE_DGRAD && a.pmean != nullptr) return GLDS_POST;  // fused BN-backward epilogue
  if (pl.mode == MODE_FWD && a.bias != nullptr) return GLDS_FOLD;     // folded eval BN epilogue
  if (pl.mode == MODE_FWD && pl.conv1) return GLDS_STEM;
  return GLDS_PLAIN;
}

static int launch_glds(const Plan& pl, hipStream_t st) {
  const int form = glds_form(pl);
  const GldsRow* r = glds_find(pl.mode, form, pl.bm, pl.bn, pl.wmw, pl.wnw, pl.stages);
  SSIP_REQUIRE(r != nullptr, SSIP_ERR_ARG, "no %s kernel for %dx%d/%dx%d/%d", GLDS_FORMS[form].what, pl.bm, pl.bn,
               pl.wmw, pl.wnw, pl.stages);
  SSIP_KLAUNCH(r->fn, pl.grid, dim3(64 * r->wmw * r->wnw), 0, st, pl.args);
  return ::ssip::check_launch(GLDS_FORMS[form].check);
}

static int launch_conv(const Plan& pl, int dtype, hipStream_t st) {
  SSIP_REQUIRE(dtype == SSIP_F32 || dtype == SSIP_BF16, SSIP_ERR_ARG, "unsupported dtype %d", dtype);
  if (dtype == SSIP_BF16 && pl.stages > 0) return launch_glds(pl, st);
  const GemmRow* r = gemm_find(pl.mode, elem_bytes_of(dtype), pl.bm, pl.bn, pl.wmw, pl.wnw, pl.conv1);
  SSIP_REQUIRE(r != nullptr, SSIP_ERR_ARG, "no %s kernel for tile %dx%d", MODE_NAME[pl.mode], pl.bm, pl.bn);
  SSIP_KLAUNCH(r->fn, pl.grid, dim3(64 * r->wmw * r->wnw), 0, st, pl.args);
  return ::ssip::check_launch("conv_gemm");
}

// Operand pointers and buffer-descriptor byte sizes of the implicit-GEMM
// kernels: FWD x and w_krsc, DGRAD dy and w_crsk, WGRAD dy and x
static void set_operands(ConvArgs& a, const ssip_conv_desc* d, int mode, const void* A, const void* B) {
  const long x_bytes = (long)d->N * d->H * d->W * d->C * 2, dy_bytes = (long)d->N * d->P * d->Q * d->K * 2;
  const long w_bytes = (long)d->K * d->R * d->S * d->C * 2;
  a.A = A; a.B = B;
  a.a_bytes = (uint32_t)(mode == MODE_FWD ? x_bytes : dy_bytes);
  a.b_bytes = (uint32_t)(mode == MODE_WGRAD ? x_bytes : w_bytes);
}

// Register-staged kernel for a FWD/DGRAD GEMM view the LDS-DMA kernel does not
// address: the strided DGRAD without its phase split, filters of > 32 taps.
static void fallback_regstaged(Plan& pl) {
  ConvArgs& a = pl.args;
  pl.stages = 0;
  a.phased = 0;
  pick_tile(a.M, a.Ng, 2, pl);
  a.tiles_n = ceil_div(a.Ng, pl.bn);
  pl.grid = dim3(ceil_div(a.M, pl.bm) * a.tiles_n, 1, 1);
}

// phases by k-steps, descending (ties in phase order): the kernel hands them
// out in this order within each tile, so the long phases start first
static void set_phase_order(ConvArgs& a) {
  int ord[4] = {0, 1, 2, 3};
  std::stable_sort(ord, ord + 4, [&](int x, int y) { return a.phase[x].ksteps > a.phase[y].ksteps; });
  a.phase_order = ord[0] | (ord[1] << 2) | (ord[2] << 4) | (ord[3] << 6);
}

// Stride-2 DGRAD as four dense sub-problems, one per output parity phase:
// phase (ph, pw) only meets the taps r = r0 + 2*ri, s = s0 + 2*si, so the
// k-loop skips the 3/4 of (tap, pixel) pairs the plain implicit GEMM would
// gather as zeros.  blockIdx.y = phase; grid.x covers the largest phase.
static void phase_split(Plan& pl, const ssip_conv_desc* d) {
  if (pl.stages == 0 || pl.conv1 || d->stride != 2) return;
  ConvArgs& a = pl.args;
  int max_tiles = 0;
  for (int f = 0; f < 4; ++f) {
    PhaseInfo& P = a.phase[f];
    P.ph = f >> 1;
    P.pw = f & 1;
    const int Hph = (d->H - P.ph + 1) / 2, Wph = (d->W - P.pw + 1) / 2;
    P.r0 = (P.ph + d->pad) % 2;
    P.s0 = (P.pw + d->pad) % 2;
    P.nr = P.r0 < d->R ? (d->R - P.r0 + 1) / 2 : 0;
    P.ns = P.s0 < d->S ? (d->S - P.s0 + 1) / 2 : 0;
    P.bh = (P.ph + d->pad - P.r0) / 2;
    P.bw = (P.pw + d->pad - P.s0) / 2;
    P.Wph = Wph;
    P.M = d->N * Hph * Wph;
    P.tiles_m = ceil_div(P.M, pl.bm);
    P.ksteps = P.nr * P.ns * (d->K / 64);
    P.div_hw = make_fastdiv((uint32_t)std::max(1, Hph * Wph));
    P.div_w = make_fastdiv((uint32_t)std::max(1, Wph));
    max_tiles = std::max(max_tiles, P.tiles_m);
  }
  a.phased = 1;
  set_phase_order(a);
  pl.grid = dim3(std::max(1, max_tiles) * a.tiles_n, 4, 1);
}

// ---- halo path (conv_halo_kernel): 3x3 / stride 1 / pad 1, 64 reduction
// channels, bf16.  SSIP_HALO=0 turns it off; an SSIP_CONV_FORCE for the pass
// selects the implicit-GEMM kernels instead (tools/tune_conv.py).
struct HaloPlan {
  int TR, tiles, units, G, cols;
};

static bool halo_plan(const ConvKnobs& k, int mode, const ssip_conv_desc* d, int dtype, HaloPlan& hp) {
  if (!k.halo_for(MODE_NAME[mode][0])) return false;
  if (dtype != SSIP_BF16 || !desc_ok(d) || d->R != 3 || d->S != 3 || d->stride != 1 || d->pad != 1 ||
      d->P != d->H || d->Q != d->W)
    return false;
  const int redc = mode == MODE_FWD ? d->C : d->K;
  const int cols = mode == MODE_FWD ? d->K : d->C;
  if (redc != 64 || cols % 64 != 0) return false;
  int TR = 0;
  for (int tr = std::min(d->H, 256 / (d->W + 2)); tr >= 1; --tr)  // TR (W+2) GEMM rows <= 256
    if (d->H % tr == 0 && (tr + 2) * (d->W + 2) <= HALO_XBUF / 128) {
      TR = tr;
      break;
    }
  if (TR == 0 || TR * d->W < 128) return false;  // short tiles: the implicit-GEMM kernels do better
  const long pix = (long)d->N * d->H * d->W;
  if (pix * 64 * 2 >= (1l << 31) || pix * cols * 2 >= (1l << 31)) return false;
  hp.TR = TR;
  hp.cols = cols;
  hp.tiles = (int)((long)d->N * d->H / TR);
  hp.units = hp.tiles * (cols / 64);
  // persistent: one workgroup per CU
  hp.G = std::min(hp.units, device_cus());
  return true;
}

// ---- stem path (conv_stem_halo_kernel): the pre-padded 7x7 / stride 2 stem
static bool stem_plan(const ConvKnobs& k, const ssip_conv_desc* d, int dtype, HaloPlan& hp) {
  if (!k.halo_for('f')) return false;
  if (dtype != SSIP_BF16 || !desc_ok(d) || d->C != 4 || d->R != 7 || d->S != 8 || d->stride != 2 || d->pad != 0 ||
      d->K % 64 != 0 || d->Q > STEM_QP || d->P % STEM_TR != 0 || d->W % 2 != 0 ||
      STEM_XROWS * d->W * 8 > STEM_XBUF || d->H < 2 * (d->P - 1) + 7)
    return false;
  const long ib = (long)d->N * d->H * d->W * 8, ob = (long)d->N * d->P * d->Q * d->K * 2;
  if (ib >= (1l << 31) || ob >= (1l << 31)) return false;
  hp.TR = STEM_TR;
  hp.cols = d->K;
  hp.tiles = d->N * d->P / STEM_TR;
  hp.units = hp.tiles * (d->K / 64);
  hp.G = std::min(hp.units, 2 * device_cus());  // 62 KiB of LDS: two workgroups per CU
  return true;
}

// ---- halo WGRAD (conv_halo_wgrad_kernel): 3x3 / stride 1 / pad 1, C = K = 64, bf16
static bool halo_wg_plan(const ConvKnobs& k, const ssip_conv_desc* d, int dtype, HaloPlan& hp) {
  if (!k.halo_for('w')) return false;
  if (dtype != SSIP_BF16 || !desc_ok(d) || d->R != 3 || d->S != 3 || d->stride != 1 || d->pad != 1 ||
      d->P != d->H || d->Q != d->W || d->C != 64 || d->K != 64)
    return false;
  const int Wp = d->W + 2;
  if (256 + 2 * Wp + 2 > HWG_XBUF / 128) return false;  // shifted reads stay inside the input image
  int TR = 0;
  for (int tr = std::min(d->H, 256 / Wp); tr >= 1; --tr)
    if (d->H % tr == 0 && (tr + 2) * Wp <= HWG_XBUF / 128) {
      TR = tr;
      break;
    }
  if (TR == 0 || TR * d->W < 128) return false;
  if ((long)d->N * d->H * d->W * 64 * 2 >= (1l << 31)) return false;
  hp.TR = TR;
  hp.cols = 576;  // slab columns: 3 x 3 x 64
  hp.tiles = d->N * d->H / TR;
  hp.units = hp.tiles;
  hp.G = std::min(hp.tiles, device_cus());
  return true;
}

// ---- stem WGRAD (conv_stem_wgrad_kernel)
static bool stem_wg_plan(const ConvKnobs& k, const ssip_conv_desc* d, int dtype, HaloPlan& hp) {
  if (!k.halo_for('w')) return false;
  if (!stem_plan(k, d, dtype, hp) || d->K != 64) return false;  // same geometry as the forward's kernel
  hp.cols = 224;  // slab columns: 7 x 8 x 4
  hp.G = std::min(hp.tiles, device_cus());
  hp.units = hp.tiles;
  return true;
}

// ---- routes: what one call runs
enum RouteKind {
  ROUTE_NONE,        // no kernel takes this descriptor (the route function's return value says why)
  ROUTE_HALO,        // conv_halo_kernel (FWD / DGRAD): hp
  ROUTE_STEM,        // conv_stem_halo_kernel (FWD): hp
  ROUTE_GLDS,        // conv_glds_kernel: pl
  ROUTE_REGSTAGED,   // conv_gemm_kernel: pl
  ROUTE_HALO_WGRAD,  // conv_halo_wgrad_kernel + slab reduce: hp
  ROUTE_STEM_WGRAD   // conv_stem_wgrad_kernel / conv_stem_bwd_wgrad2_kernel + slab reduce: hp
};
struct ConvRoute {
  int kind = ROUTE_NONE;
  Plan pl;      // the implicit-GEMM plan (for a WGRAD also beside a persistent kind: ssip_conv_wgrad_budget)
  HaloPlan hp;  // a persistent kernel's grid
  bool persistent_fwd() const { return kind == ROUTE_HALO || kind == ROUTE_STEM; }
  bool persistent_wgrad() const { return kind == ROUTE_HALO_WGRAD || kind == ROUTE_STEM_WGRAD; }
};

static int implicit_kind(const Plan& pl) { return pl.stages > 0 ? ROUTE_GLDS : ROUTE_REGSTAGED; }

// The route functions return plan_conv's verdict on the descriptor, which a
// launch returns before anything else.  The kind is set wherever a kernel's
// own test takes the geometry: the stem kernels' does not compare P with H,
// so on such a descriptor the queries answer for them and the launch fails.

// FWD: the halo kernel, the stem kernel, else the implicit GEMM
static int route_fwd(const ConvKnobs& k, const ssip_conv_desc* d, int dtype, ConvRoute& r) {
  const int rc = plan_conv(k, MODE_FWD, d, elem_bytes_of(dtype), r.pl);
  if (halo_plan(k, MODE_FWD, d, dtype, r.hp)) {
    r.kind = ROUTE_HALO;
  } else if (stem_plan(k, d, dtype, r.hp)) {
    r.kind = ROUTE_STEM;
  } else if (rc == SSIP_OK) {
    if (r.pl.stages > 0 && !r.pl.conv1 && d->R * d->S > 32) fallback_regstaged(r.pl);
    r.kind = implicit_kind(r.pl);
  }
  return rc;
}

// DGRAD: the halo kernel, else the implicit GEMM, stride 2 split by phase.
// bn_fused (ssip_conv_dgrad_bn's epilogue): no phase split, and the ring
// kernel at its 128-row tiles, the only ones the epilogue is built for
// (SSIP_CONV_FORCE for the pass aside).
static int route_dgrad(const ConvKnobs& k, const ssip_conv_desc* d, int dtype, ConvRoute& r, bool bn_fused = false) {
  Plan& pl = r.pl;
  if (int rc = plan_conv(k, MODE_DGRAD, d, elem_bytes_of(dtype), pl)) return rc;
  if (halo_plan(k, MODE_DGRAD, d, dtype, r.hp)) {
    r.kind = ROUTE_HALO;
    return SSIP_OK;
  }
  if (!bn_fused) phase_split(pl, d);
  if (pl.stages > 0 && ((d->stride != 1 && !pl.args.phased) || d->R * d->S > 32)) fallback_regstaged(pl);
  if (bn_fused && pl.stages > 0 && !k.force) {
    pl.bm = 128; pl.wmw = 4; pl.wnw = 2; pl.stages = 2;
    pl.bn = (pl.args.Ng % 128 == 0) ? 128 : 64;
    pl.args.tiles_n = ceil_div(pl.args.Ng, pl.bn);
    pl.grid = dim3(ceil_div(pl.args.M, pl.bm) * pl.args.tiles_n, 1, 1);
  }
  SSIP_REQUIRE(!bn_fused || pl.bm >= 128, SSIP_ERR_ARG, "ssip_conv_dgrad_bn: partial sizing assumes >= 128-row tiles");
  r.kind = implicit_kind(pl);
  return SSIP_OK;
}

// WGRAD under a workgroup budget (0: none): the stem kernel, the halo kernel
// (persistent: a budget means fewer workgroups, more tiles each), else the
// split-K implicit GEMM
static int route_wgrad(const ConvKnobs& k, const ssip_conv_desc* d, int dtype, int budget, ConvRoute& r) {
  const int rc = plan_conv(k, MODE_WGRAD, d, elem_bytes_of(dtype), r.pl, budget);
  if (stem_wg_plan(k, d, dtype, r.hp)) r.kind = ROUTE_STEM_WGRAD;
  else if (halo_wg_plan(k, d, dtype, r.hp)) r.kind = ROUTE_HALO_WGRAD;
  else if (rc == SSIP_OK) r.kind = implicit_kind(r.pl);
  if (r.persistent_wgrad() && budget > 0) r.hp.G = std::min(r.hp.G, budget);
  return rc;
}

// BN records per channel the route's kernel writes: one per (workgroup, wave
// row) of a persistent kernel, one per row tile of the implicit GEMM; -1: no route
static int route_records(const ConvRoute& r) {
  if (r.kind == ROUTE_NONE) return -1;
  return r.persistent_fwd() ? r.hp.G * HALO_WMW : ceil_div(r.pl.args.M, r.pl.bm);
}

// fp32 slab bytes of a wgrad: one M x Ng slab per split / per persistent workgroup
static int64_t implicit_slab_bytes(const Plan& pl) { return (int64_t)pl.splits * pl.args.M * pl.args.Ng * 4; }
static int64_t persistent_slab_bytes(const HaloPlan& hp) { return (int64_t)hp.G * 64 * hp.cols * 4; }

// A 3x3 / pad-1 / stride-s conv and its block's 1x1 / pad-0 / stride-s
// downsample over the same input and output grid: one LDS-DMA launch when the
// conv takes a 2- or 3-stage ring kernel (else false: two launches).
static bool fwd_ds_plan(const ConvKnobs& k, const ssip_conv_desc* d, const ssip_conv_desc* dds, int dtype,
                        ConvRoute& r) {
  if (dtype != SSIP_BF16 || !desc_ok(d) || !desc_ok(dds) || k.no_fwd_dsfuse) return false;
  if (d->R != 3 || d->S != 3 || d->pad != 1 || dds->R != 1 || dds->S != 1 || dds->pad != 0 ||
      dds->stride != d->stride || dds->N != d->N || dds->H != d->H || dds->W != d->W || dds->C != d->C ||
      dds->K != d->K || dds->P != d->P || dds->Q != d->Q || d->C % 64 != 0)
    return false;
  return route_fwd(k, d, dtype, r) == SSIP_OK && r.kind == ROUTE_GLDS && !r.pl.conv1 &&
         (r.pl.stages == 2 || r.pl.stages == 3);
}

// ssip_conv_*_bnrelu_in beyond the layer-1 halo geometry: the LDS-DMA ring
// kernels with the INBN operand transform, for bf16 stride-1 convs with
// 64 <= C <= GLDS_INBN_C input channels -- 1x1 / pad 0 (the ResNet-50
// bottleneck's conv3 over relu(bn2(y2))) with SSIP_BNRELU_GLDS bit 0, 3x3 /
// pad 1 with bit 1.  The transform keeps padding taps, rows past the grid
// and split tails zero.
// SSIP_BNRELU_GLDS: bit 0 the 1x1 / stride-1 form (default on: config 5,
// 60.23 vs 60.60 ms/step with the forward's z_out, profiles/r6_bnrelu_in_glds_lab.txt),
// bit 1 the 3x3 form (off: slower in both steps)
static bool glds_inbn_plan(const ConvKnobs& k, int mode, const ssip_conv_desc* d, int dtype, Plan& pl,
                           int budget = 0) {
  if (dtype != SSIP_BF16 || !desc_ok(d) || d->stride != 1 || d->C % 64 || d->C > GLDS_INBN_C || d->K % 64)
    return false;
  // the 1x1 form pays where the apply pass it removes is large: per launch it
  // wins at ResNet-50 layers 1-2 (>= 262,144 rows) and loses at layers 3-4,
  // where the conv is short and the in-ring transform is not hidden
  // (profiles/r6_bnrelu_in_glds_lab.txt); SSIP_BNRELU_GLDS_MINM overrides
  if (d->R == 1 && (long)d->N * d->H * d->W < k.bnrelu_minm) return false;
  const bool g1 = d->R == 1 && d->S == 1 && d->pad == 0 && (k.bnrelu_glds & 1);
  const bool g3 = d->R == 3 && d->S == 3 && d->pad == 1 && (k.bnrelu_glds & 2);
  if (!g1 && !g3) return false;
  ConvRoute rf;
  const int rc_fwd = route_fwd(k, d, dtype, rf);
  if (rf.kind == ROUTE_HALO) return false;  // the halo geometry has its own BN+ReLU-in kernels
  if (mode == MODE_FWD) {
    if (rc_fwd) return false;
    pl = rf.pl;
  } else if (plan_conv(k, mode, d, 2, pl, budget, false) != SSIP_OK) {
    // (the wide budget tiles of SSIP_WGRAD_BIG have no INBN form: the budget's plain tiles)
    return false;
  }
  if (pl.conv1 || pl.stages != 2) return false;
  return glds_find(mode, GLDS_INBN, pl.bm, pl.bn, pl.wmw, pl.wnw, pl.stages) != nullptr;
}

// BN+ReLU-in support: forward and wgrad both on the halo kernels (rf, rw), or
// both on an INBN ring kernel (rf.pl: the forward's plan)
static bool bnrelu_in_routes(const ConvKnobs& k, const ssip_conv_desc* d, int dtype, ConvRoute& rf, ConvRoute& rw) {
  route_fwd(k, d, dtype, rf);
  route_wgrad(k, d, dtype, 0, rw);
  if (rf.kind == ROUTE_HALO && rw.kind == ROUTE_HALO_WGRAD) return true;
  return glds_inbn_plan(k, MODE_FWD, d, dtype, rf.pl) && glds_inbn_plan(k, MODE_WGRAD, d, dtype, rw.pl);
}

// the fused stem backward (conv_stem_bwd_wgrad2_kernel): the stem wgrad's geometry at Q = 112
static bool stem_bwd_route(const ConvKnobs& k, const ssip_conv_desc* d, int dtype, ConvRoute& r) {
  route_wgrad(k, d, dtype, 0, r);
  return r.kind == ROUTE_STEM_WGRAD && d->Q * 2 == 224 && d->P % 2 == 0;
}

// ---- launches
static int launch_stem_halo(const ssip_conv_desc* d, const HaloPlan& hp, const void* X, const void* Wt, void* out,
                            float* partial, hipStream_t st) {
  StemArgs s;
  s.X = static_cast<const __bf16*>(X);
  s.Wt = static_cast<const __bf16*>(Wt);
  s.out = static_cast<__bf16*>(out);
  s.partial = partial;
  s.x_bytes = (uint32_t)((long)d->N * d->H * d->W * 8);
  s.w_bytes = (uint32_t)((long)d->K * 7 * 8 * 4 * 2);
  s.o_bytes = (uint32_t)((long)d->N * d->P * d->Q * d->K * 2);
  s.N = d->N; s.H = d->H; s.W = d->W; s.P = d->P; s.Q = d->Q; s.Ncols = d->K;
  s.tiles = hp.tiles; s.units = hp.units;
  SSIP_KLAUNCH((conv_stem_halo_kernel<4, 2>), dim3(hp.G), dim3(512), 0, st, s);
  return ::ssip::check_launch("conv_stem_halo");
}

struct HaloBnPost {
  const void* y;
  const uint8_t* bits;
  const float *mean, *invstd, *mscale, *mshift;
};

// 8 waves of 64x32 (16 waves of 32x32 were ~10 % faster in isolation but 3 %
// slower in the step, where the side streams' kernels run beside them; 4
// waves of 64x64 slower still: r3-variants branch)
typedef void (*HaloKernel)(const HaloArgs);
static HaloKernel halo_kernel(bool inbn, int bnpost, bool bias, bool add) {
  if (inbn) return conv_halo_kernel<4, 2, false, 0, false, true>;  // FWD over relu(bn(y)) of the layer below, formed in LDS
  if (bnpost == 1) return conv_halo_kernel<4, 2, false, 1>;        // DGRAD + BN-backward reduction
  if (bnpost == 2) return conv_halo_kernel<4, 2, false, 2>;        // ... with a residual gradient or mask bits
  if (bias) return add ? conv_halo_kernel<4, 2, true, 0, true> : conv_halo_kernel<4, 2, true>;  // folded eval BN epilogue
  return add ? conv_halo_kernel<4, 2, false, 0, true> : conv_halo_kernel<4, 2>;
}

static int launch_halo(int mode, const ssip_conv_desc* d, const HaloPlan& hp, const void* X, const void* Wt,
                       void* out, const void* add, float* partial, hipStream_t st, const float* bias = nullptr,
                       int relu = 0, const HaloBnPost* bp = nullptr, const float* in_scale = nullptr,
                       const float* in_shift = nullptr, void* zout = nullptr) {
  HaloArgs h;
  memset(&h, 0, sizeof(h));
  if (bp) {
    h.py = static_cast<const __bf16*>(bp->y);
    h.pbits = bp->bits;
    h.pmean = bp->mean; h.pinvstd = bp->invstd; h.pmscale = bp->mscale; h.pmshift = bp->mshift;
    h.bits_bytes = (uint32_t)((long)d->N * d->H * d->W * hp.cols / 8);
  }
  h.bias = bias;
  h.relu = relu;
  h.X = static_cast<const __bf16*>(X);
  h.Wt = static_cast<const __bf16*>(Wt);
  h.out = static_cast<__bf16*>(out);
  h.add = static_cast<const __bf16*>(add);
  h.partial = partial;
  h.x_bytes = (uint32_t)((long)d->N * d->H * d->W * 64 * 2);
  h.w_bytes = (uint32_t)((long)hp.cols * 9 * 64 * 2);
  h.o_bytes = (uint32_t)((long)d->N * d->H * d->W * hp.cols * 2);
  h.N = d->N; h.H = d->H; h.W = d->W; h.Ncols = hp.cols;
  h.TR = hp.TR; h.tiles = hp.tiles; h.units = hp.units;
  h.flip = mode == MODE_DGRAD ? 1 : 0;
  h.in_scale = in_scale;
  h.in_shift = in_shift;
  h.zout = static_cast<__bf16*>(zout);
  const int bnpost = bp == nullptr ? 0 : (add == nullptr && bp->bits == nullptr) ? 1 : 2;
  SSIP_KLAUNCH(halo_kernel(in_scale != nullptr, bnpost, bias != nullptr, add != nullptr), dim3(hp.G), dim3(512), 0,
               st, h);
  return ::ssip::check_launch("conv_halo");
}

// The fixed-order reduce of `splits` fp32 slabs [K][Ng] (Ng = R * S * C stored
// columns: C % 32 == 0, or the stem's 7 x 8 x 4) into dw [K][c_real][R][s_real]
static int launch_slab_reduce(const void* slab, int splits, int K, int Ng, int c_real, int R, int s_real, int C,
                              int S, float* dw_kcrs, int accumulate, hipStream_t st) {
  const long total4 = (long)K * Ng / 4;
  int lg = 0;  // split groups: double while splits allow and the grid stays within ~1024 workgroups
  while (lg < 6 && (2 << lg) <= splits && ((total4 << (lg + 1)) + 255) / 256 <= 1024) ++lg;
  const long blocks = (total4 + (256 >> lg) - 1) / (256 >> lg);
  SSIP_KLAUNCH(wgrad_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const float*)slab, splits, K, Ng,
               c_real, R, s_real, C, S, dw_kcrs, accumulate, lg);
  return ::ssip::check_launch("wgrad_reduce");
}

// layer-1 WGRAD on conv_halo_wgrad_kernel + its slab reduce (in_scale: the
// input is y of the BN+ReLU below, transformed in LDS)
static int launch_halo_wgrad(const ssip_conv_desc* d, const HaloPlan& hp, const void* dy, const void* x,
                             float* dw_kcrs, int c_real, int s_real, int accumulate, void* workspace,
                             int64_t workspace_bytes, hipStream_t st, const float* in_scale, const float* in_shift) {
  const int64_t hneed = persistent_slab_bytes(hp);
  SSIP_REQUIRE(workspace_bytes >= hneed, SSIP_ERR_WORKSPACE, "wgrad workspace too small: %lld < %lld",
               (long long)workspace_bytes, (long long)hneed);
  HaloWgArgs h;
  h.X = static_cast<const __bf16*>(x);
  h.DY = static_cast<const __bf16*>(dy);
  h.slab = static_cast<float*>(workspace);
  h.x_bytes = (uint32_t)((long)d->N * d->H * d->W * 64 * 2);
  h.N = d->N; h.H = d->H; h.W = d->W; h.TR = hp.TR; h.tiles = hp.tiles;
  h.in_scale = in_scale;
  h.in_shift = in_shift;
  SSIP_KLAUNCH(in_scale != nullptr ? conv_halo_wgrad_kernel<true> : conv_halo_wgrad_kernel<false>, dim3(hp.G),
               dim3(512), 0, st, h);
  if (int rc = ::ssip::check_launch("conv_halo_wgrad")) return rc;
  return launch_slab_reduce(workspace, hp.G, 64, hp.cols, c_real, 3, s_real, 64, 3, dw_kcrs, accumulate, st);
}

// the stem's WGRAD on conv_stem_wgrad_kernel + its slab reduce
static int launch_stem_wgrad(const ssip_conv_desc* d, const HaloPlan& hp, const void* dy, const void* x,
                             float* dw_kcrs, int c_real, int s_real, int accumulate, void* workspace,
                             int64_t workspace_bytes, hipStream_t st) {
  const int64_t sneed = persistent_slab_bytes(hp);
  SSIP_REQUIRE(workspace_bytes >= sneed, SSIP_ERR_WORKSPACE, "wgrad workspace too small: %lld < %lld",
               (long long)workspace_bytes, (long long)sneed);
  StemWgArgs h;
  h.X = static_cast<const __bf16*>(x);
  h.DY = static_cast<const __bf16*>(dy);
  h.slab = static_cast<float*>(workspace);
  h.x_bytes = (uint32_t)((long)d->N * d->H * d->W * 8);
  h.dy_bytes = (uint32_t)((long)d->N * d->P * d->Q * 64 * 2);
  h.N = d->N; h.H = d->H; h.W = d->W; h.P = d->P; h.Q = d->Q; h.tiles = hp.tiles;
  SSIP_KLAUNCH(conv_stem_wgrad_kernel, dim3(hp.G), dim3(512), 0, st, h);
  if (int rc = ::ssip::check_launch("conv_stem_wgrad")) return rc;
  return launch_slab_reduce(workspace, hp.G, 64, hp.cols, c_real, d->R, s_real, d->C, d->S, dw_kcrs, accumulate, st);
}

// the split-K implicit-GEMM wgrad of a planned conv + its fixed-order slab
// reduce (ssip_conv_wgrad_budget; ssip_conv_wgrad_bnrelu_in with in_scale set)
static int wgrad_implicit(Plan& pl, const ssip_conv_desc* d, int dtype, const void* dy, const void* x,
                          float* dw_kcrs, int c_real, int s_real, int accumulate, void* workspace, hipStream_t st) {
  ConvArgs& g = pl.args;
  set_operands(g, d, MODE_WGRAD, dy, x);
  g.out = workspace;
  const int PQ = d->P * d->Q, BKr = 64;  // LDS-DMA k-step rows (bf16)
  const int dn = BKr / PQ, rem = BKr % PQ;
  g.wg_dn = dn;
  g.wg_dp = rem / d->Q;
  g.wg_dq = rem % d->Q;
  g.wg_k0 = (dn * d->H * d->W + g.wg_dp * d->stride * d->W + g.wg_dq * d->stride) * d->C * 2;
  g.wg_e1 = (d->stride * d->W - d->Q * d->stride) * d->C * 2;
  g.wg_e2 = (d->H * d->W - d->P * d->stride * d->W) * d->C * 2;
  if (int rc = launch_conv(pl, dtype, st)) return rc;
  const int RS = d->R * d->S;
  if (c_real == d->C && s_real == d->S && d->C % 64 == 0 && RS <= WGR_T_MAXRS && g.Ng == RS * d->C &&
      pl.splits <= 32 && (long)d->K * (d->C / 64) >= 256 && (reinterpret_cast<uintptr_t>(dw_kcrs) & 15) == 0) {
    SSIP_KLAUNCH(wgrad_reduce_t_kernel, dim3((unsigned)(d->K * (d->C / 64))), dim3(256), 0, st,
                 (const float*)workspace, pl.splits, d->K, g.Ng, d->C, RS, dw_kcrs, accumulate);
    return ::ssip::check_launch("wgrad_reduce_t");
  }
  return launch_slab_reduce(workspace, pl.splits, d->K, g.Ng, c_real, d->R, s_real, d->C, d->S, dw_kcrs, accumulate,
                            st);
}

}  // namespace

extern "C" {

int64_t ssip_conv_fwd_partial_floats(const ssip_conv_desc* d) {
  const ConvKnobs k = conv_knobs();
  ConvRoute r32, r16;
  const int rc32 = route_fwd(k, d, SSIP_F32, r32), rc16 = route_fwd(k, d, SSIP_BF16, r16);
  if (rc32 && rc16) return -1;
  // the partial-buffer size must not depend on dtype: size for the smaller (128-row) tiles
  int64_t n = (int64_t)ceil_div((rc32 ? r16 : r32).pl.args.M, 128) * d->K * 3;
  // one record per (channel, workgroup, wave row) where bf16 takes a persistent kernel
  if (r16.persistent_fwd()) n = std::max(n, (int64_t)route_records(r16) * d->K * 3);
  // + the scratch of ssip_bn_finalize's split pass (the most records any
  // plan writes bounds the splits; the scratch starts behind the records)
  return n + fin_scratch_floats(d->K, n / (3 * d->K), 3);
}

int ssip_conv_fwd(const ssip_conv_desc* d, int dtype, const void* x, const void* w_krsc, void* y, float* bn_partial,
                  void* stream) {
  const ConvKnobs k = conv_knobs();
  ConvRoute r;
  if (int rc = route_fwd(k, d, dtype, r)) return rc;
  SSIP_REQUIRE(x && w_krsc && y, SSIP_ERR_ARG, "ssip_conv_fwd: null pointer");
  if (r.kind == ROUTE_HALO)
    return launch_halo(MODE_FWD, d, r.hp, x, w_krsc, y, nullptr, bn_partial, (hipStream_t)stream);
  if (r.kind == ROUTE_STEM) return launch_stem_halo(d, r.hp, x, w_krsc, y, bn_partial, (hipStream_t)stream);
  set_operands(r.pl.args, d, MODE_FWD, x, w_krsc);
  r.pl.args.out = y; r.pl.args.partial = bn_partial;
  return launch_conv(r.pl, dtype, (hipStream_t)stream);
}

int ssip_conv_fwd_partial_tiles(const ssip_conv_desc* d, int dtype) {
  const ConvKnobs k = conv_knobs();
  ConvRoute r;
  route_fwd(k, d, dtype, r);
  return route_records(r);
}

int ssip_conv_fwd_ds_partial_tiles(const ssip_conv_desc* d, const ssip_conv_desc* dds, int dtype) {
  const ConvKnobs k = conv_knobs();
  ConvRoute r, rds;
  if (fwd_ds_plan(k, d, dds, dtype, r)) return route_records(r);
  route_fwd(k, dds, dtype, rds);  // two launches: the downsample's own
  return route_records(rds);
}

int ssip_conv_fwd_ds(const ssip_conv_desc* d, const ssip_conv_desc* dds, int dtype, const void* x, const void* w_krsc,
                     void* y, float* bn_partial, const void* wds_kc, void* y_ds, float* bn_partial_ds, void* stream) {
  SSIP_REQUIRE(x && w_krsc && y && wds_kc && y_ds, SSIP_ERR_ARG, "ssip_conv_fwd_ds: null pointer");
  const ConvKnobs k = conv_knobs();
  ConvRoute r;
  if (!fwd_ds_plan(k, d, dds, dtype, r)) {  // two launches
    int rc = ssip_conv_fwd(d, dtype, x, w_krsc, y, bn_partial, stream);
    if (rc) return rc;
    return ssip_conv_fwd(dds, dtype, x, wds_kc, y_ds, bn_partial_ds, stream);
  }
  SSIP_REQUIRE((bn_partial == nullptr) == (bn_partial_ds == nullptr), SSIP_ERR_ARG,
               "ssip_conv_fwd_ds: both or neither BN partial buffers");
  Plan& pl = r.pl;
  ConvArgs& a = pl.args;
  set_operands(a, d, MODE_FWD, x, w_krsc);
  a.out = y; a.partial = bn_partial;
  const int T1 = (int)pl.grid.x;
  a.fwd_tiles1 = T1;
  a.Bds = wds_kc; a.out_ds = y_ds; a.partial_ds = bn_partial_ds;
  a.bds_bytes = (uint32_t)((long)d->K * d->C * 2);
  a.stat_tiles_m = ceil_div(a.M, pl.bm);
  pl.grid = dim3(2 * T1, 1, 1);
  return launch_conv(pl, dtype, (hipStream_t)stream);
}

int ssip_conv_fwd_bias(const ssip_conv_desc* d, int dtype, const void* x, const void* w_krsc, const float* bias,
                       const void* residual, int relu, void* y, void* stream) {
  const ConvKnobs k = conv_knobs();
  ConvRoute r;
  if (int rc = route_fwd(k, d, dtype, r)) return rc;
  SSIP_REQUIRE(!r.pl.conv1, SSIP_ERR_ARG, "ssip_conv_fwd_bias: not for the C = 4 stem");
  SSIP_REQUIRE(x && w_krsc && bias && y, SSIP_ERR_ARG, "ssip_conv_fwd_bias: null pointer");
  if (r.kind == ROUTE_HALO)
    return launch_halo(MODE_FWD, d, r.hp, x, w_krsc, y, residual, nullptr, (hipStream_t)stream, bias, relu ? 1 : 0);
  set_operands(r.pl.args, d, MODE_FWD, x, w_krsc);
  r.pl.args.out = y; r.pl.args.partial = nullptr;
  r.pl.args.add = residual; r.pl.args.bias = bias; r.pl.args.relu = relu ? 1 : 0;
  return launch_conv(r.pl, dtype, (hipStream_t)stream);
}

int ssip_conv_dgrad(const ssip_conv_desc* d, int dtype, const void* dy, const void* w_crsk, void* dx,
                    const void* dx_add, void* stream) {
  const ConvKnobs k = conv_knobs();
  ConvRoute r;
  if (int rc = route_dgrad(k, d, dtype, r)) return rc;
  SSIP_REQUIRE(dy && w_crsk && dx, SSIP_ERR_ARG, "ssip_conv_dgrad: null pointer");
  if (r.kind == ROUTE_HALO)
    return launch_halo(MODE_DGRAD, d, r.hp, dy, w_crsk, dx, dx_add, nullptr, (hipStream_t)stream);
  set_operands(r.pl.args, d, MODE_DGRAD, dy, w_crsk);
  r.pl.args.out = dx; r.pl.args.add = dx_add;
  return launch_conv(r.pl, dtype, (hipStream_t)stream);
}

int ssip_conv_dgrad_ds(const ssip_conv_desc* d, int dtype, const void* dy, const void* w_crsk, const void* dy_ds,
                       const void* wds_ck, void* dx, void* stream) {
  SSIP_REQUIRE(desc_ok(d) && dy && w_crsk && dy_ds && wds_ck && dx, SSIP_ERR_ARG, "ssip_conv_dgrad_ds: bad arguments");
  SSIP_REQUIRE(d->H % d->stride == 0 && d->W % d->stride == 0 && d->P * d->stride == d->H &&
                   d->Q * d->stride == d->W, SSIP_ERR_ARG,
               "ssip_conv_dgrad_ds: the 1x1 downsample's output grid must equal the conv's (H, W divisible by stride)");
  ssip_conv_desc dd = *d;  // the block's 1x1 / stride downsample: same input, same output grid
  dd.R = 1; dd.S = 1; dd.pad = 0;
  const ConvKnobs k = conv_knobs();
  ConvRoute r;
  if (int rc = route_dgrad(k, d, dtype, r)) return rc;
  const bool fuse = r.kind == ROUTE_GLDS && r.pl.args.phased && d->R == 3 && d->S == 3 && d->pad == 1 && d->stride == 2;
  if (!fuse) {  // two passes: the conv's dgrad, then the downsample's accumulated in place
    int rc = ssip_conv_dgrad(d, dtype, dy, w_crsk, dx, nullptr, stream);
    if (rc) return rc;
    return ssip_conv_dgrad(&dd, dtype, dy_ds, wds_ck, dx, dx, stream);
  }
  ConvArgs& a = r.pl.args;
  set_operands(a, d, MODE_DGRAD, dy, w_crsk);
  a.out = dx; a.add = nullptr;
  a.A2 = dy_ds; a.B2 = wds_ck;
  a.a2_bytes = a.a_bytes;
  a.b2_bytes = (uint32_t)((long)d->K * d->C * 2);
  // phase (0, 0): h = 2i, w = 2j meet tap (1, 1) at dy pixel (i, j) -- the downsample's pixel
  SSIP_REQUIRE(a.phase[0].nr == 1 && a.phase[0].ns == 1 && a.phase[0].bh == 0 && a.phase[0].bw == 0, SSIP_ERR_ARG,
               "ssip_conv_dgrad_ds: unexpected phase (0, 0) geometry");
  a.ds_from = a.phase[0].ksteps;
  a.phase[0].ksteps += d->K / 64;
  set_phase_order(a);
  return launch_conv(r.pl, dtype, (hipStream_t)stream);
}

int64_t ssip_conv_dgrad_bn_partial_floats(const ssip_conv_desc* d) {
  const ConvKnobs k = conv_knobs();
  ConvRoute r32, r16;
  const int rc32 = route_dgrad(k, d, SSIP_F32, r32, true), rc16 = route_dgrad(k, d, SSIP_BF16, r16, true);
  if (rc32 && rc16) return -1;
  long tiles = ceil_div((rc32 ? r16 : r32).pl.args.M, 128);  // the LDS-DMA / register-staged paths: >= 128-row tiles
  if (r16.kind == ROUTE_HALO) tiles = std::max<long>(tiles, route_records(r16));
  return tiles * d->C * 2 + fin_scratch_floats(d->C, tiles, 2);  // + ssip_bn_bwd_from_partials' split scratch
}

int ssip_conv_dgrad_bn_partial_tiles(const ssip_conv_desc* d, int dtype) {
  const ConvKnobs k = conv_knobs();
  ConvRoute r;
  route_dgrad(k, d, dtype, r, true);
  return route_records(r);
}

int ssip_conv_dgrad_bn(const ssip_conv_desc* d, int dtype, const void* dy, const void* w_crsk, const void* dx_add,
                       const void* zmask, const uint8_t* mask_bits, const float* mscale, const float* mshift,
                       const void* y, const float* mean, const float* invstd, void* dpre, float* partial,
                       void* stream) {
  const ConvKnobs k = conv_knobs();
  ConvRoute r;
  if (int rc = route_dgrad(k, d, dtype, r, true)) return rc;
  SSIP_REQUIRE(dy && w_crsk && y && mean && invstd && dpre && partial, SSIP_ERR_ARG,
               "ssip_conv_dgrad_bn: null pointer");
  SSIP_REQUIRE(zmask || mask_bits || (mscale && mshift), SSIP_ERR_ARG,
               "ssip_conv_dgrad_bn: one ReLU-mask source (zmask, mask_bits or mscale+mshift) is required");
  SSIP_REQUIRE(d->C % 8 == 0, SSIP_ERR_ARG, "ssip_conv_dgrad_bn: C must be a multiple of 8");
  if (r.kind == ROUTE_HALO) {
    SSIP_REQUIRE(!zmask || mask_bits || (mscale && mshift), SSIP_ERR_ARG,
                 "ssip_conv_dgrad_bn: the halo kernel takes mask bits or the BN affine, not z");
    HaloBnPost bp;
    bp.y = y; bp.bits = mask_bits; bp.mean = mean; bp.invstd = invstd;
    bp.mscale = mask_bits ? nullptr : mscale; bp.mshift = mask_bits ? nullptr : mshift;
    return launch_halo(MODE_DGRAD, d, r.hp, dy, w_crsk, dpre, dx_add, partial, (hipStream_t)stream, nullptr, 0, &bp);
  }
  ConvArgs& a = r.pl.args;
  set_operands(a, d, MODE_DGRAD, dy, w_crsk);
  a.out = dpre; a.add = dx_add;
  a.pmask = zmask; a.pbits = zmask ? nullptr : mask_bits;
  a.pmscale = (zmask || mask_bits) ? nullptr : mscale; a.pmshift = (zmask || mask_bits) ? nullptr : mshift;
  a.py = y; a.pmean = mean; a.pinvstd = invstd; a.partial = partial;
  return launch_conv(r.pl, dtype, (hipStream_t)stream);
}

int64_t ssip_conv_wgrad_workspace_bytes_budget(const ssip_conv_desc* d, int max_workgroups) {
  if (max_workgroups < 0) return -1;
  const ConvKnobs k = conv_knobs();
  ConvRoute r;
  int64_t b = -1;
  // max over dtypes so one workspace serves both, and over the INBN form's plan (glds_inbn_plan: no wide tiles)
  const struct { int elem_bytes; bool big; } plans[] = {{2, true}, {2, false}, {4, true}};
  for (const auto& p : plans)
    if ((p.big || max_workgroups > 0) &&
        plan_conv(k, MODE_WGRAD, d, p.elem_bytes, r.pl, max_workgroups, p.big) == SSIP_OK)
      b = std::max(b, implicit_slab_bytes(r.pl));
  // a persistent kernel at its full grid: a budget only shrinks it
  if (b >= 0) route_wgrad(k, d, SSIP_BF16, 0, r);
  if (r.persistent_wgrad()) b = std::max(b, persistent_slab_bytes(r.hp));
  return b;
}

int64_t ssip_conv_wgrad_workspace_bytes(const ssip_conv_desc* d) { return ssip_conv_wgrad_workspace_bytes_budget(d, 0); }

int ssip_conv_wgrad(const ssip_conv_desc* d, int dtype, const void* dy, const void* x, float* dw_kcrs, int c_real,
                    int s_real, int accumulate, void* workspace, int64_t workspace_bytes, void* stream) {
  return ssip_conv_wgrad_budget(d, dtype, dy, x, dw_kcrs, c_real, s_real, accumulate, workspace, workspace_bytes, 0,
                                stream);
}

int ssip_conv_wgrad_budget(const ssip_conv_desc* d, int dtype, const void* dy, const void* x, float* dw_kcrs,
                           int c_real, int s_real, int accumulate, void* workspace, int64_t workspace_bytes,
                           int max_workgroups, void* stream) {
  SSIP_REQUIRE(max_workgroups >= 0, SSIP_ERR_ARG, "ssip_conv_wgrad_budget: negative budget");
  const ConvKnobs k = conv_knobs();
  ConvRoute r;
  if (int rc = route_wgrad(k, d, dtype, max_workgroups, r)) return rc;
  SSIP_REQUIRE(dy && x && dw_kcrs && workspace, SSIP_ERR_ARG, "ssip_conv_wgrad: null pointer");
  // (the implicit plan's need, whichever kernel runs: the workspace query returns the maximum)
  const int64_t need = implicit_slab_bytes(r.pl);
  SSIP_REQUIRE(workspace_bytes >= need, SSIP_ERR_WORKSPACE, "wgrad workspace too small: %lld < %lld",
               (long long)workspace_bytes, (long long)need);
  SSIP_REQUIRE(c_real >= 1 && c_real <= d->C && s_real >= 1 && s_real <= d->S, SSIP_ERR_ARG, "bad c_real/s_real");
  if (r.kind == ROUTE_STEM_WGRAD)
    return launch_stem_wgrad(d, r.hp, dy, x, dw_kcrs, c_real, s_real, accumulate, workspace, workspace_bytes,
                             (hipStream_t)stream);
  if (r.kind == ROUTE_HALO_WGRAD)
    return launch_halo_wgrad(d, r.hp, dy, x, dw_kcrs, c_real, s_real, accumulate, workspace, workspace_bytes,
                             (hipStream_t)stream, nullptr, nullptr);
  return wgrad_implicit(r.pl, d, dtype, dy, x, dw_kcrs, c_real, s_real, accumulate, workspace, (hipStream_t)stream);
}

int ssip_stem_bwd_wgrad_supported(const ssip_conv_desc* d, int dtype) {
  const ConvKnobs k = conv_knobs();
  ConvRoute r;
  return stem_bwd_route(k, d, dtype, r) ? 1 : 0;
}

int ssip_stem_bwd_wgrad(const ssip_conv_desc* d, int dtype, const void* dpool, const uint8_t* idx, const void* y,
                        const void* x, const float* scale, const float* shift, const float* coef, float* dw_kcrs,
                        int c_real, int s_real, int accumulate, void* workspace, int64_t workspace_bytes,
                        void* stream) {
  const ConvKnobs k = conv_knobs();
  ConvRoute r;
  SSIP_REQUIRE(stem_bwd_route(k, d, dtype, r), SSIP_ERR_ARG, "ssip_stem_bwd_wgrad: unsupported geometry");
  SSIP_REQUIRE(dpool && idx && y && x && scale && shift && coef && dw_kcrs && workspace, SSIP_ERR_ARG,
               "ssip_stem_bwd_wgrad: null pointer");
  SSIP_REQUIRE(c_real >= 1 && c_real <= d->C && s_real >= 1 && s_real <= d->S, SSIP_ERR_ARG, "bad c_real/s_real");
  const HaloPlan& hp = r.hp;
  const int64_t need = persistent_slab_bytes(hp);
  SSIP_REQUIRE(workspace_bytes >= need, SSIP_ERR_WORKSPACE, "wgrad workspace too small: %lld < %lld",
               (long long)workspace_bytes, (long long)need);
  const int P2 = (d->P + 2 - 3) / 2 + 1, Q2 = (d->Q + 2 - 3) / 2 + 1;  // the 3x3 / 2 / 1 max-pool
  StemBwArgs h;
  h.X = static_cast<const __bf16*>(x);
  h.Y = static_cast<const __bf16*>(y);
  h.DP = static_cast<const __bf16*>(dpool);
  h.IX = idx;
  h.scale = scale; h.shift = shift; h.coef = coef;
  h.slab = static_cast<float*>(workspace);
  h.x_bytes = (uint32_t)((long)d->N * d->H * d->W * 8);
  h.y_bytes = (uint32_t)((long)d->N * d->P * d->Q * 64 * 2);
  h.dp_bytes = (uint32_t)((long)d->N * P2 * Q2 * 64 * 2);
  h.ix_bytes = (uint32_t)((long)d->N * P2 * Q2 * 64);
  h.N = d->N; h.H = d->H; h.W = d->W; h.P = d->P; h.Q = d->Q; h.P2 = P2; h.Q2 = Q2; h.tiles = hp.tiles;
  hipStream_t st = (hipStream_t)stream;
  SSIP_KLAUNCH(conv_stem_bwd_wgrad2_kernel, dim3(hp.G), dim3(768), 0, st, h);
  if (int rc = ::ssip::check_launch("conv_stem_bwd_wgrad")) return rc;
  return launch_slab_reduce(workspace, hp.G, 64, hp.cols, c_real, d->R, s_real, d->C, d->S, dw_kcrs, accumulate, st);
}

int ssip_conv_bnrelu_in_supported(const ssip_conv_desc* d, int dtype) {
  const ConvKnobs k = conv_knobs();
  ConvRoute rf, rw;
  return bnrelu_in_routes(k, d, dtype, rf, rw) ? 1 : 0;
}

int ssip_conv_fwd_bnrelu_in(const ssip_conv_desc* d, int dtype, const void* y_in, const float* in_scale,
                            const float* in_shift, const void* w_krsc, void* y, float* bn_partial, void* z_out,
                            void* stream) {
  const ConvKnobs k = conv_knobs();
  ConvRoute rf, rw;
  SSIP_REQUIRE(bnrelu_in_routes(k, d, dtype, rf, rw), SSIP_ERR_ARG,
               "ssip_conv_fwd_bnrelu_in: unsupported geometry (ssip_conv_bnrelu_in_supported)");
  SSIP_REQUIRE(y_in && in_scale && in_shift && w_krsc && y, SSIP_ERR_ARG, "ssip_conv_fwd_bnrelu_in: null pointer");
  if (rf.kind == ROUTE_HALO)
    return launch_halo(MODE_FWD, d, rf.hp, y_in, w_krsc, y, nullptr, bn_partial, (hipStream_t)stream, nullptr, 0,
                       nullptr, in_scale, in_shift, z_out);
  SSIP_REQUIRE(z_out == nullptr || (d->R == 1 && d->S == 1 && d->pad == 0), SSIP_ERR_ARG,
               "ssip_conv_fwd_bnrelu_in: z_out on the halo geometry and 1x1 convs only");
  ConvArgs& a = rf.pl.args;  // the INBN ring plan
  set_operands(a, d, MODE_FWD, y_in, w_krsc);
  a.out = y; a.partial = bn_partial; a.zout = z_out;
  a.in_scale = in_scale; a.in_shift = in_shift;
  return launch_glds(rf.pl, (hipStream_t)stream);
}

int ssip_conv_wgrad_bnrelu_in(const ssip_conv_desc* d, int dtype, const void* dy, const void* y_in,
                              const float* in_scale, const float* in_shift, float* dw_kcrs, int accumulate,
                              void* workspace, int64_t workspace_bytes, int max_workgroups, void* stream) {
  const ConvKnobs k = conv_knobs();
  ConvRoute rf, rw;
  SSIP_REQUIRE(bnrelu_in_routes(k, d, dtype, rf, rw), SSIP_ERR_ARG,
               "ssip_conv_wgrad_bnrelu_in: unsupported geometry (ssip_conv_bnrelu_in_supported)");
  SSIP_REQUIRE(dy && y_in && in_scale && in_shift && dw_kcrs && workspace && max_workgroups >= 0, SSIP_ERR_ARG,
               "ssip_conv_wgrad_bnrelu_in: bad arguments");
  if (rw.kind == ROUTE_HALO_WGRAD) {
    route_wgrad(k, d, dtype, max_workgroups, rw);  // the grid under this budget
    return launch_halo_wgrad(d, rw.hp, dy, y_in, dw_kcrs, d->C, d->S, accumulate, workspace, workspace_bytes,
                             (hipStream_t)stream, in_scale, in_shift);
  }
  Plan& pl = rw.pl;
  SSIP_REQUIRE(glds_inbn_plan(k, MODE_WGRAD, d, dtype, pl, max_workgroups), SSIP_ERR_ARG,
               "ssip_conv_wgrad_bnrelu_in: no LDS-DMA BN+ReLU-in plan under this budget");
  const int64_t need = implicit_slab_bytes(pl);
  SSIP_REQUIRE(workspace_bytes >= need, SSIP_ERR_WORKSPACE, "wgrad workspace too small: %lld < %lld",
               (long long)workspace_bytes, (long long)need);
  pl.args.in_scale = in_scale; pl.args.in_shift = in_shift;
  return wgrad_implicit(pl, d, dtype, dy, y_in, dw_kcrs, d->C, d->S, accumulate, workspace, (hipStream_t)stream);
}

/* Which kernel a conv pass selects for this geometry (tests / tuning): writes a
 * NUL-terminated name such as "glds<fwd,256x256,4x2,2>" or "halo<fwd>" into buf. */
int ssip_conv_kernel_name(int mode, const ssip_conv_desc* d, int dtype, char* buf, int buflen) {
  return ssip_conv_kernel_name_budget(mode, d, dtype, 0, buf, buflen);
}

// formats the route of the pass: no choice of its own
int ssip_conv_kernel_name_budget(int mode, const ssip_conv_desc* d, int dtype, int max_workgroups, char* buf,
                                 int buflen) {
  SSIP_REQUIRE(buf && buflen > 0, SSIP_ERR_ARG, "ssip_conv_kernel_name: no buffer");
  SSIP_REQUIRE(max_workgroups >= 0, SSIP_ERR_ARG, "ssip_conv_kernel_name_budget: negative budget");
  SSIP_REQUIRE(mode >= 0 && mode <= 2, SSIP_ERR_ARG, "ssip_conv_kernel_name: mode must be 0 (fwd), 1 (dgrad), 2 (wgrad)");
  const ConvKnobs k = conv_knobs();
  ConvRoute r;
  const int rc = mode == MODE_FWD     ? route_fwd(k, d, dtype, r)
                 : mode == MODE_DGRAD ? route_dgrad(k, d, dtype, r)
                                      : route_wgrad(k, d, dtype, max_workgroups, r);
  const Plan& pl = r.pl;
  switch (r.kind) {
    case ROUTE_HALO: snprintf(buf, buflen, "halo<%s,TR=%d,G=%d>", MODE_NAME[mode], r.hp.TR, r.hp.G); break;
    case ROUTE_STEM: snprintf(buf, buflen, "stem_halo<fwd,G=%d>", r.hp.G); break;
    case ROUTE_STEM_WGRAD: snprintf(buf, buflen, "stem_wgrad<G=%d>", r.hp.G); break;
    case ROUTE_HALO_WGRAD: snprintf(buf, buflen, "halo_wgrad<TR=%d,G=%d>", r.hp.TR, r.hp.G); break;
    case ROUTE_GLDS:
    case ROUTE_REGSTAGED:
      snprintf(buf, buflen, "%s<%s,%dx%d,%dx%d,%d%s%s,splits=%d>", r.kind == ROUTE_GLDS ? "glds" : "regstaged",
               MODE_NAME[mode], pl.bm, pl.bn, pl.wmw, pl.wnw, pl.stages, pl.conv1 ? ",stem" : "",
               pl.args.phased ? ",phased" : "", pl.splits);
      break;
    default: return rc;
  }
  return SSIP_OK;
}

}  // extern "C"

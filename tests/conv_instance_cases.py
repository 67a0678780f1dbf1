"""The conv kernel instances of csrc/conv.hip (GLDS_TABLE, GEMM_TABLE), each at
a geometry where something is ragged: one row per instance, form and geometry.
tests/test_cpu_conv_instances.py checks the table against the host planner
(no device); tests/test_gpu_conv_instances.py runs every row against a torch
CPU float64 reference.

A tile is forced (SSIP_CONV_FORCE) only where the planner's own divisibility
rules would allow it, so a failure is a kernel bug and not a configuration
the product never runs:
  * fwd / dgrad: bn divides the column count (C and K are multiples of 256);
  * wgrad 256x256: K % 256 == 0 and (R S C) % 256 == 0;
  * wgrad 128x256 and 128x128: K % 128 == 0; wgrad 64x128: K % 128 != 0;
  * a partial last column tile is legal for a wgrad (the planner selects the
    128x128, 64x128 and 128x256 tiles with R S C no multiple of the width);
  * register-staged wgrad: the tile plan_conv itself takes for the geometry
    (bm = 128 where K % 128 == 0 else 64; bn = 64 where bm = 128 and
    (R S C) % 128 == 64, else 128).

Geometry: (N, C, H, W, K, R, stride, pad).  C == 3 is the stem: stored with 4
channels and S = 8; pad 0 there means H and W already carry the zero border
of the 7x7 / pad-3 conv (the engine's pre-padded layout).

ragged: what the row exercises, recomputed from the geometry and the parsed
kernel name by the CPU test:
  m      a partial last row tile (phased dgrad: in some phase)
  n      a partial last column tile (wgrad only)
  phase  phased dgrad: some phase owns fewer row tiles than the grid
  empty  phased dgrad: some phase has no tap
  split  wgrad: >= 2 splits, the last one shorter than the others
  npq    wgrad: the last k-step is partial (N P Q no multiple of the k-step's rows)
"""
from collections import namedtuple

from ssip.ops import ConvGeom

Case = namedtuple("Case", "pas form dtype geom env budget expect ragged")

# forward / dgrad (C and K multiples of 256: every tile's bn divides the columns)
G_S1 = (3, 256, 9, 11, 512, 3, 1, 1)     # fwd / dgrad M = 297: 2.3 tiles of 128, 1.2 of 256
G_S2 = (7, 256, 15, 13, 256, 3, 2, 1)    # fwd M = 392; dgrad phases of 392 / 336 / 343 / 294 rows
G_1X1 = (7, 256, 15, 13, 512, 1, 2, 0)   # dgrad: three of the four phases have no tap
# wgrad: N P Q = 4205 or 4350, 66 or 68 k-steps in 4 splits of 17
W_A = (5, 256, 29, 29, 256, 3, 1, 1)
W_B = (5, 192, 29, 29, 128, 3, 1, 1)     # 1728 columns: % 128 = 64, % 256 = 192
W_C = (5, 64, 29, 29, 192, 3, 1, 1)      # K % 128 != 0: 64-row tiles, 576 columns
W_D = (5, 64, 57, 59, 128, 3, 2, 1)      # stride 2, odd image
# BN+ReLU-in (stride 1, C <= 512)
I_1X1 = (5, 128, 29, 29, 256, 1, 1, 0)
I_3X3 = (5, 128, 29, 29, 128, 3, 1, 1)
I_WIDE = W_A
# stem: 39x48 image, P = 20, Q = 24
STEM_PRE = (9, 3, 45, 54, 64, 7, 2, 0)   # pre-padded: the LDS-DMA stem kernels (SSIP_HALO=0)
STEM_RAW = (9, 3, 39, 48, 64, 7, 2, 3)   # padded by the kernel: register-staged

FWD_GEOMS = (G_S1, G_S2)
DGRAD_GEOMS = (G_S1, G_S2, G_1X1)
WGRAD_GEOMS = (W_A, W_B, W_C, W_D)
INBN_GEOMS = (I_1X1, I_3X3, I_WIDE)
BUDGET = 256  # the side stream's workgroup budget on a 256-CU device

INBN = "SSIP_BNRELU_GLDS=3 SSIP_BNRELU_GLDS_MINM=0 SSIP_WGRAD_BIG=0"


def F(pas, tile):
    """SSIP_CONV_FORCE for pass pas ('f' / 'd' / 'w') and tile 'bm,bn,waves_m,waves_n,stages'."""
    return f"SSIP_CONV_FORCE={pas},{tile}"


T_A, T_B, T_C, T_D = "128,128,4,2,2", "128,64,4,2,2", "256,256,4,2,2", "128,128,4,4,3"
R_A, R_B, R_C, R_D = "256,128,4,2,0", "256,64,4,2,0", "128,128,2,2,0", "128,64,2,2,0"

CASES = [
    # ---- LDS-DMA ring, bf16: forward
    Case("fwd", "plain", "bf16", G_S1, F("f", T_A), 0, "glds<fwd,128x128,4x2,2,", ("m",)),
    Case("fwd", "plain", "bf16", G_S1, F("f", T_B), 0, "glds<fwd,128x64,4x2,2,", ("m",)),
    Case("fwd", "plain", "bf16", G_S1, F("f", T_C), 0, "glds<fwd,256x256,4x2,2,", ("m",)),
    Case("fwd", "plain", "bf16", G_S1, F("f", T_D), 0, "glds<fwd,128x128,4x4,3,", ("m",)),
    Case("fwd", "plain", "bf16", G_S2, F("f", T_A), 0, "glds<fwd,128x128,4x2,2,", ("m",)),
    Case("fwd", "plain", "bf16", G_S2, F("f", T_B), 0, "glds<fwd,128x64,4x2,2,", ("m",)),
    Case("fwd", "plain", "bf16", G_S2, F("f", T_C), 0, "glds<fwd,256x256,4x2,2,", ("m",)),
    Case("fwd", "plain", "bf16", G_S2, F("f", T_D), 0, "glds<fwd,128x128,4x4,3,", ("m",)),
    # ---- dgrad: stride 1, phased 3x3, phased 1x1 (dx_add None, and accumulated in place)
    Case("dgrad", "plain", "bf16", G_S1, F("d", T_A), 0, "glds<dgrad,128x128,4x2,2,splits", ("m",)),
    Case("dgrad", "plain", "bf16", G_S1, F("d", T_B), 0, "glds<dgrad,128x64,4x2,2,splits", ("m",)),
    Case("dgrad", "plain", "bf16", G_S1, F("d", T_C), 0, "glds<dgrad,256x256,4x2,2,splits", ("m",)),
    Case("dgrad", "plain", "bf16", G_S1, F("d", T_D), 0, "glds<dgrad,128x128,4x4,3,splits", ("m",)),
    Case("dgrad", "plain", "bf16", G_S2, F("d", T_A), 0, "glds<dgrad,128x128,4x2,2,phased", ("m", "phase")),
    Case("dgrad", "plain", "bf16", G_S2, F("d", T_B), 0, "glds<dgrad,128x64,4x2,2,phased", ("m", "phase")),
    Case("dgrad", "plain", "bf16", G_S2, F("d", T_C), 0, "glds<dgrad,256x256,4x2,2,phased", ("m",)),
    Case("dgrad", "plain", "bf16", G_S2, F("d", T_D), 0, "glds<dgrad,128x128,4x4,3,phased", ("m", "phase")),
    Case("dgrad", "plain", "bf16", G_1X1, F("d", T_A), 0, "glds<dgrad,128x128,4x2,2,phased", ("m", "phase", "empty")),
    Case("dgrad", "plain", "bf16", G_1X1, F("d", T_B), 0, "glds<dgrad,128x64,4x2,2,phased", ("m", "phase", "empty")),
    Case("dgrad", "plain", "bf16", G_1X1, F("d", T_C), 0, "glds<dgrad,256x256,4x2,2,phased", ("m", "empty")),
    Case("dgrad", "plain", "bf16", G_1X1, F("d", T_D), 0, "glds<dgrad,128x128,4x4,3,phased", ("m", "phase", "empty")),
    # ---- wgrad: the planner's own choice, full grid and under the side stream's budget
    Case("wgrad", "plain", "bf16", W_A, "", 0, "glds<wgrad,128x128,4x2,2,splits=4>", ("split", "npq")),
    Case("wgrad", "plain", "bf16", W_A, "", BUDGET, "glds<wgrad,256x256,4x2,2,splits=4>", ("split", "npq")),
    Case("wgrad", "plain", "bf16", W_B, "", 0, "glds<wgrad,128x128,4x2,2,splits=4>", ("n", "split", "npq")),
    Case("wgrad", "plain", "bf16", W_B, "", BUDGET, "glds<wgrad,128x256,2x4,2,splits=4>", ("n", "split", "npq")),
    Case("wgrad", "plain", "bf16", W_C, "", 0, "glds<wgrad,64x128,2x4,2,splits=4>", ("n", "split", "npq")),
    Case("wgrad", "plain", "bf16", W_D, "", 0, "glds<wgrad,128x128,4x2,2,splits=4>", ("n", "split", "npq")),
    Case("wgrad", "plain", "bf16", W_D, "", BUDGET, "glds<wgrad,128x256,2x4,2,splits=4>", ("n", "split", "npq")),
    # ---- the pre-padded stem
    Case("fwd", "stem", "bf16", STEM_PRE, "SSIP_HALO=0", 0, "glds<fwd,128x64,4x2,2,stem,", ("m",)),
    Case("wgrad", "stem", "bf16", STEM_PRE, "SSIP_HALO=0", 0, "glds<wgrad,64x128,2x4,2,stem,splits=4>",
         ("n", "split", "npq")),
    # ---- folded eval BN (ssip_conv_fwd_bias): residual + ReLU, ReLU only, bare
    Case("fwd", "fold", "bf16", G_S1, F("f", T_A), 0, "glds<fwd,128x128,4x2,2,", ("m",)),
    Case("fwd", "fold", "bf16", G_S1, F("f", T_B), 0, "glds<fwd,128x64,4x2,2,", ("m",)),
    Case("fwd", "fold", "bf16", G_S1, F("f", T_C), 0, "glds<fwd,256x256,4x2,2,", ("m",)),
    Case("fwd", "fold", "bf16", G_S1, F("f", T_D), 0, "glds<fwd,128x128,4x4,3,", ("m",)),
    Case("fwd", "fold", "bf16", G_S2, F("f", T_A), 0, "glds<fwd,128x128,4x2,2,", ("m",)),
    Case("fwd", "fold", "bf16", G_S2, F("f", T_B), 0, "glds<fwd,128x64,4x2,2,", ("m",)),
    Case("fwd", "fold", "bf16", G_S2, F("f", T_C), 0, "glds<fwd,256x256,4x2,2,", ("m",)),
    Case("fwd", "fold", "bf16", G_S2, F("f", T_D), 0, "glds<fwd,128x128,4x4,3,", ("m",)),
    # ---- the fused conv + 1x1 downsample forward (ssip_conv_fwd_ds)
    Case("fwd", "fwd_ds", "bf16", G_S2, F("f", T_A), 0, "glds<fwd,128x128,4x2,2,", ("m",)),
    Case("fwd", "fwd_ds", "bf16", G_S2, F("f", T_B), 0, "glds<fwd,128x64,4x2,2,", ("m",)),
    Case("fwd", "fwd_ds", "bf16", G_S2, F("f", T_C), 0, "glds<fwd,256x256,4x2,2,", ("m",)),
    Case("fwd", "fwd_ds", "bf16", G_S2, F("f", T_D), 0, "glds<fwd,128x128,4x4,3,", ("m",)),
    # ---- BN+ReLU-in (unforced the small forward takes 4x4,3, which has no INBN form)
    Case("fwd", "inbn", "bf16", I_1X1, INBN + " " + F("f", T_A), 0, "glds<fwd,128x128,4x2,2,", ("m",)),
    Case("fwd", "inbn", "bf16", I_1X1, INBN + " " + F("f", T_B), 0, "glds<fwd,128x64,4x2,2,", ("m",)),
    Case("fwd", "inbn", "bf16", I_1X1, INBN + " " + F("f", T_C), 0, "glds<fwd,256x256,4x2,2,", ("m",)),
    Case("fwd", "inbn", "bf16", I_3X3, INBN + " " + F("f", T_A), 0, "glds<fwd,128x128,4x2,2,", ("m",)),
    Case("fwd", "inbn", "bf16", I_3X3, INBN + " " + F("f", T_B), 0, "glds<fwd,128x64,4x2,2,", ("m",)),
    Case("fwd", "inbn", "bf16", I_WIDE, INBN + " " + F("f", T_A), 0, "glds<fwd,128x128,4x2,2,", ("m",)),
    Case("fwd", "inbn", "bf16", I_WIDE, INBN + " " + F("f", T_B), 0, "glds<fwd,128x64,4x2,2,", ("m",)),
    Case("fwd", "inbn", "bf16", I_WIDE, INBN + " " + F("f", T_C), 0, "glds<fwd,256x256,4x2,2,", ("m",)),
    Case("wgrad", "inbn", "bf16", I_1X1, INBN + " " + F("f", T_A), 0, "glds<wgrad,128x128,4x2,2,splits=4>",
         ("split", "npq")),
    Case("wgrad", "inbn", "bf16", I_1X1, INBN + " " + F("f", T_A), BUDGET, "glds<wgrad,128x128,4x2,2,splits=4>",
         ("split", "npq")),
    Case("wgrad", "inbn", "bf16", I_3X3, INBN + " " + F("f", T_A), 0, "glds<wgrad,128x128,4x2,2,splits=4>",
         ("split", "npq")),
    Case("wgrad", "inbn", "bf16", I_3X3, INBN + " " + F("f", T_A), BUDGET, "glds<wgrad,128x128,4x2,2,splits=4>",
         ("split", "npq")),
    Case("wgrad", "inbn", "bf16", I_WIDE, INBN + " " + F("f", T_A), 0, "glds<wgrad,128x128,4x2,2,splits=4>",
         ("split", "npq")),
    Case("wgrad", "inbn", "bf16", I_WIDE, INBN + " " + F("f", T_A), BUDGET, "glds<wgrad,128x128,4x2,2,splits=4>",
         ("split", "npq")),
    # ---- register-staged, bf16
    Case("fwd", "plain", "bf16", G_S1, F("f", R_A), 0, "regstaged<fwd,256x128,4x2,0,", ("m",)),
    Case("fwd", "plain", "bf16", G_S1, F("f", R_B), 0, "regstaged<fwd,256x64,4x2,0,", ("m",)),
    Case("fwd", "plain", "bf16", G_S1, F("f", R_C), 0, "regstaged<fwd,128x128,2x2,0,", ("m",)),
    Case("fwd", "plain", "bf16", G_S1, F("f", R_D), 0, "regstaged<fwd,128x64,2x2,0,", ("m",)),
    Case("fwd", "plain", "bf16", G_S2, F("f", R_A), 0, "regstaged<fwd,256x128,4x2,0,", ("m",)),
    Case("fwd", "plain", "bf16", G_S2, F("f", R_B), 0, "regstaged<fwd,256x64,4x2,0,", ("m",)),
    Case("fwd", "plain", "bf16", G_S2, F("f", R_C), 0, "regstaged<fwd,128x128,2x2,0,", ("m",)),
    Case("fwd", "plain", "bf16", G_S2, F("f", R_D), 0, "regstaged<fwd,128x64,2x2,0,", ("m",)),
    Case("dgrad", "plain", "bf16", G_S1, F("d", R_A), 0, "regstaged<dgrad,256x128,4x2,0,", ("m",)),
    Case("dgrad", "plain", "bf16", G_S1, F("d", R_B), 0, "regstaged<dgrad,256x64,4x2,0,", ("m",)),
    Case("dgrad", "plain", "bf16", G_S1, F("d", R_C), 0, "regstaged<dgrad,128x128,2x2,0,", ("m",)),
    Case("dgrad", "plain", "bf16", G_S1, F("d", R_D), 0, "regstaged<dgrad,128x64,2x2,0,", ("m",)),
    Case("dgrad", "plain", "bf16", G_S2, F("d", R_A), 0, "regstaged<dgrad,256x128,4x2,0,", ("m",)),
    Case("dgrad", "plain", "bf16", G_S2, F("d", R_B), 0, "regstaged<dgrad,256x64,4x2,0,", ("m",)),
    Case("dgrad", "plain", "bf16", G_S2, F("d", R_C), 0, "regstaged<dgrad,128x128,2x2,0,", ("m",)),
    Case("dgrad", "plain", "bf16", G_S2, F("d", R_D), 0, "regstaged<dgrad,128x64,2x2,0,", ("m",)),
    Case("wgrad", "plain", "bf16", W_A, F("w", "128,128,2,2,0"), 0, "regstaged<wgrad,128x128,2x2,0,splits=4>",
         ("split", "npq")),
    Case("wgrad", "plain", "bf16", W_B, F("w", "128,64,2,2,0"), 0, "regstaged<wgrad,128x64,2x2,0,splits=4>",
         ("split", "npq")),
    Case("wgrad", "plain", "bf16", W_C, F("w", "64,128,2,2,0"), 0, "regstaged<wgrad,64x128,2x2,0,splits=4>",
         ("n", "split", "npq")),
    Case("wgrad", "plain", "bf16", W_D, F("w", "128,64,2,2,0"), 0, "regstaged<wgrad,128x64,2x2,0,splits=4>",
         ("split", "npq")),
    Case("fwd", "stem", "bf16", STEM_RAW, "SSIP_HALO=0", 0, "regstaged<fwd,128x64,2x2,0,stem,", ("m",)),
    Case("wgrad", "stem", "bf16", STEM_RAW, "SSIP_HALO=0", 0, "regstaged<wgrad,64x128,2x2,0,stem,splits=4>",
         ("n", "split", "npq")),
    # ---- register-staged, fp32: what the planner picks unforced
    Case("fwd", "plain", "f32", G_S1, "", 0, "regstaged<fwd,128x128,2x2,0,", ("m",)),
    Case("fwd", "plain", "f32", G_S2, "", 0, "regstaged<fwd,128x128,2x2,0,", ("m",)),
    Case("dgrad", "plain", "f32", G_S1, "", 0, "regstaged<dgrad,128x128,2x2,0,", ("m",)),
    Case("dgrad", "plain", "f32", G_S2, "", 0, "regstaged<dgrad,128x128,2x2,0,", ("m",)),
    Case("dgrad", "plain", "f32", G_1X1, "", 0, "regstaged<dgrad,128x128,2x2,0,", ("m",)),
    Case("wgrad", "plain", "f32", W_A, "", 0, "regstaged<wgrad,128x128,2x2,0,splits=8>", ("split", "npq")),
    Case("wgrad", "plain", "f32", W_B, "", 0, "regstaged<wgrad,128x64,2x2,0,splits=8>", ("split", "npq")),
    Case("wgrad", "plain", "f32", W_C, "", 0, "regstaged<wgrad,64x128,2x2,0,splits=8>", ("n", "split", "npq")),
    Case("wgrad", "plain", "f32", W_D, "", 0, "regstaged<wgrad,128x64,2x2,0,splits=8>", ("split", "npq")),
    Case("fwd", "stem", "f32", STEM_PRE, "SSIP_HALO=0", 0, "regstaged<fwd,128x64,2x2,0,stem,", ("m",)),
    Case("wgrad", "stem", "f32", STEM_PRE, "SSIP_HALO=0", 0, "regstaged<wgrad,64x128,2x2,0,stem,splits=8>",
         ("n", "split")),  # (4320 rows are whole 32-row k-steps; 135 of them in 8 splits of 17)
]

NAME_RE = (r"(glds|regstaged)<(fwd|dgrad|wgrad),(\d+)x(\d+),(\d+)x(\d+),(\d+)(,stem)?(,phased)?,splits=(\d+)>$")


def case_id(c):
    force = [e.split("=", 1)[1] for e in c.env.split(" ") if e.startswith("SSIP_CONV_FORCE=")]
    tile = force[0].replace(",", ".") if force else "auto"
    return f"{c.pas}-{c.form}-{c.dtype}-{'x'.join(map(str, c.geom))}-{tile}-b{c.budget}"


def geom(c):
    """The row's ConvGeom (the stem stored with 4 channels and 8 filter columns)."""
    N, C, H, W, K, R, st, pd = c.geom
    if C == 3:
        return ConvGeom(N, H, W, 4, K, R, 8, st, pd, 3, R)
    return ConvGeom(N, H, W, C, K, R, R, st, pd, C, R)


def ds_geom(c):
    """The block's 1x1 downsample over the same input and output grid (form fwd_ds)."""
    N, C, H, W, K, R, st, pd = c.geom
    return ConvGeom(N, H, W, C, K, 1, 1, st, 0, C, 1)


def env_items(c):
    return [e.split("=", 1) for e in c.env.split(" ") if e]

"""Writes tests/golden/conv_routes.json: every host-side planning answer of
csrc/conv.hip (kernel names, BatchNorm-record and workspace sizes, the
*_supported predicates; tests/test_cpu_conv_routes.py's ``query``) over a grid
of conv geometries, dtypes, tuning knobs and workgroup budgets, and the status
of every launching entry point called with null data pointers.  Regenerate
only when a planning answer is meant to change.

Host planning needs no device; run where none is visible, so the CU count is
the fallback 256 (the MI355X's) and the null-pointer calls stay off a GPU.

usage: python tests/golden/make_conv_route_goldens.py
"""
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
for p in (ROOT / "tests", ROOT / "semi-supervised-image-processing_amd", ROOT):
    sys.path.insert(0, str(p))

F32, BF16 = 0, 1


def geom(N, C, H, W, K, R, stride, pad, P=None, Q=None):
    """The 11 ssip_conv_desc fields; C == 4 is the stem (S stored as 8, Q from the real 7 columns)."""
    S = 8 if C == 4 else R
    return [N, H, W, C, K, R, S, stride, pad, (H + 2 * pad - R) // stride + 1 if P is None else P,
            (W + 2 * pad - R) // stride + 1 if Q is None else Q]


def resnet18(N):  # every conv at 224^2, the stem unpadded and pre-padded
    out = [geom(N, 4, 224, 224, 64, 7, 2, 3), geom(N, 4, 230, 230, 64, 7, 2, 0), geom(N, 64, 56, 56, 64, 3, 1, 1)]
    for C, H in ((64, 56), (128, 28), (256, 14)):
        out += [geom(N, C, H, H, 2 * C, 3, 2, 1), geom(N, 2 * C, H // 2, H // 2, 2 * C, 3, 1, 1),
                geom(N, C, H, H, 2 * C, 1, 2, 0)]
    return out


def resnet50(N):  # the stem and bottleneck convs at 512^2 (tests/test_gpu_c5.py, tests/test_gpu_r50_geometry.py)
    import test_gpu_r50_geometry as R50

    return [geom(N, 4, 518, 518, 64, 7, 2, 0)] + [geom(N, C, H, H, K, R, st, pd) for _, (C, H, K, R, st, pd) in R50.CONVS]


def conv_test_shapes():  # tests/test_gpu_conv.py
    import test_gpu_conv as TC

    out = []
    for shape in TC.SHAPES + [(4, 64, 28, 28, 64, 3, 1, 1)]:
        N, C, H, W, K, R, st, pd, pre = TC._unpack(shape)
        if pre:
            H, W, pd = H + 2 * pd, W + 2 * pd, 0
        out.append(geom(N, 4 if C == 3 else C, H, W, K, R, st, pd))
    return out


# no GPU test launches these: the dispatch around them
EDGES = [
    geom(8, 64, 32, 32, 64, 7, 1, 3),     # a non-stem 7x7: > 32 taps, no ring kernel (fwd and dgrad)
    geom(8, 64, 32, 32, 128, 1, 4, 0),    # stride-4 1x1: a strided dgrad without a phase split
    geom(16, 128, 28, 28, 192, 3, 1, 1),  # K = 192: 64-column tiles
    geom(8, 64, 8, 8, 64, 3, 1, 1),       # the halo geometry, too short for the halo kernel (TR * W < 128)
]
INVALID = [
    geom(8, 48, 14, 14, 64, 3, 1, 1),              # C = 48
    geom(8, 64, 56, 56, 64, 3, 1, 1, P=55),        # P inconsistent
    geom(0, 64, 56, 56, 64, 3, 1, 1),              # N = 0
]

KNOB_ENVS = [
    "SSIP_HALO=0",
    "SSIP_CONV_FORCE=f,128,128,4,2,2",
    "SSIP_CONV_FORCE=d,128,64,4,2,2",
    "SSIP_CONV_FORCE=w,128,128,4,2,2",
    "SSIP_CONV_FORCE=f,128,128,2,2,0",
    "SSIP_WGRAD_BIG=0",
    "SSIP_WGRAD_BLOCKS=64",
    "SSIP_BNRELU_GLDS=3",
    "SSIP_BNRELU_GLDS_MINM=0",
    "SSIP_NO_FWD_DSFUSE=1",
]
# the knobs that bear on the ResNet-50 convs (the product is thinned here to keep the fixture small)
R50_ENVS = ["SSIP_WGRAD_BIG=0", "SSIP_BNRELU_GLDS=3", "SSIP_BNRELU_GLDS_MINM=0"]
# SSIP_CONV_FORCE's own checks: register-staged tiles with and without a kernel, a ring tile without one
FORCE_ENVS = ["SSIP_CONV_FORCE=f,256,128,4,2,0", "SSIP_CONV_FORCE=d,256,64,4,2,0", "SSIP_CONV_FORCE=d,64,64,2,2,0",
              "SSIP_CONV_FORCE=w,64,128,2,2,0", "SSIP_CONV_FORCE=w,64,64,2,2,0", "SSIP_CONV_FORCE=w,128,256,2,4,2",
              "SSIP_CONV_FORCE=f,64,64,2,2,2", "SSIP_CONV_FORCE=f,128"]


def grid():
    """(env, geometry, dtype) of every row."""
    bf16_only = [g for n in (256, 5) for g in resnet18(n)] + resnet50(128)
    both = resnet18(128) + resnet50(16) + conv_test_shapes() + EDGES + INVALID
    rows = [("", g, BF16) for g in bf16_only] + [("", g, dt) for g in both for dt in (BF16, F32)]
    rows += [(env, g, BF16) for env in KNOB_ENVS for g in resnet18(256) + EDGES]
    rows += [(env, g, BF16) for env in ("SSIP_HALO=0", "SSIP_WGRAD_BLOCKS=64") for g in conv_test_shapes()]
    rows += [(env, g, BF16) for env in R50_ENVS for g in resnet50(128)]
    force_geoms = [geom(256, 128, 28, 28, 128, 3, 1, 1), geom(256, 4, 230, 230, 64, 7, 2, 0), geom(2, 64, 15, 13, 128, 3, 2, 1)]
    rows += [(env, g, BF16) for env in FORCE_ENVS for g in force_geoms]
    rows += [(env, force_geoms[0], F32) for env in FORCE_ENVS]
    return rows


# (entry point, geometry): a descriptor that entry point accepts
NULL_CALL_GEOMS = [
    ("ssip_conv_fwd", geom(8, 128, 28, 28, 128, 3, 1, 1)),
    ("ssip_conv_fwd", geom(8, 64, 56, 56, 64, 3, 1, 1)),
    ("ssip_conv_fwd", geom(8, 4, 230, 230, 64, 7, 2, 0)),
    ("ssip_conv_fwd_ds", geom(8, 64, 56, 56, 128, 3, 2, 1)),
    ("ssip_conv_fwd_bias", geom(8, 128, 28, 28, 128, 3, 1, 1)),
    ("ssip_conv_dgrad", geom(8, 64, 56, 56, 128, 3, 2, 1)),
    ("ssip_conv_dgrad_ds", geom(8, 64, 56, 56, 128, 3, 2, 1)),
    ("ssip_conv_dgrad_bn", geom(8, 64, 56, 56, 64, 3, 1, 1)),
    ("ssip_conv_dgrad_bn", geom(8, 128, 28, 28, 128, 3, 1, 1)),
    ("ssip_conv_wgrad", geom(8, 128, 28, 28, 128, 3, 1, 1)),
    ("ssip_conv_wgrad_budget", geom(8, 64, 56, 56, 64, 3, 1, 1)),
    ("ssip_conv_wgrad_budget", geom(8, 4, 230, 230, 64, 7, 2, 0)),
    ("ssip_conv_fwd_bnrelu_in", geom(8, 64, 56, 56, 64, 3, 1, 1)),
    ("ssip_conv_wgrad_bnrelu_in", geom(8, 64, 56, 56, 64, 3, 1, 1)),
    ("ssip_stem_bwd_wgrad", geom(8, 4, 230, 230, 64, 7, 2, 0)),
]


def main():
    import torch

    import test_cpu_conv_routes as T
    from ssip import _lib

    assert not torch.cuda.is_available(), "record where no device is visible (256 CUs assumed, null calls off the GPU)"
    lib = _lib.lib()
    rows = []
    for env, g, dt in grid():
        for name in T.KNOBS:
            os.environ.pop(name, None)
        for item in filter(None, env.split(" ")):
            name, value = item.split("=", 1)
            os.environ[name] = value
        rows.append({"env": env, "g": g, "dt": dt, "ans": T.query(lib, g, dt)})
    for name in T.KNOBS:
        os.environ.pop(name, None)
    null_calls = [{"fn": fn, "g": g, "dt": BF16, "ans": T.null_call(lib, fn, g, BF16)} for fn, g in NULL_CALL_GEOMS]
    body = ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows)
    calls = ",\n".join(json.dumps(c, separators=(",", ":")) for c in null_calls)
    out = Path(__file__).resolve().parent / "conv_routes.json"
    out.write_text('{"cus":256,\n"budgets":%s,\n"rows":[\n%s\n],\n"null_calls":[\n%s\n]}\n'
                   % (json.dumps(list(T.BUDGETS)), body, calls))
    print(len(rows), "rows,", len(null_calls), "null calls,", out.stat().st_size, "bytes")


if __name__ == "__main__":
    main()

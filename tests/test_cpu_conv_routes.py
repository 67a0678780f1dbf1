"""CPU: every host-side planning answer of csrc/conv.hip over a grid of
geometries, dtypes, tuning knobs and workgroup budgets equals the recorded one
(tests/golden/conv_routes.json, written by tests/golden/make_conv_route_goldens.py).
The name query, the BatchNorm-record and workspace size queries and the
*_supported predicates are all derived from the route a launch takes; this
pins their agreement and their values.  Host planning needs no device: the CU
count falls back to the MI355X's 256.

  * every row: the answers equal the fixture's;
  * every row whose forward is a persistent kernel (halo / stem_halo): one
    record per (channel, workgroup, wave row), partial_tiles == G * 8, and the
    partial buffer holds them (tests/test_cpu_plan_consistency.py's invariant
    on this wider grid);
  * every launching entry point, called with a valid descriptor and null data
    pointers, returns the recorded SSIP_ERR_ARG before any launch (only where
    no device is visible).
"""
import ctypes
import json
import re
from pathlib import Path

import pytest
import torch

from ssip import _lib, ops

FIXTURE = Path(__file__).resolve().parent / "golden" / "conv_routes.json"
BUDGETS = (0, 128, 256)
# every variable conv.hip's ConvKnobs reads
KNOBS = tuple(ops._PLAN_ENV) + ("SSIP_STAGGER",)


def _desc(g):
    return _lib.ConvDesc(*g)


def _name(lib, mode, d, dt, budget):
    buf = ctypes.create_string_buffer(160)
    rc = lib.ssip_conv_kernel_name_budget(mode, d, dt, budget, buf, 160)
    return buf.value.decode() if rc == 0 else [rc, lib.ssip_last_error().decode()]


def query(lib, g, dt):
    """Every planning answer for geometry g (the 11 ssip_conv_desc fields) and dtype dt."""
    d = _desc(g)
    a = {
        "fwd": _name(lib, 0, d, dt, 0),
        "dgrad": _name(lib, 1, d, dt, 0),
        "wgrad": [_name(lib, 2, d, dt, b) for b in BUDGETS],
        "fwd_tiles": int(lib.ssip_conv_fwd_partial_tiles(d, dt)),
        "fwd_floats": int(lib.ssip_conv_fwd_partial_floats(d)),
        "dgrad_bn_tiles": int(lib.ssip_conv_dgrad_bn_partial_tiles(d, dt)),
        "dgrad_bn_floats": int(lib.ssip_conv_dgrad_bn_partial_floats(d)),
        "wgrad_ws": [int(lib.ssip_conv_wgrad_workspace_bytes_budget(d, b)) for b in BUDGETS],
        "bnrelu_in": int(lib.ssip_conv_bnrelu_in_supported(d, dt)),
        "stem_bwd": int(lib.ssip_stem_bwd_wgrad_supported(d, dt)),
    }
    N, H, W, C, K, R, S, stride, pad, P, Q = g
    if R == 3 and S == 3 and pad == 1:  # with the block's 1x1 downsample over the same grids
        a["fwd_ds_tiles"] = int(lib.ssip_conv_fwd_ds_partial_tiles(d, _desc((N, H, W, C, K, 1, 1, stride, 0, P, Q)), dt))
    return a


# entry point -> its arguments behind (desc, dtype), every data pointer null
NULL_CALLS = {
    "ssip_conv_fwd": (None,) * 5,
    "ssip_conv_fwd_bias": (None, None, None, None, 0, None, None),
    "ssip_conv_dgrad": (None,) * 5,
    "ssip_conv_dgrad_ds": (None,) * 6,
    "ssip_conv_dgrad_bn": (None,) * 13,
    "ssip_conv_wgrad": (None, None, None, 1, 1, 0, None, 1 << 40, None),
    "ssip_conv_wgrad_budget": (None, None, None, 1, 1, 0, None, 1 << 40, 128, None),
    "ssip_conv_fwd_bnrelu_in": (None,) * 8,
    "ssip_conv_wgrad_bnrelu_in": (None,) * 5 + (0, None, 1 << 40, 0, None),
    "ssip_stem_bwd_wgrad": (None,) * 8 + (1, 1, 0, None, 1 << 40, None),
}


def null_call(lib, fn, g, dt):
    """[status, message] of launching entry point fn on geometry g with null data pointers."""
    d = _desc(g)
    if fn == "ssip_conv_fwd_ds":
        N, H, W, C, K, R, S, stride, pad, P, Q = g
        rc = lib.ssip_conv_fwd_ds(d, _desc((N, H, W, C, K, 1, 1, stride, 0, P, Q)), dt, *(None,) * 8)
    else:
        rc = getattr(lib, fn)(d, dt, *NULL_CALLS[fn])
    return [rc, lib.ssip_last_error().decode()]


def set_env(monkeypatch, env):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    for item in filter(None, env.split(" ")):
        name, value = item.split("=", 1)
        assert name in KNOBS, name
        monkeypatch.setenv(name, value)


@pytest.fixture(scope="module")
def golden():
    return json.loads(FIXTURE.read_text())


def _by_env(rows):
    out = {}
    for r in rows:
        out.setdefault(r["env"], []).append(r)
    return out


def test_planning_answers_equal_the_recorded_ones(golden, monkeypatch):
    if torch.cuda.is_available():
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        if cus != golden["cus"]:
            pytest.skip(f"the fixture is recorded for {golden['cus']} CUs; this device has {cus}")
    lib = _lib.lib()
    bad = []
    for env, rows in _by_env(golden["rows"]).items():
        set_env(monkeypatch, env)
        for r in rows:
            got = query(lib, r["g"], r["dt"])
            if got != r["ans"]:
                bad.append((env, r["g"], r["dt"], {k: (got.get(k), v) for k, v in r["ans"].items() if got.get(k) != v}))
    assert len(golden["rows"]) >= 400
    assert not bad, f"{len(bad)} of {len(golden['rows'])} rows differ (got, recorded); first: {bad[:3]}"


def test_persistent_forward_records_fit(golden, monkeypatch):
    lib = _lib.lib()
    seen = 0
    for env, rows in _by_env(golden["rows"]).items():
        set_env(monkeypatch, env)
        for r in rows:
            d = _desc(r["g"])
            name = _name(lib, 0, d, r["dt"], 0)
            if not (isinstance(name, str) and name.startswith(("halo<", "stem_halo<"))):
                continue
            seen += 1
            G = int(re.search(r"G=(\d+)", name).group(1))
            tiles = int(lib.ssip_conv_fwd_partial_tiles(d, r["dt"]))
            floats = int(lib.ssip_conv_fwd_partial_floats(d))
            assert tiles == G * 8, (env, r["g"], name, tiles)
            assert floats >= tiles * r["g"][4] * 3, (env, r["g"], name, tiles, floats)
    assert seen >= 20


@pytest.mark.skipif(torch.cuda.is_available(), reason="null-pointer calls are made only where no device is visible")
def test_launching_entry_points_reject_null_pointers(golden, monkeypatch):
    set_env(monkeypatch, "")
    lib = _lib.lib()
    assert {c["fn"] for c in golden["null_calls"]} == set(NULL_CALLS) | {"ssip_conv_fwd_ds"}
    for c in golden["null_calls"]:
        assert c["ans"][0] == -1  # SSIP_ERR_ARG
        assert null_call(lib, c["fn"], c["g"], c["dt"]) == c["ans"], c

"""CPU: the case table of tests/conv_instance_cases.py against the host planner
of csrc/conv.hip (no device: the CU count falls back to the MI355X's 256).

  (a) every row, under its environment: the name query returns the expected
      instance, what the row says is ragged really is (recomputed from the
      geometry and the parsed name), and the tile is one the planner's own
      divisibility rules allow for the geometry;
  (b) the table covers the kernel tables: the set of ring tiles
      SSIP_CONV_FORCE accepts per pass and form (a probe over bm, bn in
      {64, 128, 256}, waves in {2, 4}^2, stages in {2, 3}) equals the set the
      table lists, every listed register-staged tile is accepted (stages 0:
      apply_force is deliberately wider than GEMM_TABLE, which
      tests/golden/conv_routes.json pins), and the rows are exactly the
      required ones: every accepted tile at every geometry of its family the
      divisibility rules allow.  A row added to or dropped from GLDS_TABLE
      without a case fails here, and so does deleting any row of the table.
"""
import ctypes
import re
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).parent))
from ssip import _lib, ops  # noqa: E402
import conv_instance_cases as cc  # noqa: E402
from conv_instance_cases import CASES, Case  # noqa: E402

DT = {"bf16": torch.bfloat16, "f32": torch.float32}
MODE = {"fwd": 0, "dgrad": 1, "wgrad": 2}


def set_env(monkeypatch, env):
    for name in ops._PLAN_ENV:
        monkeypatch.delenv(name, raising=False)
    for item in filter(None, env.split(" ")):
        name, value = item.split("=", 1)
        assert name in ops._PLAN_ENV, name
        monkeypatch.setenv(name, value)


def parse(name):
    m = re.match(cc.NAME_RE, name)
    assert m, name
    kind, pas, bm, bn, wm, wn, st, stem, phased, splits = m.groups()
    return dict(kind=kind, pas=pas, bm=int(bm), bn=int(bn), wm=int(wm), wn=int(wn), stages=int(st),
                stem=bool(stem), phased=bool(phased), splits=int(splits))


def tile_of(p):
    return (p["bm"], p["bn"], p["wm"], p["wn"], p["stages"])


def phases(g):
    """Rows and taps of the four output-parity phases of a stride-2 dgrad."""
    out = []
    for f in range(4):
        ph, pw = f >> 1, f & 1
        rows = g.N * ((g.H - ph + 1) // 2) * ((g.W - pw + 1) // 2)
        r0, s0 = (ph + g.pad) % 2, (pw + g.pad) % 2
        nr = (g.R - r0 + 1) // 2 if r0 < g.R else 0
        ns = (g.S - s0 + 1) // 2 if s0 < g.S else 0
        out.append((rows, nr * ns))
    return out


def ragged_of(c, p):
    """What is ragged in row c run as the kernel with parsed name p."""
    g = cc.geom(c)
    out = set()
    if c.pas == "wgrad":
        bk = 64 if c.dtype == "bf16" else 32
        npq, cols = g.N * g.P * g.Q, g.R * g.S * g.C
        total = -(-npq // bk)
        ksteps = -(-total // p["splits"])
        assert -(-total // ksteps) == p["splits"]
        if g.K % p["bm"]:
            out.add("m")
        if cols % p["bn"]:
            out.add("n")
        if p["splits"] >= 2 and p["splits"] * ksteps * bk > npq:
            out.add("split")
        if npq % bk:
            out.add("npq")
    elif p["phased"]:
        ph = phases(g)
        tiles = [-(-rows // p["bm"]) for rows, _ in ph]
        if any(rows % p["bm"] for rows, _ in ph):
            out.add("m")
        if min(tiles) < max(tiles):
            out.add("phase")
        if any(taps == 0 for _, taps in ph):
            out.add("empty")
    else:
        rows = g.N * g.P * g.Q if c.pas == "fwd" else g.N * g.H * g.W
        if rows % p["bm"]:
            out.add("m")
    return out


def rule_allows(c, p):
    """The planner's own divisibility rules (conv_instance_cases' docstring)."""
    g = cc.geom(c)
    bm, bn = p["bm"], p["bn"]
    if c.pas != "wgrad":
        return (g.K if c.pas == "fwd" else g.C) % bn == 0
    cols = g.R * g.S * g.C
    if p["kind"] == "regstaged":
        want_bm = 128 if g.K % 128 == 0 else 64
        return (bm, bn) == (want_bm, 64 if want_bm == 128 and cols % 128 == 64 else 128)
    if (bm, bn) == (256, 256):
        return g.K % 256 == 0 and cols % 256 == 0
    if bm == 128:
        return g.K % 128 == 0
    return bm == 64 and g.K % 128 != 0 and g.K % 64 == 0


def query_name(c):
    return ops.conv_kernel_name(c.pas, cc.geom(c), DT[c.dtype], c.budget)


@pytest.mark.parametrize("c", CASES, ids=cc.case_id)
def test_row_selects_its_instance_and_is_ragged(c, monkeypatch):
    set_env(monkeypatch, c.env)
    g, dt = cc.geom(c), DT[c.dtype]
    name = query_name(c)
    assert name.startswith(c.expect), (name, c.expect)
    p = parse(name)
    assert p["pas"] == c.pas and p["stem"] == (c.form == "stem")
    assert c.ragged and ragged_of(c, p) == set(c.ragged), (name, ragged_of(c, p))
    assert rule_allows(c, p), name
    if c.form == "inbn":
        assert ops.conv_bnrelu_in_supported(g, dt)
        fwd = parse(ops.conv_kernel_name("fwd", g, dt))
        assert fwd["kind"] == "glds" and fwd["stages"] == 2 and g.K % fwd["bn"] == 0
    if c.form == "fwd_ds":
        gd = cc.ds_geom(c)
        assert p["kind"] == "glds" and (gd.P, gd.Q) == (g.P, g.Q)
        assert ops.conv_fwd_ds_partial_tiles(g, gd, dt) == -(-g.N * g.P * g.Q // p["bm"]) > 0
    if c.pas == "fwd":
        assert ops.conv_fwd_partial_tiles(g, dt) == -(-g.N * g.P * g.Q // p["bm"])
    if c.pas == "wgrad":  # the workspace the GPU test passes holds the plan's slabs
        assert ops.conv_wgrad_workspace_bytes(g, c.budget) >= p["splits"] * g.K * g.R * g.S * g.C * 4


# ---- (b): the table against the kernel tables
def _forced(monkeypatch, env, pas, g, dt, tile):
    """The parsed name under SSIP_CONV_FORCE=<pas>,<tile>, or None where the planner rejects it."""
    set_env(monkeypatch, (env + " " if env else "") + cc.F(pas[0], ",".join(map(str, tile))))
    buf = ctypes.create_string_buffer(160)
    rc = _lib.lib().ssip_conv_kernel_name_budget(MODE[pas], g.desc(), ops._DT[dt], 0, buf, 160)
    if rc != 0:
        assert "SSIP_CONV_FORCE: no " in _lib.lib().ssip_last_error().decode()
        return None
    p = parse(buf.value.decode())
    assert tile_of(p) == tuple(tile), (buf.value, tile)
    return p


RING_GRID = [(bm, bn, wm, wn, st) for bm in (64, 128, 256) for bn in (64, 128, 256) for wm in (2, 4)
             for wn in (2, 4) for st in (2, 3)]
# (pass, form) -> a row of the table whose geometry and environment the probe borrows
PROBE_AT = {("fwd", "plain"): cc.G_S1, ("dgrad", "plain"): cc.G_S1, ("wgrad", "plain"): cc.W_A,
            ("fwd", "stem"): cc.STEM_PRE}


def _ring_accepted(monkeypatch, pas, form):
    row = Case(pas, form, "bf16", PROBE_AT[(pas, form)], "", 0, "", ())
    env = "SSIP_HALO=0" if form == "stem" else ""
    got = set()
    for tile in RING_GRID:
        p = _forced(monkeypatch, env, pas, cc.geom(row), torch.bfloat16, tile)
        if p is not None:
            assert p["kind"] == "glds" and p["stem"] == (form == "stem")
            got.add(tile)
    return got


def _listed(monkeypatch):
    """(row, parsed name) of every row."""
    out = []
    for c in CASES:
        set_env(monkeypatch, c.env)
        out.append((c, parse(query_name(c))))
    return out


def test_ring_tiles_listed_equal_the_ones_the_planner_accepts(monkeypatch):
    listed = _listed(monkeypatch)
    for pas, form in PROBE_AT:
        have = {tile_of(p) for c, p in listed if (c.pas, c.form) == (pas, form) and p["kind"] == "glds"}
        assert have == _ring_accepted(monkeypatch, pas, form), (pas, form)
    # the stem wgrad runs the plain wgrad ring kernel on the 4-channel image: one of its tiles
    stem_wg = {tile_of(p) for c, p in listed if (c.pas, c.form) == ("wgrad", "stem") and p["kind"] == "glds"}
    assert stem_wg and stem_wg <= _ring_accepted(monkeypatch, "wgrad", "plain")
    # the forms the name query does not show take the forward's tiles: FOLD and
    # the fused downsample all of them, INBN the 2-stage ones its predicate accepts
    fwd = _ring_accepted(monkeypatch, "fwd", "plain")
    for form in ("fold", "fwd_ds"):
        assert {tile_of(p) for c, p in listed if (c.pas, c.form) == ("fwd", form)} == fwd, form
    inbn = set()
    for tile in fwd:
        set_env(monkeypatch, cc.INBN + " " + cc.F("f", ",".join(map(str, tile))))
        if ops.conv_bnrelu_in_supported(cc.geom(Case("fwd", "inbn", "bf16", cc.I_WIDE, "", 0, "", ())), torch.bfloat16):
            inbn.add(tile)
    assert len(inbn) == 3
    assert {tile_of(p) for c, p in listed if (c.pas, c.form) == ("fwd", "inbn")} == inbn


def test_listed_register_staged_tiles_are_accepted(monkeypatch):
    seen = 0
    for c, p in _listed(monkeypatch):
        if p["kind"] != "regstaged" or c.geom == cc.STEM_RAW:  # (no force reaches the stem the kernel pads)
            continue
        env = " ".join(e for e in c.env.split(" ") if not e.startswith("SSIP_CONV_FORCE="))
        q = _forced(monkeypatch, env, c.pas, cc.geom(c), DT[c.dtype], tile_of(p))
        assert q is not None and q["kind"] == "regstaged", cc.case_id(c)
        seen += 1
    assert seen >= 25


def _required(monkeypatch):
    """The rows the table must hold: (pass, form, dtype, geometry, kind, tile, budget)."""
    bf, f32 = torch.bfloat16, torch.float32
    need = set()

    def add(pas, form, dtype, geo, env, budget=0, tile=None):
        c = Case(pas, form, dtype, geo, env, budget, "", ())
        if tile is not None:
            env = (env + " " if env else "") + cc.F(pas[0], ",".join(map(str, tile)))
        set_env(monkeypatch, env)
        p = parse(ops.conv_kernel_name(pas, cc.geom(c), DT[dtype], budget))
        if rule_allows(c, p):
            need.add((pas, form, dtype, geo, p["kind"], tile_of(p), budget))

    fwd = _ring_accepted(monkeypatch, "fwd", "plain")
    for tile in fwd:
        for geo in cc.FWD_GEOMS:
            add("fwd", "plain", "bf16", geo, "", tile=tile)
            add("fwd", "fold", "bf16", geo, "", tile=tile)
        add("fwd", "fwd_ds", "bf16", cc.G_S2, "", tile=tile)
        if tile[4] == 2 and tile[3] == 2:  # the INBN forms (checked against the predicate above)
            for geo in cc.INBN_GEOMS:
                add("fwd", "inbn", "bf16", geo, cc.INBN, tile=tile)
    for tile in _ring_accepted(monkeypatch, "dgrad", "plain"):
        for geo in cc.DGRAD_GEOMS:
            add("dgrad", "plain", "bf16", geo, "", tile=tile)
    for geo in cc.WGRAD_GEOMS:  # the planner's own choices
        add("wgrad", "plain", "bf16", geo, "")
        add("wgrad", "plain", "bf16", geo, "", budget=cc.BUDGET)
        add("wgrad", "plain", "f32", geo, "")
        for tile in ((128, 128, 2, 2, 0), (128, 64, 2, 2, 0), (64, 128, 2, 2, 0)):
            add("wgrad", "plain", "bf16", geo, "", tile=tile)
    need = {r for r in need if not (r[6] and (r[0], r[1], r[2], r[3], r[4], r[5], 0) in need)}  # a budget that changes nothing
    for geo in cc.INBN_GEOMS:
        for b in (0, cc.BUDGET):
            need.add(("wgrad", "inbn", "bf16", geo, "glds", (128, 128, 4, 2, 2), b))
    for tile in ((256, 128, 4, 2, 0), (256, 64, 4, 2, 0), (128, 128, 2, 2, 0), (128, 64, 2, 2, 0)):
        for geo in cc.FWD_GEOMS:
            add("fwd", "plain", "bf16", geo, "", tile=tile)
            add("dgrad", "plain", "bf16", geo, "", tile=tile)
    for geo in cc.FWD_GEOMS:
        add("fwd", "plain", "f32", geo, "")
    for geo in cc.DGRAD_GEOMS:
        add("dgrad", "plain", "f32", geo, "")
    for pas in ("fwd", "wgrad"):
        add(pas, "stem", "bf16", cc.STEM_PRE, "SSIP_HALO=0")
        add(pas, "stem", "f32", cc.STEM_PRE, "SSIP_HALO=0")
        add(pas, "stem", "bf16", cc.STEM_RAW, "SSIP_HALO=0")
    return need


def test_rows_are_exactly_the_required_ones(monkeypatch):
    have = [(c.pas, c.form, c.dtype, c.geom, p["kind"], tile_of(p), c.budget) for c, p in _listed(monkeypatch)]
    assert len(set(have)) == len(have), "duplicate rows"
    need = _required(monkeypatch)
    assert set(have) == need, (sorted(need - set(have)), sorted(set(have) - need))

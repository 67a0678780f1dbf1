"""CPU: the conv tuning knobs (csrc/conv.hip's ConvKnobs) and the Python plan
cache (ssip.ops._plan_query) agree.  The library reads the SSIP_* variables at
every call; ops memoises the planning queries per (arguments, environment), so
every variable that can change an answer must be part of its key -- a stale
answer makes ssip_conv_fwd_bnrelu_in fail its precondition, or sizes a wgrad
workspace for another split count.  The planning queries need no device (the
CU count falls back to the MI355X's 256)."""
import re
from pathlib import Path

import torch

from ssip import _lib, ops
from ssip.ops import ConvGeom

ROOT = Path(__file__).resolve().parents[1]
BF16 = torch.bfloat16


def _set(monkeypatch, name, value):
    if value is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, value)


def test_bnrelu_in_supported_follows_the_environment(monkeypatch):
    # ResNet-50 layer-3 conv3 at batch 128: 131,072 rows, below the 262,144-row default threshold
    g = ConvGeom(128, 32, 32, 256, 1024, 1, 1, 1, 0, 256, 1)
    lib = _lib.lib()
    for name in ops._PLAN_ENV:
        monkeypatch.delenv(name, raising=False)
    for minm, want in ((None, False), ("0", True), (None, False)):
        _set(monkeypatch, "SSIP_BNRELU_GLDS_MINM", minm)
        direct = bool(lib.ssip_conv_bnrelu_in_supported(g.desc(), _lib.BF16))
        assert direct is want, minm
        assert ops.conv_bnrelu_in_supported(g, BF16) is direct, minm


def test_wgrad_workspace_bytes_follows_the_environment(monkeypatch):
    g = ConvGeom(8, 14, 14, 256, 256, 3, 3, 1, 1, 256, 3)  # ResNet-18 layer-3 3x3
    budget = 256
    lib = _lib.lib()
    for name in ops._PLAN_ENV:
        monkeypatch.delenv(name, raising=False)
    base = int(lib.ssip_conv_wgrad_workspace_bytes_budget(g.desc(), budget))
    assert base > 0
    # a target workgroup count that changes the split count, found from the library itself
    blocks = None
    for cand in ("1", "64", "4096"):
        monkeypatch.setenv("SSIP_WGRAD_BLOCKS", cand)
        if int(lib.ssip_conv_wgrad_workspace_bytes_budget(g.desc(), budget)) != base:
            blocks = cand
            break
    assert blocks is not None, "no SSIP_WGRAD_BLOCKS value changes the split count"
    seen = []
    for value in (None, blocks, None):
        _set(monkeypatch, "SSIP_WGRAD_BLOCKS", value)
        direct = int(lib.ssip_conv_wgrad_workspace_bytes_budget(g.desc(), budget))
        assert ops.conv_wgrad_workspace_bytes(g, budget) == direct, value
        seen.append(direct)
    assert seen[0] == seen[2] == base and seen[1] != base


def test_plan_cache_keys_on_every_conv_knob():
    """Every variable conv.hip reads is in the tuple ops keys its plan cache on,
    or is known not to change a planning answer."""
    src = (ROOT / "semi-supervised-image-processing_amd" / "csrc" / "conv.hip").read_text()
    read = set(re.findall(r'getenv\(\s*"(SSIP_\w+)"', src))
    assert read, "conv.hip reads no SSIP_* variable?"
    allowed = {"SSIP_STAGGER"}  # changes the launched kernel's schedule only, no query's answer
    assert read - set(ops._PLAN_ENV) - allowed == set()

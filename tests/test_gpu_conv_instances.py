"""GPU: every row of tests/conv_instance_cases.py -- each conv kernel instance
of csrc/conv.hip (GLDS_TABLE, GEMM_TABLE) in each of its forms, at a geometry
with a partial last row tile, a partial last column tile or a ragged split
tail -- against torch CPU float64 on the bf16-rounded operands (fp32 operands
for the fp32 kernels).  The row's environment selects the instance
(SSIP_CONV_FORCE only where the planner's own divisibility rules allow the
tile); the kernel name is asserted before anything runs.

Tolerances are the project's own:
  * bf16 outputs (tests/test_gpu_bench_geometry.py, test_gpu_eval_fold.py): an
    fp32 accumulation rounded once to bf16, |y - ref| <= 2^-8 |ref| + 1e-4 max|ref|
    per element, + 2^-8 |pre| for the second rounding of a residual / dgrad add;
  * fp32 weight gradients of the bf16 kernels: max|dw - ref| <= 1e-4 max|ref|
    (accumulated onto a base of the gradient's own magnitude, whose fp32 add
    rounds by 2^-24 (|base| + |dw|) < 3e-7 max|ref|, inside the same bound);
  * fp32 kernels: max|y - ref| <= 2e-5 max|ref| (tests/test_gpu_conv.py);
  * BN statistics finalized from the forward's records: mean within 1e-3 of
    the largest std, variance within 1e-3 of the largest variance.
Bit equalities: three wgrad launches; BN+ReLU-in against ssip_bn_apply + the
plain conv under the same environment (outputs, records, dw, z_out of a 1x1);
the fused conv + downsample against its two separate launches.

No stray writes: every output, record buffer and wgrad workspace is a slice
of a larger allocation with at least one full tile of sentinel bytes on
either side; outputs start as NaN.  Afterwards the sentinels are unchanged,
the output holds no NaN, and the record buffer is NaN past
conv_fwd_partial_tiles records.  The workspace is exactly
conv_wgrad_workspace_bytes(g, budget) bytes.

Each family's worst error over its bound is printed when the module ends
(pytest -s)."""
import functools
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).parent))
from ssip import ops  # noqa: E402
import conv_instance_cases as cc  # noqa: E402
from conv_instance_cases import CASES  # noqa: E402

pytestmark = pytest.mark.gpu
DT = {"bf16": torch.bfloat16, "f32": torch.float32}
SENTINEL = 0x5A
WORST = {}  # family -> (error / bound, case id)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for fam in sorted(WORST):
        print(f"\nconv instances: {fam}: worst error / bound = {WORST[fam][0]:.4f} at {WORST[fam][1]}", end="")
    print()


def _note(c, what, ratio):
    fam = f"{c.dtype} {c.pas} {c.form} {what}"
    ratio = float(ratio)
    print(f"{cc.case_id(c)} {what}: error / bound = {ratio:.4f}")
    if ratio != ratio or ratio > WORST.get(fam, (-1.0, ""))[0]:
        WORST[fam] = (ratio, cc.case_id(c))
    return ratio


class Guarded:
    """numel elements of dtype inside a larger allocation: guard_elems (at least
    a full tile) of sentinel bytes on either side; .t is the flat slice."""

    def __init__(self, dev, dtype, numel, guard_elems, fill=float("nan")):
        es = torch.empty((), dtype=dtype).element_size()
        self.gb = -(-guard_elems * es // 256) * 256
        self.nb = numel * es
        self.raw = torch.full((2 * self.gb + self.nb,), SENTINEL, dtype=torch.uint8, device=dev)
        body = self.raw[self.gb:self.gb + self.nb]
        self.t = body if dtype == torch.uint8 else body.view(dtype)
        self.t.fill_(fill)

    def intact(self):
        return bool((self.raw[:self.gb] == SENTINEL).all()) and bool((self.raw[self.gb + self.nb:] == SENTINEL).all())


def _rnd(t, dtype):
    return t.to(DT[dtype]).float()


def _is_stem(geo):
    return geo[1] == 3


def _image_and_pad(geo):
    """(H, W) of the image itself and the conv's real padding (the pre-padded
    stem carries its 3-pixel border in H and W)."""
    N, C, H, W, K, R, st, pd = geo
    return (H - 6, W - 6, 3) if _is_stem(geo) and pd == 0 else (H, W, pd)


def _gen(geo, salt):
    return torch.Generator().manual_seed(1000 * salt + sum(geo))


# ---- references: computed once per geometry and dtype, shared, never written
@functools.lru_cache(maxsize=None)
def fwd_data(geo, dtype):
    N, C, H, W, K, R, st, pd = geo
    hi, wi, pad = _image_and_pad(geo)
    gen = _gen(geo, 1)
    x = _rnd(torch.randn(N, C, hi, wi, generator=gen), dtype)
    w = _rnd(torch.randn(K, C, R, R, generator=gen) * (2.0 / (C * R * R)) ** 0.5, dtype)
    return x, w, F.conv2d(x.double(), w.double(), stride=st, padding=pad)


@functools.lru_cache(maxsize=None)
def ds_data(geo, dtype):
    """The 1x1 downsample over fwd_data's x."""
    N, C, H, W, K, R, st, pd = geo
    x = fwd_data(geo, dtype)[0]
    wd = _rnd(torch.randn(K, C, 1, 1, generator=_gen(geo, 2)) * (2.0 / C) ** 0.5, dtype)
    return wd, F.conv2d(x.double(), wd.double(), stride=st)


@functools.lru_cache(maxsize=None)
def fold_data(geo, dtype):
    """Folded eval BN: x, the fp32 weight, its per-channel factor and bias, a
    residual, and float64 conv(x, bf16(w s)) + bias."""
    N, C, H, W, K, R, st, pd = geo
    gen = _gen(geo, 3)
    x = _rnd(torch.randn(N, C, H, W, generator=gen), dtype)
    w = torch.randn(K, C, R, R, generator=gen) * (2.0 / (C * R * R)) ** 0.5
    s = torch.rand(K, generator=gen) + 0.5
    b = torch.randn(K, generator=gen) * 0.3
    wf = _rnd(w * s.view(K, 1, 1, 1), dtype)  # the folded weight as the kernel stores it
    pre = F.conv2d(x.double(), wf.double(), stride=st, padding=pd) + b.double().view(1, K, 1, 1)
    r = _rnd(torch.randn(pre.shape, generator=gen), dtype)
    return x, w, s, b, r, pre


@functools.lru_cache(maxsize=None)
def dgrad_data(geo, dtype):
    N, C, H, W, K, R, st, pd = geo
    P, Q = (H + 2 * pd - R) // st + 1, (W + 2 * pd - R) // st + 1
    gen = _gen(geo, 4)
    w = _rnd(torch.randn(K, C, R, R, generator=gen) * (2.0 / (K * R * R)) ** 0.5, dtype)
    dy = _rnd(torch.randn(N, K, P, Q, generator=gen), dtype)
    add = _rnd(torch.randn(N, C, H, W, generator=gen), dtype)
    return w, dy, add, torch.nn.grad.conv2d_input((N, C, H, W), w.double(), dy.double(), stride=st, padding=pd)


@functools.lru_cache(maxsize=None)
def wgrad_data(geo, dtype):
    N, C, H, W, K, R, st, pd = geo
    hi, wi, pad = _image_and_pad(geo)
    P, Q = (hi + 2 * pad - R) // st + 1, (wi + 2 * pad - R) // st + 1
    gen = _gen(geo, 5)
    x = _rnd(torch.relu(torch.randn(N, C, hi, wi, generator=gen)), dtype)
    dy = _rnd(torch.randn(N, K, P, Q, generator=gen) * 1e-2, dtype)
    ref = torch.nn.grad.conv2d_weight(x.double(), (K, C, R, R), dy.double(), stride=st, padding=pad)
    base = torch.randn(K, C, R, R, generator=gen) * ref.abs().max().float()
    return x, dy, ref, base


@functools.lru_cache(maxsize=None)
def inbn_data(geo):
    """y of the layer below, a BN affine of both signs whose shift is >= 0.5 on
    every second channel (a zero row transformed would be clearly non-zero),
    z = bf16(relu(fma_f32(y, scale, shift))) (ssip_bn_apply's arithmetic: the
    product is exact in fp64 and the sum rounded once, so its fp32 rounding is
    the fp32 fma), and the float64 forward and weight gradient over z."""
    N, C, H, W, K, R, st, pd = geo
    gen = _gen(geo, 6)
    y = _rnd(torch.randn(N, C, H, W, generator=gen), "bf16")
    scale = (torch.rand(C, generator=gen) + 0.25) * torch.where(torch.rand(C, generator=gen) < 0.2, -1.0, 1.0)
    shift = torch.randn(C, generator=gen) * 0.5
    shift[::2] = 0.5 + torch.rand(C // 2, generator=gen)
    z = (y.double() * scale.double()[None, :, None, None] + shift.double()[None, :, None, None]).float()
    z = torch.relu(z).bfloat16().float()
    w = _rnd(torch.randn(K, C, R, R, generator=gen) * (2.0 / (C * R * R)) ** 0.5, "bf16")
    dy = _rnd(torch.randn(N, K, H, W, generator=gen) * 1e-2, "bf16")
    ref = F.conv2d(z.double(), w.double(), padding=pd)
    refw = torch.nn.grad.conv2d_weight(z.double(), (K, C, R, R), dy.double(), padding=pd)
    base = torch.randn(K, C, R, R, generator=gen) * refw.abs().max().float()
    return y, scale, shift, z, w, dy, ref, refw, base


# ---- checks
def _check_out(c, what, got_nhwc, ref_nchw, pre=None):
    """A bf16 / fp32 output tensor against its float64 reference."""
    ref = ref_nchw.permute(0, 2, 3, 1)
    got = got_nhwc.double().cpu().reshape(ref.shape)
    assert not torch.isnan(got).any(), f"{what}: elements never written"
    err = (got - ref).abs()
    if c.dtype == "f32":
        ratio = err.max() / (2e-5 * ref.abs().max())
    else:
        bound = ref.abs() * 2.0 ** -8 + 1e-4 * ref.abs().max()
        if pre is not None:
            bound = bound + pre.permute(0, 2, 3, 1).abs() * 2.0 ** -8
        ratio = (err / bound).max()
    assert _note(c, what, ratio) <= 1.0, what


def _check_dw(c, what, got, ref):
    assert not torch.isnan(got).any(), f"{what}: elements never written"
    rel = (got.double().cpu().reshape(ref.shape) - ref).abs().max() / ref.abs().max()
    assert _note(c, what, rel / (2e-5 if c.dtype == "f32" else 1e-4)) <= 1.0, what


def _records(c, what, part, tiles, K):
    """The record buffer after the forward: tiles * K records written, NaN past them, guards intact."""
    used = tiles * K * 3
    assert part.intact(), f"{what}: write outside the record buffer"
    assert not torch.isnan(part.t[:used]).any(), f"{what}: records never written"
    assert bool(torch.isnan(part.t[used:]).all()), f"{what}: write past the {tiles} records"
    return part.t[:used].clone()


def _check_stats(c, what, part, tiles, K, ref_nchw, dev):
    """ssip_bn_finalize over the forward's records against the reference's batch statistics."""
    stats = torch.empty((4, K), device=dev)
    rm, rv = torch.zeros(K, device=dev), torch.ones(K, device=dev)
    ops.bn_finalize(K, tiles, part.t, torch.ones(K, device=dev), torch.zeros(K, device=dev), rm, rv, 0.1, 1e-5, True,
                    stats[0], stats[1], stats[2], stats[3])
    torch.cuda.synchronize()
    r = ref_nchw.permute(0, 2, 3, 1).reshape(-1, K)
    mean, var = r.mean(0), r.var(0, unbiased=False)
    m_got = stats[0].cpu().double()
    v_got = 1.0 / stats[1].cpu().double() ** 2 - 1e-5
    em = (m_got - mean).abs().max() / var.sqrt().max()
    ev = (v_got - var).abs().max() / var.max()
    assert _note(c, what + " mean", em / 1e-3) <= 1.0, what
    assert _note(c, what + " var", ev / 1e-3) <= 1.0, what


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _nhwc(t, Cp, dt, dev, pad=0):
    return ops.nchw_to_nhwc(t.to(dev), Cp, dt, pad=pad)


def _krsc(w, g, dt, dev):
    out = torch.empty((g.K, g.R, g.S, g.C), device=dev, dtype=dt)
    ops.weight_prep(w.to(dev), dt, g.C, g.S, out, None)
    return out


def _out(dev, dt, g):
    """The forward's output: NaN, guarded by 256 rows on either side."""
    return Guarded(dev, dt, g.N * g.P * g.Q * g.K, 256 * g.K)


def _part(dev, g):
    return Guarded(dev, torch.float32, ops.conv_fwd_partial_floats(g), 256 * 3 * 4)


# ---- one runner per (pass, form)
def run_fwd(c, dev, monkeypatch):
    g, dt = cc.geom(c), DT[c.dtype]
    x, w, ref = fwd_data(c.geom, c.dtype)
    xh = _nhwc(x, g.C, dt, dev, pad=_image_and_pad(c.geom)[2] if g.pad == 0 and _is_stem(c.geom) else 0)
    y, part = _out(dev, dt, g), _part(dev, g)
    ops.conv_fwd(g, xh, _krsc(w, g, dt, dev), y.t, part.t)
    torch.cuda.synchronize()
    assert y.intact(), "write outside the output"
    tiles = ops.conv_fwd_partial_tiles(g, dt)
    _records(c, "records", part, tiles, g.K)
    _check_out(c, "y", y.t, ref)
    _check_stats(c, "stats", part, tiles, g.K, ref, dev)


def run_fold(c, dev, monkeypatch):
    g, dt = cc.geom(c), DT[c.dtype]
    x, w, s, b, r, pre = fold_data(c.geom, c.dtype)
    krsc = torch.empty((g.K, g.R, g.S, g.C), device=dev, dtype=dt)
    ops.weight_prep_batch([(w.to(dev), g.C, g.S, krsc, None, s.to(dev))], dt)
    xh, rh, bd = _nhwc(x, g.C, dt, dev), _nhwc(r, g.K, dt, dev), b.to(dev)
    for res, relu in ((True, True), (False, True), (False, False)):
        ref = pre + r.double() if res else pre
        ref = ref.clamp_min(0) if relu else ref
        y = _out(dev, dt, g)
        ops.conv_fwd_bias(g, xh, krsc, bd, rh if res else None, relu, y.t)
        torch.cuda.synchronize()
        assert y.intact(), "write outside the output"
        _check_out(c, f"y res={int(res)} relu={int(relu)}", y.t, ref, pre=pre if res else None)


def run_fwd_ds(c, dev, monkeypatch):
    g, gd, dt = cc.geom(c), cc.ds_geom(c), DT[c.dtype]
    x, w, ref = fwd_data(c.geom, c.dtype)
    wd, ref_ds = ds_data(c.geom, c.dtype)
    xh, krsc, kds = _nhwc(x, g.C, dt, dev), _krsc(w, g, dt, dev), _krsc(wd, gd, dt, dev)
    runs = []
    for separate in (False, True):
        if separate:  # the two launches, under the same forced tile
            monkeypatch.setenv("SSIP_NO_FWD_DSFUSE", "1")
        y, yd, p, pd = _out(dev, dt, g), _out(dev, dt, gd), _part(dev, g), _part(dev, gd)
        tiles = (ops.conv_fwd_partial_tiles(g, dt), ops.conv_fwd_ds_partial_tiles(g, gd, dt))
        ops.conv_fwd_ds(g, xh, krsc, y.t, p.t, gd, kds, yd.t, pd.t)
        torch.cuda.synchronize()
        assert y.intact() and yd.intact(), "write outside an output"
        recs = (_records(c, "records", p, tiles[0], g.K), _records(c, "ds records", pd, tiles[1], g.K))
        runs.append((y, yd, p, pd, tiles, recs))
    monkeypatch.delenv("SSIP_NO_FWD_DSFUSE")
    (y, yd, p, pd, tiles, recs), sep = runs
    assert tiles == sep[4] and tiles[1] > 0
    assert torch.equal(_bits(y.t), _bits(sep[0].t)) and torch.equal(_bits(yd.t), _bits(sep[1].t))
    assert torch.equal(recs[0], sep[5][0]) and torch.equal(recs[1], sep[5][1])
    _check_out(c, "y", y.t, ref)
    _check_out(c, "y_ds", yd.t, ref_ds)
    _check_stats(c, "stats", p, tiles[0], g.K, ref, dev)
    _check_stats(c, "ds stats", pd, tiles[1], g.K, ref_ds, dev)


def run_dgrad(c, dev, monkeypatch):
    g, dt = cc.geom(c), DT[c.dtype]
    w, dy, add, ref = dgrad_data(c.geom, c.dtype)
    crsk = torch.empty((g.C, g.R, g.S, g.K), device=dev, dtype=dt)
    ops.weight_prep(w.to(dev), dt, g.C, g.S, None, crsk)
    dyh = _nhwc(dy, g.K, dt, dev)
    n = g.N * g.H * g.W * g.C
    dx = Guarded(dev, dt, n, 256 * g.C)
    ops.conv_dgrad(g, dyh, crsk, dx.t, None)
    # accumulated in place, as the engine adds the downsample branch into dx
    dx2 = Guarded(dev, dt, n, 256 * g.C)
    dx2.t.copy_(_nhwc(add, g.C, dt, dev).reshape(-1))
    ops.conv_dgrad(g, dyh, crsk, dx2.t, dx2.t)
    torch.cuda.synchronize()
    assert dx.intact() and dx2.intact(), "write outside dx"
    _check_out(c, "dx", dx.t, ref)
    _check_out(c, "dx+add", dx2.t, ref + add.double(), pre=ref)


def _wgrad_launches(c, dev, g, launch, base):
    """launch(dw, accumulate, workspace) three times from NaN (identical bits),
    then accumulated onto base; the workspace exactly the queried bytes, guarded."""
    cols = g.R * g.S * g.C
    ws = Guarded(dev, torch.uint8, ops.conv_wgrad_workspace_bytes(g, c.budget), 256 * cols * 4, fill=0xFF)
    n = g.K * g.c_real * g.R * g.s_real
    outs = []
    for _ in range(3):
        dw = Guarded(dev, torch.float32, n, 256 * cols)
        launch(dw.t, False, ws.t)
        outs.append(dw)
    dwa = Guarded(dev, torch.float32, n, 256 * cols)
    dwa.t.copy_(base.to(dev).reshape(-1))
    launch(dwa.t, True, ws.t)
    torch.cuda.synchronize()
    assert ws.intact(), "write outside the workspace"
    assert all(d.intact() for d in outs + [dwa]), "write outside dw"
    assert torch.equal(_bits(outs[0].t), _bits(outs[1].t)) and torch.equal(_bits(outs[0].t), _bits(outs[2].t))
    return outs[0].t, dwa.t


def run_wgrad(c, dev, monkeypatch):
    g, dt = cc.geom(c), DT[c.dtype]
    x, dy, ref, base = wgrad_data(c.geom, c.dtype)
    xh = _nhwc(x, g.C, dt, dev, pad=_image_and_pad(c.geom)[2] if g.pad == 0 and _is_stem(c.geom) else 0)
    dyh = _nhwc(dy, g.K, dt, dev)
    dw, dwa = _wgrad_launches(c, dev, g, lambda d, acc, ws: ops.conv_wgrad(g, dyh, xh, d, acc, ws, c.budget), base)
    _check_dw(c, "dw", dw, ref)
    _check_dw(c, "dw accumulated", dwa.cpu().double() - base.double().reshape(-1), ref.reshape(-1))


def run_inbn_fwd(c, dev, monkeypatch):
    g, dt = cc.geom(c), DT[c.dtype]
    assert ops.conv_bnrelu_in_supported(g, dt)
    y_in, scale, shift, z_ref, w, dy, ref, refw, base = inbn_data(c.geom)
    yh, sc, sh, krsc = _nhwc(y_in, g.C, dt, dev), scale.to(dev), shift.to(dev), _krsc(w, g, dt, dev)
    tiles = ops.conv_fwd_partial_tiles(g, dt)
    out, part = _out(dev, dt, g), _part(dev, g)
    ops.conv_fwd_bnrelu_in(g, yh, sc, sh, krsc, out.t, part.t)
    # the apply pass + the plain conv on the same tile
    z = Guarded(dev, dt, yh.numel(), 256 * g.C)
    ops.bn_apply(g.N * g.H * g.W, g.C, yh, sc, sh, None, True, z.t)
    out2, part2 = _out(dev, dt, g), _part(dev, g)
    ops.conv_fwd(g, z.t, krsc, out2.t, part2.t)
    torch.cuda.synchronize()
    assert out.intact() and out2.intact(), "write outside the output"
    rec, rec2 = _records(c, "records", part, tiles, g.K), _records(c, "plain records", part2, tiles, g.K)
    assert torch.equal(_bits(out.t), _bits(out2.t)) and torch.equal(rec, rec2)
    assert torch.equal(z.t.float().cpu().reshape(g.N, g.H, g.W, g.C), z_ref.permute(0, 2, 3, 1))
    if g.R == 1:  # the same launch storing z as it forms its tiles
        zo, out_z, part_z = Guarded(dev, dt, yh.numel(), 256 * g.C), _out(dev, dt, g), _part(dev, g)
        ops.conv_fwd_bnrelu_in(g, yh, sc, sh, krsc, out_z.t, part_z.t, z_out=zo.t)
        torch.cuda.synchronize()
        assert zo.intact() and out_z.intact(), "write outside z_out / the output"
        assert torch.equal(_bits(zo.t), _bits(z.t))
        assert torch.equal(_bits(out_z.t), _bits(out.t))
        assert torch.equal(_records(c, "z_out records", part_z, tiles, g.K), rec)
    _check_out(c, "y", out.t, ref)
    _check_stats(c, "stats", part, tiles, g.K, ref, dev)


def run_inbn_wgrad(c, dev, monkeypatch):
    g, dt = cc.geom(c), DT[c.dtype]
    assert ops.conv_bnrelu_in_supported(g, dt)
    y_in, scale, shift, z_ref, w, dy, ref, refw, base = inbn_data(c.geom)
    yh, sc, sh, dyh = _nhwc(y_in, g.C, dt, dev), scale.to(dev), shift.to(dev), _nhwc(dy, g.K, dt, dev)
    z = torch.empty_like(yh)
    ops.bn_apply(g.N * g.H * g.W, g.C, yh, sc, sh, None, True, z)
    dw, dwa = _wgrad_launches(
        c, dev, g, lambda d, acc, ws: ops.conv_wgrad_bnrelu_in(g, dyh, yh, sc, sh, d, acc, ws, c.budget), base)
    dw2, dwa2 = _wgrad_launches(c, dev, g, lambda d, acc, ws: ops.conv_wgrad(g, dyh, z, d, acc, ws, c.budget), base)
    assert torch.equal(_bits(dw), _bits(dw2)) and torch.equal(_bits(dwa), _bits(dwa2))
    _check_dw(c, "dw", dw, refw)
    _check_dw(c, "dw accumulated", dwa.cpu().double() - base.double().reshape(-1), refw.reshape(-1))


RUN = {("fwd", "plain"): run_fwd, ("fwd", "stem"): run_fwd, ("fwd", "fold"): run_fold, ("fwd", "fwd_ds"): run_fwd_ds,
       ("fwd", "inbn"): run_inbn_fwd, ("dgrad", "plain"): run_dgrad, ("wgrad", "plain"): run_wgrad,
       ("wgrad", "stem"): run_wgrad, ("wgrad", "inbn"): run_inbn_wgrad}


@pytest.mark.parametrize("c", CASES, ids=cc.case_id)
def test_instance_matches_float64_reference(dev, monkeypatch, c):
    for name in ops._PLAN_ENV:
        monkeypatch.delenv(name, raising=False)
    for name, value in cc.env_items(c):
        monkeypatch.setenv(name, value)
    name = ops.conv_kernel_name(c.pas, cc.geom(c), DT[c.dtype], c.budget)
    assert name.startswith(c.expect), (name, c.expect)
    RUN[(c.pas, c.form)](c, dev, monkeypatch)

"""ResNet-18/50 on the ssip HIP kernels, behind the torchvision module API.

Reference boundary: `create_model` (src/training/common.py:299-304) returns a
torchvision ``resnet18`` whose ``fc`` is replaced by ``nn.Linear(512, C)``;
the train loop calls ``model(inputs)`` with f32 NCHW batches
(common.py:380), ``loss.backward()`` (:382) and ``optimizer.step()``
(:383); checkpoints are ``model.state_dict()`` (:418-424) with torchvision
key names; feature extraction uses ``children()[:-1]`` = everything up to
the global average pool (src/feature_extraction.py:210-227).

Design (MI355X-first):
  * The nn.Module tree below is a *parameter container* that mirrors
    torchvision's construction order exactly (same RNG consumption, same
    state_dict keys/shapes), so seeded initialisation and checkpoints are
    interchangeable with torchvision's.  Its submodules are never called.
  * ``forward`` runs the whole network as ONE autograd node whose forward
    and backward are sequences of C-ABI launches (libssip_hip.so) on NHWC
    activations in bf16 or f32; weight gradients are written straight into
    ``param.grad`` (views into one flat fp32 arena when the model is
    flattened for the fused optimizer / RCCL all-reduce).
  * BatchNorm semantics follow torch: train mode uses batch statistics and
    updates running stats (also in the frozen-backbone stage,
    src/training/semi_supervised.py:260-285), eval mode uses running stats.
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from . import ops
from .ops import ConvGeom

# ---------------------------------------------------------------------------
# knobs: every environment variable this module reads, read once, here.  Tests
# and tools set these module attributes by name (bench.py the two WGRAD_*
# ones); the engine reads them at call time.
# ---------------------------------------------------------------------------
# dgrad epilogue + BN-backward reduction fusion (ssip_conv_dgrad_bn); see
# _Backward.conv_dgrad_bn.  Default (""): where the dgrad runs on the halo
# kernel (layer 1: 3x3 / stride 1 / 64 channels) and the BN below has no
# residual add; "1": everywhere, "0": nowhere.
_FUSE_BN_BWD = os.environ.get("SSIP_FUSE_BN_BWD", "")
# BN+ReLU of a block's first conv applied inside its second conv (layer 1's
# halo geometry: ssip_conv_fwd_bnrelu_in / ssip_conv_wgrad_bnrelu_in) instead
# of a separate apply pass (SSIP_BNRELU_IN=0: the apply pass)
_BNRELU_IN = os.environ.get("SSIP_BNRELU_IN", "1") != "0"
# SSIP_BNRELU_Z=1: with a backward to follow, the conv also writes the BN+ReLU
# output (each row once, from the tiles it forms) so its weight gradient is the
# plain halo wgrad (the in-tile transform makes that one 50-100 us longer
# beside the main stream's layer-1 backward).  Measured 6.216 vs 6.196 ms
# (4 + 4): the forward's extra 103 MB of stores cost more.  Off by default.
_BNRELU_Z = os.environ.get("SSIP_BNRELU_Z", "0") == "1"
# SSIP_NO_FWD_DSFUSE=1: a downsampling block's conv1 and its 1x1 downsample as
# two forward launches instead of one (ops.conv_fwd_ds), for A/B
_NO_FWD_DS = os.environ.get("SSIP_NO_FWD_DSFUSE") == "1"
# eval-mode BatchNorm folded into the convs (SSIP_NO_BN_FOLD=1: separate BN passes, for A/B)
_FOLD_EVAL_BN = os.environ.get("SSIP_NO_BN_FOLD") != "1"
# Weight gradients sit off the backward's critical path (dout -> BN backward ->
# dgrad -> next dout): they run on a second stream, forked from the main one
# before each wgrad and joined at the end of the backward, so the HBM- and
# latency-bound BN-backward passes and finalize launches overlap with them.
# WGRAD_SIDE_STREAM = False (SSIP_WGRAD_STREAM=0) serialises everything on the
# current stream.
WGRAD_SIDE_STREAM = os.environ.get("SSIP_WGRAD_STREAM", "1") != "0"
# measurement only (bench.py's production roofline leg): keep the side
# stream's wgrad grid budgets when everything runs serialised on one stream
WGRAD_BUDGET_SERIAL = False
# Share of the CUs the persistent layer-1 wgrad gets on the side stream (see
# _side_wgrad_budget).  Swept four times as SSIP_HALO_WG_FRAC (0.375 / 0.5 /
# 0.625 / 0.75 / 1.0): 0.5 stayed every time, so the switch is gone.
_HALO_WGRAD_CU_SHARE = 0.5

# per-process caches of the host-side answers the knobs above do not change
_fuse_cache: dict = {}    # (geometry, dtype) -> the dgrad is a halo kernel
_side_streams: dict = {}  # device index -> the wgrad side stream
_cus: dict = {}           # device index -> CU count
_side_budgets: dict = {}  # (geometry, dtype, device index) -> side-stream wgrad grid cap

# ---------------------------------------------------------------------------
# parameter containers (torchvision-compatible structure and init order)
# ---------------------------------------------------------------------------


def _conv3x3(i, o, stride=1):
    return nn.Conv2d(i, o, kernel_size=3, stride=stride, padding=1, bias=False)


def _conv1x1(i, o, stride=1):
    return nn.Conv2d(i, o, kernel_size=1, stride=stride, bias=False)


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = _conv3x3(inplanes, planes, stride)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = _conv3x3(planes, planes)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = downsample
        self.stride = stride

    def stages(self):
        return [(self.conv1, self.bn1), (self.conv2, self.bn2)]

    def forward(self, x):  # pragma: no cover - containers are never executed
        raise RuntimeError("ssip blocks are parameter containers; call the top-level model")


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        width = planes
        self.conv1 = _conv1x1(inplanes, width)
        self.bn1 = nn.BatchNorm2d(width)
        self.conv2 = _conv3x3(width, width, stride)
        self.bn2 = nn.BatchNorm2d(width)
        self.conv3 = _conv1x1(width, planes * self.expansion)
        self.bn3 = nn.BatchNorm2d(planes * self.expansion)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride

    def stages(self):
        return [(self.conv1, self.bn1), (self.conv2, self.bn2), (self.conv3, self.bn3)]

    def forward(self, x):  # pragma: no cover
        raise RuntimeError("ssip blocks are parameter containers; call the top-level model")


ARCHS = {
    "resnet18": (BasicBlock, [2, 2, 2, 2]),
    "resnet34": (BasicBlock, [3, 4, 6, 3]),
    "resnet50": (Bottleneck, [3, 4, 6, 3]),
}

_DTYPES = {"fp32": torch.float32, "f32": torch.float32, "float32": torch.float32,
           "bf16": torch.bfloat16, "bfloat16": torch.bfloat16}


STEM_PAD = 3  # torchvision conv1 padding; the input producers pre-apply it


@dataclass
class DeviceImages:
    """A batch already in the stem's NHWC4 layout and the engine dtype
    (produced by ``ssip.augment``): skips the NCHW->NHWC conversion.

    ``buf`` is [B, H+2*pad, W+2*pad, 4] with a zero border of ``pad`` pixels:
    with pad == 3 (the stem conv's own padding) the stem runs as a pad-0 conv
    whose 16-byte pixel-pair loads are aligned and never straddle the border.
    """

    buf: torch.Tensor
    pad: int = 0

    @property
    def nhwc4(self) -> torch.Tensor:
        """The unpadded [B, H, W, 4] image (a view)."""
        p = self.pad
        if p == 0:
            return self.buf
        return self.buf[:, p:self.buf.shape[1] - p, p:self.buf.shape[2] - p, :]

    def __len__(self):
        return self.buf.shape[0]


class _Identity(nn.Module):
    def forward(self, x):
        return x


# ---------------------------------------------------------------------------
# saved forward state
# ---------------------------------------------------------------------------
@dataclass
class _ConvRec:
    geom: ConvGeom
    conv: nn.Conv2d
    bn: nn.BatchNorm2d
    x: torch.Tensor          # conv input  [N,H,W,C]
    y: torch.Tensor          # conv output [N,P,Q,K] (pre-BN)
    stats: torch.Tensor      # [4, K] mean, invstd, scale, shift
    # a block's last conv, saved for a backward: the ReLU mask of the block's
    # output, one bit per element (the backward never reads the output itself)
    zbits: Optional[torch.Tensor] = None
    # x is y of the BN+ReLU below and this conv forms relu(x * scale + shift)
    # in its LDS tile (ssip_conv_*_bnrelu_in): (scale, shift)
    in_bn: Optional[Tuple[torch.Tensor, torch.Tensor]] = None


@dataclass
class _BlockRec:
    recs: List[_ConvRec]        # the main path's convs, first to last
    ds: Optional[_ConvRec]      # the downsample conv, if the block has one
    x: torch.Tensor             # the block's input


@dataclass
class _Saved:
    dtype: torch.dtype
    N: int
    stem: _ConvRec = None
    pool_idx: torch.Tensor = None
    pool_ymax: torch.Tensor = None  # pre-BN y at each max-pool window's argmax (stem backward)
    pool_hw: Tuple[int, int] = (0, 0)
    blocks: List[_BlockRec] = field(default_factory=list)
    feat: torch.Tensor = None
    logits: Optional[torch.Tensor] = None
    last: torch.Tensor = None
    last_pq: int = 0


class SSIPResNet(nn.Module):
    """torchvision-compatible ResNet whose compute runs on libssip_hip.so."""

    def __init__(self, arch: str = "resnet18", num_classes: int = 1000, dtype: str = "fp32"):
        super().__init__()
        block, layers = ARCHS[arch]
        self.arch = arch
        self.inplanes = 64
        self.dilation = 1
        self.groups = 1
        self.base_width = 64
        self.conv1 = nn.Conv2d(3, self.inplanes, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(self.inplanes)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = self._make_layer(block, 64, layers[0])
        self.layer2 = self._make_layer(block, 128, layers[1], stride=2)
        self.layer3 = self._make_layer(block, 256, layers[2], stride=2)
        self.layer4 = self._make_layer(block, 512, layers[3], stride=2)
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(512 * block.expansion, num_classes)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, (nn.BatchNorm2d, nn.GroupNorm)):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        self.compute_dtype = _DTYPES[dtype]
        self.bn_update_running = True   # may be switched off for no-update batch-stat passes
        # (id(conv), dtype) -> [krsc, crsk or None, weight version they were made from]
        self._prep: Dict[Tuple[int, torch.dtype], list] = {}
        # (id(conv), dtype) -> [krsc with the eval BN folded in, bias, state stamp]
        self._fold: Dict[Tuple[int, torch.dtype], list] = {}
        self._bn_epoch = 0
        self._arena = None
        self.embedding_only = False
        # the CPU device was asked for (src.feature_extraction --device cpu):
        # a CPU model's eval forward runs ssip/host.py instead of raising
        self.host_execution = False
        # backward tail (single process, SemiStep): leave the stem wgrad (the
        # last kernel of the backward, on the wgrad side stream) unjoined; the
        # main stream only waits for the wgrads before it, so the optimizer
        # and the compute-dtype weight refresh of every other parameter overlap
        # it.  The caller must ops.wait_stream(main, model.take_pending_side())
        # before it reads conv1.weight.grad.
        self.defer_stem_wgrad_join = False
        self._pending_side = None
        # (single process, SemiStep) called once the backward has enqueued every
        # gradient of the blocks from `early_update_block` up and of the head:
        # early_update(stream that holds the last of those wgrads)
        self.early_update = None
        self.early_update_block = -1

    def _make_layer(self, block, planes, blocks, stride=1):
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(
                _conv1x1(self.inplanes, planes * block.expansion, stride),
                nn.BatchNorm2d(planes * block.expansion),
            )
        layers = [block(self.inplanes, planes, stride, downsample)]
        self.inplanes = planes * block.expansion
        for _ in range(1, blocks):
            layers.append(block(self.inplanes, planes))
        return nn.Sequential(*layers)

    # ------------------------------------------------------------------
    def set_compute_dtype(self, dtype: str) -> "SSIPResNet":
        self.compute_dtype = _DTYPES[dtype]
        self._prep.clear()
        self._fold.clear()
        return self

    def blocks(self):
        for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
            for b in layer:
                yield b

    def _apply(self, fn, *args, **kwargs):
        self._prep.clear()
        self._fold.clear()
        self._arena = None
        return super()._apply(fn, *args, **kwargs)

    # ------------------------------------------------------------------
    # flat parameter arena (fused optimizer / bucketed all-reduce)
    # ------------------------------------------------------------------
    def flatten_parameters(self):
        """Re-home every parameter (and its grad) into one contiguous fp32
        buffer, in ``named_parameters()`` order.  Idempotent."""
        from .arena import ParamArena

        if self._arena is None or not self._arena.valid():
            self._arena = ParamArena(list(self.parameters()))
        return self._arena

    def take_pending_side(self):
        """The side stream whose stem wgrad the last backward left unjoined
        (defer_stem_wgrad_join), or None; clears it."""
        s, self._pending_side = self._pending_side, None
        if self._arena is not None and self._arena.pending_side is s:
            self._arena.pending_side = None
        return s

    def join_pending_side(self) -> None:
        """The current stream waits for a stem wgrad left unjoined (no-op otherwise)."""
        s = self.take_pending_side()
        if s is not None:
            ops.wait_stream(torch.cuda.current_stream(s.device), s)

    def prepare_weights(self, need_t: bool = True, force: bool = False) -> None:
        """Refresh the compute-dtype conv weight copies now (one launch) so a
        later forward on another stream only reads them.  force: refresh all
        of them regardless of version (a captured step must always contain
        the refresh)."""
        _prepare_weights(self, need_t, force)

    # ------------------------------------------------------------------
    def forward(self, x):
        # a previous backward's deferred stem wgrad still writes conv1's grad
        self.join_pending_side()
        if isinstance(x, DeviceImages):
            images, pad = x.buf, x.pad
            if pad not in (0, self.conv1.padding[0]):
                images, pad = x.nhwc4, 0
            if images.dtype != self.compute_dtype or not images.is_contiguous():
                images = images.to(self.compute_dtype).contiguous()
        else:
            dev = self.conv1.weight.device
            if dev.type != "cuda":
                if self.host_execution:
                    # the frozen eval pass on the CPU, asked for explicitly
                    # (feature extraction --device cpu): ssip/host.py
                    from .host import host_forward

                    return host_forward(self, x)
                raise RuntimeError("SSIPResNet runs on the HIP device only; call model.to('cuda') first")
            x = x.to(dev, non_blocking=True)
            if x.dim() != 4 or x.shape[1] != 3:
                raise ValueError(f"expected a [B,3,H,W] batch, got {tuple(x.shape)}")
            pad = self.conv1.padding[0]
            images = ops.nchw_to_nhwc(x, 4, self.compute_dtype, pad=pad)
        params = [p for p in self.parameters()]
        if not (torch.is_grad_enabled() and any(p.requires_grad for p in params)):
            # inference (eval, pseudo-labelling, weak view, extraction): no autograd node, nothing saved
            sv = _forward(self, images, train=self.training, save=False, in_pad=pad)
            return sv.feat.view(sv.N, -1, 1, 1) if self.embedding_only else sv.logits
        return _NetFn.apply(self, images, pad, *params)


class _NetFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model: SSIPResNet, images: torch.Tensor, in_pad: int, *params):
        train = model.training
        saved = _forward(model, images, train=train, save=train, in_pad=in_pad)
        ctx.model = model
        ctx.saved = saved
        out = saved.feat.view(saved.N, -1, 1, 1) if model.embedding_only else saved.logits
        if model.embedding_only:
            ctx.mark_non_differentiable(out)
        return out

    @staticmethod
    def backward(ctx, dlogits):
        model: SSIPResNet = ctx.model
        saved: _Saved = ctx.saved
        if saved is None or saved.stem is None or not model.training:
            raise RuntimeError("ssip: backward requires a train-mode forward with trainable parameters")
        _backward(model, saved, dlogits.contiguous().float())
        ctx.saved = None
        return (None, None, None) + (None,) * len(list(model.parameters()))


# ---------------------------------------------------------------------------
# forward engine
# ---------------------------------------------------------------------------
def _geom(conv: nn.Conv2d, N: int, H: int, W: int, in_pad: int = 0) -> ConvGeom:
    """in_pad: the input already carries a zero border of the conv's own
    padding (H, W include it) -> a pad-0 conv over the padded image."""
    K, C, R, S = conv.weight.shape
    stem = C == 3
    pad = conv.padding[0]
    if in_pad:
        assert in_pad == pad, "pre-padded input must carry exactly the conv padding"
        pad = 0
    return ConvGeom(N=N, H=H, W=W, C=4 if stem else C, K=K, R=R, S=8 if stem else S,
                    stride=conv.stride[0], pad=pad, c_real=C, s_real=S)


def _prepare_weights(model: SSIPResNet, need_t: bool, force: bool = False) -> None:
    """Refresh the compute-dtype KRSC (forward) and CRSK (data-gradient)
    copies of every conv weight whose fp32 master changed since the last
    refresh (torch version counter; ssip.optim.AdamW bumps it), in one
    batched launch — once per optimizer step, not once per forward."""
    dt = model.compute_dtype
    items = []
    for conv in model.modules():
        if not isinstance(conv, nn.Conv2d):
            continue
        w = conv.weight
        key = (id(conv), dt)
        ent = model._prep.get(key)
        if not force and ent is not None and ent[2] == w._version and (ent[1] is not None or not need_t):
            continue
        g = _geom(conv, 1, 1, 1)
        if ent is None or (need_t and ent[1] is None):
            krsc = torch.empty((g.K, g.R, g.S, g.C), device=w.device, dtype=dt)
            crsk = torch.empty((g.C, g.R, g.S, g.K), device=w.device, dtype=dt) if need_t else None
        else:
            krsc, crsk = ent[0], ent[1]
        model._prep[key] = [krsc, crsk, w._version]
        items.append((w.detach(), g.C, g.S, krsc, crsk))
    if items:
        ops.weight_prep_batch(items, dt)


def _prepped(model: SSIPResNet, conv: nn.Conv2d, g: ConvGeom, need_t: bool):
    ent = model._prep.get((id(conv), model.compute_dtype))
    if ent is None or ent[2] != conv.weight._version or (need_t and ent[1] is None):
        _prepare_weights(model, need_t)
        ent = model._prep[(id(conv), model.compute_dtype)]
    return ent


def _bn_stats(bn, K: int, tiles: int, partial, train: bool, update_running: bool, stats: torch.Tensor) -> None:
    """stats [4, K] = mean, invstd, scale, shift of `bn`: in train mode from
    the producing conv's per-tile records (`tiles` per channel in `partial`;
    the running statistics move when update_running), else from the running
    statistics."""
    gamma, beta = bn.weight.detach(), bn.bias.detach()
    if train:
        ops.bn_finalize(K, tiles, partial, gamma, beta, bn.running_mean, bn.running_var,
                        bn.momentum if bn.momentum is not None else 0.1, bn.eps, update_running,
                        stats[0], stats[1], stats[2], stats[3])
    else:
        ops.bn_eval_coeffs(K, gamma, beta, bn.running_mean, bn.running_var, bn.eps,
                           stats[0], stats[1], stats[2], stats[3])


def _conv_bn(model: SSIPResNet, conv, bn, x: torch.Tensor, N, H, W, train: bool, save: bool,
             update_running: bool, in_pad: int = 0, in_bn=None) -> _ConvRec:
    """in_bn = (scale, shift): x is the pre-BN y of the BN+ReLU below, applied
    inside the conv (train mode, _bnrelu_in_ok geometries)."""
    g = _geom(conv, N, H, W, in_pad)
    dt = model.compute_dtype
    krsc = _prepped(model, conv, g, need_t=save)[0]
    y = torch.empty((N, g.P, g.Q, g.K), device=x.device, dtype=dt)
    stats = torch.empty((4, g.K), device=x.device, dtype=torch.float32)
    partial = torch.empty(ops.conv_fwd_partial_floats(g), device=x.device, dtype=torch.float32) if train else None
    if in_bn is not None:
        # z_out: the halo forward writes it under SSIP_BNRELU_Z; a 1x1 conv
        # on the LDS-DMA ring always does (its in-ring wgrad transform sits
        # on the side stream's one-workgroup-per-CU grid and costs more
        # than the stores: profiles/r6_bnrelu_in_glds_lab.txt)
        one = g.R == 1 and g.S == 1
        z = torch.empty_like(x) if (save and (_BNRELU_Z or one)) else None
        ops.conv_fwd_bnrelu_in(g, x, in_bn[0], in_bn[1], krsc, y, partial, z_out=z)
        if z is not None:
            # the conv wrote relu(bn(x)) as it formed its tiles: the weight
            # gradient takes it as a plain input
            x, in_bn = z, None
    else:
        ops.conv_fwd(g, x, krsc, y, partial)
    _bn_stats(bn, g.K, ops.conv_fwd_partial_tiles(g, dt) if train else 0, partial, train, update_running, stats)
    return _ConvRec(geom=g, conv=conv, bn=bn, x=x, y=y, stats=stats, in_bn=in_bn)


def _bnrelu_in_ok(conv, N: int, H: int, W: int, dtype) -> bool:
    return _BNRELU_IN and ops.conv_bnrelu_in_supported(_geom(conv, N, H, W), dtype)


def _conv_bn_ds(model: SSIPResNet, conv, bn, ds_conv, ds_bn, x: torch.Tensor, N, H, W, train: bool, save: bool,
                update_running: bool) -> Tuple[_ConvRec, _ConvRec]:
    """_conv_bn of a downsampling block's conv1 and of its 1x1 downsample in
    one fused launch (ops.conv_fwd_ds): same input, same output grid."""
    g = _geom(conv, N, H, W)
    gd = _geom(ds_conv, N, H, W)
    dt = model.compute_dtype
    krsc = _prepped(model, conv, g, need_t=save)[0]
    kds = _prepped(model, ds_conv, gd, need_t=save)[0]
    recs = []
    ys, parts, stats = [], [], []
    for gg in (g, gd):
        ys.append(torch.empty((N, gg.P, gg.Q, gg.K), device=x.device, dtype=dt))
        stats.append(torch.empty((4, gg.K), device=x.device, dtype=torch.float32))
        parts.append(torch.empty(ops.conv_fwd_partial_floats(gg), device=x.device, dtype=torch.float32)
                     if train else None)
    ops.conv_fwd_ds(g, x, krsc, ys[0], parts[0], gd, kds, ys[1], parts[1])
    tiles = (ops.conv_fwd_partial_tiles(g, dt), ops.conv_fwd_ds_partial_tiles(g, gd, dt))
    for gg, c, b, y, part, st, nt in zip((g, gd), (conv, ds_conv), (bn, ds_bn), ys, parts, stats, tiles):
        _bn_stats(b, gg.K, nt, part, train, update_running, st)
        recs.append(_ConvRec(geom=gg, conv=c, bn=b, x=x, y=y, stats=st))
    return recs[0], recs[1]


def _fwd_ds_fusable(blk, N: int, H: int, W: int) -> bool:
    """BasicBlock conv1 (3x3, pad 1, stride s) + downsample (1x1, stride s): ops.conv_fwd_ds."""
    if _NO_FWD_DS or blk.downsample is None or not isinstance(blk, BasicBlock):
        return False
    g = _geom(blk.conv1, N, H, W)
    gd = _geom(blk.downsample[0], N, H, W)
    return (g.R, g.S, g.pad, gd.R, gd.S, gd.pad, gd.stride) == (3, 3, 1, 1, 1, 0, g.stride) and \
        (g.P, g.Q, g.K, g.C) == (gd.P, gd.Q, gd.K, gd.C)


def _forward_block_folded(model: SSIPResNet, blk, x: torch.Tensor, N, H, W):
    """One block in eval mode with its BNs folded (_prepare_folded): each conv
    carries its BN as scaled weights + bias, and the ReLU / residual add run in
    the conv epilogue (no BN passes).  -> (block output, its H, W)"""
    dt, dev = model.compute_dtype, x.device
    ident = x
    if blk.downsample is not None:
        gd = _geom(blk.downsample[0], N, H, W)
        kr, b = model._fold[(id(blk.downsample[0]), dt)][:2]
        ident = torch.empty((N, gd.P, gd.Q, gd.K), device=dev, dtype=dt)
        ops.conv_fwd_bias(gd, x, kr, b, None, False, ident)
    stages = blk.stages()
    for i, (conv, bn) in enumerate(stages):
        g = _geom(conv, N, H, W)
        kr, b = model._fold[(id(conv), dt)][:2]
        out = torch.empty((N, g.P, g.Q, g.K), device=dev, dtype=dt)
        ops.conv_fwd_bias(g, x, kr, b, ident if i == len(stages) - 1 else None, True, out)
        x, H, W = out, g.P, g.Q
    return x, H, W


def _forward_block(model: SSIPResNet, blk, x: torch.Tensor, N, H, W, train: bool, save: bool, upd: bool):
    """One block with its BNs as passes of their own (train mode, or eval
    unfolded).  -> (block output, its H, W, the _BlockRec a backward needs)"""
    dt, dev = model.compute_dtype, x.device
    recs = []
    z, h, w = x, H, W
    stages = blk.stages()
    ds = None
    fuse_ds = _fwd_ds_fusable(blk, N, H, W)
    in_bn = None
    for i, (conv, bn) in enumerate(stages):
        if i == 0 and fuse_ds:
            r, ds = _conv_bn_ds(model, conv, bn, blk.downsample[0], blk.downsample[1], z, N, h, w, train, save, upd)
        else:
            r = _conv_bn(model, conv, bn, z, N, h, w, train, save, upd, in_bn=in_bn)
        in_bn = None
        h, w = r.geom.P, r.geom.Q
        if i < len(stages) - 1:
            if train and _bnrelu_in_ok(stages[i + 1][0], N, h, w, dt):
                # the next conv applies this BN+ReLU itself; its input and
                # its wgrad's stay the pre-BN y (the backward's mask comes
                # from y and the affine, so z is never needed)
                z, in_bn = r.y, (r.stats[2], r.stats[3])
            else:
                z = torch.empty_like(r.y)
                ops.bn_apply(N * h * w, r.geom.K, r.y, r.stats[2], r.stats[3], None, True, z)
        recs.append(r)
    last = recs[-1]
    out = torch.empty_like(last.y)
    # the backward masks with 1 bit per element instead of re-reading out
    bits = torch.empty(out.numel() // 8, device=dev, dtype=torch.uint8) if save else None
    if blk.downsample is not None:
        # out = relu(bn2(y2) + bn_ds(y_ds)): the downsample's BN is formed in
        # registers by the same pass (its output is never stored)
        if ds is None:
            ds = _conv_bn(model, blk.downsample[0], blk.downsample[1], x, N, H, W, train, save, upd)
        ops.bn_apply2(N * h * w, last.geom.K, last.y, last.stats[2], last.stats[3], ds.y, ds.stats[2],
                      ds.stats[3], True, out, bits)
    else:
        ops.bn_apply(N * h * w, last.geom.K, last.y, last.stats[2], last.stats[3], x, True, out, bits)
    last.zbits = bits
    return out, h, w, _BlockRec(recs, ds, x)


def _forward(model: SSIPResNet, images: torch.Tensor, train: bool, save: bool, in_pad: int = 0) -> _Saved:
    N, H, W, C4 = images.shape
    dt = model.compute_dtype
    upd = train and model.bn_update_running
    sv = _Saved(dtype=dt, N=N)
    dev = images.device
    _prepare_weights(model, need_t=save)
    # stem: conv 7x7/2 -> BN -> ReLU -> maxpool 3x3/2
    rec = _conv_bn(model, model.conv1, model.bn1, images, N, H, W, train, save, upd, in_pad)
    g = rec.geom
    mp = model.maxpool
    k, s, pd = mp.kernel_size, mp.stride, mp.padding
    Hc = (g.P + 2 * pd - k) // s + 1
    Wc = (g.Q + 2 * pd - k) // s + 1
    x = torch.empty((N, Hc, Wc, g.K), device=dev, dtype=dt)
    # (argmax bytes only for a backward: the weak forward writes none)
    idx = torch.empty((N, Hc, Wc, g.K), device=dev, dtype=torch.uint8) if save else None
    # BN -> ReLU -> max-pool in one pass over y (the full-resolution z is never
    # stored).  (Round 5 measured the window selection inside the stem conv --
    # conv rows 2p-1..2p+1 per pooled row, BN + ReLU after on the pooled grid,
    # no y read -- at 429 us vs 164 + 180 for the two kernels: the per-element
    # selection and statistics VALU work inside the conv costs more than the
    # y read it saves; profiles/r5_stem_pool_lab.txt)
    ymax = torch.empty((N, Hc, Wc, g.K), device=dev, dtype=dt) if save else None
    ops.stem_bn_pool_fwd(N, g.P, g.Q, g.K, k, s, pd, rec.y, rec.stats[2], rec.stats[3], x, idx, ymax)
    if save:
        sv.stem, sv.pool_idx, sv.pool_ymax, sv.pool_hw = rec, idx, ymax, (g.P, g.Q)
    # blocks
    fold = not train and _FOLD_EVAL_BN
    if fold:
        _prepare_folded(model)
    for blk in model.blocks():
        if fold:
            x, Hc, Wc = _forward_block_folded(model, blk, x, N, Hc, Wc)
        else:
            x, Hc, Wc, brec = _forward_block(model, blk, x, N, Hc, Wc, train, save, upd)
            if save:
                sv.blocks.append(brec)
    # head: global average pool (+ fc)
    C = x.shape[-1]
    feat = torch.empty((N, C), device=dev, dtype=torch.float32)
    if model.embedding_only:
        ops.avgpool_fc_fwd(N, Hc * Wc, C, 0, x, None, None, feat, None)
        sv.logits = None
    else:
        J = model.fc.out_features
        logits = torch.empty((N, J), device=dev, dtype=torch.float32)
        ops.avgpool_fc_fwd(N, Hc * Wc, C, J, x, model.fc.weight.detach(), model.fc.bias.detach(), feat, logits)
        sv.logits = logits
    sv.feat = feat
    sv.last, sv.last_pq = x, Hc * Wc
    if train and upd:
        _bump_batches_tracked(model)
        model._bn_epoch += 1  # running statistics changed on the device: folded eval weights are stale
    return sv


def _prepare_folded(model: SSIPResNet) -> None:
    """Refresh the eval-mode folded copies of every block conv: w' = w * s[k]
    (s = gamma / sqrt(running_var + eps)) in the compute dtype, bias = beta -
    running_mean * s.  One coefficient launch per stale BN plus one batched
    weight launch; reused until a weight, a BN parameter or the running
    statistics change (torch version counters, and model._bn_epoch for the
    device-side running-stat updates of a train-mode forward)."""
    dt = model.compute_dtype
    items = []
    for blk in model.blocks():
        pairs = list(blk.stages()) + ([(blk.downsample[0], blk.downsample[1])] if blk.downsample is not None else [])
        for conv, bn in pairs:
            w = conv.weight
            stamp = (w._version, bn.weight._version, bn.bias._version, bn.running_mean._version,
                     bn.running_var._version, model._bn_epoch)
            key = (id(conv), dt)
            ent = model._fold.get(key)
            if ent is not None and ent[2] == stamp:
                continue
            K, C, R, S = w.shape
            if ent is None:
                ent = [torch.empty((K, R, S, C), device=w.device, dtype=dt),
                       torch.empty(K, device=w.device, dtype=torch.float32), None]
                model._fold[key] = ent
            scale = torch.empty(K, device=w.device, dtype=torch.float32)
            ops.bn_eval_coeffs(K, bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var, bn.eps,
                               None, None, scale, ent[1])
            ent[2] = stamp
            items.append((w.detach(), C, S, ent[0], None, scale))
    if items:
        ops.weight_prep_batch(items, dt)


def _bump_batches_tracked(model: SSIPResNet):
    """num_batches_tracked += 1 on every BN layer (torch's train-mode BN), one launch."""
    t = getattr(model, "_nbt", None)
    if t is None or (t and t[0].device != model.conv1.weight.device):
        t = [m.num_batches_tracked for m in model.modules()
             if isinstance(m, nn.BatchNorm2d) and m.num_batches_tracked is not None]
        model._nbt = t
    if t and t[0].is_cuda:
        ops.counters_add(t, 1)
    else:
        torch._foreach_add_(t, 1)


# ---------------------------------------------------------------------------
# backward engine
# ---------------------------------------------------------------------------
def _grad_target(p: torch.Tensor, arena) -> Tuple[torch.Tensor, bool]:
    """Tensor to write p's gradient into, and whether to accumulate."""
    if p.grad is None:
        if arena is not None and arena.owns(p):
            p.grad = arena.grad_view(p)
        else:
            p.grad = torch.empty_like(p)
        return p.grad, False
    return p.grad, True


def _cu_count(dev: torch.device) -> int:
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    n = _cus.get(idx)
    if n is None:
        n = _cus[idx] = torch.cuda.get_device_properties(idx).multi_processor_count
    return n


def _side_wgrad_budget(g, dtype, dev: torch.device) -> int:
    """Grid cap of a wgrad on the side stream, beside the main stream's dgrad /
    BN-backward chain (ssip_conv_wgrad_budget): the split-K LDS-DMA wgrads one
    workgroup per CU (SSIP_WGRAD_BLOCKS sweep: 6.431 ms at 256 vs 6.490
    uncapped), the persistent layer-1 wgrad -- one workgroup per CU holding all
    of its LDS, so a main-stream kernel cannot start beside it -- half the CUs
    (_HALO_WGRAD_CU_SHARE: 6.551 vs 6.650 ms at 100 %, 6.567 at 62 %, 6.637 at
    37 %; 3 alternated runs each, tools/gpu_r4_halo.sh)."""
    key = (g, dtype, dev.index)
    b = _side_budgets.get(key)
    if b is None:
        cus = _cu_count(dev)
        halo = ops.conv_kernel_name("wgrad", g, dtype).startswith("halo_wgrad")
        b = _side_budgets[key] = int(cus * _HALO_WGRAD_CU_SHARE) if halo else cus
    return b


def _wgrad_stream(dev: torch.device):
    if not WGRAD_SIDE_STREAM or dev.type != "cuda":
        return None
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    st = _side_streams.get(idx)
    if st is None:
        st = _side_streams[idx] = torch.cuda.Stream(device=idx)
    return st


def _fuse_bn_bwd(g: ConvGeom, dt: torch.dtype, residual: bool = False) -> bool:
    """Whether the dgrad of g also forms the ReLU mask and BN-backward reduction
    of the BN below (_FUSE_BN_BWD).  residual: that BN ends a block (mask bits
    + the identity gradient add).  (Fusing on every halo dgrad, residual ones
    included, was slower in every round of profiles/r6_knob_recheck.txt: that
    value of the knob is gone.)"""
    if _FUSE_BN_BWD in ("0", "1"):
        return _FUSE_BN_BWD == "1"
    if residual:
        return False
    key = (g, dt)
    v = _fuse_cache.get(key)
    if v is None:
        v = _fuse_cache[key] = ops.conv_kernel_name("dgrad", g, dt).startswith("halo")
    return v


def _stage_params(model: SSIPResNet):
    """(trunk parameters, per-stage parameter lists: stem, then each block),
    cached on the model (the module tree is fixed; requires_grad is read
    from the parameters at every call)."""
    st = getattr(model, "_stage_params_cache", None)
    if st is None:
        stages = [[model.conv1, model.bn1]] + [[m for m in b.modules() if m is not b] for b in model.blocks()]
        per = [[p for m in mods for p in m.parameters(recurse=False)] for mods in stages]
        st = ([p for ps in per for p in ps], per)
        object.__setattr__(model, "_stage_params_cache", st)
    return st


def _backward(model: SSIPResNet, sv: _Saved, dlogits: torch.Tensor):
    dev = dlogits.device
    side = _wgrad_stream(dev)
    if side is None:
        _Backward(model, sv, dev, None, None).run(dlogits)
        return
    main = torch.cuda.current_stream(dev)
    model._pending_side = None
    deferred = False
    try:
        deferred = _Backward(model, sv, dev, main, side).run(dlogits)
    finally:
        if deferred:
            model._pending_side = side
            if model._arena is not None:
                model._arena.pending_side = side  # AdamW.step / zero_grad join it
        else:
            ops.wait_stream(main, side)


def _hook_on_side(user_hook, main, side, params) -> None:
    """The gradient-ready hook with the wgrad side stream current: the hook's
    consumers (gradient buckets) order themselves after the current stream, and
    the side stream, joined to main here, holds every gradient of `params`."""
    side.wait_stream(main)
    with torch.cuda.stream(side):
        user_hook(params)


class _Backward:
    """One backward pass over a saved forward, head to stem: `run`.  The other
    methods are its steps; every launch goes on the current (main) stream
    except the weight gradients, which `launch_wgrad` puts on `side`."""

    def __init__(self, model: SSIPResNet, sv: _Saved, dev: torch.device, main, side):
        self.model, self.sv, self.dev = model, sv, dev
        self.dt, self.N = sv.dtype, sv.N
        self.arena = model._arena if (model._arena is not None and model._arena.valid()) else None
        self.main, self.side = main, side  # both None: everything on the current stream
        self.user_hook = getattr(model, "grad_ready_hook", None)
        self.blocks = list(model.blocks())
        # the earliest trainable stage (0: the stem, i + 1: block i) decides where dgrad can stop
        self.trunk_params, stage_params = _stage_params(model)
        self.first_trainable = next((i for i, ps in enumerate(stage_params) if any(p.requires_grad for p in ps)),
                                    None)
        self.workspace = self.coef_buf = None  # head() allocates them once it knows the trunk is trainable

    # -- the pass ---------------------------------------------------------
    def run(self, dlogits: torch.Tensor) -> bool:
        """-> the stem wgrad was left unjoined on the side stream (defer_stem_wgrad_join)"""
        dz = self.head(dlogits)
        pending = None  # (dpre, partial, tiles) of a block's last BN, formed by the dgrad of the block above
        for bi in range(len(self.sv.blocks) - 1, -1, -1):
            if dz is None:
                return False
            dz, pending = self.block(bi, dz, pending)
        return self.stem(dz) if dz is not None else False

    def grads_ready(self, params) -> None:
        """Every gradient of `params` has been enqueued: tell model.grad_ready_hook."""
        if self.user_hook is None:
            return
        if self.side is None:
            ops.host_callback(self.user_hook, params)
        else:
            ops.host_callback(_hook_on_side, self.user_hook, self.main, self.side, params)

    def head(self, dlogits: torch.Tensor) -> Optional[torch.Tensor]:
        """fc + average pool; -> the gradient of the last block's output, None
        when nothing below the head is trainable."""
        sv, fc = self.sv, self.model.fc
        C, J = sv.last.shape[-1], fc.out_features
        dw = db = None
        accw = accb = False
        if fc.weight.requires_grad:
            dw, accw = _grad_target(fc.weight, self.arena)
        if fc.bias is not None and fc.bias.requires_grad:
            db, accb = _grad_target(fc.bias, self.arena)
        if not any(p.requires_grad for p in self.trunk_params):
            if dw is not None:
                ops.avgpool_fc_bwd(self.dt, self.N, sv.last_pq, C, J, dlogits, fc.weight.detach(), sv.feat, None, dw,
                                   db, accw)
            self.grads_ready(list(fc.parameters()))
            return None
        dz = torch.empty_like(sv.last)
        if dw is not None and db is not None and accw != accb:
            raise RuntimeError("ssip: fc weight/bias grads must both be fresh or both accumulate")
        ops.avgpool_fc_bwd(self.dt, self.N, sv.last_pq, C, J, dlogits, fc.weight.detach(), sv.feat, dz, dw, db, accw)
        self.grads_ready(list(fc.parameters()))
        # one wgrad workspace for the pass: the largest any conv needs at the grid it will get
        geoms = [r.geom for b in sv.blocks for r in b.recs + ([b.ds] if b.ds is not None else [])] + [sv.stem.geom]
        ws_bytes = max(max(ops.conv_wgrad_workspace_bytes(g), ops.conv_wgrad_workspace_bytes(g, self.wgrad_budget(g)))
                       for g in geoms)
        self.workspace = torch.empty(ws_bytes, device=self.dev, dtype=torch.uint8)
        self.coef_buf = torch.empty(6 * 2048, device=self.dev, dtype=torch.float32)
        return dz

    def block(self, bi: int, dz: torch.Tensor, pending):
        """Block bi, given the gradient dz of its output (and `pending` when the
        block above already masked it and reduced it for this block's last BN).
        -> (gradient of the block's input or None, `pending` for the block below)"""
        model, blk = self.model, self.sv.blocks[bi]
        recs, ds = blk.recs, blk.ds
        need_dx = self.first_trainable is not None and self.first_trainable < bi + 1
        below = self.sv.blocks[bi - 1].recs[-1] if bi > 0 else None  # BN+ReLU producing this block's input
        dy, dy_ds, dpre = self.tail_bn(recs[-1], ds, dz, pending)
        g1 = self.conv_chain(recs, dy)
        dxin = pending = None
        ds_dgrad_left = False
        if need_dx:
            dxin = torch.empty_like(blk.x)
            if ds is None:
                pending = self.input_grad_identity(recs[0], g1, dpre, below, dxin)
            else:
                ds_dgrad_left = not self.input_grad_conv1(recs[0], ds, g1, dy_ds, below, dxin)
        if ds is not None:
            self.conv_wgrad(ds, dy_ds)
            if ds_dgrad_left:
                pending = self.input_grad_downsample(ds, dy_ds, below, dxin)
        self.grads_ready(list(self.blocks[bi].parameters()))
        if model.early_update is not None and bi == model.early_update_block:
            model.early_update(self.side if self.side is not None else self.main)
        return dxin, pending

    def stem(self, dz: torch.Tensor) -> bool:
        """max-pool backward + ReLU mask + BN backward straight from the pooled
        gradient, then conv1's wgrad; -> that wgrad was left unjoined."""
        model, sv = self.model, self.sv
        stem, mp = sv.stem, model.maxpool
        P1, Q1 = sv.pool_hw
        C1 = stem.geom.K
        dgam, dbet, acc = self.bn_grads(stem)
        partial = torch.empty(ops.stem_pool_bn_bwd_partial_floats(self.N, P1, Q1, C1), device=self.dev,
                              dtype=torch.float32)
        w1 = stem.conv.weight
        # the stem wgrad forms the BN-backward dy per tile in LDS (no full-resolution
        # dy pass) where the geometry allows: ssip_stem_bwd_wgrad
        fused = (w1.requires_grad and (mp.kernel_size, mp.stride, mp.padding) == (3, 2, 1)
                 and ops.stem_bwd_wgrad_supported(stem.geom, self.dt))
        defer = bool(fused and self.side is not None and self.user_hook is None and model.defer_stem_wgrad_join)
        dy1 = None if fused else torch.empty_like(stem.y)
        coef1 = self.coef_buf[: 3 * C1] if not fused else torch.empty(3 * C1, device=self.dev, dtype=torch.float32)
        ops.stem_pool_bn_bwd(self.N, P1, Q1, C1, mp.kernel_size, mp.stride, mp.padding, dz, sv.pool_idx, stem.y,
                             stem.stats[0], stem.stats[1], stem.stats[2], stem.stats[3], stem.bn.weight.detach(), dgam,
                             dbet, acc, dy1, partial, coef1, sv.pool_ymax)
        if fused:
            tgt, acc_w = _grad_target(w1, self.arena)
            # every tensor the side-stream kernel reads or writes was allocated
            # on main: keep the caching allocator from handing any of them to a
            # main-stream allocation before the join (deferred: after this returns)
            self.launch_wgrad(ops.stem_bwd_wgrad,
                              (stem.geom, dz, sv.pool_idx, stem.y, stem.x, stem.stats[2], stem.stats[3], coef1, tgt,
                               acc_w, self.workspace),
                              record=(dz, sv.pool_idx, stem.y, stem.x, stem.stats, coef1, self.workspace), defer=defer)
        else:
            self.conv_wgrad(stem, dy1)
        self.grads_ready([model.conv1.weight, model.bn1.weight, model.bn1.bias])
        return defer

    # -- a block's steps ----------------------------------------------------
    def tail_bn(self, last: _ConvRec, ds: Optional[_ConvRec], dz, pending):
        """The BN(s) that end a block: out = relu(BN(y_last) + identity or BN_ds(y_ds)).
        -> (dy of the last conv, dy of the downsample conv or None, dpre: the
        masked gradient that also flows to the identity, None when the dual
        form kept it in registers)"""
        if pending is None and ds is not None:
            dual = self.bn_backward_dual(last, ds, dz, last.zbits)
            if dual is not None:
                return dual[0], dual[1], None
        if pending is None:
            dpre = torch.empty_like(last.y)
            dy = self.bn_backward(last, dz, dpre, last.zbits)
        else:
            dpre, part, tiles = pending
            dy = self.bn_backward_fused(last, dpre, part, tiles)
        return dy, (self.bn_backward(ds, dpre) if ds is not None else None), dpre

    def conv_chain(self, recs: List[_ConvRec], dy: torch.Tensor) -> torch.Tensor:
        """The main path from its last conv back to its first: each conv's
        wgrad, then (above the first) its dgrad and the BN+ReLU backward below
        it.  -> the gradient of the first conv's output"""
        for i in range(len(recs) - 1, 0, -1):
            r = recs[i]
            self.conv_wgrad(r, dy)
            dzp = torch.empty_like(r.x)
            fused = self.conv_dgrad_bn(r, dy, recs[i - 1], dzp)
            if fused is None:
                dy = self.bn_relu_backward(recs[i - 1], dzp)
            else:
                dy = self.bn_backward_fused(recs[i - 1], *fused)
        self.conv_wgrad(recs[0], dy)
        return dy

    def input_grad_identity(self, r: _ConvRec, g1, dpre, below: Optional[_ConvRec], dxin):
        """dxin of a block without a downsample = dgrad(conv1) + dpre; with a
        block below, fused with that block's last BN where _fuse_bn_bwd allows
        (-> its `pending`)."""
        if below is not None:
            return self.conv_dgrad_bn(r, g1, below, dxin, dpre, residual=True)
        self.conv_dgrad(r, g1, dxin, dpre)
        return None

    def input_grad_conv1(self, r: _ConvRec, ds: _ConvRec, g1, dy_ds, below: Optional[_ConvRec], dxin) -> bool:
        """conv1's part of dxin in a block with a downsample; -> the
        downsample's part is in it too (conv1's and the downsample's input
        gradients in one launch, ssip_conv_dgrad_ds), else it has to be added
        by input_grad_downsample, after the downsample's wgrad."""
        if _ds_dgrad_fusable(r.geom, ds.geom) and (below is None or not _fuse_bn_bwd(ds.geom, self.dt, True)):
            ops.conv_dgrad_ds(r.geom, g1, _prepped_t(self.model, r)[1], ds.geom, dy_ds,
                              _prepped_t(self.model, ds)[1], dxin)
            return True
        self.conv_dgrad(r, g1, dxin)
        return False

    def input_grad_downsample(self, ds: _ConvRec, dy_ds, below: Optional[_ConvRec], dxin):
        """dxin += dgrad(downsample), fused with the last BN of the block below
        where there is one and _fuse_bn_bwd allows (-> its `pending`)."""
        if below is not None:
            return self.conv_dgrad_bn(ds, dy_ds, below, dxin, dxin, residual=True)
        self.conv_dgrad(ds, dy_ds, dxin, dxin)
        return None

    # -- weight gradients -----------------------------------------------------
    def wgrad_budget(self, g: ConvGeom) -> int:
        """Grid cap of g's wgrad: its side-stream budget when it runs beside the
        main stream (or WGRAD_BUDGET_SERIAL asks for the same grids), else 0,
        the full chip."""
        if self.side is not None or WGRAD_BUDGET_SERIAL:
            return _side_wgrad_budget(g, self.dt, self.dev)
        return 0

    def launch_wgrad(self, fn, args, record, defer: bool = False) -> None:
        """fn(*args), a weight-gradient launch: on the side stream, forked from
        main here, when there is one.  record: tensors allocated on main that
        the launch reads or writes (kept from main-stream reuse until the side
        stream is past it).  defer: the launch stays unjoined after the
        backward, so main waits here for every wgrad queued before it.
        (Round 5: holding a block's wgrads behind one event at its end -- 8
        event records instead of 19 -- made the step 3 % slower: the side
        stream idles while they wait.)"""
        if self.side is None:
            fn(*args)
            return
        ops.wait_stream(self.side, self.main)
        if defer:
            ops.wait_stream(self.main, self.side)
        with torch.cuda.stream(self.side):
            fn(*args)
        for t in record:
            t.record_stream(self.side)

    def conv_wgrad(self, rec: _ConvRec, dy: torch.Tensor) -> None:
        w = rec.conv.weight
        if not w.requires_grad:
            return
        tgt, acc = _grad_target(w, self.arena)
        budget = self.wgrad_budget(rec.geom)
        if rec.in_bn is not None:
            self.launch_wgrad(ops.conv_wgrad_bnrelu_in,
                              (rec.geom, dy, rec.x, rec.in_bn[0], rec.in_bn[1], tgt, acc, self.workspace, budget),
                              record=(dy,))
        else:
            self.launch_wgrad(ops.conv_wgrad, (rec.geom, dy, rec.x, tgt, acc, self.workspace, budget), record=(dy,))

    # -- data gradients -------------------------------------------------------
    def conv_dgrad(self, rec: _ConvRec, dy, out, add=None) -> None:
        ops.conv_dgrad(rec.geom, dy, _prepped_t(self.model, rec)[1], out, add)

    def conv_dgrad_bn(self, rec: _ConvRec, dy, below: _ConvRec, out, add=None, residual: bool = False):
        """dgrad of `rec` fused with the ReLU mask + BN-backward reduction of
        `below` (the BN+ReLU whose output is rec's input): the mask from the
        forward's mask bits where `below` ends a block (its ReLU follows the
        residual add), else from y and below's BN affine.  Only where
        _fuse_bn_bwd says so (the halo dgrads by default: the implicit-GEMM
        epilogue costs more than the reduce pass it replaces);
        elsewhere the plain dgrad, and None.
        -> (out, partial, tiles) for bn_backward_fused"""
        if not _fuse_bn_bwd(rec.geom, self.dt, residual):
            self.conv_dgrad(rec, dy, out, add)
            return None
        crsk = _prepped_t(self.model, rec)[1]
        partial = torch.empty(ops.conv_dgrad_bn_partial_floats(rec.geom), device=self.dev, dtype=torch.float32)
        bits, msc, msh = (below.zbits, None, None) if residual else (None, below.stats[2], below.stats[3])
        ops.conv_dgrad_bn(rec.geom, dy, crsk, add, None, below.y, below.stats[0], below.stats[1], out, partial,
                          mask_bits=bits, mscale=msc, mshift=msh)
        return out, partial, ops.conv_dgrad_bn_partial_tiles(rec.geom, self.dt)

    # -- BatchNorm backward ---------------------------------------------------
    def bn_grads(self, rec: _ConvRec):
        """-> (dgamma target, dbeta target, accumulate) of rec's BN"""
        bn = rec.bn
        dgam = dbet = None
        acc = False
        if bn.weight.requires_grad:
            dgam, acc = _grad_target(bn.weight, self.arena)
        if bn.bias.requires_grad:
            dbet, acc2 = _grad_target(bn.bias, self.arena)
            if dgam is not None and acc2 != acc:
                raise RuntimeError("ssip: BN weight/bias grads must both be fresh or both accumulate")
            acc = acc2
        return dgam, dbet, acc

    def bn_prologue(self, rec: _ConvRec, partial_floats=None, coefs: int = 3, targets=None):
        """What every BN-backward form starts from -> (M, dgamma, dbeta,
        accumulate, dy, partial, coef): the gradient targets (bn_grads, unless
        given), dy like rec.y, the reduction scratch of partial_floats(M, K)
        floats (None: the form brings its own) and `coefs` * K floats of the
        pass's coefficient buffer."""
        g = rec.geom
        M = self.N * g.P * g.Q
        dgam, dbet, acc = self.bn_grads(rec) if targets is None else targets
        dy = torch.empty_like(rec.y)
        partial = None
        if partial_floats is not None:
            partial = torch.empty(partial_floats(M, g.K), device=self.dev, dtype=torch.float32)
        return M, dgam, dbet, acc, dy, partial, self.coef_buf[: coefs * g.K]

    def bn_backward(self, rec: _ConvRec, dzin, dpre=None, mbits=None):
        """BN backward with its own reduction pass; mbits: the forward's ReLU
        mask bits (dpre then receives the masked gradient), None: no ReLU."""
        M, dgam, dbet, acc, dy, partial, coef = self.bn_prologue(rec, ops.bn_bwd_partial_floats)
        ops.bn_bwd(M, rec.geom.K, dzin, None, rec.y, rec.stats[0], rec.stats[1], rec.bn.weight.detach(), dgam, dbet,
                   acc, dy, dpre, partial, coef, mbits)
        return dy

    def bn_relu_backward(self, rec: _ConvRec, dzin):
        """BN+ReLU (no residual) backward; the mask comes from y and the BN affine."""
        M, dgam, dbet, acc, dy, partial, coef = self.bn_prologue(rec, ops.bn_bwd_partial_floats)
        ops.bn_relu_bwd(M, rec.geom.K, dzin, rec.y, rec.stats[0], rec.stats[1], rec.stats[2], rec.stats[3],
                        rec.bn.weight.detach(), dgam, dbet, acc, dy, partial, coef)
        return dy

    def bn_backward_fused(self, rec: _ConvRec, dpre, partial, tiles):
        """BN backward whose reduction came out of the dgrad epilogue that
        produced dpre (already ReLU-masked)."""
        M, dgam, dbet, acc, dy, _, coef = self.bn_prologue(rec)
        ops.bn_bwd_from_partials(M, rec.geom.K, tiles, partial, dpre, rec.y, rec.stats[0], rec.stats[1],
                                 rec.bn.weight.detach(), dgam, dbet, acc, dy, coef)
        return dy

    def bn_backward_dual(self, rec_a: _ConvRec, rec_b: _ConvRec, dzin, mbits):
        """Backward of z = relu(BN_a(y_a) + BN_b(y_b)) in one reduction and one
        apply pass (the masked gradient that feeds both is never stored);
        None when the two BNs' gradients do not both accumulate or both start fresh."""
        ta, tb = self.bn_grads(rec_a), self.bn_grads(rec_b)
        has_a, has_b = ta[0] is not None or ta[1] is not None, tb[0] is not None or tb[1] is not None
        if has_a and has_b and ta[2] != tb[2]:
            return None
        acc = ta[2] if has_a else tb[2]
        M, ga, ba, _, dya, _, coef = self.bn_prologue(rec_a, coefs=6, targets=ta)
        dyb = torch.empty_like(rec_b.y)
        partial = torch.empty(ops.bn_bwd_dual_partial_floats(M, rec_a.geom.K), device=self.dev, dtype=torch.float32)
        ops.bn_bwd_dual(M, rec_a.geom.K, dzin, None, rec_a.y, rec_a.stats[0], rec_a.stats[1],
                        rec_a.bn.weight.detach(), ga, ba, rec_b.y, rec_b.stats[0], rec_b.stats[1],
                        rec_b.bn.weight.detach(), tb[0], tb[1], acc, dya, dyb, partial, coef, mbits)
        return dya, dyb


def _ds_dgrad_fusable(g: ConvGeom, gds: ConvGeom) -> bool:
    """conv1 and the downsample of a block read the same input and produce the
    same output grid (BasicBlock): ssip_conv_dgrad_ds takes both."""
    return (gds.R == 1 and gds.S == 1 and gds.pad == 0 and gds.stride == g.stride
            and (g.N, g.H, g.W, g.C, g.K, g.P, g.Q) == (gds.N, gds.H, gds.W, gds.C, gds.K, gds.P, gds.Q))


def _prepped_t(model: SSIPResNet, rec: _ConvRec):
    return _prepped(model, rec.conv, rec.geom, need_t=True)


# ---------------------------------------------------------------------------
# factory helpers
# ---------------------------------------------------------------------------
def resnet(arch: str = "resnet18", num_classes: int = 1000, dtype: str = "fp32") -> SSIPResNet:
    return SSIPResNet(arch, num_classes=num_classes, dtype=dtype)


def replace_fc(model: SSIPResNet, num_classes: int) -> SSIPResNet:
    """`model.fc = nn.Linear(in_features, num_classes)` as create_model does
    (src/training/common.py:299-304) — consumes the torch RNG identically."""
    model.fc = nn.Linear(model.fc.in_features, num_classes)
    return model

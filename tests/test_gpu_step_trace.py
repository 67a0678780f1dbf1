"""Launch trace of the train-step host engine (ssip/resnet.py, ssip/semi_step.py).

ssip/_lib.py hands every C-ABI call, every ops.wait_stream and every
ops.host_callback to ``_lib.RECORDER``, and every tensor whose pointer is
taken to its ``keep`` list.  ``Tracer`` is such a recorder: it turns a region
into canonical text, one event per line --

  call <name> <args...>   integers and floats verbatim, a ConvDesc as its 11
                          fields, other ctypes structures / arrays as their
                          type name and byte length, None as 0, the trailing
                          stream as s<k>, every other pointer as
                          t<k>+<byte offset>
  wait s<dst> s<src>
  callback <n> [names]    the named_parameters() names of the parameters a
                          gradient-ready hook was handed

Streams and tensors are numbered by first appearance, a tensor being the
storage a pointer falls into (the tracer keeps them alive, so no address is
reused inside a region): the text does not depend on allocation addresses or
order, and changes when a launch, a wait, a callback, a scalar, a tensor's
identity or offset, or the stream of a launch moves.  Only stream-ordered
entry points (last argument a stream) are events: the planning queries made
through ``_lib.call`` depend on how warm the host-side caches are.

tests/golden/step_trace.json holds, per case, the event count, the count per
entry point and the SHA-256 of the text, recorded by
tests/golden/make_step_trace_goldens.py (``--full DIR`` writes the texts).
On a mismatch the test writes its text under tmp_path and names the file.
"""
import bisect
import contextlib
import ctypes
import hashlib
import json
import os
from collections import Counter
from pathlib import Path

import pytest
import torch

from ssip import SSIPResNet, _lib, replace_fc
from ssip import resnet as R

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "step_trace.json"


class Tracer:
    """Duck-typed ``_lib.RECORDER`` (see the module docstring)."""

    def __init__(self, model=None):
        self.keep = []
        self.events = []
        self.names = {id(p): n for n, p in model.named_parameters()} if model is not None else {}

    def on_call(self, name, args):
        argtypes = _lib._SIGS[name][1]
        if argtypes and argtypes[-1] is ctypes.c_void_p:
            self.events.append(("call", name, tuple(args)))

    def wait_stream(self, dst_stream, src_stream):
        self.events.append(("wait", int(dst_stream), int(src_stream)))

    def callback(self, fn, args):
        self.events.append(("callback", fn, args))

    def text(self) -> str:
        spans = {}
        for t in self.keep:
            st = t.untyped_storage()
            if st.nbytes():
                spans[st.data_ptr()] = max(spans.get(st.data_ptr(), 0), st.nbytes())
        bases = sorted(spans)
        tensors, streams = {}, {}

        def stream(s):
            return "s%d" % streams.setdefault(int(s or 0), len(streams))

        def pointer(p):
            i = bisect.bisect_right(bases, p) - 1
            if i < 0 or p >= bases[i] + spans[bases[i]]:
                raise AssertionError(f"pointer {p:#x} is in no kept tensor")
            return "t%d+%d" % (tensors.setdefault(bases[i], len(tensors)), p - bases[i])

        def arg(a, ctype):
            if isinstance(a, _lib.ConvDesc):
                return "desc(" + ",".join(str(getattr(a, f)) for f, _ in a._fields_) + ")"
            if isinstance(a, (ctypes.Structure, ctypes.Array)):
                return "%s[%d]" % (type(a).__name__, ctypes.sizeof(a))
            if a is None:
                return "0"
            if ctype is ctypes.c_void_p:
                return pointer(int(a))
            if ctype is ctypes.c_float or isinstance(a, float):
                return repr(float(a))
            return str(int(a))

        lines, ncb = [], 0
        for ev in self.events:
            if ev[0] == "call":
                _, name, args = ev
                argtypes = _lib._SIGS[name][1]
                toks = [arg(a, t) for a, t in zip(args[:-1], argtypes[:-1])]
                lines.append(" ".join(["call", name] + toks + [stream(args[-1])]))
            elif ev[0] == "wait":
                lines.append("wait %s %s" % (stream(ev[1]), stream(ev[2])))
            else:
                names = [self.names[id(p)] for a in ev[2] if isinstance(a, (list, tuple))
                         for p in a if id(p) in self.names]
                lines.append(" ".join(["callback", str(ncb)] + names))
                ncb += 1
        return "\n".join(lines) + "\n"


def summary(text: str) -> dict:
    lines = text.splitlines()
    calls = Counter(ln.split(" ")[1] if ln.startswith("call ") else ln.split(" ")[0] for ln in lines)
    return {"events": len(lines), "counts": dict(sorted(calls.items())),
            "sha256": hashlib.sha256(text.encode()).hexdigest()}


@contextlib.contextmanager
def tracing(model):
    assert _lib.RECORDER is None
    tr = _lib.RECORDER = Tracer(model)
    try:
        yield tr
    finally:
        _lib.RECORDER = None


@contextlib.contextmanager
def patched(obj=R, env=None, **attrs):
    """Module attributes (and environment variables; None = unset) for one case."""
    old = {k: getattr(obj, k) for k in attrs}
    old_env = {k: os.environ.get(k) for k in (env or {})}
    for k, v in attrs.items():
        setattr(obj, k, v)
    for k, v in (env or {}).items():
        os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            setattr(obj, k, v)
        for k, v in old_env.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def _model(dev, arch="resnet18", dtype="fp32"):
    torch.manual_seed(0)
    return replace_fc(SSIPResNet(arch, 1000, dtype=dtype), 2).to(dev).train()


def _batch(dev, N, S, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, 3, S, S, generator=g).to(dev), torch.randint(0, 2, (N,), generator=g).to(dev)


def _fwd_bwd(m, x, y):
    torch.nn.functional.cross_entropy(m(x).float(), y).backward()


def semi_step(dev, S=64, B=8, **attrs):
    """The second eager SemiStep (caches warm), resnet18 bf16, B + B images of
    S x S.  Only at S = 224 does the stem take ssip_stem_bwd_wgrad, the one
    wgrad a SemiStep leaves unjoined on the side stream (SSIP_DEFER_STEM)."""
    from ssip.semi_step import SemiStep

    env = attrs.pop("env", {"SSIP_DEFER_STEM": None})
    with patched(env=env, **attrs):
        m = _model(dev, dtype="bf16")
        step = SemiStep(m, lr=1e-3, weight_decay=1e-4, tau=0.5, image_size=S, seed=11)
        g = torch.Generator().manual_seed(4)
        x_l = torch.randint(0, 256, (B, S, S, 3), generator=g, dtype=torch.uint8).to(dev)
        x_u = torch.randint(0, 256, (B, S, S, 3), generator=g, dtype=torch.uint8).to(dev)
        y_l = torch.randint(0, 2, (B,), generator=g).to(dev)
        step(x_l, y_l, x_u)
        with tracing(m) as tr:
            step(x_l, y_l, x_u)
        torch.cuda.synchronize()
        return tr.text()


def plain(dev, arch="resnet18", dtype="fp32", N=4, S=64, **attrs):
    """Case 3 / 4: model(x) + cross_entropy(...).backward()."""
    with patched(**attrs):
        m = _model(dev, arch, dtype)
        x, y = _batch(dev, N, S)
        with tracing(m) as tr:
            _fwd_bwd(m, x, y)
        torch.cuda.synchronize()
        return tr.text()


def partial(dev, trainable=None, twice=False):
    """Case 5: resnet18 fp32, N = 3, 64x64; trainable: name prefixes that keep
    requires_grad; twice: a flattened arena and a second backward without zero_grad."""
    m = _model(dev)
    if trainable is not None:
        for n, p in m.named_parameters():
            p.requires_grad = n.startswith(trainable)
    if twice:
        m.flatten_parameters()
    x, y = _batch(dev, 3, 64)
    with tracing(m) as tr:
        _fwd_bwd(m, x, y)
        if twice:
            _fwd_bwd(m, x, y)
    torch.cuda.synchronize()
    return tr.text()


def hooked(dev, side):
    """Case 6: model.grad_ready_hook appends what it is handed to a list."""
    with patched(WGRAD_SIDE_STREAM=side):
        m = _model(dev)
        got = []
        m.grad_ready_hook = got.append
        x, y = _batch(dev, 4, 64)
        with tracing(m) as tr:
            _fwd_bwd(m, x, y)
        torch.cuda.synchronize()
        assert sum(len(ps) for ps in got) == len(list(m.parameters()))
        return tr.text()


def nograd(dev, train=False, embedding=False, **attrs):
    """Case 7: no-grad forwards, resnet18 bf16, N = 5, 96x96."""
    with patched(**attrs):
        m = _model(dev, dtype="bf16")
        m.train(train)
        m.embedding_only = embedding
        if train:
            m.bn_update_running = False  # the weak forward
        x, _ = _batch(dev, 5, 96)
        with tracing(m) as tr, torch.no_grad():
            m(x)
        torch.cuda.synchronize()
        return tr.text()


CASES = {
    "semi_step": lambda dev: semi_step(dev),
    "semi_step_no_defer": lambda dev: semi_step(dev, env={"SSIP_DEFER_STEM": "0"}),
    "semi_step_serial_budget": lambda dev: semi_step(dev, WGRAD_SIDE_STREAM=False, WGRAD_BUDGET_SERIAL=True),
    # (the fp32 4 x 64x64 cases below have no halo-kernel geometry: these knobs only act here)
    "semi_step_fuse_0": lambda dev: semi_step(dev, _FUSE_BN_BWD="0"),
    "semi_step_no_bnrelu_in": lambda dev: semi_step(dev, _BNRELU_IN=False),
    "semi_step_bnrelu_z": lambda dev: semi_step(dev, _BNRELU_Z=True),
    "semi_step_224": lambda dev: semi_step(dev, S=224, B=4),
    "semi_step_224_no_defer": lambda dev: semi_step(dev, S=224, B=4, env={"SSIP_DEFER_STEM": "0"}),
    "semi_step_224_serial_budget": lambda dev: semi_step(dev, S=224, B=4, WGRAD_SIDE_STREAM=False,
                                                         WGRAD_BUDGET_SERIAL=True),
    "plain_fuse_default": lambda dev: plain(dev, _FUSE_BN_BWD=""),
    "plain_fuse_0": lambda dev: plain(dev, _FUSE_BN_BWD="0"),
    "plain_fuse_1": lambda dev: plain(dev, _FUSE_BN_BWD="1"),
    "plain_no_bnrelu_in": lambda dev: plain(dev, _BNRELU_IN=False),
    "plain_bnrelu_z": lambda dev: plain(dev, _BNRELU_Z=True),
    "plain_no_fwd_ds": lambda dev: plain(dev, _NO_FWD_DS=True),
    "plain_bf16": lambda dev: plain(dev, dtype="bf16"),
    "resnet50_bf16": lambda dev: plain(dev, arch="resnet50", dtype="bf16", N=8, S=128),
    "partial_fc_only": lambda dev: partial(dev, trainable=("fc",)),
    "partial_from_layer3": lambda dev: partial(dev, trainable=("layer3", "layer4", "fc")),
    "accumulate_arena": lambda dev: partial(dev, twice=True),
    "hook_side": lambda dev: hooked(dev, True),
    "hook_serial": lambda dev: hooked(dev, False),
    "eval_folded": lambda dev: nograd(dev),
    "eval_unfolded": lambda dev: nograd(dev, _FOLD_EVAL_BN=False),
    "eval_embedding": lambda dev: nograd(dev, embedding=True),
    "weak_forward": lambda dev: nograd(dev, train=True),
}


@pytest.mark.parametrize("case", list(CASES))
def test_step_trace(dev, case, tmp_path):
    want = json.loads(GOLDEN.read_text())[case]
    text = CASES[case](dev)
    got = summary(text)
    if got != want:
        out = tmp_path / f"{case}.txt"
        out.write_text(text)
        moved = {k: (want["counts"].get(k, 0), got["counts"].get(k, 0))
                 for k in set(want["counts"]) | set(got["counts"]) if want["counts"].get(k, 0) != got["counts"].get(k, 0)}
        pytest.fail(f"{case}: the launch trace changed ({want['events']} -> {got['events']} events; entry points "
                    f"(recorded, now): {moved}); its text is in {out}: diff it against "
                    f"`make_step_trace_goldens.py --full DIR` run on the parent commit")

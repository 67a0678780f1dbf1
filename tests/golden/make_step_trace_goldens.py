"""Writes tests/golden/step_trace.json: per case of tests/test_gpu_step_trace.py
the number of events of the launch trace, the count per entry point and the
SHA-256 of its canonical text (the tracer and the cases live in the test
module).  Needs the device.  Regenerate only when the launch sequence is meant
to change; a restructuring of the host engine must reproduce the file as it is.

usage: python tests/golden/make_step_trace_goldens.py [--full DIR]
  --full DIR   also write each case's text to DIR/<case>.txt, to diff a
               changed trace against
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
for p in (ROOT / "tests", ROOT / "semi-supervised-image-processing_amd", ROOT):
    sys.path.insert(0, str(p))


def main():
    import torch

    import test_gpu_step_trace as T

    ap = argparse.ArgumentParser()
    ap.add_argument("--full", metavar="DIR")
    ap.add_argument("--out", default=str(Path(__file__).resolve().parent / "step_trace.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the launch trace is recorded on the device"
    dev = torch.device("cuda")
    full = Path(args.full) if args.full else None
    if full is not None:
        full.mkdir(parents=True, exist_ok=True)
    t0 = time.perf_counter()
    rows = []
    for case, run in T.CASES.items():
        text = run(dev)
        if full is not None:
            (full / f"{case}.txt").write_text(text)
        rows.append("%s:%s" % (json.dumps(case), json.dumps(T.summary(text), separators=(",", ":"))))
    Path(args.out).write_text("{\n" + ",\n".join(rows) + "\n}\n")
    print(len(rows), "cases,", "%.1f s" % (time.perf_counter() - t0))


if __name__ == "__main__":
    main()

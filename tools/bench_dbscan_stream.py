"""Time DBSCAN's two device paths on the default grid of src.clustering
(4 eps x 3 min_samples): the bitmap path (ssip_pairwise_eps, the bitmap's
download and the host labeller) and the stream path (ssip_pairwise_degree,
then ssip_dbscan_walk + ssip_dbscan_hook rounds; no stored graph), and one
ssip_dbscan_walk (M = 3) next to one ssip_pairwise_eps by HIP events.

Points: those of tools/bench_analytics.py (make_points), d = 50, N = 20000,
65536 and 200000.  The bitmap path and ssip_pairwise_eps stop at N = 65536.
Per (size, path): one child process under its own time limit, one warm-up run
discarded, then the median of 5; the host side uses at most 16 threads.

usage: python tools/bench_dbscan_stream.py [--sizes 20000 65536 200000] [--reps 5] [--warmup 1] [--threads 16]
                                           [--step-timeout 600] [--out profiles/dbscan_stream_bench.json]
Prints one JSON line per (size, path) and writes the summary file (sizes
already in the file and not measured again are kept).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "semi-supervised-image-processing_amd"
for _p in (str(ROOT), str(PKG), str(ROOT / "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from bench_analytics import D, EPS, MIN_SAMPLES, make_points  # noqa: E402

PATHS = ("bitmap", "stream", "kernels")
WALK_EPS = 1.0  # the eps of the kernel-level comparison


def _timed(run, reps, warmup, sync):
    times = []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        run()
        sync()
        if i >= warmup:
            times.append(time.perf_counter() - t0)
    return times


def _event_ms(torch, launch, reps, warmup):
    out = []
    for i in range(warmup + reps):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        launch()
        stop.record()
        stop.synchronize()
        if i >= warmup:
            out.append(start.elapsed_time(stop))
    return out


def worker(path, n, reps, warmup):
    import numpy as np
    import torch

    from ssip import analytics as A

    x = make_points(n)[0]
    be = A.DeviceBackend(x)
    rec = {"path": path, "N": n, "d": D, "reps": reps, "warmup": warmup}
    if path == "bitmap":
        def run():
            for eps in EPS:
                degree, bitmap = be.eps_graph(eps)
                for ms in MIN_SAMPLES:
                    A.dbscan_labels_from_graph(degree, bitmap, ms)
        rec["times_s"] = _timed(run, reps, warmup, torch.cuda.synchronize)
    elif path == "stream":
        walks = {}

        def run():
            for eps in EPS:
                walks[str(eps)] = A.dbscan_stream(be, eps, MIN_SAMPLES)[1]
        rec["times_s"] = _timed(run, reps, warmup, torch.cuda.synchronize)
        rec["walks"] = walks
    else:
        be.degree(WALK_EPS)
        be.dbscan_begin(MIN_SAMPLES)
        rec["eps"] = WALK_EPS
        rec["walk_ms"] = _event_ms(torch, be.dbscan_walk, reps, warmup)
        rec["degree_ms"] = _event_ms(torch, lambda: be._call("ssip_pairwise_degree", n, D, be._p(be.X), WALK_EPS,
                                                             be._p(be._db_degree)), reps, warmup)
        rec["hook_ms"] = _event_ms(torch, be.dbscan_hook, reps, warmup)
        if n <= A.EPS_MAX_N:
            degree = torch.empty(n, dtype=torch.int32, device=be.dev)
            bitmap = torch.empty((n, (n + 31) // 32), dtype=torch.int32, device=be.dev)
            rec["eps_ms"] = _event_ms(torch, lambda: be._call("ssip_pairwise_eps", n, D, be._p(be.X), WALK_EPS,
                                                              be._p(degree), be._p(bitmap)), reps, warmup)
        core = be._db_degree_host[None, :] >= np.asarray(MIN_SAMPLES)[:, None]
        rec["core_fraction"] = [float(c.mean()) for c in core]
    for key in ("times_s", "walk_ms", "degree_ms", "hook_ms", "eps_ms"):
        if key in rec:
            rec["median_s" if key == "times_s" else key + "_median"] = statistics.median(rec[key])
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="*", default=[20000, 65536, 200000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--step-timeout", type=float, default=600.0, help="seconds per (size, path) child process")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "dbscan_stream_bench.json")
    ap.add_argument("--worker", choices=PATHS, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--n", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        worker(a.worker, a.n, a.reps, a.warmup)
        return 0

    from ssip.analytics import EPS_MAX_N

    env = dict(os.environ)
    for var in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
        env[var] = str(min(a.threads, 16))
    rows = []
    for n in a.sizes:
        row = {"N": n, "d": D}
        for path in PATHS:
            if path == "bitmap" and n > EPS_MAX_N:
                continue
            cmd = [sys.executable, str(Path(__file__).resolve()), "--worker", path, "--n", str(n), "--reps",
                   str(a.reps), "--warmup", str(a.warmup)]
            proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            t0 = time.monotonic()
            while True:
                try:
                    out, err = proc.communicate(timeout=60)
                    break
                except subprocess.TimeoutExpired:
                    if time.monotonic() - t0 > a.step_timeout:
                        proc.kill()
                        proc.communicate()
                        print(f"bench_dbscan_stream: {path} N={n} exceeded {a.step_timeout:.0f} s", file=sys.stderr)
                        return 1
                    print(f"bench_dbscan_stream: {path} N={n} running, {time.monotonic() - t0:.0f} s",
                          file=sys.stderr, flush=True)
            if proc.returncode != 0:
                sys.stderr.write(err[-2000:])
                print(f"bench_dbscan_stream: {path} N={n} failed ({proc.returncode})", file=sys.stderr)
                return 1
            rec = json.loads(out.strip().splitlines()[-1])
            print(json.dumps(rec), flush=True)
            row[path] = {k: v for k, v in rec.items() if k not in ("path", "N", "d")}
        if "bitmap" in row:
            row["bitmap_over_stream"] = row["bitmap"]["median_s"] / row["stream"]["median_s"]
        if "eps_ms_median" in row["kernels"]:
            row["walk_over_eps_kernel"] = row["kernels"]["walk_ms_median"] / row["kernels"]["eps_ms_median"]
        rows.append(row)
        # written after every size, so a later size that runs out of time loses nothing
        summary = {"grid": {"dbscan_eps": EPS, "dbscan_min_samples": MIN_SAMPLES}, "threads": min(a.threads, 16),
                   "results": rows}
        if a.out.exists():  # sizes measured by an earlier run stay
            old = json.loads(a.out.read_text()).get("results", [])
            done = {r["N"] for r in rows}
            summary["results"] = sorted([r for r in old if r["N"] not in done] + rows, key=lambda r: r["N"])
        a.out.parent.mkdir(parents=True, exist_ok=True)
        a.out.write_text(json.dumps(summary, indent=1) + "\n")
    print(json.dumps({"wrote": str(a.out.relative_to(ROOT)) if a.out.is_relative_to(ROOT) else str(a.out)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())

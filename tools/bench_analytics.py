"""Time the default clustering sweep of src.clustering on the HIP kernels
(--device cuda) against the same sweep through sklearn on the host.

The sweep is what `python -m src.clustering` runs on the PCA cluster space with
its default grids: K-Means for k = 2..10 with n_init = 10, DBSCAN for 4 eps x 3
min_samples, one silhouette score per configuration (21) and one k-distance
curve.  PCA, t-SNE and the plots are host work on both sides and are left out.

Sizes: N = 1506 (the reference cohort) and N = 20000, d = 50.  Per size and
side: one warm-up sweep is discarded, then the median of 5.  Each (size, side)
runs in a child process of its own under its own time limit.

usage: python tools/bench_analytics.py [--sizes 1506 20000] [--reps 5] [--warmup 1] [--threads 16]
                                       [--sklearn-reps R] [--sklearn-warmup W] [--step-timeout 900]
                                       [--out profiles/analytics_bench.json]
Prints one JSON line per (size, side) and writes the summary file (the number of
timed sweeps and warm-ups of each side is recorded; sizes already in the file
and not measured again are kept).
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
D = 50
K_RANGE = list(range(2, 11))
N_INIT = 10
EPS = [0.5, 0.75, 1.0, 1.25]
MIN_SAMPLES = [5, 10, 15]
SEED = 42


def make_points(n):
    """8 blobs whose within-blob distances straddle the default eps grid
    (about 1.0 +- 0.07), so the DBSCAN configurations range from all-noise to
    one cluster per blob."""
    import numpy as np

    rng = np.random.default_rng(n)
    blob = rng.integers(0, 8, size=n)
    x = (rng.normal(size=(8, D)) * 3.0)[blob] + 0.1 * rng.normal(size=(n, D))
    is_labeled = rng.random(n) < 0.1
    names = np.array([f"class{b}" for b in range(8)])
    return x.astype(np.float32), is_labeled, np.where(is_labeled, names[blob], "")


def sweep_device(x, is_labeled, labels):
    import numpy as np

    from src import clustering as C
    from ssip import analytics

    bundle = C.FeatureBundle(x, np.arange(len(x)).astype(str), is_labeled, labels, None, None)
    space = C.EmbeddingResult("pca_cluster", x, {})
    backend = analytics.make_backend(x, "cuda")
    res = C.evaluate_kmeans(space, bundle, K_RANGE, N_INIT, SEED, "cuda", backend)
    res += C.evaluate_dbscan(space, bundle, EPS, MIN_SAMPLES, SEED, "all", "cuda", backend)
    C.sorted_kdistance(x, MIN_SAMPLES[0], "cuda", backend)
    return res


def sweep_sklearn(x, is_labeled, labels, threads):
    import numpy as np
    from sklearn.cluster import DBSCAN, KMeans
    from sklearn.metrics import adjusted_rand_score, normalized_mutual_info_score, silhouette_score
    from sklearn.neighbors import NearestNeighbors

    def score(pred):
        adjusted_rand_score(labels[is_labeled], pred[is_labeled])
        normalized_mutual_info_score(labels[is_labeled], pred[is_labeled])
        if 2 <= np.unique(pred).size < len(pred):
            silhouette_score(x, pred, n_jobs=threads)

    for k in K_RANGE:
        score(KMeans(n_clusters=k, n_init=N_INIT, random_state=SEED).fit_predict(x))
    for eps in EPS:
        for ms in MIN_SAMPLES:
            score(DBSCAN(eps=eps, min_samples=ms, n_jobs=threads).fit_predict(x))
    np.sort(NearestNeighbors(n_neighbors=MIN_SAMPLES[0], n_jobs=threads).fit(x).kneighbors(x)[0][:, -1])


def worker(side, n, reps, warmup, threads):
    for p in (str(ROOT), str(PKG)):
        if p not in sys.path:
            sys.path.insert(0, p)
    x, is_labeled, labels = make_points(n)
    if side == "cuda":
        import torch

        def run():
            sweep_device(x, is_labeled, labels)
            torch.cuda.synchronize()
    else:
        def run():
            sweep_sklearn(x, is_labeled, labels, threads)
    times = []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        run()
        if i >= warmup:
            times.append(time.perf_counter() - t0)
    print(json.dumps({"side": side, "N": n, "d": D, "times_s": times, "median_s": statistics.median(times),
                      "warmup": warmup, "reps": reps}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="*", default=[1506, 20000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--sklearn-reps", type=int, default=None, help="override --reps for the sklearn side")
    ap.add_argument("--sklearn-warmup", type=int, default=None, help="override --warmup for the sklearn side")
    ap.add_argument("--step-timeout", type=float, default=900.0, help="seconds per (size, side) child process")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "analytics_bench.json")
    ap.add_argument("--worker", choices=["cuda", "sklearn"], default=None, help=argparse.SUPPRESS)
    ap.add_argument("--n", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        worker(a.worker, a.n, a.reps, a.warmup, a.threads)
        return 0

    env = dict(os.environ)
    for var in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
        env[var] = str(a.threads)
    rows = []
    for n in a.sizes:
        row = {"N": n, "d": D}
        for side in ("cuda", "sklearn"):
            reps, warmup = (a.reps, a.warmup) if side == "cuda" else (a.sklearn_reps or a.reps,
                                                                      a.warmup if a.sklearn_warmup is None
                                                                      else a.sklearn_warmup)
            cmd = [sys.executable, str(Path(__file__).resolve()), "--worker", side, "--n", str(n), "--reps",
                   str(reps), "--warmup", str(warmup), "--threads", str(a.threads)]
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
                        print(f"bench_analytics: {side} N={n} exceeded {a.step_timeout:.0f} s", file=sys.stderr)
                        return 1
                    print(f"bench_analytics: {side} N={n} running, {time.monotonic() - t0:.0f} s", file=sys.stderr,
                          flush=True)
            if proc.returncode != 0:
                sys.stderr.write(err[-2000:])
                print(f"bench_analytics: {side} N={n} failed ({proc.returncode})", file=sys.stderr)
                return 1
            rec = json.loads(out.strip().splitlines()[-1])
            print(json.dumps(rec), flush=True)
            row[f"{side}_median_s"] = rec["median_s"]
            row[f"{side}_times_s"] = rec["times_s"]
            row[f"{side}_warmup"] = rec["warmup"]
        row["sklearn_over_cuda"] = row["sklearn_median_s"] / row["cuda_median_s"]
        rows.append(row)
    summary = {"sweep": {"kmeans_range": K_RANGE, "kmeans_n_init": N_INIT, "dbscan_eps": EPS,
                         "dbscan_min_samples": MIN_SAMPLES, "silhouettes": len(K_RANGE) + len(EPS) * len(MIN_SAMPLES),
                         "kdistance_curves": 1},
               "threads": a.threads, "results": rows}
    if a.out.exists():  # sizes measured by an earlier run stay
        old = json.loads(a.out.read_text()).get("results", [])
        summary["results"] = sorted([r for r in old if r["N"] not in a.sizes] + rows, key=lambda r: r["N"])
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text(json.dumps(summary, indent=1) + "\n")
    print(json.dumps({"wrote": str(a.out.relative_to(ROOT)) if a.out.is_relative_to(ROOT) else str(a.out)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())

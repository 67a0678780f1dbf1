"""Time one exact t-SNE fit on the HIP kernels (ssip.analytics.tsne_fit,
device="cuda") against sklearn's Barnes-Hut TSNE on the host, the call
`python -m src.clustering` makes by default, and score both embeddings by the
exact KL divergence.

Points: the cohort of tools/bench_analytics.py (8 blobs, d = 50) at N = 1506 and
N = 20000, perplexity 30, 1000 iterations, seed 42.  Per size and side: one
warm-up fit is discarded, then the median of 5.  Each (size, side) runs in a
child process of its own under its own time limit, and a third child evaluates
the KL divergence of both final embeddings against the same fp64 joint P
(bisection, symmetrisation and the sum over all pairs in float64 torch, on the
device when there is one).

usage: python tools/bench_tsne.py [--sizes 1506 20000] [--reps 5] [--warmup 1] [--threads 16]
                                  [--sklearn-reps R] [--sklearn-warmup W] [--step-timeout 900]
                                  [--out profiles/tsne_bench.json]
Prints one JSON line per (size, side) and writes the summary file (the number of
timed fits and warm-ups of each side is recorded; sizes already in the file and
not measured again are kept).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "semi-supervised-image-processing_amd"
PERPLEXITY = 30.0
MAX_ITER = 1000
SEED = 42


def _paths():
    for p in (str(ROOT), str(PKG), str(ROOT / "tools")):
        if p not in sys.path:
            sys.path.insert(0, p)


def make_points(n):
    _paths()
    from bench_analytics import make_points as cohort

    return cohort(n)[0]


def exact_kl(x, perplexity, embeddings, device, step=None):
    """KL(P || Q) of each embedding, everything in float64: sklearn's bisection
    for P (vectorised over rows), P = (P + P^T) / sum, Q from the Student-t
    kernel, both clamped at 2.2e-16 as sklearn's _kl_divergence does."""
    import numpy as np
    import torch

    def sqdist(a, b):
        """direct difference, one feature at a time: [len(a)][len(b)]"""
        out = torch.zeros((a.shape[0], b.shape[0]), dtype=torch.float64, device=a.device)
        for c in range(a.shape[1]):
            out += (a[:, c, None] - b[None, :, c]) ** 2
        return out

    eps = float(np.finfo(np.double).eps)
    X = torch.from_numpy(np.asarray(x, dtype=np.float64)).to(device)
    n = X.shape[0]
    P = torch.empty((n, n), dtype=torch.float64, device=device)
    target = float(np.log(perplexity))
    tiny, tol = float(np.float32(1e-8)), float(np.float32(1e-5))
    step = step or max(1, (1 << 25) // n)  # rows per chunk
    for s in range(0, n, step):
        e_ = min(n, s + step)
        d2 = sqdist(X[s:e_], X)
        off = torch.ones_like(d2)
        off[torch.arange(e_ - s, device=device), torch.arange(s, e_, device=device)] = 0.0
        r = e_ - s
        beta = torch.ones(r, dtype=torch.float64, device=device)
        lo = torch.full_like(beta, -float("inf"))
        hi = torch.full_like(beta, float("inf"))
        used, sums = beta.clone(), beta.clone()
        active = torch.ones(r, dtype=torch.bool, device=device)
        for _ in range(100):
            if not bool(active.any()):
                break
            ex = torch.exp(-d2 * beta[:, None]) * off
            s0 = ex.sum(dim=1)
            s0 = torch.where(s0 == 0.0, torch.full_like(s0, tiny), s0)
            diff = torch.log(s0) + beta * ((d2 * ex).sum(dim=1) / s0) - target
            used = torch.where(active, beta, used)
            sums = torch.where(active, s0, sums)
            done = diff.abs() <= tol
            up = active & ~done & (diff > 0)
            dn = active & ~done & ~(diff > 0)
            lo = torch.where(up, beta, lo)
            hi = torch.where(dn, beta, hi)
            nb_up = torch.where(torch.isinf(hi), beta * 2.0, (beta + hi) / 2.0)
            nb_dn = torch.where(torch.isinf(lo), beta / 2.0, (beta + lo) / 2.0)
            beta = torch.where(up, nb_up, torch.where(dn, nb_dn, beta))
            active = active & ~done
        P[s:e_] = torch.exp(-d2 * used[:, None]) * off / sums[:, None]
    total = 2.0 * float(P.sum())
    out = []
    for emb in embeddings:
        Y = torch.from_numpy(np.asarray(emb, dtype=np.float64)).to(device)
        Z = 0.0
        for s in range(0, n, step):
            w = 1.0 / (1.0 + sqdist(Y[s:s + step], Y))
            Z += float(w.sum()) - float(w.shape[0])  # the diagonal contributes exactly 1 per row
        kl = 0.0
        for s in range(0, n, step):
            e_ = min(n, s + step)
            w = 1.0 / (1.0 + sqdist(Y[s:e_], Y))
            p = torch.clamp((P[s:e_] + P[:, s:e_].T) / total, min=eps)
            q = torch.clamp(w / Z, min=eps)
            term = p * torch.log(p / q)
            term[torch.arange(e_ - s, device=device), torch.arange(s, e_, device=device)] = 0.0
            kl += float(term.sum())
        out.append(kl)
    return out


def worker(side, n, reps, warmup, threads, emb_out):
    _paths()
    import numpy as np

    x = make_points(n)
    if side == "cuda":
        import torch

        from ssip import analytics

        def run():
            emb, kl, n_iter = analytics.tsne_fit(x, PERPLEXITY, seed=SEED, max_iter=MAX_ITER, device="cuda")
            torch.cuda.synchronize()
            return emb, kl, n_iter
    else:
        from sklearn.manifold import TSNE

        def run():
            ts = TSNE(n_components=2, perplexity=PERPLEXITY, init="pca", random_state=SEED, learning_rate="auto",
                      max_iter=MAX_ITER, metric="euclidean", n_jobs=threads)
            emb = ts.fit_transform(x)
            return emb, float(ts.kl_divergence_), int(ts.n_iter_) + 1
    times = []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        emb, kl, n_iter = run()
        if i >= warmup:
            times.append(time.perf_counter() - t0)
    np.save(emb_out, np.asarray(emb))
    print(json.dumps({"side": side, "N": n, "d": int(x.shape[1]), "times_s": times,
                      "median_s": statistics.median(times), "warmup": warmup, "reps": reps, "reported_kl": kl,
                      "n_iter": n_iter}))


def kl_worker(n, paths):
    _paths()
    import numpy as np
    import torch

    device = "cuda" if torch.cuda.is_available() else "cpu"
    kls = exact_kl(make_points(n), PERPLEXITY, [np.load(p) for p in paths], device)
    print(json.dumps({"side": "kl", "N": n, "exact_kl": kls, "evaluated_on": device}))


def run_child(cmd, env, label, step_timeout):
    proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    t0 = time.monotonic()
    while True:
        try:
            out, err = proc.communicate(timeout=60)
            break
        except subprocess.TimeoutExpired:
            if time.monotonic() - t0 > step_timeout:
                proc.kill()
                proc.communicate()
                print(f"bench_tsne: {label} exceeded {step_timeout:.0f} s", file=sys.stderr)
                return None
            print(f"bench_tsne: {label} running, {time.monotonic() - t0:.0f} s", file=sys.stderr, flush=True)
    if proc.returncode != 0:
        sys.stderr.write(err[-2000:])
        print(f"bench_tsne: {label} failed ({proc.returncode})", file=sys.stderr)
        return None
    rec = json.loads(out.strip().splitlines()[-1])
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="*", default=[1506, 20000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--sklearn-reps", type=int, default=None, help="override --reps for the sklearn side")
    ap.add_argument("--sklearn-warmup", type=int, default=None, help="override --warmup for the sklearn side")
    ap.add_argument("--step-timeout", type=float, default=900.0, help="seconds per child process")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "tsne_bench.json")
    ap.add_argument("--worker", choices=["cuda", "sklearn", "kl"], default=None, help=argparse.SUPPRESS)
    ap.add_argument("--n", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--emb", type=Path, nargs="*", default=[], help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker == "kl":
        kl_worker(a.n, a.emb)
        return 0
    if a.worker:
        worker(a.worker, a.n, a.reps, a.warmup, a.threads, a.emb[0])
        return 0

    env = dict(os.environ)
    for var in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
        env[var] = str(a.threads)
    me = [sys.executable, str(Path(__file__).resolve())]
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for n in a.sizes:
            row = {"N": n}
            embs = []
            for side in ("cuda", "sklearn"):
                reps, warmup = (a.reps, a.warmup) if side == "cuda" else (
                    a.sklearn_reps or a.reps, a.warmup if a.sklearn_warmup is None else a.sklearn_warmup)
                emb = Path(tmp) / f"{side}_{n}.npy"
                rec = run_child(me + ["--worker", side, "--n", str(n), "--reps", str(reps), "--warmup", str(warmup),
                                      "--threads", str(a.threads), "--emb", str(emb)], env, f"{side} N={n}",
                                a.step_timeout)
                if rec is None:
                    return 1
                embs.append(emb)
                row["d"] = rec["d"]
                for k in ("median_s", "times_s", "warmup", "reported_kl", "n_iter"):
                    row[f"{side}_{k}"] = rec[k]
            rec = run_child(me + ["--worker", "kl", "--n", str(n), "--emb", *map(str, embs)], env, f"kl N={n}",
                            a.step_timeout)
            if rec is None:
                return 1
            row["cuda_exact_kl"], row["sklearn_exact_kl"] = rec["exact_kl"]
            row["kl_evaluated_on"] = rec["evaluated_on"]
            row["sklearn_over_cuda"] = row["sklearn_median_s"] / row["cuda_median_s"]
            rows.append(row)
    summary = {"fit": {"perplexity": PERPLEXITY, "max_iter": MAX_ITER, "seed": SEED,
                       "cuda": "ssip.analytics.tsne_fit (exact)", "sklearn": "TSNE(method='barnes_hut', init='pca')"},
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

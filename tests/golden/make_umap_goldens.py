"""Regenerate tests/golden/umap_sequential_oracle.npz.

A plain, slow, sequential restatement of umap-learn's deterministic layout
loop, written from the published algorithm (McInnes, Healy, Melville 2018 and
the documented behaviour of ``umap.UMAP(n_components=2, metric="euclidean")``):
exact kNN in fp64, ``smooth_knn_dist``, the fuzzy union, ``find_ab_params``,
then ``optimize_layout_euclidean`` as umap-learn runs it with a fixed seed:
edges visited one after another, every update applied in place at once
(Gauss-Seidel), ``move_other`` on, negative samples from one RNG stream, the
learning rate lowered after each epoch.  Nothing of ssip.analytics is used.

It stands in for the umap package, which the test machines do not have: the
GPU and CPU tests hold the native UMAP's trustworthiness against what this
sequential order reaches on the same inputs.  Pure Python; a few minutes.

    python tests/golden/make_umap_goldens.py
"""
import math
import sys
from pathlib import Path

import numpy as np
from scipy.optimize import curve_fit
from sklearn.manifold import trustworthiness

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

N, D, EPOCHS, MIN_DIST, SEEDS, TRUST_K = 300, 50, 500, 0.1, (0, 1, 2), 15


def six_blobs(n, d):
    """Six Gaussian blobs, centres x 1.5, default_rng(1)."""
    rng = np.random.default_rng(1)
    cent = rng.standard_normal((6, d)) * 1.5
    return (cent[rng.integers(0, 6, n)] + rng.standard_normal((n, d))).astype(np.float32)


def knn(x, k):
    x = np.asarray(x, dtype=np.float64)
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    idx = np.argsort(d2, axis=1, kind="stable")[:, :k]
    return np.sqrt(np.take_along_axis(d2, idx, axis=1)), idx


def smooth_knn_dist(dist):
    n, k = dist.shape
    target = math.log2(k)
    rho, sigma = np.zeros(n), np.zeros(n)
    mean_all = dist.mean()
    for i in range(n):
        nz = dist[i][dist[i] > 0.0]
        if nz.size:
            rho[i] = nz[0]
        lo, hi, mid = 0.0, math.inf, 1.0
        for _ in range(64):
            psum = 0.0
            for j in range(1, k):
                dd = dist[i, j] - rho[i]
                psum += math.exp(-dd / mid) if dd > 0.0 else 1.0
            if abs(psum - target) < 1e-5:
                break
            if psum > target:
                hi = mid
                mid = (lo + hi) / 2.0
            else:
                lo = mid
                mid = mid * 2.0 if hi == math.inf else (lo + hi) / 2.0
        sigma[i] = max(mid, 1e-3 * (dist[i].mean() if rho[i] > 0.0 else mean_all))
    return rho, sigma


def fuzzy_graph(dist, idx):
    n, k = dist.shape
    rho, sigma = smooth_knn_dist(dist)
    A = np.zeros((n, n))
    for i in range(n):
        for j in range(k):
            if idx[i, j] == i:
                continue
            dd = dist[i, j] - rho[i]
            A[i, idx[i, j]] = 1.0 if dd <= 0.0 or sigma[i] == 0.0 else math.exp(-dd / sigma[i])
    return A + A.T - A * A.T


def find_ab(min_dist, spread=1.0):
    xv = np.linspace(0, spread * 3, 300)
    yv = np.where(xv < min_dist, 1.0, np.exp(-(xv - min_dist) / spread))
    (a, b), _ = curve_fit(lambda x, a, b: 1.0 / (1.0 + a * x ** (2 * b)), xv, yv)
    return float(a), float(b)


def pca_2d(x):
    xc = np.asarray(x, dtype=np.float64)
    xc = xc - xc.mean(axis=0)
    u, s, _ = np.linalg.svd(xc, full_matrices=False)
    return u[:, :2] * s[:2]


def init_layout(x, seed):
    y = pca_2d(x) + np.random.RandomState(seed).normal(scale=1e-4, size=(x.shape[0], 2))
    return 10.0 * (y - y.min(axis=0)) / (y.max(axis=0) - y.min(axis=0))


def clip(v):
    return 4.0 if v > 4.0 else (-4.0 if v < -4.0 else v)


def sequential_layout(W, y0, a, b, seed, n_epochs, gamma=1.0, rate=5):
    n = W.shape[0]
    W = np.where(W < W.max() / n_epochs, 0.0, W)
    head, tail = np.nonzero(W)
    eps = (W.max() / W[head, tail]).tolist()
    epn = [e / rate for e in eps]
    nxt, nxt_neg = list(eps), list(epn)
    head, tail = head.tolist(), tail.tolist()
    y = [list(map(float, p)) for p in y0]
    rng = np.random.RandomState(seed)
    alpha = 1.0
    for ep in range(n_epochs):
        draws = iter(rng.randint(0, n, size=8 * len(head)).tolist())
        for e in range(len(head)):
            if nxt[e] > ep:
                continue
            cur, oth = y[head[e]], y[tail[e]]
            dx, dy = cur[0] - oth[0], cur[1] - oth[1]
            d2 = dx * dx + dy * dy
            c = -2.0 * a * b * d2 ** (b - 1.0) / (a * d2 ** b + 1.0) if d2 > 0.0 else 0.0
            gx, gy = clip(c * dx) * alpha, clip(c * dy) * alpha
            cur[0] += gx
            cur[1] += gy
            oth[0] -= gx
            oth[1] -= gy
            nxt[e] += eps[e]
            n_neg = int((ep - nxt_neg[e]) / epn[e])
            for _ in range(n_neg):
                k = next(draws)
                oth = y[k]
                dx, dy = cur[0] - oth[0], cur[1] - oth[1]
                d2 = dx * dx + dy * dy
                if d2 <= 0.0:
                    continue
                c = 2.0 * gamma * b / ((0.001 + d2) * (a * d2 ** b + 1.0))
                cur[0] += clip(c * dx) * alpha
                cur[1] += clip(c * dy) * alpha
            nxt_neg[e] += n_neg * epn[e]
        alpha = 1.0 - (ep + 1) / n_epochs
    return np.array(y)


def main():
    from test_cpu_tsne import blobs

    inputs = (("six_blobs", six_blobs(N, D), 15), ("tsne_blobs", blobs(N, D), 30))
    a, b = find_ab(MIN_DIST)
    emb = np.zeros((len(inputs), len(SEEDS), N, 2), dtype=np.float32)
    trust = np.zeros((len(inputs), len(SEEDS)))
    trust_pca = np.zeros(len(inputs))
    for q, (name, x, k) in enumerate(inputs):
        W = fuzzy_graph(*knn(x, k))
        trust_pca[q] = trustworthiness(x, pca_2d(x), n_neighbors=TRUST_K)
        for s, seed in enumerate(SEEDS):
            y = sequential_layout(W, init_layout(x, seed), a, b, seed, EPOCHS)
            emb[q, s] = y
            trust[q, s] = trustworthiness(x, y, n_neighbors=TRUST_K)
            print(f"{name} k={k} seed={seed}: trustworthiness {trust[q, s]:.4f} (pca_2d {trust_pca[q]:.4f})", flush=True)
    np.savez_compressed(HERE / "umap_sequential_oracle.npz", names=np.array([i[0] for i in inputs]),
                        n_neighbors=np.array([i[2] for i in inputs]), seeds=np.array(SEEDS), embeddings=emb,
                        trustworthiness=trust, trustworthiness_pca_2d=trust_pca, a=a, b=b,
                        n_epochs=EPOCHS, min_dist=MIN_DIST, trust_neighbors=TRUST_K)


if __name__ == "__main__":
    main()

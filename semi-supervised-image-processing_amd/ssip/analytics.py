"""Embedding analytics: K-Means, DBSCAN, silhouette and the k-distance curve
over the PCA cluster space (reference src/clustering.py:330-438).

The O(N*K*d) and O(N^2*d) distance work runs in the kernels of
csrc/analytics.hip; what stays on the host is the control flow around them:

* ``kmeans_fit`` replays ``sklearn.cluster.KMeans(n_init=..., random_state=
  seed)``: centre X by its column mean (in X's dtype), ``tol = mean(var(Xc)) *
  1e-4``, one shared ``RandomState`` over the inits, k-means++ seeding through
  the public ``sklearn.cluster.kmeans_plusplus`` on the host, then a plain
  Lloyd loop on the backend (stop on unchanged labels or on a squared centre
  shift <= tol, at most 300 iterations, one final assignment), keeping the
  lowest-inertia init.
* ``dbscan`` labels by sklearn's order-free rule: cluster ids are the
  connected components of the core-point graph numbered by their lowest core
  index, a border point takes the smallest id among its core neighbours,
  everything else is -1.  Up to ``EPS_MAX_N`` points the eps graph is a packed
  bitmap labelled breadth-first on the host; above it (``dbscan_stream``, to
  ``DBSCAN_STREAM_MAX_N``) no graph is stored: labels are propagated on the
  backend over recomputed distances, a walk and a hook per round with one
  read-back of the ``changed`` flags, for up to four min_samples at once.
* ``silhouette`` finishes a, b and s in fp64 from per-cluster distance sums.
* ``tsne_fit`` is sklearn's exact t-SNE (``TSNE(method="exact", init="pca",
  learning_rate="auto")``): the joint probabilities once (csrc/tsne.hip), then
  sklearn's two-phase schedule of gradient and momentum / gains steps with one
  read-back of four scalars on every 50th iteration and nothing else crossing
  the bus.
* ``umap_fit`` is umap-learn's algorithm with its own kernels: exact kNN (a
  pairwise kernel of csrc/analytics.hip), ``smooth_knn_dist`` and the
  membership strengths (csrc/umap.hip, like the epochs) on the backend,
  the fuzzy union / curve fit / schedule / init on the host (O(N k)), then the
  layout epochs on the backend in Jacobi order with hashed negative samples.

The Lloyd driver and the DBSCAN labeller work on a small backend object
(``assign`` / ``update`` / ``eps_graph`` / ...).  ``DeviceBackend`` launches
the HIP kernels; ``NumpyBackend`` is the opt-in host path (``--device cpu`` of
``src.clustering``, like ssip/host.py) and lets the host logic be tested
without a GPU.  Nothing here falls back from one to the other.
"""
from __future__ import annotations

import logging
from typing import Optional, Tuple

import numpy as np

MAX_ITER = 300
TOL = 1e-4
KTH_MAX = 64
EPS_MAX_N = 65536
DBSCAN_STREAM_MAX_N = 1 << 20
DBSCAN_STREAM_MAX_M = 4  # min_samples configurations of one walk
DBSCAN_MAX_WALKS = 64
SILHOUETTE_MAX_K = 256
TSNE_MAX_N = 32768  # P is N^2 floats: 4 GB at the cap (csrc/tsne.hip)
TSNE_EXPLORATION_ITERS = 250
TSNE_EARLY_EXAGGERATION = 12.0
TSNE_CHECK_EVERY = 50
TSNE_MIN_GRAD_NORM = 1e-7
KNN_MAX_K = 64
UMAP_MAX_N = 1 << 20
UMAP_NEGATIVE_SAMPLE_RATE = 5
UMAP_MAX_NEG = 65536  # draws of one edge in one epoch (csrc/umap.hip clamps alike)
UMAP_INITS = ("spectral", "pca")


# ---------------------------------------------------------------------------
# host pieces shared by both backends
# ---------------------------------------------------------------------------
def pack_adjacency(adj: np.ndarray) -> np.ndarray:
    """bool [R][N] -> uint32 [R][ceil(N/32)], bit (j % 32) of word j / 32 = adj[i][j]."""
    adj = np.asarray(adj, dtype=bool)
    rows, n = adj.shape
    words = (n + 31) // 32
    padded = np.zeros((rows, words * 32), dtype=bool)
    padded[:, :n] = adj
    return np.packbits(padded, axis=1, bitorder="little").view("<u4").reshape(rows, words)


def _bits_to_indices(words: np.ndarray, n: int) -> np.ndarray:
    return np.flatnonzero(np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:n])


def dbscan_labels_from_graph(degree: np.ndarray, bitmap: np.ndarray, min_samples: int) -> np.ndarray:
    """sklearn.cluster.DBSCAN's labels from the eps graph (degree counts self).

    ``bitmap`` is the packed adjacency (``pack_adjacency``) or a dense bool
    [N][N] matrix.  Components are grown breadth-first over the bitmap rows of
    core points, from seeds in increasing index, so ids come out numbered by
    their lowest core index and a border point keeps the first (= smallest)
    id that reaches it.
    """
    bitmap = np.asarray(bitmap)
    if bitmap.dtype == bool:
        bitmap = pack_adjacency(bitmap)
    degree = np.asarray(degree)
    n = degree.shape[0]
    core = degree >= int(min_samples)
    labels = np.full(n, -1, dtype=np.int64)
    cid = 0
    for seed in np.flatnonzero(core):
        if labels[seed] != -1:
            continue
        visited = np.zeros(bitmap.shape[1], dtype=np.uint32)
        visited[seed >> 5] = np.uint32(1) << np.uint32(seed & 31)
        frontier = np.array([seed])
        while frontier.size:
            reach = np.bitwise_or.reduce(bitmap[frontier], axis=0)
            new = reach & ~visited
            visited |= new
            idx = _bits_to_indices(new, n)
            frontier = idx[core[idx]]
        members = _bits_to_indices(visited, n)
        take = members[core[members] | (labels[members] == -1)]
        labels[take] = cid
        cid += 1
    return labels


def _dbscan_min_samples(values) -> np.ndarray:
    """int32 [M] min_samples of one walk, 1 <= M <= DBSCAN_STREAM_MAX_M."""
    ms = np.minimum(np.asarray(list(values), dtype=np.int64).reshape(-1), np.iinfo(np.int32).max).astype(np.int32)
    if not 1 <= ms.size <= DBSCAN_STREAM_MAX_M:
        raise ValueError(f"ssip.analytics: a DBSCAN walk takes 1..{DBSCAN_STREAM_MAX_M} min_samples values "
                         f"(got {ms.size})")
    return ms


def _dbscan_init_labels(degree: np.ndarray, ms: np.ndarray) -> np.ndarray:
    """int32 [M][N]: a core row starts as its own label, every other row holds the sentinel N."""
    n = degree.shape[0]
    return np.where(degree[None, :] >= ms[:, None], np.arange(n, dtype=np.int32)[None, :], np.int32(n)).astype(np.int32)


def _relocate_empty(X: np.ndarray, labels: np.ndarray, mind2: np.ndarray, old: np.ndarray) -> np.ndarray:
    """New centres when some cluster attracted no point, as sklearn's dense
    relocation does: each empty centre moves to one of the points farthest from
    its own centre, and that point leaves its donor cluster's sum."""
    k = old.shape[0]
    counts = np.bincount(labels, minlength=k).astype(np.float64)
    sums = np.zeros((k, X.shape[1]), dtype=np.float64)
    for c in np.flatnonzero(counts):
        sums[c] = X[labels == c].sum(axis=0, dtype=np.float64)
    empty = np.flatnonzero(counts == 0)
    n_empty = empty.size
    far = np.argpartition(mind2, -n_empty)[: -n_empty - 1: -1]
    for new_id, far_idx in zip(empty, far):
        donor = labels[far_idx]
        sums[donor] -= X[far_idx]
        sums[new_id] = X[far_idx]
        counts[new_id] = 1
        counts[donor] -= 1
    new = old.astype(np.float64).copy()
    nz = counts > 0
    new[nz] = sums[nz] / counts[nz, None]
    return new.astype(old.dtype)


def _float_matrix(X) -> np.ndarray:
    """X as an array of float32 or float64: every other dtype becomes float64."""
    X = np.asarray(X)
    if X.dtype not in (np.float32, np.float64):
        X = X.astype(np.float64)
    return X


def _same_clustering(a: np.ndarray, b: np.ndarray, k: int) -> bool:
    """True when the labels of a map one-to-one onto those of b (sklearn's
    check before it lets a later init replace the best one)."""
    return np.unique(a.astype(np.int64) * k + b).size == np.unique(a).size


# ---------------------------------------------------------------------------
# backends
# ---------------------------------------------------------------------------
class NumpyBackend:
    """Host backend: fp64 direct-difference distances (scipy cdist), the same
    method surface and bitmap format as the device backend."""

    name = "cpu"

    def __init__(self, X: np.ndarray):
        self.X = np.ascontiguousarray(_float_matrix(X))
        self.n, self.d = self.X.shape

    def _row_chunks(self, cols: int):
        step = max(1, (1 << 22) // max(cols, 1))
        for s in range(0, self.n, step):
            yield s, min(self.n, s + step)

    # -- K-Means --------------------------------------------------------------
    def begin(self, centres: np.ndarray) -> None:
        self.C = np.array(centres, dtype=self.X.dtype)
        self.Cn = self.C.copy()
        self._labels = np.full(self.n, -1, dtype=np.int32)
        self._prev = self._labels.copy()
        self._mind2 = np.zeros(self.n, dtype=np.float64)

    def assign(self) -> None:
        from scipy.spatial.distance import cdist

        self._prev, self._labels = self._labels, self._prev
        for s, e in self._row_chunks(self.C.shape[0]):
            d2 = cdist(self.X[s:e], self.C, "sqeuclidean")
            lab = np.argmin(d2, axis=1)
            self._labels[s:e] = lab
            self._mind2[s:e] = d2[np.arange(e - s), lab]

    def update(self) -> Tuple[float, float, int, int]:
        k = self.C.shape[0]
        counts = np.bincount(self._labels, minlength=k)
        new = self.C.astype(np.float64).copy()
        for c in np.flatnonzero(counts):
            new[c] = self.X[self._labels == c].sum(axis=0, dtype=np.float64) / counts[c]
        self.Cn = new.astype(self.X.dtype)
        self.counts = counts
        shift2 = float(((self.Cn.astype(np.float64) - self.C) ** 2).sum())
        changed = int(np.count_nonzero(self._labels != self._prev))
        return shift2, float(self._mind2.sum()), changed, int(np.count_nonzero(counts == 0))

    def relocate(self) -> float:
        self.Cn = _relocate_empty(self.X, self._labels, self._mind2, self.C)
        return float(((self.Cn.astype(np.float64) - self.C) ** 2).sum())

    def swap(self) -> None:
        self.C, self.Cn = self.Cn, self.C

    def labels(self) -> np.ndarray:
        return self._labels.copy()

    def centres(self) -> np.ndarray:
        return self.C.copy()

    # -- pairwise ---------------------------------------------------------------
    def eps_graph(self, eps: float) -> Tuple[np.ndarray, np.ndarray]:
        from scipy.spatial.distance import cdist

        words = (self.n + 31) // 32
        degree = np.zeros(self.n, dtype=np.int32)
        bitmap = np.zeros((self.n, words), dtype=np.uint32)
        e2 = float(eps) * float(eps)
        for s, e in self._row_chunks(self.n):
            adj = cdist(self.X[s:e], self.X, "sqeuclidean") <= e2
            degree[s:e] = adj.sum(axis=1)
            bitmap[s:e] = pack_adjacency(adj)
        return degree, bitmap

    # DBSCAN without the bitmap (dbscan_stream): the predicate of eps_graph in
    # row blocks, O(block x N) memory.
    def degree(self, eps: float) -> np.ndarray:
        from scipy.spatial.distance import cdist

        self._db_e2 = float(eps) * float(eps)
        self._db_degree = np.zeros(self.n, dtype=np.int32)
        for s, e in self._row_chunks(self.n):
            self._db_degree[s:e] = (cdist(self.X[s:e], self.X, "sqeuclidean") <= self._db_e2).sum(axis=1)
        return self._db_degree.copy()

    def dbscan_begin(self, min_samples_values) -> None:
        """Start the label problems of the last ``degree(eps)``, one per min_samples."""
        self._db_ms = _dbscan_min_samples(min_samples_values)
        self._db_labels = _dbscan_init_labels(self._db_degree, self._db_ms)
        self._db_nbr = np.full_like(self._db_labels, self.n)

    def dbscan_walk(self) -> None:
        """nbr_min[m][i] = min label over the core columns within eps of row i (N: none)."""
        from scipy.spatial.distance import cdist

        n = self.n
        core = self._db_degree[None, :] >= self._db_ms[:, None]
        col = np.where(core, self._db_labels, n)
        for s, e in self._row_chunks(n):
            adj = cdist(self.X[s:e], self.X, "sqeuclidean") <= self._db_e2
            for m in range(self._db_ms.size):
                self._db_nbr[m, s:e] = np.where(adj, col[m][None, :], n).min(axis=1)

    def dbscan_hook(self) -> np.ndarray:
        """Hook every core row's minimum onto itself and its label's row, then
        max(1, ceil(log2 N)) pointer jumps; returns changed[m]."""
        n = self.n
        changed = np.zeros(self._db_ms.size, dtype=np.int32)
        for m in range(self._db_ms.size):
            old, nbr = self._db_labels[m], self._db_nbr[m]
            rows = np.flatnonzero((self._db_degree >= self._db_ms[m]) & (nbr < n))
            new = old.copy()
            np.minimum.at(new, old[rows], nbr[rows])
            new[rows] = np.minimum(new[rows], nbr[rows])
            for _ in range(max(1, (n - 1).bit_length())):
                new[rows] = new[new[rows]]
            changed[m] = int(np.any(new != old))
            self._db_labels[m] = new
        return changed

    def dbscan_state(self) -> Tuple[np.ndarray, np.ndarray]:
        return self._db_labels.copy(), self._db_nbr.copy()

    def kth(self, k: int) -> np.ndarray:
        from scipy.spatial.distance import cdist

        out = np.zeros(self.n, dtype=np.float64)
        for s, e in self._row_chunks(self.n):
            d2 = cdist(self.X[s:e], self.X, "sqeuclidean")
            out[s:e] = np.sqrt(np.partition(d2, k - 1, axis=1)[:, k - 1])
        return out

    def cluster_sums(self, enc: np.ndarray, order: np.ndarray, k: int) -> np.ndarray:
        from scipy.spatial.distance import cdist

        sums = np.zeros((self.n, k), dtype=np.float64)
        starts = np.searchsorted(enc[order], np.arange(k))
        for s, e in self._row_chunks(self.n):
            dist = cdist(self.X[s:e], self.X[order], "euclidean")
            sums[s:e] = np.add.reduceat(dist, starts, axis=1)
        return sums


    # -- exact t-SNE ------------------------------------------------------------
    # The arithmetic of csrc/tsne.hip in fp64.  O(N^2) time per iteration and
    # O(N^2) memory for P: meant for --device cpu on small cohorts and for the
    # CPU tests, not as a replacement for Barnes-Hut at large N.
    def tsne_cond_p(self, perplexity: float) -> None:
        """P[i][j] = p(j|i) by sklearn's ``_binary_search_perplexity`` (beta from
        1, doubled / halved until bracketed, then bisected; at most 100 steps;
        tolerance 1e-5 on the entropy; a zero row sum counts as 1e-8), every row
        at once.  O(N^2) per step."""
        from scipy.spatial.distance import cdist

        n = self.n
        d2 = cdist(self.X, self.X, "sqeuclidean")
        off = ~np.eye(n, dtype=bool)
        target = np.log(float(perplexity))
        tiny, tol = float(np.float32(1e-8)), float(np.float32(1e-5))  # sklearn keeps both as C floats
        beta = np.ones(n)
        lo = np.full(n, -np.inf)
        hi = np.full(n, np.inf)
        used = beta.copy()
        sums = np.ones(n)
        active = np.ones(n, dtype=bool)
        for _ in range(100):
            rows = np.flatnonzero(active)
            if rows.size == 0:
                break
            b = beta[rows]
            e = np.exp(-d2[rows] * b[:, None]) * off[rows]
            s0 = e.sum(axis=1)
            s0[s0 == 0.0] = tiny
            s1 = (d2[rows] * e).sum(axis=1)
            with np.errstate(divide="ignore"):
                diff = np.log(s0) + b * (s1 / s0) - target
            used[rows] = b
            sums[rows] = s0
            done = np.abs(diff) <= tol
            up = (diff > 0.0) & ~done
            down = ~up & ~done
            r_up, r_dn = rows[up], rows[down]
            lo[r_up] = beta[r_up]
            beta[r_up] = np.where(np.isinf(hi[r_up]), beta[r_up] * 2.0, (beta[r_up] + hi[r_up]) / 2.0)
            hi[r_dn] = beta[r_dn]
            beta[r_dn] = np.where(np.isinf(lo[r_dn]), beta[r_dn] / 2.0, (beta[r_dn] + lo[r_dn]) / 2.0)
            active[rows[done]] = False
        self.P = np.exp(-d2 * used[:, None]) * off / sums[:, None]
        self.beta = used

    def tsne_joint_p(self) -> None:
        """P = (P + P^T) / sum, in place of the conditional P.  O(N^2)."""
        sym = self.P + self.P.T
        self.P = sym / sym.sum()

    def tsne_begin(self, y0: np.ndarray) -> None:
        self.Y = np.array(y0, dtype=np.float64)
        self.tsne_reset()

    def tsne_reset(self) -> None:
        self.upd = np.zeros_like(self.Y)
        self.gains = np.ones_like(self.Y)

    def tsne_grad(self, compute_error: bool) -> None:
        """attr, rep, z and (when asked) the error share of every row at the
        current Y.  O(N^2)."""
        n, Y = self.n, self.Y
        self.attr = np.zeros((n, 2))
        self.rep = np.zeros((n, 2))
        self.z = np.zeros(n)
        self.err_rows = np.zeros(n)
        for s, e in self._row_chunks(n):
            dx = Y[s:e, 0, None] - Y[None, :, 0]
            dy = Y[s:e, 1, None] - Y[None, :, 1]
            q = 1.0 + dx * dx + dy * dy
            w = 1.0 / q
            w[np.arange(e - s), np.arange(s, e)] = 0.0
            P = self.P[s:e]
            pw, w2 = P * w, w * w
            self.attr[s:e, 0] = (pw * dx).sum(axis=1)
            self.attr[s:e, 1] = (pw * dy).sum(axis=1)
            self.rep[s:e, 0] = (w2 * dx).sum(axis=1)
            self.rep[s:e, 1] = (w2 * dy).sum(axis=1)
            self.z[s:e] = w.sum(axis=1)
            if compute_error:
                pos = P > 0.0
                self.err_rows[s:e] = np.where(pos, P * (np.log(np.where(pos, P, 1.0)) + np.log(q)), 0.0).sum(axis=1)

    def tsne_step(self, exaggeration: float, momentum: float, learning_rate: float) -> None:
        """grad = 4 (exaggeration attr - rep / Z), then sklearn's gains / momentum step."""
        Z = float(self.z.sum())
        grad = 4.0 * (exaggeration * self.attr - self.rep / Z)
        self.grad = grad
        inc = self.upd * grad < 0.0
        self.gains = np.maximum(np.where(inc, self.gains + 0.2, self.gains * 0.8), 0.01)
        gained = grad * self.gains
        self.upd = momentum * self.upd - learning_rate * gained
        self.Y = self.Y + self.upd
        self._scalars = (Z, float(self.err_rows.sum()) + np.log(Z), float(np.sqrt((grad ** 2).sum())),
                         float(np.sqrt((gained ** 2).sum())))

    def tsne_scalars(self) -> Tuple[float, float, float, float]:
        return self._scalars

    def tsne_terms(self) -> dict:
        return {"attr": self.attr.copy(), "rep": self.rep.copy(), "z": self.z.copy(), "err": self.err_rows.copy(),
                "grad": self.grad.copy()}

    def tsne_embedding(self) -> np.ndarray:
        return self.Y.copy()

    def tsne_p(self) -> np.ndarray:
        return self.P.copy()

    # -- native UMAP --------------------------------------------------------------
    # The arithmetic of csrc/umap.hip with fp64 distances and forces; the
    # schedule state is float32 and advances by the same float32 operations as
    # on the device, so both backends fire the same edges and draw the same
    # negative samples.
    def knn(self, k: int) -> Tuple[np.ndarray, np.ndarray]:
        """(d2 [N][k], idx int32 [N][k]): the k smallest squared distances of
        every row, self included, ascending, a tie to the lower index.  O(N^2)."""
        from scipy.spatial.distance import cdist

        k = _check_k(k, self.n)
        d2 = np.empty((self.n, k), dtype=np.float64)
        idx = np.empty((self.n, k), dtype=np.int32)
        for s, e in self._row_chunks(self.n):
            full = cdist(self.X[s:e], self.X, "sqeuclidean")
            kth = np.partition(full, k - 1, axis=1)[:, k - 1]
            below = full <= kth[:, None]
            exact = below.sum(axis=1) == k
            rows = np.flatnonzero(exact)
            if rows.size:
                cols = np.nonzero(below[rows])[1].reshape(rows.size, k)  # ascending index
                val = np.take_along_axis(full[rows], cols, axis=1)
                order = np.argsort(val, axis=1, kind="stable")
                d2[s + rows] = np.take_along_axis(val, order, axis=1)
                idx[s + rows] = np.take_along_axis(cols, order, axis=1)
            for r in np.flatnonzero(~exact):  # ties at the k-th distance: the lowest indices win
                order = np.argsort(full[r], kind="stable")[:k]
                d2[s + r] = full[r, order]
                idx[s + r] = order
        self.set_knn(d2, idx)
        return d2.copy(), idx.copy()

    def set_knn(self, d2: np.ndarray, idx: np.ndarray) -> None:
        d2, idx = _check_knn(d2, idx, self.n)
        self._knn_d2 = np.ascontiguousarray(d2, dtype=np.float64)
        self._knn_idx = np.ascontiguousarray(idx, dtype=np.int32)

    def knn_columns(self) -> int:
        return 0 if getattr(self, "_knn_idx", None) is None else self._knn_idx.shape[1]

    def knn_indices(self, k: int) -> np.ndarray:
        return self._knn_idx[:, :k].copy()

    def umap_fuzzy(self, k: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(rho [N], sigma [N], memberships [N][k]) of umap-learn's
        ``smooth_knn_dist`` and ``compute_membership_strengths`` over the first
        k columns of the kNN result, every row at once."""
        k = _check_k(k, self.n)
        if self.knn_columns() < k:
            raise ValueError(f"ssip.analytics: umap_fuzzy({k}) needs a kNN result of at least {k} columns")
        n = self.n
        dist = np.sqrt(self._knn_d2[:, :k])
        pos = dist > 0.0
        rho = np.where(pos.any(axis=1), np.where(pos, dist, np.inf).min(axis=1), 0.0)
        target = np.log2(float(k))
        lo, hi, mid = np.zeros(n), np.full(n, np.inf), np.ones(n)
        dd = dist - rho[:, None]
        active = np.ones(n, dtype=bool)
        for _ in range(64):
            rows = np.flatnonzero(active)
            if rows.size == 0:
                break
            d = dd[rows, 1:]
            with np.errstate(over="ignore"):
                psum = np.where(d > 0.0, np.exp(-np.where(d > 0.0, d, 0.0) / mid[rows, None]), 1.0).sum(axis=1)
            done = np.abs(psum - target) < 1e-5
            gt = (psum > target) & ~done
            le = ~gt & ~done
            r_gt, r_le = rows[gt], rows[le]
            hi[r_gt] = mid[r_gt]
            mid[r_gt] = (lo[r_gt] + hi[r_gt]) / 2.0
            lo[r_le] = mid[r_le]
            mid[r_le] = np.where(np.isinf(hi[r_le]), mid[r_le] * 2.0, (lo[r_le] + hi[r_le]) / 2.0)
            active[rows[done]] = False
        floor = 1e-3 * np.where(rho > 0.0, dist.mean(axis=1), dist.mean())
        sigma = np.maximum(mid, floor)
        with np.errstate(divide="ignore", invalid="ignore"):
            memb = np.where((dd <= 0.0) | (sigma[:, None] == 0.0), 1.0, np.exp(-np.maximum(dd, 0.0) / sigma[:, None]))
        memb[self._knn_idx[:, :k] == np.arange(n)[:, None]] = 0.0
        return rho, sigma, memb

    def umap_begin(self, csr, y0: np.ndarray, a: float, b: float, seed: int, gamma: float = 1.0, state=None) -> None:
        row_ptr, col, eps = _check_csr(csr, self.n)
        self._u_rows = np.repeat(np.arange(self.n, dtype=np.int64), np.diff(row_ptr))
        self._u_col = col.astype(np.int64)
        self._u_eps = eps
        self._u_epn = eps / np.float32(UMAP_NEGATIVE_SAMPLE_RATE)
        # both "next" arrays start at their period, or at a given (next_sample, next_neg)
        self._u_next = np.array(self._u_eps if state is None else state[0], dtype=np.float32)
        self._u_next_neg = np.array(self._u_epn if state is None else state[1], dtype=np.float32)
        self._u_y = np.array(y0, dtype=np.float32).reshape(self.n, 2)
        self._u_par = (float(np.float32(a)), float(np.float32(b)), float(np.float32(gamma)), int(seed) & 0xFFFFFFFF)

    def umap_epoch(self, n: int, alpha: float) -> None:
        a, b, gamma, seed = self._u_par
        y = self._u_y.astype(np.float64)
        nf = np.float32(n)
        fire = np.flatnonzero(self._u_next <= nf)
        force = np.zeros((self.n, 2))
        if fire.size:
            i, j = self._u_rows[fire], self._u_col[fire]
            force += _scatter2(i, 2.0 * _umap_attraction(y[i] - y[j], a, b), self.n)
            self._u_next[fire] = self._u_next[fire] + self._u_eps[fire]
            epn = self._u_epn[fire]
            n_neg = np.clip(((nf - self._u_next_neg[fire]) / epn).astype(np.int32), 0, UMAP_MAX_NEG)
            self._u_next_neg[fire] = self._u_next_neg[fire] + n_neg.astype(np.float32) * epn
            for p in range(int(n_neg.max())):
                sel = n_neg > p
                ei, vi = fire[sel], i[sel]
                k = (umap_hash(seed, n, ei, p) % np.uint64(self.n)).astype(np.int64)
                keep = k != vi
                force += _scatter2(vi[keep], _umap_repulsion(y[vi[keep]] - y[k[keep]], a, b, gamma), self.n)
        self._u_y = (y + float(np.float32(alpha)) * force).astype(np.float32)

    def umap_embedding(self) -> np.ndarray:
        return self._u_y.copy()

    def umap_state(self) -> Tuple[np.ndarray, np.ndarray]:
        return self._u_next.copy(), self._u_next_neg.copy()


class DeviceBackend:
    """libssip_hip.so backend (csrc/analytics.hip).  torch only owns the
    buffers and the stream; every distance is computed by the HIP kernels."""

    name = "cuda"

    def __init__(self, X: np.ndarray):
        import torch

        from . import _lib, ops

        if not torch.cuda.is_available():
            raise RuntimeError("ssip.analytics: the device backend needs the HIP device (use device='cpu' for the "
                               "host path)")
        self._torch, self._lib, self._ops = torch, _lib, ops
        self.Xh = np.ascontiguousarray(X, dtype=np.float32)
        self.n, self.d = self.Xh.shape
        if not 1 <= self.d <= 512:
            raise ValueError(f"ssip.analytics: feature dimension {self.d} outside 1..512")
        self.dev = torch.device("cuda")
        self.X = torch.from_numpy(self.Xh).to(self.dev)

    def _call(self, name, *args):
        return self._lib.call(name, *args, self._ops.stream_ptr())

    def _p(self, t):
        return self._lib.ptr(t)

    def _workspace(self, query: str, *args):
        """(device buffer, its size) of as many bytes as the library's ``query`` entry point asks for."""
        nbytes = int(self._lib.call(query, *args))
        if nbytes < 0:
            self._lib.check(nbytes, query)
        return self._torch.empty(nbytes, dtype=self._torch.uint8, device=self.dev), nbytes

    # -- K-Means --------------------------------------------------------------
    def begin(self, centres: np.ndarray) -> None:
        t = self._torch
        k = centres.shape[0]
        self.k = k
        self.C = t.from_numpy(np.ascontiguousarray(centres, dtype=np.float32)).to(self.dev)
        self.Cn = t.empty_like(self.C)
        self._labels = t.full((self.n,), -1, dtype=t.int32, device=self.dev)
        self._prev = t.full((self.n,), -1, dtype=t.int32, device=self.dev)
        self._mind2 = t.empty(self.n, dtype=t.float32, device=self.dev)
        self._ws, self._ws_bytes = self._workspace("ssip_kmeans_workspace_bytes", self.n, self.d, k)
        self._counts = t.empty(k, dtype=t.int32, device=self.dev)
        self._scalars = t.empty(4, dtype=t.float64, device=self.dev)

    def assign(self) -> None:
        self._prev, self._labels = self._labels, self._prev
        self._call("ssip_kmeans_assign", self.n, self.d, self.k, self._p(self.X), self._p(self.C),
                   self._p(self._prev), self._p(self._labels), self._p(self._mind2), self._p(self._ws),
                   self._ws_bytes)

    def update(self) -> Tuple[float, float, int, int]:
        self._call("ssip_kmeans_update", self.n, self.d, self.k, self._p(self._ws), self._ws_bytes, self._p(self.C),
                   self._p(self.Cn), self._p(self._counts), self._p(self._scalars))
        s = self._scalars.cpu().numpy()  # the one read-back of an iteration
        return float(s[0]), float(s[1]), int(s[2]), int(s[3])

    def relocate(self) -> float:
        old = self.C.cpu().numpy()
        new = _relocate_empty(self.Xh, self._labels.cpu().numpy(), self._mind2.cpu().numpy(), old)
        self.Cn.copy_(self._torch.from_numpy(new))
        return float(((new.astype(np.float64) - old) ** 2).sum())

    def swap(self) -> None:
        self.C, self.Cn = self.Cn, self.C

    def labels(self) -> np.ndarray:
        return self._labels.cpu().numpy()

    def centres(self) -> np.ndarray:
        return self.C.cpu().numpy()

    # -- pairwise ---------------------------------------------------------------
    def eps_graph(self, eps: float) -> Tuple[np.ndarray, np.ndarray]:
        t = self._torch
        if self.n > EPS_MAX_N:
            raise ValueError(f"ssip.analytics: the eps graph supports N <= {EPS_MAX_N} (got {self.n})")
        words = (self.n + 31) // 32
        degree = t.empty(self.n, dtype=t.int32, device=self.dev)
        bitmap = t.empty((self.n, words), dtype=t.int32, device=self.dev)
        self._call("ssip_pairwise_eps", self.n, self.d, self._p(self.X), float(eps), self._p(degree),
                   self._p(bitmap))
        return degree.cpu().numpy(), bitmap.cpu().numpy().view(np.uint32)

    # DBSCAN without the bitmap (dbscan_stream): degree, labels and minima stay
    # on the device; a round reads back the changed flags only.
    def degree(self, eps: float) -> np.ndarray:
        t = self._torch
        if self.n > DBSCAN_STREAM_MAX_N:
            raise ValueError(f"ssip.analytics: DBSCAN supports N <= {DBSCAN_STREAM_MAX_N} (got {self.n})")
        self._db_eps = float(eps)
        self._db_degree = t.empty(self.n, dtype=t.int32, device=self.dev)
        self._call("ssip_pairwise_degree", self.n, self.d, self._p(self.X), self._db_eps, self._p(self._db_degree))
        self._db_degree_host = self._db_degree.cpu().numpy()
        return self._db_degree_host.copy()

    def dbscan_begin(self, min_samples_values) -> None:
        """Start the label problems of the last ``degree(eps)``, one per min_samples."""
        t = self._torch
        ms = _dbscan_min_samples(min_samples_values)
        self._db_m = int(ms.size)
        self._db_ms = t.from_numpy(ms).to(self.dev)
        self._db_labels = t.from_numpy(_dbscan_init_labels(self._db_degree_host, ms)).to(self.dev)
        self._db_next = t.empty_like(self._db_labels)
        self._db_scratch = t.empty_like(self._db_labels)
        self._db_nbr = t.full_like(self._db_labels, self.n)
        self._db_changed = t.empty(self._db_m, dtype=t.int32, device=self.dev)

    def dbscan_walk(self) -> None:
        self._call("ssip_dbscan_walk", self.n, self.d, self._p(self.X), self._db_eps, self._db_m,
                   self._p(self._db_degree), self._p(self._db_ms), self._p(self._db_labels), self._p(self._db_nbr))

    def dbscan_hook(self) -> np.ndarray:
        self._call("ssip_dbscan_hook", self.n, self._db_m, self._p(self._db_degree), self._p(self._db_ms),
                   self._p(self._db_labels), self._p(self._db_nbr), self._p(self._db_next),
                   self._p(self._db_scratch), self._p(self._db_changed))
        self._db_labels, self._db_next = self._db_next, self._db_labels
        return self._db_changed.cpu().numpy()  # the one read-back of a round

    def dbscan_state(self) -> Tuple[np.ndarray, np.ndarray]:
        return self._db_labels.cpu().numpy(), self._db_nbr.cpu().numpy()

    def kth(self, k: int) -> np.ndarray:
        t = self._torch
        out = t.empty(self.n, dtype=t.float32, device=self.dev)
        self._call("ssip_pairwise_kth", self.n, self.d, int(k), self._p(self.X), self._p(out))
        return out.cpu().numpy().astype(np.float64)

    def cluster_sums(self, enc: np.ndarray, order: np.ndarray, k: int) -> np.ndarray:
        t = self._torch
        if k > SILHOUETTE_MAX_K:
            raise ValueError(f"ssip.analytics: silhouette supports at most {SILHOUETTE_MAX_K} clusters on the device "
                             f"(got {k})")
        lab = t.from_numpy(np.ascontiguousarray(enc, dtype=np.int32)).to(self.dev)
        ordr = t.from_numpy(np.ascontiguousarray(order, dtype=np.int32)).to(self.dev)
        sums = t.empty((self.n, k), dtype=t.float32, device=self.dev)
        self._call("ssip_pairwise_cluster_sums", self.n, self.d, int(k), self._p(self.X), self._p(lab),
                   self._p(ordr), self._p(sums))
        return sums.cpu().numpy().astype(np.float64)


    # -- exact t-SNE (csrc/tsne.hip) ---------------------------------------------
    def _tsne_alloc(self) -> None:
        t = self._torch
        if getattr(self, "_tws", None) is not None:
            return
        self._tws, self._tws_bytes = self._workspace("ssip_tsne_workspace_bytes", self.n)
        self.P = t.empty((self.n, self.n), dtype=t.float32, device=self.dev)
        self._beta = t.empty(self.n, dtype=t.float64, device=self.dev)
        self._tscalars = t.empty(4, dtype=t.float64, device=self.dev)

    def tsne_cond_p(self, perplexity: float) -> None:
        self._tsne_alloc()
        self._call("ssip_tsne_cond_p", self.n, self.d, self._p(self.X), float(perplexity), self._p(self.P),
                   self._p(self._beta))

    def tsne_joint_p(self) -> None:
        self._call("ssip_tsne_joint_p", self.n, self._p(self.P), self._p(self._tws), self._tws_bytes)

    def tsne_begin(self, y0: np.ndarray) -> None:
        t = self._torch
        self._tsne_alloc()
        self.Y = t.from_numpy(np.ascontiguousarray(y0, dtype=np.float32)).to(self.dev)
        self.upd = t.zeros_like(self.Y)
        self.gains = t.ones_like(self.Y)

    def tsne_reset(self) -> None:
        self.upd.zero_()
        self.gains.fill_(1.0)

    def tsne_grad(self, compute_error: bool) -> None:
        self._call("ssip_tsne_grad", self.n, self._p(self.P), self._p(self.Y), int(bool(compute_error)),
                   self._p(self._tws), self._tws_bytes)

    def tsne_step(self, exaggeration: float, momentum: float, learning_rate: float) -> None:
        self._call("ssip_tsne_update", self.n, self._p(self._tws), self._tws_bytes, self._p(self.Y), self._p(self.upd),
                   self._p(self.gains), float(exaggeration), float(momentum), float(learning_rate),
                   self._p(self._tscalars))

    def tsne_scalars(self) -> Tuple[float, float, float, float]:
        s = self._tscalars.cpu().numpy()  # the one read-back, on error iterations only
        return float(s[0]), float(s[1]), float(s[2]), float(s[3])

    def tsne_terms(self) -> dict:
        """Row sums and gradient of the last grad + step, from the workspace (include/ssip.h)."""
        n = self.n
        head = ((4 * ((n + 255) // 256) + 1) * 8 + 15) // 16 * 16
        raw = self._tws[head:head + 8 * n * 4].cpu().numpy().view(np.float32)
        red = raw[:6 * n].reshape(6, n)
        return {"attr": red[0:2].T.copy(), "rep": red[2:4].T.copy(), "z": red[4].copy(), "err": red[5].copy(),
                "grad": raw[6 * n:].reshape(n, 2).copy()}

    def tsne_embedding(self) -> np.ndarray:
        return self.Y.cpu().numpy()

    def tsne_p(self) -> np.ndarray:
        return self.P.cpu().numpy()

    # -- native UMAP (kNN: csrc/analytics.hip, the rest: csrc/umap.hip) ----------
    def knn(self, k: int) -> Tuple[np.ndarray, np.ndarray]:
        t = self._torch
        k = _check_k(k, self.n)
        self._knn_d2 = t.empty((self.n, k), dtype=t.float32, device=self.dev)
        self._knn_idx = t.empty((self.n, k), dtype=t.int32, device=self.dev)
        self._call("ssip_knn", self.n, self.d, k, self._p(self.X), self._p(self._knn_d2), self._p(self._knn_idx))
        self._knn_idx_host = self._knn_idx.cpu().numpy()
        return self._knn_d2.cpu().numpy(), self._knn_idx_host.copy()

    def set_knn(self, d2: np.ndarray, idx: np.ndarray) -> None:
        t = self._torch
        d2, idx = _check_knn(d2, idx, self.n)
        self._knn_idx_host = np.ascontiguousarray(idx, dtype=np.int32)
        self._knn_d2 = t.from_numpy(np.ascontiguousarray(d2, dtype=np.float32)).to(self.dev)
        self._knn_idx = t.from_numpy(self._knn_idx_host).to(self.dev)

    def knn_columns(self) -> int:
        return 0 if getattr(self, "_knn_idx", None) is None else int(self._knn_idx.shape[1])

    def knn_indices(self, k: int) -> np.ndarray:
        return self._knn_idx_host[:, :k].copy()

    def umap_fuzzy(self, k: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        t = self._torch
        k = _check_k(k, self.n)
        if self.knn_columns() < k:
            raise ValueError(f"ssip.analytics: umap_fuzzy({k}) needs a kNN result of at least {k} columns")
        ws, ws_bytes = self._workspace("ssip_umap_workspace_bytes", self.n)
        rho = t.empty(self.n, dtype=t.float32, device=self.dev)
        sigma = t.empty(self.n, dtype=t.float32, device=self.dev)
        memb = t.empty((self.n, k), dtype=t.float32, device=self.dev)
        self._call("ssip_umap_fuzzy", self.n, k, self.knn_columns(), self._p(self._knn_d2), self._p(self._knn_idx),
                   self._p(rho), self._p(sigma), self._p(memb), self._p(ws), ws_bytes)
        return rho.cpu().numpy(), sigma.cpu().numpy(), memb.cpu().numpy()

    def umap_begin(self, csr, y0: np.ndarray, a: float, b: float, seed: int, gamma: float = 1.0, state=None) -> None:
        t = self._torch
        row_ptr, col, eps = _check_csr(csr, self.n)

        def up(arr, dtype):
            return t.from_numpy(np.array(arr, dtype=dtype, order="C")).to(self.dev)  # a copy: the input may be read-only

        self._u_row_ptr, self._u_col = up(row_ptr, np.int32), up(col, np.int32)
        epn = eps / np.float32(UMAP_NEGATIVE_SAMPLE_RATE)
        self._u_eps, self._u_epn = up(eps, np.float32), up(epn, np.float32)
        # both "next" arrays start at their period, or at a given (next_sample, next_neg)
        self._u_next = up(eps if state is None else state[0], np.float32)
        self._u_next_neg = up(epn if state is None else state[1], np.float32)
        if self._u_next.shape != self._u_eps.shape or self._u_next_neg.shape != self._u_eps.shape:
            raise ValueError("ssip.analytics: the schedule state must hold one value per edge")
        self._u_y = up(np.asarray(y0).reshape(self.n, 2), np.float32)
        self._u_y2 = t.empty_like(self._u_y)
        self._u_par = (float(a), float(b), float(gamma), int(seed) & 0xFFFFFFFF)

    def umap_epoch(self, n: int, alpha: float) -> None:
        a, b, gamma, seed = self._u_par
        self._call("ssip_umap_epoch", self.n, self._p(self._u_row_ptr), self._p(self._u_col), self._p(self._u_eps),
                   self._p(self._u_epn), self._p(self._u_next), self._p(self._u_next_neg), self._p(self._u_y),
                   self._p(self._u_y2), a, b, gamma, float(alpha), int(n), seed)
        self._u_y, self._u_y2 = self._u_y2, self._u_y

    def umap_embedding(self) -> np.ndarray:
        return self._u_y.cpu().numpy()

    def umap_state(self) -> Tuple[np.ndarray, np.ndarray]:
        return self._u_next.cpu().numpy(), self._u_next_neg.cpu().numpy()


def make_backend(X: np.ndarray, device: str = "cuda"):
    """'cuda' -> the HIP kernels, 'cpu' -> the numpy host path (explicit opt-in)."""
    if device == "cuda":
        return DeviceBackend(X)
    if device == "cpu":
        return NumpyBackend(X)
    raise ValueError(f"ssip.analytics: unknown device {device!r} (cuda or cpu)")


# ---------------------------------------------------------------------------
# public functions
# ---------------------------------------------------------------------------
def lloyd(backend, centres: np.ndarray, tol: float, max_iter: int = MAX_ITER):
    """One K-Means run from the given centres: (labels, inertia, centres, iterations)."""
    backend.begin(centres)
    strict = False
    inertia = float("nan")
    it = 0
    for it in range(1, max_iter + 1):
        backend.assign()
        shift2, inertia, changed, n_empty = backend.update()
        if n_empty:
            shift2 = backend.relocate()
        backend.swap()
        if changed == 0:
            # same labels -> the same means: the inertia above is already that
            # of the final centres
            strict = True
            break
        if shift2 <= tol:
            break
    if not strict:
        backend.assign()
        inertia = backend.update()[1]  # labels and inertia against the final centres; no swap
    return backend.labels(), inertia, backend.centres(), it


def kmeans_fit(X: np.ndarray, k: int, n_init: int = 10, seed: int = 42, device: str = "cuda",
               max_iter: int = MAX_ITER, tol: float = TOL):
    """(labels int32 [N], inertia, centres [k][d]) of KMeans(n_clusters=k, n_init, random_state=seed)."""
    from sklearn.cluster import kmeans_plusplus

    X = _float_matrix(X)
    if device == "cuda":
        X = X.astype(np.float32, copy=False)
    if not 2 <= int(k) <= 64:
        raise ValueError(f"ssip.analytics: k = {k} outside 2..64")
    if X.shape[0] < k:
        raise ValueError(f"ssip.analytics: n_samples={X.shape[0]} should be >= n_clusters={k}")
    mean = X.mean(axis=0)
    Xc = X - mean
    tol_abs = float(np.mean(np.var(Xc, axis=0)) * tol)
    rs = np.random.RandomState(seed)
    backend = make_backend(Xc, device)
    best = None
    for _ in range(int(n_init)):
        init, _ = kmeans_plusplus(Xc, int(k), random_state=rs)
        labels, inertia, centres, _ = lloyd(backend, init, tol_abs, max_iter)
        if best is None or (inertia < best[1] and not _same_clustering(labels, best[0], int(k))):
            best = (labels, inertia, centres)
    labels, inertia, centres = best
    return labels.astype(np.int32), float(inertia), centres + mean


def dbscan_stream(backend, eps: float, min_samples_values):
    """DBSCAN labels without a stored eps graph: (one int64 label array per
    min_samples value, the walks each of them took).

    Per chunk of up to ``DBSCAN_STREAM_MAX_M`` values, which share every tile
    of distances: a core row starts as its own label; a walk gives every row
    the smallest label among the core points within eps; the hook lowers every
    core row and the row its label names to that minimum and then jumps every
    core row to the label of its label, so a component collapses onto its
    lowest core index in O(log) rounds, not O(diameter).  The walk that changes
    nothing already holds, for every row, core or border, the lowest core index
    of the smallest-numbered cluster it touches (N = noise); ranking those
    roots numbers the clusters by their lowest core index.  The same labels as
    ``dbscan_labels_from_graph`` on the same backend's eps graph."""
    n = backend.n
    if n > DBSCAN_STREAM_MAX_N:
        raise ValueError(f"ssip.analytics: DBSCAN supports N <= {DBSCAN_STREAM_MAX_N} (got {n})")
    values = [int(v) for v in min_samples_values]
    degree = backend.degree(float(eps))
    labels, walks = [], []
    for c in range(0, len(values), DBSCAN_STREAM_MAX_M):
        chunk = values[c:c + DBSCAN_STREAM_MAX_M]
        backend.dbscan_begin(chunk)
        settled = [0] * len(chunk)  # the first walk after which a configuration did not change
        for walk in range(1, DBSCAN_MAX_WALKS + 1):
            backend.dbscan_walk()
            changed = backend.dbscan_hook()
            for m in range(len(chunk)):
                if not changed[m] and not settled[m]:
                    settled[m] = walk
            if not np.any(changed):
                break
        else:
            raise RuntimeError(f"ssip.analytics: DBSCAN labels still changing after {DBSCAN_MAX_WALKS} walks "
                               f"(N = {n}, eps = {eps}, min_samples = {chunk})")
        final, nbr_min = backend.dbscan_state()
        for m, ms in enumerate(chunk):
            roots = np.unique(final[m][degree >= ms])
            near = np.asarray(nbr_min[m], dtype=np.int64)
            labels.append(np.where(near < n, np.searchsorted(roots, near), -1).astype(np.int64))
        walks += settled
    return labels, walks


def dbscan_sweep(backend, eps: float, min_samples_values) -> list:
    """DBSCAN labels at one eps for every min_samples value (a list of int64
    arrays).  Up to ``EPS_MAX_N`` points: the eps graph once, labelled per
    value on the host.  Above it: ``dbscan_stream``."""
    if backend.n > DBSCAN_STREAM_MAX_N:
        raise ValueError(f"ssip.analytics: DBSCAN supports N <= {DBSCAN_STREAM_MAX_N} (got {backend.n})")
    if backend.n <= EPS_MAX_N:
        degree, bitmap = backend.eps_graph(float(eps))
        return [dbscan_labels_from_graph(degree, bitmap, int(ms)) for ms in min_samples_values]
    return dbscan_stream(backend, float(eps), min_samples_values)[0]


def dbscan(X: np.ndarray, eps: float, min_samples: int, device: str = "cuda", backend=None) -> np.ndarray:
    """Labels of sklearn.cluster.DBSCAN(eps, min_samples).fit_predict(X)."""
    backend = backend if backend is not None else make_backend(X, device)
    return dbscan_sweep(backend, float(eps), [int(min_samples)])[0]


def silhouette(X: np.ndarray, labels: np.ndarray, device: str = "cuda", backend=None) -> float:
    """sklearn.metrics.silhouette_score(X, labels) (a -1 noise label is a cluster
    of its own); NaN for fewer than 2 distinct labels or as many labels as points."""
    labels = np.asarray(labels)
    n = labels.shape[0]
    uniq, enc = np.unique(labels, return_inverse=True)
    k = uniq.size
    if k < 2 or k >= n:
        return float("nan")
    backend = backend if backend is not None else make_backend(X, device)
    enc = enc.astype(np.int32)
    order = np.argsort(enc, kind="stable").astype(np.int32)
    sums = np.asarray(backend.cluster_sums(enc, order, k), dtype=np.float64)
    counts = np.bincount(enc, minlength=k).astype(np.float64)
    rows = np.arange(n)
    own = counts[enc]
    with np.errstate(divide="ignore", invalid="ignore"):
        a = sums[rows, enc] / (own - 1.0)
        other = sums / counts[None, :]
        other[rows, enc] = np.inf
        b = other.min(axis=1)
        s = (b - a) / np.maximum(a, b)
    s[own == 1] = 0.0
    return float(np.mean(np.nan_to_num(s)))


def kth_neighbor_distance(X: np.ndarray, k: int, device: str = "cuda", backend=None) -> np.ndarray:
    """NearestNeighbors(n_neighbors=k).fit(X).kneighbors(X)[0][:, -1] (self at distance 0)."""
    n = np.asarray(X).shape[0]
    if not 1 <= int(k) <= KTH_MAX:
        raise ValueError(f"ssip.analytics: k = {k} outside 1..{KTH_MAX}")
    if int(k) > n:
        raise ValueError(f"ssip.analytics: Expected n_neighbors <= n_samples, but n_neighbors = {k}, n_samples = {n}")
    backend = backend if backend is not None else make_backend(X, device)
    return backend.kth(int(k))


def tsne_init(X: np.ndarray, seed: int) -> np.ndarray:
    """sklearn's init="pca": the first two randomized-PCA components as
    float32, scaled so that the first has standard deviation 1e-4."""
    from sklearn.decomposition import PCA

    emb = PCA(n_components=2, svd_solver="randomized", random_state=seed).fit_transform(X).astype(np.float32,
                                                                                                  copy=False)
    return emb / np.std(emb[:, 0]) * 1e-4


def tsne_fit(X: np.ndarray, perplexity: float, seed: int = 42, max_iter: int = 1000, device: str = "cuda",
             backend=None):
    """(embedding float32 [N][2], kl_divergence, n_iter) of exact t-SNE under
    sklearn's schedule (``_t_sne.py``: ``TSNE._tsne`` and ``_gradient_descent``):
    PCA init, learning rate max(N / 48, 50), early exaggeration 12 with
    momentum 0.5 up to iteration 250 and then 1 / 0.8, ``update`` and ``gains``
    reset at the start of each phase, the error taken on every 50th iteration
    and on the last of a phase, a stop when it has not improved for more than
    300 iterations (250 in the first phase) or when the norm of the gained
    gradient is <= 1e-7.  A stop in the first phase starts the second one, as
    in sklearn.  ``kl_divergence`` is that of the unexaggerated P at the last
    iterate the gradient was taken at; ``n_iter`` counts the steps taken.

    The scalars are read back on the error iterations only; nothing else
    synchronises host and device inside the loop."""
    X = _float_matrix(X)
    n = X.shape[0]
    if not 2 <= n <= TSNE_MAX_N:
        raise ValueError(f"ssip.analytics: exact t-SNE supports 2 <= N <= {TSNE_MAX_N} (got {n}): P is N^2 floats")
    if not 0.0 < float(perplexity) < n:
        raise ValueError(f"ssip.analytics: perplexity {perplexity} must be positive and less than n_samples = {n}")
    backend = backend if backend is not None else make_backend(X, device)
    learning_rate = max(n / TSNE_EARLY_EXAGGERATION / 4.0, 50.0)
    backend.tsne_cond_p(float(perplexity))
    backend.tsne_joint_p()
    backend.tsne_begin(tsne_init(X, seed))

    max_iter = int(max_iter)
    phases = ((min(TSNE_EXPLORATION_ITERS, max_iter), TSNE_EARLY_EXAGGERATION, 0.5, TSNE_EXPLORATION_ITERS),
              (max_iter, 1.0, 0.8, MAX_ITER))
    start, last, kl = 0, -1, float("nan")
    for end, exaggeration, momentum, patience in phases:
        if start >= end:
            continue
        backend.tsne_reset()
        best_err, best_it = np.finfo(float).max, start
        for i in range(start, end):
            check = (i + 1) % TSNE_CHECK_EVERY == 0
            want_err = check or i == end - 1
            backend.tsne_grad(want_err)
            backend.tsne_step(exaggeration, momentum, learning_rate)
            last = i
            if not want_err:
                continue
            _, kl, _, gained_norm = backend.tsne_scalars()
            if not check:
                continue
            err = exaggeration * (kl + np.log(exaggeration))  # the KL of exaggeration * P, as sklearn tracks it
            if err < best_err:
                best_err, best_it = err, i
            elif i - best_it > patience:
                break
            if gained_norm <= TSNE_MIN_GRAD_NORM:
                break
        start = last + 1
    return backend.tsne_embedding().astype(np.float32), float(kl), last + 1


# ---------------------------------------------------------------------------
# native UMAP: host pieces shared by both backends
# ---------------------------------------------------------------------------
def _check_k(k: int, n: int) -> int:
    k = int(k)
    if not 2 <= k <= min(KNN_MAX_K, n):
        raise ValueError(f"ssip.analytics: k = {k} outside 2..min({KNN_MAX_K}, N = {n})")
    if n > UMAP_MAX_N:
        raise ValueError(f"ssip.analytics: N = {n} above {UMAP_MAX_N}")
    return k


def _check_knn(d2, idx, n: int):
    d2, idx = np.asarray(d2), np.asarray(idx)
    if d2.shape != idx.shape or d2.ndim != 2 or d2.shape[0] != n or not 2 <= d2.shape[1] <= min(KNN_MAX_K, n):
        raise ValueError(f"ssip.analytics: a kNN result is (d2 [N][k], idx [N][k]) with 2 <= k <= min({KNN_MAX_K}, N); "
                         f"got {d2.shape} and {idx.shape} for N = {n}")
    if idx.size and (idx.min() < 0 or idx.max() >= n):
        raise ValueError("ssip.analytics: kNN index outside 0..N-1")
    return d2, idx


def _check_csr(csr, n: int):
    """(row_ptr int32 [N+1], col int32 [E], eps float32 [E]) of a layout graph,
    validated before a kernel walks it."""
    row_ptr, col, eps = (np.asarray(v) for v in csr)
    row_ptr = row_ptr.astype(np.int64)
    if row_ptr.shape != (n + 1,) or row_ptr[0] != 0 or np.any(np.diff(row_ptr) < 0):
        raise ValueError("ssip.analytics: row_ptr must be [N + 1], start at 0 and not decrease")
    e = int(row_ptr[-1])
    if col.shape != (e,) or eps.shape != (e,) or e >= 2 ** 31:
        raise ValueError(f"ssip.analytics: col and eps must hold row_ptr[-1] = {e} edges")
    if e and (col.min() < 0 or col.max() >= n):
        raise ValueError("ssip.analytics: edge endpoint outside 0..N-1")
    eps = eps.astype(np.float32)
    if e and not (np.all(np.isfinite(eps)) and eps.min() >= 1.0):
        raise ValueError("ssip.analytics: epochs_per_sample must be finite and >= 1 (it is max w / w)")
    return row_ptr.astype(np.int32), col.astype(np.int32), eps


def umap_hash(seed, n, e, p) -> np.ndarray:
    """ssip_umap_hash of include/ssip.h with numpy integers (uint64 holding 32-bit values)."""
    m32 = np.uint64(0xFFFFFFFF)

    def u(v):
        return np.asarray(v).astype(np.uint64) & m32

    def mix(x):
        x = x ^ (x >> np.uint64(16))
        x = (x * np.uint64(0x7FEB352D)) & m32
        x = x ^ (x >> np.uint64(15))
        x = (x * np.uint64(0x846CA68B)) & m32
        return x ^ (x >> np.uint64(16))

    h = mix(((u(seed) * np.uint64(0x9E3779B1)) + u(n)) & m32)
    h = mix(h ^ u(e))
    return mix((h + ((u(p) * np.uint64(0x85EBCA77)) & m32)) & m32)


def _scatter2(rows: np.ndarray, vals: np.ndarray, n: int) -> np.ndarray:
    return np.stack([np.bincount(rows, weights=vals[:, c], minlength=n) for c in range(2)], axis=1)


def _umap_attraction(diff: np.ndarray, a: float, b: float) -> np.ndarray:
    d2 = (diff * diff).sum(axis=1)
    ok = d2 > 0.0
    safe = np.where(ok, d2, 1.0)
    c = np.where(ok, -2.0 * a * b * safe ** (b - 1.0) / (a * safe ** b + 1.0), 0.0)
    return np.clip(c[:, None] * diff, -4.0, 4.0)


def _umap_repulsion(diff: np.ndarray, a: float, b: float, gamma: float) -> np.ndarray:
    d2 = (diff * diff).sum(axis=1)
    ok = d2 > 0.0
    safe = np.where(ok, d2, 1.0)
    c = np.where(ok, 2.0 * gamma * b / ((0.001 + safe) * (a * safe ** b + 1.0)), 0.0)
    return np.clip(c[:, None] * diff, -4.0, 4.0)


def umap_graph(idx: np.ndarray, memb: np.ndarray):
    """W = A + A^T - A o A^T (scipy CSR, float32, sorted indices, no stored
    zeros) of the directed memberships A[i][idx[i][c]] = memb[i][c].  Both
    directions of an edge hold the same bits: the sum and the product commute."""
    from scipy.sparse import csr_matrix

    n, k = idx.shape
    rows = np.repeat(np.arange(n, dtype=np.int64), k)
    A = csr_matrix((np.asarray(memb, dtype=np.float32).ravel(), (rows, np.asarray(idx, dtype=np.int64).ravel())),
                   shape=(n, n))
    A.eliminate_zeros()
    T = A.T.tocsr()
    W = (A + T - A.multiply(T)).tocsr().astype(np.float32)
    W.eliminate_zeros()
    W.sort_indices()
    return W


def find_ab_params(spread: float, min_dist: float) -> Tuple[float, float]:
    """umap-learn's find_ab_params: fit 1 / (1 + a x^(2b)) to the offset exponential."""
    from scipy.optimize import curve_fit

    def curve(x, a, b):
        return 1.0 / (1.0 + a * x ** (2 * b))

    xv = np.linspace(0, spread * 3, 300)
    yv = np.where(xv < min_dist, 1.0, np.exp(-(xv - min_dist) / spread))
    params, _ = curve_fit(curve, xv, yv)
    return float(params[0]), float(params[1])


def umap_schedule(W, n_epochs: int):
    """(row_ptr int32, col int32, epochs_per_sample float32) of the edges with
    w >= max w / n_epochs; epochs_per_sample = max w / w in float32."""
    W = W.tocsr()
    w = W.data.astype(np.float32)
    if w.size == 0:
        raise ValueError("ssip.analytics: the UMAP graph has no edges")
    wmax = np.float32(w.max())
    keep = ~(w < wmax / np.float32(n_epochs))
    rows = np.repeat(np.arange(W.shape[0]), np.diff(W.indptr))[keep]
    row_ptr = np.zeros(W.shape[0] + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=W.shape[0]), out=row_ptr[1:])
    return row_ptr.astype(np.int32), W.indices[keep].astype(np.int32), (wmax / w[keep]).astype(np.float32)


def _fix_signs(v: np.ndarray) -> np.ndarray:
    """Each column's largest-magnitude entry made positive."""
    big = v[np.abs(v).argmax(axis=0), np.arange(v.shape[1])]
    return v * np.where(big < 0.0, -1.0, 1.0)


def _pca_layout(X: np.ndarray) -> np.ndarray:
    Xc = np.asarray(X, dtype=np.float64)
    Xc = Xc - Xc.mean(axis=0)
    U, S, _ = np.linalg.svd(Xc, full_matrices=False)
    y = np.zeros((Xc.shape[0], 2))
    m = min(2, S.size)
    y[:, :m] = _fix_signs(U[:, :m] * S[:m])
    return y


def _spectral_layout(W) -> Optional[np.ndarray]:
    """The two non-trivial bottom eigenvectors of the symmetric normalised
    Laplacian, or None when the graph is not connected or ARPACK gives up."""
    from scipy.sparse import diags, identity
    from scipy.sparse.csgraph import connected_components
    from scipy.sparse.linalg import ArpackError, eigsh

    n = W.shape[0]
    k = 3
    ncv = max(2 * k + 1, int(np.sqrt(n)))
    if n <= ncv or connected_components(W, directed=False)[0] > 1:
        return None
    W64 = W.astype(np.float64)
    deg = np.asarray(W64.sum(axis=1)).ravel()
    D = diags(1.0 / np.sqrt(deg))
    L = identity(n, dtype=np.float64) - D @ W64 @ D
    try:
        vals, vecs = eigsh(L, k, which="SM", ncv=ncv, tol=1e-4, v0=np.ones(n), maxiter=n * 5)
    except ArpackError:  # ArpackNoConvergence is one
        return None
    return _fix_signs(vecs[:, np.argsort(vals)[1:3]])


def umap_init(X: np.ndarray, W, init: str, seed: int) -> Tuple[np.ndarray, str]:
    """(y0 float32 [N][2], the init that was used)."""
    if init not in UMAP_INITS:
        raise ValueError("ssip.analytics: UMAP init must be one of: " + ", ".join(UMAP_INITS))
    y, used = None, init
    if init == "spectral":
        y = _spectral_layout(W)
        if y is None:
            logging.getLogger(__name__).warning(
                "UMAP spectral init: the graph is not connected or ARPACK did not converge; using the PCA init")
            used = "pca"
    if y is None:
        y = _pca_layout(X)
    y = y + np.random.RandomState(seed).normal(scale=1e-4, size=y.shape)
    lo, span = y.min(axis=0), y.max(axis=0) - y.min(axis=0)
    return (10.0 * (y - lo) / np.where(span > 0.0, span, 1.0)).astype(np.float32), used


def knn_graph(X: np.ndarray, k: int, device: str = "cuda", backend=None) -> Tuple[np.ndarray, np.ndarray]:
    """(d2 [N][k], idx int32 [N][k]): exact k nearest neighbours of every row,
    self included, ascending, a tie to the lower index.  2 <= k <= min(64, N)."""
    backend = backend if backend is not None else make_backend(X, device)
    return backend.knn(int(k))


def umap_fit(X: np.ndarray, n_neighbors: int, min_dist: float, seed: int = 42, n_epochs: Optional[int] = None,
             init: str = "spectral", device: str = "cuda", backend=None, knn=None):
    """(embedding float32 [N][2], info) of umap-learn's algorithm under the
    defaults of ``umap.UMAP(n_components=2, metric="euclidean")``: exact kNN,
    ``smooth_knn_dist`` and the membership strengths on the backend; the fuzzy
    union, ``find_ab_params``, the edge schedule and the spectral / PCA init on
    the host; then ``n_epochs`` (500 up to 10,000 points, else 200) layout
    epochs on the backend with alpha = 1 - n / n_epochs and no read-back.

    Epochs are Jacobi-ordered and the negative samples come from a
    counter-based hash, so an embedding is reproducible bit for bit but is not
    comparable point for point with umap-learn's (sequential updates, its own
    RNG).  ``knn`` = a precomputed ``(d2, idx)`` of at least ``n_neighbors``
    columns; a backend that already holds one (``backend.knn``) is reused.
    ``info``: a, b, n_epochs, n_edges (directed, after pruning), init."""
    X = _float_matrix(X)
    n = X.shape[0]
    k = _check_k(n_neighbors, n)
    backend = backend if backend is not None else make_backend(X, device)
    if knn is not None:
        backend.set_knn(*knn)
    if backend.knn_columns() < k:
        backend.knn(k)
    _, _, memb = backend.umap_fuzzy(k)
    W = umap_graph(backend.knn_indices(k), memb)
    a, b = find_ab_params(1.0, float(min_dist))
    n_epochs = int(n_epochs) if n_epochs is not None else (500 if n <= 10000 else 200)
    if n_epochs < 1:
        raise ValueError(f"ssip.analytics: n_epochs = {n_epochs} must be >= 1")
    csr = umap_schedule(W, n_epochs)
    y0, used = umap_init(X, W, init, int(seed))
    backend.umap_begin(csr, y0, a, b, int(seed))
    for ep in range(n_epochs):
        backend.umap_epoch(ep, 1.0 - ep / n_epochs)
    info = {"a": a, "b": b, "n_epochs": n_epochs, "n_edges": int(csr[1].shape[0]), "init": used}
    return backend.umap_embedding().astype(np.float32), info

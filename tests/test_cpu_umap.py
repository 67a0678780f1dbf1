"""CPU: the native UMAP of ``ssip.analytics`` on the numpy backend, and the fp64
oracles the GPU tests (test_gpu_umap.py) share.  The oracles are written here,
scalar and slow, from umap-learn's published algorithm; they use nothing of
ssip.analytics.  The whole-fit quality conditions compare against the
sequential restatement recorded in tests/golden/umap_sequential_oracle.npz
(tests/golden/make_umap_goldens.py)."""
import functools
import json
import math
import re
from pathlib import Path

import numpy as np
import pytest

from ssip import analytics as A

GOLD = Path(__file__).resolve().parent / "golden"
HEADER = Path(__file__).resolve().parents[1] / "include" / "ssip.h"
AB = {0.1: (1.57694, 0.89506), 0.0: (1.93281, 0.79049)}  # find_ab_params(spread 1) at min_dist 0.1 / 0.0
QUALITY_MARGIN = 0.02  # the project's fixed trustworthiness margin (test_gpu_tsne.py)


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
def six_blobs(n, d):
    """Six Gaussian blobs, centres x 1.5, default_rng(1)."""
    rng = np.random.default_rng(1)
    cent = rng.standard_normal((6, d)) * 1.5
    return (cent[rng.integers(0, 6, n)] + rng.standard_normal((n, d))).astype(np.float32)


def knn_input(name):
    from test_cpu_tsne import blobs

    if name == "duplicates":
        dup = blobs(65, 8).copy()
        dup[33:] = dup[:32]  # every point but one has a twin at distance 0
        return dup
    if name == "all_duplicates":
        x = blobs(65, 8).copy()
        x[:20] = x[0]  # rows 0..19 coincide: at k <= 20 their whole neighbourhood is at distance 0
        return x
    if name == "scaled":
        return blobs(65, 8) * np.float32(100.0)
    n, d = (int(v[1:]) for v in name.split("_"))
    return blobs(n, d)


# ---------------------------------------------------------------------------
# the oracles
# ---------------------------------------------------------------------------
def oracle_d2(x):
    x = np.asarray(x, dtype=np.float64)
    out = np.empty((x.shape[0], x.shape[0]))
    for s in range(0, x.shape[0], 128):
        out[s:s + 128] = ((x[s:s + 128, None, :] - x[None, :, :]) ** 2).sum(-1)
    return out


def oracle_knn(x, k):
    """(d2 fp64 [N][k], idx [N][k], the full d2): stable argsort, so a tie goes to the lower index."""
    d2 = oracle_d2(x)
    idx = np.argsort(d2, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(d2, idx, axis=1), idx, d2


def oracle_smooth_knn(dist, idx):
    """(rho, sigma, memberships) of umap-learn's smooth_knn_dist (local
    connectivity 1, bandwidth 1, 64 steps, tolerance 1e-5, the 1e-3 floors) and
    compute_membership_strengths, one row at a time."""
    dist = np.asarray(dist, dtype=np.float64)
    n, k = dist.shape
    target = math.log2(k)
    mean_all = float(dist.mean())
    rho, sigma, memb = np.zeros(n), np.zeros(n), np.zeros((n, k))
    for i in range(n):
        row = dist[i]
        nz = row[row > 0.0]
        rho[i] = nz.min() if nz.size else 0.0
        dd = row[1:] - rho[i]
        lo, hi, mid = 0.0, math.inf, 1.0
        for _ in range(64):
            psum = float(np.where(dd > 0.0, np.exp(-np.maximum(dd, 0.0) / mid), 1.0).sum())
            if abs(psum - target) < 1e-5:
                break
            if psum > target:
                hi = mid
                mid = (lo + hi) / 2.0
            else:
                lo = mid
                mid = mid * 2.0 if hi == math.inf else (lo + hi) / 2.0
        sigma[i] = max(mid, 1e-3 * (float(row.mean()) if rho[i] > 0.0 else mean_all))
        for c in range(k):
            d = row[c] - rho[i]
            memb[i, c] = 0.0 if idx[i, c] == i else (1.0 if d <= 0.0 or sigma[i] == 0.0 else math.exp(-d / sigma[i]))
    return rho, sigma, memb


def oracle_hash(seed, n, e, p):
    """ssip_umap_hash of include/ssip.h with Python integers."""
    m = 0xFFFFFFFF

    def mix(x):
        x ^= x >> 16
        x = (x * 0x7FEB352D) & m
        x ^= x >> 15
        x = (x * 0x846CA68B) & m
        return x ^ (x >> 16)

    h = mix(((seed & m) * 0x9E3779B1 + n) & m)
    h = mix(h ^ (e & m))
    return mix((h + p * 0x85EBCA77) & m)


def schedule_step(n, eps, epn, next_sample, next_neg):
    """The float32 restatement of one epoch's schedule, in place: which edges
    fire and how many negatives each draws."""
    nf = np.float32(n)
    fire = next_sample <= nf
    n_neg = np.zeros(eps.shape[0], dtype=np.int64)
    next_sample[fire] = next_sample[fire] + eps[fire]
    n_neg[fire] = ((nf - next_neg[fire]) / epn[fire]).astype(np.int32)
    next_neg[fire] = next_neg[fire] + n_neg[fire].astype(np.float32) * epn[fire]
    assert n_neg.min() >= 0
    return fire, n_neg


def oracle_epoch(csr, y, next_sample, next_neg, n, alpha, a, b, seed, gamma=1.0):
    """One Jacobi epoch, a Python loop over the edges with fp64 forces on the
    float32 positions y: (y_new fp64, fired bool [E]); the state advances in place."""
    row_ptr, col, eps = csr
    epn = eps / np.float32(5)
    fire, n_neg = schedule_step(n, eps, epn, next_sample, next_neg)
    N = row_ptr.shape[0] - 1
    y = np.asarray(y, dtype=np.float64)
    out = y.copy()

    def clip(v):
        return np.clip(v, -4.0, 4.0)

    for i in range(N):
        total = np.zeros(2)
        for e in range(row_ptr[i], row_ptr[i + 1]):
            if not fire[e]:
                continue
            diff = y[i] - y[col[e]]
            d2 = float(diff @ diff)
            if d2 > 0.0:
                total += 2.0 * clip(-2.0 * a * b * d2 ** (b - 1.0) / (a * d2 ** b + 1.0) * diff)
            for p in range(int(n_neg[e])):
                k = oracle_hash(seed, n, e, p) % N
                if k == i:
                    continue
                diff = y[i] - y[k]
                d2 = float(diff @ diff)
                if d2 > 0.0:
                    total += clip(2.0 * gamma * b / ((0.001 + d2) * (a * d2 ** b + 1.0)) * diff)
        out[i] = y[i] + alpha * total
    return out, fire


@functools.lru_cache(maxsize=None)
def epoch_case(n):
    """A hand-built symmetric CSR graph on n vertices and a layout in [0, 10]^2:
    vertex 0 is everyone's neighbour (a row of n - 1 edges), a ring and a few
    random chords besides; the ring edge (1, 2) has w = max (eps 1: five or six
    negatives every epoch), the others fire once in 1..50 epochs; vertices 1
    and 2 coincide, and so do 3 and the hub.  (row_ptr, col, eps), y0."""
    rng = np.random.default_rng(100 + n)
    pairs = {(0, j) for j in range(1, n)} | {(j, j % (n - 1) + 1) for j in range(1, n)}
    pairs |= {tuple(sorted(rng.choice(n, 2, replace=False).tolist())) for _ in range(2 * n)}
    pairs = sorted({(min(p), max(p)) for p in pairs if p[0] != p[1]})
    w = {p: np.float32(rng.uniform(0.02, 1.0)) for p in pairs}
    w[(1, 2)] = np.float32(1.0)
    dense = {}
    for (i, j), v in w.items():
        dense[(i, j)] = dense[(j, i)] = v
    keys = sorted(dense)
    rows = np.array([k[0] for k in keys])
    col = np.array([k[1] for k in keys], dtype=np.int32)
    wv = np.array([dense[k] for k in keys], dtype=np.float32)
    row_ptr = np.zeros(n + 1, dtype=np.int32)
    row_ptr[1:] = np.cumsum(np.bincount(rows, minlength=n))
    eps = (np.float32(1.0) / wv).astype(np.float32)
    y0 = rng.uniform(0.0, 10.0, size=(n, 2)).astype(np.float32)
    y0[2] = y0[1]
    if n > 3:
        y0[3] = y0[0]
    for arr in (row_ptr, col, eps, y0):
        arr.setflags(write=False)
    return (row_ptr, col, eps), y0


def state_at(csr, n):
    """The schedule state before epoch n, from the float32 restatement."""
    eps = csr[2]
    epn = eps / np.float32(5)
    ns, nn = eps.copy(), epn.copy()
    for ep in range(n):
        schedule_step(ep, eps, epn, ns, nn)
    return ns, nn


def rel(got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref).max() / np.abs(ref).max())


@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(GOLD / "umap_sequential_oracle.npz")
    return {k: z[k] for k in z.files}


def golden_inputs():
    from test_cpu_tsne import blobs

    g = golden()
    assert list(g["names"]) == ["six_blobs", "tsne_blobs"] and list(g["n_neighbors"]) == [15, 30]
    return (("six_blobs", six_blobs(300, 50), 15), ("tsne_blobs", blobs(300, 50), 30))


def check_quality(q, x, emb):
    """The whole-fit conditions: finite, trustworthiness strictly above pca_2d's
    and no more than the margin below the lowest of the sequential oracle's
    three seeds (the margin is the larger of 0.02 and the oracle's own seed spread)."""
    from sklearn.manifold import trustworthiness

    g = golden()
    seq = g["trustworthiness"][q]
    margin = max(QUALITY_MARGIN, float(seq.max() - seq.min()))
    t = trustworthiness(x, emb, n_neighbors=int(g["trust_neighbors"]))
    print(f"MEASURED quality {g['names'][q]}: trustworthiness {t:.4f}; sequential oracle {seq.min():.4f}..{seq.max():.4f}; "
          f"pca_2d {g['trustworthiness_pca_2d'][q]:.4f}; margin {margin:.4f}")
    assert emb.shape == (x.shape[0], 2) and emb.dtype == np.float32 and np.isfinite(emb).all()
    assert t > g["trustworthiness_pca_2d"][q]
    assert t >= seq.min() - margin
    return t


# ---------------------------------------------------------------------------
# the numpy backend
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name, k", (("n5_d2", 2), ("n5_d2", 5), ("n65_d50", 15), ("n65_d50", 64), ("n257_d2", 64),
                                     ("duplicates", 15)))
def test_knn_is_the_stable_argsort(name, k):
    x = knn_input(name)
    want_d2, want_idx, _ = oracle_knn(x, k)
    d2, idx = A.knn_graph(x, k, device="cpu")
    assert idx.dtype == np.int32 and idx.shape == d2.shape == (x.shape[0], k)
    assert np.array_equal(idx, want_idx)
    assert rel(d2, want_d2) <= 1e-12
    if name == "duplicates":
        assert (want_d2[:, 1] == 0).sum() == 64 and (idx[:32, 0] == np.arange(32)).all()
        assert (idx[33:, 0] == np.arange(32)).all() and (idx[33:, 1] == np.arange(33, 65)).all()
    wide = A.knn_graph(x, min(64, x.shape[0]), device="cpu")
    assert np.array_equal(wide[1][:, :k], idx) and np.array_equal(wide[0][:, :k], d2)


def test_knn_rejects_what_it_cannot_do():
    x = np.zeros((5, 3), dtype=np.float32)
    for k in (1, 6, 65):
        with pytest.raises(ValueError, match="outside 2"):
            A.knn_graph(x, k, device="cpu")
    with pytest.raises(ValueError, match="outside 2"):
        A.umap_fit(x, 6, 0.1, device="cpu")
    with pytest.raises(ValueError, match="init"):
        A.umap_fit(np.random.default_rng(0).normal(size=(20, 3)), 5, 0.1, init="random", device="cpu")


@pytest.mark.parametrize("name, k", (("n5_d2", 2), ("n65_d50", 15), ("n257_d2", 64), ("duplicates", 15),
                                     ("all_duplicates", 15), ("scaled", 15)))
def test_fuzzy_is_smooth_knn_dist(name, k):
    x = knn_input(name)
    be = A.NumpyBackend(x)
    d2, idx = be.knn(k)  # held to the oracle's by test_knn_is_the_stable_argsort; rho is exact against these
    rho, sigma, memb = oracle_smooth_knn(np.sqrt(d2), idx)
    if name == "all_duplicates":
        own = idx[:20] == np.arange(20)[:, None]  # among twins the self column is wherever the index sorts
        assert (rho[:20] == 0).all() and (rho[20:] > 0).all() and (memb[:20][~own] == 1).all() and own.any()
    got_rho, got_sigma, got_memb = be.umap_fuzzy(k)
    assert np.array_equal(got_rho, rho)
    assert rel(got_sigma, sigma) <= 1e-9 and rel(got_memb, memb) <= 1e-9
    assert (got_memb[idx == np.arange(x.shape[0])[:, None]] == 0).all()
    # a slice of a wider kNN result gives the same
    be.knn(min(64, x.shape[0]))
    again = be.umap_fuzzy(k)
    assert all(np.array_equal(u, v) for u, v in zip(again, (got_rho, got_sigma, got_memb)))


def test_graph_is_symmetric_bit_for_bit():
    x = six_blobs(300, 50)
    be = A.NumpyBackend(x)
    _, idx = be.knn(15)
    memb = be.umap_fuzzy(15)[2].astype(np.float32)
    W = A.umap_graph(idx, memb)
    assert W.dtype == np.float32 and W.has_sorted_indices and (W.data != 0).all()
    assert W.toarray().tobytes() == np.ascontiguousarray(W.T.toarray()).tobytes()
    dense = np.zeros((300, 300))
    np.put_along_axis(dense, idx.astype(np.int64), memb.astype(np.float64), axis=1)
    assert np.abs(W.toarray() - (dense + dense.T - dense * dense.T)).max() <= 1e-6
    assert W.diagonal().max() == 0


@pytest.mark.parametrize("min_dist", (0.1, 0.0))
def test_ab_constants(min_dist):
    a, b = A.find_ab_params(1.0, min_dist)
    assert abs(a - AB[min_dist][0]) <= 1e-4 and abs(b - AB[min_dist][1]) <= 1e-4


def test_schedule_arrays():
    from scipy.sparse import csr_matrix

    w = np.array([[0, 1.0, 0.5, 0], [1.0, 0, 0.001, 0.25], [0.5, 0.001, 0, 0], [0, 0.25, 0, 0]], dtype=np.float32)
    row_ptr, col, eps = A.umap_schedule(csr_matrix(w), 500)  # 0.001 < 1 / 500: dropped, both directions
    assert row_ptr.tolist() == [0, 2, 4, 5, 6] and col.tolist() == [1, 2, 0, 3, 0, 1]
    assert eps.dtype == np.float32 and eps.tolist() == [1.0, 2.0, 1.0, 4.0, 2.0, 4.0]
    assert A.umap_schedule(csr_matrix(w), 2000)[1].shape == (8,)

    class Recorder(A.NumpyBackend):
        def umap_epoch(self, n, alpha):
            self.calls.append((n, alpha))

    for n, want in ((300, 500), (10000, 500), (10001, 200)):
        be = Recorder(np.random.default_rng(3).normal(size=(n, 2)).astype(np.float32))
        be.calls = []
        if n > 300:  # the schedule is a function of N alone: a ring graph stands in for the kNN result
            idx = (np.arange(n)[:, None] + np.arange(3)[None, :]) % n
            be.set_knn(np.tile(np.array([0.0, 1.0, 4.0]), (n, 1)), idx)
        _, info = A.umap_fit(be.X, 3 if n > 300 else 5, 0.1, init="pca", backend=be)
        assert info["n_epochs"] == want == len(be.calls)
        assert be.calls[0] == (0, 1.0) and be.calls[-1] == (want - 1, 1.0 - (want - 1) / want)
        ns, nn = be.umap_state()
        assert ns.dtype == nn.dtype == np.float32 and np.array_equal(ns, be._u_eps)
        assert np.array_equal(nn, be._u_eps / np.float32(5)) and ns.min() == 1.0 and ns.shape[0] == info["n_edges"]


def test_hash_is_the_header_formula():
    text = HEADER.read_text()
    body = text[text.index("ssip_umap_mix(uint32_t x)"):text.index("Epoch n of umap-learn")]
    for token in ("0x7feb352du", "0x846ca68bu", "0x9e3779b1u", "0x85ebca77u", "x >> 16", "x >> 15", "h ^ e"):
        assert token in body, token
    assert re.search(r"ssip_umap_mix\(seed \* 0x9e3779b1u \+ n\)", body)
    rng = np.random.default_rng(5)
    table = [(0, 0, 0, 0), (42, 499, 2 ** 27, 5), (2 ** 32 - 1, 2 ** 24 - 1, 2 ** 31 - 1, 65535), (1, 0, 0, 0),
             (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1)]
    table += [tuple(int(v) for v in rng.integers(0, 2 ** 32, 4)) for _ in range(200)]
    want = [oracle_hash(*row) for row in table]
    assert len(set(want[:7])) == 7
    cols = np.array(table, dtype=np.uint64).T
    assert A.umap_hash(*cols).tolist() == want
    assert int(A.umap_hash(42, 7, np.array([3]), 2)[0]) == oracle_hash(42, 7, 3, 2)
    draws = A.umap_hash(42, 7, np.arange(20000), 0) % np.uint64(10)
    assert np.bincount(draws.astype(np.int64), minlength=10).min() > 1800  # spread over the vertices


@pytest.mark.parametrize("n, start", ((5, 0), (65, 0), (257, 0), (257, 100)))
def test_epochs_follow_the_edge_loop(n, start):
    csr, y0 = epoch_case(n)
    a, b = AB[0.1]
    ns, nn = state_at(csr, start)
    be = A.NumpyBackend(np.zeros((n, 1), dtype=np.float32))
    be.umap_begin(csr, y0, a, b, 42, state=(ns, nn))
    y = y0
    fired_any = np.zeros(csr[1].shape[0], dtype=bool)
    for ep in range(start, start + (3 if n == 257 else 5)):
        alpha = 1.0 - ep / 500
        want, fire = oracle_epoch(csr, y, ns, nn, ep, alpha, float(np.float32(a)), float(np.float32(b)), 42)
        fired_any |= fire
        be.umap_epoch(ep, alpha)
        got = be.umap_embedding()
        assert got.dtype == np.float32
        state = be.umap_state()
        assert state[0].tobytes() == ns.tobytes() and state[1].tobytes() == nn.tobytes()
        assert rel(got, want) <= 2e-7  # one float32 rounding of the fp64 result
        y = got
    assert fired_any.any() and (n == 5 or not fired_any.all())  # some edges wait tens of epochs
    if n == 257:
        assert np.diff(csr[0]).max() == 256  # the hub row


def test_whole_fit_quality_and_rerun():
    for q, (name, x, k) in enumerate(golden_inputs()):
        emb, info = A.umap_fit(x, k, 0.1, seed=0, init="pca", device="cpu")
        assert info["init"] == "pca" and info["n_epochs"] == 500 and info["n_edges"] > 300
        assert abs(info["a"] - AB[0.1][0]) <= 1e-4 and abs(info["b"] - AB[0.1][1]) <= 1e-4
        check_quality(q, x, emb)
        if q == 0:
            again, _ = A.umap_fit(x, k, 0.1, seed=0, init="pca", device="cpu")
            assert again.tobytes() == emb.tobytes()
            knn = A.knn_graph(x, 64, device="cpu")
            assert A.umap_fit(x, k, 0.1, seed=0, init="pca", device="cpu", knn=knn)[0].tobytes() == emb.tobytes()
            other, _ = A.umap_fit(x, k, 0.1, seed=1, init="pca", device="cpu")
            assert other.tobytes() != emb.tobytes()


def test_spectral_init_and_its_fallback(caplog):
    name, x, k = golden_inputs()[0]
    emb, info = A.umap_fit(x, 50, 0.1, seed=0, init="spectral", device="cpu")
    assert info["init"] == "spectral"
    check_quality(0, x, emb)
    far = x.copy()
    far[:150] += 1000.0  # two components: no edge crosses
    with caplog.at_level("WARNING"):
        emb, info = A.umap_fit(far, 15, 0.1, seed=0, n_epochs=5, device="cpu")
    assert info["init"] == "pca" and caplog.text.count("using the PCA init") == 1 and np.isfinite(emb).all()


def test_entry_points_reject_bad_arguments():
    """An argument error, not a fault: checked before any launch, so it needs no device."""
    from ssip import _lib

    lib = _lib.lib()
    assert lib.ssip_umap_workspace_bytes(1506) >= 8 * 1507 and lib.ssip_umap_workspace_bytes(1 << 20) > 0
    for n in (1, 0, -5, (1 << 20) + 1):
        assert lib.ssip_umap_workspace_bytes(n) == -1
        assert b"outside 2.." in lib.ssip_last_error()
        assert lib.ssip_knn(n, 8, 2, 16, 16, 16, None) == -1
        assert lib.ssip_umap_fuzzy(n, 2, 2, 16, 16, 16, 16, 16, 16, 1 << 30, None) == -1
        assert lib.ssip_umap_epoch(n, 16, 16, 16, 16, 16, 16, 16, 32, 1.5, 0.9, 1.0, 1.0, 0, 42, None) == -1
    for k in (1, 65, 301):
        assert lib.ssip_knn(300, 8, k, 16, 16, 16, None) == -1
    assert lib.ssip_knn(300, 513, 15, 16, 16, 16, None) == -1
    assert lib.ssip_umap_fuzzy(300, 15, 14, 16, 16, 16, 16, 16, 16, 1 << 30, None) == -1
    need = lib.ssip_umap_workspace_bytes(300)
    assert lib.ssip_umap_fuzzy(300, 15, 15, 16, 16, 16, 16, 16, 16, need - 1, None) == -3  # SSIP_ERR_WORKSPACE
    assert lib.ssip_umap_epoch(300, 16, 16, 16, 16, 16, 16, 16, 16, 1.5, 0.9, 1.0, 1.0, 0, 42, None) == -1
    assert b"alias" in lib.ssip_last_error()


# ---------------------------------------------------------------------------
# the CLI
# ---------------------------------------------------------------------------
UMAP_GRID = ("umap_nn5_md0.00", "umap_nn5_md0.10", "umap_nn15_md0.00", "umap_nn15_md0.10")


def run_cli(root, device, method, tag, neighbors=("5", "15")):
    """src.clustering on the golden bundle with the golden's grids, no t-SNE, and --umap-method; the output root."""
    from src import clustering as C
    from test_cpu_analytics import load_gold

    gold, z = load_gold()
    npz = root / "standardized_features.npz"
    np.savez_compressed(npz, **{k: z[k] for k in z.files if k != "cluster_space"})
    out = root / tag
    argv = ["--features-npz", str(npz), "--output-root", str(out), "--device", device, "--log-level", "WARNING",
            "--kmeans-range", *map(str, gold["kmeans_range"]), "--kmeans-n-init", str(gold["kmeans_n_init"]),
            "--tsne-perplexities", "--umap-neighbors", *neighbors, "--umap-min-dist", "0.0", "0.1",
            "--dbscan-eps", *(repr(e) for e in gold["dbscan_eps"]),
            "--dbscan-min-samples", *map(str, gold["dbscan_min_samples"]), "--seed", str(gold["seed"])]
    if method is not None:
        argv += ["--umap-method", method]
    C.main(argv)
    return out


def check_umap_artefacts(out, n):
    import pandas as pd

    emb_dir = out / "features" / "dimensionality_reduction"
    assert sorted(p.name for p in emb_dir.iterdir()) == sorted(
        ["pca_2d.npz", "pca_cluster.npz", "pca_tsne_init.npz"] + [f"{name}.npz" for name in UMAP_GRID])
    embs = {}
    for name in UMAP_GRID:
        z = np.load(emb_dir / f"{name}.npz")
        nn, md = re.fullmatch(r"umap_nn(\d+)_md([\d.]+)", name).groups()
        assert sorted(z.files) == ["embedding", "params_json"]
        assert z["embedding"].shape == (n, 2) and np.isfinite(z["embedding"]).all()
        assert json.loads(str(z["params_json"])) == {"n_neighbors": int(nn), "min_dist": float(md), "seed": 42}
        embs[name] = z["embedding"]
    assert (out / "figures" / "umap2d_clusters.png").stat().st_size > 0
    table = pd.read_csv(out / "tables" / "cluster_assignments.csv")
    assert (table["umap_id"] == UMAP_GRID[0]).all() and table.shape[0] == n
    return embs


def test_cli_native_umap_on_the_host(tmp_path):
    from sklearn.manifold import trustworthiness

    from src import clustering as C
    from test_cpu_analytics import load_gold

    assert C.parse_args(["--features-npz", "x.npz"]).umap_method == "package"
    assert C.parse_args(["--features-npz", "x.npz", "--umap-method", "native"]).umap_method == "native"
    gold, z = load_gold()
    assert gold["seed"] == 42
    embs = check_umap_artefacts(run_cli(tmp_path, "cpu", "native", "out"), z["features"].shape[0])
    pca = C.run_pca(z["features"], gold["variance_target"], gold["tsne_dim"], gold["seed"])
    assert trustworthiness(pca.pca_tsne_init.data, embs["umap_nn15_md0.10"], n_neighbors=10) > 0.8  # not noise
    assert embs["umap_nn15_md0.10"].tobytes() != embs["umap_nn15_md0.00"].tobytes()


def test_cli_native_umap_skips_what_the_knn_cannot_hold(caplog):
    from src import clustering as C
    from test_cpu_tsne import blobs

    base = C.EmbeddingResult("pca_tsne_init", blobs(40, 4), {})
    with caplog.at_level("WARNING"):
        out = C.run_umap(base, [5, 50, 70], [0.1], 42, "native", "cpu")
    assert [o.name for o in out] == ["umap_nn5_md0.10"] and caplog.text.count("skipping n_neighbors") == 1
    assert "[50, 70]" in caplog.text and out[0].data.shape == (40, 2)
    with pytest.raises(ValueError, match="UMAP method"):
        C.run_umap(base, [5], [0.1], 42, "umap-learn", "cpu")


def test_cli_default_is_the_package_call(tmp_path, caplog, monkeypatch):
    import builtins

    import pandas as pd

    real_import = builtins.__import__

    def no_umap(name, *args, **kwargs):
        if name == "umap":
            raise ImportError("No module named 'umap'")
        return real_import(name, *args, **kwargs)

    monkeypatch.setattr(builtins, "__import__", no_umap)
    with caplog.at_level("WARNING"):
        out = run_cli(tmp_path, "cpu", None, "out")
    assert caplog.text.count("umap is not installed") == 1
    emb_dir = out / "features" / "dimensionality_reduction"
    assert sorted(p.name for p in emb_dir.iterdir()) == ["pca_2d.npz", "pca_cluster.npz", "pca_tsne_init.npz"]
    assert not (out / "figures" / "umap2d_clusters.png").exists()
    assert (pd.read_csv(out / "tables" / "cluster_assignments.csv")["umap_id"] == "pca_2d").all()

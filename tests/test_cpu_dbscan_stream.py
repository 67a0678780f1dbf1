"""CPU: DBSCAN without the adjacency bitmap (ssip.analytics.dbscan_stream on
the numpy backend) against the bitmap labeller and sklearn, the routing of
dbscan_sweep / src.clustering.evaluate_dbscan, and the argument checks of the
three C entry points (no device needed)."""
import ctypes
import functools

import numpy as np
import pytest

from ssip import _lib
from ssip import analytics as A


def _blobs(n, d):
    rng = np.random.default_rng(31 * n + d)
    return rng.normal(size=(n, d)) + 6.0 * rng.integers(0, 3, size=(n, 1))


def _eps_values(x):
    """Three quantiles of the pairwise distances, moved off the distance they fall on."""
    n = x.shape[0]
    if n == 1:
        return [1.0]
    dist = np.sqrt(((x[:, None] - x[None]) ** 2).sum(-1))[~np.eye(n, dtype=bool)]
    return [float(np.quantile(dist, q)) * 1.0005 for q in (0.05, 0.3, 0.7)]


def _bitmap_labels(backend, eps, values):
    degree, bitmap = backend.eps_graph(eps)
    return [A.dbscan_labels_from_graph(degree, bitmap, ms) for ms in values]


@pytest.mark.parametrize("n", (1, 2, 65, 300))
@pytest.mark.parametrize("d", (1, 6))
def test_stream_equals_bitmap_and_sklearn(n, d):
    from sklearn.cluster import DBSCAN

    x = _blobs(n, d)
    d2 = ((x[:, None] - x[None]) ** 2).sum(-1)
    values = [1, 2, 5, n + 1]
    for eps in _eps_values(x):
        assert (np.abs(d2 - eps * eps) > 1e-9 * eps * eps).all()  # no pair sits on the threshold
        be = A.NumpyBackend(x)
        got, walks = A.dbscan_stream(be, eps, values)
        want = _bitmap_labels(be, eps, values)
        assert len(got) == len(walks) == 4
        for ms, g, w in zip(values, got, want):
            assert g.dtype == np.int64 and np.array_equal(g, w), (n, d, eps, ms)
            assert np.array_equal(g, DBSCAN(eps=eps, min_samples=ms).fit_predict(x)), (n, d, eps, ms)
        assert np.array_equal(be.degree(eps), be.eps_graph(eps)[0])


def test_stream_equals_bitmap_on_threshold_ties():
    """Integer coordinates with eps on a distance that occurs: both paths use one predicate."""
    rng = np.random.default_rng(7)
    x = rng.integers(0, 12, size=(200, 2)).astype(np.float64)
    be = A.NumpyBackend(x)
    for eps in (1.0, 2.0, 5.0 ** 0.5):
        values = [2, 4, 9]
        got, _ = A.dbscan_stream(be, eps, values)
        for g, w in zip(got, _bitmap_labels(be, eps, values)):
            assert np.array_equal(g, w)


def test_shuffled_chain_settles_in_logarithmic_walks():
    """4096 points on a line, one unit apart, in shuffled order: one cluster.
    The bound on the walks is what rules out a propagation that moves one
    neighbour per walk (the chain's diameter is 4095)."""
    x = np.random.default_rng(0).permutation(4096).astype(np.float64)[:, None]
    labels, walks = A.dbscan_stream(A.NumpyBackend(x), 1.5, [2, 3])
    for lab in labels:  # min_samples 3 leaves the two ends as border points
        assert np.array_equal(lab, np.zeros(4096, dtype=np.int64))
    assert max(walks) <= 2 * 12
    print("MEASURED chain walks", walks)


@functools.lru_cache(maxsize=None)
def _lattice():
    c = np.random.default_rng(1).choice(10000, 4097, replace=False)
    x = np.stack([c // 100, c % 100], axis=1).astype(np.float32)
    x.setflags(write=False)
    return x


def test_lattice_equals_sklearn():
    from sklearn.cluster import DBSCAN

    x = _lattice()
    (labels,), (walks,) = A.dbscan_stream(A.NumpyBackend(x), 1.5, [5])
    ref = DBSCAN(eps=1.5, min_samples=5).fit(x.astype(np.float64))
    assert np.array_equal(labels, ref.labels_)
    assert labels.max() + 1 > 100 and 0.05 < np.mean(labels == -1) < 0.5  # many clusters, some noise
    assert walks <= 2 * 13


def test_hand_built_case():
    """eps 1, min_samples 5, points on a line in eighths (exact arithmetic).
    Rows 1-5 and 6-10 are two groups of five mutual neighbours (each with a
    duplicate pair), 1.75 apart at their nearest.  Rows 0 and 12 are one
    duplicated point between them, within eps of exactly one core of each group
    and of each other: degree 4, not core.  One of them has a lower index than
    every core, the other a higher one; both take the smaller cluster id.  Row
    11 is far from everything."""
    from sklearn.cluster import DBSCAN

    low = [2.25, 2.5, 2.625, 2.75, 2.75]  # cluster 0: it holds the lowest core index
    high = [0.0, 0.0, 0.125, 0.25, 0.5]
    x = np.array([1.375] + low + high + [10.0, 1.375])[:, None]
    want = np.array([0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, -1, 0])
    be = A.NumpyBackend(x)
    degree = be.degree(1.0)
    assert degree[0] == degree[12] == 4 and degree[11] == 1 and (degree[1:11] >= 5).all()
    (labels,), _ = A.dbscan_stream(be, 1.0, [5])
    assert np.array_equal(labels, want)
    assert np.array_equal(DBSCAN(eps=1.0, min_samples=5).fit_predict(x), want)
    assert np.array_equal(_bitmap_labels(be, 1.0, [5])[0], want)


def test_two_chunks_equal_single_calls():
    x = _blobs(300, 6)
    eps = _eps_values(x)[1]
    values = [1, 2, 3, 5, 8]  # more than DBSCAN_STREAM_MAX_M: two chunks
    be = A.NumpyBackend(x)
    labels, walks = A.dbscan_stream(be, eps, values)
    assert len(labels) == len(walks) == 5
    for ms, lab, w in zip(values, labels, walks):
        (one,), (w1,) = A.dbscan_stream(A.NumpyBackend(x), eps, [ms])
        assert np.array_equal(lab, one) and w == w1, ms


def test_sweep_routes_by_row_count(monkeypatch):
    x = _blobs(300, 6)
    eps = _eps_values(x)[1]
    be = A.NumpyBackend(x)
    calls = []
    real = A.dbscan_stream
    monkeypatch.setattr(A, "dbscan_stream", lambda *a: calls.append(1) or real(*a))
    below = A.dbscan_sweep(be, eps, [2, 5])
    assert not calls  # at or below EPS_MAX_N: the bitmap path
    monkeypatch.setattr(A, "EPS_MAX_N", 100)
    above = A.dbscan_sweep(be, eps, [2, 5])
    assert calls == [1]
    for a, b in zip(below, above):
        assert np.array_equal(a, b)
    assert np.array_equal(A.dbscan(x, eps, 5, device="cpu"), below[1])
    monkeypatch.setattr(A, "DBSCAN_STREAM_MAX_N", 200)
    with pytest.raises(ValueError, match="200"):
        A.dbscan_sweep(be, eps, [2])
    with pytest.raises(ValueError, match="200"):
        real(be, eps, [2])


def test_evaluate_dbscan_is_the_same_through_either_path(monkeypatch):
    from src import clustering as C

    rng = np.random.default_rng(3)
    x = _blobs(300, 6)
    is_labeled = rng.random(300) < 0.2
    truth = np.where(is_labeled, rng.integers(0, 3, size=300).astype(str), "")
    bundle = C.FeatureBundle(x, np.arange(300).astype(str), is_labeled, truth, None, None)
    space = C.EmbeddingResult("pca_cluster", x, {})
    eps_values = _eps_values(x)[:2]
    values = [1, 2, 3, 5, 8]

    def run():
        return C.evaluate_dbscan(space, bundle, eps_values, values, 42, "all", device="cpu")

    below = run()
    monkeypatch.setattr(A, "EPS_MAX_N", 100)
    above = run()
    assert len(below) == len(above) == 10
    for a, b in zip(below, above):
        assert np.array_equal(a.labels, b.labels) and a.labels.dtype == b.labels.dtype
        assert a.params == b.params and a.noise_rate == b.noise_rate and a.space == b.space
        assert (a.ari, a.nmi) == (b.ari, b.nmi)
        assert a.silhouette == b.silhouette or (np.isnan(a.silhouette) and np.isnan(b.silhouette))


def test_walk_limit_is_an_error(monkeypatch):
    x = np.arange(64, dtype=np.float64)[:, None]
    monkeypatch.setattr(A, "DBSCAN_MAX_WALKS", 1)
    with pytest.raises(RuntimeError, match="1 walks"):
        A.dbscan_stream(A.NumpyBackend(x), 1.5, [2])


def test_a_walk_takes_one_to_four_min_samples():
    be = A.NumpyBackend(_blobs(65, 1))
    be.degree(1.0)
    for bad in ([], [1, 2, 3, 4, 5]):
        with pytest.raises(ValueError):
            be.dbscan_begin(bad)


# ---------------------------------------------------------------------------
# C ABI: argument errors need no device
# ---------------------------------------------------------------------------
def test_dbscan_argument_errors_surface_as_status_codes():
    lib = _lib.lib()
    buf = (ctypes.c_int32 * 4096)()
    p = ctypes.addressof(buf)
    q, r, s = p + 4096, p + 8192, p + 12288  # disjoint for N * M <= 1024
    cap = 1 << 20
    assert lib.ssip_pairwise_degree(cap + 1, 2, p, 1.0, q, None) == -1
    assert str(cap).encode() in lib.ssip_last_error()
    assert lib.ssip_pairwise_degree(10, 513, p, 1.0, q, None) == -1
    assert lib.ssip_pairwise_degree(10, 2, p, -1.0, q, None) == -1
    assert lib.ssip_pairwise_degree(10, 2, p, 1.0, None, None) == -1
    assert lib.ssip_dbscan_walk(cap + 1, 2, p, 1.0, 1, p, p, q, r, None) == -1
    assert lib.ssip_dbscan_walk(10, 2, p, 1.0, 0, p, p, q, r, None) == -1
    assert b"M = 0" in lib.ssip_last_error()
    assert lib.ssip_dbscan_walk(10, 2, p, 1.0, 5, p, p, q, r, None) == -1
    assert b"M = 5" in lib.ssip_last_error()
    assert lib.ssip_dbscan_walk(10, 513, p, 1.0, 1, p, p, q, r, None) == -1
    assert b"513" in lib.ssip_last_error()
    assert lib.ssip_dbscan_walk(10, 2, p, -0.5, 1, p, p, q, r, None) == -1
    assert lib.ssip_dbscan_walk(10, 2, p, 1.0, 1, p, p, q, None, None) == -1
    assert b"null" in lib.ssip_last_error()
    assert lib.ssip_dbscan_walk(10, 2, p, 1.0, 1, p, p, q, q, None) == -1
    assert b"alias" in lib.ssip_last_error()
    assert lib.ssip_dbscan_hook(cap + 1, 1, p, p, p, q, r, s, p, None) == -1
    assert lib.ssip_dbscan_hook(0, 1, p, p, p, q, r, s, p, None) == -1
    assert lib.ssip_dbscan_hook(10, 0, p, p, p, q, r, s, p, None) == -1
    assert lib.ssip_dbscan_hook(10, 5, p, p, p, q, r, s, p, None) == -1
    assert lib.ssip_dbscan_hook(10, 1, p, p, p, q, r, None, p, None) == -1
    assert b"null" in lib.ssip_last_error()
    assert lib.ssip_dbscan_hook(10, 1, p, p, p, q, p, s, p, None) == -1  # labels_out is labels_in
    assert b"alias" in lib.ssip_last_error()
    assert lib.ssip_dbscan_hook(10, 4, p, p, p, q, p + 80, s, p, None) == -1  # ... or overlaps it
    assert b"alias" in lib.ssip_last_error()
    for name in (b"ssip_pairwise_degree", b"ssip_dbscan_walk", b"ssip_dbscan_hook"):
        assert lib.ssip_plan_fn_index(name) >= 0  # recordable in a launch plan

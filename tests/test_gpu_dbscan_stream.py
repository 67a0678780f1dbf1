"""GPU: DBSCAN without the adjacency bitmap (ssip_pairwise_degree,
ssip_dbscan_walk, ssip_dbscan_hook under ssip.analytics.dbscan_stream).

Everything here is exact.  The walk and the degree kernel go through the
column walk and the predicate of ssip_pairwise_eps, so their pair set is the
bitmap's bit for bit and the stream labels must equal the labels of the
device's own bitmap with no eps margin.  Against sklearn and the numpy backend
the inputs are integer lattices, whose squared distances are exact in fp32 and
fp64 alike."""
import functools
import logging

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NS = (1, 2, 63, 64, 65, 257, 1000)
DS = (1, 2, 33, 50, 512)


@functools.lru_cache(maxsize=None)
def _points(n, d):
    rng = np.random.default_rng(31 * n + d)
    x = (rng.normal(size=(n, d)) + 6.0 * rng.integers(0, 3, size=(n, 1))).astype(np.float32)
    if n == 1:
        return x, (1.0,)
    from scipy.spatial.distance import pdist

    dist = pdist(x.astype(np.float64))
    return x, tuple(float(np.float32(np.quantile(dist, q))) for q in (0.05, 0.3, 0.7))


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("d", DS)
def test_stream_equals_the_bitmap_labels(dev, n, d):
    from ssip import analytics as A

    x, eps_values = _points(n, d)
    values = [1, 2, 5, n + 1]
    be = A.DeviceBackend(x)
    for eps in eps_values:
        degree, bitmap = be.eps_graph(eps)
        got = be.degree(eps)
        assert got.dtype == np.int32 and np.array_equal(got, degree), (n, d, eps)
        labels, walks = A.dbscan_stream(be, eps, values)
        for ms, lab in zip(values, labels):
            assert lab.dtype == np.int64
            assert np.array_equal(lab, A.dbscan_labels_from_graph(degree, bitmap, ms)), (n, d, eps, ms)
        assert len(walks) == 4 and min(walks) >= 1
        assert not (labels[3] != -1).any()  # min_samples N + 1: no core point


def test_four_configurations_in_one_walk_equal_four_walks(dev):
    from ssip import analytics as A

    x, eps_values = _points(1000, 50)
    values = [1, 2, 5, 9]
    for eps in eps_values:
        labels, walks = A.dbscan_stream(A.DeviceBackend(x), eps, values)
        for ms, lab, w in zip(values, labels, walks):
            (one,), (w1,) = A.dbscan_stream(A.DeviceBackend(x), eps, [ms])
            assert np.array_equal(lab, one) and w == w1, (eps, ms)
    # five values: a chunk of four and a chunk of one
    labels5, walks5 = A.dbscan_stream(A.DeviceBackend(x), eps_values[1], values + [14])
    labels4, walks4 = A.dbscan_stream(A.DeviceBackend(x), eps_values[1], values)
    assert walks5[:4] == walks4 and all(np.array_equal(a, b) for a, b in zip(labels5, labels4))
    assert np.array_equal(labels5[4], A.dbscan_stream(A.DeviceBackend(x), eps_values[1], [14])[0][0])


def _chain():
    return np.random.default_rng(0).permutation(4096).astype(np.float32)[:, None]


def _lattice(side, count):
    c = np.random.default_rng(1).choice(side * side, count, replace=False)
    return np.stack([c // side, c % side], axis=1).astype(np.float32)


def _full_state(A, x, eps, values):
    be = A.DeviceBackend(x)
    labels, walks = A.dbscan_stream(be, eps, values)
    return labels, walks, be.dbscan_state()


@pytest.mark.parametrize("name", ("chain", "lattice"))
def test_device_equals_the_numpy_backend_and_itself(dev, name):
    """Exact arithmetic on both sides: the same labels after the same number
    of walks, and two device runs agree byte for byte."""
    from ssip import analytics as A

    x, values = (_chain(), [2, 3]) if name == "chain" else (_lattice(100, 4097), [4, 5, 6])
    ref_labels, ref_walks = A.dbscan_stream(A.NumpyBackend(x), 1.5, values)
    labels, walks, state = _full_state(A, x, 1.5, values)
    assert walks == ref_walks
    assert max(walks) <= 2 * (x.shape[0] - 1).bit_length()
    for a, b in zip(labels, ref_labels):
        assert np.array_equal(a, b)
    if name == "chain":
        assert all((lab == 0).all() for lab in labels)
    labels2, walks2, state2 = _full_state(A, x, 1.5, values)
    assert walks2 == walks
    for a, b in zip(list(labels) + list(state), list(labels2) + list(state2)):
        assert a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------
# above the bitmap's cap
# ---------------------------------------------------------------------------
BIG_N = 70000
BIG_CONFIGS = ((1.5, (4, 5, 6)), (1.0, (3,)))


@functools.lru_cache(maxsize=None)
def _big_points():
    return _lattice(400, BIG_N)


@functools.lru_cache(maxsize=None)
def _big_reference():
    """{(eps, min_samples): (labels, core mask)} of sklearn on the fp64 copy of the points."""
    from sklearn.cluster import DBSCAN

    x64 = _big_points().astype(np.float64)
    out = {}
    for eps, values in BIG_CONFIGS:
        for ms in values:
            fit = DBSCAN(eps=eps, min_samples=ms).fit(x64)
            core = np.zeros(BIG_N, dtype=bool)
            core[fit.core_sample_indices_] = True
            out[(eps, ms)] = (fit.labels_, core)
    return out


@functools.lru_cache(maxsize=None)
def _big_sweeps():
    """{eps: (labels per min_samples, walks)} of the device, through the
    public sweep (which must pick the stream path at this size)."""
    from ssip import analytics as A

    assert BIG_N > A.EPS_MAX_N
    be = A.DeviceBackend(_big_points())
    out = {}
    for eps, values in BIG_CONFIGS:
        labels, walks = A.dbscan_stream(be, eps, list(values))
        swept = A.dbscan_sweep(be, eps, list(values))
        assert all(np.array_equal(a, b) for a, b in zip(labels, swept))
        out[eps] = (labels, walks)
    return out


def test_70000_points_equal_sklearn(dev):
    ref = _big_reference()
    sweeps = _big_sweeps()
    for eps, values in BIG_CONFIGS:
        labels, walks = sweeps[eps]
        for ms, lab, w in zip(values, labels, walks):
            want, core = ref[(eps, ms)]
            clusters = int(want.max()) + 1
            noise = int((want == -1).sum())
            border = int(((want != -1) & ~core).sum())
            print(f"MEASURED eps {eps} min_samples {ms}: {clusters} clusters, noise {noise / BIG_N:.3f}, "
                  f"core {core.mean():.3f}, border {border}, walks {w}")
            assert clusters > 1000 and noise > 0 and border > 0  # the input is not trivial
            assert np.array_equal(lab, want), (eps, ms)
            assert w <= 2 * 17  # 2 * ceil(log2 N)


def test_bitmap_path_still_refuses_70000_points(dev):
    from ssip import analytics as A

    with pytest.raises(ValueError, match=str(A.EPS_MAX_N)):
        A.DeviceBackend(_big_points()).eps_graph(1.5)


def test_evaluate_dbscan_above_the_cap(dev, caplog):
    from src import clustering as C

    x = _big_points()
    is_labeled = np.zeros(BIG_N, dtype=bool)
    is_labeled[[5, 77, 4000, 31000, 69999]] = True
    truth = np.where(is_labeled, "a", "")
    truth[[77, 31000]] = "b"
    bundle = C.FeatureBundle(x, np.arange(BIG_N).astype(str), is_labeled, truth, None, None)
    space = C.EmbeddingResult("pca_cluster", x, {})
    eps, values = BIG_CONFIGS[0]
    with caplog.at_level(logging.WARNING):
        results = C.evaluate_dbscan(space, bundle, [eps], list(values), 42, "all", "cuda")
    assert [r.params["min_samples"] for r in results] == list(values)
    for r, lab in zip(results, _big_sweeps()[eps][0]):
        assert np.array_equal(r.labels, lab)
        assert r.noise_rate == float(np.mean(lab == -1))
        assert np.isnan(r.silhouette)
    assert "silhouette not computed" in caplog.text and "256 clusters" in caplog.text

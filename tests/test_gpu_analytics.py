"""GPU: the embedding-analytics kernels (csrc/analytics.hip) and their host
layer (ssip/analytics.py) against numpy fp64 oracles computed here.

Tolerances.  Labels, counts, degrees and bitmap words are exact; the oracle's
own decision margins (top-2 distance gap, eps gap) are asserted first.  The
floating-point outputs are held to 4x the largest relative difference measured
on an MI355X against the fp64 oracle over all cases of the test (printed by
each test as ``MEASURED <name> <value>``; run with -s to see them):

    mind2 (assign)             1.005e-06   max |d2 - ref| / max ref
    centres (update)           4.477e-07
    inertia (update)           5.093e-07
    shift (update)             4.284e-07
    kth distance               2.185e-07
    cluster sums               3.513e-07
    silhouette (absolute)      1.223e-08   over the five labelings here and the 9
                                           configurations of the end-to-end test

The margin of 4 is there because the fp32 fixed-order sums over N move with the
workgroup count; on one build the kernels are bit-reproducible.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# 4 x the measured figures of the module docstring
BOUND_MIND2 = 4 * 1.005e-6
BOUND_CENTRES = 4 * 4.477e-7
BOUND_INERTIA = 4 * 5.093e-7
BOUND_SHIFT = 4 * 4.284e-7
BOUND_KTH = 4 * 2.185e-7
BOUND_SUMS = 4 * 3.513e-7
BOUND_SILHOUETTE = 4 * 1.223e-8

NS = (1, 63, 64, 65, 257)
DS = (1, 2, 31, 33, 50, 512)
KS = (2, 10, 64)

_worst = {}


def _measure(name, value, bound):
    _worst[name] = max(_worst.get(name, 0.0), float(value))
    print(f"MEASURED {name} {value:.3e} (worst so far {_worst[name]:.3e}, bound {bound:.3e})")


def _d2(a, b):
    a = a.astype(np.float64)
    b = b.astype(np.float64)
    return ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)


def _top2_gap(d2):
    s = np.sort(d2, axis=1)
    return float(((s[:, 1] - s[:, 0]) / s[:, 1]).min())


@functools.lru_cache(maxsize=None)
def _assign_case(n, d, k):
    """Random points and centres whose fp64 top-2 distance gap is >= 1e-4 on
    every row: the first seed (from the oracle alone) for which that holds."""
    for seed in range(200):
        rng = np.random.default_rng(1000 * seed + 7 * n + 13 * d + k)
        x = rng.normal(size=(n, d)).astype(np.float32)
        c = rng.normal(size=(k, d)).astype(np.float32)
        d2 = _d2(x, c)
        if _top2_gap(d2) >= 1e-4:
            d2.setflags(write=False)
            return x, c, d2
    raise AssertionError("no seed gives a 1e-4 top-2 gap")


def _run_lloyd_step(A, x, c):
    be = A.DeviceBackend(x)
    be.begin(c)
    be.assign()
    scal = be.update()
    return be, scal


def _rel(got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    scale = max(float(np.abs(ref).max()), 1e-300)
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref).max() / scale)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("d", DS)
def test_assign_and_update_match_the_oracle(dev, n, d):
    from ssip import analytics as A

    for k in KS:
        x, c, d2 = _assign_case(n, d, k)
        assert _top2_gap(d2) >= 1e-4  # no row exempted
        ref_labels = d2.argmin(axis=1)
        ref_min = d2.min(axis=1)
        be, (shift2, inertia, changed, n_empty) = _run_lloyd_step(A, x, c)
        labels = be.labels()
        assert labels.dtype == np.int32 and np.array_equal(labels, ref_labels), (n, d, k)
        mind2 = be._mind2.cpu().numpy()
        _measure("mind2", _rel(mind2, ref_min), BOUND_MIND2)
        counts = be._counts.cpu().numpy()
        ref_counts = np.bincount(ref_labels, minlength=k)
        assert np.array_equal(counts, ref_counts)
        assert changed == n and n_empty == int((ref_counts == 0).sum())
        ref_c = c.astype(np.float64).copy()
        for j in np.flatnonzero(ref_counts):
            ref_c[j] = x[ref_labels == j].astype(np.float64).mean(axis=0)
        new_c = be.Cn.cpu().numpy()
        # an empty cluster keeps its centre, bit for bit
        assert np.array_equal(new_c[ref_counts == 0], c[ref_counts == 0])
        ref_shift = float(((ref_c - c.astype(np.float64)) ** 2).sum())
        e_c, e_i, e_s = _rel(new_c, ref_c), _rel(inertia, ref_min.sum()), _rel(shift2, ref_shift)
        _measure("centres", e_c, BOUND_CENTRES)
        _measure("inertia", e_i, BOUND_INERTIA)
        _measure("shift", e_s, BOUND_SHIFT)
        assert _rel(mind2, ref_min) <= BOUND_MIND2
        assert e_c <= BOUND_CENTRES and e_i <= BOUND_INERTIA and e_s <= BOUND_SHIFT, (n, d, k)
        # the same centres again: no label changes
        be.assign()
        assert be.update()[2] == 0


def test_assign_ties_go_to_the_lowest_centre(dev):
    from ssip import analytics as A

    rng = np.random.default_rng(5)
    # small integers: every fp32 distance is exact, so ties are exact ties
    x = rng.integers(-3, 4, size=(130, 5)).astype(np.float32)
    x[65:] = x[:65]  # duplicated points
    c = rng.integers(-3, 4, size=(10, 5)).astype(np.float32)
    c[2] = c[0]
    c[7] = c[4]
    c[9] = c[4]  # duplicated centres
    d2 = _d2(x, c)
    ref = d2.argmin(axis=1)
    assert (np.sort(d2, axis=1)[:, 0] == np.sort(d2, axis=1)[:, 1]).any()  # the case does contain ties
    be, _ = _run_lloyd_step(A, x, c)
    labels = be.labels()
    assert np.array_equal(labels, ref)
    assert not np.isin(labels, (2, 7, 9)).any()
    assert np.array_equal(labels[:65], labels[65:])
    assert np.array_equal(be._mind2.cpu().numpy().astype(np.float64), d2.min(axis=1))


def test_update_leaves_an_empty_cluster_alone(dev):
    from ssip import analytics as A

    x, c, _ = _assign_case(257, 33, 10)
    c = c.copy()
    c[3] += 1000.0  # attracts no point
    be, (_, _, _, n_empty) = _run_lloyd_step(A, x, c)
    counts = be._counts.cpu().numpy()
    assert counts[3] == 0 and n_empty == 1 and counts.sum() == 257
    assert np.array_equal(be.Cn.cpu().numpy()[3], c[3])


@functools.lru_cache(maxsize=None)
def _eps_case(n, d):
    """Three well-separated blobs and an eps in a gap of the sorted fp64
    pairwise distances (no distance within 1e-3 * eps), nearest to the 30 %
    quantile so that the graph is neither empty nor complete."""
    rng = np.random.default_rng(31 * n + d)
    x = (rng.normal(size=(n, d)) + 6.0 * rng.integers(0, 3, size=(n, 1))).astype(np.float32)
    dist = np.sqrt(_d2(x, x))
    if n == 1:
        return x, dist, 1.0
    vals = np.unique(dist)
    mid = 0.5 * (vals[1:] + vals[:-1])
    ok = (vals[1:] - mid >= 2e-3 * mid) & (mid - vals[:-1] >= 2e-3 * mid)
    assert ok.any()
    cand = mid[ok]
    eps = float(cand[np.abs(cand - np.quantile(dist, 0.3)).argmin()])
    return x, dist, eps


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("d", DS)
def test_eps_graph_is_exact(dev, n, d):
    from ssip import analytics as A

    x, dist, eps = _eps_case(n, d)
    eps = float(np.float32(eps))
    assert (np.abs(dist - eps) > 1e-3 * eps).all()  # eps sits in a distance gap
    adj = dist <= eps
    degree, bitmap = A.DeviceBackend(x).eps_graph(eps)
    assert degree.dtype == np.int32 and bitmap.dtype == np.uint32
    assert bitmap.shape == (n, (n + 31) // 32)
    assert np.array_equal(degree, adj.sum(axis=1))
    assert np.array_equal(bitmap, A.pack_adjacency(adj))  # padding bits of the last word are zero
    labels = A.dbscan_labels_from_graph(degree, bitmap, 4)
    assert np.array_equal(labels, A.dbscan_labels_from_graph(adj.sum(axis=1), adj, 4))


@pytest.mark.parametrize("n", (1, 15, 63, 64, 65, 257))
@pytest.mark.parametrize("d", (2, 50))
def test_kth_distance(dev, n, d):
    from ssip import analytics as A

    rng = np.random.default_rng(17 * n + d)
    x = rng.normal(size=(n, d)).astype(np.float32)
    x[n // 2] = x[0]  # a duplicate: two zero distances in those rows
    ref = np.sort(np.sqrt(_d2(x, x)), axis=1)
    be = A.DeviceBackend(x)
    for k in (1, 5, 15, 64):
        if k > n:
            # as NearestNeighbors(n_neighbors=k) does for k > n_samples
            with pytest.raises((RuntimeError, ValueError)):
                A.kth_neighbor_distance(x, k, backend=be)
            with pytest.raises(RuntimeError, match="neighbours asked"):
                be.kth(k)
            continue
        got = A.kth_neighbor_distance(x, k, backend=be)
        if k == 1:
            assert (got == 0).all()
        err = _rel(got, ref[:, k - 1])
        _measure("kth", err, BOUND_KTH)
        assert err <= BOUND_KTH, (n, d, k)


@pytest.mark.parametrize("n", (2, 63, 64, 65, 257))
@pytest.mark.parametrize("d", (2, 33, 50))
def test_kth_distance_and_knn_share_the_walk_and_the_selection(dev, n, d):
    """ssip_pairwise_kth and ssip_knn are two instantiations of one selection
    over one column walk (csrc/pairwise_tile.h), so the k-th distance is the
    root of column k - 1 of the kNN result bit for bit (both roots are
    correctly rounded fp32), and a k result is a prefix of the widest one."""
    from ssip import analytics as A

    rng = np.random.default_rng(23 * n + d)
    x = rng.normal(size=(n, d)).astype(np.float32)
    x[n // 2] = x[0]  # a duplicate: equal distances, ordered by index
    be = A.DeviceBackend(x)
    wide_d2, wide_idx = be.knn(min(64, n))  # knn(64) wherever the input has 64 rows
    for k in (2, 15, 64):
        if k > n:
            continue
        d2, idx = be.knn(k)
        assert d2.dtype == np.float32 and d2.shape == (n, k)
        assert be.kth(k).astype(np.float32).tobytes() == np.sqrt(d2[:, k - 1]).tobytes(), (n, d, k)
        assert np.ascontiguousarray(wide_d2[:, :k]).tobytes() == d2.tobytes(), (n, d, k)
        assert np.ascontiguousarray(wide_idx[:, :k]).tobytes() == idx.tobytes(), (n, d, k)


def _labelings():
    rng = np.random.default_rng(3)
    out = {}
    for k in (2, 7, 256):
        n = 300 if k == 256 else 257
        lab = np.concatenate([np.arange(k), rng.integers(0, k, size=n - k)])
        out[f"k{k}"] = (n, rng.permutation(lab))
    noise = rng.integers(-1, 4, size=257)
    out["noise"] = (257, noise)
    single = rng.integers(0, 3, size=257)
    single[[5, 100, 256]] = (3, 4, 5)  # three singleton clusters
    out["singletons"] = (257, single)
    return out


@pytest.mark.parametrize("name", ("k2", "k7", "k256", "noise", "singletons"))
def test_cluster_sums_and_silhouette(dev, name):
    from sklearn.metrics import silhouette_score

    from ssip import analytics as A

    n, labels = _labelings()[name]
    rng = np.random.default_rng(11)
    x = (rng.normal(size=(n, 20)) + 3.0 * (labels[:, None] % 5)).astype(np.float32)
    be = A.DeviceBackend(x)
    uniq, enc = np.unique(labels, return_inverse=True)
    order = np.argsort(enc, kind="stable")
    sums = be.cluster_sums(enc, order, uniq.size)
    dist = np.sqrt(_d2(x, x))
    ref = np.stack([dist[:, enc == c].sum(axis=1) for c in range(uniq.size)], axis=1)
    e_sums = _rel(sums, ref)
    _measure("sums", e_sums, BOUND_SUMS)
    got = A.silhouette(x, labels, backend=be)
    want = float(silhouette_score(x.astype(np.float64), labels))
    e_sil = abs(got - want)  # absolute: the score lives in [-1, 1]
    _measure("silhouette", e_sil, BOUND_SILHOUETTE)
    assert e_sums <= BOUND_SUMS and e_sil <= BOUND_SILHOUETTE
    assert np.isnan(A.silhouette(x, np.zeros(n, dtype=int), backend=be))
    assert np.isnan(A.silhouette(x, np.arange(n), backend=be))


def test_every_kernel_is_bit_reproducible(dev):
    from ssip import analytics as A

    x, c, _ = _assign_case(257, 50, 10)
    _, _, eps = _eps_case(257, 50)
    enc = (np.arange(257) * 7 % 5).astype(np.int32)
    order = np.argsort(enc, kind="stable")

    def once():
        be, scal = _run_lloyd_step(A, x, c)
        deg, bm = be.eps_graph(eps)
        return [be.labels(), be._mind2.cpu().numpy(), be.Cn.cpu().numpy(),
                be._counts.cpu().numpy(), np.array(scal), deg, bm, be.kth(15), *be.knn(15),
                be.cluster_sums(enc, order, 5)]

    a, b = once(), once()
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes()


def test_kmeans_fit_matches_sklearn_on_the_device(dev):
    """The whole replay on the device backend: sklearn's labels on separated blobs."""
    from sklearn.cluster import KMeans

    from ssip import analytics as A

    rng = np.random.default_rng(0)
    cent = rng.normal(size=(4, 8)) * 4
    x = (cent[rng.integers(0, 4, 280)] + rng.normal(size=(280, 8))).astype(np.float32)
    for k in (2, 4, 7):
        km = KMeans(n_clusters=k, n_init=10, random_state=42).fit(x)
        labels, inertia, centres = A.kmeans_fit(x, k, 10, 42, device="cuda")
        assert labels.dtype == np.int32 and np.array_equal(labels, km.labels_), k
        # both sides carry fp32 rounding of the 8-term distances and of sklearn's own fp32 inertia sum
        # (~N^0.5 * 6e-8 relative); centres of magnitude <= 16 hold 16 * 6e-8 * a few roundings
        assert abs(inertia - km.inertia_) <= 1e-5 * km.inertia_
        assert np.abs(centres - km.cluster_centers_).max() <= 1e-4


def test_clustering_cli_on_the_device_matches_the_reference_golden(dev, tmp_path):
    """src.clustering --device cuda on the CPU test's bundle: the golden's
    labels, ARI and NMI; silhouette within the bound measured above of the fp64
    score (and of the golden, up to the golden's own distance to fp64: sklearn
    scored fp32 input there)."""
    import json

    import pandas as pd
    from sklearn.metrics import silhouette_score

    from test_cpu_analytics import evaluate_all, load_gold, run_clustering_cli

    gold, z = load_gold()
    pca, results = evaluate_all("cuda")
    x64 = z["cluster_space"].astype(np.float64)
    assert len(results) == len(gold["results"])
    for r, g in zip(results, gold["results"]):
        assert (r.method, r.params) == (g["method"], g["params"])
        assert np.array_equal(r.labels, g["labels"]), g["params"]
        assert abs(r.ari - g["ARI"]) <= 1e-12 and abs(r.nmi - g["NMI"]) <= 1e-12
        s64 = float(silhouette_score(x64, np.array(g["labels"])))
        err = abs(r.silhouette - s64)
        _measure("silhouette", err, BOUND_SILHOUETTE)
        assert err <= BOUND_SILHOUETTE, g["params"]
        assert abs(r.silhouette - g["silhouette"]) <= BOUND_SILHOUETTE + abs(s64 - g["silhouette"])

    out = run_clustering_cli(tmp_path, "cuda")
    metrics = pd.read_csv(out / "tables" / "metrics_clustering.csv", float_precision="round_trip")
    assert list(metrics.columns) == gold["metrics_columns"]
    for (_, row), r, g in zip(metrics.iterrows(), results, gold["results"]):
        assert json.loads(row["params_json"]) == g["params"]
        assert abs(row["ARI"] - g["ARI"]) <= 1e-12 and abs(row["NMI"] - g["NMI"]) <= 1e-12
        assert row["silhouette"] == r.silhouette and row["noise_rate"] == g["noise_rate"]  # bit-reproducible
    assign = pd.read_csv(out / "tables" / "cluster_assignments.csv")
    by_params = {json.dumps(g["params"], sort_keys=True): g["labels"] for g in gold["results"]}
    assert assign["cluster_kmeans"].tolist() == by_params[json.dumps(gold["best_kmeans_params"], sort_keys=True)]
    assert assign["cluster_dbscan"].tolist() == by_params[json.dumps(gold["best_dbscan_params"], sort_keys=True)]
    assert (out / "figures" / f"kdist_plot_{gold['best_dbscan_params']['scope']}.png").stat().st_size > 0

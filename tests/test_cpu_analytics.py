"""CPU: the host layer of the embedding analytics (ssip/analytics.py on the
numpy backend) against sklearn, and the two CLIs src.standardize_features and
src.clustering --device cpu against the golden the reference's own functions
wrote (tests/golden/make_clustering_goldens.py)."""
import ctypes
import json
import sys
from pathlib import Path

import numpy as np
import pytest

from ssip import _lib
from ssip import analytics as A

GOLD = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLD))


# ---------------------------------------------------------------------------
# K-Means replay
# ---------------------------------------------------------------------------
def _kmeans_inputs():
    rng = np.random.default_rng(0)
    cent = rng.normal(size=(4, 8)) * 4
    blobs = (cent[rng.integers(0, 4, 280)] + rng.normal(size=(280, 8))).astype(np.float32)
    gauss = rng.normal(size=(300, 12)).astype(np.float32)
    return {"blobs": blobs, "gauss": gauss}


@pytest.mark.parametrize("name", ("blobs", "gauss"))
@pytest.mark.parametrize("k", (2, 3, 4, 5, 7))
def test_kmeans_replays_sklearn(name, k):
    from sklearn.cluster import KMeans

    x = _kmeans_inputs()[name]
    km = KMeans(n_clusters=k, n_init=10, random_state=42).fit(x)
    labels, inertia, centres = A.kmeans_fit(x, k, n_init=10, seed=42, device="cpu")
    assert labels.dtype == np.int32 and np.array_equal(labels, km.labels_)
    assert abs(inertia - km.inertia_) <= 1e-6 * km.inertia_
    assert centres.shape == (k, x.shape[1])


def test_lloyd_relocates_an_empty_cluster_like_sklearn():
    """A far-away initial centre attracts no point: it moves to the point
    farthest from its own centre, and the donor's sum is corrected."""
    rng = np.random.default_rng(1)
    x = rng.normal(size=(60, 3))
    init = np.vstack([x[0], x[1], np.full(3, 100.0)])
    be = A.NumpyBackend(x)
    be.begin(init)
    be.assign()
    _, _, changed, n_empty = be.update()
    assert n_empty == 1 and changed == 60
    labels = be.labels()
    far = int(np.argmax(be._mind2))
    be.relocate()
    assert np.allclose(be.Cn[2], x[far])
    donor = labels[far]
    keep = (labels == donor) & (np.arange(60) != far)
    assert np.allclose(be.Cn[donor], x[keep].mean(axis=0))
    labels_f, inertia, centres, _ = A.lloyd(A.NumpyBackend(x), init, 0.0)
    assert np.bincount(labels_f, minlength=3).min() > 0
    assert np.isclose(inertia, ((x - centres[labels_f]) ** 2).sum())


# ---------------------------------------------------------------------------
# DBSCAN labeller
# ---------------------------------------------------------------------------
def _dbscan_point_sets():
    for s in range(30):
        r = np.random.default_rng(100 + s)
        n = int(r.integers(40, 120))
        yield np.concatenate([r.normal(size=(n // 2, 2)), r.normal(size=(n - n // 2, 2)) * 0.5 + 2.5])


def test_dbscan_labeller_matches_sklearn_on_270_configurations():
    from sklearn.cluster import DBSCAN

    checked = 0
    for x in _dbscan_point_sets():
        dist = np.sqrt(((x[:, None] - x[None]) ** 2).sum(-1))  # fp64
        for eps in (0.2, 0.35, 0.5):
            adj = dist <= eps
            for ms in (3, 5, 8):
                ref = DBSCAN(eps=eps, min_samples=ms).fit_predict(x)
                assert np.array_equal(A.dbscan_labels_from_graph(adj.sum(axis=1), adj, ms), ref)
                assert np.array_equal(A.dbscan(x, eps, ms, device="cpu"), ref)
                checked += 1
    assert checked == 270


def test_pack_adjacency_layout():
    adj = np.zeros((2, 70), dtype=bool)
    adj[0, [0, 31, 32, 69]] = True
    words = A.pack_adjacency(adj)
    assert words.dtype == np.uint32 and words.shape == (2, 3)
    assert words[0].tolist() == [0x80000001, 1, 1 << 5] and not words[1].any()


def test_silhouette_and_kth_match_sklearn_on_the_host_backend():
    from sklearn.metrics import silhouette_score
    from sklearn.neighbors import NearestNeighbors

    rng = np.random.default_rng(4)
    x = rng.normal(size=(90, 6)) + 3.0 * rng.integers(0, 3, size=(90, 1))
    labels = rng.integers(-1, 3, size=90)
    labels[7] = 9  # a singleton
    assert abs(A.silhouette(x, labels, device="cpu") - silhouette_score(x, labels)) <= 1e-12
    assert np.isnan(A.silhouette(x, np.zeros(90, dtype=int), device="cpu"))
    assert np.isnan(A.silhouette(x, np.arange(90), device="cpu"))
    ref = NearestNeighbors(n_neighbors=5).fit(x).kneighbors(x)[0][:, -1]
    assert np.abs(A.kth_neighbor_distance(x, 5, device="cpu") - ref).max() <= 1e-12
    with pytest.raises(ValueError):
        A.kth_neighbor_distance(x, 91, device="cpu")


# ---------------------------------------------------------------------------
# C ABI: argument errors need no device
# ---------------------------------------------------------------------------
def test_analytics_argument_errors_surface_as_status_codes():
    lib = _lib.lib()
    buf = (ctypes.c_float * 4)()
    p = ctypes.addressof(buf)
    assert lib.ssip_pairwise_eps(65537, 2, p, 1.0, p, p, None) == -1
    assert b"65536" in lib.ssip_last_error()
    assert lib.ssip_pairwise_kth(3, 2, 5, p, p, None) == -1
    assert b"neighbours asked" in lib.ssip_last_error()
    assert lib.ssip_pairwise_kth(100, 2, 65, p, p, None) == -1
    assert lib.ssip_pairwise_cluster_sums(10, 2, 257, p, p, p, p, None) == -1
    assert lib.ssip_kmeans_assign(10, 513, 2, p, p, None, p, p, p, 1 << 20, None) == -1
    assert lib.ssip_kmeans_assign(10, 4, 65, p, p, None, p, p, p, 1 << 20, None) == -1
    need = lib.ssip_kmeans_workspace_bytes(1000, 50, 10)
    g = 4  # ceil(1000 / 256) workgroups
    assert need >= g * 10 * 50 * 4 + g * 10 * 4 + g * 12
    assert lib.ssip_kmeans_workspace_bytes(1000, 0, 10) < 0
    aligned = (p + 15) // 16 * 16
    assert lib.ssip_kmeans_assign(1000, 50, 10, p, p, None, p, p, aligned, need - 1, None) == -3
    assert lib.ssip_plan_fn_index(b"ssip_pairwise_eps") >= 0  # recordable in a launch plan


# ---------------------------------------------------------------------------
# src.standardize_features
# ---------------------------------------------------------------------------
def test_standardize_features_cli(tmp_path):
    from sklearn.preprocessing import StandardScaler

    from make_clustering_goldens import write_embeddings
    from src import standardize_features as S

    gold = json.loads((GOLD / "clustering_ref.json").read_text())
    emb, frame = write_embeddings(tmp_path / "emb")
    out = tmp_path / "features" / "standardized_features.npz"
    S.main(["--embeddings-npy", str(tmp_path / "emb" / "embeddings.npy"),
            "--embeddings-csv", str(tmp_path / "emb" / "embeddings.csv"), "--output-npz", str(out)])
    z = np.load(out, allow_pickle=True)
    kinds = {k: [z[k].dtype.kind, z[k].dtype.itemsize if z[k].dtype.kind in "fb" else 0, z[k].ndim] for k in z.files}
    assert kinds == gold["standardized_npz"]  # the reference's keys and dtypes
    sc = StandardScaler()
    want = sc.fit_transform(emb.astype(np.float32)).astype(np.float32)
    assert np.array_equal(z["features"], want)
    assert np.array_equal(z["scaler_mean"], sc.mean_.astype(np.float32))
    assert np.array_equal(z["scaler_scale"], sc.scale_.astype(np.float32))
    # rows follow the index column, not the shuffled file order
    assert z["paths"].tolist() == frame["path"].tolist()
    lab = (frame["bucket"] == "labeled").to_numpy()
    assert np.array_equal(z["is_labeled"], lab)
    assert z["labels"].tolist() == [v if m else "" for v, m in zip(frame["label"].tolist(), lab)]


# ---------------------------------------------------------------------------
# src.clustering --device cpu against the reference golden
# ---------------------------------------------------------------------------
def load_gold():
    return json.loads((GOLD / "clustering_ref.json").read_text()), np.load(GOLD / "clustering_bundle.npz",
                                                                            allow_pickle=True)


def run_clustering_cli(root: Path, device: str):
    """Runs the CLI on the golden bundle with the golden's grids; returns the output root."""
    from src import clustering as C

    gold, z = load_gold()
    npz = root / "standardized_features.npz"
    np.savez_compressed(npz, **{k: z[k] for k in z.files if k != "cluster_space"})
    out = root / "out"
    C.main(["--features-npz", str(npz), "--output-root", str(out), "--device", device, "--log-level", "WARNING",
            "--kmeans-range", *map(str, gold["kmeans_range"]), "--kmeans-n-init", str(gold["kmeans_n_init"]),
            "--tsne-perplexities", "10", "--umap-neighbors", "--umap-min-dist",
            "--dbscan-eps", *(repr(e) for e in gold["dbscan_eps"]),
            "--dbscan-min-samples", *map(str, gold["dbscan_min_samples"]), "--seed", str(gold["seed"])])
    return out


def evaluate_all(device: str):
    """Per-configuration results of the module's own evaluate_* on the golden bundle."""
    from src import clustering as C

    gold, z = load_gold()
    bundle = C.FeatureBundle(z["features"], z["paths"].astype(str), z["is_labeled"], z["labels"].astype(str), None,
                             None)
    pca = C.run_pca(bundle.features, gold["variance_target"], gold["tsne_dim"], gold["seed"])
    res = C.evaluate_kmeans(pca.cluster_space, bundle, gold["kmeans_range"], gold["kmeans_n_init"], gold["seed"],
                            device)
    res += C.evaluate_dbscan(pca.cluster_space, bundle, gold["dbscan_eps"], gold["dbscan_min_samples"], gold["seed"],
                             "all", device)
    return pca, res


def check_results_against_gold(results, gold, silhouette_tol):
    assert len(results) == len(gold["results"])
    for r, g in zip(results, gold["results"]):
        assert (r.method, r.space, r.params) == (g["method"], g["space"], g["params"])
        assert np.array_equal(r.labels, g["labels"]), g["params"]
        assert abs(r.ari - g["ARI"]) <= 1e-12 and abs(r.nmi - g["NMI"]) <= 1e-12
        assert abs(r.silhouette - g["silhouette"]) <= silhouette_tol, (g["params"], r.silhouette, g["silhouette"])
        assert r.noise_rate == g["noise_rate"]


def test_golden_eps_values_sit_in_distance_gaps():
    gold, z = load_gold()
    x = z["cluster_space"].astype(np.float64)
    dist = np.sqrt(((x[:, None] - x[None]) ** 2).sum(-1))
    for eps in gold["dbscan_eps"]:
        assert (np.abs(dist - eps) > 1e-3 * eps).all()
    db = [g for g in gold["results"] if g["method"] == "dbscan"]
    assert any(0.0 < g["noise_rate"] < 1.0 for g in db)
    assert any((((dist <= g["params"]["eps"]).sum(axis=1) < g["params"]["min_samples"])
                & (np.array(g["labels"]) >= 0)).any() for g in db)  # a border point


def test_clustering_functions_match_the_reference_golden():
    gold, z = load_gold()
    pca, results = evaluate_all("cpu")
    assert pca.cluster_space.data.shape[1] == gold["pca_components"]
    assert np.abs(pca.cluster_space.data - z["cluster_space"]).max() <= 1e-5
    check_results_against_gold(results, gold, 1e-6)


def test_clustering_cli_cpu_artefacts(tmp_path):
    import pandas as pd

    gold, z = load_gold()
    out = run_clustering_cli(tmp_path, "cpu")
    emb_dir = out / "features" / "dimensionality_reduction"
    assert sorted(p.name for p in emb_dir.iterdir()) == ["pca_2d.npz", "pca_cluster.npz", "pca_tsne_init.npz",
                                                         "tsne_perp10.npz"]
    pc = np.load(emb_dir / "pca_cluster.npz")
    assert sorted(pc.files) == ["embedding", "params_json"]
    assert json.loads(str(pc["params_json"])) == {"components": gold["pca_components"],
                                                  "variance_target": gold["variance_target"]}
    assert pc["embedding"].shape == (240, gold["pca_components"])
    assert np.abs(pc["embedding"] - z["cluster_space"]).max() <= 1e-5

    metrics = pd.read_csv(out / "tables" / "metrics_clustering.csv")
    assert list(metrics.columns) == gold["metrics_columns"]
    assert len(metrics) == len(gold["results"])
    for (_, row), g in zip(metrics.iterrows(), gold["results"]):
        assert row["method"] == g["method"] and row["space"] == g["space"]
        assert json.loads(row["params_json"]) == g["params"]
        assert abs(row["ARI"] - g["ARI"]) <= 1e-12 and abs(row["NMI"] - g["NMI"]) <= 1e-12
        assert abs(row["silhouette"] - g["silhouette"]) <= 1e-6
        assert row["noise_rate"] == g["noise_rate"] and row["seed"] == gold["seed"]

    assign = pd.read_csv(out / "tables" / "cluster_assignments.csv")
    assert list(assign.columns) == gold["assignments_columns"]
    by_params = {json.dumps(g["params"], sort_keys=True): g["labels"] for g in gold["results"]}
    assert assign["cluster_kmeans"].tolist() == by_params[json.dumps(gold["best_kmeans_params"], sort_keys=True)]
    assert assign["cluster_dbscan"].tolist() == by_params[json.dumps(gold["best_dbscan_params"], sort_keys=True)]
    assert (assign["pca_dim"] == gold["pca_components"]).all()
    assert (assign["tsne_id"] == "tsne_perp10").all()
    assert (assign["umap_id"] == "pca_2d").all()  # empty UMAP grid
    assert assign["path"].tolist() == z["paths"].tolist()

    report = (out / "notes" / "clustering_report.md").read_text()
    assert [ln for ln in report.splitlines() if ln.startswith("#")] == gold["report_headings"]
    best_scope = gold["best_dbscan_params"]["scope"]
    for fig in ("pca2d_clusters.png", "tsne2d_clusters.png", f"kdist_plot_{best_scope}.png"):
        assert (out / "figures" / fig).stat().st_size > 0
    assert not (out / "figures" / "umap2d_clusters.png").exists()


def test_clustering_cli_surface():
    from src import clustering as C

    a = C.parse_args(["--features-npz", "x.npz"])
    assert a.device == "auto" and a.kmeans_range == list(range(2, 11)) and a.dbscan_eps == [0.5, 0.75, 1.0, 1.25]
    assert a.dbscan_min_samples == [5, 10, 15] and a.tsne_perplexities == [10.0, 30.0, 50.0]
    assert a.umap_neighbors == [15, 30, 50] and a.umap_min_dist == [0.0, 0.1] and a.seed == 42
    assert a.variance_target == 0.9 and a.tsne_dim == 50 and a.dbscan_scope == "all" and not a.dbscan_auto
    assert C.resolve_device("auto") == "cuda" and C.resolve_device("cpu") == "cpu"

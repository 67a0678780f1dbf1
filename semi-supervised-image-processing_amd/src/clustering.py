"""Dimensionality reduction and clustering of the standardised embeddings —
drop-in mirror of the reference's src/clustering.py with the distance work on
the HIP kernels (ssip/analytics.py over csrc/analytics.hip).

    python -m src.clustering --features-npz outputs/features/standardized_features.npz

Same flags and defaults (:671-770), same artefacts under --output-root:
features/dimensionality_reduction/<name>.npz (``embedding`` + ``params_json``;
pca_cluster, pca_2d, pca_tsne_init, tsne_perp*, umap_nn*_md*),
tables/metrics_clustering.csv, tables/cluster_assignments.csv,
figures/{pca2d,tsne2d,umap2d}_clusters.png, figures/kdist_plot_*.png and
notes/clustering_report.md, with the reference's column names and report
headings.  Model selection is the reference's (:441-453): best ARI, then NMI,
then silhouette, external metrics on the labeled subset only.

What runs where:
  * K-Means (:340-373), DBSCAN (:376-428), the silhouette score (:330-337) and
    the k-distance curve (:430-438, :541-563) go through ssip.analytics.
    ``--device cuda`` (and ``auto``) uses the HIP kernels; ``--device cpu`` is
    an explicit host path on the same driver with the numpy backend.  Two
    extension flags: ``--device``, ``--tsne-method`` and ``--umap-method``.
    DBSCAN takes up to 2^20 rows: up to 65,536 it labels a packed eps graph on
    the host, above that it propagates labels on the backend without storing
    the graph (ssip.analytics.dbscan_sweep picks by the row count; the labels
    are the same).
  * Standardisation checks and PCA (sklearn, svd_solver="full": the reference's
    cluster space bit for bit) stay on the host: O(N*D^2) at most, against
    O(N^2*d) per DBSCAN / silhouette configuration.
  * t-SNE is the reference's sklearn Barnes-Hut call by default.
    ``--tsne-method exact`` runs the exact objective under sklearn's schedule
    through ssip.analytics.tsne_fit (csrc/tsne.hip) on the resolved --device,
    with the same artefact names, npz keys and params.
  * UMAP by default (``--umap-method package``) runs through ``umap`` when that
    package imports; when it does not, one warning is logged and the UMAP grid
    is empty, for which the assignments table names pca_2d as umap_id (the
    reference's behaviour for an empty grid, :858).  ``--umap-method native``
    needs no package: ssip.analytics.umap_fit (csrc/umap.hip) on the resolved
    --device, exact kNN computed once at the largest n_neighbors, the
    reference's artefact names, npz keys and params.  An n_neighbors above
    min(64, N) is skipped with a warning.  The embeddings are reproducible bit
    for bit but not comparable point for point with umap-learn's (Jacobi-ordered
    epochs, hashed negative samples).
"""
from __future__ import annotations

import argparse
import json
import logging
import sys
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

_PKG = Path(__file__).resolve().parents[1]
if str(_PKG) not in sys.path:
    sys.path.insert(0, str(_PKG))

from ssip import analytics  # noqa: E402

METRIC_COLUMNS = ("method", "space", "params_json", "ARI", "NMI", "silhouette", "noise_rate", "seed")
ASSIGNMENT_COLUMNS = ("path", "cluster_kmeans", "cluster_dbscan", "pca_dim", "tsne_id", "umap_id", "is_labeled",
                      "true_label")
SCOPES = ("all", "labeled", "unlabeled")
TSNE_METHODS = ("barnes_hut", "exact")
UMAP_METHODS = ("package", "native")


@dataclass(frozen=True)
class FeatureBundle:
    features: np.ndarray
    paths: np.ndarray
    is_labeled: np.ndarray
    labels: np.ndarray
    scaler_mean: Optional[np.ndarray]
    scaler_scale: Optional[np.ndarray]

    @property
    def labeled_mask(self) -> np.ndarray:
        return self.is_labeled.astype(bool)

    @property
    def unlabeled_mask(self) -> np.ndarray:
        return ~self.labeled_mask

    def scope_mask(self, scope: str) -> np.ndarray:
        if scope not in SCOPES:
            raise ValueError("scope must be one of: all, labeled, unlabeled")
        if scope == "labeled":
            return self.labeled_mask
        if scope == "unlabeled":
            return self.unlabeled_mask
        return np.ones(self.features.shape[0], dtype=bool)


@dataclass(frozen=True)
class EmbeddingResult:
    name: str
    data: np.ndarray
    params: Dict[str, object]


@dataclass(frozen=True)
class ClusteringResult:
    method: str
    space: str
    labels: np.ndarray
    params: Dict[str, object]
    ari: float
    nmi: float
    silhouette: float
    noise_rate: float
    seed: int


@dataclass(frozen=True)
class PCAResults:
    cluster_space: EmbeddingResult
    pca_2d: EmbeddingResult
    pca_tsne_init: EmbeddingResult


# ---------------------------------------------------------------------------
# loading and standardisation checks
# ---------------------------------------------------------------------------
def load_feature_bundle(npz_path: Path) -> FeatureBundle:
    if not npz_path.exists():
        raise FileNotFoundError(f"Standardized feature bundle not found: {npz_path}")
    z = np.load(npz_path, allow_pickle=True)
    absent = sorted({"features", "paths", "is_labeled", "labels"} - set(z.files))
    if absent:
        raise KeyError("Feature bundle missing required arrays: " + ", ".join(absent))
    features = np.asarray(z["features"], dtype=np.float32)
    is_labeled = np.asarray(z["is_labeled"], dtype=bool)
    labels = np.where(is_labeled, np.asarray(z["labels"], dtype=object).astype(str), "")
    paths = np.asarray(z["paths"], dtype=str)
    if features.ndim != 2:
        raise ValueError("`features` must be a 2D array of shape [N, D].")
    for name, arr in (("paths", paths), ("is_labeled", is_labeled), ("labels", labels)):
        if arr.shape[0] != features.shape[0]:
            raise ValueError(f"`{name}` must align with the first dimension of `features`.")
    opt = {k: np.asarray(z[k], dtype=np.float32) if k in z.files else None for k in ("scaler_mean", "scaler_scale")}
    return FeatureBundle(features, paths, is_labeled, labels, opt["scaler_mean"], opt["scaler_scale"])


def validate_standardization(bundle: FeatureBundle) -> Dict[str, Dict[str, float]]:
    def subset(mask):
        rows = bundle.features[mask]
        if rows.size == 0:
            return {"mean_abs_mean": float("nan"), "mean_std": float("nan")}
        return {"mean_abs_mean": float(np.mean(np.abs(rows.mean(axis=0)))), "mean_std": float(np.mean(rows.std(axis=0)))}

    stats = {"labeled": subset(bundle.labeled_mask), "unlabeled": subset(bundle.unlabeled_mask)}
    if bundle.scaler_mean is not None:
        stats["scaler_mean_abs_max"] = {"value": float(np.max(np.abs(bundle.scaler_mean)))}
    if bundle.scaler_scale is not None:
        stats["scaler_scale_mean"] = {"value": float(np.mean(bundle.scaler_scale))}
    return stats


# ---------------------------------------------------------------------------
# embeddings (host)
# ---------------------------------------------------------------------------
def run_pca(features: np.ndarray, variance_target: float, tsne_dim: int, seed: int) -> PCAResults:
    from sklearn.decomposition import PCA

    n_comp = min(features.shape)
    logging.info("Fitting PCA with up to %s components (samples=%s, features=%s)", n_comp, *features.shape)
    pca = PCA(n_components=n_comp, random_state=seed, svd_solver="full")
    proj = pca.fit_transform(features)
    cum = np.cumsum(pca.explained_variance_ratio_)
    keep = int(np.searchsorted(cum, variance_target) + 1)
    keep = max(2, min(keep, proj.shape[1]))
    logging.info("Selected %s PCA components to reach %.2f%% explained variance", keep, cum[keep - 1] * 100)
    t_comp = min(tsne_dim, proj.shape[1])
    return PCAResults(
        cluster_space=EmbeddingResult("pca_cluster", proj[:, :keep],
                                      {"variance_target": variance_target, "components": keep}),
        pca_2d=EmbeddingResult("pca_2d", proj[:, :2], {"components": 2}),
        pca_tsne_init=EmbeddingResult("pca_tsne_init", proj[:, :t_comp], {"components": t_comp}),
    )


def run_tsne(base: EmbeddingResult, perplexities: Sequence[float], seed: int, method: str = "barnes_hut",
             device: str = "cuda") -> List[EmbeddingResult]:
    """barnes_hut: the reference's sklearn call.  exact: ssip.analytics.tsne_fit
    (csrc/tsne.hip on ``device`` cuda, the numpy path on cpu); above its N cap
    one warning is logged and the sklearn call runs instead."""
    from sklearn.manifold import TSNE

    if method not in TSNE_METHODS:
        raise ValueError("t-SNE method must be one of: " + ", ".join(TSNE_METHODS))
    if method == "exact" and base.data.shape[0] > analytics.TSNE_MAX_N:
        logging.warning("exact t-SNE supports N <= %s (got %s): using the sklearn Barnes-Hut call",
                        analytics.TSNE_MAX_N, base.data.shape[0])
        method = "barnes_hut"
    out = []
    for perp in perplexities:
        logging.info("Running t-SNE (perplexity=%s, method=%s)", perp, method)
        if method == "exact":
            emb, _, _ = analytics.tsne_fit(base.data, float(perp), seed=seed, max_iter=1000, device=device)
        else:
            emb = TSNE(n_components=2, perplexity=float(perp), init="pca", random_state=seed, learning_rate="auto",
                       max_iter=1000, metric="euclidean").fit_transform(base.data)
        out.append(EmbeddingResult(f"tsne_perp{int(perp)}", np.asarray(emb), {"perplexity": float(perp), "seed": seed}))
    return out


def run_umap_native(base: EmbeddingResult, neighbor_values: Sequence[int], min_dists: Sequence[float], seed: int,
                    device: str) -> List[EmbeddingResult]:
    """ssip.analytics.umap_fit for every (n_neighbors, min_dist); the kNN graph
    is built once at the largest n_neighbors and sliced."""
    n = base.data.shape[0]
    cap = min(analytics.KNN_MAX_K, n)
    usable = [int(nn) for nn in neighbor_values if 2 <= int(nn) <= cap]
    skipped = [int(nn) for nn in neighbor_values if not 2 <= int(nn) <= cap]
    if skipped:
        logging.warning("native UMAP supports 2 <= n_neighbors <= min(%s, N = %s): skipping n_neighbors = %s",
                        analytics.KNN_MAX_K, n, skipped)
    if not usable:
        return []
    backend = analytics.make_backend(base.data, device)
    backend.knn(max(usable))
    out = []
    for nn in usable:
        for md in min_dists:
            logging.info("Running UMAP (n_neighbors=%s, min_dist=%.2f, method=native)", nn, md)
            emb, _ = analytics.umap_fit(base.data, nn, float(md), seed=seed, device=device, backend=backend)
            out.append(EmbeddingResult(f"umap_nn{int(nn)}_md{md:.2f}", emb,
                                       {"n_neighbors": int(nn), "min_dist": float(md), "seed": seed}))
    return out


def run_umap(base: EmbeddingResult, neighbor_values: Sequence[int], min_dists: Sequence[float],
             seed: int, method: str = "package", device: str = "cuda") -> List[EmbeddingResult]:
    """package: the reference's ``umap`` call (an empty grid and one warning
    when the package does not import).  native: ssip.analytics.umap_fit."""
    if method not in UMAP_METHODS:
        raise ValueError("UMAP method must be one of: " + ", ".join(UMAP_METHODS))
    if not neighbor_values or not min_dists:
        return []
    if method == "native":
        return run_umap_native(base, neighbor_values, min_dists, seed, device)
    try:
        import umap  # type: ignore
    except ImportError:
        logging.warning("umap is not installed: skipping the UMAP embeddings (umap_id falls back to pca_2d)")
        return []
    out = []
    for nn in neighbor_values:
        for md in min_dists:
            logging.info("Running UMAP (n_neighbors=%s, min_dist=%.2f)", nn, md)
            emb = umap.UMAP(n_components=2, n_neighbors=int(nn), min_dist=float(md), random_state=seed,
                            metric="euclidean").fit_transform(base.data)
            out.append(EmbeddingResult(f"umap_nn{int(nn)}_md{md:.2f}", np.asarray(emb),
                                       {"n_neighbors": int(nn), "min_dist": float(md), "seed": seed}))
    return out


# ---------------------------------------------------------------------------
# clustering (ssip.analytics)
# ---------------------------------------------------------------------------
def resolve_device(device: str) -> str:
    """auto | cuda -> the HIP kernels (an error when no device is visible, as
    in the training CLIs); cpu -> the explicit numpy host path."""
    return "cpu" if device == "cpu" else "cuda"


def compute_external_metrics(bundle: FeatureBundle, predicted: np.ndarray) -> Tuple[float, float]:
    from sklearn.metrics import adjusted_rand_score, normalized_mutual_info_score

    mask = bundle.labeled_mask
    if not mask.any():
        return float("nan"), float("nan")
    truth, pred = bundle.labels[mask], predicted[mask]
    return float(adjusted_rand_score(truth, pred)), float(normalized_mutual_info_score(truth, pred))


def compute_silhouette(space: np.ndarray, labels: np.ndarray, backend) -> float:
    try:
        return analytics.silhouette(space, labels, backend=backend)
    except ValueError as e:
        logging.warning("silhouette not computed: %s", e)
        return float("nan")


def evaluate_kmeans(space: EmbeddingResult, bundle: FeatureBundle, k_values: Sequence[int], n_init: int, seed: int,
                    device: str = "cuda", backend=None) -> List[ClusteringResult]:
    backend = backend if backend is not None else analytics.make_backend(space.data, device)
    out = []
    for k in k_values:
        if k < 2:
            continue
        logging.info("Fitting K-Means with k=%s", k)
        labels, _, _ = analytics.kmeans_fit(space.data, int(k), int(n_init), seed, device=device)
        ari, nmi = compute_external_metrics(bundle, labels)
        out.append(ClusteringResult("kmeans", space.name, labels, {"k": int(k), "n_init": int(n_init)}, ari, nmi,
                                    compute_silhouette(space.data, labels, backend), 0.0, seed))
    return out


def evaluate_dbscan(space: EmbeddingResult, bundle: FeatureBundle, eps_values: Sequence[float],
                    min_samples_values: Sequence[int], seed: int, scope: str = "all", device: str = "cuda",
                    backend=None) -> List[ClusteringResult]:
    """DBSCAN over the grids on the scope's subset; points outside it are -1
    and the silhouette is taken on the fitted subset (:384-389).  Every
    min_samples of one eps is labelled in one analytics.dbscan_sweep: from one
    eps graph up to analytics.EPS_MAX_N rows, by label propagation without a
    stored graph above that."""
    mask = bundle.scope_mask(scope)
    sub = space.data[mask]
    if backend is None or scope != "all":
        backend = analytics.make_backend(sub, device)
    out = []
    for eps in eps_values:
        logging.info("Fitting DBSCAN (scope=%s) with eps=%.3f, min_samples=%s", scope, eps, list(min_samples_values))
        sweep = analytics.dbscan_sweep(backend, float(eps), [int(ms) for ms in min_samples_values])
        for ms, sub_labels in zip(min_samples_values, sweep):
            full = np.full(space.data.shape[0], -1, dtype=int)
            full[mask] = sub_labels
            ari, nmi = compute_external_metrics(bundle, full)
            out.append(ClusteringResult(
                "dbscan", f"{space.name}:{scope}", full,
                {"eps": float(eps), "min_samples": int(ms), "scope": scope}, ari, nmi,
                compute_silhouette(sub, sub_labels, backend), float(np.mean(sub_labels == -1)), seed))
    return out


def sorted_kdistance(space: np.ndarray, min_samples: int, device: str = "cuda", backend=None) -> np.ndarray:
    return np.sort(analytics.kth_neighbor_distance(space, int(min_samples), device=device, backend=backend))


def auto_eps_from_kdistance(space: np.ndarray, min_samples: int, quantile: float = 0.98, device: str = "cuda",
                            backend=None) -> float:
    """eps = the quantile of the sorted k-distance curve (:430-438)."""
    curve = sorted_kdistance(space, min_samples, device, backend)
    return float(curve[int(np.clip(round(quantile * (curve.size - 1)), 0, curve.size - 1))])


def choose_best(results: Sequence[ClusteringResult]) -> Optional[ClusteringResult]:
    if not results:
        return None

    def key(r):
        return tuple(np.nan_to_num(v, nan=-1.0) for v in (r.ari, r.nmi, r.silhouette))

    return sorted(results, key=key, reverse=True)[0]


# ---------------------------------------------------------------------------
# artefacts
# ---------------------------------------------------------------------------
def _plt():
    import matplotlib

    matplotlib.use("Agg")
    import matplotlib.pyplot as plt

    return plt


def save_embedding_npz(root: Path, result: EmbeddingResult) -> None:
    root.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(root / f"{result.name}.npz", embedding=result.data,
                        params_json=json.dumps(result.params, sort_keys=True))


def plot_embedding(embedding: EmbeddingResult, bundle: FeatureBundle, cluster_labels: np.ndarray, labeled_title: str,
                   output_path: Path, dbscan_noise_rate: Optional[float] = None) -> None:
    plt = _plt()
    output_path.parent.mkdir(parents=True, exist_ok=True)
    fig, (left, right) = plt.subplots(1, 2, figsize=(12, 5), dpi=150)
    xy = embedding.data
    for cid in np.unique(cluster_labels):
        m = cluster_labels == cid
        tag = f"noise (n={int(m.sum())})" if cid == -1 else f"cluster {cid} (n={int(m.sum())})"
        left.scatter(xy[m, 0], xy[m, 1], s=12, alpha=0.8, label=tag)
    left.set_title(f"{embedding.name} — clusters")
    um, lm = bundle.unlabeled_mask, bundle.labeled_mask
    right.scatter(xy[um, 0], xy[um, 1], s=8, color="lightgray", alpha=0.4, label="unlabeled")
    for name in np.unique(bundle.labels[lm]):
        m = lm & (bundle.labels == name)
        right.scatter(xy[m, 0], xy[m, 1], s=20, alpha=0.9, label=str(name))
    right.set_title(labeled_title)
    for ax in (left, right):
        ax.legend(loc="best", fontsize="small", frameon=False)
        ax.set_xlabel("dim 1")
        ax.set_ylabel("dim 2")
    if dbscan_noise_rate is not None and not np.isnan(dbscan_noise_rate):
        fig.suptitle(f"DBSCAN noise rate: {dbscan_noise_rate:.2%}", fontsize=10)
    fig.tight_layout()
    fig.savefig(output_path, bbox_inches="tight")
    plt.close(fig)


def plot_k_distance(space: EmbeddingResult, min_samples: int, output_path: Path, device: str = "cuda",
                    backend=None) -> None:
    plt = _plt()
    output_path.parent.mkdir(parents=True, exist_ok=True)
    logging.info("Rendering k-distance plot for min_samples=%s (points=%s)", min_samples, space.data.shape[0])
    curve = sorted_kdistance(space.data, min_samples, device, backend)
    fig, ax = plt.subplots(figsize=(6, 4), dpi=150)
    ax.plot(np.arange(curve.size), curve)
    ax.set_xlabel("Points sorted by distance")
    ax.set_ylabel(f"{min_samples}-NN distance")
    ax.set_title("DBSCAN k-distance curve")
    fig.tight_layout()
    fig.savefig(output_path, bbox_inches="tight")
    plt.close(fig)


def write_metrics_table(results: Sequence[ClusteringResult], output_path: Path):
    import pandas as pd

    output_path.parent.mkdir(parents=True, exist_ok=True)
    rows = [dict(zip(METRIC_COLUMNS, (r.method, r.space, json.dumps(r.params, sort_keys=True), r.ari, r.nmi,
                                      r.silhouette, r.noise_rate, r.seed))) for r in results]
    frame = pd.DataFrame(rows, columns=list(METRIC_COLUMNS))
    frame.to_csv(output_path, index=False)
    return frame


def write_assignments_table(bundle: FeatureBundle, kmeans_result: ClusteringResult,
                            dbscan_result: Optional[ClusteringResult], pca_results: PCAResults,
                            tsne_choice: EmbeddingResult, umap_choice: EmbeddingResult, output_path: Path):
    import pandas as pd

    output_path.parent.mkdir(parents=True, exist_ok=True)
    db = dbscan_result.labels if dbscan_result is not None else np.full_like(kmeans_result.labels, -1)
    frame = pd.DataFrame(dict(zip(ASSIGNMENT_COLUMNS, (
        bundle.paths, kmeans_result.labels, db, pca_results.cluster_space.data.shape[1], tsne_choice.name,
        umap_choice.name, bundle.is_labeled, bundle.labels))))
    frame.to_csv(output_path, index=False)
    return frame


def write_report(output_path: Path, stats: Dict[str, Dict[str, float]], kmeans_best: ClusteringResult,
                 dbscan_best: Optional[ClusteringResult]) -> None:
    output_path.parent.mkdir(parents=True, exist_ok=True)

    def scores(r, noise=False):
        s = f"- ARI={r.ari:.4f}, NMI={r.nmi:.4f}, silhouette={r.silhouette:.4f}"
        return s + (f", noise_rate={r.noise_rate:.4f}" if noise else "")

    out = ["# Clustering Analysis Report", "", "## Standardization Checks"]
    out += [f"- {name}: " + ", ".join(f"{k}={v:.4f}" for k, v in vals.items()) for name, vals in stats.items()]
    out += ["", "## Best K-Means Configuration", f"- Params: {json.dumps(kmeans_best.params, sort_keys=True)}",
            scores(kmeans_best), "", "## Best DBSCAN Configuration"]
    if dbscan_best is not None:
        out += [f"- Params: {json.dumps(dbscan_best.params, sort_keys=True)}", scores(dbscan_best, noise=True)]
    else:
        out.append("- No viable DBSCAN configuration identified.")
    out += ["", "## Notes", "- ARI/NMI computed on labeled subset only; silhouette on full PCA space.",
            "- See tables and figures under `outputs/` for further details.", ""]
    output_path.write_text("\n".join(out), encoding="utf-8")


# ---------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------
def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    p = argparse.ArgumentParser(description="Task 3 clustering pipeline")
    p.add_argument("--features-npz", type=Path, required=True, help="Path to the standardized feature bundle (.npz).")
    p.add_argument("--output-root", type=Path, default=Path("outputs"), help="Root directory for generated artifacts.")
    p.add_argument("--variance-target", type=float, default=0.9,
                   help="Explained variance threshold for PCA cluster space.")
    p.add_argument("--tsne-dim", type=int, default=50, help="Number of PCA components fed into t-SNE and UMAP.")
    p.add_argument("--tsne-perplexities", type=float, nargs="*", default=[10.0, 30.0, 50.0],
                   help="Perplexities to evaluate for t-SNE.")
    p.add_argument("--umap-neighbors", type=int, nargs="*", default=[15, 30, 50],
                   help="n_neighbors values to evaluate for UMAP.")
    p.add_argument("--umap-min-dist", type=float, nargs="*", default=[0.0, 0.1],
                   help="min_dist values to evaluate for UMAP.")
    p.add_argument("--kmeans-range", type=int, nargs="*", default=list(range(2, 11)),
                   help="Candidate cluster counts for K-Means.")
    p.add_argument("--kmeans-n-init", type=int, default=10, help="Number of initializations for each K-Means run.")
    p.add_argument("--dbscan-eps", type=float, nargs="*", default=[0.5, 0.75, 1.0, 1.25],
                   help="Candidate epsilon values for DBSCAN.")
    p.add_argument("--dbscan-min-samples", type=int, nargs="*", default=[5, 10, 15],
                   help="Candidate min_samples values for DBSCAN.")
    p.add_argument("--dbscan-scope", type=str, default="all", choices=list(SCOPES),
                   help="Run DBSCAN on: all points, labeled subset only, or unlabeled subset only.")
    p.add_argument("--dbscan-auto", action="store_true",
                   help="Pick eps from the 98th percentile of the k-distance curve (0.8x, 1x, 1.2x per min_samples). "
                        "Overrides --dbscan-eps.")
    p.add_argument("--seed", type=int, default=42, help="Random seed for reproducible embeddings and clustering.")
    p.add_argument("--log-level", type=str, default="INFO", choices=["DEBUG", "INFO", "WARNING", "ERROR"],
                   help="Logging verbosity.")
    # ssip extension (optional)
    p.add_argument("--device", type=str, default="auto", choices=["auto", "cuda", "cpu"],
                   help="Where K-Means, DBSCAN, silhouette and the k-distance curve run: auto/cuda = the HIP kernels, "
                        "cpu = the numpy host path of the same driver.")
    p.add_argument("--tsne-method", type=str, default="barnes_hut", choices=list(TSNE_METHODS),
                   help="barnes_hut = sklearn's TSNE on the host (the reference's call); exact = the exact objective "
                        "through ssip.analytics.tsne_fit on --device.")
    p.add_argument("--umap-method", type=str, default="package", choices=list(UMAP_METHODS),
                   help="package = the umap package on the host (the reference's call; skipped with a warning when "
                        "it is not installed); native = ssip.analytics.umap_fit on --device, no package needed.")
    return p.parse_args(argv)


def main(argv: Optional[Sequence[str]] = None) -> None:
    args = parse_args(argv)
    logging.basicConfig(level=getattr(logging, args.log_level.upper()),
                        format="%(asctime)s [%(levelname)s] %(message)s")
    device = resolve_device(args.device)
    logging.info("Clustering analytics on: %s", device)

    bundle = load_feature_bundle(args.features_npz)
    stats = validate_standardization(bundle)
    logging.info("Standardization summary: %s", stats)

    pca = run_pca(bundle.features, args.variance_target, args.tsne_dim, args.seed)
    emb_dir = args.output_root / "features" / "dimensionality_reduction"
    tsne = run_tsne(pca.pca_tsne_init, args.tsne_perplexities, args.seed, args.tsne_method, device)
    umaps = run_umap(pca.pca_tsne_init, args.umap_neighbors, args.umap_min_dist, args.seed, args.umap_method, device)
    for emb in [pca.cluster_space, pca.pca_2d, pca.pca_tsne_init, *tsne, *umaps]:
        save_embedding_npz(emb_dir, emb)

    space = pca.cluster_space
    figures = args.output_root / "figures"
    full_backend = analytics.make_backend(space.data, device)
    kmeans_results = evaluate_kmeans(space, bundle, args.kmeans_range, args.kmeans_n_init, args.seed, device,
                                     full_backend)

    scope = args.dbscan_scope
    sub = space.data[bundle.scope_mask(scope)]
    sub_backend = full_backend if scope == "all" else analytics.make_backend(sub, device)
    eps_grid = list(args.dbscan_eps)
    if args.dbscan_auto:
        sub_emb = EmbeddingResult(f"pca_cluster:{scope}", sub, {})
        picks = []
        for ms in args.dbscan_min_samples:
            plot_k_distance(sub_emb, int(ms), figures / f"kdist_plot_{scope}_ms{int(ms)}.png", device, sub_backend)
            base = auto_eps_from_kdistance(sub, int(ms), 0.98, device, sub_backend)
            picks += [max(1e-6, base * f) for f in (0.8, 1.0, 1.2)]
        eps_grid = sorted({float(e) for e in picks})
    dbscan_results = evaluate_dbscan(space, bundle, eps_grid, args.dbscan_min_samples, args.seed, scope, device,
                                     sub_backend)

    metrics_path = args.output_root / "tables" / "metrics_clustering.csv"
    metrics = write_metrics_table(kmeans_results + dbscan_results, metrics_path)
    logging.info("Wrote metrics table to %s", metrics_path)

    best_kmeans = choose_best(kmeans_results)
    if best_kmeans is None:
        raise RuntimeError("K-Means sweep produced no viable solutions.")
    best_dbscan = choose_best(dbscan_results)

    tsne_choice = tsne[0] if tsne else pca.pca_2d
    umap_choice = umaps[0] if umaps else pca.pca_2d
    assignments_path = args.output_root / "tables" / "cluster_assignments.csv"
    assignments = write_assignments_table(bundle, best_kmeans, best_dbscan, pca, tsne_choice, umap_choice,
                                          assignments_path)
    logging.info("Wrote cluster assignments to %s", assignments_path)

    noise = best_dbscan.noise_rate if best_dbscan is not None else None
    todo = [(pca.pca_2d, "PCA 2D — labeled overlay", "pca2d_clusters.png")]
    if tsne:
        todo.append((tsne_choice, "t-SNE 2D — labeled overlay", "tsne2d_clusters.png"))
    if umaps:
        todo.append((umap_choice, "UMAP 2D — labeled overlay", "umap2d_clusters.png"))
    for emb, title, fname in todo:
        plot_embedding(emb, bundle, best_kmeans.labels, title, figures / fname, dbscan_noise_rate=noise)
    if best_dbscan is not None:
        best_scope = str(best_dbscan.params.get("scope", scope))
        best_sub = space.data[bundle.scope_mask(best_scope)]
        plot_k_distance(EmbeddingResult(f"pca_cluster:{best_scope}", best_sub, {}),
                        int(best_dbscan.params.get("min_samples", 5)), figures / f"kdist_plot_{best_scope}.png",
                        device, sub_backend if best_scope == scope else None)

    report_path = args.output_root / "notes" / "clustering_report.md"
    write_report(report_path, stats, best_kmeans, best_dbscan)
    logging.info("Wrote clustering report to %s", report_path)
    logging.info("Artifacts generated: %s rows in assignments, %s rows in metrics", assignments.shape[0],
                 metrics.shape[0])


if __name__ == "__main__":
    main()

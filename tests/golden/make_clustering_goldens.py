"""Writes tests/golden/clustering_ref.json and clustering_bundle.npz from the
reference's own run_pca / evaluate_kmeans / evaluate_dbscan
(src/clustering.py of Septimus4/semi-supervised-image-processing).

usage: python tests/golden/make_clustering_goldens.py --reference /path/to/reference/checkout

The reference imports ``umap`` at module level; it is stubbed in sys.modules
before the import (no UMAP grid is evaluated here).  Run where the reference
checkout and sklearn are available; the tests only read the two files.

Bundle: 240 points in 4 blobs (low-rank within-blob spread), d = 32, standardised, 80 of them labelled.
DBSCAN eps values are snapped into gaps of the sorted fp64 pairwise distances
of the cluster space (no distance within 2e-3 * eps; the tests need 1e-3), so
that an fp32 distance cannot flip a neighbourhood; the script asserts this, and
that some configuration has 0 < noise_rate < 1 and a border point.
"""
import argparse
import json
import sys
import tempfile
import types
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
K_RANGE = [2, 3, 4, 5, 6]
MIN_SAMPLES = [5, 10]
N_INIT = 10
SEED = 42
VARIANCE_TARGET = 0.9
TSNE_DIM = 50
GAP = 2e-3


def make_bundle():
    from sklearn.preprocessing import StandardScaler

    rng = np.random.default_rng(2024)
    centres = rng.normal(size=(4, 32)) * 1.6
    blob = np.arange(240) % 4
    # within-blob spread mostly along 3 directions: nearest-neighbour distances sit far below the bulk of
    # the pairwise distances, where the sorted distances are sparse enough to leave gaps for eps
    basis = rng.normal(size=(3, 32))
    spread = rng.normal(size=(240, 3)) @ basis * (0.3 + 0.15 * blob[:, None])
    raw = (centres[blob] + spread + 0.05 * rng.normal(size=(240, 32))).astype(np.float32)
    feats = StandardScaler().fit_transform(raw).astype(np.float32)
    is_labeled = np.zeros(240, dtype=bool)
    is_labeled[rng.permutation(240)[:80]] = True
    names = np.array(["glioma", "meningioma", "pituitary", "healthy"])
    labels = np.where(is_labeled, names[blob], "")
    paths = np.array([f"img_{i:04d}.jpg" for i in range(240)])
    return feats, paths, is_labeled, labels


def write_embeddings(root, seed=7, n=50, d=16):
    """A synthetic embeddings.npy / embeddings.csv pair (the feature-extraction
    outputs) with the CSV rows shuffled against their index column."""
    import pandas as pd

    rng = np.random.default_rng(seed)
    emb = (rng.normal(size=(n, d)) * rng.uniform(0.5, 3.0, size=d) + rng.normal(size=d)).astype(np.float32)
    labeled = rng.random(n) < 0.4
    frame = pd.DataFrame({
        "index": np.arange(n), "path": [f"scan_{i:03d}.jpg" for i in range(n)],
        "bucket": np.where(labeled, "labeled", "unlabeled"),
        "label": [("cancer" if i % 2 else "normal") if lab else None for i, lab in enumerate(labeled)],
    })
    root.mkdir(parents=True, exist_ok=True)
    np.save(root / "embeddings.npy", emb)
    frame.iloc[rng.permutation(n)].to_csv(root / "embeddings.csv", index=False)
    return emb, frame


def snap_to_gap(dist_sorted, target):
    mid = 0.5 * (dist_sorted[1:] + dist_sorted[:-1])
    ok = (dist_sorted[1:] - mid >= GAP * mid) & (mid - dist_sorted[:-1] >= GAP * mid)
    cand = mid[ok]
    return float(cand[np.abs(cand - target).argmin()])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", type=Path, required=True)
    a = ap.parse_args()
    sys.modules.setdefault("umap", types.ModuleType("umap"))
    sys.path.insert(0, str(a.reference))
    from src import clustering as ref  # the reference's module

    feats, paths, is_labeled, labels = make_bundle()
    bundle = ref.FeatureBundle(features=feats, paths=paths, is_labeled=is_labeled, labels=labels,
                               scaler_mean=np.zeros(32, np.float32), scaler_scale=np.ones(32, np.float32))
    pca = ref.run_pca(feats, VARIANCE_TARGET, TSNE_DIM, SEED)
    space = pca.cluster_space.data

    x = space.astype(np.float64)
    dist = np.sqrt(((x[:, None] - x[None]) ** 2).sum(-1))
    ds = np.unique(dist)
    k5 = np.sort(dist, axis=1)[:, 4]
    eps_values = sorted({snap_to_gap(ds, float(np.quantile(k5, q))) for q in (0.35, 0.7, 0.95)})
    for eps in eps_values:
        assert (np.abs(dist - eps) > 1e-3 * eps).all(), eps

    km = ref.evaluate_kmeans(pca.cluster_space, bundle, K_RANGE, N_INIT, SEED)
    db = ref.evaluate_dbscan(pca.cluster_space, bundle, eps_values, MIN_SAMPLES, SEED, scope="all")
    some_noise = border = False
    for r in db:
        some_noise |= 0.0 < r.noise_rate < 1.0
        core = (dist <= r.params["eps"]).sum(axis=1) >= r.params["min_samples"]
        border |= bool(((r.labels >= 0) & ~core).any())
    assert some_noise and border, (some_noise, border)

    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        metrics = ref.write_metrics_table(km + db, tmp / "m.csv")
        best_km, best_db = ref.choose_best(km), ref.choose_best(db)
        assign = ref.write_assignments_table(bundle, best_km, best_db, pca, pca.pca_2d, pca.pca_2d, tmp / "a.csv")
        ref.write_report(tmp / "r.md", ref.validate_standardization(bundle), best_km, best_db)
        headings = [ln for ln in (tmp / "r.md").read_text().splitlines() if ln.startswith("#")]

        from src import standardize_features as ref_std

        write_embeddings(tmp / "emb")
        ref_std.standardize_embeddings(tmp / "emb" / "embeddings.npy", tmp / "emb" / "embeddings.csv", tmp / "std.npz")
        std = np.load(tmp / "std.npz", allow_pickle=True)
        std_kinds = {k: [std[k].dtype.kind, std[k].dtype.itemsize if std[k].dtype.kind in "fb" else 0, std[k].ndim]
                     for k in std.files}

    def rec(r):
        return {"method": r.method, "space": r.space, "params": r.params, "labels": [int(v) for v in r.labels],
                "ARI": r.ari, "NMI": r.nmi, "silhouette": r.silhouette, "noise_rate": r.noise_rate}

    out = {
        "kmeans_range": K_RANGE, "kmeans_n_init": N_INIT, "seed": SEED, "variance_target": VARIANCE_TARGET,
        "tsne_dim": TSNE_DIM, "dbscan_eps": eps_values, "dbscan_min_samples": MIN_SAMPLES,
        "pca_components": int(space.shape[1]),
        "results": [rec(r) for r in km + db],
        "best_kmeans_params": best_km.params, "best_dbscan_params": best_db.params,
        "metrics_columns": list(metrics.columns), "assignments_columns": list(assign.columns),
        "report_headings": headings,
        "standardized_npz": std_kinds,
    }
    (HERE / "clustering_ref.json").write_text(json.dumps(out, indent=1) + "\n")
    np.savez_compressed(HERE / "clustering_bundle.npz", features=feats, paths=paths, is_labeled=is_labeled,
                        labels=labels, scaler_mean=bundle.scaler_mean, scaler_scale=bundle.scaler_scale,
                        cluster_space=space)
    print("eps", eps_values, "components", space.shape[1])
    for r in km + db:
        print(r.method, r.params, f"ARI={r.ari:.3f} sil={r.silhouette:.4f} noise={r.noise_rate:.3f} "
              f"clusters={len(set(r.labels.tolist()) - {-1})}")


if __name__ == "__main__":
    main()

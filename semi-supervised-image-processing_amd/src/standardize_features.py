"""Standardise the extracted embeddings into the feature bundle the clustering
stage reads — drop-in mirror of the reference's src/standardize_features.py.

Same CLI (--embeddings-npy, --embeddings-csv, --output-npz, --log-level; :66-99)
and the same bundle (:51-59): ``features`` (f32 [N, D], zero mean / unit
variance per column), ``paths``, ``is_labeled``, ``labels`` (empty for
unlabeled rows), ``scaler_mean`` and ``scaler_scale`` (f32 [D]).  The CSV rows
are aligned to the embedding rows through their ``index`` column (:35).

Standardisation is O(N*D) and stays on the host on purpose: sklearn's
StandardScaler gives the reference's features bit for bit.
"""
from __future__ import annotations

import argparse
import logging
from pathlib import Path
from typing import Optional, Sequence

import numpy as np

CSV_COLUMNS = ("index", "path", "bucket", "label")
LABELED = "labeled"


def standardize_embeddings(embeddings_path: Path, csv_path: Path, output_path: Path) -> None:
    import pandas as pd
    from sklearn.preprocessing import StandardScaler

    for what, p in (("Embeddings file", embeddings_path), ("Embeddings CSV", csv_path)):
        if not p.exists():
            raise FileNotFoundError(f"{what} not found: {p}")
    emb = np.load(embeddings_path)
    if emb.ndim != 2:
        raise ValueError(f"Embeddings must be 2D [N, D], got shape {emb.shape}")
    meta = pd.read_csv(csv_path)
    absent = sorted(set(CSV_COLUMNS) - set(meta.columns))
    if absent:
        raise KeyError(f"Embeddings CSV missing columns: {', '.join(absent)}")
    meta = meta.sort_values("index").reset_index(drop=True)
    if len(meta) != emb.shape[0]:
        raise ValueError(f"Row count mismatch between CSV ({len(meta)}) and embeddings ({emb.shape[0]})")

    scaler = StandardScaler()
    z = scaler.fit_transform(emb.astype(np.float32))
    is_labeled = (meta["bucket"].astype(str) == LABELED).to_numpy()
    labels = meta["label"].fillna("").astype(str).where(is_labeled, "").to_numpy()

    output_path.parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(
        output_path,
        features=z.astype(np.float32),
        paths=meta["path"].astype(str).to_numpy(),
        is_labeled=is_labeled,
        labels=labels,
        scaler_mean=np.asarray(scaler.mean_, dtype=np.float32),
        scaler_scale=np.asarray(scaler.scale_, dtype=np.float32),
    )
    logging.info("Wrote standardized bundle: %s (N=%d, D=%d)", output_path, z.shape[0], z.shape[1])


def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    p = argparse.ArgumentParser(
        description="Standardize embeddings and build the feature bundle for clustering "
                    "(outputs/features/embeddings.{npy,csv} -> outputs/features/standardized_features.npz).")
    p.add_argument("--embeddings-npy", type=Path, default=Path("outputs/features/embeddings.npy"),
                   help="Path to embeddings .npy file")
    p.add_argument("--embeddings-csv", type=Path, default=Path("outputs/features/embeddings.csv"),
                   help="Path to embeddings CSV file (paths + labels)")
    p.add_argument("--output-npz", type=Path, default=Path("outputs/features/standardized_features.npz"),
                   help="Path to write the standardized feature bundle")
    p.add_argument("--log-level", type=str, default="INFO", choices=["DEBUG", "INFO", "WARNING", "ERROR"],
                   help="Logging level")
    return p.parse_args(argv)


def main(argv: Optional[Sequence[str]] = None) -> None:
    args = parse_args(argv)
    logging.basicConfig(level=getattr(logging, args.log_level.upper()),
                        format="%(asctime)s [%(levelname)s] %(message)s")
    standardize_embeddings(args.embeddings_npy, args.embeddings_csv, args.output_npz)


if __name__ == "__main__":
    main()

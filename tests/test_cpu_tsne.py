"""CPU: exact t-SNE (ssip.analytics.tsne_fit on the numpy backend) against a
short fp64 restatement of sklearn's exact method, which test_gpu_tsne.py
shares: the perplexity bisection (sklearn/manifold/_utils.pyx), the joint P,
the gradient and KL of ``_kl_divergence`` through an explicit N x N form, and
the ``_gradient_descent`` step."""
import functools
import json
from pathlib import Path

import numpy as np
import pytest

from ssip import analytics as A

GOLD = Path(__file__).resolve().parent / "golden"
MACHINE_EPSILON = np.finfo(np.double).eps  # sklearn's clamp of P and Q


# ---------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------
def blobs(n, d):
    """Four Gaussian blobs, centres x 3, default_rng(0)."""
    rng = np.random.default_rng(0)
    cent = rng.normal(size=(4, d)) * 3
    return (cent[rng.integers(0, 4, n)] + rng.normal(size=(n, d))).astype(np.float32)


def oracle_d2(x):
    x = np.asarray(x, dtype=np.float64)
    return ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)


def oracle_cond_p(d2, perplexity):
    """_binary_search_perplexity, row by row; returns (P, beta of each row)."""
    d2 = np.asarray(d2, dtype=np.float64)
    n = d2.shape[0]
    tiny, tol = float(np.float32(1e-8)), float(np.float32(1e-5))  # C floats in the .pyx
    target = np.log(perplexity)
    P = np.zeros((n, n))
    betas = np.zeros(n)
    for i in range(n):
        lo, hi, beta = -np.inf, np.inf, 1.0
        others = np.arange(n) != i
        for _ in range(100):
            e = np.where(others, np.exp(-d2[i] * beta), 0.0)
            s = e.sum()
            if s == 0.0:
                s = tiny
            P[i] = e / s
            betas[i] = beta
            diff = np.log(s) + beta * (d2[i] * P[i]).sum() - target
            if abs(diff) <= tol:
                break
            if diff > 0.0:
                lo = beta
                beta = beta * 2.0 if hi == np.inf else (beta + hi) / 2.0
            else:
                hi = beta
                beta = beta / 2.0 if lo == -np.inf else (beta + lo) / 2.0
    return P, betas


def oracle_joint_p(cond):
    sym = cond + cond.T
    return sym / sym.sum()


def oracle_terms(P, Y):
    """attr [N][2], rep [N][2], z [N] and the rows of sum P log P - sum P log w."""
    P = np.asarray(P, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    diff = Y[:, None, :] - Y[None, :, :]
    q = 1.0 + (diff ** 2).sum(-1)
    w = 1.0 / q
    np.fill_diagonal(w, 0.0)
    attr = ((P * w)[:, :, None] * diff).sum(1)
    rep = ((w * w)[:, :, None] * diff).sum(1)
    pos = P > 0
    err = np.where(pos, P * (np.log(np.where(pos, P, 1.0)) + np.log(q)), 0.0).sum(1)
    return attr, rep, w.sum(1), err


def oracle_kl(P, Y):
    """_kl_divergence's error over the dense matrices, clamps included."""
    P = np.asarray(P, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    w = 1.0 / (1.0 + ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(-1))
    np.fill_diagonal(w, 0.0)
    off = ~np.eye(P.shape[0], dtype=bool)
    Q = np.maximum(w / w.sum(), MACHINE_EPSILON)
    Pc = np.maximum(P, MACHINE_EPSILON)
    return float((Pc[off] * np.log(Pc[off] / Q[off])).sum())


def oracle_grad(P, Y, exaggeration):
    attr, rep, z, _ = oracle_terms(P, Y)
    return 4.0 * (exaggeration * attr - rep / z.sum())


def oracle_step(grad, Y, upd, gains, momentum, learning_rate, dtype=np.float64):
    """_gradient_descent's step in ``dtype``; returns (Y, update, gains)."""
    f = dtype
    grad, Y, upd, gains = (np.asarray(a, dtype=f) for a in (grad, Y, upd, gains))
    inc = upd * grad < 0
    gains = np.maximum(np.where(inc, gains + f(0.2), gains * f(0.8)), f(0.01))
    upd = f(momentum) * upd - f(learning_rate) * (grad * gains)
    return Y + upd, upd, gains


def oracle_run(P, y0, n_iter, keep=()):
    """The first n_iter iterations of sklearn's schedule; {iteration: Y before it} for ``keep``, and the final Y."""
    n = P.shape[0]
    lr = max(n / 12.0 / 4.0, 50.0)
    Y = np.asarray(y0, dtype=np.float64)
    kept = {}
    for i in range(n_iter):
        if i in (0, 250):
            upd, gains = np.zeros_like(Y), np.ones_like(Y)
        if i in keep:
            kept[i] = Y.copy()
        ex, mom = (12.0, 0.5) if i < 250 else (1.0, 0.8)
        Y, upd, gains = oracle_step(oracle_grad(P, Y, ex), Y, upd, gains, mom, lr)
    return kept, Y


@functools.lru_cache(maxsize=None)
def oracle_case(n, d=8):
    """x, the oracle's joint P and its embeddings at iterations 0, 100 and 400
    (from tests/golden/tsne_oracle_embeddings.npz for the sizes written there
    by make_tsne_goldens.py: the fp64 run is too slow for a test at N >= 1000)."""
    x = blobs(n, d)
    perplexity = 2.0 if n < 32 else 10.0
    P = oracle_joint_p(oracle_cond_p(oracle_d2(x), perplexity)[0])
    y0 = A.tsne_init(x, 42)
    gold = np.load(GOLD / "tsne_oracle_embeddings.npz")
    if f"n{n}_it100" in gold.files:
        ys = {0: y0.astype(np.float64), 100: gold[f"n{n}_it100"], 400: gold[f"n{n}_it400"]}
    else:
        ys, _ = oracle_run(P, y0, 401, keep=(0, 100, 400))
    for a in (x, P, y0, *ys.values()):
        a.setflags(write=False)
    return x, perplexity, P, y0, ys


def rel(got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref).max() / max(float(np.abs(ref).max()), 1e-300))


# ---------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------
def test_oracle_bisection_matches_sklearn():
    from sklearn.manifold._utils import _binary_search_perplexity

    x = blobs(257, 8)
    d2 = oracle_d2(x).astype(np.float32)
    want = _binary_search_perplexity(d2, 10.0, 0)
    got, _ = oracle_cond_p(d2, 10.0)
    assert rel(got, want) <= 1e-12


def test_numpy_backend_matches_the_oracle():
    from scipy.spatial.distance import squareform
    from sklearn.manifold._t_sne import _joint_probabilities

    n, perplexity = 65, 10.0
    x = blobs(n, 8)
    be = A.NumpyBackend(x)
    d2 = oracle_d2(x)
    cond, betas = oracle_cond_p(d2, perplexity)
    be.tsne_cond_p(perplexity)
    assert rel(be.tsne_p(), cond) <= 1e-12 and rel(be.beta, betas) <= 1e-12
    assert (np.diag(be.tsne_p()) == 0).all()
    be.tsne_joint_p()
    P = oracle_joint_p(cond)
    assert rel(be.tsne_p(), P) <= 1e-12
    sk = squareform(_joint_probabilities(d2, perplexity, 0))
    assert rel(be.tsne_p(), sk) <= 1e-6  # sklearn rounds the distances to float32 first

    rng = np.random.default_rng(3)
    y = rng.normal(size=(n, 2))
    upd = rng.normal(size=(n, 2)) * 1e-2
    upd[::7] = 0.0
    gains = rng.uniform(0.05, 2.0, size=(n, 2))
    gains[0] = 0.011  # update is 0 there: * 0.8 takes it below the floor
    be.tsne_begin(y)
    be.upd, be.gains = upd.copy(), gains.copy()
    be.tsne_grad(True)
    be.tsne_step(12.0, 0.5, 50.0)
    attr, rep, z, err = oracle_terms(P, y)
    t = be.tsne_terms()
    for name, ref in (("attr", attr), ("rep", rep), ("z", z), ("err", err), ("grad", oracle_grad(P, y, 12.0))):
        assert rel(t[name], ref) <= 1e-12, name
    Z, kl, gnorm, gained = be.tsne_scalars()
    assert abs(Z - z.sum()) <= 1e-12 * z.sum()
    assert abs(kl - (err.sum() + np.log(z.sum()))) <= 1e-12 * abs(kl)
    assert abs(kl - oracle_kl(P, y)) <= 1e-9 * abs(kl)  # sklearn's clamps at 2.2e-16 move it by less than this
    y1, u1, g1 = oracle_step(oracle_grad(P, y, 12.0), y, upd, gains, 0.5, 50.0)
    assert rel(be.tsne_embedding(), y1) <= 1e-12 and rel(be.upd, u1) <= 1e-12 and rel(be.gains, g1) <= 1e-12
    assert g1.min() == 0.01  # the floor was hit
    assert abs(gnorm - np.linalg.norm(oracle_grad(P, y, 12.0))) <= 1e-12 * gnorm
    assert abs(gained - np.linalg.norm(oracle_grad(P, y, 12.0) * g1)) <= 1e-12 * gained


def test_numpy_backend_survives_rows_whose_exponentials_underflow():
    x = blobs(65, 8) * 100.0
    d2 = oracle_d2(x)
    assert d2[~np.eye(65, dtype=bool)].min() > 1e4
    be = A.NumpyBackend(x)
    be.tsne_cond_p(10.0)
    cond, betas = oracle_cond_p(d2, 10.0)
    assert (betas < 1.0).all() and rel(be.tsne_p(), cond) <= 1e-12
    assert np.abs(be.tsne_p().sum(axis=1) - 1.0).max() <= 1e-12


class _Recorder:
    """Backend stub: records the calls of tsne_fit and reports a slowly falling error."""

    def __init__(self, gained_norm=1.0):
        self.calls = []
        self.errors = 0
        self.gained_norm = gained_norm

    def tsne_cond_p(self, perplexity):
        self.calls.append(("cond_p", perplexity))

    def tsne_joint_p(self):
        self.calls.append(("joint_p",))

    def tsne_begin(self, y0):
        self.calls.append(("begin", y0.shape, y0.dtype))
        self.y0 = y0

    def tsne_reset(self):
        self.calls.append(("reset",))

    def tsne_grad(self, compute_error):
        self.calls.append(("grad", bool(compute_error)))

    def tsne_step(self, exaggeration, momentum, learning_rate):
        self.calls.append(("step", exaggeration, momentum, learning_rate))

    def tsne_scalars(self):
        self.calls.append(("scalars",))
        self.errors += 1
        return 100.0, 5.0 - 0.01 * self.errors, 1.0, self.gained_norm

    def tsne_embedding(self):
        return self.y0


@pytest.mark.parametrize("n, max_iter", ((300, 1000), (4800, 1000), (300, 1013)))
def test_schedule(n, max_iter):
    x = np.random.default_rng(1).normal(size=(n, 5)).astype(np.float32)
    rec = _Recorder()
    emb, kl, n_iter = A.tsne_fit(x, 30.0, seed=42, max_iter=max_iter, backend=rec)
    assert emb.shape == (n, 2) and emb.dtype == np.float32 and n_iter == max_iter
    assert rec.calls[:3] == [("cond_p", 30.0), ("joint_p",), ("begin", (n, 2), np.float32)]
    assert abs(np.std(rec.y0[:, 0]) - 1e-4) <= 1e-9
    lr = 50.0 if n == 300 else n / 48.0
    it, grads, steps, resets, reads = 0, [], [], [], []
    pending = None
    for c in rec.calls[3:]:
        if c[0] == "reset":
            resets.append(it)
        elif c[0] == "grad":
            grads.append(c[1])
            pending = it
        elif c[0] == "step":
            steps.append(c[1:])
            it += 1
        elif c[0] == "scalars":
            reads.append(pending)
    assert len(grads) == len(steps) == max_iter
    assert resets == [0, 250]  # update and gains start over with each phase
    assert all(s == (12.0, 0.5, lr) for s in steps[:250]) and all(s == (1.0, 0.8, lr) for s in steps[250:])
    want_err = sorted(set(range(49, max_iter, 50)) | {max_iter - 1})
    assert [i for i, g in enumerate(grads) if g] == want_err
    assert reads == want_err  # the only read-backs
    assert kl == 5.0 - 0.01 * len(want_err)


def test_schedule_stops_on_the_gradient_norm_and_on_no_progress():
    x = np.random.default_rng(1).normal(size=(300, 5)).astype(np.float32)
    rec = _Recorder(gained_norm=1e-8)
    _, _, n_iter = A.tsne_fit(x, 30.0, backend=rec)
    # sklearn: the first phase ends at its first check, the second starts right after and ends at its first
    assert n_iter == 100 and [c for c in rec.calls if c[0] == "step"][50][1:3] == (1.0, 0.8)

    class Flat(_Recorder):
        def tsne_scalars(self):
            self.calls.append(("scalars",))
            return 100.0, 5.0, 1.0, 1.0

    rec = Flat()
    _, _, n_iter = A.tsne_fit(x, 30.0, backend=rec)
    # best error at iteration 299 (the first check of phase two); 649 is the first check more than 300 later
    assert n_iter == 650


def test_tsne_fit_rejects_what_it_cannot_do():
    x = np.zeros((5, 3), dtype=np.float32)
    with pytest.raises(ValueError, match="perplexity"):
        A.tsne_fit(x, 5.0, device="cpu")
    with pytest.raises(ValueError, match="N <="):
        A.tsne_fit(np.zeros((A.TSNE_MAX_N + 1, 2), dtype=np.float32), 5.0, backend=_Recorder())


def test_entry_points_reject_sizes_outside_the_cap():
    """An argument error, not a fault: checked before any launch, so it needs no device."""
    from ssip import _lib

    lib = _lib.lib()
    assert lib.ssip_tsne_workspace_bytes(1506) > 0 and lib.ssip_tsne_workspace_bytes(A.TSNE_MAX_N) > 0
    for n in (1, 0, -5, A.TSNE_MAX_N + 1):
        assert lib.ssip_tsne_workspace_bytes(n) == -1
        assert b"outside 2.." in lib.ssip_last_error()
        assert lib.ssip_tsne_cond_p(n, 8, 16, 10.0, 16, 16, None) == -1
        assert lib.ssip_tsne_joint_p(n, 16, 16, 1 << 30, None) == -1
        assert lib.ssip_tsne_grad(n, 16, 16, 0, 16, 1 << 30, None) == -1
        assert lib.ssip_tsne_update(n, 16, 1 << 30, 16, 16, 16, 1.0, 0.5, 50.0, 16, None) == -1
    need = lib.ssip_tsne_workspace_bytes(300)
    assert lib.ssip_tsne_grad(300, 16, 16, 0, 16, need - 1, None) == -3  # SSIP_ERR_WORKSPACE


def run_cli(root, device, method, tag):
    """src.clustering on the golden bundle with the golden's grids and --tsne-method; returns the output root."""
    from src import clustering as C
    from test_cpu_analytics import load_gold

    gold, z = load_gold()
    npz = root / "standardized_features.npz"
    np.savez_compressed(npz, **{k: z[k] for k in z.files if k != "cluster_space"})
    out = root / tag
    C.main(["--features-npz", str(npz), "--output-root", str(out), "--device", device, "--log-level", "WARNING",
            "--tsne-method", method,
            "--kmeans-range", *map(str, gold["kmeans_range"]), "--kmeans-n-init", str(gold["kmeans_n_init"]),
            "--tsne-perplexities", "10", "--umap-neighbors", "--umap-min-dist",
            "--dbscan-eps", *(repr(e) for e in gold["dbscan_eps"]),
            "--dbscan-min-samples", *map(str, gold["dbscan_min_samples"]), "--seed", str(gold["seed"])])
    return out


def check_tsne_artefact(out, n):
    emb_dir = out / "features" / "dimensionality_reduction"
    assert sorted(p.name for p in emb_dir.iterdir()) == ["pca_2d.npz", "pca_cluster.npz", "pca_tsne_init.npz",
                                                         "tsne_perp10.npz"]
    ts = np.load(emb_dir / "tsne_perp10.npz")
    assert sorted(ts.files) == ["embedding", "params_json"]
    assert ts["embedding"].shape == (n, 2) and np.isfinite(ts["embedding"]).all()
    assert json.loads(str(ts["params_json"])) == {"perplexity": 10.0, "seed": 42}
    assert (out / "figures" / "tsne2d_clusters.png").stat().st_size > 0
    return ts["embedding"]


def test_cli_flag_and_exact_method_on_the_host(tmp_path):
    from sklearn.manifold import trustworthiness

    from src import clustering as C
    from test_cpu_analytics import load_gold

    assert C.parse_args(["--features-npz", "x.npz"]).tsne_method == "barnes_hut"
    assert C.parse_args(["--features-npz", "x.npz", "--tsne-method", "exact"]).tsne_method == "exact"
    gold, z = load_gold()
    assert gold["seed"] == 42
    emb = check_tsne_artefact(run_cli(tmp_path, "cpu", "exact", "out"), z["features"].shape[0])
    pca = C.run_pca(z["features"], gold["variance_target"], gold["tsne_dim"], gold["seed"])
    assert trustworthiness(pca.pca_tsne_init.data, emb, n_neighbors=10) > 0.8  # an embedding, not noise


def test_cli_falls_back_above_the_cap(monkeypatch, caplog):
    from src import clustering as C

    monkeypatch.setattr(A, "TSNE_MAX_N", 50)
    base = C.EmbeddingResult("pca_tsne_init", blobs(60, 4), {})
    with caplog.at_level("WARNING"):
        out = C.run_tsne(base, [5.0], 42, "exact", "cpu")
    assert "Barnes-Hut" in caplog.text and out[0].name == "tsne_perp5" and out[0].data.shape == (60, 2)

"""GPU: the exact t-SNE kernels (csrc/tsne.hip) and ``ssip.analytics.tsne_fit``
on the device against the fp64 oracle of test_cpu_tsne.py.

Tolerances.  Zero diagonals, the symmetry of the joint P, the update rule and
run-to-run reproducibility are exact.  Row sums (1e-6), row entropies (2e-5)
and the quality bounds (KL <= 1.05 x sklearn exact, trustworthiness no more
than 0.02 below) are fixed ahead of any run.  The remaining floating-point
outputs are held to 4x the largest difference measured on an MI355X against
the fp64 oracle over all cases of the test (each test prints ``MEASURED <name>
<value>``; run with -s to see them), and never to more than the cap:

                                   measured    cap
    conditional P                  1.983e-05   1e-4   max |dP| / max P
    joint P                        6.062e-08   1e-4
    attr                           3.548e-07   1e-4   max |d| / max |ref|
    rep                            1.839e-07   1e-4
    Z                              3.594e-08   1e-4   relative
    KL                             3.211e-06   1e-4   relative
    gradient                       3.226e-07   1e-4   max |d grad| / (4 max (|ex attr| + |rep / Z|))
    Y after five iterations        9.400e-07   1e-3   max |dY| / max |Y|

The margin of 4 is there because the fp32 fixed-order sums move with the
number of column splits, which is a function of N.  The conditional P's
figure is set by one case (n65_d50); the others sit at 5e-8 to 8e-6.  A
difference of that size is what one bisection step more or less on a row
gives, which the fp32 distances can cause where the entropy lands within
rounding of the 1e-5 stop.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MEASURED = {"cond": 1.983e-5, "joint": 6.062e-8, "attr": 3.548e-7, "rep": 1.839e-7, "Z": 3.594e-8, "KL": 3.211e-6,
            "grad": 3.226e-7, "traj": 9.400e-7}
CAP = {"cond": 1e-4, "joint": 1e-4, "attr": 1e-4, "rep": 1e-4, "Z": 1e-4, "KL": 1e-4, "grad": 1e-4, "traj": 1e-3}
BOUND = {k: min(4 * MEASURED[k], CAP[k]) for k in CAP}

GRAD_NS = (5, 64, 65, 257, 1030, 1570)  # 1570: 2 rows past a row block of 32, 13 splits of 2 column tiles, the last of 1

_worst = {}


def _measure(name, value):
    _worst[name] = max(_worst.get(name, 0.0), float(value))
    print(f"MEASURED {name} {value:.3e} (worst so far {_worst[name]:.3e}, bound {BOUND[name]:.3e})")
    return float(value)


def _cond_inputs():
    from test_cpu_tsne import blobs

    cases = {f"n{n}_d{d}": (blobs(n, d), 2.0 if n == 5 else 10.0) for n in (5, 64, 65, 257) for d in (2, 50)}
    dup = blobs(65, 8).copy()
    dup[33:] = dup[:32]  # every point but one has a twin at distance 0
    cases["duplicates"] = (dup, 10.0)
    cases["underflow"] = (blobs(65, 8) * np.float32(100.0), 10.0)
    return cases


COND_CASES = tuple(_cond_inputs())


@functools.lru_cache(maxsize=None)
def _cond_case(name):
    from test_cpu_tsne import oracle_cond_p, oracle_d2

    x, perplexity = _cond_inputs()[name]
    d2 = oracle_d2(x)
    cond, betas = oracle_cond_p(d2, perplexity)
    for a in (x, d2, cond, betas):
        a.setflags(write=False)
    return x, perplexity, d2, cond, betas


def _device_cond(A, x, perplexity):
    be = A.DeviceBackend(x)
    be.tsne_cond_p(perplexity)
    return be, be.tsne_p()


@pytest.mark.parametrize("name", COND_CASES)
def test_conditional_p(dev, name):
    from ssip import analytics as A
    from test_cpu_tsne import rel

    x, perplexity, d2, ref, ref_beta = _cond_case(name)
    n = x.shape[0]
    off = ~np.eye(n, dtype=bool)
    if name == "underflow":
        assert d2[off].min() > 1e4 and np.exp(-d2[off].min()) == 0.0 and (ref_beta < 1.0).all()
    if name == "duplicates":
        assert (np.sort(d2, axis=1)[:, 1] == 0).sum() == 64
    be, P = _device_cond(A, x, perplexity)
    assert P.dtype == np.float32 and P.shape == (n, n)
    P64 = P.astype(np.float64)
    assert (np.diag(P) == 0).all()
    assert np.abs(P64.sum(axis=1) - 1.0).max() <= 1e-6
    pos = P64 > 0
    entropy = -(np.where(pos, P64 * np.log(np.where(pos, P64, 1.0)), 0.0)).sum(axis=1)
    assert np.abs(entropy - np.log(perplexity)).max() <= 2e-5
    err = _measure("cond", rel(P64, ref))
    assert err <= BOUND["cond"]
    assert rel(be._beta.cpu().numpy(), ref_beta) <= 1e-3  # the same search, not another root


@pytest.mark.parametrize("name", ("n5_d2", "n64_d50", "n65_d2", "n257_d50", "duplicates"))
def test_joint_p(dev, name):
    from ssip import analytics as A
    from test_cpu_tsne import oracle_joint_p, rel

    x, perplexity, _, _, _ = _cond_case(name)
    be, cond = _device_cond(A, x, perplexity)
    be.tsne_joint_p()
    P = be.tsne_p()
    assert P.tobytes() == np.ascontiguousarray(P.T).tobytes()
    assert (np.diag(P) == 0).all()
    assert abs(P.astype(np.float64).sum() - 1.0) <= 1e-6
    err = _measure("joint", rel(P, oracle_joint_p(cond.astype(np.float64))))
    assert err <= BOUND["joint"]


def _device_with_p(A, x, P32):
    import torch

    be = A.DeviceBackend(x)
    be._tsne_alloc()
    be.P.copy_(torch.from_numpy(P32))
    return be


@pytest.mark.parametrize("n", GRAD_NS)
def test_gradient(dev, n):
    from ssip import analytics as A
    from test_cpu_tsne import oracle_case, oracle_kl, oracle_terms, rel

    x, _, P, _, ys = oracle_case(n)
    P32 = P.astype(np.float32)
    P64 = P32.astype(np.float64)
    be = _device_with_p(A, x, P32)
    assert sorted(ys) == [0, 100, 400]
    for it, Y in ys.items():
        Y32 = Y.astype(np.float32)
        attr, rep, z, _ = oracle_terms(P64, Y32)
        Z, kl = float(z.sum()), oracle_kl(P64, Y32)
        for ex in (12.0, 1.0):
            be.tsne_begin(Y32)
            be.tsne_grad(True)
            be.tsne_step(ex, 0.5, 50.0)
            t = be.tsne_terms()
            dZ, dkl, gnorm, _ = be.tsne_scalars()
            grad = 4.0 * (ex * attr - rep / Z)
            scale = 4.0 * float((np.abs(ex * attr) + np.abs(rep / Z)).max())
            e = {"attr": rel(t["attr"], attr), "rep": rel(t["rep"], rep), "Z": abs(dZ - Z) / Z,
                 "KL": abs(dkl - kl) / abs(kl), "grad": float(np.abs(t["grad"] - grad).max() / scale)}
            for k, v in e.items():
                _measure(k, v)
            assert all(v <= BOUND[k] for k, v in e.items()), (n, it, ex, e)
            assert abs(gnorm - np.linalg.norm(t["grad"].astype(np.float64))) <= 1e-12 * gnorm


def test_update_is_the_numpy_rule_in_float32(dev):
    import torch

    from ssip import analytics as A
    from test_cpu_tsne import oracle_case, oracle_step

    n = 257
    x, _, P, _, ys = oracle_case(n)
    be = _device_with_p(A, x, P.astype(np.float32))
    rng = np.random.default_rng(9)
    Y0 = ys[100].astype(np.float32)
    upd0 = (rng.normal(size=(n, 2)) * 0.3).astype(np.float32)
    upd0[::5] = 0.0  # update * grad is exactly 0: not an increase
    gains0 = rng.uniform(0.05, 3.0, size=(n, 2)).astype(np.float32)
    gains0[::3] = np.float32(0.0101)  # * 0.8 falls below the 0.01 floor wherever update * grad >= 0
    for ex, mom, lr in ((12.0, 0.5, 50.0), (1.0, 0.8, 133.25)):
        be.tsne_begin(Y0)
        be.upd.copy_(torch.from_numpy(upd0))
        be.gains.copy_(torch.from_numpy(gains0))
        be.tsne_grad(False)
        be.tsne_step(ex, mom, lr)
        grad = be.tsne_terms()["grad"]
        assert grad.dtype == np.float32
        Y1, upd1, gains1 = oracle_step(grad, Y0, upd0, gains0, mom, lr, dtype=np.float32)
        assert Y1.dtype == np.float32
        inc = upd0 * grad < 0
        assert inc.any() and (~inc).any() and (gains1 == np.float32(0.01)).any() and (upd0 * grad == 0).any()
        assert be.gains.cpu().numpy().tobytes() == gains1.tobytes()
        assert be.upd.cpu().numpy().tobytes() == upd1.tobytes()
        assert be.Y.cpu().numpy().tobytes() == Y1.tobytes()


def test_five_iterations_follow_the_oracle(dev):
    from ssip import analytics as A
    from test_cpu_tsne import oracle_case, oracle_run, rel

    x, perplexity, P, y0, _ = oracle_case(257)
    emb, kl, n_iter = A.tsne_fit(x, perplexity, seed=42, max_iter=5, device="cuda")
    assert n_iter == 5 and emb.dtype == np.float32 and np.isfinite(kl)
    _, want = oracle_run(P, y0, 5)
    err = _measure("traj", rel(emb, want))
    assert err <= BOUND["traj"]


def test_fit_is_bit_reproducible(dev):
    from ssip import analytics as A
    from test_cpu_tsne import blobs

    x = blobs(257, 8)
    a = A.tsne_fit(x, 10.0, max_iter=300, device="cuda")
    b = A.tsne_fit(x, 10.0, max_iter=300, device="cuda")
    assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1] and a[2] == b[2] == 300


@pytest.mark.parametrize("n, d, perplexity", ((257, 8, 10.0), (300, 50, 30.0)))
def test_whole_fit_is_as_good_as_sklearn_exact(dev, n, d, perplexity):
    """Measured on an MI355X, both KLs by ``oracle_kl`` over the oracle's joint P:
    (257, 8, 10):  KL 0.650465 against sklearn exact's 0.635177, ratio 1.0241; trustworthiness 0.9721 against 0.9726;
    (300, 50, 30): KL 0.571598 against 0.571887, ratio 0.9995; trustworthiness 0.9510 against 0.9518."""
    from sklearn.manifold import TSNE, trustworthiness

    from ssip import analytics as A
    from test_cpu_tsne import blobs, oracle_cond_p, oracle_d2, oracle_joint_p, oracle_kl

    x = blobs(n, d)
    P = oracle_joint_p(oracle_cond_p(oracle_d2(x), perplexity)[0])
    emb, kl, n_iter = A.tsne_fit(x, perplexity, seed=42, max_iter=1000, device="cuda")
    sk = TSNE(method="exact", init="pca", random_state=42, learning_rate="auto", perplexity=perplexity).fit_transform(x)
    kl_dev, kl_sk = oracle_kl(P, emb), oracle_kl(P, sk)
    t_dev, t_sk = trustworthiness(x, emb, n_neighbors=10), trustworthiness(x, sk, n_neighbors=10)
    print(f"MEASURED quality n={n}: KL device {kl_dev:.6f} sklearn exact {kl_sk:.6f} ratio {kl_dev / kl_sk:.4f}; "
          f"trustworthiness device {t_dev:.4f} sklearn {t_sk:.4f}; reported kl {kl:.6f}, {n_iter} iterations")
    assert np.isfinite(emb).all() and emb.shape == (n, 2)
    assert kl_dev <= 1.05 * kl_sk
    assert t_dev >= t_sk - 0.02
    assert abs(kl - kl_dev) <= 1e-2 * kl_dev  # the reported error is that of the iterate before the last step


def test_clustering_cli_exact_tsne_on_the_device(dev, tmp_path):
    from test_cpu_analytics import load_gold
    from test_cpu_tsne import check_tsne_artefact, run_cli

    _, z = load_gold()
    exact = run_cli(tmp_path, "cuda", "exact", "exact")
    check_tsne_artefact(exact, z["features"].shape[0])
    bh = run_cli(tmp_path, "cuda", "barnes_hut", "bh")
    check_tsne_artefact(bh, z["features"].shape[0])
    # t-SNE feeds no clustering decision: nothing else moved
    for table in ("metrics_clustering.csv", "cluster_assignments.csv"):
        assert (exact / "tables" / table).read_bytes() == (bh / "tables" / table).read_bytes()

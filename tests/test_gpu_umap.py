"""GPU: the native UMAP kernels (csrc/umap.hip) and ``ssip.analytics.umap_fit``
on the device against the fp64 oracles of test_cpu_umap.py.

Tolerances.  The kNN order and tie rule, the prefix property, rho, the zero
self column, the float32 schedule state, the set of edges that fire, the
untouched input buffer and run-to-run reproducibility are exact.  The kNN
exemption (rows whose k-th and (k+1)-th fp64 squared distances differ by less
than 1e-5 relative, at most 2 % of a case's rows) and the quality bounds
(trustworthiness strictly above pca_2d's and no more than 0.02 below the
lowest of the sequential oracle's three seeds) are fixed ahead of any run.  The
remaining floating-point outputs are held to 4x the largest difference measured
on an MI355X against the fp64 oracle over all cases of the test (each test
prints ``MEASURED <name> <value>``; run with -s to see them), and never to
more than the cap:

                                   measured    cap
    kNN squared distances          3.614e-07 1e-4   max |d| / max |ref|
    sigma                          5.362e-11 1e-4   max |d| / max |ref|
    memberships                    2.980e-08 1e-4
    y after one epoch              4.992e-08 1e-4   max |dy| / max |y|
    y after five epochs            5.783e-04 1e-3

The margin of 4 is there because the fp32 fixed-order sums move with the row
length (the number of features for a distance, of edges for a vertex).  sigma
is mostly exact: a bisection of a few dozen steps ends on a dyadic number that
float32 holds.  The five-epoch figure is set by two cases (n257 and n1030 from
epoch 100; the others sit at 2e-7 to 5e-5) and is the float32 rounding of the
positions, amplified about tenfold per epoch by the map itself: the numpy
backend, with fp64 forces and float32 positions, gives the same 5.78e-4 there.
With float32 forces in the kernel that case measured 1.23e-3, above the cap,
which is why the kernel computes the forces in fp64.  On the kNN cases the
oracle exempted at most 7 of 1,030 rows (n1030_d50, k = 64), 1 row in two other
cases and none elsewhere, and no row differed at all.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MEASURED = {"knn": 3.614e-7, "sigma": 5.362e-11, "memb": 2.980e-8, "epoch": 4.992e-8, "traj": 5.783e-4}
CAP = {"knn": 1e-4, "sigma": 1e-4, "memb": 1e-4, "epoch": 1e-4, "traj": 1e-3}
BOUND = {k: min(4 * MEASURED[k], CAP[k]) for k in CAP}

KNN_NS, KNN_DS, KNN_KS = (5, 64, 65, 257, 1030), (2, 50), (2, 15, 64)
KNN_CASES = tuple(f"n{n}_d{d}" for n in KNN_NS for d in KNN_DS)
EPOCH_NS = (5, 64, 65, 257, 1030)
EXEMPT_GAP, EXEMPT_ROWS = 1e-5, 0.02

_worst = {}


def _measure(name, value):
    _worst[name] = max(_worst.get(name, 0.0), float(value))
    print(f"MEASURED {name} {value:.3e} (worst so far {_worst[name]:.3e}, bound {BOUND[name]:.3e})")
    return float(value)


@functools.lru_cache(maxsize=None)
def _knn_case(name):
    """(x, the full fp64 squared distances, their stable argsort)."""
    from test_cpu_umap import knn_input, oracle_d2

    x = knn_input(name)
    full = oracle_d2(x)
    order = np.argsort(full, axis=1, kind="stable")
    for a in (x, full, order):
        a.setflags(write=False)
    return x, full, order


@functools.lru_cache(maxsize=None)
def _device_knn(name, k):
    from ssip import analytics as A

    x, _, _ = _knn_case(name)
    d2, idx = A.knn_graph(x, k, device="cuda")
    d2.setflags(write=False)
    idx.setflags(write=False)
    return d2, idx


def _ks(n):
    return tuple(k for k in KNN_KS if k <= n)


@pytest.mark.parametrize("name", KNN_CASES + ("duplicates",))
def test_knn(dev, name):
    from test_cpu_umap import rel

    x, full, order = _knn_case(name)
    n = x.shape[0]
    first_twin = (full == 0).argmax(axis=1)  # the row itself, or its lowest-index exact duplicate
    for k in _ks(n):
        d2, idx = _device_knn(name, k)
        assert d2.dtype == np.float32 and idx.dtype == np.int32 and d2.shape == idx.shape == (n, k)
        assert idx.min() >= 0 and idx.max() < n
        assert all(np.unique(row).size == k for row in idx)
        # each distance is that of its index
        err = _measure("knn", rel(d2, np.take_along_axis(full, idx.astype(np.int64), axis=1)))
        assert err <= BOUND["knn"]
        # ascending, equal distances by index
        gap, step = np.diff(d2, axis=1), np.diff(idx, axis=1)
        assert ((gap > 0) | ((gap == 0) & (step > 0))).all()
        assert (idx[:, 0] == first_twin).all() and (d2[:, 0] == 0).all()
        # the oracle's index sets, but for rows it cannot decide itself
        want = order[:, :k]
        srt = np.take_along_axis(full, order, axis=1)
        # (an exact tie, as between twins, is no such row: float32 ties there too and the index decides)
        tail = srt[:, k] - srt[:, k - 1] if k < n else np.ones(n)
        exempt = (tail > 0) & (tail < EXEMPT_GAP * srt[:, min(k, n - 1)])
        same = np.array([set(a) == set(b) for a, b in zip(idx.tolist(), want.tolist())])
        print(f"{name} k={k}: {int(exempt.sum())} rows exempt, {int((~same).sum())} rows differ")
        assert exempt.mean() <= EXEMPT_ROWS
        assert same[~exempt].all()
    if name == "duplicates":
        d2, idx = _device_knn(name, 15)
        assert (d2[:, 1] == 0).sum() == 64 and (gap == 0).any()
        assert (idx[33:, 0] == np.arange(32)).all() and (idx[33:, 1] == np.arange(33, 65)).all()
    if n >= 64:
        wide, narrow = _device_knn(name, 64), _device_knn(name, 15)
        assert np.ascontiguousarray(wide[0][:, :15]).tobytes() == narrow[0].tobytes()
        assert np.ascontiguousarray(wide[1][:, :15]).tobytes() == narrow[1].tobytes()


@pytest.mark.parametrize("name", KNN_CASES + ("duplicates", "all_duplicates", "scaled"))
def test_fuzzy(dev, name):
    from ssip import analytics as A
    from test_cpu_umap import oracle_smooth_knn, rel

    x, _, _ = _knn_case(name)
    n = x.shape[0]
    be = A.DeviceBackend(x)
    kmax = max(_ks(n))
    d2, idx = be.knn(kmax)
    for k in _ks(n):
        # the device's own distances: sqrt in float32, correctly rounded
        dist = np.sqrt(d2[:, :k]).astype(np.float32)
        rho, sigma, memb = oracle_smooth_knn(dist.astype(np.float64), idx[:, :k])
        got_rho, got_sigma, got_memb = be.umap_fuzzy(k)  # a slice of the kmax result
        assert got_rho.dtype == got_sigma.dtype == got_memb.dtype == np.float32 and got_memb.shape == (n, k)
        assert np.array_equal(got_rho, rho.astype(np.float32))
        own = idx[:, :k] == np.arange(n)[:, None]
        assert (got_memb[own] == 0).all() and (got_memb >= 0).all() and (got_memb <= 1).all()
        if name == "all_duplicates" and k == 15:
            assert (got_rho[:20] == 0).all() and (got_rho[20:] > 0).all() and (got_memb[:20][~own[:20]] == 1).all()
        e_sigma, e_memb = _measure("sigma", rel(got_sigma, sigma)), _measure("memb", rel(got_memb, memb))
        assert e_sigma <= BOUND["sigma"] and e_memb <= BOUND["memb"], (name, k)


def _device_epochs(A, n, start, count, seed=42):
    """count epochs from `start` on the device; (backend, y after each, the state before the first)."""
    from test_cpu_umap import AB, epoch_case, state_at

    csr, y0 = epoch_case(n)
    state = state_at(csr, start)
    be = A.DeviceBackend(np.zeros((n, 1), dtype=np.float32))
    be.umap_begin(csr, y0, *AB[0.1], seed, state=state)
    ys = []
    for ep in range(start, start + count):
        be.umap_epoch(ep, 1.0 - ep / 500)
        ys.append(be.umap_embedding())
    return be, ys, state


@pytest.mark.parametrize("n", EPOCH_NS)
def test_one_epoch(dev, n):
    from ssip import analytics as A
    from test_cpu_umap import AB, epoch_case, oracle_epoch, rel

    csr, y0 = epoch_case(n)
    a, b = (float(np.float32(v)) for v in AB[0.1])
    rows = np.diff(csr[0])
    assert rows.max() == n - 1 and csr[2].min() == 1.0 and csr[2].max() > (10.0 if n > 5 else 1.0)
    assert (y0[1] == y0[2]).all()  # at n >= 257 the hub row is longer than a wave
    for ep in (1, 7, 30):  # 1: only the w = max edges fire
        be, ys, (ns, nn) = _device_epochs(A, n, ep, 1)
        before = ns.copy()
        want, fire = oracle_epoch(csr, y0, ns, nn, ep, 1.0 - ep / 500, a, b, 42)  # advances ns, nn
        got_ns, got_nn = be.umap_state()
        assert got_ns.tobytes() == ns.tobytes() and got_nn.tobytes() == nn.tobytes()
        assert np.array_equal(got_ns != before, fire) and fire.any() and (n == 5 or not fire.all())
        assert be._u_y2.cpu().numpy().tobytes() == y0.tobytes()  # the buffer the epoch read
        assert ys[0].dtype == np.float32 and _measure("epoch", rel(ys[0], want)) <= BOUND["epoch"], (n, ep)


@pytest.mark.parametrize("n", EPOCH_NS)
@pytest.mark.parametrize("start", (0, 100))
def test_five_epochs_follow_the_oracle(dev, n, start):
    from ssip import analytics as A
    from test_cpu_umap import AB, epoch_case, oracle_epoch, rel

    csr, y0 = epoch_case(n)
    a, b = (float(np.float32(v)) for v in AB[0.1])
    be, ys, (ns, nn) = _device_epochs(A, n, start, 5)
    want = y0.astype(np.float64)
    for ep in range(start, start + 5):
        want, _ = oracle_epoch(csr, want, ns, nn, ep, 1.0 - ep / 500, a, b, 42)
    got_ns, got_nn = be.umap_state()
    assert got_ns.tobytes() == ns.tobytes() and got_nn.tobytes() == nn.tobytes()
    assert np.abs(want - y0).max() > 1e-3  # something moved
    assert _measure("traj", rel(ys[-1], want)) <= BOUND["traj"]


def test_fit_is_bit_reproducible(dev):
    from ssip import analytics as A
    from test_cpu_umap import six_blobs

    x = six_blobs(300, 50)
    a, info_a = A.umap_fit(x, 15, 0.1, seed=0, n_epochs=200, device="cuda")
    b, info_b = A.umap_fit(x, 15, 0.1, seed=0, n_epochs=200, device="cuda")
    assert a.tobytes() == b.tobytes() and info_a == info_b and info_a["n_epochs"] == 200
    knn = A.knn_graph(x, 64, device="cuda")
    c, _ = A.umap_fit(x, 15, 0.1, seed=0, n_epochs=200, device="cuda", knn=knn)
    assert c.tobytes() == a.tobytes()
    d, _ = A.umap_fit(x, 15, 0.1, seed=1, n_epochs=200, device="cuda")
    assert d.tobytes() != a.tobytes()


@pytest.mark.parametrize("q", (0, 1))
def test_whole_fit_quality(dev, q):
    """Trustworthiness (15 neighbours) measured on an MI355X, seed 0, PCA init:
    six_blobs (k = 15) 0.9685 against the sequential oracle's 0.9683..0.9696 and pca_2d's 0.9145;
    tsne_blobs (k = 30) 0.9371 against 0.9357..0.9390 and 0.9236."""
    from ssip import analytics as A
    from test_cpu_umap import check_quality, golden_inputs

    name, x, k = golden_inputs()[q]
    emb, info = A.umap_fit(x, k, 0.1, seed=0, init="pca", device="cuda")
    assert info["init"] == "pca" and info["n_epochs"] == 500
    check_quality(q, x, emb)


def test_whole_fit_quality_from_the_spectral_init(dev):
    """Measured on an MI355X (six_blobs, k = 50, spectral init): 0.9635 against the sequential oracle's
    0.9683..0.9696 (k = 15, PCA init) and pca_2d's 0.9145."""
    from ssip import analytics as A
    from test_cpu_umap import check_quality, golden_inputs

    name, x, k = golden_inputs()[0]
    emb, info = A.umap_fit(x, 50, 0.1, seed=0, init="spectral", device="cuda")
    assert info["init"] == "spectral"
    check_quality(0, x, emb)


def test_clustering_cli_native_umap_on_the_device(dev, tmp_path):
    from test_cpu_analytics import load_gold
    from test_cpu_umap import check_umap_artefacts, run_cli

    _, z = load_gold()
    check_umap_artefacts(run_cli(tmp_path, "cuda", "native", "out"), z["features"].shape[0])

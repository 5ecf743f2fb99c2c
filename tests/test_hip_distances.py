"""Stage A distances on the MI355X (jamie_amd/distances.py, csrc/distances.hip) against the host path's scipy / sklearn
arithmetic in float64.  Run on the GPU box:  pytest -m gpu"""
import ast
import contextlib
import io
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), 'golden')
# |dD| <= EUC_TOL * max(D): fp32 rounding of the centred Gram form (||x_i||^2 + ||x_j||^2 - 2 G_ij)
EUC_TOL = 1e-5


@pytest.fixture(scope='module')
def jd():
    from jamie_amd import _native
    _native.require_gpu()
    from jamie_amd import distances
    return distances


def _far_clusters():
    """test_host_cpu.test_geodesic_distances_properties' data: two clusters of 30 cells in 3-D, 50 apart."""
    rng = np.random.default_rng(0)
    return np.concatenate([rng.standard_normal((30, 3)), rng.standard_normal((30, 3)) + 50.0])


def _host_k(X, kmax):
    """The k utilities.geodesic_distances ends with (its growth loop, restated), clipped to N."""
    import scipy.sparse.csgraph as csgraph
    from sklearn.neighbors import NearestNeighbors
    N, k = len(X), 5

    def graph(k):
        return NearestNeighbors(n_neighbors=min(k, N)).fit(X).kneighbors_graph(X, mode='distance')
    while csgraph.connected_components(graph(k), directed=False)[0] != 1:
        if k > np.max((kmax, 0.01 * N)):
            break
        k += 2
    return min(k, N)


def _check_layout(D, N):
    assert torch.is_tensor(D) and D.is_cuda and D.dtype == torch.float32 and tuple(D.shape) == (N, N)
    h = D.cpu().numpy()
    assert np.array_equal(h, h.T)
    assert (np.diag(h) == 0).all()
    return h


@pytest.mark.parametrize('case', ['d2000', 'far_d3', 'squared'])
def test_euclidean_vs_sklearn(jd, case):
    from sklearn.metrics import pairwise_distances
    rng = np.random.default_rng(11)
    X = _far_clusters() if case == 'far_d3' else rng.standard_normal((700, 2000)) + 3.0
    squared = case == 'squared'
    want = pairwise_distances(X, metric='sqeuclidean' if squared else 'euclidean')
    got = _check_layout(jd.euclidean(X, squared=squared), len(X)).astype(np.float64)
    err = np.abs(got - want).max() / want.max()
    assert err <= EUC_TOL, err


def test_euclidean_takes_a_device_tensor(jd):
    rng = np.random.default_rng(2)
    X = rng.standard_normal((130, 17)).astype(np.float32)
    a = jd.euclidean(X)
    b = jd.euclidean(torch.from_numpy(X).cuda())
    assert torch.equal(a, b)


@pytest.mark.parametrize('N,d,k', [(500, 64, 12), (1200, 2000, 42), (7, 3, 7), (300, 5, 1),
                                   # K > 256: several slots of the key fill and the bitonic sort per thread; 1024 = TOPK_MAX
                                   (3000, 16, 257), (2000, 64, 300), (3000, 8, 513), (3000, 32, 1024)])
def test_knn_vs_argsort(jd, N, d, k):
    from sklearn.metrics import pairwise_distances
    rng = np.random.default_rng(N + d)
    X = rng.standard_normal((N, d))
    idx, w = jd.knn(X, k)
    idx, w = idx.cpu().numpy(), w.cpu().numpy()
    assert idx.shape == (N, k) and w.dtype == np.float32
    assert (idx[:, 0] == np.arange(N)).all() and (w[:, 0] == 0).all()
    D = pairwise_distances(X)
    np.fill_diagonal(D, -1.0)
    order = np.argsort(D, axis=1, kind='stable')
    for i in range(N):
        if set(idx[i]) != set(order[i, :k]):            # only a near-tie between the k-th and (k+1)-th may differ
            s = np.sort(D[i])
            assert abs(s[k] - s[k - 1]) <= 1e-5 * s[k], i
    rows = np.arange(N)[:, None]
    np.testing.assert_allclose(w[:, 1:], D[rows, idx][:, 1:], rtol=1e-6)
    assert (np.diff(D[rows, idx][:, 1:], axis=1) >= -1e-6 * D.max()).all()    # ascending


@pytest.mark.parametrize('N', [1, 2, 63, 64, 65, 1000, 2049, 4096])
def test_apsp_on_the_device_graph_equals_scipy(jd, N):
    import scipy.sparse as sp
    import scipy.sparse.csgraph as csgraph
    rng = np.random.default_rng(N)
    X = rng.standard_normal((N, 6))
    D, k, idx, w = jd.geodesic(X, kmax=7, return_graph=True)
    got = _check_layout(D, N).astype(np.float64)
    if N == 1:
        assert got.tolist() == [[0.0]]
        return
    idx, w = idx.cpu().numpy()[:, 1:k], w.cpu().numpy()[:, 1:k].astype(np.float64)
    g = sp.csr_matrix((w.ravel(), (np.repeat(np.arange(N), k - 1), idx.ravel())), shape=(N, N))
    want = csgraph.shortest_path(g, method='D', directed=False)
    fin = want[np.isfinite(want)]
    want[~np.isfinite(want)] = 2 * (fin.max() if fin.size else 0.0)
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=0)


def _swiss_roll(N=1500):
    from sklearn.datasets import make_swiss_roll
    X, _ = make_swiss_roll(N, noise=0.05, random_state=0)
    return X


@pytest.mark.parametrize('case', ['gaussian', 'two_clusters', 'swiss_roll'])
def test_geodesic_vs_host(jd, case):
    from jamie_amd.utilities import geodesic_distances
    rng = np.random.default_rng(5)
    X, kmax = {'gaussian': (rng.standard_normal((900, 20)), 40), 'two_clusters': (_far_clusters(), 7),
               'swiss_roll': (_swiss_roll(), 10)}[case]
    want = geodesic_distances(X, kmax)
    D, k, _, _ = jd.geodesic(X, kmax, return_graph=True)
    assert k == _host_k(X, kmax)
    got = _check_layout(D, len(X)).astype(np.float64)
    # rtol 1e-5, plus an absolute floor of 1e-7 * max(D): an edge weight comes from fp32 coordinates, whose rounding is relative to
    # the coordinates' size, not to the edge's length; on the swiss roll (coordinates ~10) two of 2.25 M pairs joined by one short
    # edge came out 1.4e-5 relative (4.8e-7 absolute) off the float64 path
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-7 * want.max())
    if case == 'two_clusters':                  # the growth loop ran out: unreachable pairs take 2 * the largest finite distance
        within = max(want[:30, :30].max(), want[30:, 30:].max())
        np.testing.assert_allclose(got[:30, 30:], 2 * within, rtol=1e-6)
    if case == 'swiss_roll':                    # multi-hop paths: far longer than the straight line
        from sklearn.metrics import pairwise_distances
        assert (got / np.maximum(pairwise_distances(X), 1e-12)).max() > 3.0


def test_facade_device_distances_on_the_pd3_pipeline():
    """The pd3 fixture's stage A / B through the facade with distances='device': euclidean distances on the device (float32
    tensors), Prime_Dual straight on them."""
    import jamie_amd
    g = np.load(os.path.join(GOLD, 'pd3_pipeline.npz'))
    m = ast.literal_eval(str(g['meta']))
    with contextlib.redirect_stdout(io.StringIO()):
        jm = jamie_amd.JAMIE(distance_mode='euclidean', epoch_pd=m['epoch_pd'], output_dim=4, batch_size=56, epoch_DNN=12,
                             min_epochs=5, pca_dim=None, use_f_tilde=True, log_DNN=10 ** 9, log_pd=50, distances='device')
        emb = jm.fit_transform(dataset=[g['X'], g['Y']])
    for got, want in zip(jm.dist, (g['dist0'], g['dist1'])):
        assert torch.is_tensor(got) and got.is_cuda and got.dtype == torch.float32
        assert np.abs(got.cpu().numpy() - want).max() <= EUC_TOL * want.max()
    np.testing.assert_allclose(np.asarray(jm.match_result[0]), g['F'], rtol=2e-3, atol=2e-6)
    assert len(emb) == 2 and np.isfinite(emb[0]).all() and np.isfinite(emb[1]).all()


def test_facade_default_geodesic_device_matches_host():
    """The default distance mode (geodesic) on both paths: on data where both choose the same k and kNN sets, F agrees."""
    import jamie_amd
    rng = np.random.default_rng(8)
    Z = rng.standard_normal((160, 4))
    data = [Z @ rng.standard_normal((4, 24)) + 0.1 * rng.standard_normal((160, 24)),
            Z @ rng.standard_normal((4, 16)) + 0.1 * rng.standard_normal((160, 16))]
    out = {}
    for mode in ('host', 'device'):
        with contextlib.redirect_stdout(io.StringIO()):
            jm = jamie_amd.JAMIE(epoch_pd=300, output_dim=4, batch_size=64, epoch_DNN=6, min_epochs=3, pca_dim=None,
                                 log_DNN=10 ** 9, log_pd=10 ** 9, distances=mode)
            jm.fit_transform(dataset=data)
        out[mode] = (jm.dist, np.asarray(jm.match_result[0]))
    for h, d in zip(out['host'][0], out['device'][0]):
        np.testing.assert_allclose(d.cpu().numpy(), h, rtol=1e-5, atol=0)
    np.testing.assert_allclose(out['device'][1], out['host'][1], rtol=2e-3, atol=2e-6)


# ---- duplicates and near-duplicates, exact ties, large K, the K limit, > 4 GiB outputs, inputs ----
from test_host_distances import duplicate_data, tie_rule_geodesic, tie_rule_order   # noqa: E402


@pytest.mark.parametrize('d', [16, 50, 2000])
def test_euclidean_on_near_duplicates(jd, d):
    """The Gram form cancels on (near-)duplicate cells; jamie_gram_to_distances recomputes those pairs by direct difference."""
    from scipy.spatial.distance import cdist
    X = duplicate_data(d)
    want = cdist(X, X)
    got = _check_layout(jd.euclidean(X), len(X)).astype(np.float64)
    err = np.abs(got - want).max() / want.max()
    assert err <= EUC_TOL, err
    assert (got[want == 0] == 0).all()                     # exact duplicates: exactly 0
    sq = jd.euclidean(X, squared=True).cpu().numpy().astype(np.float64)
    assert np.abs(sq - want ** 2).max() <= EUC_TOL * (want ** 2).max() and (sq[want == 0] == 0).all()


@pytest.mark.parametrize('d', [16, 50, 2000])
def test_knn_on_near_duplicates(jd, d):
    """Neighbour sets against exact float64 distances (k = 8 ends inside the groups of 13 near-duplicates)."""
    from scipy.spatial.distance import cdist
    X = duplicate_data(d)
    N, k = len(X), 8
    idx, w = (t.cpu().numpy() for t in jd.knn(X, k))
    assert (idx[:, 0] == np.arange(N)).all() and (w[:, 0] == 0).all()
    D = cdist(X, X)
    np.fill_diagonal(D, -1.0)
    order = np.argsort(D, axis=1, kind='stable')
    for i in range(N):
        if set(idx[i]) != set(order[i, :k]):
            s = np.sort(D[i])
            assert abs(s[k] - s[k - 1]) <= 1e-5 * s[k], i
    rows = np.arange(N)[:, None]
    # weights: rtol 1e-6 plus the fp32 rounding of the centred coordinates (~2^-24 of their size, not of the 0.004 edge)
    np.testing.assert_allclose(w[:, 1:], D[rows, idx][:, 1:], rtol=1e-6, atol=1e-7 * D.max())


@pytest.mark.parametrize('d', [16, 50, 2000])
def test_geodesic_on_near_duplicates(jd, d):
    from jamie_amd.utilities import geodesic_distances
    X = duplicate_data(d)
    want = geodesic_distances(X, 40)
    got = _check_layout(jd.geodesic(X, 40), len(X)).astype(np.float64)
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-7 * want.max())


def _lattice():
    """{-5..5}^3: column means exactly 0, so every centred coordinate, Gram entry and D^2 is an exact integer."""
    g = np.arange(-5, 6, dtype=np.float64)
    return np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3)


def test_knn_exact_ties_on_a_lattice(jd):
    X = _lattice()
    N, k = len(X), 100
    D2 = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)
    idx, w = (t.cpu().numpy() for t in jd.knn(X, k))
    assert np.array_equal(idx, tie_rule_order(D2, k))      # stable order by (value, column), row by row
    np.testing.assert_allclose(w, np.sqrt(D2[np.arange(N)[:, None], idx]), rtol=1e-7, atol=0)


def test_geodesic_exact_ties_on_a_lattice(jd):
    X = _lattice()
    want, k_want = tie_rule_geodesic(X, 40)
    D, k, _, _ = jd.geodesic(X, 40, return_graph=True)
    assert k == k_want
    np.testing.assert_allclose(_check_layout(D, len(X)).astype(np.float64), want, rtol=1e-5, atol=0)


def test_all_equal_rows_select_on_column_digits_only(jd):
    """X = I_2048 (dyadic: the centred Gram is exact): every off-diagonal D is sqrt(2), so each row's select runs on its column
    index digits alone; the geodesic graph of k = 5 is the 4 lowest other indices per cell, every pair one or two edges apart."""
    N = 2048
    X = np.eye(N)
    assert (jd.euclidean(X).cpu().numpy() == np.float32(np.sqrt(2)) * (1 - np.eye(N, dtype=np.float32))).all()
    idx, w = (t.cpu().numpy() for t in jd.knn(X, 1024))
    want = np.array([[i] + [j for j in range(1024) if j != i][:1023] for i in range(N)])
    assert np.array_equal(idx, want)
    assert (w[:, 1:] == np.float32(np.sqrt(2))).all()
    D, k, _, _ = jd.geodesic(X, 1022, return_graph=True)
    assert k == 5
    edge = np.zeros((N, N), bool)
    for i in range(N):
        edge[i, [j for j in range(5) if j != i][:4]] = True
    edge |= edge.T
    r2 = np.float32(np.sqrt(2))
    want = np.where(edge, r2, 2 * r2).astype(np.float32)
    np.fill_diagonal(want, 0)
    assert np.array_equal(_check_layout(D, N), want)


def test_geodesic_kmax_beyond_the_top_k_limit(jd):
    """kmax = 1100 asks for K = 1102 > 1024 top-K slots, but connected data stops the growth loop at k = 5: the device path runs
    and equals the host path.  Data that really needs k > 1024 raises ValueError."""
    from jamie_amd.utilities import geodesic_distances
    rng = np.random.default_rng(12)
    X = rng.standard_normal((3000, 10))
    D, k, idx, _ = jd.geodesic(X, 1100, return_graph=True)
    assert k == 5 and idx.shape == (3000, 1024)
    want = geodesic_distances(X, 1100)
    np.testing.assert_allclose(_check_layout(D, 3000).astype(np.float64), want, rtol=1e-5, atol=1e-7 * want.max())
    far = np.concatenate([rng.standard_normal((1100, 3)), rng.standard_normal((1100, 3)) + 50.0])   # joined only at k > 1100
    with pytest.raises(ValueError, match='1024'):
        jd.geodesic(far, 1200)
    with pytest.raises(ValueError, match='1024'):
        jd.knn(X, 1025)


BIG_N = 33001               # N^2 * 4 bytes = 4.36 GB > 4 GiB; ragged against 64 and 128


def _rows_past_4gib(N, rng, count=16):
    """Sampled rows: the first and last, rows either side of byte offset 2^32 and of the last 128 / 256 tile rows, random rows."""
    edge = (1 << 32) // (4 * N)
    fixed = [0, 1, 127, 128, edge - 1, edge, edge + 1, N - 256 - 1, N - (N % 256), N - (N % 128) - 1, N - (N % 128), N - 1]
    return np.unique(np.concatenate([fixed, rng.choice(N, count, replace=False)]))


def _symmetric_on_device(D, step=4096):
    N = D.shape[0]
    return all(torch.equal(D[r:r + step], D[:, r:r + step].t()) for r in range(0, N, step))


def test_euclidean_beyond_4gib(jd):
    from scipy.spatial.distance import cdist
    rng = np.random.default_rng(33)
    X = rng.standard_normal((BIG_N, 16))
    D = jd.euclidean(X)
    assert bool(torch.isfinite(D).all()) and bool((D.diagonal() == 0).all()) and _symmetric_on_device(D)
    rows = _rows_past_4gib(BIG_N, rng)
    got = D[torch.from_numpy(rows).cuda()].cpu().numpy().astype(np.float64)
    want = cdist(X[rows], X)
    assert np.abs(got - want).max() <= EUC_TOL * float(D.max())
    del D
    torch.cuda.empty_cache()


def test_geodesic_beyond_4gib(jd):
    import scipy.sparse as sp
    import scipy.sparse.csgraph as csgraph
    rng = np.random.default_rng(34)
    X = rng.standard_normal((BIG_N, 6))
    D, k, idx, w = jd.geodesic(X, 40, return_graph=True)
    assert idx.shape[1] == 333                               # K = ceil(N / 100) + 2 > 256
    assert bool(torch.isfinite(D).all()) and bool((D.diagonal() == 0).all()) and _symmetric_on_device(D)
    rows = _rows_past_4gib(BIG_N, rng)[-16:]
    idx, w = idx[:, 1:k].cpu().numpy(), w[:, 1:k].cpu().numpy().astype(np.float64)
    g = sp.csr_matrix((w.ravel(), (np.repeat(np.arange(BIG_N), k - 1), idx.ravel())), shape=(BIG_N, BIG_N))
    want = csgraph.shortest_path(g, method='D', directed=False, indices=rows)
    assert np.isfinite(want).all()
    got = D[torch.from_numpy(rows).cuda()].cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=0)
    del D
    torch.cuda.empty_cache()


@pytest.mark.parametrize('mode', ['euclidean', 'knn', 'geodesic'])
@pytest.mark.parametrize('bad', [np.nan, np.inf])
def test_non_finite_input_raises(jd, mode, bad):
    X = np.random.default_rng(4).standard_normal((50, 5))
    X[7, 3] = bad
    call = {'euclidean': jd.euclidean, 'knn': lambda X: jd.knn(X, 5), 'geodesic': lambda X: jd.geodesic(X, 7)}[mode]
    with pytest.raises(ValueError):
        call(X)
    with pytest.raises(ValueError):
        call(torch.from_numpy(X).cuda())


def test_integer_and_sparse_input_equal_float64(jd):
    import scipy.sparse as sp
    rng = np.random.default_rng(6)
    Xi = rng.integers(-3, 4, (300, 40)) * (rng.random((300, 40)) < 0.3)
    Xi[:, :4] += 1 << 30                    # 2^30 + small: exact in float64, not in float32 (its ulp there is 128)
    Xf = Xi.astype(np.float64)
    for f in (jd.euclidean, lambda X: jd.geodesic(X, 10)):
        want = f(Xf)
        for X in (Xi, torch.from_numpy(Xi), sp.csr_matrix(Xf), sp.csr_matrix(Xi)):
            assert torch.equal(f(X), want), type(X)

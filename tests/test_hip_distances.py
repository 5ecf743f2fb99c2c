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


@pytest.mark.parametrize('N,d,k', [(500, 64, 12), (1200, 2000, 42), (7, 3, 7), (300, 5, 1)])
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

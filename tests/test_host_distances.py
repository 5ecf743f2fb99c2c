"""Stage A distances on the device (jamie_amd/distances.py, csrc/distances.hip): the design restated in numpy, checked on the
CPU against the host path's scipy / sklearn calls, and the facade's `distances=` keyword."""
import numpy as np
import pytest


def _knn_graph(rng, N, k, clusters=1):
    """A random kNN graph (scipy csr, weights = euclidean distances) over `clusters` far-apart groups (disconnected if > 1)."""
    from sklearn.neighbors import NearestNeighbors
    X = rng.standard_normal((N, 3)) + 100.0 * (np.arange(N) % clusters)[:, None]
    return NearestNeighbors(n_neighbors=min(k, N)).fit(X).kneighbors_graph(X, mode='distance')


def blocked_floyd_warshall(W, T=16):
    """The schedule of jamie_apsp_fw in numpy: rows / columns padded with +inf to a multiple of T; round r closes the diagonal
    block (phase 1), then the blocks of row r and column r through it (phase 2), then every other block as an independent
    min-plus product of its column-r and row-r blocks (phase 3).  W: dense [N, N] with +inf for no edge, 0 diagonal."""
    N = W.shape[0]
    P = -(-N // T) * T
    D = np.full((P, P), np.inf, np.float32)
    D[:N, :N] = W
    nb = P // T
    blk = lambda b: slice(b * T, (b + 1) * T)     # noqa: E731

    def close(C, A, B):                           # C = min(C, A (min,+) B), k sequential (A or B may alias C)
        for k in range(T):
            C[:] = np.minimum(C, A[:, k:k + 1] + B[k:k + 1, :])
    for r in range(nb):
        R = blk(r)
        d = D[R, R]
        close(d, d, d)                                                       # phase 1
        for b in range(nb):                                                  # phase 2
            if b != r:
                row, col = D[R, blk(b)], D[blk(b), R]
                close(row, d, row)
                close(col, col, d)
        A, B = D[:, R].copy(), D[R, :].copy()                                 # phase 3
        for bi in range(nb):
            for bj in range(nb):
                if bi != r and bj != r:
                    C = D[blk(bi), blk(bj)]
                    C[:] = np.minimum(C, (A[blk(bi)][:, :, None] + B[:, blk(bj)][None, :, :]).min(axis=1))
    return D[:N, :N]


@pytest.mark.parametrize('N', [1, 15, 16, 17, 100])
@pytest.mark.parametrize('clusters', [1, 3])
def test_blocked_floyd_warshall_schedule_equals_dijkstra(N, clusters):
    import scipy.sparse.csgraph as csgraph
    rng = np.random.default_rng(N * 7 + clusters)
    g = _knn_graph(rng, N, 4, clusters)
    want = csgraph.shortest_path(g, method='D', directed=False)
    W = np.full((N, N), np.inf, np.float32)
    coo = g.tocoo()
    for i, j, w in zip(coo.row, coo.col, coo.data):                           # directed=False: both directions, smaller weight
        W[i, j] = min(W[i, j], w)
        W[j, i] = min(W[j, i], w)
    np.fill_diagonal(W, 0)
    got = blocked_floyd_warshall(W)
    assert np.array_equal(np.isinf(got), np.isinf(want))
    fin = np.isfinite(want)
    np.testing.assert_allclose(got[fin], want[fin], rtol=1e-6, atol=1e-6)
    if clusters > 1 and N >= 15:
        assert np.isinf(want).any()                                           # the disconnected case is exercised


def test_prefixes_of_one_top_k_equal_kneighbors_graph_at_every_k_of_the_growth_loop():
    """jamie_knn_topk's contract: one ascending list of K_max neighbours per cell (the cell itself first), whose first k columns
    are sklearn's kneighbors_graph(X) with n_neighbors = k for every k the growth loop of geodesic_distances visits."""
    from sklearn.metrics import pairwise_distances
    from sklearn.neighbors import NearestNeighbors
    from jamie_amd.distances import K_MIN, k_max
    rng = np.random.default_rng(3)
    N, kmax = 300, 12
    X = rng.standard_normal((N, 8))
    D = pairwise_distances(X)
    np.fill_diagonal(D, -1.0)                                                 # the cell itself first
    K = k_max(N, kmax)
    order = np.lexsort((np.broadcast_to(np.arange(N), (N, N)), D), axis=1)[:, :K]
    assert (order[:, 0] == np.arange(N)).all()
    k = K_MIN
    while k <= max(kmax, 0.01 * N) + 2:
        kk = min(k, N)
        g = NearestNeighbors(n_neighbors=kk).fit(X).kneighbors_graph(X, mode='distance').tocsr()
        for i in range(N):
            cols = g.indices[g.indptr[i]:g.indptr[i + 1]]
            assert set(cols) == set(order[i, :kk]), (k, i)
            np.testing.assert_allclose(g[i, order[i, 1:kk]].toarray().ravel(), D[i, order[i, 1:kk]], rtol=1e-12)
        k += 2
    assert K == kmax + 2 and k - 2 <= K


def test_k_max_bounds_the_growth_loop():
    from jamie_amd.distances import K_MIN, k_max
    for N in (2, 7, 60, 999, 1000, 1001, 8192, 16384):
        for kmax in (1, 5, 7, 40):
            k = K_MIN
            while k <= max(kmax, 0.01 * N):       # the loop's last increment happens while k <= max(kmax, N / 100)
                k += 2
            assert min(k, N) <= k_max(N, kmax), (N, kmax)


def test_distances_keyword_is_validated():
    import jamie_amd
    with pytest.raises(ValueError):
        jamie_amd.JAMIE(distances='gpu')
    with pytest.raises(ValueError):
        jamie_amd.JAMIE(distances='device', distance_mode='spearman')
    for mode in ('geodesic', 'euclidean', 'l2', 'sqeuclidean'):
        assert jamie_amd.JAMIE(distances='device', distance_mode=mode).distances == 'device'
    assert jamie_amd.JAMIE().distances == 'host'

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


# ---- duplicates, ties and the Gram form's cancellation (shared with test_hip_distances.py) ----
TAU = 2.0 ** -10            # csrc/distances.hip DIST_TAU: q < TAU (n_i + n_j) is recomputed by direct difference


def duplicate_data(d, seed=0):
    """A Gaussian background of 600 cells plus the near-duplicates of real single-cell data: exact copies of 20 cells, 6 groups of
    12 copies with noise sigma = 1e-3 around a background cell, and one group of 45 copies of a cell (46 identical cells, more
    than kmax = 40).  Rows shuffled, so that the duplicates meet across tiles."""
    rng = np.random.default_rng(seed + d)
    B = rng.standard_normal((600, d))
    exact = B[rng.choice(600, 20, replace=False)]
    noisy = np.repeat(B[rng.choice(600, 6, replace=False)], 12, axis=0) + 1e-3 * rng.standard_normal((72, d))
    group = np.repeat(B[rng.integers(600)][None], 45, axis=0)
    X = np.concatenate([B, exact, noisy, group])
    return X[rng.permutation(len(X))]


def tie_rule_order(D, K):
    """jamie_knn_topk's order in float64: per row the cell itself, then the other columns ascending by (D, column); first K."""
    N = len(D)
    D = np.array(D, np.float64)
    np.fill_diagonal(D, -1.0)
    return np.lexsort((np.broadcast_to(np.arange(N), D.shape), D), axis=1)[:, :K]


def tie_rule_geodesic(X, kmax, D=None):
    """utilities.geodesic_distances restated in float64 with jamie_knn_topk's tie rule: the growth loop's graph of k neighbours is
    the first k columns of tie_rule_order (explicit zero weights are edges, as in kneighbors_graph).  -> (dist, k)."""
    import scipy.sparse as sp
    import scipy.sparse.csgraph as csgraph
    from scipy.spatial.distance import cdist
    X = np.asarray(X, np.float64)
    N = len(X)
    D = cdist(X, X) if D is None else D
    order = tie_rule_order(D, min(N, max(int(kmax) + 2, int(np.ceil(0.01 * N)) + 2, 5)))

    def graph(k):
        k = min(k, N)
        rows, cols = np.repeat(np.arange(N), k), order[:, :k].ravel()
        return sp.csr_matrix((D[rows, cols], (rows, cols)), shape=(N, N))
    k = 5
    while csgraph.connected_components(graph(k), directed=False)[0] != 1:
        if k > np.max((kmax, 0.01 * N)):
            break
        k += 2
    dist = csgraph.shortest_path(graph(k), method='D', directed=False)
    fin = dist[np.isfinite(dist)]
    dist[~np.isfinite(dist)] = 2 * (fin.max() if fin.size else 0.0)
    return dist, min(k, N)


def _gram_form_fp32(X):
    """Centred fp32 rows and q = n_i + n_j - 2 G_ij in fp32 with the device's two summation orders: n lane by lane (64 strided
    partial sums, then a tree), G one fp32 matrix product.  -> (Xc, q, n_i + n_j)."""
    Xc = (X - X.mean(0)).astype(np.float32)
    N, d = Xc.shape
    P = np.zeros((N, -(-d // 64) * 64), np.float32)
    P[:, :d] = Xc
    n = np.zeros((N, 64), np.float32)
    for c in range(0, P.shape[1], 64):
        n = n + P[:, c:c + 64] * P[:, c:c + 64]
    while n.shape[1] > 1:
        n = n[:, 0::2] + n[:, 1::2]
    s = n[:, 0][:, None] + n[:, 0][None, :]
    return Xc, np.maximum(s - np.float32(2) * (Xc @ Xc.T), 0).astype(np.float32), s


@pytest.mark.parametrize('d', [16, 50, 2000])
def test_recomputing_cancelled_pairs_restores_the_euclidean_contract(d):
    """The rule of jamie_gram_to_distances restated: on near-duplicate cells the Gram form alone is off by far more than
    1e-5 max D (and exact duplicates do not come out 0); recomputing the pairs with q < TAU (n_i + n_j) by direct difference
    brings both back, and on plain Gaussian data it recomputes nothing."""
    from scipy.spatial.distance import cdist
    X = duplicate_data(d)
    want = cdist(X, X)
    Xc, q, s = _gram_form_fp32(X)
    np.fill_diagonal(q, 0)
    err0 = np.abs(np.sqrt(q) - want).max() / want.max()
    assert err0 > 1e-5, err0                                   # the case the device tests exercise
    redo = (q < np.float32(TAU) * s) & ~np.eye(len(X), dtype=bool)
    ii, jj = np.nonzero(redo)
    q[ii, jj] = ((Xc[ii] - Xc[jj]) ** 2).sum(1, dtype=np.float32)
    err = np.abs(np.sqrt(q) - want).max() / want.max()
    assert err <= 1e-5, err
    assert (np.sqrt(q)[want == 0] == 0).all()
    assert redo.mean() < 0.01
    _, qg, sg = _gram_form_fp32(np.random.default_rng(d).standard_normal((700, d)))
    np.fill_diagonal(qg, np.inf)
    assert not (qg < np.float32(TAU) * sg).any()


@pytest.mark.parametrize('d', [16, 2000])
def test_tie_rule_geodesic_equals_the_host_path_on_duplicates(d):
    """What the device's geodesic is held to on duplicate_data: its tie rule picks other identical cells than sklearn does, but
    identical cells are interchangeable, so the distances are the host path's."""
    from jamie_amd.utilities import geodesic_distances
    X = duplicate_data(d)
    got, _ = tie_rule_geodesic(X, 40)
    want = geodesic_distances(X, 40)         # (sklearn takes kNN distances in the Gram form: exact duplicates ~1e-7 apart)
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-7 * want.max())

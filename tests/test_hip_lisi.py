"""Neighbourhoods on the device (jamie_amd/neighbors.py, csrc/neighbors.hip) against the float64 references of lisi_util.py.

The search: the neighbour sets equal the stable argsort's except at queries whose K-th and (K + 1)-th distances lie within 1e-5
(the project's fp32 distance tolerance; their share in the reference is capped at 3 %), and exactly, bit for bit, on
integer-valued data, across the 64 / 65 seam of the two passes and for every segment length.  LISI: the device solve on the
device's own lists equals the float64 loop within 1e-12 relative (K <= 128 fp64 terms, a handful of ulps each, identical branch
decisions: cells whose trace comes within 1e-11 of a branch are left out, at most 0.5 % of them), end to end within
lisi_util.LISI_TOL of the all-float64 host route.  Every figure is printed before it is asserted."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lisi_util as lu  # noqa: E402
import metrics_util as mu  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = list(range(len(lu.SHAPES)))


@pytest.fixture(scope='module')
def jn():
    from jamie_amd import neighbors
    return neighbors


_lists = {}


def device_lists(jn, which):
    """self_knn on SHAPES[which], once: (idx int64 numpy, dist fp32 numpy)."""
    if which not in _lists:
        c = lu.shape_case(which)
        idx, dist = jn.self_knn(c['X'], c['K'])
        assert idx.dtype == torch.int32 and dist.dtype == torch.float32
        assert idx.shape == (len(c['X']), c['K']) and dist.shape == idx.shape
        _lists[which] = (idx.cpu().numpy().astype(np.int64), dist.cpu().numpy())
    return _lists[which]


def _check_against_argsort(X, K, idx, dist, ref_idx, ref_dist, ds):
    from scipy.spatial.distance import cdist
    N = len(X)
    amb = mu.near_tied(ds, K)
    print(f'queries with the K-th and (K+1)-th distance within 1e-5: {amb.mean():.4f}')
    assert amb.mean() <= 0.03
    assert idx.min() >= 0 and idx.max() < N
    assert all(len(set(r)) == K for r in idx)
    assert not np.any(idx == np.arange(N)[:, None])
    same = np.array([set(a) == set(b) for a, b in zip(idx, ref_idx)])
    print(f'neighbour sets equal: {same.mean():.4f} of the queries, {int((~same & ~amb).sum())} differ without a near tie')
    assert np.all(same | amb)
    dist = dist.astype(np.float64)
    assert np.all(np.diff(dist, axis=1) >= 0)
    got = np.take_along_axis(cdist(X.astype(np.float64), X.astype(np.float64)), idx, axis=1)
    print(f'max relative distance error {np.max(np.abs(dist - got) / np.maximum(got, 1e-300)):.2e}')
    np.testing.assert_allclose(dist, got, rtol=1e-6, atol=0)
    np.testing.assert_allclose(dist[~amb], ref_dist[~amb], rtol=1e-6, atol=0)


@pytest.mark.parametrize('which', CASES)
def test_self_knn_vs_argsort(jn, which):
    c = lu.shape_case(which)
    idx, dist = device_lists(jn, which)
    _check_against_argsort(c['X'], c['K'], idx, dist, c['idx'], c['dist'], c['ds'])
    i2, d2 = jn.self_knn(c['X'], c['K'], seg_rows=128)
    assert np.array_equal(i2.cpu().numpy(), idx) and np.array_equal(d2.cpu().numpy(), dist)


@pytest.mark.parametrize('N,L,K', [(8, 3, 7), (130, 5, 128)])
def test_self_knn_every_other_row(jn, N, L, K):
    X = np.random.default_rng(N + L + K).standard_normal((N, L)).astype(np.float32)
    ref_idx, ref_dist, ds = lu.knn_reference(X, K)
    idx, dist = jn.self_knn(X, K)
    _check_against_argsort(X, K, idx.cpu().numpy().astype(np.int64), dist.cpu().numpy(), ref_idx, ref_dist, ds)
    i2, d2 = jn.self_knn(X, K, seg_rows=128)
    assert torch.equal(i2, idx) and torch.equal(d2, dist)


def test_self_knn_ties_duplicates_and_the_seam_exact(jn):
    """Integer-valued cells: every q is exact, nearly every cell ties at the 64 / 65 seam, and the order is (q, lower index)."""
    from scipy.spatial.distance import cdist
    X = lu.integer_cells()
    d = cdist(X.astype(np.float64), X.astype(np.float64))
    np.fill_diagonal(d, np.inf)
    order = np.argsort(d, axis=1, kind='stable')
    ds = np.take_along_axis(d, order, axis=1)
    print(f'cells whose 64th and 65th neighbours tie: {(ds[:, 63] == ds[:, 64]).mean():.4f}')
    assert (ds[:, 63] == ds[:, 64]).mean() > 0.9
    x = torch.from_numpy(X).cuda()
    for K in (1, 16, 17, 63, 64, 65, 90, 128):
        for seg in (0, 128, 256):
            idx, dist = jn.self_knn(x, K, seg_rows=seg)
            assert np.array_equal(idx.cpu().numpy(), order[:, :K]), (K, seg)
            assert np.array_equal(dist.cpu().numpy(), ds[:, :K].astype(np.float32)), (K, seg)
    # 200 identical rows: the K lowest other indices, every distance 0
    same = np.tile(X[:1], (200, 1))
    for K in (5, 64, 100):
        idx, dist = jn.self_knn(same, K)
        want = np.array([[j for j in range(K + 1) if j != i][:K] for i in range(200)])
        assert np.array_equal(idx.cpu().numpy(), want) and not dist.any()
    # an exact copy at a lower index is neighbour 0 at distance 0; the cell itself is absent
    Y = np.random.default_rng(4).standard_normal((300, 6)).astype(np.float32)
    Y[217] = Y[40]
    for K in (3, 70):
        idx, dist = jn.self_knn(Y, K)
        idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
        assert idx[217, 0] == 40 and dist[217, 0] == 0 and idx[40, 0] == 217 and dist[40, 0] == 0
        assert 217 not in idx[217] and 40 not in idx[40]
        assert not np.any(idx == np.arange(300)[:, None])


@pytest.mark.parametrize('which', CASES)
def test_lisi_on_the_devices_own_lists(jn, which):
    c = lu.shape_case(which)
    K = c['K']
    idx, dist = device_lists(jn, which)
    codes = np.stack([c['mod'], c['lcode']])
    for u in [p for p in (K / 3, 21.7, 42.5) if 1 < p < K]:
        ref, ref_tries, margin = lu.lisi_reference(idx, dist.astype(np.float64), codes, (c['M'], c['T']), u)
        got, tries = jn.lisi_from_neighbors(idx, dist, codes, u, return_tries=True)
        assert got.shape == ref.shape and got.dtype == np.float64 and tries.dtype == np.int32
        near = margin < 1e-11
        rel = np.max(np.abs(got - ref) / ref, axis=0)
        print(f'perplexity {u:.4g}: cells within 1e-11 of a branch {near.mean():.4f}, tries differ on '
              f'{int((tries != ref_tries)[~near].sum())}, max relative |dLISI| {rel[~near].max():.2e}')
        assert near.mean() <= 0.005
        assert np.array_equal(tries[~near], ref_tries[~near])
        assert np.all(rel[~near] <= 1e-12)
        # one set alone gives the bits of the same set among two
        alone = jn.lisi_from_neighbors(idx, dist, c['lcode'], u)
        assert alone.shape == (1, len(idx)) and np.array_equal(alone[0], got[1])


def test_lisi_edge_cases(jn):
    N, K = 300, 30
    rng = np.random.default_rng(12)
    idx = np.stack([rng.permutation(N)[:K] for _ in range(N)]).astype(np.int32)
    codes = rng.integers(0, 3, (2, N))
    # every distance 0: uniform weights, the cap of 50 tries, a finite figure equal to the reference's
    zero = np.zeros((N, K), np.float32)
    got, tries = jn.lisi_from_neighbors(idx, zero, codes, 10.0, return_tries=True)
    ref, ref_tries, _ = lu.lisi_reference(idx, zero.astype(np.float64), codes, (3, 3), 10.0)
    assert np.all(tries == 50) and np.all(ref_tries == 50) and np.all(np.isfinite(got))
    uniform = 1.0 / np.array([[sum((np.sum(c[idx[i]] == b) / K) ** 2 for b in range(3)) for i in range(N)] for c in codes])
    print(f'all distances 0: against uniform weights {np.max(np.abs(got - uniform) / uniform):.2e}')
    assert np.all(np.abs(got - uniform) <= 1e-12 * uniform) and np.all(np.abs(got - ref) <= 1e-12 * ref)
    # every distance 1e30: every weight underflows at every beta
    far = np.full((N, K), 1e30, np.float32)
    far[7] = np.linspace(0.5, 2.0, K)
    got = jn.lisi_from_neighbors(idx, far, codes, 10.0)
    assert np.all(np.isnan(got[:, np.arange(N) != 7])) and np.all(np.isfinite(got[:, 7]))
    # the integer cells at K = 90: a few cells stop at the cap, and the figures are the reference's
    X = lu.integer_cells()
    ii, dd = jn.self_knn(X, 90)
    ii, dd = ii.cpu().numpy().astype(np.int64), dd.cpu().numpy()
    codes = np.stack([np.arange(len(X)) % 2, np.arange(len(X)) % 5])
    ref, ref_tries, margin = lu.lisi_reference(ii, dd.astype(np.float64), codes, (2, 5), 30.0)
    got, tries = jn.lisi_from_neighbors(ii, dd, codes, 30.0, return_tries=True)
    near = margin < 1e-11
    print(f'integer cells: at the cap {(ref_tries == 50).mean():.4f}, within 1e-11 of a branch {near.mean():.4f}')
    assert 0 < (ref_tries == 50).mean() < 0.01 and near.mean() <= 0.005
    assert np.array_equal(tries[~near], ref_tries[~near])
    assert np.all(np.abs(got - ref)[:, ~near] <= 1e-12 * ref[:, ~near])
    # the scale of the embedding: no cell fails
    emb, lab = lu.mixture(3, 4, 8, (300, 260))
    for scale in (1000.0, 1e-6):
        out = jn.lisi([e * np.float32(scale) for e in emb], lab)
        print(f"scale {scale:g}: n_failed {out['n_failed']}, iLISI median {out['ilisi_median']:.4f}")
        assert out['n_failed'] == 0 and np.all(np.isfinite(out['ilisi'])) and np.all(np.isfinite(out['clisi']))
    # a failed cell is counted and the medians skip it
    apart = [np.concatenate([emb[0], np.full((1, 8), 1e18, np.float32)]), emb[1]]
    out = jn.lisi(apart, [np.concatenate([lab[0], lab[0][:1]]), lab[1]])
    assert out['n_failed'] == 1 and np.isnan(out['ilisi'][300]) and np.isfinite(out['ilisi_median'])


def test_refusals_before_allocating(jn):
    from jamie_amd import JAMIE
    from jamie_amd import _native as nv
    X = np.zeros((100, 4), np.float32)
    x = torch.zeros(100, 4, device='cuda')
    idx = torch.zeros(100, 129, dtype=torch.int32, device='cuda')
    dist = torch.zeros(100, 129, device='cuda')
    codes = torch.zeros(5, 100, dtype=torch.int32, device='cuda')
    out = torch.zeros(5, 100, dtype=torch.float64, device='cuda')
    ws = torch.empty(1 << 20, dtype=torch.uint8, device='cuda')
    idx30, dist30, idx1, dist1 = (t.contiguous() for t in (idx[:, :30], dist[:, :30], idx[:, :1], dist[:, :1]))
    bad = X.copy()
    bad[3, 2] = np.nan
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    for k in (0, 129, 100):
        with pytest.raises(ValueError):
            jn.self_knn(x, k)
        with pytest.raises(ValueError):
            jn.knn_graph([x], k=k)
    with pytest.raises(ValueError):
        jn.self_knn(x, 5, seg_rows=100)
    with pytest.raises(ValueError):
        jn.lisi([x], perplexity=1.0)
    with pytest.raises(ValueError):
        jn.lisi([x], perplexity=30, n_neighbors=30)
    with pytest.raises(ValueError):
        jn.lisi([x], perplexity=30, n_neighbors=129)
    with pytest.raises(ValueError):
        jn.lisi([x], [np.zeros(99)], perplexity=5)
    with pytest.raises(ValueError):
        jn.lisi_from_neighbors(idx30, dist30, np.zeros((5, 100)), 10.0)
    with pytest.raises(ValueError):
        jn.lisi_from_neighbors(idx30, dist30, np.zeros(100), 30.0)
    with pytest.raises(ValueError):
        jn.lisi_from_neighbors(idx1, dist1, np.zeros(100), 1.5)
    with pytest.raises(ValueError):
        jn.lisi_from_neighbors(idx, dist, np.zeros(100), 30.0)
    # the ABI refuses them too, before a launch
    for k, seg in ((0, 0), (129, 0), (100, 0), (5, 100)):
        with pytest.raises(nv.JamieHipError):
            nv.self_knn(x, k, idx, dist, ws, seg)
    with pytest.raises(nv.JamieHipError):
        nv.self_knn(x, 90, idx, dist, ws[:1000])
    with pytest.raises(nv.JamieHipError):
        nv.lisi(idx1, dist1, codes[:1], 1.5, out)
    with pytest.raises(nv.JamieHipError):
        nv.lisi(idx, dist, codes[:1], 30.0, out)
    with pytest.raises(nv.JamieHipError):
        nv.lisi(idx30, dist30, codes, 10.0, out)
    for u in (1.0, 30.0):
        with pytest.raises(nv.JamieHipError):
            nv.lisi(idx30, dist30, codes[:1], u, out)
    assert torch.cuda.max_memory_allocated() == before
    # NaN / inf on the device route
    with pytest.raises(ValueError):
        jn.self_knn(bad, 5)
    with pytest.raises(ValueError):
        JAMIE(metrics='device').test_lisi([bad], perplexity=5)
    with pytest.raises(ValueError):
        JAMIE(metrics='device').neighbors([bad], k=5)


@pytest.mark.parametrize('which', CASES)
def test_facade_on_the_device_vs_the_host(jn, which, capsys):
    from jamie_amd import JAMIE
    c = lu.shape_case(which)
    K = c['K']
    u = K / 3
    amb = mu.near_tied(c['ds'], K)
    emb64 = [e.astype(np.float64) for e in c['emb']]
    host = JAMIE().test_lisi(emb64, c['lab'], perplexity=u, n_neighbors=K)
    capsys.readouterr()
    dev = JAMIE(metrics='device').test_lisi(emb64, c['lab'], perplexity=u, n_neighbors=K)
    lines = capsys.readouterr().out.strip().splitlines()[-2:]
    assert lines == [f"iLISI (median): {dev['ilisi_median']}", f"cLISI (median): {dev['clisi_median']}"]
    for name in ('ilisi', 'clisi'):
        rel = np.abs(dev[name] - host[name]) / host[name]
        print(f'{name}: max relative difference off the near-tied cells {rel[~amb].max():.2e}, over all cells {rel.max():.2e}; '
              f'median {dev[name + "_median"]!r} against {host[name + "_median"]!r}')
        assert np.all(rel[~amb] <= lu.LISI_TOL)
        for fig in ('_median', '_scaled'):
            assert abs(dev[name + fig] - host[name + fig]) <= lu.LISI_TOL * abs(host[name + fig])
    assert dev['n_neighbors'] == host['n_neighbors'] == K and dev['n_failed'] == host['n_failed'] == 0
    assert np.array_equal(dev['labels'], host['labels'])
    bare = JAMIE(metrics='device').test_lisi(emb64, perplexity=u, n_neighbors=K)
    assert np.array_equal(bare['ilisi'], dev['ilisi']) and bare['clisi'] is None and bare['labels'] is None
    # the graph
    k = min(K, 15)
    amb_k = mu.near_tied(c['ds'], k)
    hg = JAMIE().neighbors(emb64, k=k)
    dg = JAMIE(metrics='device').neighbors(emb64, k=k)
    N = len(c['X'])
    assert dg.shape == (N, N) and dg.dtype == np.float64 and np.array_equal(np.diff(dg.indptr), np.full(N, k))
    hi, di = hg.indices.reshape(N, k), dg.indices.reshape(N, k)
    swapped = np.any(hi != di, axis=1)
    print(f'graph rows that differ from the host: {int(swapped.sum())}, of them near-tied at k: {int((swapped & amb_k).sum())}')
    # (two neighbours within the fp32 tolerance of each other inside the list may swap places: there the sets must agree)
    inside = np.any(np.diff(c['ds'][:, :k], axis=1) <= mu.REL_TOL * c['ds'][:, 1:k], axis=1)
    assert np.array_equal(hi[~amb_k & ~inside], di[~amb_k & ~inside])
    assert all(set(a) == set(b) for a, b in zip(hi[~amb_k], di[~amb_k]))
    np.testing.assert_allclose(dg.data.reshape(N, k)[~amb_k], hg.data.reshape(N, k)[~amb_k], rtol=1e-6, atol=0)
    cg = JAMIE(metrics='device').neighbors(emb64, k=k, mode='connectivity')
    assert np.array_equal(cg.data, np.ones(N * k)) and np.array_equal(cg.indices, dg.indices)


def test_two_calls_are_bit_identical(jn):
    emb, lab = lu.mixture(9, 4, 32, (2500, 2300))
    X = np.concatenate(emb)
    i1, d1 = jn.self_knn(X, 90)
    i2, d2 = jn.self_knn(X, 90)
    assert torch.equal(i1, i2) and torch.equal(d1, d2)
    codes = np.stack([np.arange(len(X)) % 2, np.arange(len(X)) % 7])
    a = jn.lisi_from_neighbors(i1, d1, codes, 30.0, return_tries=True)
    b = jn.lisi_from_neighbors(i1, d1, codes, 30.0, return_tries=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_memory_at_20000_cells(jn):
    """20 000 pooled cells, L = 32, K = 90: peak device memory under inputs + outputs + workspace + 64 MiB (an N x N fp32
    matrix would be 1.6 GB), and two samples of one mixture mix."""
    from jamie_amd import _native as nv
    emb, lab = lu.mixture(21, 6, 32, (10000, 10000), shift=0.0)
    xs = [torch.from_numpy(e).cuda() for e in emb]
    N, L, K = 20000, 32, 90
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = jn.lisi(xs, lab)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    budget = N * L * 4 + N * K * 8 + nv.self_knn_workspace(N, K) + 64 * 2 ** 20
    print(f"device memory above the resident inputs {extra / 2 ** 20:.1f} MiB, budget {budget / 2 ** 20:.1f} MiB; iLISI median "
          f"{out['ilisi_median']:.4f}, cLISI median {out['clisi_median']:.4f}")
    assert extra < budget
    assert out['n_neighbors'] == K and out['n_failed'] == 0 and out['ilisi_median'] > 1.8

"""Alignment metrics on the device (jamie_amd/metrics.py, csrc/metrics.hip) against float64 references.

The contract for a count: lo <= count <= hi, with lo / hi the float64 counts under d(i, j) < d(i, i) (1 -/+ 1e-5); 1e-5 is the
relative tolerance the project holds its fp32 distances to, and an fp32 direct-difference sum of L <= 100 terms is inside it in
the worst case (L 2^-24 on q, half of that on d: 3e-6).  Before a device result is looked at, the reference alone must show
that the band is narrow (at most 2e-4 of the 2 N^2 pairs) and the figure neither degenerate nor saturated (FOSCTTM in
[0.05, 0.45]).  Every figure is printed before it is asserted."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metrics_util as mu  # noqa: E402

pytestmark = pytest.mark.gpu

BAND_MAX = 2e-4


@pytest.fixture(scope='module')
def jm():
    from jamie_amd import metrics
    return metrics


def _check_band(ref):
    print(f"reference: foscttm {ref['value']:.6f}, band share {ref['share']:.3e}")
    assert ref['share'] <= BAND_MAX
    assert 0.05 <= ref['value'] <= 0.45


def _check_counts(ref, row, col, value):
    N = len(row)
    for name, got, lo, hi, ex in (('row', row, ref['lo'][0], ref['hi'][0], ref['exact'][0]),
                                  ('col', col, ref['lo'][1], ref['hi'][1], ref['exact'][1])):
        print(f'{name}: cells off the exact float64 count {int((got != ex).sum())}, outside the band '
              f'{int(((got < lo) | (got > hi)).sum())}')
        assert np.all(got >= lo) and np.all(got <= hi)
    print(f"device foscttm {value!r}, float64 {ref['value']!r}")
    assert value == (int(row.sum()) + int(col.sum())) / (2 * N ** 2)
    assert abs(value - ref['value']) <= ref['share']


@pytest.mark.parametrize('N,L,s', [(1000, 5, 0.7), (3001, 32, 1.5), (2500, 64, 2.0), (777, 100, 2.5)])
def test_foscttm_vs_float64(jm, N, L, s):
    A, B = mu.noisy_pair(N, L, s, seed=N + L)
    ref = mu.foscttm_band(A, B)
    _check_band(ref)
    value, (row, col) = jm.foscttm(A, B, return_counts=True)
    assert row.dtype == np.int64 and col.dtype == np.int64
    _check_counts(ref, row, col, value)


def test_foscttm_ties_are_exact(jm):
    """Integer-valued data: every q is a small integer, exact in fp32 in any order, and many pairs tie with their own pair
    distance.  Strict <, j = i excluded by index: the counts equal the float64 reference exactly."""
    rng = np.random.default_rng(11)
    A = rng.integers(-2, 3, (1500, 4)).astype(np.float32)
    B = rng.integers(-2, 3, (1500, 4)).astype(np.float32)
    ref = mu.foscttm_band(A, B)
    from scipy.spatial.distance import cdist
    d = cdist(A.astype(np.float64), B.astype(np.float64))
    ties = int((d == np.diag(d)[:, None]).sum()) - len(A)
    print(f"off-diagonal pairs tied with the row's own pair distance: {ties}; foscttm {ref['value']:.4f}")
    assert ties > 10000
    value, (row, col) = jm.foscttm(A, B, return_counts=True)
    assert np.array_equal(row, ref['exact'][0]) and np.array_equal(col, ref['exact'][1])
    assert value == ref['value']
    # every own pair at distance 0: nothing is closer
    value, (row, col) = jm.foscttm(A, A.copy(), return_counts=True)
    assert value == 0.0 and not row.any() and not col.any()
    # all rows identical: every pair ties
    C = np.tile(A[:1], (1500, 1))
    D = np.tile(B[:1], (1500, 1))
    value, (row, col) = jm.foscttm(C, D, return_counts=True)
    assert value == 0.0 and not row.any() and not col.any()


def test_foscttm_input_kinds_and_errors(jm):
    A, B = mu.noisy_pair(700, 12, 1.0, seed=5)
    _, c32 = jm.foscttm(A, B, return_counts=True)
    _, c64 = jm.foscttm(A.astype(np.float64), B.astype(np.float64), return_counts=True)
    _, cdev = jm.foscttm(torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda(), return_counts=True)
    for x, y in zip(c32, c64):
        assert np.array_equal(x, y)
    for x, y in zip(c32, cdev):
        assert np.array_equal(x, y)
    with pytest.raises(ValueError):
        jm.foscttm(A, B[:-1])
    with pytest.raises(ValueError):
        jm.foscttm(A, B[:, :-1])
    bad = A.copy()
    bad[3, 2] = np.nan
    with pytest.raises(ValueError):
        jm.foscttm(bad, B)
    with pytest.raises(ValueError):
        jm.foscttm(A[0], B[0])


def test_facade_test_closer_on_the_device(jm, capsys):
    from jamie_amd import JAMIE
    A, B = mu.noisy_pair(1000, 5, 0.7, seed=1005)
    e0, e1 = A.astype(np.float64), B.astype(np.float64)
    ref = mu.foscttm_band(A, B)
    _check_band(ref)
    host = JAMIE().test_closer([e0, e1])
    host_line = capsys.readouterr().out.strip().splitlines()[-1]
    dev = JAMIE(metrics='device').test_closer([e0, e1])
    dev_line = capsys.readouterr().out.strip().splitlines()[-1]
    print(f'host {host!r} device {dev!r} band share {ref["share"]:.3e}')
    assert isinstance(dev, float)
    assert abs(dev - host) <= ref['share']
    assert host_line == f'foscttm: {host}' and dev_line == f'foscttm: {dev}'
    assert JAMIE(metrics='device').test_closer([e0, e1], distance_metric='euclidean') == dev
    with pytest.raises(AssertionError):
        JAMIE(metrics='device').test_closer([e0, e1, e0])
    with pytest.raises(ValueError):
        JAMIE(metrics='device').test_closer([e0, e1], distance_metric='cosine')


@pytest.mark.parametrize('Nq,Nr,L,K', [(500, 700, 32, 5), (1300, 999, 64, 64), (7, 3, 3, 3), (3000, 5000, 8, 1),
                                       (2049, 4097, 100, 30)])
def test_cross_knn_vs_argsort(jm, Nq, Nr, L, K):
    from scipy.spatial.distance import cdist
    rng = np.random.default_rng(Nq + Nr + L + K)
    Q = rng.standard_normal((Nq, L)).astype(np.float32)
    R = rng.standard_normal((Nr, L)).astype(np.float32)
    d = cdist(Q.astype(np.float64), R.astype(np.float64))
    order = np.argsort(d, axis=1, kind='stable')
    ds = np.take_along_axis(d, order, axis=1)
    amb = mu.near_tied(ds, K)
    print(f'queries with the K-th and (K+1)-th distance within 1e-5: {amb.mean():.4f}')
    assert amb.mean() <= 0.03
    idx, dist = jm.cross_knn(Q, R, K)
    assert idx.dtype == torch.int32 and dist.dtype == torch.float32 and idx.shape == (Nq, K) and dist.shape == (Nq, K)
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy().astype(np.float64)
    assert idx.min() >= 0 and idx.max() < Nr
    assert all(len(set(r)) == K for r in idx)
    same = np.array([set(a) == set(b) for a, b in zip(idx, order[:, :K])])
    print(f'neighbour sets equal: {same.mean():.4f} of the queries, {int((~same & ~amb).sum())} differ without a near tie')
    assert np.all(same | amb)
    assert np.all(np.diff(dist, axis=1) >= 0)
    got = np.take_along_axis(d, idx.astype(np.int64), axis=1)
    print(f'max relative distance error {np.max(np.abs(dist - got) / np.maximum(got, 1e-300)):.2e}')
    np.testing.assert_allclose(dist, got, rtol=1e-6, atol=0)
    np.testing.assert_allclose(dist[~amb], ds[~amb, :K], rtol=1e-6, atol=0)


def test_cross_knn_ties_by_lower_index(jm):
    from scipy.spatial.distance import cdist
    rng = np.random.default_rng(2)
    Q = rng.integers(-2, 3, (600, 3)).astype(np.float32)
    R = rng.integers(-2, 3, (900, 3)).astype(np.float32)
    d = cdist(Q.astype(np.float64), R.astype(np.float64))
    for K in (1, 10, 64):
        order = np.argsort(d, axis=1, kind='stable')[:, :K]
        idx, dist = jm.cross_knn(Q, R, K)
        assert np.array_equal(idx.cpu().numpy(), order)
        assert np.array_equal(dist.cpu().numpy(), np.take_along_axis(d, order, axis=1).astype(np.float32))


def test_cross_knn_refuses_large_k_before_allocating(jm):
    Q = np.zeros((10, 4), np.float32)
    R = np.zeros((100, 4), np.float32)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    with pytest.raises(ValueError):
        jm.cross_knn(Q, R, 65)
    with pytest.raises(ValueError):
        jm.cross_knn(Q, R[:3], 4)
    with pytest.raises(ValueError):
        jm.cross_knn(Q, R, 0)
    assert torch.cuda.max_memory_allocated() == before
    # the ABI refuses it too, before a launch
    from jamie_amd import _native as nv
    q, r = torch.zeros(10, 4, device='cuda'), torch.zeros(100, 4, device='cuda')
    idx = torch.empty(10, 65, dtype=torch.int32, device='cuda')
    dist = torch.empty(10, 65, device='cuda')
    ws = torch.empty(1 << 20, dtype=torch.uint8, device='cuda')
    with pytest.raises(nv.JamieHipError):
        nv.cross_knn(q, r, 65, idx, dist, ws)


@pytest.mark.parametrize('k', [1, 5, 6, 30])
def test_label_transfer_vs_sklearn(jm, k, capsys):
    from scipy.spatial.distance import cdist
    from sklearn.neighbors import KNeighborsClassifier
    from jamie_amd import JAMIE
    e0, l0, e1, l1 = mu.labelled_sets()
    ds = np.sort(cdist(e0, e1), axis=1)
    amb = mu.near_tied(ds, k)
    print(f'k = {k}: near-tied queries {amb.mean():.4f}')
    assert amb.mean() <= 0.01
    clf = KNeighborsClassifier(n_neighbors=k).fit(e1, l1)
    sk_pred = clf.predict(e0)
    sk_acc = float(np.mean(sk_pred == l0))
    acc, pred = jm.label_transfer_accuracy(e0, l0, e1, l1, k=k, return_pred=True)
    print(f'sklearn {sk_acc!r} device {acc!r}; predictions differ on {int((pred != sk_pred).sum())} queries')
    assert np.all((pred == sk_pred) | amb)
    assert abs(acc - sk_acc) <= amb.mean()
    assert 0.3 < sk_acc < 0.99
    capsys.readouterr()
    facade = JAMIE(metrics='device').test_LabelTA([e0, e1], [l0, l1], k=k)
    assert facade == acc
    assert capsys.readouterr().out.strip().splitlines()[-1] == f'label transfer accuracy: {acc}'


def _sampled_reference(A, B, cells):
    """float64 band counts for `cells` only: their rows and their columns of the distance matrix, in chunks on the host."""
    from scipy.spatial.distance import cdist
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    lo_r, hi_r, lo_c, hi_c = [], [], [], []
    for c in np.array_split(cells, 8):
        own = np.sqrt(((A64[c] - B64[c]) ** 2).sum(axis=1))
        dr = cdist(A64[c], B64)                      # rows c: |A_c - B_j|
        dc = cdist(B64[c], A64)                      # columns c: |A_i - B_c|
        dr[np.arange(len(c)), c] = np.inf
        dc[np.arange(len(c)), c] = np.inf
        lo_r.append((dr < (own * (1 - mu.REL_TOL))[:, None]).sum(axis=1))
        hi_r.append((dr < (own * (1 + mu.REL_TOL))[:, None]).sum(axis=1))
        lo_c.append((dc < (own * (1 - mu.REL_TOL))[:, None]).sum(axis=1))
        hi_c.append((dc < (own * (1 + mu.REL_TOL))[:, None]).sum(axis=1))
    return [np.concatenate(x) for x in (lo_r, hi_r, lo_c, hi_c)]


def test_benchmark_size_and_memory(jm):
    """N = 100 000, L = 32: the band contract on 512 cells drawn at random, and at most 256 MiB of device memory above the
    inputs over the call (an N x N fp32 matrix would be 40 GB)."""
    N, L = 100000, 32
    A, B = mu.noisy_pair(N, L, 1.5, seed=77)
    cells = np.sort(np.random.default_rng(8).choice(N, 512, replace=False))
    lo_r, hi_r, lo_c, hi_c = _sampled_reference(A, B, cells)
    share = (int((hi_r - lo_r).sum()) + int((hi_c - lo_c).sum())) / (2 * len(cells) * N)
    mid = (int(hi_r.sum()) + int(hi_c.sum())) / (2 * len(cells) * N)
    print(f'sampled reference: foscttm of the sample {mid:.6f}, band share {share:.3e}')
    assert share <= BAND_MAX and 0.05 <= mid <= 0.45
    a, b = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    value, (row, col) = jm.foscttm(a, b, return_counts=True)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    print(f'foscttm {value!r}; device memory above the inputs {extra / 2 ** 20:.1f} MiB')
    assert extra < 256 * 2 ** 20
    for name, got, lo, hi in (('row', row[cells], lo_r, hi_r), ('col', col[cells], lo_c, hi_c)):
        print(f'{name}: sampled cells outside the band {int(((got < lo) | (got > hi)).sum())}')
        assert np.all(got >= lo) and np.all(got <= hi)
    assert value == (int(row.sum()) + int(col.sum())) / (2 * N ** 2)

    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    idx, dist = jm.cross_knn(a, b, 5)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    print(f'cross_knn: device memory above the inputs {extra / 2 ** 20:.1f} MiB')
    assert extra < 256 * 2 ** 20
    from scipy.spatial.distance import cdist
    sub = cells[:64]
    d = cdist(A[sub].astype(np.float64), B.astype(np.float64))
    order = np.argsort(d, axis=1, kind='stable')
    ds = np.take_along_axis(d, order, axis=1)
    amb = mu.near_tied(ds, 5)
    got = idx[torch.from_numpy(sub).cuda()].cpu().numpy()
    same = np.array([set(x) == set(y) for x, y in zip(got, order[:, :5])])
    assert np.all(same | amb)
    np.testing.assert_allclose(dist[torch.from_numpy(sub).cuda()].cpu().numpy()[~amb], ds[~amb, :5], rtol=1e-6)


def test_two_calls_are_bit_identical(jm):
    A, B = mu.noisy_pair(5000, 32, 1.5, seed=9)
    v1, (r1, c1) = jm.foscttm(A, B, return_counts=True)
    v2, (r2, c2) = jm.foscttm(A, B, return_counts=True)
    assert v1 == v2 and np.array_equal(r1, r2) and np.array_equal(c1, c2)
    i1, d1 = jm.cross_knn(A, B[:3000], 20)
    i2, d2 = jm.cross_knn(A, B[:3000], 20)
    assert torch.equal(i1, i2) and torch.equal(d1, d2)
    e0, l0, e1, l1 = mu.labelled_sets()
    p1 = jm.label_transfer_accuracy(e0, l0, e1, l1, k=6, return_pred=True)[1]
    p2 = jm.label_transfer_accuracy(e0, l0, e1, l1, k=6, return_pred=True)[1]
    assert np.array_equal(p1, p2)

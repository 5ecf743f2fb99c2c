"""Layout quality on the device (jamie_amd/coranking.py, csrc/coranking.hip): `jamie_list_ranks` against the numpy restatement of
its design (coranking_util.restated_list_ranks) by exact integer equality -- shapes off every tile size, the scalar staging path,
an unaligned X, ties and duplicates at every threshold, every segment length, lists in any order with entries that are not
ranked, lists that are no neighbours at all -- the arguments it refuses, the device sums against numpy, and
`JAMIE(metrics='device').test_layout` against the float64 host route within the near-tie bounds of test_host_coranking.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coranking_util as cu  # noqa: E402

pytestmark = pytest.mark.gpu

# (N, L, K): N off 64 and 128; several 32-feature trips; a partial trip; L % 4 != 0 (scalar staging)
SHAPES = [(1301, 32, 15), (733, 8, 64), (550, 100, 15), (1020, 3, 63), (900, 2, 15), (517, 33, 1)]


@pytest.fixture(scope='module')
def jc():
    from jamie_amd import coranking
    return coranking


@pytest.fixture(scope='module')
def nv():
    from jamie_amd import _native
    return _native


def _cells(N, L, seed):
    return cu.mixture(seed, 5, L, (N,))[0][0]


def _raw_ranks(nv, x, idx, seg_rows=0):
    rank = torch.full(idx.shape, -7, dtype=torch.int32, device='cuda')
    ws = torch.empty(nv.list_ranks_workspace(x.shape[0], idx.shape[1], seg_rows), dtype=torch.uint8, device='cuda')
    nv.list_ranks(x, idx, rank, ws, seg_rows)
    return rank.cpu().numpy()


@pytest.mark.parametrize('N,L,K', SHAPES)
def test_ranks_of_another_spaces_lists(jc, nv, N, L, K):
    from jamie_amd.neighbors import self_knn
    X = _cells(N, L, N + L + K)
    Y = X @ cu.projection(L, N) + np.random.default_rng(K).standard_normal((N, 2)).astype(np.float32)
    idx, _ = self_knn(Y, K)
    want = cu.restated_list_ranks(X, idx.cpu().numpy())
    got = jc.list_ranks(X, idx)
    assert got.dtype == torch.int32 and got.shape == (N, K)
    got = got.cpu().numpy()
    print(f'N {N} L {L} K {K}: ranks up to {want.max()}, {int((got != want).sum())} differ')
    assert np.array_equal(got, want)
    # the lists of X itself rank 0 .. K - 1
    own, _ = self_knn(X, K)
    assert np.array_equal(jc.list_ranks(X, own).cpu().numpy(), np.tile(np.arange(K, dtype=np.int32), (N, 1)))
    # X one float off a 16-byte boundary
    buf = torch.empty(N * L + 1, dtype=torch.float32, device='cuda')
    view = buf[1:].view(N, L)
    view.copy_(torch.from_numpy(X))
    assert view.data_ptr() % 16 == 4
    assert np.array_equal(_raw_ranks(nv, view, idx), want)


@pytest.mark.parametrize('K', [64, 15])
def test_integer_cells_ties_and_duplicates_exact(jc, K):
    """Every q is a small integer: ties at every threshold, duplicate cells ranked by index, and the float64 order is the answer."""
    X = cu.integer_cells()
    Y = cu.integer_cells(L=2, seed=6)
    pos_x, order_x, _ = cu.full_order(X)
    pos_y, order_y, _ = cu.full_order(Y)
    for Z, idx, pos in ((X, order_y[:, :K], pos_x), (Y, order_x[:, :K], pos_y)):
        for seg in (0, 128):
            got = jc.list_ranks(Z, idx.astype(np.int32), seg_rows=seg).cpu().numpy()
            assert np.array_equal(got, np.take_along_axis(pos, idx, axis=1)), seg


def test_every_segment_length_gives_the_same_bits(jc):
    from jamie_amd.neighbors import self_knn
    N, L, K = 5000, 32, 15
    X = _cells(N, L, 77)
    x = torch.from_numpy(X).cuda()
    Y = X @ cu.projection(L, 78)
    idx, _ = self_knn(Y, K)
    runs = [jc.list_ranks(x, idx, seg_rows=s) for s in (128, 1024, 0, 0, 128)]
    for r in runs[1:]:
        assert torch.equal(r, runs[0])
    rows = np.concatenate([np.arange(0, 130), np.arange(2490, 2620), np.arange(N - 130, N)])
    want = cu.restated_list_ranks(X, idx.cpu().numpy(), rows=rows)
    assert np.array_equal(runs[0].cpu().numpy()[rows], want)


def test_list_handling(jc):
    from jamie_amd.neighbors import self_knn
    N, L, K = 700, 16, 24
    rng = np.random.default_rng(3)
    X = _cells(N, L, 31)
    idx = self_knn(X @ cu.projection(L, 32), K)[0].cpu().numpy()
    base = jc.list_ranks(X, idx).cpu().numpy()
    assert np.array_equal(base, cu.restated_list_ranks(X, idx))
    # rows shuffled within the row: the same shuffle of the ranks
    perm = np.argsort(rng.random((N, K)), axis=1)
    shuffled = np.take_along_axis(idx, perm, axis=1)
    assert np.array_equal(jc.list_ranks(X, shuffled).cpu().numpy(), np.take_along_axis(base, perm, axis=1))
    # entries that are not ranked get -1 and leave the others alone; a repeated entry gets equal ranks
    edit = idx.copy()
    edit[np.arange(N), rng.integers(0, K, N)] = np.arange(N)
    edit[::3, 0] = -1
    edit[1::3, K - 1] = N
    edit[2::3, 5] = edit[2::3, 6]
    got = jc.list_ranks(X, edit).cpu().numpy()
    unranked = (edit < 0) | (edit >= N) | (edit == np.arange(N)[:, None])
    assert unranked.sum() >= N and np.all(got[unranked] == -1) and np.all(got[~unranked] >= 0)
    kept = edit == idx
    assert np.array_equal(got[kept], base[kept])
    assert np.array_equal(got[2::3, 5], got[2::3, 6])
    assert np.array_equal(got, cu.restated_list_ranks(X, edit))
    # a whole row that is not ranked
    edit[11] = 11
    assert np.all(jc.list_ranks(X, edit).cpu().numpy()[11] == -1)
    # random lists, no neighbours at all: ranks up to N - 2, every pair of the row below some threshold
    for K2 in (16, 64):
        anyone = rng.integers(0, N, (N, K2)).astype(np.int32)
        want = cu.restated_list_ranks(X, anyone)
        got = jc.list_ranks(X, anyone).cpu().numpy()
        print(f'random lists of {K2}: ranks up to {want.max()} of {N - 2}')
        assert want.max() >= N - 10 and np.array_equal(got, want)


def test_refused_arguments_return_an_error_before_any_launch(nv):
    lib = nv.load()
    N, L = 300, 8
    x = torch.from_numpy(_cells(N, L, 9)).cuda()
    idx = torch.zeros(N, 64, dtype=torch.int32, device='cuda')
    rank = torch.full((N, 64), -7, dtype=torch.int32, device='cuda')
    ws = torch.empty(N * 65 * 4, dtype=torch.uint8, device='cuda')

    def call(n, K, seg_rows, ws_bytes):
        return lib.jamie_list_ranks(x.data_ptr(), n, L, idx.data_ptr(), K, rank.data_ptr(), seg_rows, ws.data_ptr(), ws_bytes, None)
    need = nv.list_ranks_workspace(N, 15)
    assert need == N * 15 * 4
    for n, K, seg_rows, ws_bytes in ((N, 0, 0, ws.numel()), (N, 65, 0, ws.numel()), (1, 15, 0, ws.numel()), (N, 15, 0, need - 1),
                                     (N, 15, 100, ws.numel())):
        assert call(n, K, seg_rows, ws_bytes) != 0, (n, K, seg_rows, ws_bytes)
        torch.cuda.synchronize()
        assert bool((rank == -7).all()), (n, K, seg_rows, ws_bytes)
    with pytest.raises(nv.JamieHipError):
        nv.list_ranks(x, idx[:, :15].contiguous(), rank[:, :15].contiguous(), ws, 100)
    assert call(N, 15, 0, need) == 0
    torch.cuda.synchronize()
    assert bool((rank.view(-1)[:N * 15] != -7).all())


def test_facade_device_route_against_the_host_route(jc):
    from jamie_amd import JAMIE
    c = cu.shape_case(0)
    N = len(c['X'])
    for K in cu.KS:
        dev = JAMIE(metrics='device').test_layout(c['high'], c['low'], n_neighbors=K, return_ranks=True)
        host = JAMIE(metrics='host').test_layout(c['high'], c['low'], n_neighbors=K, return_ranks=True)
        # the device sums are the numpy sums of the device ranks
        for name in ('rank_high', 'rank_low'):
            pen, ov, cell = jc.rank_sums(torch.from_numpy(dev[name]).cuda())
            hp, ho, hc = jc.host_rank_sums(dev[name])
            assert np.array_equal(pen, hp) and np.array_equal(ov, ho) and np.array_equal(cell, hc)
        # ranks: equal where the lists agree and no other key of the row is within REL_TOL of the entry's
        for name, lists, ds in (('rank_high', 'idx_low', c['ds_x']), ('rank_low', 'idx_high', c['ds_y'])):
            same_entry = dev[lists] == host[lists]
            near = cu.near_keys(ds, host[name]) > 0
            differ = dev[name] != host[name]
            print(f'K = {K} {name}: lists agree at {same_entry.mean():.4f} of the entries, {near.mean():.4f} have a key within 1e-5, '
                  f'{int((differ & same_entry).sum())} ranks differ')
            assert near.mean() <= cu.EXCLUDED_CAP
            assert not np.any(differ & same_entry & ~near)
        unit = 2.0 / (N * K * (2.0 * N - 3.0 * K - 1.0))
        slack_t = cu.penalty_slack(host['rank_high'], c['ds_x'], c['pos_x'], c['ds_y'], c['order_y'], K)
        slack_c = cu.penalty_slack(host['rank_low'], c['ds_y'], c['pos_y'], c['ds_x'], c['order_x'], K)
        print(f"K = {K}: trustworthiness {dev['trustworthiness']:.9f} (host {host['trustworthiness']:.9f}, bound {slack_t * unit:.2e}), "
              f"continuity {dev['continuity']:.9f} (host {host['continuity']:.9f}, bound {slack_c * unit:.2e})")
        assert abs(dev['trustworthiness'] - host['trustworthiness']) <= slack_t * unit + 1e-14
        assert abs(dev['continuity'] - host['continuity']) <= slack_c * unit + 1e-14
        # the curves: at k the places of the first k columns, the unit of k; an entry counts in Q_NX(k) unless its rank crosses k
        for k in sorted({k for k in (1, 2, 3, 5, 8, 13, 21, 34, 55, K - 1, K) if k <= K}):
            u = 2.0 / (N * k * (2.0 * N - 3.0 * k - 1.0))
            st = cu.penalty_slack(host['rank_high'][:, :k], c['ds_x'], c['pos_x'], c['ds_y'], c['order_y'], k)
            sc = cu.penalty_slack(host['rank_low'][:, :k], c['ds_y'], c['pos_y'], c['ds_x'], c['order_x'], k)
            assert abs(dev['trustworthiness_curve'][k - 1] - host['trustworthiness_curve'][k - 1]) <= st * u + 1e-14, k
            assert abs(dev['continuity_curve'][k - 1] - host['continuity_curve'][k - 1]) <= sc * u + 1e-14, k
            moved = cu.overlap_slack(host['rank_high'][:, :k], c['ds_x'], c['ds_y'], k)
            assert abs(dev['qnx'][k - 1] - host['qnx'][k - 1]) <= moved / (N * k) + 1e-14, k
            assert abs(dev['lcmc'][k - 1] - host['lcmc'][k - 1]) <= moved / (N * k) + 1e-14, k
        assert dev['k_best'] == int(np.argmax(dev['lcmc'])) + 1
        assert dev['n_neighbors'] == K and dev['n_cells'] == N
        for key in ('cell_trustworthiness', 'cell_continuity'):
            assert [len(v) for v in dev[key]] == list(c['sizes']) and all(v.dtype == np.float64 for v in dev[key])
        assert abs(np.concatenate(dev['cell_trustworthiness']).mean() - dev['trustworthiness']) <= 1e-12

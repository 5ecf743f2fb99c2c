"""Layout quality, the parts that need no GPU: `JAMIE(metrics='host').test_layout` against sklearn's trustworthiness in both
directions, the numpy restatement of the device ranks (coranking_util.restated_list_ranks) against the float64 ranks, the curves
against separate calls and a direct overlap count, exact ranks on integer-valued cells, the exports and the argument checks.
Every figure is printed before it is asserted."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coranking_util as cu  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(w, K) for w in range(len(cu.SHAPES)) for K in cu.KS]


def _host(c, K, **kw):
    from jamie_amd import JAMIE
    return JAMIE(metrics='host').test_layout(c['high'], c['low'], n_neighbors=K, **kw)


@pytest.mark.parametrize('which,K', CASES)
def test_host_route_against_sklearn(which, K):
    """sklearn expands |x|^2 + |y|^2 - 2 x.y and searches the lists with its own neighbour search: a rank may move across the keys
    within REL_TOL relative of it, and a list may trade members whose keys straddle its end within REL_TOL.  The bound is the
    count of such places (coranking_util.penalty_slack), each worth 2 / (N K (2N - 3K - 1))."""
    from sklearn.manifold import trustworthiness
    c = cu.shape_case(which)
    N = len(c['X'])
    out = _host(c, K)
    rank_high, rank_low, _, _ = cu.reference_ranks(c, K)
    unit = 2.0 / (N * K * (2.0 * N - 3.0 * K - 1.0))
    X64, Y64 = c['X'].astype(np.float64), c['Y'].astype(np.float64)
    for name, got, want, slack in (
            ('trustworthiness', out['trustworthiness'], trustworthiness(X64, Y64, n_neighbors=K),
             cu.penalty_slack(rank_high, c['ds_x'], c['pos_x'], c['ds_y'], c['order_y'], K)),
            ('continuity', out['continuity'], trustworthiness(Y64, X64, n_neighbors=K),
             cu.penalty_slack(rank_low, c['ds_y'], c['pos_y'], c['ds_x'], c['order_x'], K))):
        print(f'{cu.SHAPES[which]} K = {K}: {name} {got:.9f}, sklearn {want:.9f}, difference {abs(got - want):.2e}, bound '
              f'{slack} places = {slack * unit:.2e}')
        assert abs(got - want) <= slack * unit + 1e-14
    assert out['n_neighbors'] == K and out['n_cells'] == N
    assert [len(v) for v in out['cell_trustworthiness']] == list(c['sizes'])
    assert [len(v) for v in out['cell_continuity']] == list(c['sizes'])
    assert abs(np.concatenate(out['cell_trustworthiness']).mean() - out['trustworthiness']) <= 1e-12
    assert abs(np.concatenate(out['cell_continuity']).mean() - out['continuity']) <= 1e-12


@pytest.mark.parametrize('which,K', CASES)
def test_restated_ranks_against_float64(which, K):
    """The fp32 chain of the device against float64 distances: equal at every entry with no other key of its row within REL_TOL
    relative of its own."""
    c = cu.shape_case(which)
    rank_high, rank_low, idx_high, idx_low = cu.reference_ranks(c, K)
    for name, Z, idx, want, ds in (('high', c['X'], idx_low, rank_high, c['ds_x']), ('low', c['Y'], idx_high, rank_low, c['ds_y'])):
        got = cu.restated_list_ranks(Z, idx)
        near = cu.near_keys(ds, want) > 0
        differ = got != want
        print(f'{cu.SHAPES[which]} K = {K}, ranks in {name}: {near.mean():.4f} of the entries have a key within 1e-5, '
              f'{int(differ.sum())} ranks differ, {int((differ & ~near).sum())} of them without one')
        assert near.mean() <= cu.EXCLUDED_CAP
        assert not np.any(differ & ~near)


def test_curves_against_separate_calls_and_the_overlap():
    c = cu.shape_case(1)
    K = 20
    out = _host(c, K, return_ranks=True)
    N = out['n_cells']
    for k in range(1, K + 1):
        one = _host(c, k)
        assert one['trustworthiness'] == out['trustworthiness_curve'][k - 1], k
        assert one['continuity'] == out['continuity_curve'][k - 1], k
        assert one['qnx'][k - 1] == out['qnx'][k - 1]
    for k in (1, 7, K):
        shared = sum(len(set(a[:k]) & set(b[:k])) for a, b in zip(out['idx_high'], out['idx_low']))
        assert out['qnx'][k - 1] == shared / (N * k), k
        # the same count from the other rank array: both orders are total
        assert np.count_nonzero(out['rank_low'][:, :k] < k) == shared
    assert np.array_equal(out['lcmc'], out['qnx'] - np.arange(1, K + 1) / (N - 1.0))
    assert out['k_best'] == int(np.argmax(out['lcmc'])) + 1 and 1 <= out['k_best'] <= K
    assert out['trustworthiness'] == out['trustworthiness_curve'][-1] and out['continuity'] == out['continuity_curve'][-1]
    assert out['rank_high'].shape == (N, K) and out['rank_high'].dtype == np.int32 and out['idx_low'].dtype == np.int32
    # a space against itself keeps everything
    same = _host(dict(high=c['high'], low=c['high']), K)
    assert same['trustworthiness'] == 1.0 and same['continuity'] == 1.0 and np.all(same['qnx'] == 1.0)
    # and a shuffled copy keeps nothing beyond chance
    rng = np.random.default_rng(0)
    noise = [rng.standard_normal((len(e), 2)).astype(np.float32) for e in c['high']]
    rand = _host(dict(high=c['high'], low=noise), K)
    print(f"random layout: trustworthiness {rand['trustworthiness']:.4f}, qnx[K] {rand['qnx'][-1]:.4f}")
    assert rand['trustworthiness'] < 0.6 and rand['qnx'][-1] < 0.1


@pytest.mark.parametrize('K', [64, 15])
def test_integer_cells_exact(K):
    """Heavy ties and duplicate cells: every q is exact in fp32, so the restatement equals the float64 route at every entry."""
    X = cu.integer_cells()
    Y = cu.integer_cells(L=2, seed=6)
    pos_x, order_x, ds_x = cu.full_order(X)
    pos_y, order_y, _ = cu.full_order(Y)
    print(f'cells whose K-th and (K+1)-th neighbours tie: {(ds_x[:, K - 1] == ds_x[:, K]).mean():.4f}')
    assert (ds_x[:, K - 1] == ds_x[:, K]).mean() > 0.5
    for Z, idx, pos in ((X, order_y[:, :K], pos_x), (Y, order_x[:, :K], pos_y)):
        got = cu.restated_list_ranks(Z, idx)
        assert np.array_equal(got, np.take_along_axis(pos, idx, axis=1))
    # the lists of the space itself rank 0 .. K - 1, in any order within the row
    own = order_x[:, :K][:, ::-1]
    assert np.array_equal(cu.restated_list_ranks(X, own), np.tile(np.arange(K)[::-1], (len(X), 1)))


def test_header_declarations_and_ctypes_arity():
    from jamie_amd import _native as nv
    hdr = open(os.path.join(ROOT, 'include', 'jamie_hip.h')).read()
    assert 'Layout quality on the device' in hdr
    for name in ('jamie_list_ranks_workspace', 'jamie_list_ranks', 'jamie_coranking_sums'):
        m = re.search(r'\b(?:int|long long) ' + name + r'\(([^)]*)\);', hdr)
        assert m, name
        assert name in nv.EXPORTS and len(nv.EXPORTS[name][1]) == m.group(1).count(',') + 1, name
    src = open(os.path.join(ROOT, 'jamie_amd', 'csrc', 'coranking.hip')).read()
    assert '#include "pair_tile.h"' in src and 'pair_tile<MI>(' in src and 'q_step(' in src


def test_exports_and_workspace_arithmetic():
    import jamie_amd
    jamie_amd.build_library()
    from jamie_amd import _native as nv
    handle = nv.load()
    for name in ('jamie_list_ranks_workspace', 'jamie_list_ranks', 'jamie_coranking_sums'):
        assert hasattr(handle, name), name
    ws = nv.list_ranks_workspace
    assert ws(1, 1) == 0 and ws(100, 0) == 0 and ws(1000, 65) == 0 and ws(1000, 5, 100) == 0 and ws(1000, 5, -128) == 0
    assert ws(2, 1) == 8 and ws(1000, 64, 256) == 1000 * 64 * 4 == ws(1000, 64) and ws(1000000, 15) == 1000000 * 15 * 4


def test_facade_host_route_runs(capsys):
    c = cu.shape_case(1)
    out = _host(c, 15)
    lines = capsys.readouterr().out.strip().splitlines()[-2:]
    assert lines == [f"trustworthiness: {out['trustworthiness']}", f"continuity: {out['continuity']}"]
    assert 0.5 < out['trustworthiness'] <= 1.0 and 0.5 < out['continuity'] <= 1.0
    for key in ('trustworthiness_curve', 'continuity_curve', 'qnx', 'lcmc'):
        assert out[key].shape == (15,) and out[key].dtype == np.float64
    assert 'rank_high' not in out
    # the host sums are the definition, entry by entry
    rank = np.array([[0, 5, -1], [3, 1, 9]])
    from jamie_amd.coranking import host_rank_sums
    pen, ov, cell = host_rank_sums(rank)
    assert pen.tolist() == [3, 6, 11] and ov.tolist() == [1, 2, 2] and cell.tolist() == [3, 8]


def test_arguments_are_checked():
    from jamie_amd import JAMIE
    from jamie_amd import coranking as jcr
    c = cu.shape_case(1)
    N = len(c['X'])
    jm = JAMIE(metrics='host')
    for k in (0, -3, 65, N // 2 + 1):
        with pytest.raises(ValueError, match='test_layout'):
            jm.test_layout(c['high'], c['low'], n_neighbors=k)
        with pytest.raises(ValueError, match='neighborhood_preservation'):
            jcr.neighborhood_preservation(c['high'], c['low'], n_neighbors=k)
    small = [e[:40] for e in c['high']]
    with pytest.raises(ValueError, match='test_layout'):
        jm.test_layout(small, [e[:40] for e in c['low']], n_neighbors=40)       # 40 is not below 80 / 2
    assert jm.test_layout(small, [e[:40] for e in c['low']], n_neighbors=39)['n_neighbors'] == 39
    with pytest.raises(ValueError, match='same cells'):
        jm.test_layout(c['high'], [c['low'][0], c['low'][1][:-1]])
    with pytest.raises(ValueError, match='same cells'):
        jcr.neighborhood_preservation(c['high'], [c['low'][0][1:], c['low'][1]])
    with pytest.raises(ValueError, match='one array per modality'):
        jm.test_layout(c['high'], c['low'][:1])
    with pytest.raises(ValueError, match='one array per modality'):
        jcr.neighborhood_preservation(c['high'][:1], c['low'])
    with pytest.raises(ValueError, match='one array per modality'):
        jm.test_layout([], [])
    bad = [c['low'][0].copy(), c['low'][1]]
    bad[0][3, 1] = np.nan
    with pytest.raises(ValueError):
        jm.test_layout(c['high'], bad)

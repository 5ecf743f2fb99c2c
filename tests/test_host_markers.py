"""Marker features without a GPU: the new symbols, the facade's host `rank_features` against scipy's Mann-Whitney, Welch and
Benjamini-Hochberg, the places where a statistic is NaN, the ranking order, the argument checks and the plan arithmetic."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import markers_util as mu  # noqa: E402

SYMBOLS = ('jamie_markers_workspace', 'jamie_group_rank_sums', 'jamie_group_moments')
FLOATS = ('auroc', 'z', 'pvals', 'pvals_adj', 'mean', 'var', 'mean_rest', 'var_rest', 't', 't_df', 't_pvals', 'logfoldchanges',
          'mean_difference')
INTS = ('n', 'rank_sum2', 'tie_term', 'U2', 'ranking')


def _host(X, labels, **kw):
    from jamie_amd import JAMIE
    return JAMIE(metrics='host').rank_features(X, labels, **kw)


def test_symbols_are_declared_and_exported():
    from jamie_amd import _native as nv
    hdr = open(os.path.join(ROOT, 'include', 'jamie_hip.h')).read()
    assert 'Marker features on the device' in hdr
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    handle = nv.load()
    for name in SYMBOLS:
        assert re.search(r'\b' + name + r'\s*\(', code), name
        assert name in nv.EXPORTS and hasattr(handle, name), name
    from jamie_amd import markers
    for name in ('rank_features', 'plan', 'finish', 'group_rank_sums', 'group_moments'):
        assert callable(getattr(markers, name)), name


def _case_300():
    rng = np.random.default_rng(5)
    N, d, G = 300, 6, 4
    labels = np.array(['b', 'a', 'd', 'c'])[rng.integers(0, G, N)]
    code = np.unique(labels, return_inverse=True)[1]
    X = np.round(rng.exponential(1.0, (N, d)) * 2) / 2 * (rng.random((N, d)) < 0.5)
    X += 0.5 * (code[:, None] == np.arange(d)[None, :] % G)
    X[:, 5] = rng.exponential(1.0, N) + 0.4 * (code == 1)                  # continuous, and positive as log1p data is
    return X, labels


def test_host_route_equals_scipy(capsys):
    from scipy import stats
    X, labels = _case_300()
    out = _host(X, labels)
    line = capsys.readouterr().out.strip().splitlines()[-1]
    assert line == f"rank_features: 4 groups, 6 features, largest |z| {float(np.nanmax(np.abs(out['z'])))}"
    assert list(out['groups']) == ['a', 'b', 'c', 'd'] and out['n'].sum() == 300
    for k in FLOATS:
        assert out[k].dtype == np.float64 and out[k].shape == (4, 6), k
    for k in INTS:
        assert out[k].dtype == np.int64, k
    assert out['rank_sum2'].shape == out['U2'].shape == (4, 6) and out['tie_term'].shape == (6,) and out['ranking'].shape == (4, 6)
    assert (out['tie_term'][:5] > 0).all() and out['tie_term'][5] == 0
    N = 300
    for g, name in enumerate(out['groups']):
        n_g = int((labels == name).sum())
        assert out['n'][g] == n_g
        for f in range(6):
            a, b = X[labels == name, f], X[labels != name, f]
            u = stats.mannwhitneyu(a, b, method='asymptotic', use_continuity=False)
            assert out['U2'][g, f] == 2 * u.statistic                  # exactly
            assert out['auroc'][g, f] == u.statistic / (n_g * (N - n_g))
            assert u.pvalue > 1e-300 and abs(out['pvals'][g, f] - u.pvalue) <= 1e-10 * u.pvalue
            assert (out['z'][g, f] > 0) == (out['auroc'][g, f] > 0.5)
            t = stats.ttest_ind(a, b, equal_var=False)
            assert t.pvalue > 1e-300 and abs(out['t_pvals'][g, f] - t.pvalue) <= 1e-10 * t.pvalue
            assert abs(out['t'][g, f] - t.statistic) <= 1e-10 * abs(t.statistic) and abs(out['t_df'][g, f] - t.df) <= 1e-10 * t.df
            assert abs(out['mean'][g, f] - a.mean()) <= 1e-13 and abs(out['mean_rest'][g, f] - b.mean()) <= 1e-13
            assert abs(out['var'][g, f] - a.var(ddof=1)) <= 1e-12 and abs(out['var_rest'][g, f] - b.var(ddof=1)) <= 1e-12
            assert abs(out['mean_difference'][g, f] - (a.mean() - b.mean())) <= 1e-13
            lfc = np.log2((np.expm1(a.mean()) + 1e-9) / (np.expm1(b.mean()) + 1e-9))
            assert abs(out['logfoldchanges'][g, f] - lfc) <= 1e-10
        adj = stats.false_discovery_control(out['pvals'][g])
        assert np.max(np.abs(out['pvals_adj'][g] - adj) / adj) <= 1e-10
    # the marked features lead their groups
    assert [int(r[0]) for r in out['ranking']] in ([0, 5, 2, 3], [4, 5, 2, 3], [0, 1, 2, 3], [4, 1, 2, 3])
    # integer labels and tensors give the same figures
    import torch
    code = np.unique(labels, return_inverse=True)[1]
    again = _host(torch.from_numpy(X), torch.from_numpy(code), n_top=2)
    assert np.array_equal(again['rank_sum2'], out['rank_sum2']) and again['z'].tobytes() == out['z'].tobytes()
    assert np.array_equal(again['ranking'], out['ranking'][:, :2])


def test_tie_correct_false_drops_the_tie_term():
    X, labels = _case_300()
    out, plain = _host(X, labels), _host(X, labels, tie_correct=False)
    N = 300.0
    ng = out['n'].astype(np.float64)[:, None]
    nr = N - ng
    want = (out['U2'] / 2.0 - ng * nr / 2.0) / np.sqrt(ng * nr / 12.0 * (N + 1.0))
    assert np.max(np.abs(plain['z'] - want)) <= 1e-13
    assert np.array_equal(plain['U2'], out['U2']) and np.array_equal(plain['tie_term'], out['tie_term'])
    tied = out['tie_term'] > 0
    assert (np.abs(plain['z'][:, tied]) < np.abs(out['z'][:, tied])).all()         # ties shrink the variance
    assert plain['z'][:, ~tied].tobytes() == out['z'][:, ~tied].tobytes()


def _nan_keys(out):
    return {k for k in FLOATS if np.isnan(out[k]).any()}


def test_nan_exactly_where_undefined():
    rng = np.random.default_rng(3)
    X = np.round(rng.exponential(1.0, (40, 4)) * 2) / 2
    # a single group: no rest
    one = _host(X, np.zeros(40, np.int64))
    assert one['n'].tolist() == [40] and one['U2'].tolist() == [[0] * 4]
    for k in ('auroc', 'z', 'pvals', 'pvals_adj', 'mean_rest', 'var_rest', 't', 't_df', 't_pvals', 'mean_difference', 'logfoldchanges'):
        assert np.isnan(one[k]).all(), k
    assert not np.isnan(one['mean']).any() and not np.isnan(one['var']).any()
    assert one['ranking'].tolist() == [[0, 1, 2, 3]]
    # a constant feature: z and t have no value, the AUROC is 1/2
    labels = rng.integers(0, 3, 40)
    Xc = X.copy()
    Xc[:, 2] = 1.5
    const = _host(Xc, labels)
    assert const['tie_term'][2] == 40 ** 3 - 40 and (const['auroc'][:, 2] == 0.5).all()
    for k in ('z', 'pvals', 'pvals_adj', 't', 't_df', 't_pvals'):
        assert np.isnan(const[k][:, 2]).all() and not np.isnan(np.delete(const[k], 2, axis=1)).any(), k
    assert (const['var'][:, 2] == 0).all() and (const['var_rest'][:, 2] == 0).all() and (const['mean'][:, 2] == 1.5).all()
    assert _nan_keys(const) == {'z', 'pvals', 'pvals_adj', 't', 't_df', 't_pvals'}
    assert _nan_keys(_host(Xc, labels, tie_correct=False)) == {'z', 'pvals', 'pvals_adj', 't', 't_df', 't_pvals'}
    # a group of one cell: no variance, no t; the rank statistics stand
    lone = labels.copy()
    lone[lone == 2] = 0
    lone[7] = 2
    single = _host(X, lone)
    assert single['n'].tolist()[2] == 1
    for k in ('var', 't', 't_df', 't_pvals'):
        assert np.isnan(single[k][2]).all() and not np.isnan(single[k][:2]).any(), k
    assert _nan_keys(single) == {'var', 't', 't_df', 't_pvals'}
    # ... and as the rest of the other group when there are two
    two = _host(X, (np.arange(40) == 7).astype(np.int64))
    assert np.isnan(two['var_rest'][0]).all() and np.isnan(two['var'][1]).all() and np.isnan(two['t']).all()
    assert not np.isnan(two['z']).any()


def test_signed_zeros_tie():
    x = np.array([-0.0, 0.0, 1.0, -0.0, 0.0, -1.0, 0.0, 2.0], np.float32)[:, None]
    assert np.signbit(x[0, 0]) and not np.signbit(x[1, 0])
    out = _host(x, np.array([0, 1, 0, 1, 0, 1, 0, 1]))
    assert out['tie_term'].tolist() == [5 ** 3 - 5]                    # the five zeros are one tie group
    # ranks: -1 -> 1, zeros -> 4 each, 1 -> 7, 2 -> 8
    assert out['rank_sum2'].tolist() == [[2 * (4 + 7 + 4 + 4)], [2 * (4 + 4 + 1 + 8)]]


def test_ranking_order():
    from jamie_amd import markers as jmk
    # z per feature, one group against one other: feature 1 and 3 tie, feature 2 is constant (NaN)
    X = np.array([[0, 5, 1, 5, 9], [1, 6, 1, 6, 8], [2, 1, 1, 1, 1], [3, 2, 1, 2, 0]], np.float64)
    out = _host(X, np.array([1, 1, 0, 0]), n_top=4)
    z = out['z'][1]
    assert np.isnan(z[2]) and z[1] == z[3] and z[4] == z[1] and z[0] < 0
    assert out['ranking'][1].tolist() == [1, 3, 4, 0]                  # ties by ascending index, the NaN beyond n_top
    assert out['ranking'][0].tolist() == [0, 1, 3, 4]
    full = _host(X, np.array([1, 1, 0, 0]))
    assert full['ranking'].shape == (2, 5) and full['ranking'][1].tolist() == [1, 3, 4, 0, 2]      # NaN last
    assert jmk.finish(out['groups'], out['n'], out['rank_sum2'], out['tie_term'], X[0], np.zeros((2, 5, 2)), 2)['ranking'].shape == (2, 2)


def test_bad_arguments_raise_value_error_without_a_gpu():
    from jamie_amd import JAMIE
    from jamie_amd import markers as jmk
    a = np.zeros((6, 3), np.float32)
    lab = np.arange(6) % 2
    too_many = np.broadcast_to(np.float32(0), (2 ** 21 + 1, 1))        # a shape, no memory behind it
    assert too_many.strides == (0, 0)
    routes = [JAMIE(metrics='host').rank_features, JAMIE(metrics='device').rank_features, jmk.rank_features]
    for fn in routes:
        for data, labels, kw in ((a[0], lab, {}), (a[:1], lab[:1], {}), (a[:, :0], lab, {}), (a, lab[:5], {}), (a, lab[:, None], {}),
                                 (a, lab, dict(n_top=0)), (a, lab, dict(n_top=1.5)), (too_many, lab, {})):
            with pytest.raises(ValueError):
                fn(data, labels, **kw)
    for fn in routes[1:]:
        with pytest.raises(ValueError):
            fn(a, lab, max_workspace=8 * jmk.CHUNK - 1)
    for bad in (np.nan, np.inf, -np.inf):
        b = a.copy()
        b[3, 1] = bad
        with pytest.raises(ValueError):
            routes[0](b, lab)
    with pytest.raises(ValueError):
        jmk.plan(2 ** 21 + 1, 4)
    with pytest.raises(ValueError):
        jmk.plan(1, 4)
    with pytest.raises(ValueError):
        jmk.plan(4, 0)


def test_plan_arithmetic():
    from jamie_amd import _native as nv
    from jamie_amd import markers as jmk
    C = jmk.CHUNK
    N = 2 ** 21
    assert jmk.MAX_CELLS == N and N ** 3 - N < 2 ** 63 and (N + 1) ** 3 - (N + 1) >= 2 ** 63 and 2 * N < 2 ** 32
    per = 8 * N                                                        # N is a multiple of CHUNK: no padding
    p = jmk.plan(N, 70, 30 * per + per - 1)
    assert p['Npad'] == N and p['runs'] == N // C == 512 and p['passes'] == 9
    assert p['groups'] == [(0, 30), (30, 30), (60, 10)] and p['workspace'] == 30 * per
    assert jmk.plan(N, 3, per)['groups'] == [(0, 1), (1, 1), (2, 1)]
    with pytest.raises(ValueError):
        jmk.plan(N, 3, per - 1)
    for n, runs, passes in ((2, 1, 0), (C, 1, 0), (C + 1, 2, 1), (2 * C + 1, 3, 2), (3 * C + 1, 4, 2), (N - 1, 512, 9)):
        p = jmk.plan(n, 10)
        assert (p['Npad'], p['runs'], p['passes']) == (runs * C, runs, passes), (n, p)
        assert p['groups'] == [(0, 10)] and p['workspace'] == 8 * p['Npad'] * 10
        assert nv.markers_workspace(n, 10, 5, 1) == p['workspace']
        assert nv.markers_workspace(n, 10, 5, 0) == (n // jmk.PIECE + 5) * 10 * 16
    assert [n for _, n in jmk.plan(2, 2 * jmk.MAX_GROUP + 1, 1 << 40)['groups']] == [jmk.MAX_GROUP, jmk.MAX_GROUP, 1]
    assert nv.markers_workspace(N + 1, 10, 5, 1) == 0 and nv.markers_workspace(0, 10, 5, 0) == 0
    assert nv.markers_workspace(10, 0, 5, 0) == 0 and nv.markers_workspace(10, 10, 0, 0) == 0 and nv.markers_workspace(10, 10, 5, 2) == 0


def test_group_layout_and_pieces():
    from jamie_amd import markers as jmk
    rng = np.random.default_rng(1)
    labels = rng.choice(np.array(['t', 'b', 'nk']), 1500, p=[0.8, 0.15, 0.05])
    lay = jmk.group_layout(labels)
    assert list(lay['groups']) == ['b', 'nk', 't'] and lay['n'].sum() == 1500
    assert lay['order'].dtype == lay['sorted_codes'].dtype == lay['seg_off'].dtype == lay['piece_off'].dtype == np.int32
    assert np.array_equal(lay['groups'][lay['sorted_codes']], labels[lay['order']])
    assert np.all(np.diff(lay['sorted_codes']) >= 0)
    for g in range(3):
        seg = lay['order'][lay['seg_off'][g]:lay['seg_off'][g + 1]]
        assert len(seg) == lay['n'][g] and np.all(np.diff(seg) > 0)    # stable: the cells of a group keep their order
    assert lay['piece_off'].tolist() == np.concatenate([[0], np.cumsum(-(-lay['n'] // jmk.PIECE))]).tolist()
    assert lay['piece_off'][-1] <= 1500 // jmk.PIECE + 3 and lay['n'][2] > 2 * jmk.PIECE


def test_restated_moments_meet_their_own_tolerance():
    """The tolerances of the device test are 8 x what the numpy restatement of the device's arithmetic shows on the same cases."""
    worst_mean = worst_var = worst_t = 0.0
    for N, d, G in mu.CASES:
        e_mean, e_var = mu.restated_error(N, d, G)
        worst_mean, worst_var, worst_t = max(worst_mean, e_mean), max(worst_var, e_var), max(worst_t, mu.restated_t_error(N, d, G))
    print(f'restatement against the two-pass reference: mean {worst_mean:.3e}, var {worst_var:.3e}; t against the host route {worst_t:.3e}')
    for worst, tol in ((worst_mean, mu.MEAN_TOL), (worst_var, mu.VAR_TOL), (worst_t, mu.T_TOL)):
        assert tol / 64 <= worst <= tol / 8 * 1.0001                   # the note beside them is current


def test_markers_kernels_use_no_scratch():
    """private_segment_fixed_size == 0 for every kernel of csrc/markers.hip, read from the code object hipcc built."""
    import isa_check as ic
    obj = os.path.join(ROOT, 'jamie_amd', 'csrc', '_obj', 'markers.o')
    if not os.path.exists(obj):
        pytest.skip('the library is not built')
    if not os.path.exists(ic.OBJDUMP):
        pytest.skip('llvm-objdump not found')
    meta = ic.kernel_metadata(obj)
    names = ' '.join(meta)
    for kernel in ('group_key_kernel', 'group_rank_kernel', 'group_moments_kernel', 'group_moments_final_kernel', 'chunk_sort_kernel',
                   'rank_merge_kernel'):
        assert kernel in names, (kernel, names)
    assert len(meta) == 6
    for name, m in meta.items():
        assert m['private_segment_fixed_size'] == 0, (name, m)
        assert m.get('vgpr_spill_count', 0) == 0, (name, m)

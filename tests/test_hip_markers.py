"""Marker features on the device (jamie_amd/markers.py, csrc/markers.hip) against the float64 host route and a two-pass reference.

`n`, `rank_sum2` and `tie_term` are integers and must equal the host route's exactly; `z`, `pvals`, `auroc` and `ranking` come from
them through the same `markers.finish` and must then be equal bit for bit, NaN included.  `mean` and `var` are held to
markers_util.MEAN_TOL / VAR_TOL, which are 8 x the distance of a numpy restatement of the device's arithmetic from the two-pass
reference -- never derived from the device's output.  Before a device result is looked at the reference alone must show that the
case is what it claims: NaN only where a statistic is undefined, ties present, groups that differ.  Every figure is printed before
it is asserted."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import markers_util as mu  # noqa: E402

pytestmark = pytest.mark.gpu

FLOATS = ('auroc', 'z', 'pvals', 'pvals_adj', 'mean', 'var', 'mean_rest', 'var_rest', 't', 't_df', 't_pvals', 'logfoldchanges',
          'mean_difference')
EXACT = ('auroc', 'z', 'pvals', 'pvals_adj')
INTS = ('n', 'rank_sum2', 'tie_term', 'U2')


@pytest.fixture(scope='module')
def jmk():
    from jamie_amd import markers
    return markers


def _check_reference(N, d, G):
    """The host route on the case, and what must hold of it alone."""
    X, labels = mu.case(N, d, G)
    ref = mu.host_reference(N, d, G)
    n = ref['n']
    groups = len(n)
    assert groups == min(G, N) and n.sum() == N and n.min() >= 1
    lone, lone_rest = n < 2, (N - n) < 2
    want = {k: np.zeros((groups, d), bool) for k in FLOATS}
    constant = np.ptp(X, axis=0) == 0
    if N > 2:                                                          # (N = 2: the two cells of the one column may be equal)
        assert list(np.where(constant)[0]) == ([mu.CONSTANT] if d > mu.CONSTANT else [])
    for k in ('z', 'pvals', 'pvals_adj', 't', 't_df', 't_pvals'):
        want[k][:, constant] = True
    if d > mu.OFFSET:
        want['logfoldchanges'][:, mu.OFFSET] = True                    # expm1(1e4) overflows on both sides: the column is not log1p data
    for k in ('var', 't', 't_df', 't_pvals'):
        want[k][lone] = True
    for k in ('var_rest', 't', 't_df', 't_pvals'):
        want[k][lone_rest] = True
    inflated = np.array([f for f in range(d) if f not in (mu.CONTINUOUS, mu.CONSTANT)])
    spread = np.abs(np.nanmean(ref['auroc'], axis=1) - 0.5)
    print(f'reference ({N}, {d}, {G}): groups of {n.min()} .. {n.max()} cells, {int(lone.sum())} of one; NaN '
          f'{ {k: int(np.isnan(ref[k]).sum()) for k in FLOATS if np.isnan(ref[k]).any()} }; smallest tie term of the zero-inflated '
          f'columns {ref["tie_term"][inflated].min()}; largest |mean AUROC - 0.5| of a group {spread.max():.4f}')
    for k in FLOATS:
        assert np.array_equal(np.isnan(ref[k]), want[k]), k
    assert (ref['tie_term'][inflated] > 0).all()
    assert np.array_equal(ref['tie_term'] == N ** 3 - N, constant)
    if N > 2:
        assert spread.max() > 1e-3                                     # the groups differ (N = 2: one cell against one)
    if G == 300 and N > 300:
        assert lone.sum() >= 20 and np.sum(n < 64) >= 250              # one-cell groups, and segments shorter than a wave
    return X, labels, ref


def _check_against(out, ref, X, labels):
    for k in INTS:
        print(f'{k}: {int((out[k] != ref[k]).sum())} entries off')
    for k in INTS + ('ranking',):
        assert out[k].dtype == np.int64 and np.array_equal(out[k], ref[k]), k
    for k in EXACT:
        assert out[k].dtype == np.float64 and out[k].tobytes() == ref[k].tobytes(), k
    for k in FLOATS:
        assert np.array_equal(np.isnan(out[k]), np.isnan(ref[k])), k
    mean, var = mu.reference_mean_var(X, labels)
    e_mean, e_var = mu.scaled_error(out['mean'], mean), mu.scaled_error(out['var'], var)
    print(f'mean: {e_mean:.3e} (tolerance {mu.MEAN_TOL:.3e}); var: {e_var:.3e} (tolerance {mu.VAR_TOL:.3e})')
    assert e_mean <= mu.MEAN_TOL and e_var <= mu.VAR_TOL
    # the statistics built on the moments, against the host route, whose sums are numpy's
    for k, tol in (('mean_rest', mu.MEAN_TOL), ('mean_difference', mu.MEAN_TOL), ('var_rest', mu.VAR_TOL), ('t', mu.T_TOL)):
        e = mu.scaled_error(out[k], ref[k])
        print(f'{k}: {e:.3e} from the host route (tolerance {tol:.3e})')
        assert e <= tol, k


def _same_bits(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in INTS + FLOATS + ('ranking',))


@pytest.mark.parametrize('N,d,G', mu.CASES)
def test_rank_features_equals_the_host_route(jmk, N, d, G):
    """N = 4097: a second sorted run of one real key; 8193: a third run that the first merge pass copies; 12289: four runs, two
    passes.  d = 130: three column tiles.  G = 300: one-cell groups, a wave's 64 cells span several groups."""
    X, labels, ref = _check_reference(N, d, G)
    out = jmk.rank_features(X, labels)
    _check_against(out, ref, X, labels)
    assert _same_bits(out, jmk.rank_features(X, labels))               # a second call: bit-identical


def test_single_group(jmk):
    X, _ = mu.case(257, 33, 7)
    labels = np.full(257, 'all')
    from jamie_amd.jamie import _host_rank_features
    ref = _host_rank_features(X, labels, 25, True)
    for k in ('auroc', 'z', 'pvals', 'mean_rest', 'var_rest', 't', 'mean_difference'):
        assert np.isnan(ref[k]).all(), k
    assert not np.isnan(ref['mean']).any() and not np.isnan(ref['var']).any()
    out = jmk.rank_features(X, labels)
    assert list(out['groups']) == ['all'] and out['n'].tolist() == [257]
    assert np.array_equal(out['rank_sum2'], np.full((1, 33), 257 * 258)) and np.array_equal(out['U2'], np.zeros((1, 33), np.int64))
    _check_against(out, ref, X, labels)


def test_signed_zeros_tie_on_the_device(jmk):
    x = np.array([-0.0, 0.0, 1.0, -0.0, 0.0, -1.0, 0.0, 2.0], np.float32)[:, None]
    assert np.signbit(x[0, 0]) and not np.signbit(x[1, 0])
    out = jmk.rank_features(x, np.array([0, 1, 0, 1, 0, 1, 0, 1]))
    print(f"tie term {out['tie_term'].tolist()}, rank sums {out['rank_sum2'].tolist()}")
    assert out['tie_term'].tolist() == [5 ** 3 - 5]
    assert out['rank_sum2'].tolist() == [[2 * (4 + 7 + 4 + 4)], [2 * (4 + 4 + 1 + 8)]]


def test_feature_groups_under_a_workspace_cap(jmk):
    N, d, G = 4097, 70, 300
    X, labels, ref = _check_reference(N, d, G)
    per = 8 * 2 * jmk.CHUNK
    assert jmk.plan(N, d, per)['groups'] == [(f, 1) for f in range(d)] and len(jmk.plan(N, d)['groups']) == 1
    groups = jmk.plan(N, d, 30 * per)['groups']
    print(f'groups under a cap of {30 * per} bytes: {groups}')
    assert groups == [(0, 30), (30, 30), (60, 10)]
    free = jmk.rank_features(X, labels)
    one = jmk.rank_features(X, labels, max_workspace=per)              # a feature at a time
    some = jmk.rank_features(X, labels, max_workspace=30 * per)
    assert np.array_equal(free['rank_sum2'], ref['rank_sum2']) and np.array_equal(free['tie_term'], ref['tie_term'])
    assert _same_bits(one, free) and _same_bits(some, free)
    with pytest.raises(ValueError):
        jmk.rank_features(X, labels, max_workspace=per - 1)


def test_a_permutation_of_the_cells_gives_the_same_integers(jmk):
    N, d, G = 8193, 33, 300
    X, labels, ref = _check_reference(N, d, G)
    perm = np.random.default_rng(11).permutation(N)
    out = jmk.rank_features(X[perm], labels[perm])
    for k in INTS + ('ranking',):
        assert np.array_equal(out[k], ref[k]), k
    for k in EXACT:
        assert out[k].tobytes() == ref[k].tobytes(), k


def test_tie_correct_false_n_top_and_input_kinds(jmk):
    N, d, G = 257, 33, 7
    X, labels, ref = _check_reference(N, d, G)
    plain_ref = mu.host_reference(N, d, G, False)
    assert not np.array_equal(plain_ref['z'][:, 0], ref['z'][:, 0])
    names = np.array([f'type {c}' for c in 'gfedcba'])[labels]         # strings whose order reverses the codes
    out = jmk.rank_features(torch.from_numpy(X.copy()).cuda(), names, n_top=3, tie_correct=False)
    assert list(out['groups']) == sorted(set(names)) and out['ranking'].shape == (G, 3)
    for k in ('n', 'rank_sum2', 'U2'):
        assert np.array_equal(out[k], plain_ref[k][::-1]), k
    assert np.array_equal(out['tie_term'], plain_ref['tie_term'])
    for k in EXACT:
        assert out[k].tobytes() == plain_ref[k][::-1].tobytes(), k
    assert np.array_equal(out['ranking'], plain_ref['ranking'][::-1, :3])
    again = jmk.rank_features(X.astype(np.float64), torch.from_numpy(labels.copy()), tie_correct=False)
    assert _same_bits(again, jmk.rank_features(X, labels, tie_correct=False))
    for bad in (np.nan, np.inf):
        b = X.copy()
        b[5, 7] = bad
        with pytest.raises(ValueError):
            jmk.rank_features(b, labels)


def test_facade_device_equals_the_module(jmk, capsys):
    from jamie_amd import JAMIE
    N, d, G = 4097, 130, 40
    X, labels, ref = _check_reference(N, d, G)
    dev = JAMIE(metrics='device').rank_features(X, labels, n_top=5)
    line = capsys.readouterr().out.strip().splitlines()[-1]
    assert line == f"rank_features: {G} groups, {d} features, largest |z| {float(np.nanmax(np.abs(ref['z'])))}"
    mod = jmk.rank_features(X, labels, n_top=5)
    assert set(dev) == set(mod) == set(ref) and _same_bits(dev, mod)
    assert np.array_equal(dev['ranking'], ref['ranking'][:, :5])


def _layout_on_device(jmk, labels):
    lay = jmk.group_layout(labels)
    return lay, {k: torch.from_numpy(lay[k]).cuda() for k in ('order', 'sorted_codes', 'seg_off', 'piece_off')}


def test_sort_stages(jmk):
    """last_stage = 2: every chunk of a column ascends; 3: the whole column does.  As multisets the keys are the column's order
    keys and the padding's sentinels; the sums are not formed."""
    from jamie_amd import _native as nv
    N, d, G = 8193, 33, 300
    X, labels = mu.case(N, d, G)
    lay, dv = _layout_on_device(jmk, labels)
    p = jmk.plan(N, d)
    Npad, C = p['Npad'], jmk.CHUNK
    assert (Npad, p['runs'], p['passes']) == (3 * C, 3, 2)             # two passes: the result is in the first buffer again
    x = torch.from_numpy(X.copy()).cuda()
    want = np.full((d, Npad), 0xFFFFFFFF, np.uint32)
    want[:, :N] = mu.order_keys(X.T.copy().reshape(-1)).reshape(d, N)
    assert (want[:, :N] != 0xFFFFFFFF).all()
    R2 = torch.full((d, len(lay['n'])), -1, dtype=torch.int64, device='cuda')
    tie = torch.full((d,), -1, dtype=torch.int64, device='cuda')
    for stage in (1, 2, 3):
        ws = torch.zeros(p['workspace'], dtype=torch.uint8, device='cuda')
        nv.group_rank_sums(x, dv['order'], dv['sorted_codes'], len(lay['n']), 0, d, R2, tie, ws, last_stage=stage)
        keys = ws.cpu().numpy().view(np.uint32)[:d * Npad].reshape(d, Npad)
        chunks = keys.reshape(d, Npad // C, C)
        sorted_chunks = bool(np.all(chunks[:, :, :-1] <= chunks[:, :, 1:]))
        sorted_columns = bool(np.all(keys[:, :-1] <= keys[:, 1:]))
        print(f'stage {stage}: chunks ascend {sorted_chunks}, columns ascend {sorted_columns}')
        assert np.array_equal(np.sort(keys, axis=1), np.sort(want, axis=1))
        if stage == 1:
            assert np.array_equal(keys, want)
        assert sorted_chunks == (stage >= 2) and sorted_columns == (stage >= 3)
        assert int(R2.abs().sum()) == 0 and int(tie.abs().sum()) == 0
    # a feature group in the middle leaves the other features' sums alone
    R2.fill_(-1)
    tie.fill_(-1)
    ws = torch.zeros(jmk.plan(N, 5)['workspace'], dtype=torch.uint8, device='cuda')
    nv.group_rank_sums(x, dv['order'], dv['sorted_codes'], len(lay['n']), 7, 5, R2, tie, ws)
    ref = mu.host_reference(N, d, G)
    got, got_tie = R2.cpu().numpy(), tie.cpu().numpy()
    assert np.array_equal(got[7:12], ref['rank_sum2'].T[7:12]) and np.array_equal(got_tie[7:12], ref['tie_term'][7:12])
    assert (got[:7] == -1).all() and (got[12:] == -1).all() and (got_tie[:7] == -1).all() and (got_tie[12:] == -1).all()


def test_moments_entry_point(jmk):
    """Through _native: the sums equal the numpy restatement's first moments exactly (additions in the same order) and its second
    moments to the last bits (the device may fuse dx * dx + acc)."""
    N, d, G = 4097, 70, 300
    X, labels = mu.case(N, d, G)
    lay = jmk.group_layout(labels)
    assert lay['n'].max() > 2 * jmk.PIECE and lay['piece_off'][-1] > len(lay['n'])
    pivot, sums = jmk.group_moments(torch.from_numpy(X.copy()).cuda(), lay)
    want_pivot, want = mu.restated_sums(X, labels)
    rel = float(np.max(np.abs(sums[:, :, 1] - want[:, :, 1]) / np.maximum(want[:, :, 1], 1e-300)))
    print(f'first moments off at {int((sums[:, :, 0] != want[:, :, 0]).sum())} entries; second moments within {rel:.3e} relative')
    assert np.array_equal(pivot, want_pivot) and np.array_equal(sums[:, :, 0], want[:, :, 0])
    assert rel <= 2.0 ** -44                                           # at most 512 roundings of 2^-53 apart


def test_entry_points_refuse_bad_arguments_without_a_launch(jmk):
    from jamie_amd import _native as nv
    N, d, G = 257, 33, 7
    X, labels = mu.case(N, d, G)
    lay, dv = _layout_on_device(jmk, labels)
    x = torch.from_numpy(X.copy()).cuda()
    R2 = torch.full((d, G), -1, dtype=torch.int64, device='cuda')
    tie = torch.full((d,), -1, dtype=torch.int64, device='cuda')
    sums = torch.full((G, d, 2), -1.0, dtype=torch.float64, device='cuda')
    ws = torch.zeros(max(nv.markers_workspace(N, d, G, 1), nv.markers_workspace(N, d, G, 0)), dtype=torch.uint8, device='cuda')
    order, codes, seg, piece = dv['order'], dv['sorted_codes'], dv['seg_off'], dv['piece_off']
    n_pieces = int(lay['piece_off'][-1])

    class Shape:                                                       # a tensor's pointer under another shape: nothing is read
        def __init__(self, t, shape):
            self.t, self.shape, self.is_cuda = t, shape, True

        def data_ptr(self):
            return self.t.data_ptr()

    too_many = Shape(x, (2 ** 21 + 1, d))
    for call in (lambda: nv.group_rank_sums(x, None, codes, G, 0, d, R2, tie, ws),
                 lambda: nv.group_rank_sums(x, order, codes, G, 0, d, None, tie, ws),
                 lambda: nv.group_rank_sums(too_many, order, codes, G, 0, d, R2, tie, ws),
                 lambda: nv.group_rank_sums(x, order, codes, G, 1, d, R2, tie, ws),
                 lambda: nv.group_rank_sums(x, order, codes, G, -1, 2, R2, tie, ws),
                 lambda: nv.group_rank_sums(x, order, codes, G, 0, 0, R2, tie, ws),
                 lambda: nv.group_rank_sums(x, order, codes, 0, 0, d, R2, tie, ws),
                 lambda: nv.group_rank_sums(x, order, codes, G, 0, d, R2, tie, ws[:nv.markers_workspace(N, d, G, 1) - 1]),
                 lambda: nv.group_rank_sums(x, order, codes, G, 0, d, R2, tie, ws, last_stage=5),
                 lambda: nv.group_moments(x, order, None, piece, G, n_pieces, sums, ws),
                 lambda: nv.group_moments(too_many, order, seg, piece, G, n_pieces, sums, ws),
                 lambda: nv.group_moments(x, order, seg, piece, G, 0, sums, ws),
                 lambda: nv.group_moments(x, order, seg, piece, G, N // jmk.PIECE + G + 1, sums, ws),
                 lambda: nv.group_moments(x, order, seg, piece, G, n_pieces, sums, ws[:nv.markers_workspace(N, d, G, 0) - 1])):
        with pytest.raises(nv.JamieHipError):
            call()
    torch.cuda.synchronize()
    assert int((R2 != -1).sum()) == 0 and int((tie != -1).sum()) == 0 and int((sums != -1.0).sum()) == 0       # nothing ran
    nv.group_rank_sums(x, order, codes, G, 0, d, R2, tie, ws)
    nv.group_moments(x, order, seg, piece, G, n_pieces, sums, ws)
    ref = mu.host_reference(N, d, G)
    assert np.array_equal(R2.cpu().numpy().T, ref['rank_sum2']) and np.array_equal(tie.cpu().numpy(), ref['tie_term'])

"""k-means, ARI and NMI, the parts that need no GPU: `JAMIE(metrics='host').test_clustering` against the float64 reference of
clustering_util.py and sklearn's two scores, what the figures say on inputs whose answer is known, the numpy restatement of the
device design against the float64 route (seeds, iterations and labels exactly, on cases whose margin implies it), the block order
of the weighted pick, the argument checks and the exports.  Every figure is printed before it is asserted."""
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clustering_util as cu  # noqa: E402
import lisi_util as lu  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ['jamie_kmeans_workspace', 'jamie_kmeans_step', 'jamie_kmeans_min_update', 'jamie_weighted_pick', 'jamie_contingency']


@pytest.fixture(scope='module')
def lib():
    import jamie_amd
    jamie_amd.build_library()
    from jamie_amd import _native
    return _native


def _sklearn_scores(true, pred):
    from sklearn.metrics import adjusted_rand_score, normalized_mutual_info_score
    return adjusted_rand_score(true, pred), normalized_mutual_info_score(true, pred, average_method='arithmetic')


def _labels_of(table):
    """(pred, true) code arrays that have the contingency table `table` [clusters, labels]."""
    pred = np.concatenate([np.full(int(v), i) for i, row in enumerate(table) for v in row])
    true = np.concatenate([np.full(int(v), j) for row in table for j, v in enumerate(row)])
    return pred, true


@pytest.mark.parametrize('case', [cu.CASES[4], cu.CASES[7], cu.CASES[12]])
def test_facade_host_route_equals_the_reference(case, capsys):
    from jamie_amd import JAMIE
    which, k, seed = case
    emb, lab, X = cu.case_data(which, seed)
    ref = cu.case_reference(which, k, seed)
    emb64 = [e.astype(np.float64) for e in emb]
    out = JAMIE().test_clustering(emb64, lab, n_clusters=k, n_init=cu.N_INIT, seed=seed)
    lines = capsys.readouterr().out.strip().splitlines()[-2:]
    assert lines == [f"ARI: {out['ari']}", f"NMI: {out['nmi']}"]
    clusters = np.concatenate(out['clusters'])
    assert [len(c) for c in out['clusters']] == [len(e) for e in emb] and clusters.dtype == np.int32
    assert np.array_equal(clusters, ref['labels']) and out['n_iter'] == ref['n_iter'] and out['run'] == ref['run']
    assert out['converged'] == ref['converged'] and out['n_empty'] == ref['n_empty']
    assert out['centers'].dtype == np.float64 and out['centers'].shape == (k, X.shape[1])
    rel_c = np.max(np.abs(out['centers'] - ref['centers'])) / np.max(np.abs(ref['centers']))
    rel_i = abs(out['inertia'] - ref['inertia']) / ref['inertia']
    print(f'host route against the reference: centres {rel_c:.2e}, inertia {rel_i:.2e}')
    assert rel_c <= 1e-12 and rel_i <= 1e-12
    assert out['sizes'].dtype == np.int64 and np.array_equal(out['sizes'], np.bincount(clusters, minlength=k))
    classes, lcode = np.unique(np.concatenate(lab), return_inverse=True)
    mod = np.repeat(np.arange(len(emb)), [len(e) for e in emb])
    assert np.array_equal(out['labels'], classes)
    assert np.array_equal(out['contingency'], cu.contingency_reference(clusters, lcode.reshape(-1), k, len(classes)))
    assert np.array_equal(out['modality_contingency'], cu.contingency_reference(clusters, mod, k, len(emb)))
    ari, nmi = _sklearn_scores(lcode.reshape(-1), clusters)
    print(f"ARI {out['ari']!r} (sklearn {ari!r}), NMI {out['nmi']!r} (sklearn {nmi!r})")
    assert abs(out['ari'] - ari) <= 1e-12 and abs(out['nmi'] - nmi) <= 1e-12
    # without labels: the same clustering, no scores; n_clusters defaults to the number of labels
    bare = JAMIE().test_clustering(emb64, n_clusters=k, n_init=cu.N_INIT, seed=seed)
    assert np.array_equal(np.concatenate(bare['clusters']), clusters)
    assert all(bare[name] is None for name in ('ari', 'nmi', 'contingency', 'labels'))
    assert capsys.readouterr().out.strip().splitlines()[-2:] == ['ARI: None', 'NMI: None']
    assert JAMIE().test_clustering(emb64, lab, n_init=1, max_iter=2)['centers'].shape[0] == len(classes)


@pytest.mark.parametrize('table', [
    [[30, 2, 0], [1, 40, 5], [0, 3, 25]],
    [[30, 2, 0], [0, 0, 0], [1, 40, 5], [4, 3, 25]],       # an empty cluster row
    [[17], [5], [9]],                                      # a single label
    [[12, 7, 3]],                                          # a single cluster
    [[31]],
    [[5, 0], [0, 7]],
])
def test_scores_equal_sklearn_on_tables(table):
    from jamie_amd.clustering import ari_nmi
    table = np.array(table)
    pred, true = _labels_of(table)
    ari, nmi = ari_nmi(table)
    want = _sklearn_scores(true, pred)
    print(f'ARI {ari!r} (sklearn {want[0]!r}), NMI {nmi!r} (sklearn {want[1]!r})')
    assert abs(ari - want[0]) <= 1e-12 and abs(nmi - want[1]) <= 1e-12
    rng = np.random.default_rng(table.size)
    big = rng.integers(0, 4000, (7, 5))
    pred, true = _labels_of(big)
    got, want = ari_nmi(big), _sklearn_scores(true, pred)
    assert abs(got[0] - want[0]) <= 1e-12 and abs(got[1] - want[1]) <= 1e-12
    for bad in (np.zeros((2, 2)), -np.ones((2, 2)), np.ones(3)):
        with pytest.raises(ValueError):
            ari_nmi(bad)


def test_figures_on_inputs_with_a_known_answer(capsys):
    from jamie_amd import JAMIE
    sizes, L = (400, 333), 8
    tight, lab = lu.mixture(7, lu.N_LABELS, L, sizes, spread=0.1)
    out = JAMIE().test_clustering(tight, lab)
    print(f"spread 0.1, k = T: ARI {out['ari']!r}, NMI {out['nmi']!r}, sizes {out['sizes']}")
    assert out['ari'] == 1.0 and out['nmi'] == 1.0 and out['n_empty'] == 0 and out['converged']
    assert np.count_nonzero(out['contingency']) == lu.N_LABELS
    rng = np.random.default_rng(3)
    shuffled = [rng.permutation(np.concatenate(lab))[:sizes[0]], rng.permutation(np.concatenate(lab))[:sizes[1]]]
    out = JAMIE().test_clustering(tight, shuffled)
    print(f"shuffled labels: ARI {out['ari']!r}")
    assert abs(out['ari']) < 0.05
    one = JAMIE().test_clustering(tight, lab, n_clusters=1)
    assert one['n_iter'] == 2 and one['converged']          # (the centre moves to the mean, then the labels repeat)
    assert one['ari'] == 0.0 and np.array_equal(one['sizes'], [sum(sizes)]) and not np.concatenate(one['clusters']).any()
    np.testing.assert_allclose(one['centers'][0], np.concatenate(tight).astype(np.float64).mean(axis=0), rtol=1e-12, atol=1e-12)


def test_runs_init_and_repeatability():
    from jamie_amd import JAMIE
    emb, lab, X = cu.case_data(1, 0)
    k, seed = 7, 7                                         # (a seed whose best run is not the first)
    X64 = X.astype(np.float64)
    singles = []
    for r in range(4):
        s = cu.seeds(X64, np.random.default_rng([seed, r]).random(k), False)
        one = JAMIE().test_clustering(emb, lab, n_clusters=k, init=X64[s], n_init=9)
        assert one['run'] == 0                              # init= forces one run
        singles.append(one['inertia'])
    out = JAMIE().test_clustering(emb, lab, n_clusters=k, n_init=4, seed=seed)
    print(f"inertia of runs 0 .. 3: {singles}; kept run {out['run']} at {out['inertia']!r}")
    assert len(set(singles)) > 1 and int(np.argmin(singles)) != 0
    assert out['run'] == int(np.argmin(singles)) and out['inertia'] == min(singles)
    again = JAMIE().test_clustering(emb, lab, n_clusters=k, n_init=4, seed=seed)
    for name in ('centers', 'sizes', 'contingency', 'modality_contingency'):
        assert np.array_equal(out[name], again[name])
    assert np.array_equal(np.concatenate(out['clusters']), np.concatenate(again['clusters']))
    assert (out['inertia'], out['n_iter'], out['run'], out['ari'], out['nmi']) == \
        (again['inertia'], again['n_iter'], again['run'], again['ari'], again['nmi'])
    other = JAMIE().test_clustering(emb, lab, n_clusters=k, n_init=1, seed=seed + 1)
    assert not np.array_equal(other['centers'], out['centers'])
    # max_iter = 1: one iteration, not converged (the labels have nothing to equal, the centres moved)
    first = JAMIE().test_clustering(emb, lab, n_clusters=k, n_init=1, seed=seed, max_iter=1)
    assert first['n_iter'] == 1 and not first['converged']


def test_design_restated():
    """The device's arithmetic in numpy (fp32 chain, fp32 centres, fp64 sums, the pick's block order) against the float64 route:
    the same seeds, iterations, winning run and labels on every case, whose float64 margin (asserted) is above band(L)."""
    assert len(cu.CASES) >= 12 and len(set(cu.CASES)) == len(cu.CASES)
    worst = 0.0
    for which, k, seed in cu.CASES:
        sizes, L, _ = lu.SHAPES[which]
        X = cu.case_data(which, seed)[2]
        ref, got = cu.case_reference(which, k, seed), cu.case_restated(which, k, seed)
        centre_sq = float((ref['centers'][ref['labels']] ** 2).sum())
        bound = cu.inertia_bound_rounded_centres(L, ref['inertia'], centre_sq)
        diff = abs(got['inertia'] - ref['inertia'])
        print(f"{sizes} L={L} k={k} seed={seed}: margin {ref['margin']:.3e} (band {cu.band(L):.3e}), n_iter {ref['n_iter']} / "
              f"{got['n_iter']}, run {ref['run']} / {got['run']}, inertia differs by {diff / ref['inertia']:.2e} "
              f"(bound {bound / ref['inertia']:.2e})")
        assert ref['margin'] > cu.band(L)
        assert np.array_equal(got['seeds'], ref['seeds']) and got['n_iter'] == ref['n_iter'] and got['run'] == ref['run']
        assert np.array_equal(got['labels'], ref['labels']) and got['converged'] == ref['converged']
        assert got['centers'].dtype == np.float32 and diff <= bound
        worst = max(worst, diff / ref['inertia'])
    print(f'largest relative inertia difference: {worst:.2e}')
    # the cases left out have margins below the band, as stated where they are replaced
    for which, k, seed in cu.REPLACED:
        assert cu.case_reference(which, k, seed)['margin'] <= cu.band(lu.SHAPES[which][1])


def test_pick_block_order():
    rng = np.random.default_rng(8)
    for n in (1, 5, 1023, 1024, 1025, 5000):
        w = rng.integers(0, 50, n).astype(np.float32)
        w[rng.integers(0, n, n // 3)] = 0
        for u in list(rng.random(25)) + [0.0, 1.0 - 2.0 ** -53]:
            assert cu.pick_restated(w, u) == cu.pick_float64(w, u), (n, u)
    # all weights 0: floor(u N)
    for u in (0.0, 0.37, 0.999):
        assert cu.pick_restated(np.zeros(2500, np.float32), u) == int(u * 2500) == cu.pick_float64(np.zeros(2500), u)
    # real weights: the pick's exact prefix straddles the exact target within the rounding of n fp64 additions
    w = (rng.random(5000) ** 4).astype(np.float32)
    exact = [math.fsum(w[:i + 1].astype(np.float64)) for i in range(len(w))]
    slack = len(w) * 2.0 ** -52 * exact[-1]
    moved = 0
    for u in rng.random(200):
        i = cu.pick_restated(w, u)
        moved += i != cu.pick_float64(w, u)
        assert exact[i] > u * exact[-1] - slack and (i == 0 or exact[i - 1] <= u * exact[-1] + slack)
    print(f'picks that differ from np.cumsum order on real weights: {moved} of 200')


@pytest.mark.parametrize('route', ['host', 'device'])
def test_value_errors_on_both_routes(route):
    """Every refusal comes from the shared argument checks, before either route touches a device."""
    from jamie_amd import JAMIE
    j = JAMIE(metrics=route)
    emb, lab = lu.mixture(1, 3, 4, (60, 50))
    bad = [emb[0].copy(), emb[1]]
    bad[0][3, 2] = np.nan
    refusals = [
        dict(datatype=[lab[0][:-1], lab[1]], n_clusters=3),            # one label per cell
        dict(datatype=lab[:1], n_clusters=3),
        dict(n_clusters=0), dict(n_clusters=111), dict(n_clusters=1025), dict(),          # k range; no labels and no k
        dict(n_clusters=3, init=np.zeros((3, 5))), dict(n_clusters=3, init=np.zeros((2, 4))), dict(n_clusters=3, init=np.zeros(4)),
        dict(n_clusters=3, init=np.full((3, 4), np.inf)),
        dict(n_clusters=3, n_init=0), dict(n_clusters=3, max_iter=0), dict(n_clusters=3, tol=-1e-9),
        dict(n_clusters=3, tol=float('nan')),
    ]
    for kw in refusals:
        with pytest.raises(ValueError):
            j.test_clustering(emb, **kw)
    for data in (bad, [emb[0], emb[1][:, :3]], []):
        with pytest.raises(ValueError):
            j.test_clustering(data, n_clusters=3)
    bad[0][3, 2] = np.inf
    with pytest.raises(ValueError):
        j.test_clustering(bad, lab)


def test_symbols_are_declared_and_exported(lib):
    hdr = open(os.path.join(ROOT, 'include', 'jamie_hip.h')).read()
    assert 'Clustering on the device' in hdr
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    handle = lib.load()
    for name in SYMBOLS:
        assert re.search(r'\b' + name + r'\s*\(', code), name
        assert name in lib.EXPORTS and hasattr(handle, name), name
    from jamie_amd import clustering
    for name in ('kmeans', 'kmeans_plusplus', 'assign', 'contingency', 'ari_nmi'):
        assert callable(getattr(clustering, name)), name


def _workspace_restated(N, L, k, seg_rows):
    S = -(-N // seg_rows)
    parts = -(-k * L // 256)
    return -(-(8 * S * k * L + 8 * S + 8 * parts + 4 * S * k + 4 * S) // 16) * 16


def test_workspace_arithmetic(lib):
    ws = lib.kmeans_workspace
    # refused arguments
    assert ws(0, 4, 1) == 0 and ws(100, 0, 5) == 0 and ws(100, 4, 0) == 0 and ws(100, 4, 101) == 0 and ws(5000, 4, 1025) == 0
    assert ws(1000, 4, 5, 100) == 0 and ws(1000, 4, 5, -128) == 0
    for N, L, k, seg in ((1301, 32, 5, 128), (1301, 32, 17, 256), (733, 8, 129, 384), (20000, 32, 40, 1280), (550, 100, 300, 128),
                         (1020, 3, 1020, 1024), (1, 1, 1, 128)):
        assert ws(N, L, k, seg) == _workspace_restated(N, L, k, seg), (N, L, k, seg)
    # the library's choice: whole 128-row tiles, one segment per tile while they all fit on the device at once
    for N in (1, 128, 129, 1301, 12800):
        assert ws(N, 32, 1) == _workspace_restated(N, 32, 1, 128)
    sizes = [ws(n, 32, 40) for n in (1000, 100000, 1000000)]
    assert 0 < sizes[0] < sizes[1] <= sizes[2]
    # at most two workgroups per compute unit (256 of them): the workspace stops growing with N
    assert ws(10 ** 7, 64, 256) <= _workspace_restated(512 * 128, 64, 256, 128)

"""LISI and the kNN graph, the parts that need no GPU: `JAMIE(metrics='host').test_lisi` / `.neighbors` against the float64
references of lisi_util.py, what the figures say on inputs whose answer is known, the numpy restatements of the device design
(fp32 distances into the fp64 solve; the two passes above a floor key for K > 64), the argument checks and the exports."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lisi_util as lu  # noqa: E402
import metrics_util as mu  # noqa: E402


@pytest.fixture(scope='module')
def lib():
    import jamie_amd
    jamie_amd.build_library()
    from jamie_amd import _native
    return _native


def _rel(a, b):
    return np.max(np.abs(a - b) / np.abs(b))


@pytest.mark.parametrize('which', [1, 3])
def test_facade_host_route_equals_the_reference(which, capsys):
    from jamie_amd import JAMIE
    c = lu.shape_case(which)
    K = c['K']
    u = K / 3
    ref, _, _ = lu.shape_lisi(which, u)
    emb64 = [e.astype(np.float64) for e in c['emb']]
    out = JAMIE().test_lisi(emb64, c['lab'], perplexity=u, n_neighbors=K)
    lines = capsys.readouterr().out.strip().splitlines()[-2:]
    assert lines == [f"iLISI (median): {out['ilisi_median']}", f"cLISI (median): {out['clisi_median']}"]
    print(f'host route against the reference: iLISI {_rel(out["ilisi"], ref[0]):.2e}, cLISI {_rel(out["clisi"], ref[1]):.2e}')
    assert _rel(out['ilisi'], ref[0]) <= 1e-12 and _rel(out['clisi'], ref[1]) <= 1e-12
    assert out['ilisi_median'] == np.nanmedian(out['ilisi']) and out['clisi_median'] == np.nanmedian(out['clisi'])
    assert out['ilisi_scaled'] == (out['ilisi_median'] - 1) / (c['M'] - 1)
    assert out['clisi_scaled'] == (c['T'] - out['clisi_median']) / (c['T'] - 1)
    assert out['n_neighbors'] == K and out['n_failed'] == 0
    assert np.array_equal(out['labels'], np.unique(np.concatenate(c['lab'])))
    # without labels: the same iLISI, no cLISI; the default k is min(int(3 u), N - 1)
    bare = JAMIE().test_lisi(emb64, perplexity=u, n_neighbors=K)
    assert np.array_equal(bare['ilisi'], out['ilisi']) and bare['clisi'] is None and bare['clisi_median'] is None
    assert bare['clisi_scaled'] is None and bare['labels'] is None
    assert capsys.readouterr().out.strip().splitlines()[-1] == 'cLISI (median): None'
    assert JAMIE().test_lisi([e[:40] for e in emb64], perplexity=5)['n_neighbors'] == 15
    assert JAMIE().test_lisi([e[:20] for e in emb64], perplexity=30)['n_neighbors'] == 39
    # the graph
    for k in (1, 15, K):
        g = JAMIE().neighbors(emb64, k=k)
        assert g.shape == (len(c['X']), len(c['X'])) and g.dtype == np.float64
        assert np.array_equal(np.diff(g.indptr), np.full(len(c['X']), k))
        assert np.array_equal(g.indices.reshape(-1, k), c['idx'][:, :k])
        assert _rel(g.data.reshape(-1, k), c['dist'][:, :k]) <= 1e-12
    g = JAMIE().neighbors(emb64, k=7, mode='connectivity')
    assert np.array_equal(g.data, np.ones(7 * len(c['X']))) and np.array_equal(g.indices.reshape(-1, 7), c['idx'][:, :7])


def test_figures_on_inputs_with_a_known_answer(capsys):
    from jamie_amd import JAMIE
    sizes, L = (400, 333), 8
    mixed, lab = lu.mixture(7, lu.N_LABELS, L, sizes, shift=0.0)
    out = JAMIE().test_lisi(mixed, lab)
    print(f"same mixture: iLISI median {out['ilisi_median']:.4f}, cLISI median {out['clisi_median']:.4f}")
    assert out['ilisi_median'] > 1.8
    assert 0.0 <= out['ilisi_scaled'] <= 1.0 and 0.0 <= out['clisi_scaled'] <= 1.0
    apart, lab = lu.mixture(7, lu.N_LABELS, L, sizes, shift=50.0)
    out = JAMIE().test_lisi(apart, lab)
    print(f"shift 50: iLISI median {out['ilisi_median']:.4f}")
    assert out['ilisi_median'] < 1.05
    assert 0.0 <= out['ilisi_scaled'] <= 1.0 and 0.0 <= out['clisi_scaled'] <= 1.0
    tight, lab = lu.mixture(7, lu.N_LABELS, L, sizes, spread=0.1)
    out = JAMIE().test_lisi(tight, lab)
    print(f"spread 0.1: cLISI median {out['clisi_median']:.4f}")
    assert out['clisi_median'] < 1.05
    assert 0.0 <= out['ilisi_scaled'] <= 1.0 and 0.0 <= out['clisi_scaled'] <= 1.0


def test_design_restated():
    """fp32 direct-difference distances into the float64 solve, against the all-float64 route, on the cells without a near tie
    at the K-th / (K + 1)-th neighbour: LISI_TOL is 4 x the largest relative difference printed here."""
    worst = 0.0
    for which, (sizes, L, K) in enumerate(lu.SHAPES):
        c = lu.shape_case(which)
        u = K / 3
        ref, _, _ = lu.shape_lisi(which, u)
        idx, dist = lu.restated_self_knn(c['X'], K)
        got, _, _ = lu.lisi_reference(idx, dist.astype(np.float64), np.stack([c['mod'], c['lcode']]), (c['M'], c['T']), u)
        amb = mu.near_tied(c['ds'], K)
        rel = np.max(np.abs(got - ref) / ref, axis=0)
        print(f'{sizes} L={L} K={K}: near-tied {amb.mean():.4f}, max relative |dLISI| off them {rel[~amb].max():.3e}, over all '
              f'cells {rel.max():.3e}')
        assert amb.mean() <= 0.03
        worst = max(worst, rel[~amb].max())
    print(f'largest: {worst:.3e}; LISI_TOL {lu.LISI_TOL:.3e}')
    assert lu.LISI_TOL <= 1e-4
    assert 2 * worst <= lu.LISI_TOL                        # (numpy's exp / log differ between builds in the last bit, too)


@pytest.mark.parametrize('K', [65, 90, 128])
def test_two_passes_equal_one_sort(K):
    from scipy.spatial.distance import cdist
    X = lu.integer_cells()
    q = (cdist(X, X) ** 2).astype(np.float32)
    np.fill_diagonal(q, np.inf)
    order = np.argsort(q, axis=1, kind='stable')
    seam = np.take_along_axis(q, order[:, 63:65], axis=1)
    print(f'cells whose 64th and 65th neighbours tie: {(seam[:, 0] == seam[:, 1]).mean():.4f}')
    assert (seam[:, 0] == seam[:, 1]).mean() > 0.9
    for i in range(len(X)):
        assert np.array_equal(lu.two_pass_select(q[i], K), order[i, :K]), i


@pytest.mark.parametrize('route', ['host', 'device'])
def test_value_errors_on_both_routes(route):
    """Every refusal comes from the shared argument checks, before either route touches a device."""
    from jamie_amd import JAMIE
    j = JAMIE(metrics=route)
    emb, lab = lu.mixture(1, 3, 4, (60, 50))
    with pytest.raises(ValueError):
        j.test_lisi(emb, lab, perplexity=1)
    with pytest.raises(ValueError):
        j.test_lisi(emb, lab, perplexity=0.5)
    with pytest.raises(ValueError):
        j.test_lisi(emb, lab, perplexity=20, n_neighbors=20)
    with pytest.raises(ValueError):
        j.test_lisi(emb, lab, perplexity=30, n_neighbors=25)
    big, big_lab = lu.mixture(1, 3, 4, (100, 100))
    with pytest.raises(ValueError):
        j.test_lisi(big, big_lab, perplexity=30, n_neighbors=129)
    with pytest.raises(ValueError):
        j.test_lisi(emb, lab, perplexity=30, n_neighbors=110)           # > N - 1 = 109
    with pytest.raises(ValueError):
        j.test_lisi(emb, [lab[0][:-1], lab[1]], perplexity=5)
    with pytest.raises(ValueError):
        j.test_lisi(emb, lab[:1], perplexity=5)
    with pytest.raises(ValueError):
        j.neighbors(big, k=0)
    with pytest.raises(ValueError):
        j.neighbors(big, k=129)
    with pytest.raises(ValueError):
        j.neighbors(emb, k=110)
    with pytest.raises(ValueError):
        j.neighbors(emb, k=5, mode='weights')


def test_nan_input_is_refused_on_the_host_route():
    from jamie_amd import JAMIE
    emb, lab = lu.mixture(1, 3, 4, (60, 50))
    bad = [emb[0].copy(), emb[1]]
    bad[0][3, 2] = np.nan
    with pytest.raises(ValueError):
        JAMIE().test_lisi(bad, lab, perplexity=5)
    with pytest.raises(ValueError):
        JAMIE().neighbors(bad, k=5)
    bad[0][3, 2] = np.inf
    with pytest.raises(ValueError):
        JAMIE().test_lisi(bad, lab, perplexity=5)


def test_exports_and_workspace_arithmetic(lib):
    handle = lib.load()
    for name in ('jamie_self_knn_workspace', 'jamie_self_knn', 'jamie_lisi'):
        assert name in lib.EXPORTS and hasattr(handle, name), name
    ws = lib.self_knn_workspace
    assert ws(1, 1) == 0 and ws(100, 0) == 0 and ws(1000, 129) == 0 and ws(1000, 5, 100) == 0 and ws(1000, 5, -128) == 0
    # S segments of N min(K, 64) (q, index) pairs, and a floor key per row beyond 64
    assert ws(1000, 5, 128) == 8 * 1000 * 5 * 8 and ws(1000, 64, 256) == 4 * 1000 * 64 * 8
    assert ws(1000, 65, 256) == 4 * 1000 * 64 * 8 + 1000 * 8 == ws(1000, 128, 256)
    assert ws(1000, 90, 1024) == 1000 * 64 * 8 + 1000 * 8
    sizes = [ws(n, 90) for n in (91, 1000, 100000, 1000000)]
    assert all(0 < a < b for a, b in zip(sizes, sizes[1:])) and sizes[-1] < 33 * 1000000 * 64 * 8 + 8000000

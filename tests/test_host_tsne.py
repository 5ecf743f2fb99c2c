"""The t-SNE layout, the parts that need no GPU: the float64 references of tsne_util.py on inputs whose answer is known, the numpy
restatement of the device design (where the gradient tolerance of test_hip_tsne.py comes from), `JAMIE(metrics='host').tsne` on
four blobs, the argument checks on both routes, the exports and the workspace arithmetic."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lisi_util as lu  # noqa: E402
import tsne_util as tu  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('jamie_tsne_affinities', 'jamie_tsne_mutual', 'jamie_tsne_fill', 'jamie_tsne_repulsion_workspace', 'jamie_tsne_repulsion',
           'jamie_tsne_step_workspace', 'jamie_tsne_step')


@pytest.fixture(scope='module')
def lib():
    import jamie_amd
    jamie_amd.build_library()
    from jamie_amd import _native
    return _native


def test_exports_and_header(lib):
    hdr = open(os.path.join(ROOT, 'include', 'jamie_hip.h')).read()
    assert 'Layout on the device' in hdr
    handle = lib.load()
    for name in SYMBOLS:
        assert name in lib.EXPORTS and hasattr(handle, name), name
        assert re.search(r'\b' + name + r'\s*\(', hdr), name


def _round16(b):
    return (b + 15) // 16 * 16


def _repulsion_workspace(N, seg_rows):
    """jamie_tsne_repulsion_workspace restated: S segments of 3 fp64 per row, and one fp64 per block of 256 rows."""
    tiles = -(-N // 128)
    if seg_rows == 0:
        S = max(1, min(1024 // -(-N // 1024), tiles))
        seg_rows = -(-tiles // S) * 128
    S = -(-N // seg_rows)
    return _round16(S * 3 * N * 8) + _round16(-(-N // 256) * 8)


def test_workspace_arithmetic(lib):
    ws = lib.tsne_repulsion_workspace
    assert ws(1) == 0 and ws(1000, 100) == 0 and ws(1000, -128) == 0 and ws(2 ** 31) == 0
    for N in (2, 8, 130, 257, 600, 1000, 1024, 1025, 20000, 200000, 1000000, 3000000):
        for seg in (0, 128, 256, 1024):
            if N / max(seg, 1) > 65535 and seg:
                continue
            assert ws(N, seg) == _repulsion_workspace(N, seg), (N, seg)
    assert ws(1000, 128) == 8 * 3 * 1000 * 8 + 32 and ws(1000, 0) == ws(1000, 128)
    # O(N): the segments shrink as the rows grow
    assert ws(1000000) <= 3 * 24 * 1000000 and ws(200000) <= 6 * 24 * 200000
    assert lib.tsne_step_workspace(1) == 0
    for N in (2, 130, 1001, 1000000):
        assert lib.tsne_step_workspace(N) == _round16(16 * N) + _round16(8 * N)


@pytest.mark.parametrize('route', ['host', 'device'])
def test_value_errors_on_both_routes(route):
    """Every refusal comes from the shared argument checks, before either route touches a device."""
    from jamie_amd import JAMIE
    from jamie_amd import tsne as jts
    j = JAMIE(metrics=route)
    emb, _ = lu.mixture(1, 3, 4, (60, 50))
    N = 110
    bad_nan = [emb[0].copy(), emb[1]]
    bad_nan[0][3, 2] = np.nan
    bad_inf = [emb[0].copy(), emb[1]]
    bad_inf[1][0, 0] = np.inf
    init_nan = np.zeros((N, 2), np.float32)
    init_nan[5, 1] = np.nan
    cases = [dict(perplexity=1), dict(perplexity=0.5), dict(perplexity=20, n_neighbors=20), dict(perplexity=30, n_neighbors=25),
             dict(perplexity=30, n_neighbors=110), dict(perplexity=30, n_neighbors=129), dict(n_iter=0),
             dict(n_iter=10, exaggeration_iter=11), dict(exaggeration_iter=-1), dict(early_exaggeration=0.5),
             dict(early_exaggeration=float('inf')), dict(early_exaggeration=float('nan')), dict(learning_rate=float('inf')),
             dict(learning_rate=float('nan')),
             dict(learning_rate=0), dict(learning_rate=-1.0), dict(learning_rate='fast'), dict(log_every=0), dict(init='umap'),
             dict(init=np.zeros((N, 3))), dict(init=np.zeros((N - 1, 2))), dict(init=init_nan), dict(seg_rows=100)]
    for kw in cases:
        kw = dict(dict(perplexity=10, n_iter=20, exaggeration_iter=5), **kw)
        with pytest.raises(ValueError):
            j.tsne(emb, **kw)
        if route == 'device':
            with pytest.raises(ValueError):
                jts.tsne(emb, **kw)
    for bad in (bad_nan, bad_inf, [emb[0], emb[1][:, :3]], []):
        with pytest.raises(ValueError):
            j.tsne(bad, perplexity=10, n_iter=20, exaggeration_iter=5)
        if route == 'device':
            with pytest.raises(ValueError):
                jts.tsne(bad, perplexity=10, n_iter=20, exaggeration_iter=5)


def test_reference_solve_on_the_lisi_shapes():
    from jamie_amd.jamie import _host_affinities
    for which, (sizes, L, K) in enumerate(lu.SHAPES):
        c = lu.shape_case(which)
        u = K / 3
        C, beta, tries, ent, margin = tu.affinity_reference(c['dist'], u)
        off = np.abs(ent - np.log(u))
        capped = tries >= 100
        near = margin < tu.NEAR_BRANCH
        print(f'{sizes} L={L} K={K}: largest |H - log u| {off.max():.3e}, at the cap {capped.mean():.4f}, near a branch '
              f'{near.mean():.4f}, tries {tries.min()} .. {tries.max()}, beta {beta.min():.3e} .. {beta.max():.3e}')
        assert np.all((off <= 1e-5) | capped)
        assert capped.mean() == 0
        assert near.mean() <= tu.NEAR_BRANCH_CAP
        assert np.abs(C.sum(axis=1) - 1).max() <= 1e-14 and np.all(C >= 0)
        hC, hbeta, htries = _host_affinities(c['dist'], u)
        assert np.array_equal(hC, C) and np.array_equal(hbeta, beta) and np.array_equal(htries, tries)


def test_reference_joint_matrix():
    for N in (8, 130, 600):
        c = tu.shape_case(N)
        C = tu.affinity_reference(c['dist'], c['u'])[0]
        P = tu.joint_reference(c['idx'], C)
        asym = abs(P - P.T).max()
        print(f'N = {N}: nnz {P.nnz}, |P - P^T| {asym:.1e}, |sum - 1| {abs(P.sum() - 1):.2e}')
        assert asym == 0 and abs(P.sum() - 1) <= 1e-12
        order = tu.row_order(c['idx'])
        assert sum(len(r) for r in order) == P.nnz
        for i in (0, N // 2, N - 1):
            assert sorted(order[i]) == list(P.indices[P.indptr[i]:P.indptr[i + 1]])


def _states(N):
    c = tu.shape_case(N)
    from jamie_amd import tsne as jts
    yield 'zero', np.zeros((N, 2), np.float32)
    yield 'init', jts.initial_layout(c['X'], 'pca', 0)
    yield 'spread', tu.spread_layout(N)


def test_design_restated():
    """fp32 pair arithmetic with fp32 partials over 32 columns into float64 sums, against all-float64: GRAD_TOL may not exceed
    4 x the largest figure printed here."""
    worst = 0.0
    for N in sorted(tu.SHAPES):
        c = tu.shape_case(N)
        C = tu.affinity_reference(c['dist'], c['u'])[0].astype(np.float32)
        P = tu.joint_reference(c['idx'], C).astype(np.float32).astype(np.float64)
        for name, Y in _states(N):
            ref = tu.gradient_reference(P, Y)
            for seg in (0, 128) + (tu.SEG_ROWS_LONG if N > 1024 else ()):
                err = tu.gradient_errors(tu.restated_gradient(P, Y, seg), ref)
                print(f'N = {N} {name} seg_rows = {seg}: ' + ', '.join(f'{k} {v:.3e}' for k, v in err.items()))
                if name == 'zero':
                    assert err['R'] == 0 and err['Z'] == 0 and ref['Z'] == N * (N - 1)
                worst = max(worst, *err.values())
    emb, _ = tu.blobs()
    X = np.concatenate(emb)
    idx, dist, _ = lu.knn_reference(X, 90)
    C = tu.affinity_reference(dist, 30)[0].astype(np.float32)
    P = tu.joint_reference(idx, C).astype(np.float32).astype(np.float64)
    Y = np.concatenate(tu.host_run(0)['layout'])
    err = tu.gradient_errors(tu.restated_gradient(P, Y), tu.gradient_reference(P, Y))
    print('blobs, the host route\'s final layout: ' + ', '.join(f'{k} {v:.3e}' for k, v in err.items()))
    worst = max(worst, *err.values())
    print(f'largest: {worst:.3e}; GRAD_TOL {tu.GRAD_TOL:.3e}')
    assert worst <= tu.GRAD_TOL <= 4 * worst


def test_host_route_on_four_blobs():
    from jamie_amd import tsne as jts
    emb, lab = tu.blobs()
    labels = np.concatenate(lab)
    finals = []
    for seed in (0, 1, 2):
        out = tu.host_run(seed)
        Y = np.concatenate(out['layout'])
        kl = out['kl_history']
        p = tu.purity(Y, labels)
        print(f'seed {seed}: KL at {list(out["logged_at"])} = {np.round(kl, 4)}, |grad| {out["grad_norm_history"][-1]:.2e}, 10-NN purity {p}')
        assert list(out['logged_at']) == [50, 100, 150, 200, 250, 300] and out['n_iter'] == 300 and out['n_neighbors'] == 90
        assert out['learning_rate'] == 50.0 and out['kl'] == kl[-1]
        assert [a.shape for a in out['layout']] == [(200, 2), (200, 2)] and out['layout'][0].dtype == np.float32
        assert np.all(np.diff(kl[1:]) <= 0)                 # (logged at 100: the layout the exaggeration leaves)
        assert p == 1.0
        finals.append(out['kl'])
    print(f'final KL of the three inits: {finals}, relative spread {(max(finals) - min(finals)) / min(finals):.3e}')
    X = np.concatenate(emb)
    for init in ('pca', 'random'):
        a, b = jts.initial_layout(X, init, 3), jts.initial_layout(X, init, 3)
        assert a.dtype == np.float32 and a.shape == (400, 2) and np.array_equal(a, b)
    assert not np.array_equal(jts.initial_layout(X, 'random', 3), jts.initial_layout(X, 'random', 4))
    pca = jts.initial_layout(X, 'pca', 0)
    assert abs(np.std(pca[:, 0].astype(np.float64)) - 1e-4) <= 1e-10 and np.std(pca[:, 1]) <= np.std(pca[:, 0])
    given = np.arange(800, dtype=np.float32).reshape(400, 2)
    assert np.array_equal(jts.initial_layout(X, given, 0), given)

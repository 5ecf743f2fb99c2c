"""Graph structure, the parts that need no GPU: the exports and the refusals, the argument checks on both routes,
the synchronous rounds in numpy against a breadth-first search and scipy on every shape case with their round counts, the host
route of JAMIE.test_graph on hand cases, its kBET against scipy.stats.chisquare, kBET's rates on mixed and on shifted modalities
and the per-label expected shares.  Every figure is printed before it is asserted."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graph_util as gu  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('jamie_graph_hook', 'jamie_graph_jump', 'jamie_kbet_stat')
KEYS = {'components', 'n_components', 'component_sizes', 'largest_share', 'modality_contingency', 'label_contingency', 'rounds', 'jumps',
        'graph_connectivity', 'label_connectivity', 'label_components', 'labels', 'kbet_rejection', 'kbet_acceptance', 'kbet_pvalues',
        'kbet_stat', 'kbet_tested', 'label_kbet_rejection', 'n_neighbors', 'n_edges', 'alpha', 'expected', 'graph'}


def host():
    from jamie_amd import JAMIE
    return JAMIE(metrics='host')


def test_symbols_are_declared_and_exported():
    from jamie_amd import _native as nv
    from jamie_amd import graph as jgr
    hdr = open(os.path.join(ROOT, 'include', 'jamie_hip.h')).read()
    assert 'Graph structure on the device' in hdr
    for s in SYMBOLS:
        assert s in nv.EXPORTS and f'{s}(' in hdr, s
    lib = nv.load()
    for s in SYMBOLS:
        assert hasattr(lib, s)
    src = open(os.path.join(ROOT, 'jamie_amd', 'csrc', 'graph.hip')).read()
    assert f'GR_GROUP = {gu.HOOK_GROUP};' in src and f'GR_LONG = {gu.HOOK_LONG};' in src
    assert f'KB_KMAX = {jgr.KBET_K_MAX};' in src and f'KB_BMAX = {jgr.KBET_B_MAX};' in src
    # the refusals come before any launch: no device is needed to see them
    assert lib.jamie_graph_hook(None, 8, 0, 4, None, 8, 16, 8, None) != 0 and b'null' in lib.jamie_last_error()
    assert lib.jamie_graph_hook(8, None, 3, 4, None, 8, 16, 8, None) != 0 and b'null' in lib.jamie_last_error()
    assert lib.jamie_graph_hook(8, 8, 0, 4, None, 8, 16, None, None) != 0
    assert lib.jamie_graph_hook(8, 8, 0, 0, None, 8, 16, 8, None) != 0 and b'2^31' in lib.jamie_last_error()
    assert lib.jamie_graph_hook(8, 8, 0, 1 << 31, None, 8, 16, 8, None) != 0
    assert lib.jamie_graph_hook(8, 8, -1, 4, None, 8, 16, 8, None) != 0
    assert lib.jamie_graph_hook(8, 8, 0, 4, None, 8, 8, 8, None) != 0 and b'differ' in lib.jamie_last_error()
    assert lib.jamie_graph_jump(8, 8, 4, 8, None) != 0 and b'differ' in lib.jamie_last_error()
    assert lib.jamie_graph_jump(8, 16, 0, 8, None) != 0
    assert lib.jamie_graph_jump(8, 16, 1 << 31, 8, None) != 0
    assert lib.jamie_graph_jump(8, 16, 4, None, None) != 0 and b'null' in lib.jamie_last_error()
    assert lib.jamie_kbet_stat(8, 4, 0, 8, 2, 8, 1, None, 8, 8, None, None) != 0
    assert lib.jamie_kbet_stat(8, 4, 129, 8, 2, 8, 1, None, 8, 8, None, None) != 0 and b'128' in lib.jamie_last_error()
    assert lib.jamie_kbet_stat(8, 4, 14, 8, 65, 8, 1, None, 8, 8, None, None) != 0 and b'64' in lib.jamie_last_error()
    assert lib.jamie_kbet_stat(8, 4, 14, 8, 0, 8, 1, None, 8, 8, None, None) != 0
    assert lib.jamie_kbet_stat(8, 4, 14, 8, 2, 8, 0, None, 8, 8, None, None) != 0
    assert lib.jamie_kbet_stat(8, 0, 14, 8, 2, 8, 1, None, 8, 8, None, None) != 0
    assert lib.jamie_kbet_stat(8, 4, 14, 8, 2, None, 1, None, 8, 8, None, None) != 0 and b'null' in lib.jamie_last_error()


def test_graph_kernels_use_no_scratch():
    """private_segment_fixed_size == 0 and no spills for the kernels of csrc/graph.hip, read from the code object hipcc built; the
    LDS is what DESIGN.md §26 states: a few words for the hook and the jump, 12 bytes x 64 categories x 16 cells (and two words
    per cell) for kBET."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import isa_check as ic
    obj = os.path.join(ROOT, 'jamie_amd', 'csrc', '_obj', 'graph.o')
    if not os.path.exists(obj):
        pytest.skip('the library is not built')
    if not os.path.exists(ic.OBJDUMP):
        pytest.skip('llvm-objdump not found')
    meta = ic.kernel_metadata(obj)
    names = ' '.join(meta)
    for kernel in ('gr_hook_kernel', 'gr_jump_kernel', 'kb_stat_kernel'):
        assert kernel in names, (kernel, names)
    assert len(meta) == 3
    for name, m in meta.items():
        print(name, {k: m.get(k) for k in ('vgpr_count', 'sgpr_count', 'group_segment_fixed_size', 'private_segment_fixed_size')})
        assert m['private_segment_fixed_size'] == 0, (name, m)
        assert m.get('vgpr_spill_count', 0) == 0 and m.get('sgpr_spill_count', 0) == 0, (name, m)
        lds = m.get('group_segment_fixed_size', 0)
        if 'kb_stat_kernel' in name:
            assert 12 * 64 * 16 <= lds <= 12 * 64 * 16 + 512, (name, m)
        else:
            assert lds <= 512, (name, m)


@pytest.mark.parametrize('route', ['host', 'device'])
def test_value_errors_on_both_routes(route):
    """Every refusal comes from the shared argument checks, names test_graph, and comes before either route touches a device."""
    from jamie_amd import JAMIE
    j = JAMIE(metrics=route)
    rng = np.random.default_rng(0)
    emb = [rng.standard_normal((60, 4)).astype(np.float32), rng.standard_normal((50, 4)).astype(np.float32)]
    lab = [np.arange(60) % 3, np.arange(50) % 3]
    bad_nan = [emb[0].copy(), emb[1]]
    bad_nan[0][3, 2] = np.nan
    cases = [dict(n_neighbors=1), dict(n_neighbors=111), dict(n_neighbors=130), dict(alpha=0.0), dict(alpha=1.0), dict(alpha=-0.1),
             dict(alpha=float('nan')), dict(expected='batch'), dict(expected='label'), dict(datatype=[lab[0]]),
             dict(datatype=[lab[0], lab[1][:-1]])]
    for kw in cases:
        with pytest.raises(ValueError, match='test_graph'):
            j.test_graph(emb, **kw)
    with pytest.raises(ValueError, match='test_graph: no embeddings'):
        j.test_graph([])
    with pytest.raises(ValueError, match='same features'):
        j.test_graph([emb[0], emb[1][:, :3]])
    with pytest.raises(ValueError, match='NaN or infinity'):
        j.test_graph(bad_nan)
    with pytest.raises(ValueError, match='n_neighbors = 15'):
        j.test_graph([emb[0][:10]])


@pytest.mark.parametrize('name', gu.CASES)
def test_numpy_rounds_equal_the_search_and_scipy(name):
    from jamie_amd import graph as jgr
    c = gu.graph_case(name)
    want = gu.bfs_components(c['rowptr'], c['col'], c['n'], c['group'])
    sc = gu.scipy_components(c['rowptr'], c['col'], c['n'], c['group'])
    run = gu.restated_rounds(c['rowptr'], c['col'], c['n'], c['group'])
    trace = []
    root, rounds, jumps = jgr.host_rounds(c['rowptr'], c['col'], c['n'], c['group'], trace)
    print(f"{name}: n {c['n']}, entries {len(c['col'])}, components {len(np.unique(want))}, rounds {run['rounds']} (bound "
          f"{gu.round_bound(c['n'])}), jumps {run['jumps']}")
    assert np.array_equal(sc, want)
    assert np.array_equal(run['root'], want) and run['root'].dtype == np.int32
    assert run['rounds'] <= gu.round_bound(c['n'])
    # the host route's own rounds are the restatement's, array for array
    assert (rounds, jumps) == (run['rounds'], run['jumps']) and np.array_equal(root, want)
    assert [t for t, _ in trace] == [t for t, _ in run['steps']]
    assert all(np.array_equal(a, b) for (_, a), (_, b) in zip(trace, run['steps']))


def test_round_counts_of_the_paths():
    counts = {name: gu.restated_rounds(**{k: gu.graph_case(name)[k] for k in ('rowptr', 'col', 'n')})['rounds']
              for name in ('path_up', 'path_down', 'path_zigzag', 'path_perm')}
    print(counts)
    assert counts['path_up'] == 2 and counts['path_down'] == 2 and counts['path_zigzag'] == 3
    assert 3 < counts['path_perm'] <= gu.round_bound(5000)


@functools.lru_cache(maxsize=None)
def three_blobs():
    X, blob = gu.blobs(11, (50, 40, 30), 4, 50.0)
    perm = np.random.default_rng(5).permutation(len(X))
    X, blob = X[perm].astype(np.float32), blob[perm]
    return [X[:70], X[70:]], [blob[:70], blob[70:]]


def test_host_route_on_three_far_blobs():
    emb, blob = three_blobs()
    out = host().test_graph(emb, blob, n_neighbors=5, return_graph=True)
    assert set(out) == KEYS
    print({k: out[k] for k in ('n_components', 'component_sizes', 'largest_share', 'rounds', 'jumps', 'graph_connectivity',
                               'label_connectivity', 'label_components', 'kbet_rejection', 'kbet_tested')})
    assert out['n_components'] == 3 and out['component_sizes'].tolist() == [50, 40, 30]
    assert out['largest_share'] == 50 / 120
    comp = np.concatenate(out['components'])
    assert comp.dtype == np.int32 and [c.shape[0] for c in out['components']] == [70, 50]
    assert np.array_equal(comp, np.concatenate(blob))                  # (ids by descending size: the blobs in their order)
    assert out['modality_contingency'].shape == (3, 2) and out['modality_contingency'].sum(axis=1).tolist() == [50, 40, 30]
    assert np.array_equal(out['label_contingency'], np.diag([50, 40, 30]))
    assert out['graph_connectivity'] == 1.0 and out['label_connectivity'].tolist() == [1.0] * 3
    assert out['label_components'].tolist() == [1, 1, 1] and out['labels'].tolist() == [0, 1, 2]
    assert out['graph'].shape == (120, 120) and out['n_edges'] == out['graph'].nnz and out['n_neighbors'] == 5
    # the components equal scipy's on the returned graph and the restated rounds' counts
    g = out['graph']
    want = gu.bfs_components(g.indptr, g.indices, 120)
    assert np.array_equal(gu.scipy_components(g.indptr, g.indices, 120), want)
    pooled = np.concatenate(out['components'])
    assert all(len(np.unique(want[pooled == c])) == 1 for c in range(3)) and len(np.unique(want)) == 3
    run = gu.restated_rounds(g.indptr, g.indices, 120)
    assert (out['rounds'], out['jumps']) == (run['rounds'], run['jumps'])
    assert 0.0 <= out['kbet_rejection'] <= 1.0 and out['kbet_acceptance'] == 1.0 - out['kbet_rejection']
    assert out['kbet_tested'] == 120 and out['label_kbet_rejection'].shape == (3,)


def test_host_route_label_of_two_far_blobs_and_single_embedding():
    emb, blob = three_blobs()
    X, b = np.concatenate(emb), np.concatenate(blob)
    keep = np.concatenate([np.nonzero(b == 0)[0], np.nonzero(b == 1)[0][:30], np.nonzero(b == 2)[0][:10]])
    X, b = X[keep], b[keep]
    labels = np.where(b == 0, 'near', 'split')                         # 'split' = the far blobs of 30 and 10 cells
    out = host().test_graph([X], [labels], n_neighbors=5)
    print({k: out[k] for k in ('n_components', 'component_sizes', 'graph_connectivity', 'label_connectivity', 'label_components')})
    assert out['n_components'] == 3 and out['component_sizes'].tolist() == [50, 30, 10]
    assert out['labels'].tolist() == ['near', 'split']
    assert out['label_connectivity'].tolist() == [1.0, 0.75] and out['label_components'].tolist() == [1, 2]
    assert out['graph_connectivity'] == (1.0 + 0.75) / 2
    for k in ('kbet_rejection', 'kbet_acceptance', 'kbet_pvalues', 'kbet_stat', 'kbet_tested', 'label_kbet_rejection'):
        assert out[k] is None, k
    assert out['graph'] is None
    plain = host().test_graph([X], n_neighbors=5)
    for k in ('graph_connectivity', 'label_connectivity', 'label_components', 'labels', 'label_contingency'):
        assert plain[k] is None, k
    assert np.array_equal(plain['components'][0], out['components'][0])


def test_host_kbet_equals_scipy_chisquare():
    from scipy.stats import chisquare
    from jamie_amd import graph as jgr
    from jamie_amd import jamie as jj
    rng = np.random.default_rng(2)
    N, K, B = 200, 14, 3
    X = rng.standard_normal((N, 5))
    codes = rng.integers(0, B, N)
    order = gu.knn_lists(X, K).astype(np.int64)
    shares = (np.bincount(codes, minlength=B) / N)[None, :]
    stat, df, counts = jj._host_kbet(order, codes, shares, None)
    p, rejected = jgr.kbet_decisions(stat, df, 0.05)
    rs, rdf, rcounts = gu.restated_kbet(order, codes, shares)
    assert np.array_equal(counts, rcounts) and np.array_equal(df, rdf) and np.array_equal(stat, rs)
    worst_s = worst_p = 0.0
    for i in range(N):
        o = np.bincount(codes[order[i]], minlength=B)
        ref = chisquare(o, K * shares[0])
        worst_s = max(worst_s, abs(stat[i] - ref.statistic) / max(1.0, abs(ref.statistic)))
        worst_p = max(worst_p, abs(p[i] - ref.pvalue))
    print(f'kBET vs scipy.stats.chisquare on {N} cells: statistic {worst_s:.3e}, p-value {worst_p:.3e}; rejected {int(rejected.sum())}')
    assert (df == B - 1).all() and worst_s <= 1e-12 and worst_p <= 1e-12
    assert np.array_equal(rejected, p < 0.05)


@functools.lru_cache(maxsize=None)
def two_modalities(shift):
    rng = np.random.default_rng(0)
    a = rng.standard_normal((1000, 8)).astype(np.float32)
    b = (rng.standard_normal((1000, 8)) + shift).astype(np.float32)
    return host().test_graph([a, b], n_neighbors=15)


def test_kbet_accepts_one_gaussian_in_two_modalities():
    out = two_modalities(0.0)
    print(f"mixed: kBET rejection {out['kbet_rejection']:.4f} of {out['kbet_tested']} cells, components {out['n_components']}")
    assert out['kbet_tested'] == 2000 and out['kbet_rejection'] <= 0.10
    assert out['kbet_acceptance'] == 1.0 - out['kbet_rejection']
    p = np.concatenate(out['kbet_pvalues'])
    assert out['kbet_rejection'] == float((p < 0.05).sum()) / 2000


def test_kbet_rejects_a_shifted_modality():
    out = two_modalities(20.0)
    print(f"shifted: kBET rejection {out['kbet_rejection']:.4f}, components {out['n_components']}")
    assert out['kbet_rejection'] == 1.0 and out['kbet_acceptance'] == 0.0
    assert out['n_components'] >= 2 and (out['modality_contingency'] > 0).sum(axis=1).tolist() == [1] * out['n_components']


def test_expected_label_uses_the_shares_of_the_label():
    from jamie_amd import graph as jgr
    rng = np.random.default_rng(4)
    # label A 3 : 1 over the two modalities, label B 1 : 3; the labels 30 apart
    nA, nB = (90, 30), (40, 120)
    emb = [np.concatenate([rng.standard_normal((nA[m], 4)), rng.standard_normal((nB[m], 4)) + 30.0]).astype(np.float32) for m in (0, 1)]
    lab = [np.array(['A'] * nA[m] + ['B'] * nB[m]) for m in (0, 1)]
    mod = np.repeat([0, 1], [sum(x) for x in zip(nA, nB)])
    lcode = np.concatenate([(lb == 'B').astype(np.int64) for lb in lab])
    shares, erow = jgr.expected_rows(mod, 2, lcode, 2, 'label')
    print(shares)
    assert np.array_equal(shares, np.array([[0.75, 0.25], [0.25, 0.75]])) and np.array_equal(erow, lcode)
    g_shares, g_erow = jgr.expected_rows(mod, 2, lcode, 2, 'global')
    assert g_erow is None and np.array_equal(g_shares, np.array([[130 / 280, 150 / 280]]))
    by_label = host().test_graph(emb, lab, n_neighbors=15, expected='label', return_graph=True)
    overall = host().test_graph(emb, lab, n_neighbors=15, expected='global')
    # per cell: the statistic under the shares of the cell's own label, on the lists of the returned graph
    g = by_label['graph']
    order = np.stack([g.indices[g.indptr[i]:g.indptr[i] + 14] for i in range(280)])
    rs, rdf, _ = gu.restated_kbet(order, mod, shares, lcode)
    assert np.array_equal(np.concatenate(by_label['kbet_stat']), rs) and by_label['expected'] == 'label'
    rs_g, _, _ = gu.restated_kbet(order, mod, g_shares)
    assert np.array_equal(np.concatenate(overall['kbet_stat']), rs_g)
    print(f"expected='label': rejection {by_label['kbet_rejection']:.4f} {by_label['label_kbet_rejection']}; 'global': "
          f"{overall['kbet_rejection']:.4f} {overall['label_kbet_rejection']}")
    # the labels are mixed at their own shares: under 'label' few cells are rejected, under 'global' more of them
    assert by_label['kbet_rejection'] <= 0.15 and by_label['kbet_rejection'] < overall['kbet_rejection']
    assert by_label['label_kbet_rejection'].shape == (2,) and by_label['graph_connectivity'] == 1.0

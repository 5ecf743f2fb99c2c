"""Graph structure on the device (jamie_amd/graph.py, csrc/graph.hip) against the restatements of graph_util.py: the array after
every hook and every completed compress element for element, the round and jump counts, the partition against scipy, two runs to
the bit; jamie_kbet_stat's counts, degrees of freedom and statistic to the bit; the facade's two routes; leiden's communities as
single components.  Every figure is printed before it is asserted."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graph_util as gu  # noqa: E402

pytestmark = pytest.mark.gpu

FUZZY = ('fuzzy5', 'fuzzy15')          # the fuzzy graph of 4 blobs x 500 cells at n_neighbors = 5 and 15
KBET_SHAPES = [(K, B) for K in (1, 14, 64, 128) for B in (1, 2, 3, 64)]


@pytest.fixture(scope='module')
def jgr():
    from jamie_amd import graph
    return graph


class Csr:
    def __init__(self, rowptr, col, n):
        self.rowptr = torch.from_numpy(np.ascontiguousarray(rowptr, dtype=np.int64)).cuda()
        self.col = torch.from_numpy(np.ascontiguousarray(col, dtype=np.int32)).cuda()
        self.n = int(n)


_cases = {}


def case(name):
    """(the graph on the device, dict(rowptr, col, n, group) on the host, the restated run) of a shape case or a fuzzy graph."""
    if name not in _cases:
        if name in FUZZY:
            from jamie_amd import spectral as jsp
            X, _ = gu.blobs(21, (500, 500, 500, 500), 8, 12.0)
            G = jsp.build_graph(torch.from_numpy(X.astype(np.float32)).cuda(), int(name[5:]))
            c = dict(rowptr=G.rowptr.cpu().numpy(), col=G.col.cpu().numpy(), n=G.n, group=None)
        else:
            c = gu.graph_case(name)
            G = Csr(c['rowptr'], c['col'], c['n'])
        _cases[name] = (G, c, gu.restated_rounds(c['rowptr'], c['col'], c['n'], c['group']))
    return _cases[name]


@pytest.mark.parametrize('name', gu.CASES + FUZZY)
def test_every_hook_and_compress_equals_the_restatement(jgr, name):
    G, c, want = case(name)
    trace = []
    label, rounds, jumps = jgr.components(G, group=c['group'], trace=trace)
    print(f"{name}: n {c['n']}, entries {len(c['col'])}, longest row {int(np.diff(c['rowptr']).max())}, components "
          f"{len(np.unique(want['root']))}, rounds {rounds} (restated {want['rounds']}), jumps {jumps} (restated {want['jumps']})")
    assert [t for t, _ in trace] == [t for t, _ in want['steps']]
    for (tag, got), (_, ref) in zip(trace, want['steps']):
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), ref), tag
    assert (rounds, jumps) == (want['rounds'], want['jumps'])
    assert label.dtype == torch.int32 and np.array_equal(label.cpu().numpy(), want['root'])
    # scipy's partition, ids mapped through their smallest member
    assert np.array_equal(label.cpu().numpy(), gu.scipy_components(c['rowptr'], c['col'], c['n'], c['group']))
    again, r2, j2 = jgr.components(G, group=c['group'])
    assert torch.equal(again, label) and (r2, j2) == (rounds, jumps)


def test_one_launch_of_each_kernel_on_a_given_state(jgr):
    """A hook and a jump from a state that is not the first round's: the root of the restatement's second round."""
    from jamie_amd import _native as nv
    G, c, want = case('n65537')
    roots = [a for t, a in want['steps'] if t == 'root']
    hooks = [a for t, a in want['steps'] if t == 'hook']
    root = torch.from_numpy(roots[0]).cuda()
    parent = root.clone()
    flag = torch.zeros(2, dtype=torch.int32, device='cuda')
    nv.graph_hook(G.rowptr, G.col, None, root, parent, flag[0:1])
    assert np.array_equal(parent.cpu().numpy(), hooks[1]) and np.array_equal(root.cpu().numpy(), roots[0])
    out = torch.empty_like(parent)
    nv.graph_jump(parent, out, flag[1:2])
    assert np.array_equal(out.cpu().numpy(), hooks[1][hooks[1]]) and flag.cpu().tolist() == [1, 1]
    # at the fixed point neither kernel raises its flag
    last = torch.from_numpy(want['root']).cuda()
    parent, flag = last.clone(), torch.zeros(2, dtype=torch.int32, device='cuda')
    nv.graph_hook(G.rowptr, G.col, None, last, parent, flag[0:1])
    nv.graph_jump(parent, out, flag[1:2])
    assert torch.equal(parent, last) and torch.equal(out, last) and flag.cpu().tolist() == [0, 0]


def test_components_raises_before_returning_a_half_merged_labelling(jgr):
    G, c, want = case('path_perm')
    assert want['rounds'] > 2
    with pytest.raises(RuntimeError, match='max_rounds = 1'):
        jgr.components(G, max_rounds=1)
    with pytest.raises(RuntimeError, match='max_rounds'):
        jgr.components(G, max_rounds=want['rounds'] - 1)
    label, rounds, _ = jgr.components(G, max_rounds=want['rounds'])
    assert rounds == want['rounds'] and int(label.max()) == 0
    with pytest.raises(ValueError, match='one group per node'):
        jgr.components(G, group=np.zeros(7, np.int32))


def test_neighbour_lists_as_a_graph(jgr):
    _, c, want = case('knn')
    idx = c['col'].reshape(c['n'], 14)
    label, rounds, jumps = jgr.components(jgr.lists_as_csr(idx))
    assert np.array_equal(label.cpu().numpy(), want['root']) and (rounds, jumps) == (want['rounds'], want['jumps'])
    import jamie_amd
    assert jamie_amd.components is jgr.components


def kbet_inputs(K, B, N=403):
    rng = np.random.default_rng(1000 * K + B)
    idx = rng.integers(0, N, (N, K)).astype(np.int32)
    codes = rng.integers(0, B, N).astype(np.int32)
    shares = rng.random((3, B)) + 0.05
    if B >= 3:
        shares[1, B - 1] = 0.0                          # a category the cells of row 1 do not expect
    shares /= shares.sum(axis=1, keepdims=True)
    erow = rng.integers(0, 3, N).astype(np.int32)
    # the special rows: entries -1 and N; every entry outside (k_i = 0); a code outside [0, B)
    idx[0, :] = -1
    idx[1, :] = N
    idx[2, 0] = -1
    idx[3, K - 1] = N
    codes[5] = B
    codes[6] = -1
    if B >= 3:
        # cell 10 uses row 1 and sees no cell of the category that row does not expect (df is one less); cell 11 sees one (NaN)
        quiet = np.nonzero((codes >= 0) & (codes < B - 1))[0].astype(np.int32)
        erow[10] = erow[11] = 1
        idx[10, :] = quiet[rng.integers(0, len(quiet), K)]
        idx[11, :] = idx[10, :]
        idx[11, 0] = np.nonzero(codes == B - 1)[0][0]
    return idx, codes, shares, erow


@pytest.mark.parametrize('K,B', KBET_SHAPES)
def test_kbet_statistic_equals_the_restatement_to_the_bit(jgr, K, B):
    idx, codes, shares, erow = kbet_inputs(K, B)
    N = len(idx)
    for rows in (erow, None):
        got = jgr.kbet_from_neighbors(idx, codes, shares, rows, alpha=0.05, return_counts=True)
        stat, df, counts = gu.restated_kbet(idx, codes, shares, rows)
        ok = (codes[np.clip(idx, 0, N - 1)] >= 0) & (codes[np.clip(idx, 0, N - 1)] < B) & (idx >= 0) & (idx < N)
        binc = np.stack([np.bincount(codes[idx[i][ok[i]]], minlength=B) for i in range(N)])
        tested = ~np.isnan(stat)
        rel = np.abs(got['stat'][tested] - stat[tested]) / np.maximum(np.abs(stat[tested]), 1e-300)
        print(f"K {K} B {B} erow {rows is not None}: tested {int(tested.sum())} of {N}, df {np.unique(df).tolist()}, worst relative "
              f"difference {rel.max() if rel.size else 0.0:.3e} (bound {(B + 4) * gu.U:.3e})")
        assert np.array_equal(got['counts'], binc) and np.array_equal(binc, counts) and got['counts'].dtype == np.int32
        assert np.array_equal(got['df'], df) and got['df'].dtype == np.int32
        assert np.array_equal(np.isnan(got['stat']), ~tested)
        assert rel.size == 0 or rel.max() <= (B + 4) * gu.U
        assert np.array_equal(got['stat'][tested], stat[tested])         # the operation order is held: the same bits
        assert not tested[0] and not tested[1] and df[0] == 0            # k_i = 0
        if B == 1:
            assert not tested.any() and (got['df'] == 0).all()           # df < 1: nothing is tested
        if B >= 3 and rows is not None:
            assert tested[10] and df[10] == B - 2 and not tested[11] and df[11] == 0
        p = got['pvalues']
        assert np.array_equal(np.isnan(p), ~tested) and np.array_equal(got['rejected'], tested & (np.nan_to_num(p, nan=1.0) < 0.05))
    with pytest.raises(ValueError, match='erow'):
        jgr.kbet_from_neighbors(idx, codes, shares, np.full(N, 3))


def restated_dict_checks(out, emb, labels, nn, alpha, expected):
    """The device route's dict against the restatements on the device's own graph."""
    g = out['graph']
    N = g.shape[0]
    n_cells = [len(e) for e in emb]
    mod = np.repeat(np.arange(len(emb)), n_cells)
    run = gu.restated_rounds(g.indptr, g.indices, N)
    root = gu.bfs_components(g.indptr, g.indices, N)
    assert np.array_equal(run['root'], root) and (out['rounds'], out['jumps']) == (run['rounds'], run['jumps'])
    ids, first, counts = np.unique(root, return_index=True, return_counts=True)
    rank = sorted(range(len(ids)), key=lambda c: (-int(counts[c]), int(first[c])))
    new = np.empty(len(ids), np.int64)
    new[rank] = np.arange(len(ids))
    comp = new[np.searchsorted(ids, root)]
    got = np.concatenate(out['components'])
    assert got.dtype == np.int32 and np.array_equal(got, comp) and [len(c) for c in out['components']] == n_cells
    assert out['n_components'] == len(ids) and np.array_equal(out['component_sizes'], np.sort(counts)[::-1])
    assert out['largest_share'] == float(counts.max()) / float(N)
    table = np.zeros((len(ids), len(emb)), np.int64)
    np.add.at(table, (comp, mod), 1)
    assert np.array_equal(out['modality_contingency'], table)
    assert out['n_edges'] == g.nnz and out['n_neighbors'] == nn and out['alpha'] == alpha and out['expected'] == expected
    if labels is None:
        assert out['graph_connectivity'] is None and out['label_connectivity'] is None and out['label_components'] is None
    else:
        classes, lcode = np.unique(np.concatenate(labels), return_inverse=True)
        groot = gu.bfs_components(g.indptr, g.indices, N, lcode)
        share, count = [], []
        for t in range(len(classes)):
            sizes = np.unique(groot[lcode == t], return_counts=True)[1]
            share.append(float(sizes.max()) / float(sizes.sum()))
            count.append(len(sizes))
        assert np.array_equal(out['labels'], classes) and np.array_equal(out['label_connectivity'], np.array(share))
        assert np.array_equal(out['label_components'], np.array(count)) and out['graph_connectivity'] == float(np.mean(share))
    if len(emb) > 1:
        from scipy.special import chdtrc
        K = nn - 1
        order = np.stack([g.indices[g.indptr[i]:g.indptr[i] + K] for i in range(N)])
        if expected == 'global':
            shares, erow = (np.bincount(mod) / float(N))[None, :], None
        else:
            shares = np.stack([np.bincount(mod[lcode == t], minlength=len(emb)) / float((lcode == t).sum()) for t in range(len(classes))])
            erow = lcode
        stat, df, _ = gu.restated_kbet(order, mod, shares, erow)
        tested = ~np.isnan(stat)
        p = np.full(N, np.nan)
        p[tested] = chdtrc(df[tested].astype(np.float64), stat[tested])
        assert np.array_equal(np.concatenate(out['kbet_stat']), stat, equal_nan=True)
        assert np.array_equal(np.concatenate(out['kbet_pvalues']), p, equal_nan=True)
        assert out['kbet_tested'] == int(tested.sum())
        assert out['kbet_rejection'] == float((p[tested] < alpha).sum()) / int(tested.sum())
        assert out['kbet_acceptance'] == 1.0 - out['kbet_rejection']
    else:
        assert out['kbet_rejection'] is None and out['kbet_stat'] is None and out['kbet_pvalues'] is None


def same_dicts(a, b):
    assert set(a) == set(b)
    for k in a:
        if k == 'graph':
            assert (a[k] is None) == (b[k] is None)
            if a[k] is not None:
                assert np.array_equal(a[k].indptr, b[k].indptr) and np.array_equal(a[k].indices, b[k].indices)
        elif isinstance(a[k], list):
            assert len(a[k]) == len(b[k]) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a[k], b[k])), k
        elif isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == 'f'), k
        else:
            assert a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]), k


def test_facade_on_the_device_against_the_restatement_on_its_own_graph():
    from jamie_amd import JAMIE
    rng = np.random.default_rng(8)
    centres = rng.standard_normal((5, 8)) * 2.5
    emb, lab = [], []
    for m, n in enumerate((700, 500)):
        c = rng.integers(0, 5, n)
        emb.append((centres[c] + rng.standard_normal((n, 8)) + 0.4 * m).astype(np.float32))
        lab.append(np.array(['t%d' % v for v in c]))
    dev = JAMIE(metrics='device')
    for labels, nn, expected in ((lab, 15, 'global'), (lab, 6, 'label'), (None, 4, 'global')):
        out = dev.test_graph(emb, labels, n_neighbors=nn, alpha=0.05, expected=expected, return_graph=True)
        restated_dict_checks(out, emb, labels, nn, 0.05, expected)
        again = dev.test_graph(emb, labels, n_neighbors=nn, alpha=0.05, expected=expected, return_graph=True)
        same_dicts(out, again)
    single = dev.test_graph([emb[0]], [lab[0]], n_neighbors=5, return_graph=True)
    restated_dict_checks(single, [emb[0]], [lab[0]], 5, 0.05, 'global')
    for k in ('kbet_rejection', 'kbet_acceptance', 'kbet_pvalues', 'kbet_stat', 'kbet_tested', 'label_kbet_rejection'):
        assert single[k] is None, k


@pytest.mark.parametrize('data', ['integers', 'blobs'])
def test_the_two_routes_return_the_same_dict(data):
    """Integer-valued cells (every distance exact in fp32 and float64, ties by the lower index on both routes) and well-separated
    blobs of distinct cells: the neighbour lists of the two routes are equal there, and so is every key but the graph's values."""
    from jamie_amd import JAMIE
    rng = np.random.default_rng(12)
    if data == 'integers':
        emb = [rng.integers(-6, 7, (260, 3)).astype(np.float32), rng.integers(-6, 7, (220, 3)).astype(np.float32) + np.float32(2.0)]
        lab = [rng.integers(0, 3, 260), rng.integers(0, 3, 220)]
    else:
        X, blob = gu.blobs(17, (120, 90, 60, 30), 5, 60.0)
        perm = rng.permutation(len(X))
        X, blob = X[perm].astype(np.float32), blob[perm]
        emb, lab = [X[:170], X[170:]], [blob[:170] // 2, blob[170:] // 2]        # a label = two far blobs
    for nn, expected in ((5, 'label'), (8, 'global')):
        a = JAMIE(metrics='device').test_graph(emb, lab, n_neighbors=nn, expected=expected, return_graph=True)
        b = JAMIE(metrics='host').test_graph(emb, lab, n_neighbors=nn, expected=expected, return_graph=True)
        print(f"{data} nn {nn} {expected}: components {a['n_components']} / {b['n_components']}, connectivity "
              f"{a['graph_connectivity']} / {b['graph_connectivity']}, kBET {a['kbet_rejection']} / {b['kbet_rejection']}")
        same_dicts(a, b)
    if data == 'blobs':
        assert a['n_components'] == 4 and a['component_sizes'].tolist() == [120, 90, 60, 30]
        assert a['label_components'].tolist() == [2, 2] and a['label_connectivity'].tolist() == [120 / 210, 60 / 90]


def test_leiden_communities_are_single_components_on_the_device(jgr):
    """Every community `leiden` returns is one component of the device's `components` on the entries inside it (DESIGN.md §24's
    promise, checked there with scipy on the host)."""
    from jamie_amd import leiden as jld
    from jamie_amd import spectral as jsp
    X, _ = gu.blobs(31, (400, 300, 300, 200), 8, 4.0)
    G = jsp.build_graph(torch.from_numpy(X.astype(np.float32)).cuda(), 15)
    for gamma in (1.0, 2.0):
        out = jld.communities(G, resolution=gamma)
        clusters = np.asarray(out['clusters'])
        glabel, rounds, _ = jgr.components(G, group=clusters)
        glabel = glabel.cpu().numpy()
        parts = [len(np.unique(glabel[clusters == c])) for c in range(len(out['sizes']))]
        whole = len(np.unique(jgr.components(G)[0].cpu().numpy()))
        print(f"gamma {gamma}: {len(parts)} communities (stop {out['stop']}), components inside each {sorted(set(parts))}, rounds "
              f"{rounds}; the graph itself has {whole}")
        assert out['stop'] != 'max_levels' and parts == [1] * len(parts)
        assert np.array_equal(glabel, gu.scipy_components(G.rowptr.cpu().numpy(), G.col.cpu().numpy(), G.n, clusters))

"""Louvain communities, the parts that need no GPU: the host route `_host_louvain_graph` against the per-node restatement of
louvain_util.py element for element, its modularity against networkx on the float64 graph within a bound derived from the
quantisation, its quality against networkx's Louvain, the levels, the two components of `apart`, the well-separated blobs, the
facade's ARI / NMI against sklearn, the argument checks on both routes and the exports.  Every figure is printed before it is
asserted."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import louvain_util as vu  # noqa: E402
import lisi_util as lu  # noqa: E402
import spectral_util as su  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('jamie_louvain_quantise', 'jamie_louvain_workspace', 'jamie_louvain_move', 'jamie_louvain_apply', 'jamie_louvain_internal')
GRAPHS = ('blobs4', 'blobs20', 'sheet', 'apart', 'cells40')
GAMMAS = (1.0, 0.5)
QUALITY_MARGIN = 0.03


@functools.lru_cache(maxsize=None)
def host_run(name, gamma):
    from jamie_amd import jamie as jj
    return jj._host_louvain_graph(*su.host_graph(name), resolution=gamma)


@functools.lru_cache(maxsize=None)
def nx_graph(name):
    import networkx as nx
    rowptr, col, val = su.host_graph(name)
    n = len(rowptr) - 1
    row = np.repeat(np.arange(n), np.diff(rowptr))
    G = nx.Graph()
    G.add_nodes_from(range(n))
    G.add_weighted_edges_from((int(i), int(j), float(v)) for i, j, v in zip(row, col, val) if i < j)
    return G


def members(clusters):
    return [set(np.nonzero(clusters == c)[0].tolist()) for c in np.unique(clusters)]


def test_symbols_are_declared_and_exported():
    from jamie_amd import _native as nv
    from jamie_amd import louvain as jlv
    hdr = open(os.path.join(ROOT, 'include', 'jamie_hip.h')).read()
    assert 'Louvain communities on the device' in hdr
    for s in SYMBOLS:
        assert s in nv.EXPORTS and f'{s}(' in hdr, s
    lib = nv.load()
    for s in SYMBOLS:
        assert hasattr(lib, s)
    # the workspace: 12 bytes per slot, the power of two from 2 len + 2 up; the Python mirror agrees
    assert nv.louvain_workspace([2049]) == 12 * 8192 and nv.louvain_workspace([3, 5000]) == 12 * (8 + 16384)
    assert nv.louvain_workspace([-1]) == 0 and nv.louvain_workspace([]) == 0
    assert [jlv.table_slots(v) for v in (0, 1, 3, 2047, 2049, 5000)] == [2, 4, 8, 4096, 8192, 16384]
    csrc = os.path.join(ROOT, 'jamie_amd', 'csrc')
    src = open(os.path.join(csrc, 'community_rows.h')).read()
    assert f'CR_SHORT_MAX = {jlv.SHORT_MAX};' in src and f'CR_LONG_MAX = {jlv.LONG_MAX};' in src
    assert (jlv.SHORT_MAX, jlv.LONG_MAX) == (vu.SHORT_MAX, vu.LONG_MAX)
    own = open(os.path.join(csrc, 'louvain.hip')).read()                     # the one pair of bin constants is the header's
    assert 'community_rows.h' in own and 'SHORT_MAX =' not in own and 'LONG_MAX =' not in own
    # the refusals come before any launch: no device is needed to see them
    p = [8] * 3
    assert lib.jamie_louvain_move(*p, 0, 4, 8, 8, 8, 8, 1.0, 1 << 52, 8, 4, 0, 0, None, 0, None, 0, 16, 8, None) != 0
    assert b'two_m' in lib.jamie_last_error()
    assert lib.jamie_louvain_move(*p, 0, 4, 8, 8, 8, 8, 1.0, 10, 8, 4, 0, 0, None, 0, None, 0, 8, 8, None) != 0
    assert b'differ' in lib.jamie_last_error()
    assert lib.jamie_louvain_move(*p, 0, 4, 8, 8, 8, 8, float('nan'), 10, 8, 4, 0, 0, None, 0, None, 0, 16, 8, None) != 0
    assert lib.jamie_louvain_move(*p, 0, 4, 8, 8, 8, 8, 1.0, 10, 8, 2, 2, 1, None, 0, None, 0, 16, 8, None) != 0
    assert lib.jamie_louvain_move(*p, 0, 4, 8, 8, 8, 8, 1.0, 10, 8, 2, 1, 1, 8, 10, 16, 100, 16, 8, None) != 0 and b'workspace' in lib.jamie_last_error()
    assert lib.jamie_louvain_apply(8, 0, 8, 8, 16, 8, 8, 8, 4, None) != 0
    assert lib.jamie_louvain_internal(None, 8, 8, 0, 4, 8, 8, 8, None) != 0 and b'null' in lib.jamie_last_error()
    assert lib.jamie_louvain_quantise(8, 8, 0, 0, 8, 8, None) != 0


def test_louvain_kernels_use_no_scratch():
    """private_segment_fixed_size == 0 and no spills for the kernels of csrc/louvain.hip, read from the code object hipcc built;
    the LDS tables are the sizes DESIGN.md §23 states: 12 bytes x 128 slots x 4 waves, and 12 bytes x 4096 slots (and the
    reduction's few words) within a 64 KiB workgroup."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import isa_check as ic
    obj = os.path.join(ROOT, 'jamie_amd', 'csrc', '_obj', 'louvain.o')
    if not os.path.exists(obj):
        pytest.skip('the library is not built')
    if not os.path.exists(ic.OBJDUMP):
        pytest.skip('llvm-objdump not found')
    meta = ic.kernel_metadata(obj)
    names = ' '.join(meta)
    for kernel in ('lv_quantise_kernel', 'lv_move_short_kernel', 'lv_move_long_kernel', 'lv_move_global_kernel', 'lv_apply_kernel',
                   'lv_internal_kernel'):
        assert kernel in names, (kernel, names)
    assert len(meta) == 6
    for name, m in meta.items():
        print(name, {k: m.get(k) for k in ('vgpr_count', 'sgpr_count', 'group_segment_fixed_size', 'private_segment_fixed_size')})
        assert m['private_segment_fixed_size'] == 0, (name, m)
        assert m.get('vgpr_spill_count', 0) == 0 and m.get('sgpr_spill_count', 0) == 0, (name, m)
        lds = m.get('group_segment_fixed_size', 0)
        if 'lv_move_short_kernel' in name:
            assert lds == 12 * 128 * 4, (name, m)
        elif 'lv_move_long_kernel' in name:
            assert 12 * 4096 <= lds <= 12 * 4096 + 256, (name, m)
        else:
            assert lds <= 256, (name, m)


@pytest.mark.parametrize('route', ['host', 'device'])
def test_value_errors_on_both_routes(route):
    """Every refusal comes from the shared argument checks, names louvain, and comes before either route touches a device."""
    from jamie_amd import JAMIE
    from jamie_amd import louvain as jlv
    j = JAMIE(metrics=route)
    emb, _ = lu.mixture(1, 3, 4, (60, 50))
    bad_nan = [emb[0].copy(), emb[1]]
    bad_nan[0][3, 2] = np.nan
    cases = [dict(resolution=0.0), dict(resolution=-1.0), dict(resolution=float('inf')), dict(resolution=float('nan')),
             dict(n_neighbors=1), dict(n_neighbors=111), dict(n_neighbors=130), dict(max_levels=0), dict(max_sweeps=0), dict(tol=-1e-3),
             dict(tol=float('nan'))]

    def refused(call):
        with pytest.raises(ValueError, match='louvain'):
            call()
    for kw in cases:
        refused(lambda: j.louvain(emb, **kw))
        refused(lambda: jlv.check_louvain(emb, **kw))
    for bad in (bad_nan, [emb[0], emb[1][:, :3]], []):
        refused(lambda: j.louvain(bad))
    refused(lambda: j.louvain(emb, datatype=[np.zeros(60), np.zeros(49)]))      # one label per cell
    refused(lambda: jlv.check_totals(5, 1 << 52))
    refused(lambda: jlv.check_totals(1 << 31, 10))
    refused(lambda: jlv.check_totals(5, 0))
    assert jlv.check_louvain(emb) == (1.0, 15, 20, 32, 1e-7)


def test_shared_definitions():
    from jamie_amd import louvain as jlv
    val = np.array([0.0, 1e-9, 2.0 ** -21, 1.5 * 2.0 ** -20, 2.5 * 2.0 ** -20, 3.5 * 2.0 ** -20, 1.0, 0.123456], np.float32)
    want = [1, 1, 1, 2, 2, 4, 1 << 20, round(float(np.float32(0.123456)) * 2 ** 20)]          # halves go to the even integer
    assert jlv.quantise(val).tolist() == want and vu.restated_quantise(val).tolist() == want and jlv.quantise(val).dtype == np.int64
    ids = np.array([0, 1, 2, 3, 1000, 123456789, 2 ** 31 - 1])
    assert jlv.node_class(ids).tolist() == [vu.node_class(i) for i in ids]
    assert set(jlv.node_class(np.arange(4096)).tolist()) == set(range(8))
    for h, want in (([5], False), ([5, 4, 4, 4], False), ([5, 4, 4, 4, 4], True), ([9, 3, 5, 4, 6], True), ([9, 8, 7, 6, 5], False),
                    ([2, 2, 2, 2], True)):
        assert jlv.stalled(h) is want and vu.restated_stalled(h) is want, h
    inside, tot = np.array([10, 0, 6], np.int64), np.array([14, 0, 10], np.int64)
    q = jlv.modularity_from_tables(inside, tot, 24, 0.5)
    assert q == vu.restated_modularity(inside, tot, 24, 0.5) and abs(q - (16 / 24 - 0.5 * (196 + 100) / 576)) < 1e-15
    comm = np.array([7, 3, 3, 7, 9, 9, 1])
    clusters, sizes = jlv.relabel(comm)
    assert clusters.tolist() == [0, 1, 1, 0, 2, 2, 3] and sizes.tolist() == [2, 2, 2, 1] and clusters.dtype == np.int32
    assert np.array_equal(vu.restated_relabel(comm)[0], clusters)


@pytest.mark.parametrize('gamma', GAMMAS)
@pytest.mark.parametrize('name', GRAPHS)
def test_host_route_equals_the_restatement(name, gamma):
    got = host_run(name, gamma)
    want = vu.restated_fuzzy(*su.host_graph(name), gamma)
    print(f"{name} gamma = {gamma}: {len(got['sizes'])} clusters, modularity {got['modularity']!r} (restated {want['modularity']!r}), "
          f"levels {[(lv['nodes'], lv['communities'], lv['moved']) for lv in got['levels']]}")
    assert np.array_equal(got['clusters'], want['clusters']) and np.array_equal(got['sizes'], want['sizes'])
    assert got['modularity'] == want['modularity'] and got['levels'] == want['levels']
    assert got['clusters'].dtype == np.int32 and len(got['levels']) >= 1


@pytest.mark.parametrize('gamma', GAMMAS)
@pytest.mark.parametrize('name', GRAPHS)
def test_modularity_against_networkx(name, gamma):
    """Q on the integer graph against networkx's Q of the same partition on the float64 graph.  With eps_e the error of entry e
    in units of val (2^-21 from the rounding, 2^-20 where the floor of 1 applies), E = sum eps_e and W = sum val: the inside
    fraction I / W moves by at most 2 E / W (its numerator and its denominator by E each, I <= W), and sum_c (tot_c / W)^2 by at
    most 2 * 2 E / W (each tot_c / W <= 1 moves by (dtot_c + tot_c E / W) / W, weighted by itself and summed), so |dQ| <= (2 + 4
    gamma) E / W to first order; 1 % and 1e-12 cover the second order and the float64 sums of both sides."""
    import networkx as nx
    rowptr, col, val = su.host_graph(name)
    out = host_run(name, gamma)
    ref = nx.community.modularity(nx_graph(name), members(out['clusters']), weight='weight', resolution=gamma)
    v = val.astype(np.float64)
    eps = np.where(v * 2.0 ** 20 < 0.5, 2.0 ** -20, 2.0 ** -21)
    bound = (2.0 + 4.0 * gamma) * eps.sum() / v.sum() * 1.01 + 1e-12
    diff = abs(out['modularity'] - ref)
    print(f'{name} gamma = {gamma}: modularity {out["modularity"]:.9f}, networkx {ref:.9f}, difference {diff:.3e}, bound {bound:.3e}')
    assert diff <= bound


@pytest.mark.parametrize('gamma', GAMMAS)
@pytest.mark.parametrize('name', GRAPHS)
def test_quality_against_networkx_louvain(name, gamma):
    import networkx as nx
    G = nx_graph(name)
    ours = host_run(name, gamma)['modularity']
    theirs = []
    for seed in range(5):
        part = nx.community.louvain_communities(G, weight='weight', resolution=gamma, seed=seed)
        theirs.append(nx.community.modularity(G, part, weight='weight', resolution=gamma))
    print(f'{name} gamma = {gamma}: modularity {ours:.6f}; networkx seeds 0 .. 4: {[round(t, 6) for t in theirs]}; deficit to the '
          f'best {max(theirs) - ours:.6f} (margin {QUALITY_MARGIN})')
    assert ours >= max(theirs) - QUALITY_MARGIN


@pytest.mark.parametrize('name', GRAPHS)
def test_levels_increase_and_two_m_is_conserved(name):
    from jamie_amd import louvain as jlv
    rowptr, col, val = su.host_graph(name)
    two_m = int(jlv.quantise(val).sum())
    for gamma in GAMMAS:
        levels = host_run(name, gamma)['levels']
        qs = [lv['modularity'] for lv in levels]
        print(f'{name} gamma = {gamma}: two_m {two_m}, modularity per level {qs}')
        assert all(b > a for a, b in zip(qs, qs[1:])) and qs[-1] == host_run(name, gamma)['modularity']
        assert all(lv['two_m'] == two_m for lv in levels)
        assert all(a['communities'] == b['nodes'] for a, b in zip(levels, levels[1:])) and levels[0]['nodes'] == len(rowptr) - 1
        assert all(lv['sweeps'] == len(lv['moved']) <= 32 and lv['communities'] < lv['nodes'] for lv in levels)


def test_apart_keeps_its_components():
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    rowptr, col, val = su.host_graph('apart')
    n = len(rowptr) - 1
    ncomp, comp = connected_components(csr_matrix((val, col, rowptr), shape=(n, n)), directed=False)
    assert ncomp == 2
    for gamma in GAMMAS:
        clusters = host_run('apart', gamma)['clusters']
        mixed = [c for c in np.unique(clusters) if len(np.unique(comp[clusters == c])) > 1]
        print(f'apart gamma = {gamma}: {len(np.unique(clusters))} clusters, {len(mixed)} of them across the components')
        assert not mixed
    half = host_run('apart', 0.5)['clusters']
    assert len(np.unique(half)) == 2 and len(set(zip(half.tolist(), comp.tolist()))) == 2


@functools.lru_cache(maxsize=None)
def blob_run(case, gamma):
    from jamie_amd import JAMIE
    X, labels = vu.separated_blobs(*case)
    half = len(X) // 2
    return JAMIE(metrics='host').louvain([X[:half], X[half:]], [labels[:half], labels[half:]], resolution=gamma, n_neighbors=15), labels


@pytest.mark.parametrize('gamma', [1.0, 0.5])
@pytest.mark.parametrize('case', vu.WELL_SEPARATED)
def test_well_separated_blobs_are_recovered(case, gamma):
    out, labels = blob_run(case, gamma)
    print(f"{case} gamma = {gamma}: {out['n_clusters']} clusters, sizes {out['sizes'].tolist()}, ARI {out['ari']}, NMI {out['nmi']}")
    assert out['n_clusters'] == case[0] and out['ari'] == 1.0
    assert [len(c) for c in out['clusters']] == [len(labels) // 2, len(labels) - len(labels) // 2]


def test_facade_figures_against_sklearn():
    from sklearn.metrics import adjusted_rand_score, normalized_mutual_info_score
    from jamie_amd import JAMIE
    emb, nn, _ = su.cells('blobs20')
    rng = np.random.default_rng(0)
    labels = [rng.integers(0, 7, len(e)) for e in emb]
    half = len(emb[0])
    truth = host_run('blobs20', 1.0)['clusters']
    labels[0][:700] = truth[:700] % 7                         # (partly informative labels: an ARI strictly between 0 and 1)
    out = JAMIE(metrics='host').louvain(list(emb), labels, n_neighbors=nn, return_graph=True)
    pooled, lab = np.concatenate(out['clusters']), np.concatenate(labels)
    ari, nmi = adjusted_rand_score(lab, pooled), normalized_mutual_info_score(lab, pooled)
    print(f"blobs20: ARI {out['ari']!r} (sklearn {ari!r}), NMI {out['nmi']!r} (sklearn {nmi!r}), {out['n_clusters']} clusters")
    assert abs(out['ari'] - ari) <= 1e-12 and abs(out['nmi'] - nmi) <= 1e-12 and 0.0 < ari < 1.0
    assert np.array_equal(pooled, truth) and out['modularity'] == host_run('blobs20', 1.0)['modularity']
    assert out['clusters'][0].dtype == np.int32 and len(out['clusters'][0]) == half
    assert out['sizes'].tolist() == np.bincount(pooled).tolist() and np.all(np.diff(out['sizes']) <= 0)
    assert out['n_clusters'] == len(out['sizes']) and out['n_neighbors'] == nn
    assert out['modality_contingency'].shape == (out['n_clusters'], 2)
    assert np.array_equal(out['modality_contingency'].sum(axis=1), out['sizes'])
    assert out['contingency'].shape == (out['n_clusters'], 7) and out['contingency'].sum() == len(pooled)
    assert out['labels'].tolist() == list(range(7))
    assert out['graph'].shape == (len(pooled), len(pooled)) and out['graph'].nnz == out['n_edges']
    plain = JAMIE(metrics='host').louvain(list(emb), n_neighbors=nn)
    assert plain['ari'] is None and plain['nmi'] is None and plain['contingency'] is None and plain['graph'] is None
    assert np.array_equal(np.concatenate(plain['clusters']), pooled)

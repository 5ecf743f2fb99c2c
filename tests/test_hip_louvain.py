"""Louvain communities on the device (jamie_amd/louvain.py, csrc/louvain.hip) against the per-node restatement of louvain_util.py
run on the device's own graph, downloaded: every sum is an integer sum, so everything is compared for equality -- the weights,
every target of every class, the state after every application, the coarse graph, the clusters, the history of every level and
the modularity to the bit.  Then the two routes of the facade on well-separated blobs, the quality against a sequential Louvain
and the memory.  Every figure is printed before it is asserted."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import louvain_util as vu  # noqa: E402
import spectral_util as su  # noqa: E402
import umap_util as uu  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPE_CASES = (8, 130, 257, 600, 1000, 'hub', 'special')
SYNTHETIC = ('star64', 'star65', 'star2048', 'star2049', 'star5000', 'heavy', 'ring', 'pairs', 'empty')
# (short, long, global) rows of the synthetic graphs: the hub's row is the only one past 64 entries
BINS = {'star64': (65, 0, 0), 'star65': (65, 1, 0), 'star2048': (2048, 1, 0), 'star2049': (2049, 0, 1), 'star5000': (5000, 0, 1)}
RUN_CASES = ('blobs4', 'blobs20', 'sheet', 'apart', 'hub', 'special')
QUALITY_CASES = ('blobs3', 'blobs20', 'apart')
QUALITY_MARGIN = 0.02


@pytest.fixture(scope='module')
def jlv():
    from jamie_amd import louvain
    return louvain


_graphs, _levels, _runs = {}, {}, {}


def device_graph(name):
    """The fuzzy graph of a case on the device, once, as `louvain.louvain` builds it; its arrays on the host."""
    if name not in _graphs:
        from jamie_amd import spectral as jsp
        if name in su.BLOBS or name in ('sheet', 'apart'):
            emb, nn, _ = su.cells(name)
            X = np.concatenate(emb, axis=0)
        else:
            c = uu.shape_case(name)
            X, nn = c['X'], c['nn']
        G = jsp.build_graph(torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).cuda(), nn)
        _graphs[name] = dict(G=G, rowptr=G.rowptr.cpu().numpy(), col=G.col.cpu().numpy(), val=G.val.cpu().numpy())
    return _graphs[name]


def level_pair(jlv, name):
    """(the level graph on the device, the same graph for the restatement) of a shape case or a synthetic graph."""
    if name not in _levels:
        if name in SYNTHETIC:
            g = vu.synthetic(name)
            G = jlv.LevelGraph.from_numpy(g['rowptr'], g['col'], g['w'], g['loop'])
        else:
            d = device_graph(name)
            G = jlv.level_graph(d['G'])
            g = vu.graph_of(d['rowptr'], d['col'], G.w.cpu().numpy())
        _levels[name] = (G, g)
    return _levels[name]


def restated_run(name, gamma=1.0):
    if (name, gamma) not in _runs:
        d = device_graph(name)
        _runs[(name, gamma)] = vu.restated_fuzzy(d['rowptr'], d['col'], d['val'], gamma)
    return _runs[(name, gamma)]


def classes_of(n):
    return [[i for i in range(n) if vu.node_class(i) == s] for s in range(8)]


@pytest.mark.parametrize('name', SHAPE_CASES)
def test_quantise_equals_the_restatement(jlv, name):
    d = device_graph(name)
    G = jlv.level_graph(d['G'])
    w = vu.restated_quantise(d['val'])
    g = vu.graph_of(d['rowptr'], d['col'], w)
    print(f"{name}: {G.n} nodes, {len(w)} entries, weights {w.min()} .. {w.max()}, two_m {G.two_m} (restated {g['two_m']})")
    assert G.w.dtype == torch.int64 and np.array_equal(G.w.cpu().numpy(), w)
    assert np.array_equal(G.k.cpu().numpy(), g['k']) and G.two_m == g['two_m'] and int(G.loop.abs().sum()) == 0
    assert np.array_equal(w, jlv.quantise(d['val']))
    wt = w.reshape(-1)
    row = np.repeat(np.arange(G.n), np.diff(d['rowptr']))
    sym = {(int(i), int(j)): int(v) for i, j, v in zip(row, d['col'], wt)}
    assert all(sym[(j, i)] == v for (i, j), v in sym.items())               # the stored graph is symmetric to the bit


@pytest.mark.parametrize('name', SHAPE_CASES + SYNTHETIC)
def test_move_equals_the_restatement_in_every_target(jlv, name):
    G, g = level_pair(jlv, name)
    lists = classes_of(g['n'])
    mid = vu.singleton_state(g)
    vu.restated_sweep(g, *mid, 1.0)
    taken = np.zeros(3, np.int64)
    for tag, host_state, gamma in (('singletons', vu.singleton_state(g), 1.0), ('after one sweep', mid, 0.7)):
        state = jlv.state_of(G, host_state[0])
        assert np.array_equal(state.tot.cpu().numpy(), host_state[1]) and np.array_equal(state.size.cpu().numpy(), host_state[2])
        wrong = leaving = 0
        for s in range(8):
            state.target.fill_(-7)
            counts = jlv.move(G, state, s, gamma)
            want = vu.restated_move(g, *host_state, lists[s], gamma)
            got = state.target.cpu().numpy()
            assert sum(counts) == len(lists[s])
            taken += counts if tag == 'singletons' else 0
            wrong += sum(int(got[i]) != d for i, d in want.items())
            leaving += sum(int(host_state[0][i]) != d for d, i in zip(want.values(), want))
            others = np.ones(g['n'], bool)
            others[lists[s]] = False
            assert np.all(got[others] == -7)                                  # the other classes' entries are left alone
        print(f'{name}, {tag}, gamma = {gamma}: {g["n"]} nodes, longest row {int(np.diff(g["rowptr"]).max())}, {leaving} nodes '
              f'want to move, {wrong} targets differ from the restatement')
        assert wrong == 0 and int(state.flag.item()) == 0
        assert np.array_equal(state.comm.cpu().numpy(), host_state[0])       # comm is not written
    lens = np.diff(g['rowptr'])
    want_bins = ((lens <= vu.SHORT_MAX).sum(), ((lens > vu.SHORT_MAX) & (lens <= vu.LONG_MAX)).sum(), (lens > vu.LONG_MAX).sum())
    print(f'   rows taken per bin (short, long, global): {taken.tolist()}')
    assert tuple(taken) == tuple(int(v) for v in want_bins)
    if name in BINS:
        assert tuple(taken) == BINS[name]
    if name == 1000:
        assert taken[1] == 1000                                               # K = 128: every row is a workgroup's
    if name == 'pairs':                                                       # the singleton rule: the higher node joins the lower
        state = jlv.singletons(G)
        for s in range(8):
            jlv.move(G, state, s)
        assert state.target.cpu().numpy().tolist() == [0, 0, 2, 2]


# (graph, what is wrong, the (short, long, global) counts the hub is listed under, the flag bit)
REFUSALS = (('star65', 'bin', (1, 0, 0), 1), ('star65', 'comm', (0, 1, 0), 2), ('star2049', 'table', (0, 0, 1), 4))


@pytest.mark.parametrize('name, what, counts, bit', REFUSALS)
def test_move_refuses_a_row_it_cannot_take(jlv, name, what, counts, bit):
    """The hub alone in a hand-made node list: listed in the short bin, with its community out of range, and with a table of
    too few slots.  The flag names the reason, the hub stays where it is and nothing else is written: the row is never walked."""
    from jamie_amd import _native as nv
    G, g = level_pair(jlv, name)
    n, hub, dev = g['n'], 0, G.col.device
    state = jlv.singletons(G)
    if what == 'comm':
        state.comm[hub] = n
    state.target.fill_(-7)
    nodes = torch.tensor([hub], dtype=torch.int32, device=dev)
    slot_off = torch.tensor([0, 2048], dtype=torch.int64, device=dev) if what == 'table' else None       # the row needs 8192
    ws = torch.full((12 * 2048,), 0x55, dtype=torch.uint8, device=dev)
    before = [t.clone() for t in (state.comm, state.tot, state.size)]
    nv.louvain_move(G.rowptr, G.col, G.w, G.k, state.comm, state.tot, state.size, 1.0, G.two_m, nodes, counts, slot_off, ws,
                    state.target, state.flag)
    got, flag = state.target.cpu().numpy(), int(state.flag.item())
    print(f'{name}, {what}: a row of {int(G.lens[hub])} entries listed as {counts}: flag {flag}, target of the hub {got[hub]}, '
          f'{int((got[1:] != -7).sum())} other targets written')
    assert flag == bit
    assert got[hub] == int(before[0][hub]) and np.all(got[1:] == -7)
    assert all(torch.equal(a, b) for a, b in zip(before, (state.comm, state.tot, state.size)))
    if what == 'table':                                                       # the cleared table: no slot was claimed
        assert int(ws[:8 * 2048].view(torch.int64).abs().sum()) == 0 and bool((ws[8 * 2048:].view(torch.int32) == -1).all())
    else:
        assert bool((ws == 0x55).all())


@pytest.mark.parametrize('name', (130, 600, 'hub', 'star2049', 'heavy', 'ring', 'pairs', 'empty'))
def test_apply_and_sweep_keep_the_tables_exact(jlv, name):
    G, g = level_pair(jlv, name)
    lists = classes_of(g['n'])
    state = jlv.singletons(G)
    comm, tot, size = vu.singleton_state(g)
    k = g['k']
    for sweep in range(2):
        total = 0
        for s in range(8):
            jlv.move(G, state, s)
            before = int(state.moved.item())
            jlv.apply(G, state, s)
            moved = vu.restated_apply(g, comm, tot, size, vu.restated_move(g, comm, tot, size, lists[s], 1.0))
            total += moved
            got = state.comm.cpu().numpy()
            assert int(state.moved.item()) - before == moved and np.array_equal(got, comm)
            want_tot = np.zeros(g['n'], np.int64)
            np.add.at(want_tot, got, k)
            assert np.array_equal(state.tot.cpu().numpy(), want_tot) and np.array_equal(want_tot, tot)
            assert np.array_equal(state.size.cpu().numpy(), np.bincount(got, minlength=g['n']))
        print(f'{name}: sweep {sweep} moved {total} nodes, {len(np.unique(comm))} communities')
    again = jlv.singletons(G)
    first = jlv.sweep(G, again)
    check = vu.singleton_state(g)
    assert first == vu.restated_sweep(g, *check, 1.0) and np.array_equal(again.comm.cpu().numpy(), check[0])
    inside = jlv.internal_weights(G, state.comm).cpu().numpy()
    assert np.array_equal(inside, vu.restated_internal(g, comm))


@pytest.mark.parametrize('name', (130, 1000, 'hub', 'special', 'star2049', 'heavy', 'ring', 'empty'))
def test_aggregate_equals_the_restatement(jlv, name):
    G, g = level_pair(jlv, name)
    state, history = jlv.run_level(G, 1.0, 32)
    comm = state.comm.cpu().numpy().astype(np.int64)
    want_comm, _, _, want_history = vu.restated_level(g, 1.0)
    assert history == want_history and np.array_equal(comm, want_comm)
    nxt, cmap = jlv.aggregate(G, state.comm)
    want, want_map = vu.restated_aggregate(g, comm)
    print(f"{name}: {g['n']} nodes in {nxt.n} communities after {len(history)} sweeps {history}; {nxt.col.numel()} coarse entries, "
          f"longest coarse row {int(nxt.lens.max()) if nxt.n else 0}, two_m {nxt.two_m}")
    assert nxt.n == want['n'] and np.array_equal(cmap.cpu().numpy(), want_map)
    assert np.array_equal(nxt.rowptr.cpu().numpy(), want['rowptr']) and np.array_equal(nxt.col.cpu().numpy(), want['col'])
    assert np.array_equal(nxt.w.cpu().numpy(), want['w']) and np.array_equal(nxt.loop.cpu().numpy(), want['loop'])
    assert np.array_equal(nxt.k.cpu().numpy(), want['k']) and nxt.two_m == g['two_m'] == G.two_m
    assert nxt.col.dtype == torch.int32 and nxt.rowptr.dtype == torch.int64
    col, ptr = want['col'], want['rowptr']
    assert all(np.all(np.diff(col[ptr[r]:ptr[r + 1]]) > 0) for r in range(want['n']))      # ascending columns, no diagonal
    assert all(r not in col[ptr[r]:ptr[r + 1]] for r in range(want['n']))


@pytest.mark.parametrize('gamma', [1.0, 0.5])
@pytest.mark.parametrize('name', RUN_CASES)
def test_whole_run_equals_the_restatement(jlv, name, gamma):
    d = device_graph(name)
    got = jlv.communities(d['G'], resolution=gamma)
    want = restated_run(name, gamma)
    print(f"{name} gamma = {gamma}: {len(got['sizes'])} clusters, modularity {got['modularity']!r} (restated {want['modularity']!r}), "
          f"levels {[(lv['nodes'], lv['communities'], lv['moved']) for lv in got['levels']]}")
    assert np.array_equal(got['clusters'], want['clusters']) and np.array_equal(got['sizes'], want['sizes'])
    assert got['levels'] == want['levels'] and got['modularity'] == want['modularity']
    again = jlv.communities(d['G'], resolution=gamma)
    assert np.array_equal(again['clusters'], got['clusters']) and again['levels'] == got['levels']
    assert again['modularity'] == got['modularity']
    qs = [lv['modularity'] for lv in got['levels']]
    assert all(b > a for a, b in zip(qs, qs[1:])) and len({lv['two_m'] for lv in got['levels']}) == 1


@pytest.mark.parametrize('case', vu.WELL_SEPARATED)
def test_facade_routes_agree_on_well_separated_blobs(case):
    from jamie_amd import JAMIE
    from jamie_amd.clustering import ari_nmi
    X, labels = vu.separated_blobs(*case)
    half = len(X) // 2
    emb, lab = [X[:half], X[half:]], [labels[:half], labels[half:]]
    for gamma in (1.0, 0.5):
        dev = JAMIE(metrics='device').louvain(emb, lab, resolution=gamma, n_neighbors=15)
        host = JAMIE(metrics='host').louvain(emb, lab, resolution=gamma, n_neighbors=15)
        a, b = np.concatenate(dev['clusters']), np.concatenate(host['clusters'])
        table = np.zeros((dev['n_clusters'], host['n_clusters']), np.int64)
        np.add.at(table, (a, b), 1)
        between = ari_nmi(table)[0]
        print(f"{case} gamma = {gamma}: device {dev['n_clusters']} clusters ARI {dev['ari']}, host {host['n_clusters']} clusters ARI "
              f"{host['ari']}, between the routes {between}; modularity {dev['modularity']:.6f} / {host['modularity']:.6f}")
        assert dev['n_clusters'] == host['n_clusters'] == case[0] and dev['ari'] == 1.0 and host['ari'] == 1.0 and between == 1.0
        assert dev['clusters'][0].dtype == np.int32 and [len(c) for c in dev['clusters']] == [half, len(X) - half]
        assert np.array_equal(dev['contingency'].sum(axis=1), dev['sizes']) and dev['modality_contingency'].shape == (case[0], 2)
        assert dev['n_edges'] > 0 and dev['graph'] is None


@pytest.mark.parametrize('name', QUALITY_CASES)
def test_quality_against_sequential_louvain(jlv, name):
    d = device_graph(name)
    got = jlv.communities(d['G'])
    g = vu.graph_of(d['rowptr'], d['col'], vu.restated_quantise(d['val']))
    part, q_seq = vu.sequential_louvain(g)
    assert abs(vu.partition_modularity(g, got['clusters'], 1.0) - got['modularity']) <= 1e-12
    print(f"{name}: modularity {got['modularity']:.6f} in {len(got['sizes'])} clusters; sequential Louvain {q_seq:.6f} in "
          f"{len(np.unique(part))}; deficit {q_seq - got['modularity']:.6f} (margin {QUALITY_MARGIN})")
    assert got['modularity'] >= q_seq - QUALITY_MARGIN


def test_memory_at_20000_cells(jlv):
    """No N x N: the peak of a whole run above the resident fuzzy graph stays below 256 bytes per stored entry and per cell plus
    8 MiB.  The enumerated need is less -- the weights (8 bytes per entry), the sort of the aggregation with its keys, masks,
    permutation, inverse and gathered weights (some 150) and a few dozen bytes per node of state and node lists; the rest is
    room for the sort's own workspace and the allocator's rounding.  At this size the bound is below half of an N x N byte
    matrix, and the whole call (kNN lists and graph included) stays below one."""
    from jamie_amd import spectral as jsp
    N, L = 20000, 32
    rng = np.random.default_rng(4)
    centres = rng.standard_normal((10, L)) * 1.2
    x = torch.from_numpy((centres[rng.integers(0, 10, N)] + rng.standard_normal((N, L))).astype(np.float32)).cuda()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    G = jsp.build_graph(x, 15)
    built = torch.cuda.max_memory_allocated() - base
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    resident = torch.cuda.memory_allocated()
    out = jlv.communities(G)
    peak = torch.cuda.max_memory_allocated() - resident
    nnz = int(G.col.numel())
    bound = 256 * nnz + 256 * N + (8 << 20)
    print(f"N = {N}: the graph's {nnz} entries built within {built / 2 ** 20:.1f} MiB; the run's peak above it {peak / 2 ** 20:.1f} MiB "
          f"(bound {bound / 2 ** 20:.1f} MiB, N x N bytes {N * N / 2 ** 20:.0f} MiB), {len(out['sizes'])} clusters, modularity "
          f"{out['modularity']:.4f}, levels {[(lv['nodes'], lv['sweeps']) for lv in out['levels']]}")
    assert peak < bound < N * N // 2 and built < N * N

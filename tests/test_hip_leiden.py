"""Leiden communities on the device (jamie_amd/leiden.py, csrc/leiden.hip) against the per-node restatement of leiden_util.py run
on the device's own graph, downloaded: every sum is an integer sum, so everything is compared for equality -- the cut table, every
target of every class, the state after every application, the clusters, the record of every level, the stop and the modularity
to the bit.  Then the connectivity of every community, the two routes of the facade on well-separated blobs and the memory.
Every figure is printed before it is asserted."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import leiden_util as du  # noqa: E402
import louvain_util as vu  # noqa: E402
import spectral_util as su  # noqa: E402
import umap_util as uu  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPE_CASES = (8, 130, 257, 600, 1000, 'hub', 'special')
STARS = ('star64', 'star65', 'star2048', 'star2049', 'star5000')
SYNTHETIC = STARS + ('filtered', 'heavy', 'ring', 'empty', 'chain', 'pairs', 'stuck')
# (short, long, global) rows of the star graphs: the hub's row is the only one past 64 entries
BINS = {'star64': (65, 0, 0), 'star65': (65, 1, 0), 'star2048': (2048, 1, 0), 'star2049': (2049, 0, 1), 'star5000': (5000, 0, 1)}
RUN_CASES = ('blobs4', 'blobs20', 'sheet', 'apart', 'hub', 'special')


@pytest.fixture(scope='module')
def jld():
    from jamie_amd import leiden
    return leiden


_graphs, _levels, _runs = {}, {}, {}


def device_graph(name):
    """The fuzzy graph of a case on the device, once, as `leiden.leiden` builds it; its arrays on the host."""
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


def level_case(name):
    """(the level graph on the device, the same graph for the restatement, the communities the refinement runs inside) of a case,
    once.  The stars are one community (the hub's row holds only same-community entries), `filtered` a hub whose entries mostly
    lie in other communities, `chain` and `stuck` the hand-built cases of leiden_util; every other graph takes the communities of
    the restated move phase of its level 0."""
    if name not in _levels:
        from jamie_amd import louvain as jlv
        if name in SYNTHETIC:
            if name == 'filtered':
                g, comm = du.filtered_hub()
            elif name == 'chain':
                g, comm = du.cancel_chain()[:2]
            elif name == 'stuck':
                g, comm = du.stuck_pair()
            else:
                g = vu.synthetic(name)
                comm = np.zeros(g['n'], np.int64) if name in STARS else vu.restated_level(g, 1.0)[0]
            G = jlv.LevelGraph.from_numpy(g['rowptr'], g['col'], g['w'], g['loop'])
        else:
            d = device_graph(name)
            G = jlv.level_graph(d['G'])
            g = vu.graph_of(d['rowptr'], d['col'], G.w.cpu().numpy())
            comm = vu.restated_level(g, 1.0)[0]
        _levels[name] = (G, g, np.asarray(comm, np.int64))
    return _levels[name]


def two_starts(g, comm, tot):
    """(tag, gamma, ref, rtot, rsize) with every node alone, and after the first three sub-sweeps of the restatement."""
    later = du.fresh(g)
    lists = du.class_lists(g['n'])
    for s in range(3):
        du.restated_subsweep(g, comm, tot, *later, s, 1.0, lists)
    return (('alone', 1.0, *du.fresh(g)), ('after three sub-sweeps', 0.7, *later))


@pytest.mark.parametrize('name', SHAPE_CASES + SYNTHETIC)
def test_cut_and_refine_equal_the_restatement_in_every_target(jld, name):
    from jamie_amd import louvain as jlv
    G, g, comm = level_case(name)
    lists = du.class_lists(g['n'])
    _, tot, _ = vu.state_of(g, comm)
    state = jlv.state_of(G, comm)
    assert np.array_equal(state.tot.cpu().numpy(), tot)
    taken = np.zeros(3, np.int64)
    for tag, gamma, ref, rtot, rsize in two_starts(g, comm, tot):
        R = jld.refinement_of(G, ref)
        assert np.array_equal(R.rtot.cpu().numpy(), rtot) and np.array_equal(R.rsize.cpu().numpy(), rsize)
        R.cut.fill_(-3)                                                   # (the wrapper zeroes it)
        jld.cut_table(G, state.comm, R)
        cut = du.restated_cut(g, comm, ref)
        assert np.array_equal(R.cut.cpu().numpy(), cut)
        wrong = leaving = alone = 0
        for s in range(8):
            R.target.fill_(-7)
            counts = jld.refine(G, state, R, s, gamma)
            want = du.restated_targets(g, comm, tot, ref, rtot, rsize, cut, lists[s], gamma)
            got = R.target.cpu().numpy()
            assert sum(counts) == len(lists[s])
            taken += counts if tag == 'alone' else 0
            wrong += sum(int(got[i]) != d for i, d in want.items())
            leaving += sum(int(ref[i]) != d for i, d in want.items())
            alone += sum(int(rsize[ref[i]]) == 1 for i in lists[s])
            others = np.ones(g['n'], bool)
            others[lists[s]] = False
            assert np.all(got[others] == -7)                              # the other classes' entries are left alone
        print(f'{name}, {tag}, gamma = {gamma}: {g["n"]} nodes in {len(np.unique(comm))} communities, longest row '
              f'{int(np.diff(g["rowptr"]).max())}, {alone} nodes alone, {leaving} want to join, cut total {int(cut.sum())}, '
              f'{wrong} targets differ from the restatement')
        assert wrong == 0 and int(R.flag.item()) == 0
        assert np.array_equal(R.ref.cpu().numpy(), ref) and np.array_equal(state.comm.cpu().numpy(), comm)      # neither is written
    lens = np.diff(g['rowptr'])
    want_bins = ((lens <= vu.SHORT_MAX).sum(), ((lens > vu.SHORT_MAX) & (lens <= vu.LONG_MAX)).sum(), (lens > vu.LONG_MAX).sum())
    print(f'   rows taken per bin (short, long, global): {taken.tolist()}')
    assert tuple(taken) == tuple(int(v) for v in want_bins)
    if name in BINS:
        assert tuple(taken) == BINS[name]
        inside = sum(1 for e in range(g['rowptr'][0], g['rowptr'][1]) if comm[g['col'][e]] == comm[0])
        assert inside == int(name[4:])                                        # the hub's row: that many same-community entries
    if name == 1000:
        assert taken[1] == 1000                                               # K = 128: every row is a workgroup's
    if name == 'filtered':
        inside = sum(1 for e in range(g['rowptr'][0], g['rowptr'][1]) if comm[g['col'][e]] == comm[0])
        assert 0 < 5 * inside < lens[0] and taken[1] == 1                     # most of the hub's entries are filtered out


# (graph, what is wrong, the (short, long, global) counts the hub is listed under, the flag bit)
REFUSALS = (('star65', 'bin', (1, 0, 0), 1), ('star65', 'comm', (0, 1, 0), 2), ('star2049', 'table', (0, 0, 1), 4))


@pytest.mark.parametrize('name, what, counts, bit', REFUSALS)
def test_refine_refuses_a_row_it_cannot_take(jld, name, what, counts, bit):
    """The hub, alone in its part, alone in a hand-made node list: listed in the short bin, with its community out of range, and
    with a table of too few slots.  The flag names the reason, the hub stays alone and nothing else is written: the row is never
    walked."""
    from jamie_amd import _native as nv
    from jamie_amd import louvain as jlv
    G, g, comm = level_case(name)
    n, hub, dev = g['n'], 0, G.col.device
    state = jlv.state_of(G, comm)
    if what == 'comm':
        state.comm[hub] = n
    R = jld.start(G)
    R.target.fill_(-7)
    nodes = torch.tensor([hub], dtype=torch.int32, device=dev)
    slot_off = torch.tensor([0, 2048], dtype=torch.int64, device=dev) if what == 'table' else None       # the row needs 8192
    ws = torch.full((12 * 2048,), 0x55, dtype=torch.uint8, device=dev)
    held = (state.comm, state.tot, R.ref, R.rtot, R.rsize, R.cut)
    before = [t.clone() for t in held]
    nv.leiden_refine(G.rowptr, G.col, G.w, G.k, state.comm, state.tot, R.ref, R.rtot, R.rsize, R.cut, 1.0, G.two_m, nodes, counts,
                     slot_off, ws, R.target, R.flag)
    got, flag = R.target.cpu().numpy(), int(R.flag.item())
    print(f'{name}, {what}: a row of {int(G.lens[hub])} entries listed as {counts}: flag {flag}, target of the hub {got[hub]}, '
          f'{int((got[1:] != -7).sum())} other targets written')
    assert flag == bit
    assert got[hub] == hub and np.all(got[1:] == -7)
    assert all(torch.equal(a, b) for a, b in zip(before, held))
    if what == 'table':                                                       # the cleared table: no slot was claimed
        assert int(ws[:8 * 2048].view(torch.int64).abs().sum()) == 0 and bool((ws[8 * 2048:].view(torch.int32) == -1).all())
    else:
        assert bool((ws == 0x55).all())


@pytest.mark.parametrize('name', (130, 600, 'hub', 'star65', 'star2049', 'filtered', 'heavy', 'ring', 'empty', 'chain', 'stuck'))
def test_apply_keeps_the_tables_exact_after_every_subsweep(jld, name):
    from jamie_amd import louvain as jlv
    G, g, comm = level_case(name)
    lists = du.class_lists(g['n'])
    _, tot, _ = vu.state_of(g, comm)
    state = jlv.state_of(G, comm)
    R = jld.start(G)
    ref, rtot, rsize = du.fresh(g)
    merged = cancelled = 0
    for s in range(8):
        R.target.copy_(R.ref)
        jld.cut_table(G, state.comm, R)
        jld.refine(G, state, R, s, 1.0)
        jld.apply(G, R, s)
        cut, targets, m, c = du.restated_subsweep(g, comm, tot, ref, rtot, rsize, s, 1.0, lists)
        merged, cancelled = merged + m, cancelled + c
        got = R.ref.cpu().numpy()
        assert np.array_equal(got, ref) and np.array_equal(R.cut.cpu().numpy(), cut)
        assert R.counts.tolist() == [merged, cancelled]
        want_tot = np.zeros(g['n'], np.int64)
        np.add.at(want_tot, got, g['k'])
        assert np.array_equal(R.rtot.cpu().numpy(), want_tot) and np.array_equal(want_tot, rtot)
        assert np.array_equal(R.rsize.cpu().numpy(), np.bincount(got, minlength=g['n'])) and np.array_equal(rsize, R.rsize.cpu().numpy())
        assert np.all(got[got] == got)                                        # a part is named after a member that stays
    print(f'{name}: {merged} nodes merged into {len(np.unique(ref))} parts of {len(np.unique(comm))} communities, {cancelled} cancelled')
    again = jld.start(G)
    assert jld.refine_level(G, state, again, 1.0) == (merged, cancelled) and np.array_equal(again.ref.cpu().numpy(), ref)
    assert int(R.flag.item()) == 0
    if name == 'chain':
        _, _, i, u, t = du.cancel_chain()
        assert (merged, cancelled) == (1, 1) and ref[u] == t and ref[i] == i
    if name == 'stuck':
        assert (merged, cancelled) == (0, 0)


def restated_run(name, gamma):
    if (name, gamma) not in _runs:
        d = device_graph(name)
        trace = []
        _runs[(name, gamma)] = (du.restated_fuzzy(d['rowptr'], d['col'], d['val'], gamma, trace=trace), trace)
    return _runs[(name, gamma)]


@pytest.mark.parametrize('gamma', [1.0, 0.5])
@pytest.mark.parametrize('name', RUN_CASES)
def test_whole_run_equals_the_restatement_and_is_connected(jld, name, gamma):
    d = device_graph(name)
    trace = []
    got = jld.communities(d['G'], resolution=gamma, trace=trace)
    want, want_trace = restated_run(name, gamma)
    print(f"{name} gamma = {gamma}: {len(got['sizes'])} clusters, stop {got['stop']}, modularity {got['modularity']!r} (restated "
          f"{want['modularity']!r}), levels {[(lv['nodes'], lv['communities'], lv['refined'], lv['merged'], lv['cancelled']) for lv in got['levels']]}")
    assert du.same_trace(trace, want_trace)
    assert np.array_equal(got['clusters'], want['clusters']) and np.array_equal(got['sizes'], want['sizes'])
    assert got['levels'] == want['levels'] and got['modularity'] == want['modularity'] and got['stop'] == want['stop']
    again = jld.communities(d['G'], resolution=gamma)
    assert np.array_equal(again['clusters'], got['clusters']) and again['levels'] == got['levels']
    assert again['modularity'] == got['modularity'] and again['stop'] == got['stop']
    assert len({lv['two_m'] for lv in got['levels']}) == 1
    parts, comms = du.components_within(d['rowptr'], d['col'], got['clusters'])
    print(f'   {comms} communities in {parts} connected parts')
    assert got['stop'] in ('singletons', 'stuck') and parts == comms == len(got['sizes'])


def test_max_levels_and_the_level_graph_runs(jld):
    from jamie_amd import louvain as jlv
    d = device_graph('blobs4')
    one = jld.communities(d['G'], max_levels=1)
    louvain = jlv.communities(d['G'], max_levels=1)
    assert one['stop'] == 'max_levels' and len(one['levels']) == 1 and one['levels'][0]['refined'] is None
    assert np.array_equal(one['clusters'], louvain['clusters']) and one['modularity'] == louvain['modularity']
    for name, stop in (('chain', 'singletons'), ('ring', None), ('heavy', None), ('empty', None)):
        G, g, _ = level_case(name)
        got = jld.communities_of_level_graph(G)
        want = du.restated_run(g)
        clusters, sizes = jlv.relabel(got['comm'])
        print(f"{name}: stop {got['stop']}, {len(sizes)} clusters, modularity {got['modularity']!r}, {len(got['levels'])} levels")
        assert np.array_equal(clusters, want['clusters']) and got['levels'] == want['levels'] and got['stop'] == want['stop']
        assert got['modularity'] == want['modularity'] and (stop is None or got['stop'] == stop)
    rowptr, col, val = du.stuck_graph()                       # the pinned fuzzy graph that ends stuck, as a level graph
    G = jlv.LevelGraph.from_numpy(rowptr, col, jlv.quantise(val), np.zeros(len(rowptr) - 1, np.int64))
    got, want = jld.communities_of_level_graph(G), du.restated_fuzzy(rowptr, col, val)
    clusters, sizes = jlv.relabel(got['comm'])
    parts, comms = du.components_within(rowptr, col, clusters)
    last = got['levels'][-1]
    print(f"pinned stuck graph: stop {got['stop']}, {len(sizes)} parts of {last['communities']} communities, modularity "
          f"{got['modularity']!r} against {last['modularity']!r}")
    assert got['stop'] == 'stuck' and np.array_equal(clusters, want['clusters']) and got['levels'] == want['levels']
    assert got['modularity'] == want['modularity'] >= last['modularity'] and parts == comms == last['nodes'] > last['communities']


@pytest.mark.parametrize('case', vu.WELL_SEPARATED)
def test_facade_routes_agree_on_well_separated_blobs(jld, case):
    from jamie_amd import JAMIE
    from jamie_amd.clustering import ari_nmi
    X, labels = vu.separated_blobs(*case)
    half = len(X) // 2
    emb, lab = [X[:half], X[half:]], [labels[:half], labels[half:]]
    for gamma in (1.0, 0.5):
        dev = JAMIE(metrics='device').leiden(emb, lab, resolution=gamma, n_neighbors=15)
        host = JAMIE(metrics='host').leiden(emb, lab, resolution=gamma, n_neighbors=15)
        a, b = np.concatenate(dev['clusters']), np.concatenate(host['clusters'])
        table = np.zeros((dev['n_clusters'], host['n_clusters']), np.int64)
        np.add.at(table, (a, b), 1)
        between = ari_nmi(table)[0]
        print(f"{case} gamma = {gamma}: device {dev['n_clusters']} clusters ARI {dev['ari']} stop {dev['stop']}, host {host['n_clusters']} "
              f"clusters ARI {host['ari']} stop {host['stop']}, between the routes {between}; modularity {dev['modularity']:.6f} / "
              f"{host['modularity']:.6f}")
        assert dev['n_clusters'] == host['n_clusters'] == case[0] and dev['ari'] == 1.0 and host['ari'] == 1.0 and between == 1.0
        assert dev['clusters'][0].dtype == np.int32 and [len(c) for c in dev['clusters']] == [half, len(X) - half]
        assert np.array_equal(dev['contingency'].sum(axis=1), dev['sizes']) and dev['modality_contingency'].shape == (case[0], 2)
        assert dev['n_edges'] > 0 and dev['graph'] is None and dev['stop'] in jld.STOPS and set(dev) == set(host)


def test_memory_at_20000_cells(jld):
    """No N x N: the peak of a whole run above the resident fuzzy graph stays within Louvain's bound, 256 bytes per stored entry
    and per cell plus 8 MiB.  The refinement adds ref, target, rsize (4 bytes each), rtot and cut (8 each): 28 bytes per node."""
    from jamie_amd import spectral as jsp
    N, L = 20000, 32
    rng = np.random.default_rng(4)
    centres = rng.standard_normal((10, L)) * 1.2
    x = torch.from_numpy((centres[rng.integers(0, 10, N)] + rng.standard_normal((N, L))).astype(np.float32)).cuda()
    G = jsp.build_graph(x, 15)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    resident = torch.cuda.memory_allocated()
    out = jld.communities(G)
    peak = torch.cuda.max_memory_allocated() - resident
    nnz = int(G.col.numel())
    bound = 256 * nnz + 256 * N + (8 << 20)
    print(f"N = {N}: {nnz} entries; the run's peak above the graph {peak / 2 ** 20:.1f} MiB (bound {bound / 2 ** 20:.1f} MiB, N x N bytes "
          f"{N * N / 2 ** 20:.0f} MiB), {len(out['sizes'])} clusters, stop {out['stop']}, modularity {out['modularity']:.4f}, levels "
          f"{[(lv['nodes'], lv['sweeps'], lv['refined']) for lv in out['levels']]}")
    assert peak < bound < N * N // 2

"""Leiden communities, the parts that need no GPU: the host route `_host_leiden_graph` against the per-node restatement of
leiden_util.py element for element (ref and cut after every sub-sweep, the counts, the levels, the clusters, the stop and the
modularity to the bit), the connectivity of every returned community, a run that ends stuck, the cancelled join, max_levels = 1,
the modularity against the host Louvain, the argument checks on both routes and the exports.  Every figure is printed before it
is asserted."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import leiden_util as du  # noqa: E402
import lisi_util as lu  # noqa: E402
import louvain_util as vu  # noqa: E402
import spectral_util as su  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('jamie_leiden_cut', 'jamie_leiden_refine', 'jamie_leiden_apply')
GRAPHS = ('blobs4', 'blobs3', 'blobs20', 'sheet', 'apart', 'cells40')
GAMMAS = (1.0, 0.5)
LOUVAIN_MARGIN = 0.02          # DESIGN.md §23's allowance against sequential Louvain


@functools.lru_cache(maxsize=None)
def host_run(name, gamma):
    from jamie_amd import jamie as jj
    trace = []
    out = jj._host_leiden_graph(*su.host_graph(name), resolution=gamma, trace=trace)
    return out, trace


def test_symbols_are_declared_and_exported():
    from jamie_amd import _native as nv
    hdr = open(os.path.join(ROOT, 'include', 'jamie_hip.h')).read()
    assert 'Leiden communities on the device' in hdr
    for s in SYMBOLS:
        assert s in nv.EXPORTS and f'{s}(' in hdr, s
    lib = nv.load()
    for s in SYMBOLS:
        assert hasattr(lib, s)
    csrc = os.path.join(ROOT, 'jamie_amd', 'csrc')
    src = open(os.path.join(csrc, 'community_rows.h')).read()
    assert f'CR_SHORT_MAX = {vu.SHORT_MAX};' in src and f'CR_LONG_MAX = {vu.LONG_MAX};' in src
    own = open(os.path.join(csrc, 'leiden.hip')).read()                      # the one pair of bin constants is the header's
    assert 'community_rows.h' in own and 'SHORT_MAX =' not in own and 'LONG_MAX =' not in own


def test_leiden_kernels_use_no_scratch():
    """private_segment_fixed_size == 0 and no spills for the kernels of csrc/leiden.hip, read from the code object hipcc built; the
    LDS tables are the sizes DESIGN.md §24 states, those of the move kernels: 12 bytes x 128 slots x 4 waves, and 12 bytes x 4096
    slots (and the reduction's few words)."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import isa_check as ic
    obj = os.path.join(ROOT, 'jamie_amd', 'csrc', '_obj', 'leiden.o')
    if not os.path.exists(obj):
        pytest.skip('the library is not built')
    if not os.path.exists(ic.OBJDUMP):
        pytest.skip('llvm-objdump not found')
    meta = ic.kernel_metadata(obj)
    names = ' '.join(meta)
    for kernel in ('ld_cut_kernel', 'ld_refine_short_kernel', 'ld_refine_long_kernel', 'ld_refine_global_kernel', 'ld_apply_kernel'):
        assert kernel in names, (kernel, names)
    assert len(meta) == 5
    for name, m in meta.items():
        print(name, {k: m.get(k) for k in ('vgpr_count', 'sgpr_count', 'group_segment_fixed_size', 'private_segment_fixed_size')})
        assert m['private_segment_fixed_size'] == 0, (name, m)
        assert m.get('vgpr_spill_count', 0) == 0 and m.get('sgpr_spill_count', 0) == 0, (name, m)
        lds = m.get('group_segment_fixed_size', 0)
        if 'ld_refine_short_kernel' in name:
            assert lds == 12 * 128 * 4, (name, m)
        elif 'ld_refine_long_kernel' in name:
            assert 12 * 4096 <= lds <= 12 * 4096 + 256, (name, m)
        else:
            assert lds <= 256, (name, m)


def test_bad_arguments_are_refused_before_any_launch():
    """The refusals come before any launch: no device is needed to see them."""
    from jamie_amd import _native as nv
    lib = nv.load()

    def refine(gamma=1.0, two_m=10, counts=(4, 0, 0), slot_off=None, n_slots=0, ws=None, ws_bytes=0, target=16, ref=8, n=4, k=8):
        return lib.jamie_leiden_refine(8, 8, 8, 0, n, k, 24, 8, ref, 8, 8, 8, gamma, two_m, 8, *counts, slot_off, n_slots, ws, ws_bytes,
                                       target, 8, None)
    assert refine(two_m=1 << 52) != 0 and b'two_m' in lib.jamie_last_error()
    assert refine(two_m=0) != 0 and b'two_m' in lib.jamie_last_error()
    assert refine(gamma=float('nan')) != 0 and b'gamma' in lib.jamie_last_error()
    assert refine(gamma=0.0) != 0 and b'gamma' in lib.jamie_last_error()
    assert refine(target=8) != 0 and b'differ' in lib.jamie_last_error()          # target is ref
    assert refine(target=24) != 0 and b'differ' in lib.jamie_last_error()         # target is comm
    assert refine(k=None) != 0 and b'null' in lib.jamie_last_error()
    assert refine(n=0) != 0 and refine(n=1 << 31) != 0
    assert refine(counts=(2, 2, 1)) != 0
    assert refine(counts=(2, 1, 1), slot_off=8, n_slots=10, ws=16, ws_bytes=100) != 0 and b'workspace' in lib.jamie_last_error()
    assert lib.jamie_leiden_cut(None, 8, 8, 0, 4, 8, 8, 8, None) != 0 and b'null' in lib.jamie_last_error()
    assert lib.jamie_leiden_cut(8, 8, 8, 0, 0, 8, 8, 8, None) != 0 and lib.jamie_leiden_cut(8, 8, 8, -1, 4, 8, 8, 8, None) != 0
    assert lib.jamie_leiden_apply(8, 0, 8, 8, 16, 8, 8, 8, 4, None) != 0           # count < 1
    assert lib.jamie_leiden_apply(8, 5, 8, 8, 16, 8, 8, 8, 4, None) != 0           # count > n
    assert lib.jamie_leiden_apply(8, 2, 16, 8, 16, 8, 8, 8, 4, None) != 0 and b'differ' in lib.jamie_last_error()
    assert lib.jamie_leiden_apply(8, 2, 8, 8, 16, 8, 8, None, 4, None) != 0 and b'null' in lib.jamie_last_error()


@pytest.mark.parametrize('route', ['host', 'device'])
def test_value_errors_on_both_routes(route):
    """Every refusal of JAMIE.louvain is JAMIE.leiden's: it comes from the shared argument checks, names leiden, and comes before
    either route touches a device."""
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
        with pytest.raises(ValueError, match='leiden'):
            call()
    for kw in cases:
        refused(lambda: j.leiden(emb, **kw))
        with pytest.raises(ValueError, match='louvain'):
            jlv.check_louvain(emb, **kw)
    for bad in (bad_nan, [emb[0], emb[1][:, :3]], []):
        refused(lambda: j.leiden(bad))
    refused(lambda: j.leiden(emb, datatype=[np.zeros(60), np.zeros(49)]))       # one label per cell


@pytest.mark.parametrize('gamma', GAMMAS)
@pytest.mark.parametrize('name', GRAPHS)
def test_host_route_equals_the_restatement(name, gamma):
    got, trace = host_run(name, gamma)
    want_trace = []
    want = du.restated_fuzzy(*su.host_graph(name), gamma, trace=want_trace)
    print(f"{name} gamma = {gamma}: {len(got['sizes'])} clusters, stop {got['stop']} (restated {want['stop']}), modularity "
          f"{got['modularity']!r} (restated {want['modularity']!r}), levels "
          f"{[(lv['nodes'], lv['communities'], lv['refined'], lv['merged'], lv['cancelled']) for lv in got['levels']]}")
    assert du.same_trace(trace, want_trace)                 # ref and cut after every sub-sweep, the counts so far
    assert np.array_equal(got['clusters'], want['clusters']) and np.array_equal(got['sizes'], want['sizes'])
    assert got['stop'] == want['stop'] and got['modularity'] == want['modularity'] and got['levels'] == want['levels']
    assert got['clusters'].dtype == np.int32 and len(got['levels']) >= 2 and len(trace) >= 1
    levels = got['levels']
    assert all(a['refined'] == b['nodes'] < a['nodes'] for a, b in zip(levels, levels[1:]))      # every level shrinks the graph
    assert len({lv['two_m'] for lv in levels}) == 1


@pytest.mark.parametrize('gamma', GAMMAS)
@pytest.mark.parametrize('name', GRAPHS)
def test_every_community_is_connected(name, gamma):
    rowptr, col, _ = su.host_graph(name)
    got, _ = host_run(name, gamma)
    parts, comms = du.components_within(rowptr, col, got['clusters'])
    print(f"{name} gamma = {gamma}: stop {got['stop']}, {comms} communities in {parts} connected parts")
    assert got['stop'] != 'max_levels' and parts == comms


@pytest.mark.parametrize('gamma', GAMMAS)
@pytest.mark.parametrize('name', GRAPHS)
def test_modularity_against_the_host_louvain(name, gamma):
    from jamie_amd import jamie as jj
    got, _ = host_run(name, gamma)
    louvain = jj._host_louvain_graph(*su.host_graph(name), resolution=gamma)
    g = vu.graph_of(*su.host_graph(name)[:2], vu.restated_quantise(su.host_graph(name)[2]))
    assert abs(vu.partition_modularity(g, got['clusters'], gamma) - got['modularity']) <= 1e-12      # Q is the returned partition's
    print(f"{name} gamma = {gamma}: leiden {got['modularity']:.6f} in {len(got['sizes'])} clusters, louvain {louvain['modularity']:.6f} "
          f"in {len(louvain['sizes'])}; deficit {louvain['modularity'] - got['modularity']:.6f} (margin {LOUVAIN_MARGIN})")
    assert got['modularity'] >= louvain['modularity'] - LOUVAIN_MARGIN


@pytest.mark.parametrize('name', ('blobs4', 'sheet'))
def test_max_levels_one_is_the_first_level_of_louvain(name):
    from jamie_amd import jamie as jj
    graph = su.host_graph(name)
    one = jj._host_leiden_graph(*graph, max_levels=1)
    louvain = jj._host_louvain_graph(*graph, max_levels=1)
    print(f"{name}: {len(one['sizes'])} clusters, stop {one['stop']}, modularity {one['modularity']!r} (louvain {louvain['modularity']!r})")
    assert one['stop'] == 'max_levels' and len(one['levels']) == 1 and one['levels'][0]['refined'] is None
    assert np.array_equal(one['clusters'], louvain['clusters']) and one['modularity'] == louvain['modularity']
    assert one['levels'][0]['moved'] == louvain['levels'][0]['moved']
    two = jj._host_leiden_graph(*graph, max_levels=2)
    assert two['stop'] == 'max_levels' and len(two['levels']) == 2 and two['levels'][0]['merged'] > 0


def test_cancelled_join():
    """The chain i - u - t with i and u of one class: u leaves for t in the sub-sweep in which i wants to join u, so i's join is
    cancelled and i stays alone; one level up the part of i joins the part {t, u}."""
    from jamie_amd import jamie as jj
    g, comm, i, u, t = du.cancel_chain()
    s = vu.node_class(i)
    assert vu.node_class(u) == s != vu.node_class(t) and t < u < i
    _, tot, _ = vu.state_of(g, comm)
    trace, want_trace = [], []
    ref, merged, cancelled = jj._host_leiden_refine(g['rowptr'], g['col'], g['w'], g['k'], comm, tot, 1.0, g['two_m'], trace)
    want = du.restated_refine(g, comm, tot, 1.0, want_trace)
    print(f'chain {i} - {u} - {t} (class {s}): merged {merged}, cancelled {cancelled}, ref of the three {ref[[i, u, t]].tolist()}')
    assert du.same_trace([trace], [want_trace]) and np.array_equal(ref, want[0])
    assert (merged, cancelled) == (1, 1) == want[1:]
    assert trace[s - 1]['merged'] == 0 and (trace[s]['merged'], trace[s]['cancelled']) == (1, 1)
    assert ref[u] == t and ref[i] == i and np.sum(ref == i) == 1           # i is still alone after its sub-sweep and at the end
    # the targets of that sub-sweep: i proposed u, u proposed t
    st = du.fresh(g)
    for c in range(s):
        du.restated_subsweep(g, comm, tot, *st, c, 1.0)
    cut = du.restated_cut(g, comm, st[0])
    targets = du.restated_targets(g, comm, tot, *st, cut, du.class_lists(g['n'])[s], 1.0)
    assert targets[i] == u and targets[u] == t
    # later: one level up, i's part and the part {t, u} share a community and merge
    nxt, cmap = vu.restated_aggregate(g, ref)
    comm0 = du.restated_next(comm, cmap, nxt['n'])
    _, tot0, _ = vu.state_of(nxt, comm0)
    ref2, merged2, cancelled2 = jj._host_leiden_refine(nxt['rowptr'], nxt['col'], nxt['w'], nxt['k'], comm0, tot0, 1.0, nxt['two_m'])
    assert comm0[cmap[i]] == comm0[cmap[t]] == min(cmap[i], cmap[t]) and cmap[u] == cmap[t] != cmap[i]
    assert (merged2, cancelled2) == (1, 0) and ref2[cmap[i]] == ref2[cmap[t]]
    # and the whole run from these communities' graph ends with the three in one community
    out = jj._host_leiden_levels(g['rowptr'], g['col'], g['w'], g['loop'])
    assert out['comm'][i] == out['comm'][u] == out['comm'][t] and out['stop'] == 'singletons'


def test_a_stuck_run_returns_the_parts():
    """The pinned graph of leiden_util.stuck_graph ends stuck at resolution 1: the last level's nodes are returned, each one
    connected, and their Q is no lower than that of the communities whose parts refused to merge."""
    from jamie_amd import jamie as jj
    rowptr, col, val = du.stuck_graph()
    got = jj._host_leiden_graph(rowptr, col, val)
    want = du.restated_fuzzy(rowptr, col, val)
    last = got['levels'][-1]
    parts, comms = du.components_within(rowptr, col, got['clusters'])
    g = vu.graph_of(rowptr, col, vu.restated_quantise(val))
    print(f"stuck: {len(rowptr) - 1} cells, levels {[(lv['nodes'], lv['communities'], lv['refined'], lv['merged']) for lv in got['levels']]}; "
          f"the {len(got['sizes'])} parts have modularity {got['modularity']!r}, the {last['communities']} communities {last['modularity']!r}; "
          f"{comms} returned communities in {parts} connected parts")
    assert got['stop'] == 'stuck' == want['stop'] and last['merged'] == 0 and last['refined'] == last['nodes']
    assert len(got['sizes']) == last['nodes'] > last['communities']             # the parts, not the communities
    assert got['modularity'] >= last['modularity']
    assert abs(vu.partition_modularity(g, got['clusters'], 1.0) - got['modularity']) <= 1e-12
    assert np.array_equal(got['clusters'], want['clusters']) and got['levels'] == want['levels'] and got['modularity'] == want['modularity']
    assert parts == comms


def test_stuck_pair_returns_the_parts():
    """Two nodes of one community with w_ab <= gamma k_a k_b / two_m: the refinement merges nothing (the gain of the join is not
    positive) and the run would return the level's nodes."""
    from jamie_amd import jamie as jj
    g, comm = du.stuck_pair()
    _, tot, _ = vu.state_of(g, comm)
    ref, merged, cancelled = jj._host_leiden_refine(g['rowptr'], g['col'], g['w'], g['k'], comm, tot, 1.0, g['two_m'])
    want = du.restated_refine(g, comm, tot, 1.0)
    assert ref.tolist() == [0, 1] == want[0].tolist() and (merged, cancelled) == (0, 0) == want[1:]
    assert float(g['w'][0]) <= 1.0 * float(g['k'][0]) * float(g['k'][1]) / float(g['two_m'])

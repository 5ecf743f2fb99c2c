"""Shared by tests/test_host_leiden.py and tests/test_hip_leiden.py: a per-node restatement of DESIGN.md §24 steps 3-5 in plain
Python integers and floats, one node at a time (no code shared with `_host_leiden_graph` or jamie_amd/leiden.py; the move phase,
the aggregation and the tables of Q are louvain_util's restatements), the whole run around it, the connectivity of a partition
and the hand-built level graphs of the refinement's special cases."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import louvain_util as vu  # noqa: E402


# ---- the refinement, node by node ----
def well(x, t, T, gamma, two_m):
    return float(x) >= ((float(gamma) * float(t)) * float(T - t)) / float(two_m)


def fresh(g):
    """ref, rtot, rsize with every node alone."""
    return np.arange(g['n'], dtype=np.int64), g['k'].copy(), np.ones(g['n'], np.int64)


def restated_cut(g, comm, ref):
    cut = [0] * g['n']
    for i in range(g['n']):
        for e in range(g['rowptr'][i], g['rowptr'][i + 1]):
            j = int(g['col'][e])
            if comm[j] == comm[i] and ref[j] != ref[i]:
                cut[int(ref[i])] += int(g['w'][e])
    return np.array(cut, np.int64)


def restated_targets(g, comm, tot, ref, rtot, rsize, cut, nodes, gamma):
    """{node: target} of `nodes` (one class) from the state as it stands: ref for a node that is no longer alone."""
    two_m = g['two_m']
    out = {}
    for i in nodes:
        out[i] = int(ref[i])
        if rsize[ref[i]] != 1:
            continue
        assert ref[i] == i
        C, ki = int(comm[i]), int(g['k'][i])
        T = int(tot[C])
        cut_i, kis = 0, {}
        for e in range(g['rowptr'][i], g['rowptr'][i + 1]):
            j = int(g['col'][e])
            if comm[j] == C:
                cut_i += int(g['w'][e])
                kis[int(ref[j])] = kis.get(int(ref[j]), 0) + int(g['w'][e])
        if not well(cut_i, ki, T, gamma, two_m):
            continue
        best_gain = None
        for S in sorted(kis):                                # ascending: the first of equal gains is the lowest id
            if rsize[S] == 1 and S > i:
                continue
            if not well(int(cut[S]), int(rtot[S]), T, gamma, two_m):
                continue
            gain = float(kis[S]) - ((float(gamma) * float(ki)) * float(int(rtot[S]))) / float(two_m)
            if gain > 0.0 and (best_gain is None or gain > best_gain):
                out[i], best_gain = S, gain
    return out


def restated_join(g, ref, rtot, rsize, targets):
    """Applies {node: target} in place; (merged, cancelled).  The targets of the other classes' nodes are their ref: a founder of
    another class never leaves in this sub-sweep."""
    merged = cancelled = 0
    for i, S in targets.items():
        if S == ref[i]:
            continue
        if targets.get(S, S) != S:
            cancelled += 1
            continue
        ki = int(g['k'][i])
        rtot[ref[i]] -= ki
        rsize[ref[i]] -= 1
        rtot[S] += ki
        rsize[S] += 1
        merged += 1
    for i, S in targets.items():                             # (ref is read above as it stood: the joins of a sub-sweep do not chain)
        if S != ref[i] and targets.get(S, S) == S:
            ref[i] = S
    return merged, cancelled


def class_lists(n):
    return [[i for i in range(n) if vu.node_class(i) == s] for s in range(8)]


def restated_subsweep(g, comm, tot, ref, rtot, rsize, s, gamma, lists=None):
    """One class: (cut, targets, merged, cancelled); ref, rtot, rsize change in place."""
    nodes = (lists or class_lists(g['n']))[s]
    cut = restated_cut(g, comm, ref)
    targets = restated_targets(g, comm, tot, ref, rtot, rsize, cut, nodes, gamma)
    merged, cancelled = restated_join(g, ref, rtot, rsize, targets)
    return cut, targets, merged, cancelled


def restated_refine(g, comm, tot, gamma, trace=None):
    """(ref, merged, cancelled) of a level's refinement; `trace` as the routes fill it."""
    ref, rtot, rsize = fresh(g)
    lists = class_lists(g['n'])
    merged = cancelled = 0
    for s in range(8):
        cut, _, m, c = restated_subsweep(g, comm, tot, ref, rtot, rsize, s, gamma, lists)
        merged, cancelled = merged + m, cancelled + c
        if trace is not None:
            trace.append(dict(ref=ref.copy(), cut=cut, merged=merged, cancelled=cancelled))
    return ref, merged, cancelled


def restated_moves(g, comm0, gamma, max_sweeps=32):
    """The move phase from comm0: louvain_util's sweeps and stop rule."""
    comm, tot, size = vu.state_of(g, comm0)
    history = []
    for _ in range(max_sweeps):
        history.append(vu.restated_sweep(g, comm, tot, size, gamma))
        if history[-1] == 0 or vu.restated_stalled(history):
            break
    return comm, tot, size, history


def restated_next(comm, cmap, nc):
    low = {}
    for c, r in zip(comm, cmap):
        low[int(c)] = min(low.get(int(c), nc), int(r))
    comm0 = np.empty(nc, np.int64)
    for c, r in zip(comm, cmap):
        comm0[r] = low[int(c)]
    return comm0


def restated_run(g, gamma=1.0, max_levels=20, max_sweeps=32, trace=None):
    """dict(clusters, sizes, modularity, levels, stop) of the whole run on a level graph."""
    two_m = g['two_m']
    cells = np.arange(g['n'], dtype=np.int64)
    comm0, levels = cells.copy(), []

    def done(result, q, stop):
        clusters, sizes = vu.restated_relabel(result)
        return dict(clusters=clusters, sizes=sizes, modularity=q, levels=levels, stop=stop)
    while True:
        comm, tot, size, history = restated_moves(g, comm0, gamma, max_sweeps)
        q = vu.restated_modularity(vu.restated_internal(g, comm), tot, two_m, gamma)
        nc = len(set(comm.tolist()))
        rec = dict(nodes=g['n'], communities=nc, sweeps=len(history), moved=history, modularity=q, two_m=two_m, refined=None,
                   merged=None, cancelled=None)
        levels.append(rec)
        if nc == g['n']:
            return done(comm[cells], q, 'singletons')
        if len(levels) == max_levels:
            return done(comm[cells], q, 'max_levels')
        sub = None
        if trace is not None:
            sub = []
            trace.append(sub)
        ref, merged, cancelled = restated_refine(g, comm, tot, gamma, sub)
        rec.update(merged=merged, cancelled=cancelled)
        if merged == 0:
            rec.update(refined=g['n'])
            return done(cells, vu.restated_modularity(g['loop'], g['k'], two_m, gamma), 'stuck')
        nxt, cmap = vu.restated_aggregate(g, ref)
        rec.update(refined=nxt['n'])
        comm0 = restated_next(comm, cmap, nxt['n'])
        cells = cmap[cells]
        g = nxt


def restated_fuzzy(rowptr, col, val, gamma=1.0, **kw):
    return restated_run(vu.graph_of(rowptr, col, vu.restated_quantise(val)), gamma, **kw)


def same_trace(got, want):
    """Whether two traces (a list per refined level of one dict per sub-sweep) are equal element for element."""
    if len(got) != len(want):
        return False
    for a, b in zip(got, want):
        if len(a) != len(b) or len(a) != 8:
            return False
        for x, y in zip(a, b):
            if not (np.array_equal(x['ref'], y['ref']) and np.array_equal(x['cut'], y['cut'])
                    and (x['merged'], x['cancelled']) == (y['merged'], y['cancelled'])):
                return False
    return True


# ---- connectivity ----
def components_within(rowptr, col, clusters):
    """(connected components of the graph's entries with both ends in one community, communities)."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    rowptr, col, clusters = np.asarray(rowptr, np.int64), np.asarray(col, np.int64), np.asarray(clusters)
    n = len(rowptr) - 1
    row = np.repeat(np.arange(n), np.diff(rowptr))
    keep = clusters[row] == clusters[col]
    A = csr_matrix((np.ones(int(keep.sum())), (row[keep], col[keep])), shape=(n, n))
    return int(connected_components(A, directed=False)[0]), len(np.unique(clusters))


# ---- hand-built level graphs ----
def same_class_pair(lo=1, hi=400):
    """The lowest (u, i) with u < i in [lo, hi) of one class."""
    for u in range(lo, hi):
        for i in range(u + 1, hi):
            if vu.node_class(i) == vu.node_class(u):
                return u, i
    raise AssertionError('no pair')


@functools.lru_cache(maxsize=None)
def cancel_chain():
    """(g, comm, i, u, t): a chain i - u - t in one community, i and u of one class and t = 0 of an earlier one with t < u < i.
    In the class of i and u both are alone: u's best part is t (the heavier edge), i's only candidate is u, so i's join is
    cancelled and i stays alone in that sub-sweep (t itself has no admitted candidate in its class: u is alone and above it).
    The other ids are isolated nodes with a loop, each a community of its own."""
    t = 0
    s0 = vu.node_class(t)
    u, i = next((u, i) for u in range(1, 400) for i in range(u + 1, 400)
                if vu.node_class(u) == vu.node_class(i) and vu.node_class(u) > s0)
    n = i + 1
    loop = np.full(n, 3, np.int64)
    loop[[t, u, i]] = 0
    g = vu.from_edges(n, [(t, u, 9), (u, i, 4)], loop)
    comm = np.arange(n, dtype=np.int64)
    comm[[u, i]] = t
    return g, comm, i, u, t


@functools.lru_cache(maxsize=None)
def stuck_pair():
    """(g, comm): two nodes in one community whose edge is too light to merge them: w_ab = 1 <= gamma k_a k_b / two_m with loops
    of 50 (k = 51, two_m = 102: 25.5), so the gain of the join is negative and the refinement merges nothing."""
    g = vu.from_edges(2, [(0, 1, 1)], [50, 50])
    return g, np.zeros(2, np.int64)


STUCK_CELLS = (3, 120, 4, 1.0, 1, 15)      # (blobs, cells per blob, L, centre spread, seed, n_neighbors): ends stuck at resolution 1


@functools.lru_cache(maxsize=None)
def stuck_graph():
    """(rowptr, col, val fp32) of the host route's fuzzy graph of STUCK_CELLS: 360 cells of three overlapping blobs, found by a
    search over 6 shapes x 8 seeds x 2 neighbour counts x 3 resolutions with the host route (29 of the 288 runs ended stuck)."""
    from jamie_amd import jamie as jj
    T, per, L, spread, seed, nn = STUCK_CELLS
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((T, L)) * spread
    X = np.repeat(centres, per, axis=0) + rng.standard_normal((T * per, L))
    X = X[rng.permutation(T * per)].astype(np.float32)
    order, dist = jj._host_sorted_neighbors([X], nn - 1, 'leiden')
    W, _, _, _ = jj._host_smooth_knn(dist, nn)
    return jj._host_fuzzy_graph(order, W)


def filtered_hub(m=300, inside=40, seed=5):
    """(g, comm): node 0 has m leaves of which only `inside` share its community (the others form communities of their own ring
    neighbours), so most of the hub's entries are dropped by the community filter."""
    rng = np.random.default_rng(seed)
    edges = [(0, j, int(rng.integers(1, 8))) for j in range(1, m + 1)]
    edges += [(j, j + 1 if j < m else 1, int(rng.integers(1, 6))) for j in range(1, m + 1)]
    g = vu.from_edges(m + 1, edges)
    comm = np.zeros(m + 1, np.int64)
    comm[inside + 1:] = inside + 1 + ((np.arange(m - inside) // 7) * 7)
    return g, comm

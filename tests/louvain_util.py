"""Shared by tests/test_host_louvain.py and tests/test_hip_louvain.py: a per-node restatement of DESIGN.md §23 in plain Python
integers and floats (one dict of candidates per node; no code shared with `_host_louvain_graph` or jamie_amd/louvain.py), a
sequential Louvain as a quality reference, the well-separated blobs and synthetic integer level graphs."""
import functools

import numpy as np

SHORT_MAX, LONG_MAX = 64, 2048         # the bin limits of the move kernel, as the issue of the feature names them
WELL_SEPARATED = ((6, 60, 8, 6.0, 11), (3, 43, 4, 8.0, 12), (12, 50, 16, 5.0, 13))      # (T, per, L, spread, seed)
QUANT = 2.0 ** 20


# ---- graphs ----
def graph_of(rowptr, col, w, loop=None):
    """dict(n, rowptr, col, w, loop, k, two_m) of Python-friendly int64 arrays."""
    rowptr, col, w = np.asarray(rowptr, np.int64), np.asarray(col, np.int64), np.asarray(w, np.int64)
    n = len(rowptr) - 1
    loop = np.zeros(n, np.int64) if loop is None else np.asarray(loop, np.int64)
    k = np.array([int(w[rowptr[i]:rowptr[i + 1]].sum()) + int(loop[i]) for i in range(n)], np.int64)
    return dict(n=n, rowptr=rowptr, col=col, w=w, loop=loop, k=k, two_m=int(k.sum()))


def restated_quantise(val):
    """max(1, round-half-even(val 2^20)) entry by entry with Python's round (which rounds half to even)."""
    return np.array([max(1, round(float(np.float32(v)) * QUANT)) for v in val], np.int64)


def from_edges(n, edges, loop=None):
    """The symmetric level graph of undirected (i, j, w) edges, rows in ascending column order."""
    rows = [dict() for _ in range(n)]
    for i, j, w in edges:
        assert i != j and j not in rows[i]
        rows[i][j] = int(w)
        rows[j][i] = int(w)
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    col = [j for r in rows for j in sorted(r)]
    w = [r[j] for r in rows for j in sorted(r)]
    return graph_of(rowptr, col, w, loop)


@functools.lru_cache(maxsize=None)
def synthetic(name):
    """Integer level graphs for the paths of the move kernel."""
    if name.startswith('star'):          # node 0 has `m` leaves (weights 1 .. 7), the leaves form a ring (weights 1 .. 5)
        m = int(name[4:])
        rng = np.random.default_rng(m)
        edges = [(0, j, int(rng.integers(1, 8))) for j in range(1, m + 1)]
        edges += [(j, j + 1 if j < m else 1, int(rng.integers(1, 6))) for j in range(1, m + 1)]
        return from_edges(m + 1, edges)
    if name == 'heavy':                  # loops and weights near 2^40: sums beyond 2^32 and beyond fp32
        rng = np.random.default_rng(3)
        n = 60
        edges = {}
        for i in range(n):
            for j in rng.choice(n, 5, replace=False):
                if i != j:
                    edges[(min(i, j), max(i, j))] = (1 << 40) + int(rng.integers(-1000, 1000))
        loop = (1 << 39) + rng.integers(0, 1 << 30, n)
        loop[::7] = 0
        return from_edges(n, [(i, j, w) for (i, j), w in sorted(edges.items())], loop)
    if name == 'ring':                   # equal weights: every gain ties
        n = 37
        return from_edges(n, [(i, (i + 1) % n, 5) for i in range(n)])
    if name == 'pairs':                  # two isolated pairs: without the singleton rule the two nodes of a pair swap
        return from_edges(4, [(0, 1, 3), (2, 3, 3)])
    if name == 'empty':                  # node 9 has an empty row (and a loop), node 10 an empty row and no loop
        return from_edges(11, [(i, (i + 1) % 9, 1 + i % 3) for i in range(9)], [0] * 9 + [4, 0])
    raise KeyError(name)


def separated_blobs(T, per, L, spread, seed):
    """(X float32 [T per, L], labels int64): the recipe of the well-separated blobs."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((T, L)) * spread
    X = np.repeat(centres, per, axis=0) + rng.standard_normal((T * per, L))
    labels = np.repeat(np.arange(T), per)
    perm = rng.permutation(T * per)
    return X[perm].astype(np.float32), labels[perm]


# ---- the restatement, node by node ----
def node_class(i):
    return ((int(i) * 2654435761) >> 7) & 7


def restated_move(g, comm, tot, size, nodes, gamma):
    """{node: target} of `nodes` from the state as it stands."""
    rowptr, col, w, two_m = g['rowptr'], g['col'], g['w'], float(g['two_m'])
    out = {}
    for i in nodes:
        c, ki = int(comm[i]), int(g['k'][i])
        kid = {}
        for e in range(rowptr[i], rowptr[i + 1]):
            d = int(comm[col[e]])
            kid[d] = kid.get(d, 0) + int(w[e])
        gki = float(gamma) * float(ki)
        stay = float(kid.get(c, 0)) - (gki * float(int(tot[c]) - ki)) / two_m
        best, best_gain = c, None
        for d in sorted(kid):                                # ascending: the first of equal gains is the lowest id
            if d == c or (size[c] == 1 and size[d] == 1 and d > c):
                continue
            gain = float(kid[d]) - (gki * float(int(tot[d]))) / two_m
            if gain > stay and (best_gain is None or gain > best_gain):
                best, best_gain = d, gain
        out[i] = best
    return out


def restated_apply(g, comm, tot, size, targets):
    """Applies {node: target} in place; the number of nodes moved."""
    moved = 0
    for i, d in targets.items():
        c = int(comm[i])
        if d != c:
            ki = int(g['k'][i])
            comm[i] = d
            tot[c] -= ki
            tot[d] += ki
            size[c] -= 1
            size[d] += 1
            moved += 1
    return moved


def singleton_state(g):
    return np.arange(g['n'], dtype=np.int64), g['k'].copy(), np.ones(g['n'], np.int64)


def state_of(g, comm):
    comm = np.asarray(comm, np.int64).copy()
    tot, size = np.zeros(g['n'], np.int64), np.zeros(g['n'], np.int64)
    for i, c in enumerate(comm):
        tot[c] += g['k'][i]
        size[c] += 1
    return comm, tot, size


def restated_sweep(g, comm, tot, size, gamma):
    moved = 0
    for s in range(8):
        nodes = [i for i in range(g['n']) if node_class(i) == s]
        moved += restated_apply(g, comm, tot, size, restated_move(g, comm, tot, size, nodes, gamma))
    return moved


def restated_stalled(history, patience=3):
    low = min(history)
    return len(history) - 1 - history.index(low) >= patience


def restated_level(g, gamma, max_sweeps=32):
    comm, tot, size = singleton_state(g)
    history = []
    for _ in range(max_sweeps):
        history.append(restated_sweep(g, comm, tot, size, gamma))
        if history[-1] == 0 or restated_stalled(history):
            break
    return comm, tot, size, history


def restated_internal(g, comm):
    inside = np.zeros(g['n'], np.int64)
    for i in range(g['n']):
        inside[comm[i]] += g['loop'][i]
        for e in range(g['rowptr'][i], g['rowptr'][i + 1]):
            if comm[g['col'][e]] == comm[i]:
                inside[comm[i]] += g['w'][e]
    return inside


def restated_modularity(inside, tot, two_m, gamma):
    q = 0.0
    for a, t in zip(inside, tot):                            # ascending community id
        x = float(int(t)) / float(two_m)
        q = q + (float(int(a)) / float(two_m) - float(gamma) * (x * x))
    return q


def restated_aggregate(g, comm):
    """(the coarse graph, new id of every node)."""
    ids = sorted(set(int(c) for c in comm))
    new = {c: r for r, c in enumerate(ids)}
    rows = [dict() for _ in ids]
    loop = [0] * len(ids)
    for i in range(g['n']):
        a = new[int(comm[i])]
        loop[a] += int(g['loop'][i])
        for e in range(g['rowptr'][i], g['rowptr'][i + 1]):
            b = new[int(comm[g['col'][e]])]
            if a == b:
                loop[a] += int(g['w'][e])
            else:
                rows[a][b] = rows[a].get(b, 0) + int(g['w'][e])
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    col = [b for r in rows for b in sorted(r)]
    w = [r[b] for r in rows for b in sorted(r)]
    return graph_of(rowptr, col, w, loop), np.array([new[int(c)] for c in comm], np.int64)


def restated_relabel(comm):
    members = {}
    for i, c in enumerate(comm):
        members.setdefault(int(c), []).append(i)
    order = sorted(members, key=lambda c: (-len(members[c]), members[c][0]))
    out = np.empty(len(comm), np.int32)
    for r, c in enumerate(order):
        out[members[c]] = r
    return out, np.array([len(members[c]) for c in order], np.int64)


def restated_run(g, gamma=1.0, max_levels=20, max_sweeps=32, tol=1e-7):
    """dict(clusters, sizes, modularity, levels) of the whole run on a level graph."""
    two_m = g['two_m']
    q_prev = restated_modularity(g['loop'], g['k'], two_m, gamma)
    result = np.arange(g['n'], dtype=np.int64)
    levels = []
    while len(levels) < max_levels:
        comm, tot, size, history = restated_level(g, gamma, max_sweeps)
        q = restated_modularity(restated_internal(g, comm), tot, two_m, gamma)
        if not q > q_prev + tol:
            break
        nxt, cmap = restated_aggregate(g, comm)
        levels.append(dict(nodes=g['n'], communities=nxt['n'], sweeps=len(history), moved=history, modularity=q, two_m=nxt['two_m']))
        result = cmap[result]
        g, q_prev = nxt, q
    clusters, sizes = restated_relabel(result)
    return dict(clusters=clusters, sizes=sizes, modularity=q_prev, levels=levels)


def restated_fuzzy(rowptr, col, val, gamma=1.0, **kw):
    return restated_run(graph_of(rowptr, col, restated_quantise(val)), gamma, **kw)


def partition_modularity(g, part, gamma):
    """Q of any partition (one id per node) on a level graph."""
    comm = np.unique(np.asarray(part), return_inverse=True)[1].reshape(-1)
    _, tot, _ = state_of(g, comm)
    return restated_modularity(restated_internal(g, comm), tot, g['two_m'], gamma)


# ---- the quality reference ----
def sequential_louvain(g, gamma=1.0):
    """Plain sequential Louvain (index order, immediate updates, passes until nothing moves, levels until nothing merges):
    (partition of the level-0 nodes, its modularity)."""
    result = np.arange(g['n'], dtype=np.int64)
    while True:
        comm, tot, size = singleton_state(g)
        any_move, moved = False, True
        while moved:
            moved = False
            for i in range(g['n']):
                if restated_apply(g, comm, tot, size, restated_move(g, comm, tot, size, [i], gamma)):
                    moved = any_move = True
        if not any_move:
            break
        g, cmap = restated_aggregate(g, comm)
        result = cmap[result]
    return result, restated_modularity(g['loop'], g['k'], g['two_m'], gamma)

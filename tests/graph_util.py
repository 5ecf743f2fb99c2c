"""Restatements for the graph-structure tests that share no code with either route of jamie_amd: the components by
a breadth-first search in Python integers, the synchronous min-label rounds in numpy with every intermediate array, scipy's weak
components mapped to their smallest member, kBET per cell in Python floats in the stated order, and the shape cases."""
import functools
import math
from collections import deque

import numpy as np

U = 2.0 ** -53
HOOK_GROUP = 16            # lanes of a row of the hook (csrc/graph.hip GR_GROUP)
HOOK_ROWS = 256 // HOOK_GROUP      # rows of a workgroup
HOOK_LONG = 256            # entries beyond which the workgroup takes a row (csrc/graph.hip GR_LONG)
CASES = ('one', 'two_empty', 'empty', 'path_up', 'path_down', 'path_zigzag', 'path_perm', 'star', 'star_out', 'star_in', 'knn',
         'dups', 'outside', 'n257', 'n65537', 'group_path')


def counted(rowptr, col, n, group=None):
    """(row, col) of the entries that count: 0 <= j < n, j != i, and one group on both ends when there are groups."""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    ok = (col >= 0) & (col < n)
    ok[ok] &= col[ok] != row[ok]
    if group is not None:
        g = np.asarray(group)
        ok[ok] &= g[row[ok]] == g[col[ok]]
    return row[ok], col[ok]


def bfs_components(rowptr, col, n, group=None):
    """root int64 [n]: the smallest node of every node's component, by a per-node breadth-first search over the entries that
    count, each taken both ways."""
    row, c = counted(rowptr, col, n, group)
    nb = [[] for _ in range(n)]
    for i, j in zip(row.tolist(), c.tolist()):
        nb[i].append(j)
        nb[j].append(i)
    root = [-1] * n
    for s in range(n):                                  # (ascending: s is the smallest node of a component it starts)
        if root[s] >= 0:
            continue
        root[s] = s
        queue = deque([s])
        while queue:
            i = queue.popleft()
            for j in nb[i]:
                if root[j] < 0:
                    root[j] = s
                    queue.append(j)
    return np.array(root, dtype=np.int64)


def scipy_components(rowptr, col, n, group=None):
    """root int64 [n] from `scipy.sparse.csgraph.connected_components(connection='weak')`, ids mapped through their smallest member."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    row, c = counted(rowptr, col, n, group)
    A = coo_matrix((np.ones(len(row), np.int8), (row, c)), shape=(n, n)).tocsr()
    _, lab = connected_components(A, directed=True, connection='weak')
    first = np.full(lab.max() + 1, n, np.int64)
    np.minimum.at(first, lab, np.arange(n))
    return first[lab]


def restated_rounds(rowptr, col, n, group=None):
    """The rounds of DESIGN.md §26 in numpy: dict(root, rounds, jumps, steps); `steps` is every array in order: ('hook', parent)
    after a round's hook, then ('root', root) after its completed compress (absent in the last round, whose hook finds nothing)."""
    row, c = counted(rowptr, col, n, group)
    root = np.arange(n, dtype=np.int32)
    steps, rounds, jumps = [], 0, 0
    while True:
        rounds += 1
        a, b = root[row], root[c]
        ne = a != b
        parent = root.copy()
        np.minimum.at(parent, np.where(a > b, a, b)[ne], np.where(a > b, b, a)[ne])
        steps.append(('hook', parent.copy()))
        if not ne.any():
            break
        while True:
            jumps += 1
            nxt = parent[parent]
            same = bool((nxt == parent).all())
            parent = nxt
            if same:
                break
        root = parent
        steps.append(('root', root.copy()))
    return dict(root=root, rounds=rounds, jumps=jumps, steps=steps)


def round_bound(n):
    return math.ceil(math.log2(n)) + 2 if n > 1 else 2


def restated_kbet(idx, codes, expected, erow=None):
    """(stat float64 [N], df int32 [N], counts int64 [N, B]) per cell in Python floats: the sum in ascending category over the
    categories with expected > 0 of ((o - e) * (o - e)) / e, e = k * expected."""
    idx, codes, expected = np.asarray(idx), np.asarray(codes), np.asarray(expected, dtype=np.float64)
    N, K = idx.shape
    B = expected.shape[1]
    stat, df, counts = np.full(N, np.nan), np.zeros(N, np.int32), np.zeros((N, B), np.int64)
    for i in range(N):
        o = [0] * B
        for t in range(K):
            j = int(idx[i, t])
            if 0 <= j < N:
                b = int(codes[j])
                if 0 <= b < B:
                    o[b] += 1
        counts[i] = o
        k = sum(o)
        f = [float(v) for v in expected[0 if erow is None else int(erow[i])]]
        cats = sum(1 for v in f if v > 0.0)
        if k == 0 or cats - 1 < 1 or any(o[b] > 0 and not f[b] > 0.0 for b in range(B)):
            continue
        s = 0.0
        for b in range(B):
            if f[b] > 0.0:
                e = float(k) * f[b]
                d = float(o[b]) - e
                s = s + (d * d) / e
        stat[i], df[i] = s, cats - 1
    return stat, df, counts


def csr_of(rows, n):
    """(rowptr int64 [n + 1], col int32) from a list of n rows of column lists."""
    rowptr = np.zeros(n + 1, np.int64)
    rowptr[1:] = np.cumsum([len(r) for r in rows])
    col = np.array([j for r in rows for j in r], dtype=np.int64).astype(np.int32)
    return rowptr, col


def path_rows(order, forward=True, backward=True):
    """The rows of the path that visits the nodes in `order`: an entry to the next node, to the previous one, or both."""
    n = len(order)
    rows = [[] for _ in range(n)]
    for p in range(n - 1):
        u, v = int(order[p]), int(order[p + 1])
        if forward:
            rows[u].append(v)
        if backward:
            rows[v].append(u)
    return rows


def blobs(seed, sizes, L, apart, sd=1.0):
    """(X float64 [sum sizes, L], blob index [sum sizes]): gaussian blobs of standard deviation `sd` whose centres are `apart`
    from each other along the first axis."""
    rng = np.random.default_rng(seed)
    X = np.concatenate([rng.standard_normal((s, L)) * sd + np.eye(1, L)[0] * apart * b for b, s in enumerate(sizes)])
    return X, np.repeat(np.arange(len(sizes)), sizes)


def knn_lists(X, K):
    """idx int32 [N, K] by float64 direct differences, the row itself excluded, ties by the lower index."""
    from scipy.spatial.distance import cdist
    d = cdist(X, X)
    np.fill_diagonal(d, np.inf)
    return np.argsort(d, axis=1, kind='stable')[:, :K].astype(np.int32)


@functools.lru_cache(maxsize=None)
def graph_case(name):
    """dict(rowptr, col, n, group) of a shape case."""
    rng = np.random.default_rng(len(name) * 7919 + sum(map(ord, name)))
    group = None
    if name == 'one':
        n, rows = 1, [[]]
    elif name == 'two_empty':
        n, rows = 2, [[], []]
    elif name == 'empty':
        n = 300
        rows = [[] for _ in range(n)]
    elif name in ('path_up', 'path_down'):              # the same path, stored towards the larger or towards the smaller id only
        n = 5000
        rows = path_rows(np.arange(n), forward=name == 'path_up', backward=name == 'path_down')
    elif name == 'path_zigzag':                         # 0, n - 1, 1, n - 2, ...
        n = 5000
        order = np.empty(n, np.int64)
        order[0::2], order[1::2] = np.arange(n // 2), n - 1 - np.arange(n // 2)
        rows = path_rows(order)
    elif name == 'path_perm':
        n = 5000
        rows = path_rows(rng.permutation(n))
    elif name in ('star', 'star_out', 'star_in'):       # the hub is node 7: its row holds 5000 entries
        n, hub = 5001, 7
        leaves = [i for i in range(n) if i != hub]
        rows = [[] for _ in range(n)]
        if name != 'star_in':
            rows[hub] = list(leaves)
        if name != 'star_out':
            for i in leaves:
                rows[i] = [hub]
    elif name == 'knn':                                 # lists without mirrors: 4 blobs, 14 neighbours
        X, _ = blobs(3, (700, 600, 400, 300), 6, 40.0)
        idx = knn_lists(X, 14)
        n, rows = len(X), idx.tolist()
    elif name == 'dups':                                # duplicate entries and self loops; 40 rings of 10 nodes
        n = 400
        rows = [[i, (i // 10) * 10 + (i + 1) % 10, (i // 10) * 10 + (i + 1) % 10, i] for i in range(n)]
    elif name == 'outside':                             # columns -1, n and n + 5 are skipped: two halves stay apart
        n = 200
        rows = [[-1, (i + 1) % 100 + 100 * (i // 100), n, n + 5] for i in range(n)]
    elif name in ('n257', 'n65537'):                    # random rows of 0 .. 3 entries; long rows astride the workgroups' 16 rows
        n = int(name[1:])
        lens = rng.integers(0, 4, n)
        for i, length in ((15, 300), (16, 257), (17, 256), (n - 1, 1000)):
            lens[i] = min(length, n)
        rows = [rng.integers(0, n, int(v)).tolist() for v in lens]
        if name == 'n257':
            rows[40], rows[41] = [], []
    elif name == 'group_path':                          # one ascending path, two labels interleaved in runs of 3
        n = 3000
        rows = path_rows(np.arange(n))
        group = ((np.arange(n) // 3) % 2).astype(np.int32)
    else:
        raise KeyError(name)
    rowptr, col = csr_of(rows, n)
    return dict(rowptr=rowptr, col=col, n=n, group=group)

"""Louvain communities of the pooled cells on the MI355X: multi-level modularity optimisation of the fuzzy graph with integer weights,
O(nnz) memory.

    quantise(val), node_class(i), stalled(history)     the integer weights, the class of a node and the stop rule of a level
    modularity_from_tables(inside, tot, two_m, gamma)  Q of a partition from its two int64 tables
    relabel(comm), louvain_summary(...)                cluster ids by descending size; the dict of JAMIE.louvain
    level_graph(graph)                                 a `FuzzyGraph` as the integer level graph (w, k, loop) on the device
    singletons(G), move, apply, sweep                  one class's targets, their application, the 8 sub-sweeps of a sweep
    internal_weights(G, comm), aggregate(G, comm)      in_c, and the next level's graph
    communities(graph), louvain(embeddings, labels)    the whole run on a `FuzzyGraph`; JAMIE.louvain on the device

The kernels are in csrc/louvain.hip (include/jamie_hip.h, "Louvain communities on the device").  The graph is `umap.fuzzy_graph`'s
(`spectral.build_graph`).  The definition (shared with the int64 / float64 host route of jamie.py) is DESIGN.md §23: every sum of
weights is an int64 sum, so the device route equals a numpy restatement element for element and run for run.
"""
import numpy as np
import torch

from . import _native as nv
from .clustering import ari_nmi, check_finite, contingency
from .neighbors import SELF_KNN_MAX, _n_rows, _pool, pooled_codes

WEIGHT_SCALE = 2.0 ** 20       # w = max(1, rint(val * WEIGHT_SCALE))
TWO_M_MAX = 2 ** 52            # every integer a gain converts to fp64 stays exact
NODES_MAX = 2 ** 31
CLASSES = 8                    # sub-sweeps of a sweep
CLASS_MULT = 2654435761
CLASS_SHIFT = 7
PATIENCE = 3
# the bins of jamie_louvain_move (csrc/community_rows.h CR_SHORT_MAX, CR_LONG_MAX): a row of at most SHORT_MAX entries is a wave's,
# one of at most LONG_MAX a workgroup's with its table in LDS, a longer one a workgroup's with its table in the workspace
SHORT_MAX = 64
LONG_MAX = 2048
BINS = ('short', 'long', 'global')


# ---- the argument checks and the definitions both routes share ----
def check_louvain(embeddings, labels=None, resolution=1.0, n_neighbors=15, max_levels=20, max_sweeps=32, tol=1e-7, what='louvain'):
    """The checks of JAMIE.louvain in their order; (resolution, n_neighbors, max_levels, max_sweeps, tol).  Nothing is allocated on
    a device."""
    if len(embeddings) < 1:
        raise ValueError(f'{what}: no embeddings')
    for e in embeddings:
        if len(e.shape) != 2 or e.shape[1] != embeddings[0].shape[1] or e.shape[1] < 1:
            raise ValueError(f'{what}: the embeddings must be [cells, features] with the same features')
    n_cells = [int(e.shape[0]) for e in embeddings]
    N = int(sum(n_cells))
    pooled_codes(n_cells, labels, what)
    resolution = float(resolution)
    if not resolution > 0.0 or not np.isfinite(resolution):
        raise ValueError(f'{what}: resolution = {resolution}; it must be positive and finite')
    nn = int(n_neighbors)
    if nn < 2 or nn > min(N, SELF_KNN_MAX + 1):
        raise ValueError(f'{what}: n_neighbors = {nn}; 2 <= n_neighbors <= min(cells = {N}, {SELF_KNN_MAX + 1})')
    max_levels, max_sweeps, tol = int(max_levels), int(max_sweeps), float(tol)
    if max_levels < 1:
        raise ValueError(f'{what}: max_levels = {max_levels}; at least 1')
    if max_sweeps < 1:
        raise ValueError(f'{what}: max_sweeps = {max_sweeps}; at least 1')
    if not tol >= 0.0:
        raise ValueError(f'{what}: tol = {tol}; at least 0')
    check_finite(embeddings, what)
    return resolution, nn, max_levels, max_sweeps, tol


def check_totals(n, two_m, what='louvain'):
    """Refuses a graph without weight, two_m >= 2^52 and n >= 2^31."""
    if n < 1 or n >= NODES_MAX:
        raise ValueError(f'{what}: {n} nodes; 1 <= nodes < 2^31')
    if two_m < 1 or two_m >= TWO_M_MAX:
        raise ValueError(f'{what}: the weights sum to {two_m}; 1 <= two_m < 2^52')


def quantise(val):
    """w = max(1, rint(val * 2^20)) as int64: the product in float64 (exact for fp32 values), round half to even."""
    return np.maximum(np.rint(np.asarray(val, dtype=np.float64) * WEIGHT_SCALE), 1.0).astype(np.int64)


def node_class(i):
    """The class ((uint64)i * 2654435761 >> 7) & 7 of node i (an int or an array of node ids below 2^31)."""
    v = (np.asarray(i).astype(np.uint64) * np.uint64(CLASS_MULT)) >> np.uint64(CLASS_SHIFT)
    return (v & np.uint64(CLASSES - 1)).astype(np.int64)


def stalled(history, patience=PATIENCE):
    """True when the smallest moved count of the level (the first one on ties) is `patience` or more sweeps old."""
    return len(history) > 0 and len(history) - 1 - int(np.argmin(history)) >= patience


def modularity_from_tables(inside, tot, two_m, gamma):
    """Q = sum_c (in_c / two_m - gamma (tot_c / two_m)^2) from the int64 tables, added in ascending community id in float64."""
    m2 = float(int(two_m))
    inside, tot = np.asarray(inside, dtype=np.int64), np.asarray(tot, dtype=np.int64)
    terms = inside.astype(np.float64) / m2 - float(gamma) * ((tot.astype(np.float64) / m2) * (tot.astype(np.float64) / m2))
    return float(np.cumsum(terms)[-1]) if len(terms) else 0.0      # (cumsum adds one term after the other)


def relabel(comm):
    """(clusters int32 [N], sizes int64): ids 0 .. by descending size, ties by the smallest member cell."""
    comm = np.asarray(comm, dtype=np.int64)
    ids, first, counts = np.unique(comm, return_index=True, return_counts=True)
    order = np.lexsort((first, -counts))
    new = np.empty(len(ids), dtype=np.int64)
    new[order] = np.arange(len(ids))
    return new[np.searchsorted(ids, comm)].astype(np.int32), counts[order].astype(np.int64)


def louvain_summary(clusters, sizes, modularity, levels, n_cells, table_mod, table_lab, classes, resolution, n_neighbors, n_edges,
                    graph):
    """The dict of JAMIE.louvain (shared by the device and the host route)."""
    cuts = np.cumsum(n_cells)[:-1]
    ari, nmi = ari_nmi(table_lab) if table_lab is not None else (None, None)
    return {'clusters': np.split(np.asarray(clusters, dtype=np.int32), cuts), 'n_clusters': int(len(sizes)),
            'sizes': np.asarray(sizes, dtype=np.int64), 'modularity': float(modularity), 'levels': levels,
            'modality_contingency': np.asarray(table_mod, dtype=np.int64), 'ari': ari, 'nmi': nmi,
            'contingency': None if table_lab is None else np.asarray(table_lab, dtype=np.int64), 'labels': classes,
            'resolution': float(resolution), 'n_neighbors': int(n_neighbors), 'n_edges': int(n_edges), 'graph': graph}


def level_record(nodes, communities, history, modularity, two_m):
    return {'nodes': int(nodes), 'communities': int(communities), 'sweeps': len(history), 'moved': [int(m) for m in history],
            'modularity': float(modularity), 'two_m': int(two_m)}


def host_tables(clusters, n_cells, labels, k):
    """(cluster x modality, cluster x label or None, classes) as exact integer tables in numpy."""
    mod, lcode, classes = pooled_codes(n_cells, labels, 'louvain')
    table_mod = np.zeros((k, len(n_cells)), np.int64)
    np.add.at(table_mod, (clusters, mod), 1)
    table_lab = None
    if lcode is not None:
        table_lab = np.zeros((k, len(classes)), np.int64)
        np.add.at(table_lab, (clusters, lcode), 1)
    return table_mod, table_lab, classes


def table_slots(length):
    """Slots of the workspace table of a row of `length` entries: the power of two from 2 length + 2 up (csrc/community_rows.h)."""
    s = 2
    while s < 2 * int(length) + 2:
        s *= 2
    return s


# ---- the device route ----
class LevelGraph:
    """An integer level graph on the device: rowptr int64 [n + 1], col int32 [nnz], w int64 [nnz], loop int64 [n], k int64 [n]
    (k_i = the row's weights + loop_i) and two_m = sum k.  Rows never store the diagonal."""

    def __init__(self, rowptr, col, w, loop, k=None):
        self.rowptr, self.col, self.w, self.loop = rowptr, col, w, loop
        self.n = int(loop.numel())
        if rowptr.dtype != torch.int64 or col.dtype != torch.int32 or w.dtype != torch.int64 or loop.dtype != torch.int64:
            raise ValueError('louvain: a level graph is (rowptr int64, col int32, w int64, loop int64)')
        if rowptr.numel() != self.n + 1 or col.numel() != w.numel():
            raise ValueError('louvain: rowptr must be [nodes + 1] and col, w of one length')
        for t in (rowptr, col, w, loop):
            if not t.is_contiguous():
                raise ValueError('louvain: a level graph holds contiguous tensors')
        lens = rowptr[1:] - rowptr[:-1]
        if int(rowptr[0]) != 0 or int(rowptr[-1]) != col.numel() or (self.n and int(lens.min()) < 0):
            raise ValueError('louvain: rowptr must ascend from 0 to the number of entries')
        if col.numel() and (int(col.min()) < 0 or int(col.max()) >= self.n):
            raise ValueError(f'louvain: the graph has a column outside [0, {self.n})')
        if (col.numel() and int(w.min()) < 1) or (self.n and int(loop.min()) < 0):
            raise ValueError('louvain: weights are at least 1 and loops at least 0')
        self.lens = lens
        if k is None:
            row = torch.repeat_interleave(torch.arange(self.n, device=col.device), lens)
            k = loop.clone().index_add_(0, row, w)
        self.k = k
        self.two_m = int(k.sum().item())
        self._plan = None

    @classmethod
    def from_numpy(cls, rowptr, col, w, loop, device='cuda'):
        t = torch.as_tensor
        return cls(t(np.asarray(rowptr, np.int64)).to(device), t(np.asarray(col, np.int32)).to(device),
                   t(np.asarray(w, np.int64)).to(device), t(np.asarray(loop, np.int64)).to(device))

    def plan(self):
        """The node lists of the 8 classes, each ordered short rows, long rows, rows beyond the LDS cap (ascending id within a
        bin); per class the three counts, the slot offsets of its workspace tables and the bytes they need."""
        if self._plan is None:
            dev = self.col.device
            ids = torch.arange(self.n, dtype=torch.int64, device=dev)
            cls = ((ids * CLASS_MULT) >> CLASS_SHIFT) & (CLASSES - 1)          # (ids < 2^31: the product stays below 2^63)
            bins = (self.lens > SHORT_MAX).long() + (self.lens > LONG_MAX).long()
            key = cls * 3 + bins
            order = torch.sort(key, stable=True)[1]
            counts = torch.bincount(key, minlength=3 * CLASSES).cpu().numpy().reshape(CLASSES, 3)
            nodes = order.to(torch.int32).contiguous()
            starts = np.concatenate([[0], np.cumsum(counts.reshape(-1))]).reshape(-1)
            slot_off, ws_bytes = [], 0
            for s in range(CLASSES):
                g0, g1 = int(starts[3 * s + 2]), int(starts[3 * s + 3])
                if g1 > g0:
                    lens = self.lens[order[g0:g1]].cpu().numpy()
                    off = np.concatenate([[0], np.cumsum([table_slots(v) for v in lens])]).astype(np.int64)
                    ws_bytes = max(ws_bytes, nv.louvain_workspace(lens))
                    slot_off.append(torch.from_numpy(off).to(dev))
                else:
                    slot_off.append(None)
            ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
            self._plan = dict(nodes=nodes, counts=counts, starts=starts, slot_off=slot_off, ws=ws)
        return self._plan

    def of_class(self, cls):
        """What a launch over the nodes of class `cls` takes from the plan: (its node list in bin order, its (short, long, global)
        counts, the slot offsets of its workspace tables or None, the workspace)."""
        p = self.plan()
        counts = tuple(int(c) for c in p['counts'][cls])
        first = int(p['starts'][3 * cls])
        return p['nodes'][first:first + sum(counts)], counts, p['slot_off'][cls], p['ws']


class State:
    """comm int32 [n], tot int64 [n], size int32 [n] of a level on the device, and the targets of the last `move`."""

    def __init__(self, comm, tot, size):
        self.comm, self.tot, self.size = comm, tot, size
        self.target = comm.clone()
        self.moved = torch.zeros(1, dtype=torch.int64, device=comm.device)
        self.flag = torch.zeros(1, dtype=torch.int32, device=comm.device)


def level_graph(graph):
    """The level-0 graph of a `FuzzyGraph` (or any CSR with fp32 values on the device): w and k by jamie_louvain_quantise, loops 0."""
    nv.require_gpu()
    n, nnz = graph.n, int(graph.col.numel())
    dev = graph.col.device
    w = torch.empty(nnz, dtype=torch.int64, device=dev)
    k = torch.empty(n, dtype=torch.int64, device=dev)
    nv.louvain_quantise(graph.rowptr, graph.val, w, k)
    return LevelGraph(graph.rowptr, graph.col, w, torch.zeros(n, dtype=torch.int64, device=dev), k)


def singletons(G):
    dev = G.col.device
    return State(torch.arange(G.n, dtype=torch.int32, device=dev), G.k.clone(), torch.ones(G.n, dtype=torch.int32, device=dev))


def state_of(G, comm):
    """The state of the partition `comm` (numpy or tensor, ids in [0, n)): tot and size by integer sums."""
    dev = G.col.device
    comm = torch.as_tensor(np.asarray(comm) if not torch.is_tensor(comm) else comm).to(dev, torch.int32).contiguous()
    if comm.numel() != G.n or (G.n and (int(comm.min()) < 0 or int(comm.max()) >= G.n)):
        raise ValueError(f'louvain: one community in [0, {G.n}) per node is needed')
    tot = torch.zeros(G.n, dtype=torch.int64, device=dev).index_add_(0, comm.long(), G.k)
    size = torch.bincount(comm.long(), minlength=G.n).to(torch.int32)
    return State(comm, tot, size)


def move(G, state, cls, gamma=1.0):
    """The targets of the nodes of class `cls` from the state as it stands, into state.target (the other classes' entries are left
    alone); the (short, long, global) row counts the launch took."""
    nv.require_gpu()
    nodes, counts, slot_off, ws = G.of_class(cls)
    if sum(counts):
        nv.louvain_move(G.rowptr, G.col, G.w, G.k, state.comm, state.tot, state.size, float(gamma), G.two_m, nodes, counts, slot_off,
                        ws, state.target, state.flag)
    return counts


def apply(G, state, cls):
    """Applies state.target to the nodes of class `cls`: comm, tot, size by integer atomics; state.moved grows by the moves."""
    nv.require_gpu()
    nodes = G.of_class(cls)[0]
    if nodes.numel():
        nv.louvain_apply(nodes, state.target, G.k, state.comm, state.tot, state.size, state.moved)


def sweep(G, state, gamma=1.0):
    """The 8 sub-sweeps of one sweep; the nodes moved."""
    state.moved.zero_()
    for s in range(CLASSES):
        move(G, state, s, gamma)
        apply(G, state, s)
    if int(state.flag.item()):
        raise RuntimeError('louvain: a row did not fit the bin its node list put it in')
    return int(state.moved.item())


def internal_weights(G, comm):
    """in_c int64 [n]: the weights of the stored entries with both ends in c, plus the loops."""
    nv.require_gpu()
    out = torch.empty(G.n, dtype=torch.int64, device=G.col.device)
    nv.louvain_internal(G.rowptr, G.col, G.w, G.loop, comm, out)
    return out


def aggregate(G, comm):
    """(the next level's graph, new id int64 [n] of every node): communities renumbered in ascending id, a coarse row one entry
    per distinct other community with ascending columns and summed w, loop = the loops plus the inside entries.  Integer plumbing
    on O(nnz) keys: a sort, `unique_consecutive`, int64 `index_add_`."""
    dev = G.col.device
    c = comm.long()
    present = torch.zeros(G.n, dtype=torch.int64, device=dev)
    present[c] = 1
    new = torch.cumsum(present, 0) - 1
    nc = int(present.sum().item())
    cmap = new[c]
    row = torch.repeat_interleave(cmap, G.lens)
    other = cmap[G.col.long()]
    inside = row == other
    loop = torch.zeros(nc, dtype=torch.int64, device=dev).index_add_(0, cmap, G.loop)
    loop.index_add_(0, row[inside], G.w[inside])
    keys, perm = torch.sort((row * nc + other)[~inside])
    ukeys, inverse = torch.unique_consecutive(keys, return_inverse=True)
    w = torch.zeros(ukeys.numel(), dtype=torch.int64, device=dev).index_add_(0, inverse, G.w[~inside][perm])
    rowptr = torch.zeros(nc + 1, dtype=torch.int64, device=dev)
    urow = torch.div(ukeys, nc, rounding_mode='floor')
    rowptr[1:] = torch.cumsum(torch.bincount(urow, minlength=nc), 0)
    col = (ukeys - urow * nc).to(torch.int32)
    return LevelGraph(rowptr, col.contiguous(), w, loop), cmap


def run_level(G, gamma, max_sweeps, comm0=None):
    """The sweeps of one level from the partition comm0 (None: singletons) until nothing moves or the run stalls: (state, the moved
    history)."""
    state = singletons(G) if comm0 is None else state_of(G, comm0)
    history = []
    for _ in range(max_sweeps):
        history.append(sweep(G, state, gamma))
        if history[-1] == 0 or stalled(history):
            break
    return state, history


def communities_of_level_graph(G, resolution=1.0, max_levels=20, max_sweeps=32, tol=1e-7):
    """The run of DESIGN.md §23 on an integer level graph: dict(comm int64 numpy [n]: the composed map of the accepted levels,
    modularity, levels)."""
    check_totals(G.n, G.two_m)
    two_m = G.two_m
    q_prev = modularity_from_tables(G.loop.cpu().numpy(), G.k.cpu().numpy(), two_m, resolution)
    comm = torch.arange(G.n, dtype=torch.int64, device=G.col.device)
    levels = []
    while len(levels) < max_levels:
        state, history = run_level(G, resolution, max_sweeps)
        inside = internal_weights(G, state.comm)
        q = modularity_from_tables(inside.cpu().numpy(), state.tot.cpu().numpy(), two_m, resolution)
        if not q > q_prev + tol:
            break
        nxt, cmap = aggregate(G, state.comm)
        levels.append(level_record(G.n, nxt.n, history, q, nxt.two_m))
        comm = cmap[comm]
        G, q_prev = nxt, q
    return dict(comm=comm.cpu().numpy(), modularity=q_prev, levels=levels)


def communities(graph, resolution=1.0, max_levels=20, max_sweeps=32, tol=1e-7):
    """Louvain communities of a `FuzzyGraph`: dict(clusters int32 [N], sizes, modularity, levels).  Bit-identical from run to
    run."""
    out = communities_of_level_graph(level_graph(graph), resolution, max_levels, max_sweeps, tol)
    clusters, sizes = relabel(out['comm'])
    return dict(clusters=clusters, sizes=sizes, modularity=out['modularity'], levels=out['levels'])


def louvain(embeddings, labels=None, resolution=1.0, n_neighbors=15, max_levels=20, max_sweeps=32, tol=1e-7, return_graph=False,
            device='cuda'):
    """Louvain communities of M embeddings [N_m, L] pooled into one set of cells:

        clusters                    one int32 array per embedding: ids 0 .. by descending size
        n_clusters, sizes           int64 [n_clusters]
        modularity                  Q of the result on the integer graph at `resolution`
        levels                      per accepted level: nodes, communities, sweeps, moved (per sweep), modularity, two_m
        modality_contingency        int64 [n_clusters, M]
        ari, nmi, contingency, labels                as JAMIE.test_clustering (None without labels)
        n_neighbors, n_edges, graph                  as JAMIE.umap

    Bit-identical from run to run."""
    checked = check_louvain(embeddings, labels, resolution, n_neighbors, max_levels, max_sweeps, tol, 'louvain')
    return louvain_checked(embeddings, labels, *checked, return_graph, device)


def louvain_checked(embeddings, labels, resolution, n_neighbors, max_levels, max_sweeps, tol, return_graph=False, device='cuda'):
    """`louvain` behind its argument checks: the arguments are what `check_louvain` returned."""
    return pooled_run('louvain', communities, run_summary, embeddings, labels, resolution, n_neighbors, max_levels, max_sweeps, tol,
                      return_graph, device)


def run_summary(out, *rest):
    """`louvain_summary` of the dict of `communities`."""
    return louvain_summary(out['clusters'], out['sizes'], out['modularity'], out['levels'], *rest)


def pooled_run(what, run, summary, embeddings, labels, resolution, n_neighbors, max_levels, max_sweeps, tol, return_graph, device):
    """The front end of `louvain` and `leiden.leiden`: the pooled cells, their fuzzy graph, `run` (a `communities`) on it, the two
    contingency tables of its clusters and `summary` of it all."""
    from .spectral import build_graph
    n_cells = [_n_rows(e) for e in embeddings]
    mod, lcode, classes = pooled_codes(n_cells, labels, what)
    xs, x = _pool(embeddings, device, what)
    G = build_graph(x, n_neighbors, device)
    out = run(G, resolution, max_levels, max_sweeps, tol)
    k = len(out['sizes'])
    table_mod = contingency(out['clusters'], mod, k, len(xs), device=x.device)
    table_lab = None if lcode is None else contingency(out['clusters'], lcode, k, len(classes), device=x.device)
    graph = G.to_scipy() if return_graph else None
    return summary(out, n_cells, table_mod, table_lab, classes, resolution, n_neighbors, G.col.numel(), graph)

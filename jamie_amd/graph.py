"""Graph structure of the pooled cells on the MI355X: connected components of the fuzzy graph, scIB's graph connectivity of the
labels and kBET's rejection rate of the modalities, from ONE neighbour search, O(nnz) memory.

    check_graph_metrics(...)                           the argument checks of JAMIE.test_graph
    host_rounds(rowptr, col, n, group)                 the synchronous rounds in numpy: (root, rounds, jumps)
    component_tables(label, n_cells, lcode)            component ids by descending size, their sizes and tables
    label_connectivity(glabel, lcode, T)               per label: the largest component's share and the component count
    expected_rows(mod, M, lcode, T, expected)          the expected modality shares of kBET and the row a cell uses
    kbet_decisions(stat, df, alpha)                    p-values (scipy's chdtrc on the host) and the rejected cells
    graph_summary(...)                                 the dict of JAMIE.test_graph
    lists_as_csr(idx), components(graph, group)        neighbour lists as a CSR graph; the components on the device
    graph_connectivity(graph, lcode, T)                one `components` run with group = the label
    kbet_from_neighbors(idx, codes, expected, ...)     the per-cell statistic on the device
    graph_metrics(embeddings, labels, ...)             JAMIE.test_graph on the device

The kernels are in csrc/graph.hip (include/jamie_hip.h, "Graph structure on the device").  The graph is `umap.fuzzy_graph`'s
(`spectral.build_graph`).  The definition (shared with the scipy / numpy host route of jamie.py) is DESIGN.md §26: the components
are integers, the kBET statistic is fp64 in one fixed order, so the device route equals a numpy restatement element for element and
run for run.
"""
import numpy as np
import torch

from . import _native as nv
from .clustering import check_finite
from .louvain import NODES_MAX, relabel
from .neighbors import SELF_KNN_MAX, _n_rows, _pool, pooled_codes, self_knn

KBET_K_MAX = 128               # neighbours of one jamie_kbet_stat call
KBET_B_MAX = 64                # categories of one jamie_kbet_stat call
EXPECTED = ('global', 'label')
FLAGS_PER_READ = 8             # launches (a hook and jumps, or jumps) that share one host read of their flags


# ---- the argument checks and the definitions both routes share ----
def check_graph_metrics(embeddings, labels=None, n_neighbors=15, alpha=0.05, expected='global', what='test_graph'):
    """The checks of JAMIE.test_graph in their order; (n_neighbors, alpha, expected).  Nothing is allocated on a device."""
    if len(embeddings) < 1:
        raise ValueError(f'{what}: no embeddings')
    for e in embeddings:
        if len(e.shape) != 2 or e.shape[1] != embeddings[0].shape[1] or e.shape[1] < 1:
            raise ValueError(f'{what}: the embeddings must be [cells, features] with the same features')
    n_cells = [int(e.shape[0]) for e in embeddings]
    N = int(sum(n_cells))
    pooled_codes(n_cells, labels, what)
    nn = int(n_neighbors)
    if nn < 2 or nn > min(N, SELF_KNN_MAX + 1):
        raise ValueError(f'{what}: n_neighbors = {nn}; 2 <= n_neighbors <= min(cells = {N}, {SELF_KNN_MAX + 1})')
    alpha = float(alpha)
    if not 0.0 < alpha < 1.0:
        raise ValueError(f'{what}: alpha = {alpha}; 0 < alpha < 1')
    if expected not in EXPECTED:
        raise ValueError(f'{what}: expected = {expected!r}; one of {EXPECTED}')
    if expected == 'label' and labels is None:
        raise ValueError(f"{what}: expected = 'label' needs labels")
    if len(embeddings) > KBET_B_MAX:
        raise ValueError(f'{what}: {len(embeddings)} embeddings; kBET takes at most {KBET_B_MAX} modalities')
    check_finite(embeddings, what)
    return nn, alpha, expected


def host_rounds(rowptr, col, n, group=None, trace=None):
    """The rounds of DESIGN.md §26 in numpy: (root int32 [n], rounds, jumps).  A round copies root to parent, hooks every entry
    that counts with `np.minimum.at`, and jumps parent = parent[parent] until a pass changes nothing; the run ends with the first
    round whose hook finds nothing.  `jumps` counts every pass up to and including a round's first idle one.  `trace`: a list that
    receives ('hook', parent) and ('root', root) copies in order."""
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    n = int(n)
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    keep = (col >= 0) & (col < n) & (col != row)
    row, col = row[keep], col[keep]
    if group is not None:
        group = np.asarray(group)
        keep = group[row] == group[col]
        row, col = row[keep], col[keep]
    root = np.arange(n, dtype=np.int32)
    rounds = jumps = 0
    while True:
        rounds += 1
        a, b = root[row], root[col]
        differ = a != b
        parent = root.copy()
        np.minimum.at(parent, np.maximum(a, b)[differ], np.minimum(a, b)[differ])
        if trace is not None:
            trace.append(('hook', parent.copy()))
        if not differ.any():
            return root, rounds, jumps
        while True:
            nxt = parent[parent]
            jumps += 1
            idle = np.array_equal(nxt, parent)
            parent = nxt
            if idle:
                break
        root = parent
        if trace is not None:
            trace.append(('root', root.copy()))


def component_tables(label, n_cells, lcode=None):
    """(component int32 [N]: ids 0 .. by descending size, ties by the smallest member cell; sizes int64; the component x modality
    table int64; the component x label table or None) of the root labels `label` of the pooled cells."""
    label = label.cpu().numpy() if torch.is_tensor(label) else np.asarray(label)
    comp, sizes = relabel(label)
    mod = np.repeat(np.arange(len(n_cells), dtype=np.int64), n_cells)
    table_mod = np.zeros((len(sizes), len(n_cells)), np.int64)
    np.add.at(table_mod, (comp, mod), 1)
    table_lab = None
    if lcode is not None:
        table_lab = np.zeros((len(sizes), int(np.max(lcode)) + 1), np.int64)
        np.add.at(table_lab, (comp, np.asarray(lcode)), 1)
    return comp, sizes, table_mod, table_lab


def label_connectivity(glabel, lcode, T):
    """(share float64 [T], count int64 [T]) from the component roots `glabel` of the graph cut between labels: per label t the
    largest component among its cells over their number, and how many components they form.  NaN and 0 for a label without cells."""
    glabel = glabel.cpu().numpy() if torch.is_tensor(glabel) else np.asarray(glabel)
    lcode = np.asarray(lcode)
    share, count = np.full(T, np.nan), np.zeros(T, np.int64)
    for t in range(T):
        cells = glabel[lcode == t]
        if len(cells):
            sizes = np.unique(cells, return_counts=True)[1]
            share[t], count[t] = float(sizes.max()) / float(len(cells)), len(sizes)
    return share, count


def expected_rows(mod, M, lcode, T, expected):
    """(shares float64 [n_e, M], erow int64 [N] or None) of kBET: 'global': one row, the modality shares of the pooled cells;
    'label': one row per label, the shares among the cells of that label, and erow = the cell's label code."""
    mod = np.asarray(mod, dtype=np.int64)
    if expected == 'global':
        counts = np.bincount(mod, minlength=M).astype(np.float64)[None, :]
        erow = None
    else:
        erow = np.asarray(lcode, dtype=np.int64)
        counts = np.zeros((T, M), np.float64)
        np.add.at(counts, (erow, mod), 1.0)
    return counts / counts.sum(axis=1, keepdims=True), erow


def kbet_decisions(stat, df, alpha):
    """(pvalues float64 [N], NaN where the cell is not tested; rejected bool [N]): the upper tail of chi-square(df) at stat."""
    from scipy.special import chdtrc
    stat, df = np.asarray(stat, dtype=np.float64), np.asarray(df)
    p = np.full(stat.shape, np.nan)
    tested = (df >= 1) & ~np.isnan(stat)
    p[tested] = chdtrc(df[tested].astype(np.float64), stat[tested])
    return p, tested & (p < alpha)


def graph_summary(label, rounds, jumps, n_cells, lcode, classes, label_share, label_count, kbet, n_neighbors, n_edges, alpha,
                  expected, graph):
    """The dict of JAMIE.test_graph (shared by the device and the host route).  `label`: the smallest cell of every cell's
    component; `kbet`: dict(stat, df) of the pooled cells, or None for a single embedding."""
    cuts = np.cumsum(n_cells)[:-1]
    comp, sizes, table_mod, table_lab = component_tables(label, n_cells, lcode)
    out = {'components': np.split(comp, cuts), 'n_components': int(len(sizes)), 'component_sizes': sizes,
           'largest_share': float(sizes[0]) / float(len(comp)), 'modality_contingency': table_mod, 'label_contingency': table_lab,
           'rounds': int(rounds), 'jumps': int(jumps),
           'graph_connectivity': None, 'label_connectivity': None, 'label_components': None, 'labels': classes,
           'kbet_rejection': None, 'kbet_acceptance': None, 'kbet_pvalues': None, 'kbet_stat': None, 'kbet_tested': None,
           'label_kbet_rejection': None,
           'n_neighbors': int(n_neighbors), 'n_edges': int(n_edges), 'alpha': float(alpha), 'expected': expected, 'graph': graph}
    if lcode is not None:
        present = ~np.isnan(label_share)
        out['graph_connectivity'] = float(np.mean(label_share[present]))
        out['label_connectivity'], out['label_components'] = label_share, label_count
    if kbet is not None:
        stat = np.asarray(kbet['stat'], dtype=np.float64)
        p, rejected = kbet_decisions(stat, kbet['df'], alpha)
        tested = ~np.isnan(p)
        n_tested = int(tested.sum())
        out['kbet_rejection'] = float(rejected.sum()) / n_tested if n_tested else float('nan')
        out['kbet_acceptance'] = 1.0 - out['kbet_rejection']
        out['kbet_pvalues'], out['kbet_stat'], out['kbet_tested'] = np.split(p, cuts), np.split(stat, cuts), n_tested
        if lcode is not None:
            T = len(classes)
            rej = np.bincount(lcode[tested], weights=rejected[tested].astype(np.float64), minlength=T)
            cnt = np.bincount(lcode[tested], minlength=T).astype(np.float64)
            out['label_kbet_rejection'] = np.where(cnt > 0, rej / np.maximum(cnt, 1.0), np.nan)
    return out


# ---- the device route ----
class ListGraph:
    """Neighbour lists idx int32 [N, K] on the device as a CSR graph: row i holds idx[i, :]."""

    def __init__(self, idx):
        if len(idx.shape) != 2 or idx.dtype != torch.int32:
            raise ValueError('graph: neighbour lists are int32 [cells, k]')
        self.n, self.k = int(idx.shape[0]), int(idx.shape[1])
        self.col = idx.contiguous().view(-1)
        self.rowptr = torch.arange(self.n + 1, dtype=torch.int64, device=idx.device) * self.k


def lists_as_csr(idx):
    nv.require_gpu()
    return ListGraph(torch.as_tensor(idx).to('cuda', torch.int32))


def _graph_arrays(graph, group, what):
    n = int(graph.n)
    rowptr, col = graph.rowptr, graph.col
    if rowptr.dtype != torch.int64 or col.dtype != torch.int32 or not rowptr.is_cuda or not col.is_cuda:
        raise ValueError(f'{what}: a graph is (rowptr int64, col int32) on the device')
    if n < 1 or n >= NODES_MAX or rowptr.numel() != n + 1:
        raise ValueError(f'{what}: {n} nodes with rowptr of {rowptr.numel()}; 1 <= nodes < 2^31 and rowptr [nodes + 1]')
    if not rowptr.is_contiguous() or not col.is_contiguous():
        raise ValueError(f'{what}: a graph holds contiguous tensors')
    if group is not None:
        group = torch.as_tensor(np.asarray(group) if not torch.is_tensor(group) else group).to(col.device, torch.int32).contiguous()
        if group.numel() != n:
            raise ValueError(f'{what}: one group per node, got {group.numel()} for {n} nodes')
    return n, rowptr, col, group


def components(graph, group=None, max_rounds=64, trace=None):
    """The connected components of a `FuzzyGraph` (or anything with rowptr int64, col int32 and n on the device: `lists_as_csr`
    for neighbour lists) by the rounds of DESIGN.md §26: (label int32 device tensor [n]: the smallest node of every node's
    component, rounds, jumps).  An entry links both ways (weak connectivity); with `group` (integers [n]) only entries inside a
    group count.  `rounds` counts the round that finds nothing, `jumps` every pass up to and including a round's first idle one.
    `trace`: a list that receives ('hook', parent) and ('root', root) clones in order.  RuntimeError when `max_rounds` rounds do
    not reach the fixed point.  Bit-identical from run to run."""
    nv.require_gpu()
    n, rowptr, col, group = _graph_arrays(graph, group, 'components')
    dev = col.device
    root = torch.arange(n, dtype=torch.int32, device=dev)
    parent, spare = torch.empty_like(root), torch.empty_like(root)
    flags = torch.zeros(FLAGS_PER_READ, dtype=torch.int32, device=dev)
    rounds = jumps = 0
    for _ in range(int(max_rounds)):
        rounds += 1
        parent.copy_(root)
        flags.zero_()
        nv.graph_hook(rowptr, col, group, root, parent, flags[0:1])
        if trace is not None:
            trace.append(('hook', parent.clone()))
        first, idle = 1, False
        while not idle:
            # (a jump launched after the fixed point, or after a hook that found nothing, changes nothing)
            for f in range(first, FLAGS_PER_READ):
                nv.graph_jump(parent, spare, flags[f:f + 1])
                parent, spare = spare, parent
            seen = flags.cpu().numpy()
            if first == 1 and not seen[0]:
                return root, rounds, jumps
            for f in range(first, FLAGS_PER_READ):
                jumps += 1
                if not seen[f]:
                    idle = True
                    break
            first = 0
            flags.zero_()
        root, parent = parent, root
        if trace is not None:
            trace.append(('root', root.clone()))
    raise RuntimeError(f'components: no fixed point within max_rounds = {int(max_rounds)} rounds')


def graph_connectivity(graph, lcode, T):
    """scIB's graph connectivity on `graph` from ONE `components` run with group = the label code: dict(score: the mean over the
    labels present of the share of a label's cells in its largest component; share [T]; count [T]: components per label; rounds,
    jumps)."""
    glabel, rounds, jumps = components(graph, group=lcode)
    share, count = label_connectivity(glabel, lcode, T)
    return dict(score=float(np.mean(share[~np.isnan(share)])), share=share, count=count, rounds=rounds, jumps=jumps)


def kbet_from_neighbors(idx, codes, expected, erow=None, alpha=0.05, return_counts=False):
    """kBET's test of every cell from its neighbour lists (idx int32 [N, K <= 128], device tensor or numpy) under the categories
    `codes` (integers [N] in [0, B)) and the expected shares `expected` (float64 [n_e, B <= 64]; cell i uses row erow[i], row 0
    without `erow`): dict(stat, df, pvalues (NaN where the cell is not tested), rejected, and counts int32 [N, B] with
    `return_counts`) in numpy."""
    nv.require_gpu()
    expected = np.ascontiguousarray(expected, dtype=np.float64)
    expected = expected.reshape(1, -1) if expected.ndim == 1 else expected
    if len(idx.shape) != 2 or not 1 <= idx.shape[1] <= KBET_K_MAX or idx.shape[0] < 1:
        raise ValueError(f'kbet_from_neighbors: idx must be [cells, 1 <= k <= {KBET_K_MAX}], got {tuple(idx.shape)}')
    N = int(idx.shape[0])
    if expected.ndim != 2 or not 1 <= expected.shape[1] <= KBET_B_MAX or expected.shape[0] < 1:
        raise ValueError(f'kbet_from_neighbors: expected must be [rows, 1 <= categories <= {KBET_B_MAX}], got {expected.shape}')
    codes = np.asarray(codes.cpu() if torch.is_tensor(codes) else codes).reshape(-1)
    if codes.shape[0] != N:
        raise ValueError(f'kbet_from_neighbors: one code per cell, got {codes.shape[0]} for {N} cells')
    if erow is not None:
        erow = np.asarray(erow).reshape(-1)
        if erow.shape[0] != N or (N and (erow.min() < 0 or erow.max() >= expected.shape[0])):
            raise ValueError(f'kbet_from_neighbors: erow must hold one row of `expected` in [0, {expected.shape[0]}) per cell')
    alpha = float(alpha)
    if not 0.0 < alpha < 1.0:
        raise ValueError(f'kbet_from_neighbors: alpha = {alpha}; 0 < alpha < 1')
    idx_d = torch.as_tensor(idx).to('cuda', torch.int32).contiguous()
    dev = idx_d.device
    codes_d = torch.from_numpy(np.ascontiguousarray(codes, dtype=np.int32)).to(dev)
    exp_d = torch.from_numpy(expected).to(dev)
    erow_d = None if erow is None else torch.from_numpy(np.ascontiguousarray(erow, dtype=np.int32)).to(dev)
    stat = torch.empty(N, dtype=torch.float64, device=dev)
    df = torch.empty(N, dtype=torch.int32, device=dev)
    counts = torch.empty(N, expected.shape[1], dtype=torch.int32, device=dev) if return_counts else None
    nv.kbet_stat(idx_d, codes_d, exp_d, erow_d, stat, df, counts)
    out = dict(stat=stat.cpu().numpy(), df=df.cpu().numpy())
    out['pvalues'], out['rejected'] = kbet_decisions(out['stat'], out['df'], alpha)
    if return_counts:
        out['counts'] = counts.cpu().numpy()
    return out


def graph_metrics(embeddings, labels=None, n_neighbors=15, alpha=0.05, expected='global', return_graph=False, device='cuda'):
    """Connected components, graph connectivity and kBET of M embeddings [N_m, L] pooled into one set of cells,
    from ONE neighbour search:

        components                  one int32 array per embedding: ids 0 .. by descending size
        n_components, component_sizes, largest_share, modality_contingency [components, M], label_contingency, rounds, jumps
        graph_connectivity          the mean over labels of label_connectivity [T]: the share of a label's cells in the largest
                                    component of the graph cut down to that label; label_components [T]; labels (None without)
        kbet_rejection              the share of tested cells whose neighbours' modalities differ from the expected shares at
                                    level alpha (chi-square); kbet_acceptance = 1 - it; kbet_pvalues, kbet_stat per embedding;
                                    kbet_tested; label_kbet_rejection [T]; each None for a single embedding
        n_neighbors, n_edges, alpha, expected, graph                  `graph` as JAMIE.umap

    Bit-identical from run to run."""
    checked = check_graph_metrics(embeddings, labels, n_neighbors, alpha, expected, 'graph_metrics')
    return graph_metrics_checked(embeddings, labels, *checked, return_graph, device)


def graph_metrics_checked(embeddings, labels, n_neighbors, alpha, expected, return_graph=False, device='cuda'):
    """`graph_metrics` behind its argument checks: the arguments are what `check_graph_metrics` returned."""
    from . import umap as jum
    n_cells = [_n_rows(e) for e in embeddings]
    mod, lcode, classes = pooled_codes(n_cells, labels, 'graph_metrics')
    xs, x = _pool(embeddings, device, 'graph_metrics')
    idx, dist = self_knn(x, n_neighbors - 1, device)            # (the graph exactly as `spectral.build_graph` builds it)
    W, _, _, _ = jum.smooth_knn(idx, dist, n_neighbors)
    del dist
    G = jum.fuzzy_graph(idx, W)
    label, rounds, jumps = components(G)
    share = count = None
    if lcode is not None:
        conn = graph_connectivity(G, lcode, len(classes))
        share, count = conn['share'], conn['count']
    kbet = None
    if len(xs) > 1:
        shares, erow = expected_rows(mod, len(xs), lcode, None if classes is None else len(classes), expected)
        kbet = kbet_from_neighbors(idx, mod, shares, erow, alpha)
    graph = G.to_scipy() if return_graph else None
    return graph_summary(label, rounds, jumps, n_cells, lcode, classes, share, count, kbet, n_neighbors, G.col.numel(), alpha,
                         expected, graph)

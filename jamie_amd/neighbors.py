"""Neighbourhoods of the pooled cells on the MI355X: the self k-nearest-neighbour search, LISI and the kNN graph, without an N x N
matrix.

    self_knn(X, k)                                 the k nearest OTHER rows of X, as (idx, dist) [N, k]; k <= 128
    lisi_from_neighbors(idx, dist, codes, u)       the local inverse Simpson index of every cell under 1 .. 4 sets of categories
    lisi(embeddings, labels)                       JAMIE.test_lisi: iLISI (categories = modality) and cLISI (categories = label)
                                                   of the pooled cells from one search (Korsunsky et al. 2019)
    knn_graph(embeddings, k)                       JAMIE.neighbors: the kNN graph of the pooled cells as a scipy CSR matrix

The kernels are in csrc/neighbors.hip (include/jamie_hip.h, "Neighbourhoods on the device"): the workgroup of `metrics.cross_knn`
with the cell's own row refused by index, a second pass above a per-cell floor key for k > 64, and one wave per cell for the
perplexity solve in fp64.  Device memory is the input plus O(N k).  DESIGN.md §17.
"""
import numpy as np
import torch

from . import _native as nv
from .metrics import _device_input

SELF_KNN_MAX = 128     # largest k of jamie_self_knn
LISI_SETS_MAX = 4      # category sets of one jamie_lisi call
SEGMENT_TILE = 128     # seg_rows is a multiple of it


def _n_rows(X):
    return X.shape[0] if hasattr(X, 'shape') and len(X.shape) == 2 else len(X)


def check_k(k, n, what):
    """k under the rule 1 <= k <= min(n - 1, 128) for n cells.  Shared by the device and the host route."""
    k = int(k)
    if k < 1 or k > SELF_KNN_MAX:
        raise ValueError(f'{what}: k = {k}; the device search takes 1 <= k <= {SELF_KNN_MAX}')
    if k > n - 1:
        raise ValueError(f'{what}: k = {k} neighbours asked of the {n - 1} other rows')
    return k


def check_perplexity(perplexity, n_neighbors, n, what):
    """(perplexity, n_neighbors) under the rule 1 < perplexity < n_neighbors <= min(128, n - 1); n_neighbors None: min(int(3 *
    perplexity), n - 1).  Shared by the device and the host route."""
    perplexity = float(perplexity)
    if not perplexity > 1.0:
        raise ValueError(f'{what}: perplexity = {perplexity}; it must exceed 1')
    k = min(int(3 * perplexity), n - 1) if n_neighbors is None else int(n_neighbors)
    if k > min(SELF_KNN_MAX, n - 1):
        raise ValueError(f'{what}: n_neighbors = {k}; at most min({SELF_KNN_MAX}, cells - 1 = {n - 1})')
    if not perplexity < k:
        raise ValueError(f'{what}: perplexity = {perplexity} must be below n_neighbors = {k}')
    return perplexity, k


def self_knn(X, k, device='cuda', seg_rows=0):
    """The k rows of X nearest to every row of X other than itself, ascending by (distance, then lower index): (idx int32 [N, k],
    dist float32 [N, k]) device tensors, euclidean distances by direct difference in fp32.  A row is excluded by index: an exact
    copy of it is a neighbour at distance 0.  `seg_rows`: rows per segment of the walked side (0: the library's choice; else a
    multiple of 128); the result does not depend on it."""
    k = check_k(k, _n_rows(X), 'self_knn')
    seg_rows = int(seg_rows)
    if seg_rows < 0 or seg_rows % SEGMENT_TILE:
        raise ValueError(f'self_knn: seg_rows = {seg_rows}; 0 or a positive multiple of {SEGMENT_TILE}')
    x = _device_input(X, device, 'self_knn')
    if x.shape[1] < 1:
        raise ValueError('self_knn: empty input')
    N = x.shape[0]
    idx = torch.empty(N, k, dtype=torch.int32, device=x.device)
    dist = torch.empty(N, k, dtype=torch.float32, device=x.device)
    ws = torch.empty(nv.self_knn_workspace(N, k, seg_rows), dtype=torch.uint8, device=x.device)
    nv.self_knn(x, k, idx, dist, ws, seg_rows)
    return idx, dist


def lisi_from_neighbors(idx, dist, codes, perplexity, return_tries=False):
    """LISI of every cell from its neighbour lists (idx int32 [N, k], dist float32 [N, k], device tensors or numpy) under the
    category codes `codes` (integers, [N] or [n_sets, N], n_sets <= 4): float64 numpy [n_sets, N]; NaN where every neighbour
    weight underflowed.  `return_tries`: also the bisection steps per cell, int32 numpy [N]."""
    nv.require_gpu()
    codes = np.asarray(codes)
    codes = codes.reshape(1, -1) if codes.ndim == 1 else codes
    k = int(idx.shape[1]) if len(idx.shape) == 2 else 0
    if len(idx.shape) != 2 or tuple(idx.shape) != tuple(dist.shape):
        raise ValueError(f'lisi_from_neighbors: idx and dist must be [cells, k] of one shape, got {tuple(idx.shape)} and '
                         f'{tuple(dist.shape)}')
    N = int(idx.shape[0])
    if k < 2 or k > SELF_KNN_MAX:
        raise ValueError(f'lisi_from_neighbors: k = {k}; 2 <= k <= {SELF_KNN_MAX}')
    if codes.ndim != 2 or not 1 <= codes.shape[0] <= LISI_SETS_MAX or codes.shape[1] != N:
        raise ValueError(f'lisi_from_neighbors: codes must be [n_sets <= {LISI_SETS_MAX}, {N}], got {codes.shape}')
    perplexity = float(perplexity)
    if not 1.0 < perplexity < k:
        raise ValueError(f'lisi_from_neighbors: perplexity = {perplexity}; 1 < perplexity < k = {k}')
    idx_d = torch.as_tensor(idx).to('cuda', torch.int32).contiguous()
    dist_d = torch.as_tensor(dist).to(idx_d.device, torch.float32).contiguous()
    codes_d = torch.from_numpy(np.ascontiguousarray(codes, dtype=np.int32)).to(idx_d.device)
    out = torch.empty(codes.shape[0], N, dtype=torch.float64, device=idx_d.device)
    tries = torch.empty(N, dtype=torch.int32, device=idx_d.device) if return_tries else None
    nv.lisi(idx_d, dist_d, codes_d, perplexity, out, tries)
    if return_tries:
        return out.cpu().numpy(), tries.cpu().numpy()
    return out.cpu().numpy()


def pooled_codes(n_cells, labels, what):
    """(modality code int64 [N], label code int64 [N] or None, classes or None) of M embeddings of n_cells[m] cells."""
    M = len(n_cells)
    mod = np.repeat(np.arange(M, dtype=np.int64), n_cells)
    if labels is None:
        return mod, None, None
    if len(labels) != M:
        raise ValueError(f'{what}: one label array per embedding, got {len(labels)} for {M} embeddings')
    labs = [np.asarray(lab) for lab in labels]
    for m in range(M):
        if labs[m].ndim != 1 or labs[m].shape[0] != n_cells[m]:
            raise ValueError(f'{what}: one label per cell, got {labs[m].shape} for the {n_cells[m]} cells of embedding {m}')
    classes, lcode = np.unique(np.concatenate(labs), return_inverse=True)
    return mod, lcode.reshape(-1).astype(np.int64), classes


def lisi_summary(ilisi, clisi, M, classes, k):
    """The dict of `lisi` from the per-cell values (shared by the device and the host route)."""
    def med(v):
        return float(np.nanmedian(v)) if np.any(~np.isnan(v)) else float('nan')
    out = {'ilisi': ilisi, 'clisi': clisi, 'ilisi_median': med(ilisi), 'clisi_median': None, 'ilisi_scaled': float('nan'),
           'clisi_scaled': None, 'n_neighbors': int(k), 'n_failed': int(np.isnan(ilisi).sum()), 'labels': classes}
    if M > 1:
        out['ilisi_scaled'] = (out['ilisi_median'] - 1.0) / (M - 1)
    if clisi is not None:
        T = len(classes)
        out['clisi_median'] = med(clisi)
        out['clisi_scaled'] = (T - out['clisi_median']) / (T - 1) if T > 1 else float('nan')
    return out


def _pool(embeddings, device, what):
    if len(embeddings) < 1:
        raise ValueError(f'{what}: no embeddings')
    xs = [_device_input(e, device, what) for e in embeddings]
    for t in xs:
        if t.shape[1] != xs[0].shape[1]:
            raise ValueError(f'{what}: the embeddings must have the same features, got {t.shape[1]} and {xs[0].shape[1]}')
    return xs, (torch.cat(xs, dim=0) if len(xs) > 1 else xs[0])


def lisi(embeddings, labels=None, perplexity=30, n_neighbors=None, device='cuda'):
    """iLISI and cLISI of M embeddings [N_m, L] pooled into one set of cells (Korsunsky et al. 2019), from ONE neighbour search:

        ilisi [sum N_m], ilisi_median, ilisi_scaled     categories = the modality; 1: a cell sees one modality, M: all of them
                                                        evenly; scaled = (median - 1) / (M - 1), NaN for M = 1
        clisi [sum N_m], clisi_median, clisi_scaled     categories = np.unique of the pooled labels (T of them); scaled =
                                                        (T - median) / (T - 1); None without labels
        n_neighbors, n_failed, labels                   the k used (default min(int(3 perplexity), N - 1)), the cells whose
                                                        weights all underflowed (NaN; the medians skip them), np.unique labels
    """
    n_cells = [_n_rows(e) for e in embeddings]
    N = int(sum(n_cells))
    perplexity, k = check_perplexity(perplexity, n_neighbors, N, 'lisi')
    mod, lcode, classes = pooled_codes(n_cells, labels, 'lisi')
    xs, x = _pool(embeddings, device, 'lisi')
    idx, dist = self_knn(x, k, device)
    codes = mod[None, :] if lcode is None else np.stack([mod, lcode])
    values = lisi_from_neighbors(idx, dist, codes, perplexity)
    return lisi_summary(values[0], None if lcode is None else values[1], len(xs), classes, k)


def graph_from_lists(idx, dist, mode):
    """scipy CSR [N, N] with the k neighbours of every row in the row's neighbour order: float64 distances, or ones."""
    from scipy.sparse import csr_matrix
    if mode not in ('distance', 'connectivity'):
        raise ValueError(f"knn_graph: mode must be 'distance' or 'connectivity', not {mode!r}")
    N, k = idx.shape
    data = np.ones(N * k, np.float64) if mode == 'connectivity' else np.asarray(dist, dtype=np.float64).reshape(-1)
    return csr_matrix((data, np.asarray(idx, dtype=np.int32).reshape(-1), np.arange(0, N * k + 1, k, dtype=np.int64)), shape=(N, N))


def knn_graph(embeddings, k=15, mode='distance', device='cuda'):
    """The kNN graph of the pooled cells of M embeddings [N_m, L]: scipy CSR [N, N], k entries per row (the cell's k nearest
    other cells, nearest first), the distances as float64 (`mode='distance'`) or ones (`mode='connectivity'`): the form
    clustering and layout tools take."""
    if mode not in ('distance', 'connectivity'):
        raise ValueError(f"knn_graph: mode must be 'distance' or 'connectivity', not {mode!r}")
    k = check_k(k, int(sum(_n_rows(e) for e in embeddings)), 'knn_graph')
    _, x = _pool(embeddings, device, 'knn_graph')
    idx, dist = self_knn(x, k, device)
    return graph_from_lists(idx.cpu().numpy(), dist.cpu().numpy(), mode)

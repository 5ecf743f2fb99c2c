"""Layout quality of the pooled cells on the MI355X: how much of the neighbourhoods of one space survives in another, without an
N x N matrix.

    list_ranks(X, idx)                             where the entries of neighbour lists made elsewhere rank in the space X
    neighborhood_preservation(high, low, k)        JAMIE.test_layout: trustworthiness and continuity (Venna & Kaski 2001, sklearn's
                                                   definition), their curves over k = 1 .. K, the co-ranking curve Q_NX, LCMC
                                                   (Lee & Verleysen 2009) and the per-cell terms

The kernels are in csrc/coranking.hip (include/jamie_hip.h, "Layout quality on the device"): the neighbour lists are
`neighbors.self_knn`'s in both spaces, and one pass over the pair space of each space ranks the other space's list entries under
the same total order (q, index).  Every reduction is an integer sum; the figures are divided once on the host.  Device memory is
the inputs plus O(N k).  DESIGN.md §25.
"""
import numpy as np
import torch

from . import _native as nv
from .metrics import _device_input
from .neighbors import SEGMENT_TILE, _n_rows, self_knn

RANK_K_MAX = 64        # largest K of jamie_list_ranks


def check_neighbors(k, n, what):
    """k under sklearn's rule for trustworthiness, 1 <= k < n / 2, and the device's, k <= 64.  Shared by the device and the host
    route."""
    k = int(k)
    if k < 1 or k > RANK_K_MAX:
        raise ValueError(f'{what}: n_neighbors = {k}; the device ranks take 1 <= n_neighbors <= {RANK_K_MAX}')
    if not k < n / 2:
        raise ValueError(f'{what}: n_neighbors = {k} must be below half of the {n} cells')
    return k


def check_spaces(high, low, what):
    """The cells per modality of two lists of arrays that describe the same cells."""
    if len(high) < 1 or len(high) != len(low):
        raise ValueError(f'{what}: one array per modality in both spaces, got {len(high)} and {len(low)}')
    n_cells = [_n_rows(e) for e in high]
    for m, (n, e) in enumerate(zip(n_cells, low)):
        if _n_rows(e) != n:
            raise ValueError(f'{what}: both spaces must hold the same cells, got {n} and {_n_rows(e)} for modality {m}')
    return n_cells


def list_ranks(X, idx, device='cuda', seg_rows=0):
    """rank int32 [N, K] (device tensor): rank[i, t] = the rows of X other than i that lie before row idx[i, t] in the order
    (distance to row i, then lower index); 0 for the nearest other row, so an entry `self_knn(X, .)` puts at list position p has
    rank p.  idx int32 [N, K], K <= 64, in any order within a row; an entry equal to i or outside [0, N) gets -1.  `seg_rows` as in
    `self_knn`; the result does not depend on it."""
    seg_rows = int(seg_rows)
    if seg_rows < 0 or seg_rows % SEGMENT_TILE:
        raise ValueError(f'list_ranks: seg_rows = {seg_rows}; 0 or a positive multiple of {SEGMENT_TILE}')
    x = _device_input(X, device, 'list_ranks')
    idx_d = torch.as_tensor(idx).to(x.device, torch.int32).contiguous()
    N = x.shape[0]
    if idx_d.dim() != 2 or idx_d.shape[0] != N or not 1 <= idx_d.shape[1] <= RANK_K_MAX:
        raise ValueError(f'list_ranks: idx must be [{N}, 1 .. {RANK_K_MAX}], got {tuple(idx_d.shape)}')
    if N < 2 or x.shape[1] < 1:
        raise ValueError(f'list_ranks: at least 2 cells and 1 feature, got {tuple(x.shape)}')
    rank = torch.empty_like(idx_d)
    ws = torch.empty(nv.list_ranks_workspace(N, idx_d.shape[1], seg_rows), dtype=torch.uint8, device=x.device)
    nv.list_ranks(x, idx_d, rank, ws, seg_rows)
    return rank


def rank_sums(rank):
    """The integer sums of a rank array int32 [N, K] whose column p belongs to list position p: (penalty int64 [K], overlap int64
    [K], cell_penalty int64 [N]) as numpy -- see jamie_coranking_sums."""
    N, K = rank.shape
    penalty = torch.empty(K, dtype=torch.int64, device=rank.device)
    overlap = torch.empty(K, dtype=torch.int64, device=rank.device)
    cell = torch.empty(N, dtype=torch.int64, device=rank.device)
    nv.coranking_sums(rank, penalty, overlap, cell)
    return penalty.cpu().numpy(), overlap.cpu().numpy(), cell.cpu().numpy()


def host_rank_sums(rank):
    """`rank_sums` in numpy (the host route, and the restatement the device sums are tested against)."""
    rank = np.asarray(rank, dtype=np.int64)
    N, K = rank.shape
    penalty, overlap = np.empty(K, np.int64), np.empty(K, np.int64)
    for k in range(1, K + 1):
        r = rank[:, :k]
        penalty[k - 1] = np.maximum(r + 1 - k, 0).sum()
        overlap[k - 1] = np.count_nonzero((r >= 0) & (r < k))
    return penalty, overlap, np.maximum(rank + 1 - K, 0).sum(axis=1)


def preservation_summary(n_cells, K, sums_trust, sums_cont):
    """The dict of `neighborhood_preservation` from the integer sums of the two rank arrays (shared by the device and the host
    route): sums_trust of the low-space lists ranked in the high space, sums_cont of the high-space lists ranked in the low."""
    N = int(sum(n_cells))
    k = np.arange(1, K + 1, dtype=np.float64)
    norm = 2.0 / (N * k * (2.0 * N - 3.0 * k - 1.0))
    cell_norm = 2.0 / (K * (2.0 * N - 3.0 * K - 1.0))
    cuts = np.cumsum(n_cells)[:-1]
    t_curve = 1.0 - norm * sums_trust[0]
    c_curve = 1.0 - norm * sums_cont[0]
    qnx = sums_trust[1] / (N * k)
    lcmc = qnx - k / (N - 1.0)
    return {'trustworthiness': float(t_curve[-1]), 'continuity': float(c_curve[-1]), 'trustworthiness_curve': t_curve,
            'continuity_curve': c_curve, 'qnx': qnx, 'lcmc': lcmc, 'k_best': int(np.argmax(lcmc)) + 1,
            'cell_trustworthiness': np.split(1.0 - cell_norm * sums_trust[2], cuts),
            'cell_continuity': np.split(1.0 - cell_norm * sums_cont[2], cuts), 'n_neighbors': int(K), 'n_cells': N}


def neighborhood_preservation(high, low, n_neighbors=15, device='cuda', return_ranks=False):
    """How well the space `low` keeps the neighbourhoods of the space `high`: two lists of arrays [N_m, L_high] and [N_m, L_low]
    of the same cells, one pair per modality, pooled into one set of N cells.  With K = n_neighbors (1 <= K < N / 2, K <= 64):

        trustworthiness, continuity                    sklearn's `trustworthiness`: 1 - 2 / (N K (2N - 3K - 1)) sum max(0, r - K), r
                                                       the 1-based rank; trustworthiness ranks the K nearest of `low` in `high`
                                                       (false neighbours), continuity the K nearest of `high` in `low` (torn ones)
        trustworthiness_curve, continuity_curve [K]    the same at k = 1 .. K
        qnx [K], lcmc [K], k_best                      Q_NX(k): the mean share of a cell's k nearest in one space that are among
                                                       its k nearest in the other; LCMC = Q_NX(k) - k / (N - 1); its argmax (1-based)
        cell_trustworthiness, cell_continuity          one float64 array per modality: the cell's own term at K (their mean over
                                                       all cells is the headline figure)
        n_neighbors, n_cells                           K and N
        rank_high, rank_low, idx_high, idx_low         with `return_ranks`: int32 numpy [N, K]; rank_high[i, p] is the 0-based rank
                                                       in `high` of idx_low[i, p], rank_low[i, p] the rank in `low` of idx_high[i, p]
    """
    what = 'neighborhood_preservation'
    n_cells = check_spaces(high, low, what)
    N = int(sum(n_cells))
    K = check_neighbors(n_neighbors, N, what)
    spaces = []
    for side in (high, low):
        xs = [_device_input(e, device, what) for e in side]
        for t in xs:
            if t.shape[1] != xs[0].shape[1] or t.shape[1] < 1:
                raise ValueError(f'{what}: the arrays of one space must have the same features, got {t.shape[1]} and {xs[0].shape[1]}')
        spaces.append(torch.cat(xs, dim=0) if len(xs) > 1 else xs[0])
    x_high, x_low = spaces
    idx_high, _ = self_knn(x_high, K, device)
    idx_low, _ = self_knn(x_low, K, device)
    rank_high = list_ranks(x_high, idx_low, device)
    rank_low = list_ranks(x_low, idx_high, device)
    out = preservation_summary(n_cells, K, rank_sums(rank_high), rank_sums(rank_low))
    if return_ranks:
        out.update(rank_high=rank_high.cpu().numpy(), rank_low=rank_low.cpu().numpy(), idx_high=idx_high.cpu().numpy(),
                   idx_low=idx_low.cpu().numpy())
    return out

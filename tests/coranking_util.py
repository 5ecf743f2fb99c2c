"""Shared by tests/test_host_coranking.py and tests/test_hip_coranking.py: inputs, the float64 reference ranks, the numpy
restatement of what csrc/coranking.hip computes, and the near-tie counts the bounds are derived from."""
import functools

import numpy as np

from lisi_util import integer_cells, mixture, restated_self_knn  # noqa: F401
from metrics_util import REL_TOL

# ((cells per modality), L): the pooled N are no multiples of 64 or 128
SHAPES = [((700, 601), 32), ((400, 333), 8), ((300, 250), 100)]
KS = (15, 64)
EXCLUDED_CAP = 0.10    # largest share of list entries with another key within REL_TOL


def projection(L, seed):
    """A seeded standard-normal [L, 2] in fp32."""
    return np.random.default_rng(seed).standard_normal((L, 2)).astype(np.float32)


def restated_list_ranks(X, idx, rows=None):
    """The device ranks in numpy, for all rows or the rows `rows` only: q by direct difference in fp32 accumulated in ascending
    feature order (the product and the add of one feature rounded once, as the fma does; NaN read as +inf), the diagonal excluded
    by index, rank[i, t] = the rows l != i with (q(i, l), l) < (q(i, j), j), j = idx[i, t], by a stable sort on (q, index); -1
    where j == i or j is outside [0, N).  int32 [len(rows), K]."""
    X = np.asarray(X, np.float32)
    idx = np.asarray(idx, np.int64)
    N, L = X.shape
    rows = np.arange(N) if rows is None else np.asarray(rows)
    out = np.empty((len(rows), idx.shape[1]), np.int32)
    for a in range(0, len(rows), 512):
        r = rows[a:a + 512]
        q = np.zeros((len(r), N), np.float32)
        with np.errstate(invalid='ignore', over='ignore'):
            for c in range(L):
                t = (X[r, None, c] - X[None, :, c]).astype(np.float64)  # (the fp32 difference, widened: its square is exact in fp64)
                q = (q.astype(np.float64) + t * t).astype(np.float32)
        q[np.isnan(q)] = np.inf
        order = np.argsort(q, axis=1, kind='stable')                    # the row itself included, at its key (q(i, i), i)
        pos = np.empty(order.shape, np.int64)
        np.put_along_axis(pos, order, np.arange(N)[None, :], axis=1)
        j = idx[r]
        ok = (j >= 0) & (j < N) & (j != r[:, None])
        jj = np.where(ok, j, 0)
        own_first = np.take_along_axis(pos, r[:, None], axis=1) < np.take_along_axis(pos, jj, axis=1)
        out[a:a + 512] = np.where(ok, np.take_along_axis(pos, jj, axis=1) - own_first, -1)
    return out


def full_order(X):
    """float64 direct-difference distances of X, the diagonal at +inf, a stable argsort: (pos int64 [N, N] the 0-based rank of
    every cell j among the others of row i, order [N, N], ds [N, N - 1] the ascending distances to the other cells)."""
    from scipy.spatial.distance import cdist
    X = np.asarray(X, np.float64)
    d = cdist(X, X)
    np.fill_diagonal(d, np.inf)
    order = np.argsort(d, axis=1, kind='stable')
    pos = np.empty(order.shape, np.int64)
    np.put_along_axis(pos, order, np.arange(len(X))[None, :], axis=1)
    return pos, order, np.take_along_axis(d, order, axis=1)[:, :-1]


def near_keys(ds, rank, rel=REL_TOL):
    """For every list entry, given its 0-based rank in the ascending float64 distances ds [N, N - 1] of its row: the number of
    OTHER keys of the row within `rel` relative of its distance -- the places its rank may move when the distances are formed
    another way."""
    out = np.empty(rank.shape, np.int64)
    for i in range(len(ds)):
        d = ds[i, rank[i]]
        out[i] = np.searchsorted(ds[i], d * (1 + rel), side='right') - np.searchsorted(ds[i], d * (1 - rel), side='left') - 1
    return out


def penalty_slack(ref_rank, ds_rank_space, pos_rank_space, ds_list_space, order_list_space, K):
    """How far the penalty sum_{i, p < K} max(0, rank + 1 - K) may move between two routes whose distances agree within REL_TOL
    relative, in places (each worth 2 / (N K (2N - 3K - 1)) of trustworthiness): every list entry's rank by the keys within the
    tolerance of it in the ranking space, and, where keys of the list space within the tolerance of the K-th straddle the end of
    the list, a swap of list members: the members of that group inside the list times the spread of the group's penalties."""
    places = int(near_keys(ds_rank_space, ref_rank).sum())
    N = len(ds_list_space)
    for i in range(N):
        d = ds_list_space[i]
        lo = np.searchsorted(d, d[K - 1] * (1 - REL_TOL), side='left')
        hi = np.searchsorted(d, d[K - 1] * (1 + REL_TOL), side='right')
        if hi > K:                                                      # the group [lo, hi) reaches past the list
            pen = np.maximum(pos_rank_space[i, order_list_space[i, lo:hi]] + 1 - K, 0)
            places += int((K - lo) * (pen.max() - pen.min()))
    return places


def overlap_slack(ref_rank, ds_rank_space, ds_list_space, K):
    """How far the count #{(i, p < K) : rank < K} may move between two such routes: the entries with another key within the
    tolerance of theirs (only their ranks can cross K), and the list members a straddling group may trade."""
    moved = int(np.count_nonzero(near_keys(ds_rank_space, ref_rank) > 0))
    for d in ds_list_space:
        lo = np.searchsorted(d, d[K - 1] * (1 - REL_TOL), side='left')
        if np.searchsorted(d, d[K - 1] * (1 + REL_TOL), side='right') > K:
            moved += int(K - lo)
    return moved


@functools.lru_cache(maxsize=None)
def shape_case(which):
    """Inputs and float64 references of SHAPES[which], computed once: dict(sizes, high, low (lists of fp32 arrays), X, Y (pooled),
    pos_x, order_x, ds_x, pos_y, order_y, ds_y)."""
    sizes, L = SHAPES[which]
    high, _ = mixture(200 + which, 5, L, sizes)
    X = np.concatenate(high, axis=0)
    Y = X @ projection(L, 300 + which)
    low = np.split(Y, np.cumsum(sizes)[:-1])
    pos_x, order_x, ds_x = full_order(X)
    pos_y, order_y, ds_y = full_order(Y)
    return dict(sizes=sizes, high=high, low=low, X=X, Y=Y, pos_x=pos_x, order_x=order_x, ds_x=ds_x, pos_y=pos_y, order_y=order_y,
                ds_y=ds_y)


def reference_ranks(c, K):
    """(rank_high, rank_low, idx_high, idx_low) of a shape_case in float64: rank_high[i, p] the rank in X of the p-th nearest of
    Y, rank_low[i, p] the rank in Y of the p-th nearest of X."""
    idx_high, idx_low = c['order_x'][:, :K], c['order_y'][:, :K]
    return (np.take_along_axis(c['pos_x'], idx_low, axis=1), np.take_along_axis(c['pos_y'], idx_high, axis=1), idx_high, idx_low)

"""Shared by tests/test_host_metrics.py and tests/test_hip_metrics.py: inputs, float64 references and the numpy restatements of
what csrc/metrics.hip computes."""
import numpy as np

REL_TOL = 1e-5          # relative distance tolerance the project holds its fp32 distances to (EUC_TOL of the distance tests)


def noisy_pair(N, L, s, seed=0):
    """A = Z + s E1, B = Z + s E2 for independent standard normal Z, E1, E2 [N, L], rounded to fp32 (returned as fp32) so that
    the reference sees the device's inputs: two noisy views of the same cells."""
    rng = np.random.default_rng(seed)
    Z = rng.standard_normal((N, L))
    A = Z + s * rng.standard_normal((N, L))
    B = Z + s * rng.standard_normal((N, L))
    return A.astype(np.float32), B.astype(np.float32)


def reference_loop(e0, e1):
    """The loop of JAMIE.test_closer, returning the per-cell counts as well: (foscttm, row_closer, col_closer)."""
    from sklearn.metrics.pairwise import pairwise_distances
    d = pairwise_distances(np.concatenate([e0, e1], axis=0), metric='euclidean')
    size = e0.shape[0]
    row, col = np.zeros(size, np.int64), np.zeros(size, np.int64)
    for i in range(size):
        ld = d[i][size:]
        row[i] = np.sum(ld < ld[i])
        ld = d[size + i][:size]
        col[i] = np.sum(ld < ld[i])
    return (row.sum() + col.sum()) / (2 * size ** 2), row, col


def band_counts(d, own_rows, own_cols, rel):
    """Counts of d[i, j] < own * (1 + rel) along the rows (own_rows[i]) and down the columns (own_cols[j]) of a float64 distance
    block; the own pairs are not in `d` or are masked by the caller."""
    row = (d < (own_rows * (1 + rel))[:, None]).sum(axis=1)
    col = (d < (own_cols * (1 + rel))[None, :]).sum(axis=0)
    return row, col


def foscttm_band(A, B):
    """float64 reference of the FOSCTTM counts: exact counts and the band [lo, hi] under d(i, j) < d(i, i) (1 -/+ REL_TOL).
    Returns dict(exact=(row, col), lo=(row, col), hi=(row, col), value=float, share=band pairs / 2 N^2)."""
    from scipy.spatial.distance import cdist
    d = cdist(A.astype(np.float64), B.astype(np.float64))
    N = d.shape[0]
    own = np.diag(d).copy()
    np.fill_diagonal(d, np.inf)                      # j = i never counts
    out = {}
    for name, rel in (('exact', 0.0), ('lo', -REL_TOL), ('hi', REL_TOL)):
        out[name] = band_counts(d, own, own, rel)
    out['value'] = (out['exact'][0].sum() + out['exact'][1].sum()) / (2 * N ** 2)
    out['share'] = sum(int((h - l).sum()) for h, l in zip(out['hi'], out['lo'])) / (2 * N ** 2)
    return out


def tiled_counts(A, B, tile_i, tile_j):
    """The schedule of foscttm_kernel in numpy: the pair space in tile_i x tile_j tiles (ragged at the end), q by direct difference
    in fp32, each tile computed once and feeding the row counts and the column counts, j = i excluded by index."""
    A, B = np.asarray(A, np.float32), np.asarray(B, np.float32)
    N = A.shape[0]
    own = ((A - B) ** 2).sum(axis=1, dtype=np.float32)
    row, col = np.zeros(N, np.int64), np.zeros(N, np.int64)
    for i0 in range(0, N, tile_i):
        i1 = min(i0 + tile_i, N)
        for j0 in range(0, N, tile_j):
            j1 = min(j0 + tile_j, N)
            q = ((A[i0:i1, None, :] - B[None, j0:j1, :]) ** 2).sum(axis=2, dtype=np.float32)
            pair = np.arange(i0, i1)[:, None] != np.arange(j0, j1)[None, :]
            row[i0:i1] += (pair & (q < own[i0:i1, None])).sum(axis=1)
            col[j0:j1] += (pair & (q < own[None, j0:j1])).sum(axis=0)
    return row, col


def labelled_sets(seed=3, n_classes=7, dim=16, n_query=2000, n_ref=2300):
    """Two samples of one mixture of `n_classes` overlapping gaussians with string labels: (e0, l0) the queries, (e1, l1) the
    references; fp32-representable float64, so that sklearn and the device see the same numbers."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((n_classes, dim)) * 1.2
    names = np.array([f'type_{chr(ord("a") + c)}' for c in range(n_classes)])

    def draw(n):
        c = rng.integers(0, n_classes, n)
        x = centres[c] + rng.standard_normal((n, dim)) * 1.6
        return x.astype(np.float32).astype(np.float64), names[c]
    e0, l0 = draw(n_query)
    e1, l1 = draw(n_ref)
    return e0, l0, e1, l1


def vote_rule(d, ref_labels, k):
    """The device's prediction rule in numpy on a float64 distance matrix d [Nq, Nr]: neighbours ordered by (distance, index),
    majority vote over the classes of np.unique, ties to the lowest class.  Returns (pred, tied): tied[q] = the vote was tied."""
    classes, codes = np.unique(ref_labels, return_inverse=True)
    order = np.argsort(d, axis=1, kind='stable')[:, :k]
    votes = np.zeros((d.shape[0], len(classes)), np.int64)
    for s in range(k):
        np.add.at(votes, (np.arange(d.shape[0]), codes[order[:, s]]), 1)
    top = votes.max(axis=1)
    return classes[votes.argmax(axis=1)], (votes == top[:, None]).sum(axis=1) > 1


def near_tied(d_sorted, k, rel=REL_TOL):
    """Queries whose k-th and (k+1)-th neighbours are within `rel` relative distance (rows of ascending float64 distances)."""
    if k >= d_sorted.shape[1]:
        return np.zeros(d_sorted.shape[0], bool)
    return (d_sorted[:, k] - d_sorted[:, k - 1]) <= rel * d_sorted[:, k]

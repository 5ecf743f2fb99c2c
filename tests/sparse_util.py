"""Test data and float64 references for the sparse-input tests (tests/test_host_sparse_input.py, tests/test_hip_sparse_input.py)."""
import numpy as np
import scipy.sparse as sp

# the tolerances tests/test_hip_step.py holds jamie_col_stats to
MEAN_TOL = dict(rtol=1e-12, atol=1e-12)
SD_TOL = dict(rtol=1e-10, atol=1e-12)
# ... and the standardised cells
CELL_TOL = dict(rtol=2e-6, atol=1e-6)

EMPTY_COL, ONE_COL, FULL_COL, CONST_COL, OFFSET_COL = 0, 1, 2, 3, 4
CONST = 3.25


def sparse_counts(N, d, seed=0, dtype=np.float64):
    """(csr, dense): Poisson(0.3) counts masked to about 12 % density; first and last rows empty, row N // 2 fully stored, an entry
    in the last column of the last non-empty row (N - 2), three explicitly stored zeros.  From 8 features on, columns 0 .. 4 are: no
    entries, one entry, fully stored Poisson(5) + 1, fully stored constant 3.25, an offset of 1e4 on its stored entries (the two full
    columns are stored in all N rows, the first and the last included, so those two rows are then empty but for them: with fewer
    than 8 features they are empty).  Every value is exact in fp32."""
    assert N >= 8 and d >= 1
    rng = np.random.default_rng([seed, N, d])
    X = rng.poisson(0.3, (N, d)).astype(np.float64) * (rng.random((N, d)) < 0.46)
    stored = X != 0
    full_row = N // 2
    X[full_row] = rng.poisson(5.0, d) + 1.0
    stored[full_row] = True
    X[[0, N - 1]] = 0.0
    stored[[0, N - 1]] = False
    X[N - 2, d - 1] = 2.0
    stored[N - 2, d - 1] = True
    special = d >= 8
    if special:
        X[:, EMPTY_COL] = 0.0
        stored[:, EMPTY_COL] = False
        X[:, ONE_COL] = 0.0
        stored[:, ONE_COL] = False
        X[full_row, ONE_COL] = 4.0
        stored[full_row, ONE_COL] = True
        X[:, FULL_COL] = rng.poisson(5.0, N) + 1.0
        stored[:, FULL_COL] = True
        X[:, CONST_COL] = CONST
        stored[:, CONST_COL] = True
        X[stored[:, OFFSET_COL], OFFSET_COL] += 1e4
    # three explicitly stored zeros: unstored positions of rows 1 .. N - 2, right of the special columns
    first = 5 if special else 0
    free = np.argwhere(~stored[1:N - 1, first:])
    for r, c in free[np.linspace(0, len(free) - 1, 3).astype(int)] if len(free) >= 3 else free:
        stored[r + 1, c + first] = True
    rows, cols = np.nonzero(stored)
    A = sp.csr_matrix((X[rows, cols].astype(dtype), (rows, cols)), shape=(N, d))
    assert A.nnz == stored.sum() and (A.data == 0).sum() >= min(3, len(free))
    return A, X.astype(dtype)


def _segment_sum(v, lanes=256):
    """One segment's partial in the kernel's order: lane t adds elements t, t + lanes, ... in turn, then a halving tree over the lanes."""
    acc = np.zeros(lanes)
    pad = np.zeros(-(-len(v) // lanes) * lanes)
    pad[:len(v)] = v
    for row in pad.reshape(-1, lanes):
        acc = acc + row
    s = lanes // 2
    while s > 0:
        acc[:s] = acc[:s] + acc[s:2 * s]
        s //= 2
    return float(acc[0])


def restated_stats(vals, colptr, N, S):
    """The device's statistics in numpy, in the kernel's summation order: per column the stored values (CSC order) in segments of S,
    one float64 partial each (`_segment_sum`), the partials added in ascending order; mean = sum / N, sd = sqrt((sum of stored
    (v - mean)^2 + (N - n_c) mean^2) / N).  The means are the kernel's to the bit; the device contracts the squares into fused
    multiply-adds, so the sd agrees to rounding only."""
    d = len(colptr) - 1
    mean, sd = np.zeros(d), np.zeros(d)
    for c in range(d):
        v = np.asarray(vals[colptr[c]:colptr[c + 1]], dtype=np.float64)
        s = 0.0
        for b in range(0, len(v), S):
            s += _segment_sum(v[b:b + S])
        mean[c] = s / N
        q = 0.0
        for b in range(0, len(v), S):
            dv = v[b:b + S] - mean[c]
            q += _segment_sum(dv * dv)
        sd[c] = np.sqrt((q + (N - len(v)) * (mean[c] * mean[c])) / N)
    return mean, sd


class Ann:
    """The part of an AnnData object the facade looks at: `.X`."""

    def __init__(self, X):
        self.X = X

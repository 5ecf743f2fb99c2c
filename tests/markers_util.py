"""Cases, references and tolerances for the marker-feature tests (tests/test_host_markers.py, tests/test_hip_markers.py)."""
import functools

import numpy as np

PIECE = 512             # cells of a moments piece (jamie_amd/markers.py PIECE), 16 row groups in it
NRG = 16

# mean and var of a group against a two-pass centred float64 reference, as |got - ref| / (1 + |ref|).  Measured with
# `restated_error` on the cases of tests/test_hip_markers.py (CASES below): the float64 numpy restatement of the device's
# arithmetic -- the same shift by row 0, the same row groups, pieces and orders, through the same `markers.finish` -- lies at most
# 6.09e-16 (mean, at (257, 70, 40)) and 9.64e-14 (var, at (8193, 70, 2)) from that reference over all of CASES; the column offset
# by 1e4 does not stand out, the shift takes it away.  The tolerance is 8 x the measured distance: inside a piece the device may
# contract dx * dx + acc into one fused multiply-add, which numpy does not.
MEAN_TOL = 8 * 6.09e-16
VAR_TOL = 8 * 9.64e-14
# `mean_rest`, `mean_difference` and `var_rest` come from the same sums by the same arithmetic and are held to the same bounds,
# against the host route.  Welch's t against the host route's, same measure: the restatement lies at most 3.85e-14 from it (at
# (12289, 130, 300)); 8 x that.
T_TOL = 8 * 3.85e-14

# (N, d, G): every N, d and G of the issue at least once; G = 300 with one-cell groups and segments shorter than a wave
CASES = [(2, 1, 2), (257, 33, 7), (257, 70, 40), (4097, 1, 2), (4097, 130, 40), (8193, 33, 300), (8193, 70, 2), (12289, 33, 7),
         (12289, 130, 300), (4097, 70, 300), (257, 130, 40)]
CONTINUOUS, CONSTANT, OFFSET = 1, 2, 3      # the special columns, where d has room; every other column is zero-inflated


@functools.lru_cache(maxsize=None)
def case(N, d, G, seed=0):
    """(X fp32 [N, d], labels int64 [N]), read-only.  Zero-inflated values rounded to halves (heavy ties) whose rate of non-zeros
    is raised in group f mod G of feature f, so the groups do differ; column 1 continuous, column 2 constant, column 3 offset by
    1e4.  Every group has a cell; the sizes fall off with the group index, so with many groups the late ones keep one cell.  The
    cells are shuffled: no group is contiguous."""
    rng = np.random.default_rng(seed + 7919 * N + 31 * d + G)
    G = min(G, N)
    weights = 1.0 / (1.0 + np.arange(G)) ** 2
    labels = np.concatenate([np.arange(G), rng.choice(G, N - G, p=weights / weights.sum())]).astype(np.int64)
    labels = labels[rng.permutation(N)]
    marked = labels[:, None] == (np.arange(d) % G)[None, :]
    X = np.round(rng.exponential(1.5, (N, d)) * 2) / 2 * (rng.random((N, d)) < np.where(marked, 0.85, 0.35))
    if d > CONTINUOUS:
        X[:, CONTINUOUS] = rng.exponential(1.0, N) + 0.5 * marked[:, CONTINUOUS]
    if d > CONSTANT:
        X[:, CONSTANT] = 3.0
    if d > OFFSET:
        X[:, OFFSET] += 1e4
    X = X.astype(np.float32)
    X.setflags(write=False)
    labels.setflags(write=False)
    return X, labels


@functools.lru_cache(maxsize=None)
def host_reference(N, d, G, tie_correct=True, seed=0):
    """The host route's dict for `case(N, d, G)`: computed once, shared, not to be written to."""
    from jamie_amd.jamie import _host_rank_features
    X, labels = case(N, d, G, seed)
    return _host_rank_features(X, labels, 25, tie_correct)


def reference_mean_var(X, labels):
    """(mean, var) [G, d] per group in float64, two passes, centred; var is NaN for a group of one cell."""
    X = np.asarray(X, dtype=np.float64)
    groups = np.unique(labels)
    mean, var = np.empty((len(groups), X.shape[1])), np.full((len(groups), X.shape[1]), np.nan)
    for g, name in enumerate(groups):
        x = X[labels == name]
        mean[g] = x.mean(0)
        if len(x) > 1:
            var[g] = ((x - mean[g]) ** 2).sum(0) / (len(x) - 1)
    return mean, var


def restated_sums(X, labels):
    """(pivot [d], sums [G, d, 2]): the device's moments pass in float64 numpy.  A group's cells in stable label order are cut
    into pieces of PIECE; in a piece cell m goes to row group m mod 16, a row group adds its cells in order, the row groups are
    added in order, and the pieces in ascending order."""
    X32 = np.asarray(X, dtype=np.float32)
    pivot = X32[0].astype(np.float64)
    groups, codes = np.unique(labels, return_inverse=True)
    order = np.argsort(codes.reshape(-1), kind='stable')
    sizes = np.bincount(codes.reshape(-1))
    sums = np.zeros((len(groups), X32.shape[1], 2))
    start = 0
    for g, n in enumerate(sizes):
        for p0 in range(start, start + n, PIECE):
            dx = X32[order[p0:min(p0 + PIECE, start + n)]].astype(np.float64) - pivot
            piece = np.zeros((2, X32.shape[1]))
            for rg in range(NRG):
                acc = np.zeros((2, X32.shape[1]))
                for row in dx[rg::NRG]:
                    acc[0] += row
                    acc[1] += row * row
                piece += acc
            sums[g, :, 0] += piece[0]
            sums[g, :, 1] += piece[1]
        start += n
    return pivot, sums


def scaled_error(got, ref):
    """max |got - ref| / (1 + |ref|) over the entries where the reference has a figure; 0 where it has none."""
    ok = ~np.isnan(ref)
    return float(np.max(np.abs(got - ref)[ok] / (1.0 + np.abs(ref[ok])))) if ok.any() else 0.0


def restated_error(N, d, G):
    """How far the restatement of the device's arithmetic lies from the two-pass reference on `case(N, d, G)`: (mean, var)."""
    from jamie_amd import markers as jmk
    X, labels = case(N, d, G)
    ref = host_reference(N, d, G)
    pivot, sums = restated_sums(X, labels)
    out = jmk.finish(ref['groups'], ref['n'], ref['rank_sum2'], ref['tie_term'], pivot, sums)
    mean, var = reference_mean_var(X, labels)
    return scaled_error(out['mean'], mean), scaled_error(out['var'], var)


def restated_t_error(N, d, G):
    """How far Welch's t of the restated sums lies from the host route's on `case(N, d, G)`."""
    from jamie_amd import markers as jmk
    ref = host_reference(N, d, G)
    pivot, sums = restated_sums(*case(N, d, G))
    out = jmk.finish(ref['groups'], ref['n'], ref['rank_sum2'], ref['tie_term'], pivot, sums)
    return scaled_error(out['t'], ref['t'])


def order_keys(x):
    """The device's fp32 -> uint32 key: the order of the floats, -0.0 on +0.0's key."""
    u = np.asarray(x, dtype=np.float32).view(np.uint32).copy()
    u[u == 0x80000000] = 0
    return np.where(u & 0x80000000, ~u, u | np.uint32(0x80000000)).astype(np.uint32)

"""Shared by tests/test_host_imputation.py and tests/test_hip_imputation.py: inputs, float64 references and the numpy restatement
of what csrc/imputation.hip computes (key map, chunk sort, rank merge, count)."""
import functools

import numpy as np

R_TOL = 1e-10           # |r - r_ref|: fp64 sums of pivot-shifted values (the same arithmetic on the host is within 1.3e-14 at
MSE_RTOL = 1e-12        # N = 5000; fp64 without the pivot misses by 1.6e-6, a shift in fp32 by 1.9e-9), MSE relative
AUROC_TOL = 1e-12       # host roc_auc_score against U2 / (2 n_pos n_neg)
SENTINEL = np.uint32(0xFFFFFFFF)


# ---- references ----
def reference_r_mse(X, Y):
    """float64: r from centred columns, NaN where a column of either input is constant (np.ptp == 0); MSE."""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    xc, yc = X - X.mean(0), Y - Y.mean(0)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = (xc * yc).sum(0) / np.sqrt((xc * xc).sum(0) * (yc * yc).sum(0))
    r[(np.ptp(X, axis=0) == 0) | (np.ptp(Y, axis=0) == 0)] = np.nan
    return r, ((X - Y) ** 2).mean(0)


def reference_u2(X, Y, thr):
    """(U2, n_pos) int64 [d]: label Y > thr (compared in fp32, as the device does), U2 = sum over positives of
    (#negatives below + #negatives not above) from np.searchsorted on the sorted negatives."""
    X, Y = np.asarray(X, dtype=np.float32), np.asarray(Y, dtype=np.float32)
    N, d = X.shape
    thr = np.broadcast_to(np.asarray(thr, dtype=np.float32), (d,))
    U2, n_pos = np.zeros(d, np.int64), np.zeros(d, np.int64)
    for f in range(d):
        lab = Y[:, f] > thr[f]
        neg, pos = np.sort(X[~lab, f]), X[lab, f]
        n_pos[f] = lab.sum()
        U2[f] = int(np.searchsorted(neg, pos, 'left').sum()) + int(np.searchsorted(neg, pos, 'right').sum())
    return U2, n_pos


def auroc_of(U2, n_pos, N):
    pairs = 2.0 * n_pos.astype(np.float64) * (N - n_pos).astype(np.float64)
    out = np.full(len(U2), np.nan)
    np.divide(U2.astype(np.float64), pairs, out=out, where=pairs > 0)
    return out


def brute_force_u2(x, label):
    """All pairs: 2 #{(p, n) : n < p} + #{(p, n) : n == p}, compared as floats."""
    pos, neg = x[label][:, None], x[~label][None, :]
    return 2 * int((neg < pos).sum()) + int((neg == pos).sum())


# ---- the device's pipeline in numpy ----
def order_keys(x):
    """fp32 -> uint32 in the order of the floats; -0.0 takes the key of +0.0."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).copy()
    u[u == np.uint32(0x80000000)] = 0
    neg = (u & np.uint32(0x80000000)) != 0
    return np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def rank_merge_pass(keys, R):
    """One pass over runs of R keys: the left run's element at i goes to i + lower_bound(right run), the right run's at j to
    j + upper_bound(left run); a last run without a partner is copied."""
    n = len(keys)
    out = np.full(n, 0, np.uint32)
    written = np.zeros(n, bool)
    for base in range(0, n, 2 * R):
        a, b = keys[base:base + R], keys[base + R:base + 2 * R]
        if len(b) == 0:
            to_a, to_b = base + np.arange(len(a)), np.zeros(0, np.int64)
        else:
            to_a = base + np.arange(len(a)) + np.searchsorted(b, a, 'left')
            to_b = base + np.arange(len(b)) + np.searchsorted(a, b, 'right')
        for to, v in ((to_a, a), (to_b, b)):
            assert not written[to].any()
            out[to] = v
            written[to] = True
    assert written.all()
    return out


def merge_split(A, B, diag, lanes=64):
    """How many keys of A are among the first `diag` keys of merge(A, B), A first on ties, found as the kernel finds it: `lanes`
    evenly spaced candidates per step.  Returns (split, steps); every index it reads is checked to lie inside A and B."""
    nA, nB = len(A), len(B)
    lo, hi, steps = max(0, diag - nB), min(diag, nA), 0
    while lo < hi:
        step = (hi - lo + lanes - 1) // lanes
        cnt = 0
        for lane in range(lanes):
            mid = lo + lane * step
            if mid < hi:
                assert 0 <= mid < nA and 0 <= diag - 1 - mid < nB
                before = A[mid] <= B[diag - 1 - mid]
                assert not before or cnt == lane               # the candidates that hold are a prefix
                cnt += bool(before)
        if cnt == 0:
            hi = lo
        else:
            m = lo + (cnt - 1) * step
            lo, hi = m + 1, min(hi, m + step)
        steps += 1
    return lo, steps


def merge_pass_windows(keys, R, T, lanes=64):
    """rank_merge_pass as the kernel walks it: windows of T consecutive output keys, their two slices found by merge_split and
    ranked against each other."""
    n = len(keys)
    assert R % T == 0 and n % T == 0
    out = np.zeros(n, np.uint32)
    for og in range(0, n, T):
        base = og // (2 * R) * (2 * R)
        b0 = base + R
        if b0 >= n:
            out[og:og + T] = keys[og:og + T]
            continue
        A, B = keys[base:b0], keys[b0:min(b0 + R, n)]
        d0 = og - base
        assert d0 + T <= len(A) + len(B)
        a0, a1 = merge_split(A, B, d0, lanes)[0], merge_split(A, B, d0 + T, lanes)[0]
        sa, sb = A[a0:a1], B[d0 - a0:d0 + T - a1]
        assert 0 <= a1 - a0 <= T and len(sa) + len(sb) == T
        win = np.zeros(T, np.uint32)
        hit = np.zeros(T, bool)
        for to, v in ((np.arange(len(sa)) + np.searchsorted(sb, sa, 'left'), sa), (np.arange(len(sb)) + np.searchsorted(sa, sb, 'right'), sb)):
            assert not hit[to].any()
            win[to] = v
            hit[to] = True
        assert hit.all()
        out[og:og + T] = win
    return out


def pipeline_u2(x, label, chunk):
    """Key map -> sentinel for positives and padding -> chunk sort -> rank-merge passes -> every positive ranked in the first
    n_neg keys.  Returns (U2, n_pos, passes)."""
    n = len(x)
    npad = (n + chunk - 1) // chunk * chunk
    keys = np.full(npad, SENTINEL, np.uint32)
    k = order_keys(x)
    keys[:n][~label] = k[~label]
    keys = np.sort(keys.reshape(-1, chunk), axis=1).reshape(-1)
    R, passes = chunk, 0
    while R < npad:
        keys = rank_merge_pass(keys, R)
        R *= 2
        passes += 1
    n_pos = int(label.sum())
    neg = keys[:n - n_pos]
    assert np.all(neg[:-1] <= neg[1:]) and np.all(keys[n - n_pos:] == SENTINEL)
    pk = k[label]
    return int(np.searchsorted(neg, pk, 'left').sum() + np.searchsorted(neg, pk, 'right').sum()), n_pos, passes


# ---- inputs ----
@functools.lru_cache(maxsize=None)
def stats_case(N, d, seed=0):
    """(X, Y) fp32 [N, d], read-only: two noisy views of one signal.  Where d has room: column 0 at mean 1e4 (X) and 3e4 (Y) with
    unit spread, column 1 scaled by 1e-3, column 2 constant in X (0.1f), column 3 X == Y, column 4 constant in Y."""
    rng = np.random.default_rng(1000 * seed + N + d)
    Z = rng.standard_normal((N, d))
    X = Z + 0.6 * rng.standard_normal((N, d))
    Y = Z + 0.6 * rng.standard_normal((N, d))
    X[:, 0] += 1e4
    Y[:, 0] += 3e4
    if d > 1:
        X[:, 1] *= 1e-3
        Y[:, 1] *= 1e-3
    if d > 2:
        X[:, 2] = 0.1
    X, Y = X.astype(np.float32), Y.astype(np.float32)
    if d > 3:
        Y[:, 3] = X[:, 3]
    if d > 4:
        Y[:, 4] = -7.25
    X.setflags(write=False)
    Y.setflags(write=False)
    return X, Y


SPECIAL = 7             # columns 1 .. 7 of an AUROC case are the edge cases below, where d has room


@functools.lru_cache(maxsize=None)
def auroc_case(N, d, halves=False, seed=0):
    """(X, Y, real) for threshold 0: scores X = signal + noise, measurement Y = signal + noise, fp32 [N, d], read-only; `real`
    marks the plain real-valued columns.  `halves`: every score rounded to a multiple of 1/2 (heavy ties).  Where d has room:
    column 1 scores rounded to halves, 2 scores among -0.0, +0.0, -1, 1, 3 one negative, 4 one positive, 5 all positive, 6 all
    negative, 7 every score equal."""
    rng = np.random.default_rng(1000 * seed + N + 7 * d + halves)
    Z = rng.standard_normal((N, d))
    X = (Z + 1.2 * rng.standard_normal((N, d))).astype(np.float32)
    Y = (Z + 0.5 * rng.standard_normal((N, d))).astype(np.float32)
    real = np.ones(d, bool)
    real[1:1 + SPECIAL] = False
    if halves:
        X = (np.round(X * 2) / 2).astype(np.float32)
    if d > 1:
        X[:, 1] = np.round(X[:, 1] * 2) / 2
    if d > 2:
        X[:, 2] = rng.choice(np.array([-0.0, 0.0, -1.0, 1.0], np.float32), N)
    if d > 3:
        Y[:, 3] = 1.0
        Y[N // 3, 3] = -1.0
    if d > 4:
        Y[:, 4] = -1.0
        Y[N // 2, 4] = 1.0
    if d > 5:
        Y[:, 5] = 2.0
    if d > 6:
        Y[:, 6] = 0.0                                     # (not above the threshold: strict)
    if d > 7:
        X[:, 7] = 3.5
    for a in (X, Y, real):
        a.setflags(write=False)
    return X, Y, real


@functools.lru_cache(maxsize=None)
def auroc_reference(N, d, halves=False, seed=0):
    X, Y, real = auroc_case(N, d, halves, seed)
    U2, n_pos = reference_u2(X, Y, 0.0)
    U2.setflags(write=False)
    n_pos.setflags(write=False)
    return U2, n_pos

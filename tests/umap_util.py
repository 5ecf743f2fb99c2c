"""Shared by tests/test_host_umap.py and tests/test_hip_umap.py: inputs, float64 references and the numpy restatement of what
csrc/umap.hip computes."""
import functools

import numpy as np

import lisi_util as lu
import tsne_util as tu

EPS = 2.0 ** -24
NEAR_BRANCH = tu.NEAR_BRANCH          # a solve whose trace comes this close to a branch is left out of the device comparison
NEAR_BRANCH_CAP = tu.NEAR_BRANCH_CAP
GROUP = 16                            # lanes that own a row in the epoch kernel
NEG = 5                               # negative_sample_rate of the tests
LONGEST_ROW = 299                     # the hub's row: the longest row of any test below

# Relative tolerance of the device's move delta_i (per row and coordinate) against float64 numpy on the same fp32 layout, the same
# firing entries and the same draws, relative to the float64 sum of the MAGNITUDES of the row's terms.  DESIGN.md §20 derives it
# from the kernel's operation order, with u = 2^-24 and to first order:
#   dx, dy                      one rounding each                                                  u
#   d2 = fma(dx, dx, dy dy)     dy dy carries 2u + u, dx dx 2u, the fma rounds once                 4u
#   p = powf(d2, b)             b 4u handed on, and 1 ulp of powf (ROCm's documented figure) <= 2u  (4b + 2)u
#   q = fma(a, p, 1)            at most p's error, and one rounding                                (4b + 3)u
#   m2ab p                      the constant's rounding, p, the product                            (4b + 4)u
#   d2 q                        4u + (4b + 3)u + u                                                 (4b + 8)u
#   c = (m2ab p) / (d2 q)       both, and the quotient's rounding                                  (8b + 13)u
#   c dx                        dx's rounding and the product's                                    (8b + 15)u
# (the repulsive term has fewer: (4b + 14)u; the clip is 1-Lipschitz and the factor 2 is exact).  With b <= 1 a term is good to
# 23u of its magnitude.  The additions: a term passes at most NEG additions inside its entry's sum, one per entry of its lane
# (ceil(row / 16) of them) and the 4 levels of the lane tree, each adding at most u of the magnitudes summed so far.  For the
# longest row of the tests (299 entries: 19 per lane) that is 5 + 19 + 4 = 28, so 51u; 52u leaves the second-order terms room.
TERM_ROUNDINGS = 23
ADD_DEPTH = NEG + -(-LONGEST_ROW // GROUP) + 4
UPDATE_TOL = (TERM_ROUNDINGS + ADD_DEPTH + 1) * EPS
TINY = 1e-37                          # below the fp32 normal range a term has no relative accuracy

# pooled N -> ((cells per modality), L, n_neighbors): K = N - 1 (every row is full); a typical row; rows of two entries per lane;
# K = 64, rows just past a wave; K = 128
SHAPES = {8: ((5, 3), 4, 8), 130: ((70, 60), 8, 15), 257: ((129, 128), 16, 31), 600: ((350, 250), 32, 65), 1000: ((1000,), 3, 129)}
CASES = tuple(sorted(SHAPES)) + ('hub', 'special')
BLOCK = (10, 27)       # 'special': cells 10 .. 26 are one point (n_neighbors + 2 = 17 of them)
TRIPLE = (40, 44)      # 'special': cell 40 has three copies
OUTLIER = 77           # 'special': one cell far from everything
HUB = 123


@functools.lru_cache(maxsize=None)
def shape_case(name):
    """Inputs and float64 lists of a case, computed once: dict(emb, X fp32 pooled, nn, K, idx, dist)."""
    if name == 'hub':            # 299 cells on a sphere and its centre: every cell lists the centre, whose row has 299 entries
        rng = np.random.default_rng(4)
        X = rng.standard_normal((300, 64))
        X /= np.linalg.norm(X, axis=1, keepdims=True)
        X[HUB] = 0.0
        emb, nn = [X.astype(np.float32)], 15
    elif name == 'special':
        X = np.concatenate(lu.mixture(330, 5, 8, (70, 60))[0], axis=0)
        X[BLOCK[0]:BLOCK[1]] = X[BLOCK[0]]
        X[TRIPLE[0]:TRIPLE[1]] = X[TRIPLE[0]]
        X[OUTLIER] = X[OUTLIER] + np.float32(1e4)
        emb, nn = [X[:70].copy(), X[70:].copy()], 15
    else:
        sizes, L, nn = SHAPES[name]
        emb, _ = lu.mixture(200 + name, 5, L, sizes)
    X = np.concatenate(emb, axis=0)
    idx, dist, _ = lu.knn_reference(X, nn - 1)
    return dict(emb=emb, X=X, nn=nn, K=nn - 1, idx=idx, dist=dist)


def smooth_reference(dist, nn):
    """The float64 loop of DESIGN.md §20 step 1 over all cells: dict(W float64 [N, K], rho, sigma, tries, psi_sum (the last sum of
    the solve), floored (the floor decided sigma), margin: the smallest of | |sum - target| - 1e-5 | and |sum - target| seen in
    the trace, where a last-bit difference could change a branch)."""
    dist = np.asarray(dist, np.float64)
    N, K = dist.shape
    target = np.log2(float(nn))
    W, rho, sigma, tries = np.empty((N, K)), np.empty(N), np.empty(N), np.empty(N, np.int64)
    psi_sum, floored, margin = np.empty(N), np.zeros(N, bool), np.empty(N)
    for i in range(N):
        d = dist[i]
        r = d[d > 0].min() if np.any(d > 0) else 0.0
        e = d - r
        lo, hi, mid, m = 0.0, np.inf, 1.0, np.inf
        for t in range(1, 65):
            s = sum_psi = np.where(e > 0, np.exp(-np.where(e > 0, e, 0.0) / mid), 1.0).sum()
            m = min(m, abs(abs(s - target) - 1e-5), abs(s - target))
            if abs(s - target) < 1e-5:
                break
            if s > target:
                hi = mid
                mid = (lo + hi) / 2
            else:
                lo = mid
                mid = mid * 2 if hi == np.inf else (lo + hi) / 2
        fl = 1e-3 * d.sum() / nn
        sg = max(mid, fl)
        W[i] = 1.0 if sg == 0 else np.where(e > 0, np.exp(-np.where(e > 0, e, 0.0) / sg), 1.0)
        rho[i], sigma[i], tries[i], psi_sum[i], floored[i], margin[i] = r, sg, t, sum_psi, fl > mid, m
    return dict(W=W, rho=rho, sigma=sigma, tries=tries, psi_sum=psi_sum, floored=floored, margin=margin)


def union_reference(idx, W):
    """W + W^T - W o W^T as scipy CSR in float64 with sorted indices, from lists idx [N, K] and weights W [N, K]."""
    from scipy.sparse import csr_matrix
    N, K = idx.shape
    D = csr_matrix((np.asarray(W, np.float64).reshape(-1), np.asarray(idx).reshape(-1), np.arange(0, N * K + 1, K)), shape=(N, N))
    A = D + D.T - D.multiply(D.T)
    A = csr_matrix(A)
    A.sort_indices()
    return A


def graph_arrays(idx, W):
    """(rowptr, col, val float32, row) of the fuzzy graph in the defined row order, from float64 arithmetic on the fp32 weights W."""
    N, K = idx.shape
    A = union_reference(idx, np.asarray(W, np.float32)).todok()
    order = tu.row_order(np.asarray(idx))
    rowptr = np.zeros(N + 1, np.int64)
    rowptr[1:] = np.cumsum([len(r) for r in order])
    col = np.concatenate([np.asarray(r, np.int64) for r in order])
    row = np.repeat(np.arange(N), np.diff(rowptr))
    val = np.array([A[i, j] for i, j in zip(row, col)], np.float64).astype(np.float32)
    return rowptr, col.astype(np.int32), val, row


def schedule_scalar(val, n_epochs, epochs):
    """The fp32 schedule as a scalar loop: (eps, next after `epochs` epochs, fired [epochs, nnz] bool)."""
    f = np.float32
    top = f(max(val))
    eps, nxt = [], []
    for v in val:
        e = f(top / f(v)) if f(v) >= f(top / f(n_epochs)) else f(np.inf)
        eps.append(e)
        nxt.append(e)
    fired = np.zeros((epochs, len(val)), bool)
    for n in range(epochs):
        for k in range(len(val)):
            if nxt[k] <= f(n):
                fired[n, k] = True
                nxt[k] = f(nxt[k] + eps[k])
    return np.array(eps, f), np.array(nxt, f), fired


def _coefficients(d2, a, b, gamma, attract):
    safe = np.where(d2 > 0, d2, 1.0)
    p = safe ** b
    c = -2.0 * a * b * (p / safe) / (1.0 + a * p) if attract else 2.0 * gamma * b / ((0.001 + safe) * (1.0 + a * p))
    return np.where(d2 > 0, c, 0.0)


def epoch_reference(row, col, fire, Y, n, a, b, gamma, neg, seed):
    """The float64 move of epoch n at the layout Y over the firing entries `fire` (bool [nnz]) with the definition's draws:
    dict(delta [N, 2], mag [N, 2] the sums of the terms' magnitudes, fired [N], self_draws, zero_terms)."""
    from jamie_amd.umap import negative_cells
    Y = np.asarray(Y, np.float64)
    N = len(Y)
    e = np.nonzero(fire)[0]
    i, j = row[e], col[e].astype(np.int64)
    d = Y[i] - Y[j]
    d2 = (d * d).sum(axis=1)
    t = 2.0 * np.clip(_coefficients(d2, a, b, gamma, True)[:, None] * d, -4.0, 4.0)
    move, mag = t.copy(), np.abs(t)
    zero = int((d2 == 0).sum())
    cells = negative_cells(seed, e, n, neg, N)
    own = 0
    for r in range(neg):
        k = cells[:, r]
        d = Y[i] - Y[k]
        d2 = (d * d).sum(axis=1)
        t = np.clip(_coefficients(d2, a, b, gamma, False)[:, None] * d, -4.0, 4.0) * (k != i)[:, None]
        move += t
        mag += np.abs(t)
        own += int((k == i).sum())
        zero += int(((d2 == 0) & (k != i)).sum())
    def rows(v):
        return np.stack([np.bincount(i, weights=v[:, 0], minlength=N), np.bincount(i, weights=v[:, 1], minlength=N)], axis=1)
    return dict(delta=rows(move), mag=rows(mag), fired=np.bincount(i, minlength=N), self_draws=own, zero_terms=zero)


def _f32(x):
    return np.asarray(x, np.float64).astype(np.float32)


def _restated_terms(dx, dy, a, b, m2ab, g2b, attract):
    """clip(c dx), clip(c dy) in the kernel's fp32 operation order (an fma is formed in float64 and rounded to fp32)."""
    f = np.float32
    d2 = _f32(dx.astype(np.float64) ** 2 + (dy * dy).astype(np.float64))
    safe = np.where(d2 > 0, d2, f(1))
    p = np.power(safe, f(b)).astype(f)
    q = _f32(np.float64(f(a)) * p.astype(np.float64) + 1.0)
    c = (f(m2ab) * p) / (safe * q) if attract else f(g2b) / ((f(0.001) + safe) * q)
    c = np.where(d2 > 0, c, f(0)).astype(f)
    return np.clip(c * dx, f(-4), f(4)).astype(f), np.clip(c * dy, f(-4), f(4)).astype(f)


def restated_epoch(rowptr, col, fire, Y, n, a, b, gamma, neg, seed):
    """The device design in numpy fp32: the terms as `_restated_terms`; an entry's sum 2 attraction + draw 0 + draw 1 + ...; lane l
    of a row's 16 adds its entries l, l + 16, ... in order; the lanes by the xor tree 8, 4, 2, 1.  delta float32 [N, 2]."""
    from jamie_amd.umap import negative_cells
    f = np.float32
    Y = np.asarray(Y, f)
    N = len(Y)
    a, b = f(a), f(b)
    m2ab, g2b = f(-2.0 * float(a) * float(b)), f(2.0 * gamma * float(b))
    row = np.repeat(np.arange(N), np.diff(rowptr))
    e = np.nonzero(fire)[0]
    i, j = row[e], col[e].astype(np.int64)
    tx, ty = _restated_terms(Y[i, 0] - Y[j, 0], Y[i, 1] - Y[j, 1], a, b, m2ab, g2b, True)
    sx, sy = f(2) * tx, f(2) * ty
    cells = negative_cells(seed, e, n, neg, N)
    for r in range(neg):
        k = cells[:, r]
        tx, ty = _restated_terms(Y[i, 0] - Y[k, 0], Y[i, 1] - Y[k, 1], a, b, m2ab, g2b, False)
        sx = np.where(k != i, sx + tx, sx).astype(f)
        sy = np.where(k != i, sy + ty, sy).astype(f)
    lanes = np.zeros((N, GROUP, 2), f)
    lane = (e - rowptr[i]) % GROUP
    for t in range(len(e)):                                 # (ascending e: a lane's entries in their order)
        lanes[i[t], lane[t], 0] += sx[t]
        lanes[i[t], lane[t], 1] += sy[t]
    for s in (8, 4, 2, 1):
        lanes = lanes + lanes[:, np.arange(GROUP) ^ s, :]
    return lanes[:, 0, :]


def update_error(delta, ref):
    """The largest error of a move relative to UPDATE_TOL times the float64 sum of its terms' magnitudes (plus TINY)."""
    err = np.abs(np.asarray(delta, np.float64) - ref['delta'])
    return float(np.max(err / (UPDATE_TOL * ref['mag'] + TINY))) * UPDATE_TOL


@functools.lru_cache(maxsize=None)
def host_run(seed, n_epochs=200, init='random'):
    """`JAMIE(metrics='host').umap` of the blobs."""
    from jamie_amd import JAMIE
    emb, _ = tu.blobs()
    return JAMIE(metrics='host').umap(emb, n_epochs=n_epochs, init=init, seed=seed)


@functools.lru_cache(maxsize=None)
def spread_layout(name):
    """A spread-out layout of a case: the host route's after 50 epochs, float32 [N, 2]."""
    from jamie_amd import JAMIE
    c = shape_case(name)
    out = JAMIE(metrics='host').umap(c['emb'], n_neighbors=c['nn'], n_epochs=50)
    return np.concatenate(out['layout'], axis=0)

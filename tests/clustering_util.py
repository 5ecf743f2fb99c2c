"""Shared by tests/test_host_clustering.py and tests/test_hip_clustering.py: the float64 reference of the k-means definition
(DESIGN.md §18), the numpy restatement of what csrc/clustering.hip computes (the fp32 chain of q, fp32 centres, fp64 sums, the
block order of the weighted pick), the bounds derived from the number formats, and the case list."""
import functools

import numpy as np

import lisi_util as lu

U32 = 2.0 ** -24       # unit roundoff of fp32
PICK_BLOCK = 1024


def band(L):
    """Relative gap between a cell's two nearest centres below which fp32 may order them otherwise: either q carries at most
    (L + 2) roundings (the difference, L additions, and one to spare) of 2^-24 each; twice that for the pair, twice again for
    a centre rounded to fp32."""
    return 4 * (L + 2) * U32


def q_float64(X, C):
    from scipy.spatial.distance import cdist
    return cdist(np.asarray(X, np.float64), np.asarray(C, np.float64), 'sqeuclidean')


def q_restated(X, C):
    """The device's q in numpy: the fp32 difference, its square added to the running fp32 sum with one rounding (the fma), in
    ascending feature order from 0.  fp32 [N, k]."""
    X, C = np.asarray(X, np.float32), np.asarray(C, np.float32)
    q = np.zeros((len(X), len(C)), np.float32)
    for c in range(X.shape[1]):
        t64 = (X[:, None, c] - C[None, :, c]).astype(np.float64)   # (the fp32 difference, widened: its square is exact in fp64)
        q64 = q.astype(np.float64)
        q = (q64 + t64 * t64).astype(np.float32)
    return q


def pick_float64(w, u):
    """The smallest i whose prefix sum of w exceeds u * total (np.cumsum order); floor(u N) where total == 0."""
    prefix = np.cumsum(np.asarray(w, np.float64))
    n = len(prefix)
    if prefix[-1] > 0:
        return min(int(np.searchsorted(prefix, u * prefix[-1], side='right')), n - 1)
    return min(int(u * n), n - 1)


def pick_restated(w, u):
    """jamie_weighted_pick's order of additions: fp64 totals of blocks of 1024 by the tree v[i] += v[i + s], s = 512 .. 1; the
    block prefix in ascending order; an ascending scan inside the first block whose inclusive prefix exceeds u * total."""
    w = np.asarray(w, np.float32)
    n = len(w)
    nb = (n + PICK_BLOCK - 1) // PICK_BLOCK
    v = np.zeros(nb * PICK_BLOCK, np.float64)
    v[:n] = w
    v = v.reshape(nb, PICK_BLOCK)
    while v.shape[1] > 1:
        h = v.shape[1] // 2
        v = v[:, :h] + v[:, h:]
    totals = v[:, 0]
    total = 0.0
    for b in range(nb):
        total = total + totals[b]
    if not total > 0:
        return min(int(u * n), n - 1)
    target = u * total
    before, b = 0.0, 0
    while b < nb - 1 and not before + totals[b] > target:
        before = before + totals[b]
        b += 1
    i1 = min(n, (b + 1) * PICK_BLOCK)
    run, last = before, i1 - 1
    for i in range(b * PICK_BLOCK, i1):
        run = run + float(w[i])
        if w[i] > 0:
            last = i
        if run > target:
            return i
    return last


def _margin(q):
    """The smallest relative gap between the two nearest centres over the rows of q [N, k] (inf for k == 1)."""
    if q.shape[1] < 2:
        return np.inf
    two = np.partition(np.asarray(q, np.float64), 1, axis=1)[:, :2]
    gap = (two[:, 1] - two[:, 0]) / np.where(two[:, 1] > 0, two[:, 1], 1.0)
    return float(gap.min())


def lloyd(X, C, max_iter, tol_abs, restated):
    """Iterations of the definition from the centres C.  restated: X fp32, q by `q_restated`, centres (float)(sum / count) with
    the sum in fp64; else everything in float64.  dict(labels, centers = C_{t+1}, inertia, n_iter, converged, sizes, n_empty,
    margin = the smallest relative gap between a cell's two nearest centres over all iterations, in this route's q)."""
    N, L = X.shape
    k = len(C)
    X64 = np.asarray(X, np.float64)
    prev, converged, margin = None, False, np.inf
    for t in range(1, max_iter + 1):
        q = q_restated(X, C) if restated else q_float64(X, C)
        margin = min(margin, _margin(q))
        lab = np.argmin(q, axis=1)
        inertia = float(q[np.arange(N), lab].astype(np.float64).sum())
        counts = np.bincount(lab, minlength=k)
        sums = np.zeros((k, L))
        np.add.at(sums, lab, X64)
        new = np.array(C, dtype=np.float64)
        new[counts > 0] = sums[counts > 0] / counts[counts > 0, None]
        if restated:
            new = new.astype(np.float32)
        shift = float(((new.astype(np.float64) - np.asarray(C, np.float64)) ** 2).sum())
        same = prev is not None and np.array_equal(lab, prev)
        C, prev = new, lab
        if same or shift <= tol_abs:
            converged = True
            break
    return dict(labels=lab, centers=C, inertia=inertia, n_iter=t, converged=converged, sizes=counts,
                n_empty=int((counts == 0).sum()), margin=margin)


def seeds(X, u, restated):
    """Plain k-means++ from the uniform numbers u: the cells picked, int64 [k]."""
    N = len(X)
    q = q_restated if restated else q_float64
    pick = pick_restated if restated else pick_float64
    out = np.empty(len(u), np.int64)
    out[0] = min(int(u[0] * N), N - 1)
    minq = q(X, X[out[0]][None])[:, 0]
    for j in range(1, len(u)):
        out[j] = pick(minq, u[j])
        minq = np.minimum(minq, q(X, X[out[j]][None])[:, 0])
    return out


def kmeans(X, k, n_init=4, max_iter=300, tol=1e-4, seed=0, init=None, restated=False):
    """The definition: float64 throughout, or (`restated`) the device's arithmetic on the fp32 cells.  The dict of `lloyd` plus
    run, seeds (of the winning run) and margin over all runs."""
    X = np.asarray(X, np.float32 if restated else np.float64)
    tol_abs = tol * float(np.mean(np.var(np.asarray(X, np.float64), axis=0)))
    best, margin = None, np.inf
    for r in range(1 if init is not None else n_init):
        if init is None:
            s = seeds(X, np.random.default_rng([seed, r]).random(k), restated)
            C = X[s].copy()
        else:
            s, C = None, np.asarray(init, X.dtype).copy()
        out = lloyd(X, C, max_iter, tol_abs, restated)
        margin = min(margin, out['margin'])
        if best is None or out['inertia'] < best['inertia']:
            best = dict(out, run=r, seeds=s)
    best['margin'] = margin
    return best


def inertia_bound_same_centres(L, inertia):
    """|sum of the fp32 chain's minq - the float64 inertia| under the SAME fp32 centres and labels: a q of the chain carries the
    rounding of each difference (squared: 2 u) and of L additions, gamma_(L + 2); the fp64 sum of N terms adds N 2^-53.  (L + 3) u
    covers gamma's second order for L < 2^20."""
    return (L + 3) * U32 * inertia


def inertia_bound_rounded_centres(L, inertia, centre_sq):
    """... and where the centres are the float64 ones rounded to fp32 (|dc| <= u |c| by feature): every cell's q moves by at most
    2 |x - c| |dc| + |dc|^2, summed with Cauchy-Schwarz: 2 u sqrt(inertia * sum_i |c(i)|^2) + u^2 sum_i |c(i)|^2.  centre_sq: sum
    over the cells of the squared norm of their centre."""
    return inertia_bound_same_centres(L, inertia) + 2 * U32 * np.sqrt(inertia * centre_sq) + U32 ** 2 * centre_sq


# (which of lisi_util.SHAPES, k, seed): data mixture(seed + 11, 5, L, sizes); n_init = 2 runs each.  All four shapes, k = 5 and 17,
# seeds 0 and 1, except the three of those 16 whose float64 margin over all iterations of both runs is below band(L): they take the
# first later seed that has the margin (the seeds tried in between fell short as well, 1.0e-7 to 6.0e-6).  The restatement and
# the float64 route agreed in seeds, iterations and labels on the three replaced cases too; they are left out because agreement
# there is not implied by the arithmetic.  test_host_clustering.py::test_design_restated prints and asserts every margin.
N_INIT = 2
REPLACED = {(0, 17, 0): 9,     # (700, 601) L = 32: margin 1.05e-6 < 8.1e-6; seeds 2 .. 8 also below
            (2, 5, 0): 2,      # (300, 250) L = 100: margin 2.4e-6 < 2.4e-5
            (2, 17, 1): 4}     # (300, 250) L = 100: margin 2.6e-7 < 2.4e-5; seeds 2, 3 also below
CASES = [(w, k, REPLACED.get((w, k, s), s)) for w in range(len(lu.SHAPES)) for k in (5, 17) for s in (0, 1)]


@functools.lru_cache(maxsize=None)
def case_data(which, seed):
    sizes, L, _ = lu.SHAPES[which]
    emb, lab = lu.mixture(seed + 11, 5, L, sizes)
    return emb, lab, np.concatenate(emb, axis=0)


@functools.lru_cache(maxsize=None)
def case_reference(which, k, seed):
    """The float64 route on a case, computed once."""
    return kmeans(case_data(which, seed)[2], k, n_init=N_INIT, seed=seed)


@functools.lru_cache(maxsize=None)
def case_restated(which, k, seed):
    return kmeans(case_data(which, seed)[2], k, n_init=N_INIT, seed=seed, restated=True)


def contingency_reference(a, b, na, nb):
    t = np.zeros((na, nb), np.int64)
    np.add.at(t, (np.asarray(a), np.asarray(b)), 1)
    return t

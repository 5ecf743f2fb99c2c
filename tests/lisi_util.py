"""Shared by tests/test_host_lisi.py and tests/test_hip_lisi.py: inputs, float64 references and the numpy restatements of what
csrc/neighbors.hip computes."""
import functools

import numpy as np

# Per-cell relative tolerance of a device LISI (fp32 direct-difference distances, fp64 solve) against the all-float64 route, on
# cells without a near tie at the K-th / (K + 1)-th neighbour: 4 x the largest difference the numpy restatement of that design
# shows over those cells of SHAPES (test_host_lisi.py::test_design_restated prints it: 7.8e-6).  The factor is there because the
# device's exp / log and sqrtf differ from numpy's in the last bit and can move a stopping iteration.
LISI_TOL = 3.2e-5

# ((cells per modality), L, K): the pooled N are no multiples of 64 or 128
SHAPES = [((700, 601), 32, 90), ((400, 333), 8, 30), ((300, 250), 100, 126), ((500, 520), 3, 63)]
N_LABELS = 5


def mixture(seed, T, L, sizes, spread=1.6, shift=0.3):
    """T gaussian centres (sigma 1.2); modality m holds sizes[m] cells = centre + spread * noise + shift * m, fp32.  Returns
    (embeddings, labels): a list of fp32 [sizes[m], L] and a list of string label arrays."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((T, L)) * 1.2
    names = np.array([f'type_{chr(ord("a") + c)}' for c in range(T)])
    emb, lab = [], []
    for m, n in enumerate(sizes):
        c = rng.integers(0, T, n)
        emb.append((centres[c] + spread * rng.standard_normal((n, L)) + shift * m).astype(np.float32))
        lab.append(names[c])
    return emb, lab


def knn_reference(X, K):
    """float64 `cdist`, the diagonal at +inf, a stable argsort: (idx [N, K], dist [N, K], ds [N, K + 1]); ds are the ascending
    distances with one more column (where N allows) for `metrics_util.near_tied`."""
    from scipy.spatial.distance import cdist
    X = np.asarray(X, np.float64)
    d = cdist(X, X)
    np.fill_diagonal(d, np.inf)
    order = np.argsort(d, axis=1, kind='stable')
    ds = np.take_along_axis(d, order[:, :K + 1], axis=1)
    keep = min(K + 1, len(X) - 1)
    return order[:, :K], ds[:, :K], ds[:, :keep]


def simpson_reference(D, codes_nb, C, perplexity):
    """`compute_simpson_index` of the LISI package for one cell in float64: D its K neighbour distances, codes_nb the neighbours'
    category codes ([K], or [n_sets, K] with C a sequence), C the number of categories.  Returns (lisi, tries, margin): lisi a
    float (or a list, one per set), NaN where every weight underflowed; margin the smallest of | |Hdiff| - 1e-5 | and |Hdiff|
    seen in the trace: the places where a last-bit difference could change a branch."""
    D = np.asarray(D, np.float64)
    log_u = np.log(perplexity)

    def hbeta(beta):
        P = np.exp(-D * beta)
        s = P.sum()
        if s == 0:
            return 0.0, np.zeros_like(D)
        return float(np.log(s) + beta * np.sum(D * P) / s), P / s

    beta, bmin, bmax = 1.0, -np.inf, np.inf
    H, P = hbeta(beta)
    diff, tries = H - log_u, 0
    margin = min(abs(abs(diff) - 1e-5), abs(diff))
    while abs(diff) > 1e-5 and tries < 50:
        if diff > 0:
            bmin = beta
            beta = beta * 2 if bmax == np.inf else (beta + bmax) / 2
        else:
            bmax = beta
            beta = beta / 2 if bmin == -np.inf else (beta + bmin) / 2
        H, P = hbeta(beta)
        diff, tries = H - log_u, tries + 1
        margin = min(margin, abs(abs(diff) - 1e-5), abs(diff))

    def one(codes, n):
        if H == 0:
            return float('nan')
        codes = np.asarray(codes)
        return 1.0 / float(sum(P[codes == b].sum() ** 2 for b in range(n)))
    codes_nb = np.asarray(codes_nb)
    if codes_nb.ndim == 1:
        return one(codes_nb, C), tries, margin
    return [one(c, n) for c, n in zip(codes_nb, C)], tries, margin


def lisi_reference(idx, dist, codes, C, perplexity):
    """simpson_reference over all cells: idx [N, K], dist [N, K], codes [n_sets, N], C [n_sets] -> (lisi [n_sets, N], tries [N],
    margin [N])."""
    codes = np.asarray(codes)
    N = len(idx)
    out, tries, margin = np.empty((len(codes), N)), np.empty(N, np.int64), np.empty(N)
    for i in range(N):
        v, tries[i], margin[i] = simpson_reference(dist[i], codes[:, idx[i]], C, perplexity)
        out[:, i] = v
    return out, tries, margin


def restated_self_knn(X, K):
    """The device search in numpy: q by direct difference in fp32 accumulated in ascending feature order (the product and the add
    of one feature rounded once, as the fma does), the diagonal excluded by index, neighbours ascending by (q, index), dist =
    sqrt in fp32.  (idx [N, K], dist fp32 [N, K])."""
    X = np.asarray(X, np.float32)
    N, L = X.shape
    q = np.zeros((N, N), np.float32)
    for c in range(L):
        t = (X[:, None, c] - X[None, :, c]).astype(np.float64)      # (the fp32 difference, widened: its square is exact in fp64)
        q = (q.astype(np.float64) + t * t).astype(np.float32)
    np.fill_diagonal(q, np.inf)
    order = np.argsort(q, axis=1, kind='stable')[:, :K]
    return order, np.sqrt(np.take_along_axis(q, order, axis=1))


def two_pass_select(q, K, first=64):
    """The two passes of the device search for K > 64 on one row of keys q (index = position; the caller has taken the cell
    itself out): the `first` smallest (q, index), then the K - first smallest of the keys above the floor, the last key of the
    first pass."""
    idx = np.arange(len(q))
    order = np.lexsort((idx, q))
    a = order[:first]
    fq, fi = q[a[-1]], a[-1]
    above = (q > fq) | ((q == fq) & (idx > fi))
    cand = idx[above]
    b = cand[np.lexsort((cand, q[cand]))][:K - first]
    return np.concatenate([a, b])


def integer_cells(n=900, L=3, seed=5):
    """Integer-valued cells in [-2, 2]: every q is a small integer, exact in fp32, and most cells tie at every list boundary
    (98.7 % at the 64th / 65th neighbour).  One cell has no copy of itself and more than 30 neighbours at distance 1: at
    perplexity 30 its entropy cannot come down to log(30) and its solve stops at the cap of 50 tries."""
    return np.random.default_rng(seed).integers(-2, 3, (n, L)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def shape_case(which):
    """Inputs and float64 references of SHAPES[which], computed once: dict(emb, lab, X fp32 pooled, K, mod, lcode, T, idx, dist,
    ds)."""
    sizes, L, K = SHAPES[which]
    emb, lab = mixture(100 + which, N_LABELS, L, sizes)
    X = np.concatenate(emb, axis=0)
    classes, lcode = np.unique(np.concatenate(lab), return_inverse=True)
    mod = np.repeat(np.arange(len(sizes)), sizes)
    idx, dist, ds = knn_reference(X, K)
    return dict(emb=emb, lab=lab, X=X, K=K, mod=mod, lcode=lcode.reshape(-1), T=len(classes), M=len(sizes), idx=idx, dist=dist, ds=ds)


@functools.lru_cache(maxsize=None)
def shape_lisi(which, perplexity):
    """The all-float64 LISI of SHAPES[which] (modality, label): (lisi [2, N], tries, margin)."""
    c = shape_case(which)
    return lisi_reference(c['idx'], c['dist'], np.stack([c['mod'], c['lcode']]), (c['M'], c['T']), perplexity)

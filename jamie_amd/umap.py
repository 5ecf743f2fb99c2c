"""UMAP layout of the pooled cells on the MI355X: the fuzzy neighbour graph and synchronous stochastic epochs, O(N K) memory.

    find_ab(spread, min_dist)                      the curve 1 / (1 + a x^(2b)) fitted to umap-learn's target
    smooth_knn(idx, dist, n_neighbors)             (W fp32 [N, K], rho, sigma, tries): umap-learn's `smooth_knn_dist`
    fuzzy_graph(idx, W)                            A = W + W^T - W o W^T as a CSR matrix on the device (`JointP` layout, to_scipy())
    edge_schedule(graph, n_epochs)                 (eps, next) fp32 [nnz]: epochs per sample of every entry and its first firing
    epoch(graph, Y_in, Y_out, eps, nxt, n, ...)    one epoch on device tensors: for tests and for other optimisers
    optimize(graph, Y, eps, nxt, n_epochs, ...)    all epochs enqueued without a read-back
    umap(embeddings)                               JAMIE.umap on the device: the layout of M embeddings pooled into one set of cells

The kernels are in csrc/umap.hip (include/jamie_hip.h, "UMAP layout on the device").  The neighbours are `neighbors.self_knn`'s:
n_neighbors - 1 <= 128 other cells per cell.  The definition (shared with the float64 host route of jamie.py) is DESIGN.md §20;
it departs from umap-learn in four places: the epochs are synchronous (every read is from the layout the epoch started with),
every firing draws exactly `negative_sample_rate` cells, sigma has a per-row floor, and the init is PCA, not spectral (the
spectral init is `spectral.spectral(...)['umap_init']`, passed as the array `init`: jamie_amd/spectral.py).
"""
import numpy as np
import torch

from . import _native as nv
from . import tsne as jts
from .clustering import check_finite
from .neighbors import SELF_KNN_MAX, _n_rows, _pool, self_knn

MAX_TRIES = 64         # of the sigma solve
SUM_TOL = 1e-5
SIGMA_FLOOR = 1e-3     # sigma >= SIGMA_FLOOR * (sum of the row's distances) / n_neighbors
NEG_MAX = 64
INIT_SPAN = 10.0
_M32 = np.uint64(0xffffffff)


# ---- the random draws both routes share ----
def philox4x32_10(counter, key):
    """Philox4x32 with 10 rounds (Salmon et al., SC'11) in numpy, the twin of csrc/common.h's: `counter` four and `key` two arrays
    (or ints) of 32-bit words, broadcast against one another; the four output words as uint64 arrays of 32-bit values."""
    c0, c1, c2, c3 = (np.asarray(x, dtype=np.uint64) & _M32 for x in counter)
    k0, k1 = (np.asarray(x, dtype=np.uint64) & _M32 for x in key)
    m0, m1, w0, w1, s32 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85), np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2                            # < 2^64: both factors are below 2^32
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & _M32, (p0 >> s32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + w0) & _M32, (k1 + w1) & _M32
    return c0, c1, c2, c3


def negative_cells(seed, e, n, negative_sample_rate, N):
    """The cells drawn by the entries at CSR positions `e` (int array) in epoch `n`: int64 [len(e), negative_sample_rate].  Draw r
    is word r & 3 of Philox4x32-10 at counter (e & 0xffffffff, e >> 32, n, r >> 2) under key (seed & 0xffffffff, seed >> 32), and
    the cell is (word * N) >> 32: a function of (seed, e, n, r) and N only."""
    e = np.asarray(e, dtype=np.uint64).reshape(-1)
    seed = np.uint64(int(seed) & 0xffffffffffffffff)
    out = np.empty((len(e), int(negative_sample_rate)), dtype=np.int64)
    for q in range((int(negative_sample_rate) + 3) // 4):
        words = philox4x32_10((e & _M32, e >> np.uint64(32), np.uint64(int(n)), np.uint64(q)), (seed & _M32, seed >> np.uint64(32)))
        for w in range(4):
            r = 4 * q + w
            if r < out.shape[1]:
                out[:, r] = ((words[w] * np.uint64(int(N))) >> np.uint64(32)).astype(np.int64)
    return out


# ---- the argument checks and the definitions both routes share ----
def find_ab(spread=1.0, min_dist=0.1):
    """(a, b) of 1 / (1 + a x^(2b)) fitted by `scipy.optimize.curve_fit` to umap-learn's target on linspace(0, 3 spread, 300): 1
    below min_dist, exp(-(x - min_dist) / spread) above.  (1.5769435, 0.8950609) at the defaults."""
    from scipy.optimize import curve_fit
    x = np.linspace(0.0, 3.0 * float(spread), 300)
    y = np.where(x < min_dist, 1.0, np.exp(-(x - min_dist) / spread))
    (a, b), _ = curve_fit(lambda x, a, b: 1.0 / (1.0 + a * x ** (2.0 * b)), x, y)
    return float(a), float(b)


def default_epochs(N):
    return 500 if N <= 10000 else 200


def smooth_target(n_neighbors):
    """log2(n_neighbors) as the one double both routes and the kernel use."""
    return float(np.log2(float(n_neighbors)))


def _positive(v, name, what):
    v = float(v)
    if not v > 0.0 or not np.isfinite(v):
        raise ValueError(f'{what}: {name} = {v}; it must be positive and finite')
    return v


def check_umap(embeddings, n_neighbors, min_dist, spread, n_epochs, learning_rate, negative_sample_rate, repulsion_strength, init,
               a, b, what='umap'):
    """The checks of JAMIE.umap in their order; (n_neighbors, n_epochs, learning_rate, negative_sample_rate, repulsion_strength,
    init, a, b) with n_epochs None resolved to 500 (N <= 10 000) or 200, an array init as float32 [N, 2], and a, b fitted by
    `find_ab(spread, min_dist)` unless both are given.  Nothing is allocated on a device."""
    if len(embeddings) < 1:
        raise ValueError(f'{what}: no embeddings')
    for e in embeddings:
        if len(e.shape) != 2 or e.shape[1] != embeddings[0].shape[1] or e.shape[1] < 1:
            raise ValueError(f'{what}: the embeddings must be [cells, features] with the same features')
    N = int(sum(int(e.shape[0]) for e in embeddings))
    nn = int(n_neighbors)
    if nn < 2 or nn > min(N, SELF_KNN_MAX + 1):
        raise ValueError(f'{what}: n_neighbors = {nn}; 2 <= n_neighbors <= min(cells = {N}, {SELF_KNN_MAX + 1})')
    min_dist, spread = float(min_dist), float(spread)
    if not spread > 0.0 or not np.isfinite(spread):
        raise ValueError(f'{what}: spread = {spread}; it must be positive and finite')
    if not 0.0 <= min_dist <= spread:
        raise ValueError(f'{what}: min_dist = {min_dist}; 0 <= min_dist <= spread = {spread}')
    n_epochs = default_epochs(N) if n_epochs is None else int(n_epochs)
    if n_epochs < 1:
        raise ValueError(f'{what}: n_epochs = {n_epochs}; at least 1')
    learning_rate = _positive(learning_rate, 'learning_rate', what)
    nsr = int(negative_sample_rate)
    if nsr < 1 or nsr > NEG_MAX or nsr != negative_sample_rate:
        raise ValueError(f'{what}: negative_sample_rate = {negative_sample_rate}; an integer in 1 .. {NEG_MAX}')
    gamma = _positive(repulsion_strength, 'repulsion_strength', what)
    if isinstance(init, str):
        if init not in ('pca', 'random'):
            raise ValueError(f"{what}: init must be 'pca', 'random' or an array [cells, 2], not {init!r}")
    else:
        init = np.asarray(init.detach().cpu().numpy() if torch.is_tensor(init) else init, dtype=np.float32)
        if init.shape != (N, 2):
            raise ValueError(f'{what}: init must be [{N}, 2], got {init.shape}')
        if not np.isfinite(init).all():
            raise ValueError(f'{what}: init contains NaN or infinity')
    if (a is None) != (b is None):
        raise ValueError(f'{what}: a and b are given together')
    if a is not None:
        a, b = _positive(a, 'a', what), _positive(b, 'b', what)
    check_finite(embeddings, what)
    if a is None:
        a, b = find_ab(spread, min_dist)
    return nn, n_epochs, learning_rate, nsr, gamma, init, a, b


def initial_layout(X, init, seed):
    """Y_0 float32 [N, 2] from the pooled cells X (numpy [N, L]): 'pca' -- `tsne.initial_layout`'s scores; 'random' --
    `default_rng(seed).uniform(0, 10, (N, 2))`; both then mapped per column onto [0, 10] in float64 (a constant column becomes 5);
    an array is taken as it is.  One function for both routes: they start from identical bits."""
    if not isinstance(init, str):
        return np.ascontiguousarray(init, dtype=np.float32).copy()
    if init == 'random':
        Y = np.random.default_rng(seed).uniform(0.0, INIT_SPAN, (len(X), 2))
    else:
        Y = jts.initial_layout(X, 'pca', seed).astype(np.float64)
    lo, hi = Y.min(axis=0), Y.max(axis=0)
    span = np.where(hi > lo, hi - lo, 1.0)
    return np.where(hi > lo, INIT_SPAN * (Y - lo) / span, INIT_SPAN / 2).astype(np.float32)


def schedule_arrays(val, n_epochs):
    """(eps, next) float32 of the graph values `val` (numpy float32): eps = max / val as an fp32 division where val >= max /
    n_epochs (an fp32 division too), else +inf; next starts at eps."""
    val = np.asarray(val, dtype=np.float32)
    top = val.max() if val.size else np.float32(0)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        eps = np.where(val >= top / np.float32(n_epochs), top / val, np.float32(np.inf)).astype(np.float32)
    return eps, eps.copy()


def curve32(a, b):
    """(a, b) as the epochs use them: rounded to fp32 once (the kernel holds them so), as doubles."""
    return float(np.float32(a)), float(np.float32(b))


def alpha_of(learning_rate, n, n_epochs):
    return float(learning_rate) * (1.0 - float(n) / float(n_epochs))


def umap_summary(Y, n_cells, a, b, n_epochs, n_neighbors, n_edges, n_fired, graph):
    """The dict of JAMIE.umap (shared by the device and the host route)."""
    return {'layout': np.split(np.asarray(Y, dtype=np.float32), np.cumsum(n_cells)[:-1]), 'a': float(a), 'b': float(b),
            'n_epochs': int(n_epochs), 'n_neighbors': int(n_neighbors), 'n_edges': int(n_edges), 'n_fired': int(n_fired),
            'graph': graph}


# ---- the device route ----
def smooth_knn(idx, dist, n_neighbors):
    """Smooth kNN distances of every cell over its neighbour list (idx int32 [N, K], dist float32 [N, K] nearest first, K =
    n_neighbors - 1: `self_knn`): (W float32 [N, K], rho float64 [N], sigma float64 [N], tries int32 [N]) device tensors.  One fp64
    bisection per cell for the sigma at which sum_j exp(-max(d_j - rho, 0) / sigma) is log2(n_neighbors) within 1e-5 (at most 64
    tries), floored at 1e-3 of the row's mean distance."""
    nv.require_gpu()
    if len(idx.shape) != 2 or tuple(idx.shape) != tuple(dist.shape):
        raise ValueError(f'umap smooth_knn: idx and dist must be [cells, k] of one shape, got {tuple(idx.shape)} and {tuple(dist.shape)}')
    k, nn = int(idx.shape[1]), int(n_neighbors)
    if k < 1 or k > SELF_KNN_MAX or nn < 2:
        raise ValueError(f'umap smooth_knn: k = {k}, n_neighbors = {nn}; 1 <= k <= {SELF_KNN_MAX}, n_neighbors >= 2')
    dist_d = torch.as_tensor(dist).to('cuda', torch.float32).contiguous()
    N = dist_d.shape[0]
    W = torch.empty(N, k, dtype=torch.float32, device=dist_d.device)
    rho = torch.empty(N, dtype=torch.float64, device=dist_d.device)
    sigma = torch.empty(N, dtype=torch.float64, device=dist_d.device)
    tries = torch.empty(N, dtype=torch.int32, device=dist_d.device)
    nv.umap_smooth_knn(dist_d, nn, smooth_target(nn), W, rho, sigma, tries)
    return W, rho, sigma, tries


class FuzzyGraph(jts.JointP):
    """A = W + W^T - W o W^T in the CSR layout of `tsne.JointP` (rowptr int64 [N + 1], col int32, val float32): row i holds its own
    K neighbours in neighbour order, then the cells that list i without being listed by i, ascending.  Symmetric to the bit."""
    checked = False


def fuzzy_graph(idx, W):
    """`FuzzyGraph` from the lists and their smooth weights (idx int32 [N, k], W float32 [N, k]; device tensors or numpy)."""
    nv.require_gpu()
    idx = torch.as_tensor(idx).to('cuda', torch.int32).contiguous()
    W = torch.as_tensor(W).to(idx.device, torch.float32).contiguous()
    if len(idx.shape) != 2 or tuple(idx.shape) != tuple(W.shape) or not 1 <= idx.shape[1] <= SELF_KNN_MAX:
        raise ValueError(f'umap fuzzy_graph: idx and W must be [cells, k <= {SELF_KNN_MAX}] of one shape')
    N, k = idx.shape
    dev = idx.device
    val = torch.empty(N, k, dtype=torch.float32, device=dev)
    mutual = torch.empty(N, k, dtype=torch.int32, device=dev)
    nv.umap_mutual(idx, W, val, mutual)
    # (as tsne.joint_from_affinities) the pairs (i -> j) that j does not return, sorted by (j, then i)
    pos = torch.nonzero(mutual.view(-1) == 0).view(-1)
    tgt, perm = torch.sort(idx.view(-1)[pos], stable=True)
    rev_pos = pos[perm].contiguous()
    rev_start = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    if rev_pos.numel():
        rev_start[1:] = torch.cumsum(torch.bincount(tgt.long(), minlength=N), dim=0)
    rowptr = torch.arange(N + 1, dtype=torch.int64, device=dev) * k + rev_start
    nnz = N * k + int(rev_pos.numel())
    col = torch.empty(nnz, dtype=torch.int32, device=dev)
    aval = torch.empty(nnz, dtype=torch.float32, device=dev)
    nv.tsne_fill(idx, val, rowptr, rev_pos, tgt.contiguous(), rev_start, col, aval)
    return FuzzyGraph(rowptr, col, aval, N, k)


def edge_schedule(graph, n_epochs):
    """(eps, next) float32 [nnz] device tensors: eps = max(A) / A_e rounded to fp32 once where A_e >= max(A) / n_epochs, else +inf
    (the entry never fires); next starts at eps.  (The quotients are taken in fp64 and rounded: 53 bits are more than twice 24 plus
    2, so the result is the correctly rounded fp32 quotient.)"""
    n_epochs = int(n_epochs)
    if n_epochs < 1:
        raise ValueError(f'umap edge_schedule: n_epochs = {n_epochs}; at least 1')
    val = graph.val
    if val.numel() == 0:
        return val.clone(), val.clone()
    top = val.max().double()
    keep = val >= (top / float(n_epochs)).float()
    eps = torch.where(keep, (top / val.double()).float(), torch.full_like(val, float('inf')))
    return eps, eps.clone()


def _check_graph(graph, Y, what):
    if tuple(Y.shape) != (graph.n, 2) or Y.dtype != torch.float32 or not Y.is_contiguous():
        raise ValueError(f'{what}: the layout must be contiguous float32 [{graph.n}, 2], got {Y.dtype} {tuple(Y.shape)}')
    if not getattr(graph, 'checked', False):                 # once per graph: the kernel skips such an entry, it cannot refuse it
        if graph.col.numel() and (int(graph.col.min()) < 0 or int(graph.col.max()) >= graph.n):
            raise ValueError(f'{what}: the graph has a column outside [0, {graph.n})')
        graph.checked = True


def epoch(graph, Y_in, Y_out, eps, nxt, n, alpha, a, b, repulsion_strength=1.0, negative_sample_rate=5, seed=0, delta=None,
          fired=None, fired_total=None):
    """Epoch `n` of DESIGN.md §20 in one launch: reads the layout Y_in, writes Y_out (two float32 [N, 2] device tensors), advances
    `nxt` in place.  Optional outputs: delta float32 [N, 2] (the move before alpha), fired int32 [N] (the firing entries per row),
    fired_total int64 [N] (the same count added to it)."""
    nv.require_gpu()
    _check_graph(graph, Y_in, 'umap epoch')
    _check_graph(graph, Y_out, 'umap epoch')
    if Y_in.data_ptr() == Y_out.data_ptr():
        raise ValueError('umap epoch: Y_in and Y_out must be two buffers')
    if eps.numel() != graph.col.numel() or nxt.numel() != graph.col.numel():
        raise ValueError('umap epoch: eps and next must have one entry per entry of the graph')
    nv.umap_epoch(graph.rowptr, graph.col, eps, nxt, Y_in, Y_out, n, alpha, a, b, repulsion_strength, negative_sample_rate, seed,
                  delta, fired, fired_total)


def optimize(graph, Y, eps, nxt, n_epochs, learning_rate, a, b, repulsion_strength=1.0, negative_sample_rate=5, seed=0, first=0,
             count=None, fired_total=None):
    """Epochs first .. first + count - 1 (default: all the rest) of an n_epochs schedule from the layout Y (float32 [N, 2] device
    tensor, left unchanged): the layout after them, a new tensor.  `nxt` advances in place.  Nothing is read back: the host does
    not wait between the first and the last epoch."""
    _check_graph(graph, Y, 'umap optimize')
    count = n_epochs - first if count is None else int(count)
    bufs = [Y.clone(), torch.empty_like(Y)]
    for t in range(count):
        n = first + t
        epoch(graph, bufs[t & 1], bufs[(t + 1) & 1], eps, nxt, n, alpha_of(learning_rate, n, n_epochs), a, b, repulsion_strength,
              negative_sample_rate, seed, fired_total=fired_total)
    return bufs[count & 1]


def umap(embeddings, n_neighbors=15, min_dist=0.1, spread=1.0, n_epochs=None, learning_rate=1.0, negative_sample_rate=5,
         repulsion_strength=1.0, init='pca', seed=0, a=None, b=None, return_graph=False, device='cuda'):
    """UMAP of M embeddings [N_m, L] pooled into one set of cells:

        layout                      one float32 [N_m, 2] array per embedding
        a, b                        the curve 1 / (1 + a d^(2b)) (fitted to min_dist and spread unless given)
        n_epochs, n_neighbors       the epochs run (default 500 up to 10 000 cells, else 200) and the list length
        n_edges                     stored entries of the fuzzy graph (both directions)
        n_fired                     entries fired over all epochs
        graph                       the fuzzy graph as scipy CSR float32 (`return_graph`), else None

    `init`: 'pca', 'random' (from `seed`) or an array [N, 2].  Bit-identical from run to run."""
    checked = check_umap(embeddings, n_neighbors, min_dist, spread, n_epochs, learning_rate, negative_sample_rate, repulsion_strength,
                         init, a, b, 'umap')
    return umap_checked(embeddings, *checked, seed, return_graph, device)


def umap_checked(embeddings, n_neighbors, n_epochs, learning_rate, negative_sample_rate, repulsion_strength, init, a, b, seed,
                 return_graph=False, device='cuda'):
    """`umap` behind its argument checks: the arguments are what `check_umap` returned (JAMIE.umap has run it for both routes)."""
    n_cells = [_n_rows(e) for e in embeddings]
    _, x = _pool(embeddings, device, 'umap')
    y0 = initial_layout(x.cpu().numpy() if isinstance(init, str) and init == 'pca' else np.empty((x.shape[0], 0)), init, seed)
    idx, dist = self_knn(x, n_neighbors - 1, device)
    W, _, _, _ = smooth_knn(idx, dist, n_neighbors)
    del dist
    G = fuzzy_graph(idx, W)
    del idx, W
    eps, nxt = edge_schedule(G, n_epochs)
    total = torch.zeros(G.n, dtype=torch.int64, device=x.device)
    Y = optimize(G, torch.from_numpy(y0).to(x.device), eps, nxt, n_epochs, learning_rate, a, b, repulsion_strength,
                 negative_sample_rate, seed, fired_total=total)
    graph = G.to_scipy() if return_graph else None
    return umap_summary(Y.cpu().numpy(), n_cells, a, b, n_epochs, n_neighbors, G.col.numel(), int(total.sum().item()), graph)

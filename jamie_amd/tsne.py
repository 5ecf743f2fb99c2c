"""t-SNE layout of the pooled cells on the MI355X with the exact gradient, without an N x N matrix.

    affinities(idx, dist, perplexity)              conditional affinities on neighbour lists: (C fp32 [N, K], beta, tries)
    joint_probabilities(idx, dist, perplexity)     P = (C + C^T) / (2N) as a CSR matrix on the device (`JointP`)
    gradient(P, Y, exaggeration, seg_rows)         (grad fp32 [N, 2], Z, KL) at a layout Y: for tests and for other optimisers
    tsne(embeddings)                               JAMIE.tsne on the device: the layout of M embeddings pooled into one set of cells

The kernels are in csrc/tsne.hip (include/jamie_hip.h, "Layout on the device").  The neighbours are `neighbors.self_knn`'s, at
most 128 per cell, so with the default n_neighbors = int(3 perplexity) the perplexity stays below 43.  Device memory is the input
plus O(N K).  The definition (shared with the float64 host route of jamie.py) is DESIGN.md §19.
"""
import numpy as np
import torch

from . import _native as nv
from .clustering import _check_seg_rows, check_finite
from .neighbors import _n_rows, _pool, check_perplexity, self_knn

MAX_TRIES = 100        # of the perplexity solve
ENTROPY_TOL = 1e-5
INIT_STD = 1e-4


# ---- the argument checks and the definitions both routes share ----
def check_tsne(embeddings, perplexity, n_neighbors, n_iter, early_exaggeration, exaggeration_iter, learning_rate, init, log_every,
               what):
    """The checks of JAMIE.tsne in their order; (perplexity, k, n_iter, early_exaggeration, exaggeration_iter, learning_rate,
    init, log_every) with learning_rate 'auto' resolved to max(N / early_exaggeration / 4, 50) and an array init as float32
    [N, 2].  Nothing is allocated on a device."""
    if len(embeddings) < 1:
        raise ValueError(f'{what}: no embeddings')
    for e in embeddings:
        if len(e.shape) != 2 or e.shape[1] != embeddings[0].shape[1] or e.shape[1] < 1:
            raise ValueError(f'{what}: the embeddings must be [cells, features] with the same features')
    N = int(sum(int(e.shape[0]) for e in embeddings))
    perplexity, k = check_perplexity(perplexity, n_neighbors, N, what)     # (1 < perplexity < k: at least 2 neighbours, 3 cells)
    n_iter, exaggeration_iter, log_every = int(n_iter), int(exaggeration_iter), int(log_every)
    early_exaggeration = float(early_exaggeration)
    if n_iter < 1:
        raise ValueError(f'{what}: n_iter = {n_iter}; at least 1')
    if not 0 <= exaggeration_iter <= n_iter:
        raise ValueError(f'{what}: exaggeration_iter = {exaggeration_iter}; 0 <= exaggeration_iter <= n_iter = {n_iter}')
    if not early_exaggeration >= 1.0 or not np.isfinite(early_exaggeration):
        raise ValueError(f'{what}: early_exaggeration = {early_exaggeration}; at least 1')
    if isinstance(learning_rate, str):
        if learning_rate != 'auto':
            raise ValueError(f"{what}: learning_rate must be a positive number or 'auto', not {learning_rate!r}")
        learning_rate = max(N / early_exaggeration / 4.0, 50.0)
    learning_rate = float(learning_rate)
    if not learning_rate > 0.0 or not np.isfinite(learning_rate):
        raise ValueError(f'{what}: learning_rate = {learning_rate}; it must be positive')
    if log_every < 1:
        raise ValueError(f'{what}: log_every = {log_every}; at least 1')
    if isinstance(init, str):
        if init not in ('pca', 'random'):
            raise ValueError(f"{what}: init must be 'pca', 'random' or an array [cells, 2], not {init!r}")
    else:
        init = np.asarray(init.detach().cpu().numpy() if torch.is_tensor(init) else init, dtype=np.float32)
        if init.shape != (N, 2):
            raise ValueError(f'{what}: init must be [{N}, 2], got {init.shape}')
        if not np.isfinite(init).all():
            raise ValueError(f'{what}: init contains NaN or infinity')
    check_finite(embeddings, what)
    return perplexity, k, n_iter, early_exaggeration, exaggeration_iter, learning_rate, init, log_every


def initial_layout(X, init, seed):
    """Y_0 float32 [N, 2] from the pooled cells X (numpy [N, L]): 'pca' -- the scores on the two leading eigenvectors of the
    L x L covariance in float64 (each eigenvector with its largest-magnitude entry positive), scaled so that the first column has
    standard deviation 1e-4; 'random' -- `default_rng(seed).standard_normal((N, 2)) * 1e-4`; an array is taken as it is.  One
    function for both routes: they start from identical bits."""
    N = len(X)
    if not isinstance(init, str):
        return np.ascontiguousarray(init, dtype=np.float32).copy()
    if init == 'random':
        return (np.random.default_rng(seed).standard_normal((N, 2)) * INIT_STD).astype(np.float32)
    X = np.asarray(X, dtype=np.float64)
    Xc = X - X.mean(axis=0)
    _, vecs = np.linalg.eigh(Xc.T @ Xc / max(N - 1, 1))                  # ascending eigenvalues
    V = np.zeros((X.shape[1], 2))
    lead = vecs[:, ::-1][:, :2]
    V[:, :lead.shape[1]] = lead
    for c in range(lead.shape[1]):
        r = int(np.argmax(np.abs(V[:, c])))
        if V[r, c] < 0:
            V[:, c] = -V[:, c]
    Y = Xc @ V
    sd = float(np.std(Y[:, 0]))
    return (Y * (INIT_STD / sd if sd > 0 else 0.0)).astype(np.float32)


def schedule(n_iter, exaggeration_iter, early_exaggeration, log_every):
    """([(alpha, momentum)] per iteration, logged_at): the KL and the gradient norm are taken at the layout after `t` iterations
    for every t in logged_at: the multiples of log_every below n_iter, and n_iter.  The gradient there is the one the next
    iteration uses (alpha = 1 after the last)."""
    phases = [(early_exaggeration, 0.5) if t < exaggeration_iter else (1.0, 0.8) for t in range(n_iter)]
    logged_at = [t for t in range(log_every, n_iter, log_every)] + [n_iter]
    return phases, logged_at


def tsne_summary(Y, n_cells, kl_history, gsq_history, logged_at, k, learning_rate, n_iter):
    """The dict of JAMIE.tsne (shared by the device and the host route)."""
    kl_history = np.asarray(kl_history, dtype=np.float64)
    return {'layout': np.split(np.asarray(Y, dtype=np.float32), np.cumsum(n_cells)[:-1]), 'kl': float(kl_history[-1]),
            'kl_history': kl_history, 'grad_norm_history': np.sqrt(np.asarray(gsq_history, dtype=np.float64)),
            'logged_at': np.asarray(logged_at, dtype=np.int64), 'n_neighbors': int(k), 'learning_rate': float(learning_rate),
            'n_iter': int(n_iter)}


# ---- the device route ----
def _lists(idx, dist, perplexity, what):
    nv.require_gpu()
    if len(idx.shape) != 2 or tuple(idx.shape) != tuple(dist.shape):
        raise ValueError(f'{what}: idx and dist must be [cells, k] of one shape, got {tuple(idx.shape)} and {tuple(dist.shape)}')
    k = int(idx.shape[1])
    if k < 2 or k > 128:
        raise ValueError(f'{what}: k = {k}; 2 <= k <= 128')
    perplexity = float(perplexity)
    if not 1.0 < perplexity < k:
        raise ValueError(f'{what}: perplexity = {perplexity}; 1 < perplexity < k = {k}')
    idx_d = torch.as_tensor(idx).to('cuda', torch.int32).contiguous()
    dist_d = torch.as_tensor(dist).to(idx_d.device, torch.float32).contiguous()
    return idx_d, dist_d, perplexity


def affinities(idx, dist, perplexity):
    """Conditional affinities of every cell over its neighbour list (idx int32 [N, k], dist float32 [N, k] ascending: `self_knn`):
    (C float32 [N, k] with rows summing to 1, beta float64 [N], tries int32 [N]) device tensors.  One fp64 solve per cell for the
    beta at which the entropy of P_j = exp(-beta (d_j^2 - d_1^2)) / s is log(perplexity) within 1e-5 (at most 100 tries)."""
    idx_d, dist_d, perplexity = _lists(idx, dist, perplexity, 'affinities')
    N, k = idx_d.shape
    C = torch.empty(N, k, dtype=torch.float32, device=idx_d.device)
    beta = torch.empty(N, dtype=torch.float64, device=idx_d.device)
    tries = torch.empty(N, dtype=torch.int32, device=idx_d.device)
    nv.tsne_affinities(dist_d, perplexity, C, beta, tries)
    return C, beta, tries


class JointP:
    """P = (C + C^T) / (2N) in CSR form on the device: rowptr int64 [N + 1], col int32, val float32.  Row i holds its own k
    neighbours in neighbour order, then the cells that list i without being listed by i, in ascending index."""

    def __init__(self, rowptr, col, val, n, k):
        self.rowptr, self.col, self.val, self.n, self.k = rowptr, col, val, int(n), int(k)

    def to_scipy(self):
        from scipy.sparse import csr_matrix
        return csr_matrix((self.val.cpu().numpy(), self.col.cpu().numpy(), self.rowptr.cpu().numpy()), shape=(self.n, self.n))


def joint_from_affinities(idx, C):
    """`JointP` from the lists and their conditional affinities (device tensors idx int32 [N, k], C float32 [N, k])."""
    N, k = idx.shape
    dev = idx.device
    val = torch.empty(N, k, dtype=torch.float32, device=dev)
    mutual = torch.empty(N, k, dtype=torch.int32, device=dev)
    nv.tsne_mutual(idx, C, val, mutual)
    # the pairs (i -> j) that j does not return, sorted by (j, then i): the flat positions ascend with i, and the sort is stable
    pos = torch.nonzero(mutual.view(-1) == 0).view(-1)
    tgt, perm = torch.sort(idx.view(-1)[pos], stable=True)
    rev_pos = pos[perm].contiguous()
    rev_start = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    if rev_pos.numel():
        rev_start[1:] = torch.cumsum(torch.bincount(tgt.long(), minlength=N), dim=0)
    rowptr = torch.arange(N + 1, dtype=torch.int64, device=dev) * k + rev_start
    nnz = N * k + int(rev_pos.numel())
    col = torch.empty(nnz, dtype=torch.int32, device=dev)
    pval = torch.empty(nnz, dtype=torch.float32, device=dev)
    nv.tsne_fill(idx, val, rowptr, rev_pos, tgt.contiguous(), rev_start, col, pval)
    return JointP(rowptr, col, pval, N, k)


def joint_probabilities(idx, dist, perplexity):
    """P = (C + C^T) / (2N) of the conditional affinities C of `affinities`, as a `JointP`: every ordered pair (i, j) with j in
    the list of i or i in the list of j once, a missing direction counting as 0; symmetric to the bit."""
    idx_d, dist_d, perplexity = _lists(idx, dist, perplexity, 'joint_probabilities')
    C, _, _ = affinities(idx_d, dist_d, perplexity)
    return joint_from_affinities(idx_d, C)


class _Gradient:
    """The buffers of one gradient evaluation on N points, allocated once."""

    def __init__(self, N, dev, seg_rows):
        self.R = torch.empty(N, 2, dtype=torch.float64, device=dev)
        self.z = torch.empty(N, dtype=torch.float64, device=dev)
        self.Z = torch.empty(1, dtype=torch.float64, device=dev)
        self.ws_rep = torch.empty(nv.tsne_repulsion_workspace(N, seg_rows), dtype=torch.uint8, device=dev)
        self.ws_step = torch.empty(nv.tsne_step_workspace(N), dtype=torch.uint8, device=dev)
        self.seg_rows = seg_rows


def gradient(P, Y, exaggeration=1.0, seg_rows=0, return_parts=False):
    """The t-SNE gradient at the layout Y [N, 2] under the joint probabilities P (`JointP`): (grad float32 [N, 2] device tensor,
    Z, KL), grad_i = 4 (exaggeration A_i - R_i / Z); KL with the unexaggerated P.  `return_parts`: also a dict of the device
    tensors A, R (float64 [N, 2]) and z (float64 [N]).  `seg_rows`: columns per segment of the all-pairs pass (0: the library's
    choice; else a multiple of 128); the last bits may depend on it."""
    nv.require_gpu()
    seg_rows = _check_seg_rows(seg_rows, 'gradient')
    if float(exaggeration) < 1.0:
        raise ValueError(f'gradient: exaggeration = {exaggeration}; at least 1')
    y = torch.as_tensor(Y).to(P.val.device, torch.float32).contiguous().clone()
    if tuple(y.shape) != (P.n, 2):
        raise ValueError(f'gradient: Y must be [{P.n}, 2], got {tuple(y.shape)}')
    buf = _Gradient(P.n, y.device, seg_rows)
    grad = torch.empty(P.n, 2, dtype=torch.float32, device=y.device)
    A = torch.empty(P.n, 2, dtype=torch.float64, device=y.device)
    log = torch.empty(2, dtype=torch.float64, device=y.device)
    nv.tsne_repulsion(y, buf.R, buf.z, buf.Z, buf.ws_rep, seg_rows)
    nv.tsne_step(P.rowptr, P.col, P.val, y, buf.R, buf.Z, exaggeration, 0.0, 1.0, None, None, False, buf.ws_step, grad=grad, A=A,
                 kl=log[0:1], gsq=log[1:2])
    out = (grad, float(buf.Z.item()), float(log[0].item()))
    return out + ({'A': A, 'R': buf.R, 'z': buf.z},) if return_parts else out


def descend(P, Y, u, gain, phases, learning_rate, logged_at=(), seg_rows=0):
    """Run len(phases) iterations in place on the device tensors Y, u, gain (float32 [N, 2]); phases: (alpha, momentum) per
    iteration.  Returns the device history float64 [2, len(logged_at)] (KL, squared gradient norm) at the layouts after t
    iterations, t in logged_at.  Nothing is read back: the host does not wait between the first and the last iteration."""
    N = P.n
    buf = _Gradient(N, Y.device, seg_rows)
    logged_at = list(logged_at)
    hist = torch.zeros(2, max(len(logged_at), 1), dtype=torch.float64, device=Y.device)
    slot = {t: s for s, t in enumerate(logged_at)}
    for t, (alpha, momentum) in enumerate(phases):
        nv.tsne_repulsion(Y, buf.R, buf.z, buf.Z, buf.ws_rep, seg_rows)
        s = slot.get(t)
        nv.tsne_step(P.rowptr, P.col, P.val, Y, buf.R, buf.Z, alpha, momentum, learning_rate, u, gain, True, buf.ws_step,
                     kl=None if s is None else hist[0, s:s + 1], gsq=None if s is None else hist[1, s:s + 1])
    s = slot.get(len(phases))
    if s is not None:
        nv.tsne_repulsion(Y, buf.R, buf.z, buf.Z, buf.ws_rep, seg_rows)
        nv.tsne_step(P.rowptr, P.col, P.val, Y, buf.R, buf.Z, 1.0, 0.0, learning_rate, None, None, False, buf.ws_step,
                     kl=hist[0, s:s + 1], gsq=hist[1, s:s + 1])
    return hist


def tsne(embeddings, perplexity=30, n_neighbors=None, n_iter=1000, early_exaggeration=12.0, exaggeration_iter=250,
         learning_rate='auto', init='pca', seed=0, log_every=50, device='cuda', seg_rows=0):
    """t-SNE of M embeddings [N_m, L] pooled into one set of cells, with the exact gradient:

        layout                      one float32 [N_m, 2] array per embedding
        kl, kl_history              the Kullback-Leibler divergence after the last iteration, and at every layout of `logged_at`
        grad_norm_history           the 2-norm of the gradient there
        logged_at                   iterations completed at each entry: the multiples of log_every below n_iter, and n_iter
        n_neighbors, learning_rate, n_iter    the k used (default min(int(3 perplexity), N - 1), at most 128: a perplexity below
                                    43 with the default), the step ('auto': max(N / early_exaggeration / 4, 50)), the iterations

    sklearn's schedule: exaggeration `early_exaggeration` and momentum 0.5 for the first `exaggeration_iter` iterations, then 1
    and 0.8; gains as `_gradient_descent`; no recentring, no early stop.  `init`: 'pca', 'random' (from `seed`) or an array
    [N, 2].  Bit-identical from run to run at the same `seg_rows` (0: the library's choice; else a multiple of 128)."""
    seg_rows = _check_seg_rows(seg_rows, 'tsne')
    checked = check_tsne(embeddings, perplexity, n_neighbors, n_iter, early_exaggeration, exaggeration_iter, learning_rate, init,
                         log_every, 'tsne')
    return tsne_checked(embeddings, *checked, seed, device, seg_rows)


def tsne_checked(embeddings, perplexity, k, n_iter, early_exaggeration, exaggeration_iter, learning_rate, init, log_every, seed,
                 device, seg_rows):
    """`tsne` behind its argument checks: the arguments are what `check_tsne` returned (JAMIE.tsne has run it for both routes)."""
    n_cells = [_n_rows(e) for e in embeddings]
    _, x = _pool(embeddings, device, 'tsne')
    y0 = initial_layout(x.cpu().numpy() if isinstance(init, str) and init == 'pca' else np.empty((x.shape[0], 0)), init, seed)
    idx, dist = self_knn(x, k, device)
    C, _, _ = affinities(idx, dist, perplexity)
    del dist
    P = joint_from_affinities(idx, C)
    del idx, C
    Y = torch.from_numpy(y0).to(x.device)
    u = torch.zeros_like(Y)
    gain = torch.ones_like(Y)
    phases, logged_at = schedule(n_iter, exaggeration_iter, early_exaggeration, log_every)
    hist = descend(P, Y, u, gain, phases, learning_rate, logged_at, seg_rows).cpu().numpy()
    return tsne_summary(Y.cpu().numpy(), n_cells, hist[0], hist[1], logged_at, k, learning_rate, n_iter)

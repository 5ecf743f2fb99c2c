"""Spectral embedding and diffusion map of the pooled cells on the MI355X: the leading eigenvectors of the normalised fuzzy graph
by Chebyshev-filtered subspace iteration, O(nnz + N B) memory.

    check_spectral(embeddings, ...)                the argument checks of JAMIE.spectral, for both routes
    normalised_operator(graph, density_normalize)  (scale, degree) fp64 [N]: S = diag(scale) A diag(scale)
    apply(graph, scale, X), cheb_step(...)         S X, and one step out = alpha S in + gamma in - beta prev, in one launch
    gram(Y, Z), rotate(Y1, M1, Y2, M2)             Y^T Z [B, B] and Y1 M1 (+ Y2 M2) on [N, B] fp64 blocks
    orthonormalise(Y), rayleigh_ritz(graph, s, X)  the two host-side B x B eigenproblems around them
    eigen(graph, scale, k, ...)                    the k largest eigenpairs of S
    spectral(embeddings)                           JAMIE.spectral on the device
    umap_init(vectors), pseudotime(out, root)      host float64 on the returned vectors, shared by both routes

The kernels are in csrc/spectral.hip (include/jamie_hip.h, "Spectral embedding on the device").  The graph is `umap.fuzzy_graph`'s
on `neighbors.self_knn`'s lists, exactly as `umap.umap` builds it.  The definition (shared with the float64 host route of
jamie.py) is DESIGN.md §21.
"""
import math

import numpy as np
import torch

from . import _native as nv
from . import umap as jum
from .clustering import check_finite
from .neighbors import SELF_KNN_MAX, _n_rows, _pool, self_knn

KINDS = ('laplacian', 'diffmap')
MAX_COMPONENTS = 27
AMPLIFICATION = 2.0e6      # between the wanted and the damped end of one filter
GAP_FLOOR = 1e-6           # the damped interval ends at 1 - GAP_FLOOR at the latest
CLAMP = 2.0 ** -40         # eigenvalues of a Gram matrix below CLAMP of its largest are raised to it


# ---- the argument checks and the definitions both routes share ----
def block_width(k):
    """Columns of the iterated block for k wanted eigenpairs."""
    return 16 if k <= 12 else 32


def check_spectral(embeddings, n_components=2, n_neighbors=15, kind='laplacian', density_normalize=None, tol=1e-8, max_iter=100,
                   max_degree=60, what='spectral'):
    """The checks of JAMIE.spectral in their order; (n_components, n_neighbors, kind, density_normalize, tol, max_iter,
    max_degree) with density_normalize None resolved to kind == 'diffmap'.  Nothing is allocated on a device."""
    if len(embeddings) < 1:
        raise ValueError(f'{what}: no embeddings')
    for e in embeddings:
        if len(e.shape) != 2 or e.shape[1] != embeddings[0].shape[1] or e.shape[1] < 1:
            raise ValueError(f'{what}: the embeddings must be [cells, features] with the same features')
    if kind not in KINDS:
        raise ValueError(f"{what}: kind must be 'laplacian' or 'diffmap', not {kind!r}")
    nc = int(n_components)
    if nc < 1 or nc > MAX_COMPONENTS or nc != n_components:
        raise ValueError(f'{what}: n_components = {n_components}; an integer in 1 .. {MAX_COMPONENTS}')
    N = int(sum(int(e.shape[0]) for e in embeddings))
    B = block_width(nc + 1)
    if N < B:
        raise ValueError(f'{what}: {N} cells; n_components = {nc} iterates a block of {B} vectors and needs at least {B} cells')
    nn = int(n_neighbors)
    if nn < 2 or nn > min(N, SELF_KNN_MAX + 1):
        raise ValueError(f'{what}: n_neighbors = {nn}; 2 <= n_neighbors <= min(cells = {N}, {SELF_KNN_MAX + 1})')
    tol = float(tol)
    if not 0.0 < tol < 1.0:
        raise ValueError(f'{what}: tol = {tol}; 0 < tol < 1')
    max_iter, max_degree = int(max_iter), int(max_degree)
    if max_iter < 1:
        raise ValueError(f'{what}: max_iter = {max_iter}; at least 1')
    if max_degree < 2:
        raise ValueError(f'{what}: max_degree = {max_degree}; at least 2')
    check_finite(embeddings, what)
    dn = (kind == 'diffmap') if density_normalize is None else bool(density_normalize)
    return nc, nn, kind, dn, tol, max_iter, max_degree


def check_degree(degree, what='spectral'):
    """Refuses a cell whose degree is 0 or not finite (float64 numpy)."""
    bad = ~(np.isfinite(degree) & (degree > 0))
    if bad.any():
        raise ValueError(f'{what}: cell {int(np.nonzero(bad)[0][0])} has degree {degree[bad][0]}; every cell needs a positive finite '
                         'degree')


def filter_plan(theta, max_degree):
    """(p, e, c, sigma1) of the filter after a Rayleigh-Ritz step with Ritz values `theta` (descending, B of them): the damped
    interval [-1, a], a = min(theta_B, 1 - 1e-6), has half-width e and centre c; top = max(theta_1, 1); the degree p is the
    smallest at which the Chebyshev polynomial at `top` exceeds 2 10^6, clamped to 2 .. max_degree."""
    a = min(float(theta[-1]), 1.0 - GAP_FLOOR)
    e, c = (a + 1.0) / 2.0, (a - 1.0) / 2.0
    top = max(float(theta[0]), 1.0)
    t = (top - c) / e
    rho = t + math.sqrt(t * t - 1.0)
    p = int(min(max(math.ceil(math.log(AMPLIFICATION) / math.log(rho)), 2), max_degree))
    return p, e, c, e / (top - c)


def filter_coefficients(p, e, c, sigma1):
    """[(alpha, gamma, beta)] of the p steps Y_j = alpha S Y_(j-1) + gamma Y_(j-1) - beta Y_(j-2) (beta = 0 in the first)."""
    steps = [(sigma1 / e, -(sigma1 / e) * c, 0.0)]
    sigma = sigma1
    for _ in range(1, p):
        nxt = 1.0 / (2.0 / sigma1 - sigma)
        steps.append((2.0 * nxt / e, -(2.0 * nxt / e) * c, sigma * nxt))
        sigma = nxt
    return steps


def ritz(H):
    """(theta descending, V) of the symmetrised B x B matrix H, float64 numpy."""
    w, V = np.linalg.eigh((H + H.T) / 2.0)
    order = np.argsort(-w, kind='stable')
    return w[order], np.ascontiguousarray(V[:, order])


def whitening(G):
    """M with (Y M)^T (Y M) = I for the Gram matrix G = Y^T Y (float64 numpy [B, B]): the columns are scaled to unit norm, the
    scaled G symmetrised, its eigenvalues clamped at 2^-40 of the largest, M = D U w^-1/2."""
    d = 1.0 / np.sqrt(np.diag(G))
    Gs = G * d[:, None] * d[None, :]
    w, U = np.linalg.eigh((Gs + Gs.T) / 2.0)
    w = np.maximum(w, w.max() * CLAMP)
    return np.ascontiguousarray(d[:, None] * (U / np.sqrt(w)[None, :]))


def fix_signs(Q):
    """Every column's entry of largest magnitude made positive (the lowest index on ties)."""
    Q = np.array(Q, dtype=np.float64)
    at = np.argmax(np.abs(Q), axis=0)                        # (the first maximum)
    flip = Q[at, np.arange(Q.shape[1])] < 0
    Q[:, flip] = -Q[:, flip]
    return Q


def start_block(degree, B, seed):
    """X_0 float64 [N, B]: column 0 the square root of the degree, the others standard normal draws of `seed`."""
    N = len(degree)
    X = np.empty((N, B))
    X[:, 0] = np.sqrt(degree)
    X[:, 1:] = np.random.default_rng(seed).standard_normal((N, B - 1))
    return X


def umap_init(vectors):
    """Columns q_2, q_3 of the pooled vectors [N, k >= 2] mapped per column onto [0, 10] in float64 (a constant column, and a
    missing q_3, become 5), float32 [N, 2]: `umap.initial_layout`'s mapping, usable as `JAMIE.umap(init=...)`."""
    Q = np.asarray(vectors, dtype=np.float64)
    Y = np.zeros((len(Q), 2))
    take = min(2, Q.shape[1] - 1)
    Y[:, :take] = Q[:, 1:1 + take]
    lo, hi = Y.min(axis=0), Y.max(axis=0)
    span = np.where(hi > lo, hi - lo, 1.0)
    return np.where(hi > lo, jum.INIT_SPAN * (Y - lo) / span, jum.INIT_SPAN / 2).astype(np.float32)


def pseudotime(out, root):
    """Diffusion pseudotime from cell `root` (an index into the pooled cells) on the truncated basis of a `spectral` result:
    sqrt(sum_{l >= 2} (theta_l / (1 - theta_l))^2 (q_l(x) - q_l(root))^2), float64 [N] (scanpy's DPT).  Refuses a graph whose
    second eigenvalue is within 10 tol of 1 (it is not connected)."""
    Q = np.concatenate(out['vectors'], axis=0)
    theta = np.asarray(out['eigenvalues'], dtype=np.float64)
    root = int(root)
    if root < 0 or root >= len(Q):
        raise ValueError(f'spectral pseudotime: root = {root} outside [0, {len(Q)})')
    if len(theta) < 2 or theta[1] >= 1.0 - 10.0 * float(out['tol']):
        raise ValueError(f'spectral pseudotime: the second eigenvalue is {theta[1] if len(theta) > 1 else None}; the graph is not '
                         'connected')
    wgt = theta[1:] / (1.0 - theta[1:])
    diff = Q[:, 1:] - Q[root, 1:][None, :]
    return np.sqrt(np.sum((wgt[None, :] * diff) ** 2, axis=1))


def spectral_summary(Q, theta, resid, degree, n_cells, converged, iterations, applies, degrees, n_neighbors, n_edges, kind,
                     density_normalize, tol, graph):
    """The dict of JAMIE.spectral (shared by the device and the host route)."""
    Q = fix_signs(Q)
    cuts = np.cumsum(n_cells)[:-1]
    return {'vectors': np.split(Q, cuts), 'embedding': [np.ascontiguousarray(v[:, 1:]) for v in np.split(Q, cuts)],
            'eigenvalues': np.asarray(theta, dtype=np.float64), 'residuals': np.asarray(resid, dtype=np.float64),
            'degree': np.split(np.asarray(degree, dtype=np.float64), cuts), 'umap_init': umap_init(Q), 'converged': bool(converged),
            'iterations': int(iterations), 'applies': int(applies), 'degrees': [int(p) for p in degrees],
            'n_neighbors': int(n_neighbors), 'n_edges': int(n_edges), 'kind': kind, 'density_normalize': bool(density_normalize),
            'tol': float(tol), 'graph': graph}


# ---- the device route ----
def _check_graph(graph, what):
    if not getattr(graph, 'checked', False):                 # once per graph: the kernel skips such an entry, it cannot refuse it
        if graph.col.numel() and (int(graph.col.min()) < 0 or int(graph.col.max()) >= graph.n):
            raise ValueError(f'{what}: the graph has a column outside [0, {graph.n})')
        graph.checked = True


def _check_block(n, X, what):
    if (not torch.is_tensor(X) or X.dtype != torch.float64 or len(X.shape) != 2 or X.shape[0] != n or X.shape[1] not in (16, 32)
            or not X.is_contiguous()):
        raise ValueError(f'{what}: a block must be a contiguous float64 [{n}, 16 or 32] device tensor, got '
                         f'{getattr(X, "dtype", type(X))} {tuple(getattr(X, "shape", ()))}')


def _check_vector(n, v, what):
    if not torch.is_tensor(v) or v.dtype != torch.float64 or tuple(v.shape) != (n,) or not v.is_contiguous():
        raise ValueError(f'{what}: one contiguous float64 value per cell ([{n}]) is needed, got {getattr(v, "dtype", type(v))} '
                         f'{tuple(getattr(v, "shape", ()))}')


def _square(M, B, dev, what):
    M = torch.as_tensor(M, dtype=torch.float64).to(dev).contiguous()
    if tuple(M.shape) != (B, B):
        raise ValueError(f'{what}: the matrix must be [{B}, {B}], got {tuple(M.shape)}')
    return M


def rowsum(graph, w=None):
    """sum_j A_ij w_j (w = 1 when None) as a float64 [N] device tensor."""
    nv.require_gpu()
    _check_graph(graph, 'spectral rowsum')
    if w is not None:
        _check_vector(graph.n, w, 'spectral rowsum')
    out = torch.empty(graph.n, dtype=torch.float64, device=graph.col.device)
    nv.graph_rowsum(graph.rowptr, graph.col, graph.val, w, out)
    return out


def normalised_operator(graph, density_normalize=False):
    """(scale, degree) float64 [N] device tensors of S = diag(scale) A diag(scale).  Plain: degree d = A 1, scale = d^-1/2.
    Density-normalised (scanpy's alpha = 1): A' = A / (d_i d_j), degree d' = A' 1, scale = d^-1 d'^-1/2.  The square root of
    `degree` is the eigenvector of eigenvalue 1.  A cell of degree 0 (or not finite) is refused."""
    d = rowsum(graph)
    check_degree(d.cpu().numpy())
    if not density_normalize:
        return 1.0 / torch.sqrt(d), d
    inv = 1.0 / d
    d2 = rowsum(graph, inv) * inv
    check_degree(d2.cpu().numpy())
    return inv / torch.sqrt(d2), d2


def cheb_step(graph, scale, X, prev, out, alpha, gamma, beta):
    """out = alpha S X + gamma X - beta prev in one launch (prev None: no last term; out may be prev, never X)."""
    nv.require_gpu()
    _check_graph(graph, 'spectral cheb_step')
    _check_vector(graph.n, scale, 'spectral cheb_step')
    for t in (X, out) + (() if prev is None else (prev,)):
        _check_block(graph.n, t, 'spectral cheb_step')
    if out.shape != X.shape or (prev is not None and prev.shape != X.shape):
        raise ValueError('spectral cheb_step: the blocks must have one shape')
    if out.data_ptr() == X.data_ptr() or (prev is not None and prev.data_ptr() == X.data_ptr()):
        raise ValueError('spectral cheb_step: the input block must differ from out and prev')
    nv.graph_cheb_step(graph.rowptr, graph.col, graph.val, scale, X, prev, out, alpha, gamma, beta)
    return out


def apply(graph, scale, X, out=None):
    """S X."""
    out = torch.empty_like(X) if out is None else out
    return cheb_step(graph, scale, X, None, out, 1.0, 0.0, 0.0)


def gram(Y, Z, ws=None):
    """Y^T Z as a float64 [B, B] device tensor; bit-identical from run to run."""
    nv.require_gpu()
    _check_block(Y.shape[0], Y, 'spectral gram')
    _check_block(Y.shape[0], Z, 'spectral gram')
    if Z.shape != Y.shape:
        raise ValueError('spectral gram: the blocks must have one shape')
    N, B = Y.shape
    if ws is None or ws.dtype != torch.float64 or ws.numel() * 8 < nv.block_gram_workspace(N, B):
        ws = torch.empty(nv.block_gram_workspace(N, B) // 8, dtype=torch.float64, device=Y.device)
    out = torch.empty(B, B, dtype=torch.float64, device=Y.device)
    nv.block_gram(Y, Z, ws, out)
    return out


def rotate(Y1, M1, Y2=None, M2=None, out=None):
    """Y1 M1 (+ Y2 M2): M float64 [B, B] (numpy or device tensors)."""
    nv.require_gpu()
    N, B = Y1.shape[0], Y1.shape[1]
    _check_block(N, Y1, 'spectral rotate')
    if (Y2 is None) != (M2 is None):
        raise ValueError('spectral rotate: Y2 and M2 are given together')
    M1 = _square(M1, B, Y1.device, 'spectral rotate')
    if Y2 is not None:
        _check_block(N, Y2, 'spectral rotate')
        M2 = _square(M2, B, Y1.device, 'spectral rotate')
    out = torch.empty_like(Y1) if out is None else out
    _check_block(N, out, 'spectral rotate')
    if Y2 is not None and Y2.shape != Y1.shape or out.shape != Y1.shape:
        raise ValueError('spectral rotate: the blocks must have one shape')
    nv.block_rotate(Y1, M1, Y2, M2, out)
    return out


def orthonormalise(Y, tmp, ws=None):
    """Y with orthonormal columns spanning the same space, by two passes of Gram matrix, `whitening` on the host and one rotation
    each.  `tmp` is a second block; the result is in Y's buffer."""
    rotate(Y, whitening(gram(Y, Y, ws).cpu().numpy()), out=tmp)
    return rotate(tmp, whitening(gram(tmp, tmp, ws).cpu().numpy()), out=Y)


def rayleigh_ritz(graph, scale, X, SX, X_out, SX_out, ws=None):
    """(theta descending [B], X V in X_out, S X V in SX_out) for orthonormal X: one apply (into SX), H = X^T S X, `ritz` on the
    host, two rotations."""
    apply(graph, scale, X, SX)
    theta, V = ritz(gram(X, SX, ws).cpu().numpy())
    rotate(X, V, out=X_out)
    rotate(SX, V, out=SX_out)
    return theta, X_out, SX_out


def residual_norms(X, SX, theta, R, ws=None):
    """||S x_i - theta_i x_i||_2 per column: R = S X - X Theta is formed on the device and its column norms are the diagonal of
    R^T R (not a difference of Gram matrices, which bottoms out at the square root of the unit roundoff)."""
    B = X.shape[1]
    rotate(SX, np.eye(B), X, -np.diag(theta), out=R)
    return np.sqrt(np.diag(gram(R, R, ws).cpu().numpy()))


def eigen(graph, scale, k, tol=1e-8, max_iter=100, max_degree=60, seed=0, degree=None):
    """The k largest eigenpairs of S by Chebyshev-filtered subspace iteration: dict(vectors float64 numpy [N, k]
    with orthonormal columns, eigenvalues [k] descending, residuals [k], converged, iterations, applies, degrees).  `degree`
    (device tensor or numpy, default scale^-2) gives the first column of the start block."""
    nv.require_gpu()
    k = int(k)
    B = block_width(k)
    N = graph.n
    if k < 1 or k > MAX_COMPONENTS + 1 or N < B:
        raise ValueError(f'spectral eigen: k = {k} of {N} cells; 1 <= k <= {MAX_COMPONENTS + 1} and at least {B} cells')
    dev = graph.col.device
    deg = (1.0 / (scale * scale)) if degree is None else torch.as_tensor(degree)
    blocks = [torch.empty(N, B, dtype=torch.float64, device=dev) for _ in range(5)]
    X = torch.from_numpy(start_block(deg.cpu().numpy() if torch.is_tensor(deg) else np.asarray(deg), B, seed)).to(dev)
    ws = torch.empty(nv.block_gram_workspace(N, B) // 8, dtype=torch.float64, device=dev)
    a, b, c, d, r = blocks
    X = orthonormalise(X, a, ws)
    theta, Xr, SXr = rayleigh_ritz(graph, scale, X, a, b, c, ws)
    free = [X, a, d]                                          # Xr = b, SXr = c, the residual in r
    applies, iterations, degrees = 1, 0, []
    resid = residual_norms(Xr, SXr, theta, r, ws)
    while not np.max(resid[:k]) <= tol and iterations < max_iter:
        p, e, cc, sigma1 = filter_plan(theta, max_degree)
        cur, old = free[0], Xr                               # Y_1 from X; from then on the new block takes the place of Y_(j-2)
        src = Xr
        for j, (al, ga, be) in enumerate(filter_coefficients(p, e, cc, sigma1)):
            if j == 0:
                cheb_step(graph, scale, src, None, cur, al, ga, be)
            else:
                cheb_step(graph, scale, cur, old, old, al, ga, be)
                cur, old = old, cur
        applies += p
        degrees.append(p)
        iterations += 1
        spare = [t for t in (free[0], Xr, SXr, free[1], free[2]) if t is not cur]
        X = orthonormalise(cur, spare[0], ws)
        theta, Xr, SXr = rayleigh_ritz(graph, scale, X, spare[0], spare[1], spare[2], ws)
        free = [X, spare[0], spare[3]]
        resid = residual_norms(Xr, SXr, theta, r, ws)
    return dict(vectors=Xr[:, :k].cpu().numpy(), eigenvalues=theta[:k].copy(), residuals=resid[:k].copy(),
                converged=bool(np.max(resid[:k]) <= tol), iterations=iterations, applies=applies, degrees=degrees)


def build_graph(x, n_neighbors, device='cuda'):
    """The fuzzy graph of the pooled cells x exactly as `umap.umap_checked` builds it."""
    idx, dist = self_knn(x, n_neighbors - 1, device)
    W, _, _, _ = jum.smooth_knn(idx, dist, n_neighbors)
    del dist
    return jum.fuzzy_graph(idx, W)


def spectral(embeddings, n_components=2, n_neighbors=15, kind='laplacian', density_normalize=None, tol=1e-8, max_iter=100,
             max_degree=60, seed=0, return_graph=False, device='cuda'):
    """Spectral embedding of M embeddings [N_m, L] pooled into one set of cells:

        vectors                     one float64 [N_m, k] array per embedding, k = n_components + 1: the eigenvectors of the k
                                    largest eigenvalues of S, unit norm, the largest entry positive; column 0 is the trivial one
        embedding                   the same without column 0 (umap-learn's `spectral_layout`, scanpy's `X_diffmap`)
        eigenvalues, residuals      float64 [k], descending; ||S q - theta q||_2
        degree                      float64 per embedding (d, or d' when density-normalised)
        umap_init                   float32 [N, 2]: q_2, q_3 on [0, 10], usable as JAMIE.umap(init=...)
        converged, iterations, applies, degrees      of the solver (`degrees`: the filter degree of every outer iteration)
        n_neighbors, n_edges, graph                  as JAMIE.umap

    Bit-identical from run to run."""
    checked = check_spectral(embeddings, n_components, n_neighbors, kind, density_normalize, tol, max_iter, max_degree, 'spectral')
    return spectral_checked(embeddings, *checked, seed, return_graph, device)


def spectral_checked(embeddings, n_components, n_neighbors, kind, density_normalize, tol, max_iter, max_degree, seed=0,
                     return_graph=False, device='cuda'):
    """`spectral` behind its argument checks: the arguments are what `check_spectral` returned."""
    n_cells = [_n_rows(e) for e in embeddings]
    _, x = _pool(embeddings, device, 'spectral')
    G = build_graph(x, n_neighbors, device)
    scale, degree = normalised_operator(G, density_normalize)
    out = eigen(G, scale, n_components + 1, tol, max_iter, max_degree, seed, degree)
    graph = G.to_scipy() if return_graph else None
    return spectral_summary(out['vectors'], out['eigenvalues'], out['residuals'], degree.cpu().numpy(), n_cells, out['converged'],
                            out['iterations'], out['applies'], out['degrees'], n_neighbors, G.col.numel(), kind, density_normalize,
                            tol, graph)

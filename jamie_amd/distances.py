"""Stage A of the correspondence path on the MI355X: the cell x cell distance matrices of `compute_distances` (reference
jamie.py:839-890) for the euclidean modes, the geodesic mode (`utilities.geodesic_distances`), the correlation family and the L1
family, as float32 device tensors.

    euclidean(X, squared=False)   sklearn pairwise_distances(metric='euclidean' | 'sqeuclidean')
    knn(X, k)                     sklearn NearestNeighbors(k).kneighbors_graph(X, mode='distance'), as (idx, w) [N, k]
    geodesic(X, kmax)             utilities.geodesic_distances(X, kmax), step for step
    cosine(X), correlation(X)     sklearn pairwise_distances(metric='cosine' | 'correlation')
    pearson(X)                    (1 - np.corrcoef(X)) / 2 (utilities.distance_matrix 'pearson')
    manhattan(X), chebyshev(X)    sklearn pairwise_distances(metric='manhattan' (= 'l1', 'cityblock') | 'chebyshev')

The kernels are in csrc/distances.hip (include/jamie_hip.h, "Stage A distances on the device").  The columns are centred first
(distances do not change under a shift; centring cuts the cancellation of the Gram form), G = Xc Xc^T is the exact-fp32 GEMM
(configuration 17) written straight into the N x N result, which every later pass then works on in place: peak device memory
N^2 * 4 bytes plus O(N (d + K)).  The only host work is the geodesic growth loop's connectivity test: scipy's
`connected_components` on the N x k neighbour list, the same call the host path makes.

The correlation family is that Gram pass on unit rows (1 - u.v = |u - v|^2 / 2).  jamie_row_normalise takes X as it is -- these
distances change under a column shift of X -- and the unit rows are then column-centred like the euclidean input: on all-positive
data (counts) they are nearly parallel, and the uncentred Gram form would lose 1e-5 at d = 2000.  The L1 family has no Gram form: jamie_pairwise_absdiff takes all pairs by direct
difference.
"""
import math

import numpy as np
import torch

from . import _native as nv

GRAM_CFG = 17          # gemm_f32.hip: 128 x 128 tiles on the fp32 matrix pipe (exact fp32; not the bf16x3 pieces)
K_MIN = 5              # growth loop of geodesic_distances: k from 5, +2 per step
TOPK_MAX = 1024        # largest K of jamie_knn_topk (csrc/distances.hip)


def _device_input(X, device='cuda'):
    """numpy (dense or with .toarray()) or a tensor -> contiguous fp32 / fp64 device tensor [N, d]; any other dtype (integers)
    goes to fp64, so that it centres exactly as the same values given as fp64 do.  NaN / inf raise ValueError, as sklearn does
    on the host path."""
    nv.require_gpu()
    if torch.is_tensor(X):
        t = X.to(device)
    else:
        X = X.toarray() if hasattr(X, 'toarray') else np.asarray(X)
        t = torch.from_numpy(np.ascontiguousarray(X)).to(device)
    if t.dtype not in (torch.float32, torch.float64):
        t = t.to(torch.float64)
    if t.dim() != 2:
        raise ValueError(f'distances: X must be 2-D [cells, features], got shape {tuple(t.shape)}')
    if not bool(torch.isfinite(t).all()):
        raise ValueError('distances: X contains NaN or infinity')
    return t.contiguous()


def centred(X, device='cuda'):
    """(X - column mean) as fp32 [N, d] on the device: jamie_col_stats, then jamie_standardise with sd = 1 (in fp64, one rounding)."""
    t = _device_input(X, device)
    N, d = t.shape
    R = int(max(1, min(256, (N + 2047) // 2048)))
    part = torch.empty(R * d, dtype=torch.float64, device=t.device)
    mean = torch.empty(d, dtype=torch.float64, device=t.device)
    sd = torch.empty(d, dtype=torch.float64, device=t.device)
    out = torch.empty(N, d, dtype=torch.float32, device=t.device)
    f64 = int(t.dtype == torch.float64)
    nv._call('jamie_col_stats', nv.ptr(t), f64, N, d, d, nv.ptr(part), R, nv.ptr(mean), nv.ptr(sd), nv._stream())
    sd.fill_(1.0)
    nv._call('jamie_standardise', nv.ptr(t), f64, N, d, d, nv.ptr(mean), nv.ptr(sd), nv.ptr(out), nv._stream())
    return out


def _euclidean_centred(Xc, squared=False, out=None):
    N, d = Xc.shape
    D = torch.empty(N, N, dtype=torch.float32, device=Xc.device) if out is None else out
    nv.gemm([nv.gemm_problem(Xc, Xc, D, N, N, d, d, d, N)], nv.NT, GRAM_CFG)           # G = Xc Xc^T
    sqn = torch.empty(N, dtype=torch.float32, device=Xc.device)
    nv.row_sqnorm(Xc, sqn)
    nv.gram_to_distances(D, sqn, Xc, squared)
    return D


def euclidean(X, squared=False, device='cuda'):
    """[N, N] float32 device tensor of euclidean (or squared euclidean) distances; diagonal exactly 0, exactly symmetric."""
    return _euclidean_centred(centred(X, device), squared)


def _unit_row_distances(X, centre, scale, name, device):
    """scale * |u_i - u_j|^2 on the unit rows of X (row-centred first if `centre`)."""
    t = _device_input(X, device)
    N, d = t.shape
    if N == 1:
        return torch.zeros(1, 1, dtype=torch.float32, device=t.device)
    U = torch.empty(N, d, dtype=torch.float32, device=t.device)
    norm = torch.empty(N, dtype=torch.float32, device=t.device)
    nv.row_normalise(t, centre, U, norm)
    if centre:
        flat = torch.nonzero(norm == 0)
        if flat.numel():
            raise ValueError(f'{name}: row {int(flat[0])} is constant, its correlation with any row is undefined (the host path '
                             f'returns NaN)')
    del t
    Uc = centred(U, device)                    # columns: the Gram form then cancels as little as the euclidean one
    del U
    D = torch.empty(N, N, dtype=torch.float32, device=Uc.device)
    nv.gemm([nv.gemm_problem(Uc, Uc, D, N, N, d, d, d, N)], nv.NT, GRAM_CFG)           # G = Uc Uc^T
    sqn = torch.empty(N, dtype=torch.float32, device=Uc.device)
    nv.row_sqnorm(Uc, sqn)
    nv.gram_to_scaled_sqdist(D, sqn, Uc, scale, norm)
    return D


def cosine(X, device='cuda'):
    """[N, N] float32 device tensor of cosine distances 1 - x_i.x_j / (|x_i| |x_j|); diagonal exactly 0, exactly symmetric.  A zero
    row is at distance 1 from every other row, as in sklearn."""
    return _unit_row_distances(X, False, 0.5, 'cosine', device)


def correlation(X, device='cuda'):
    """[N, N] float32 device tensor of correlation distances 1 - r_ij (r: Pearson correlation of rows i and j).  A constant row
    raises ValueError."""
    return _unit_row_distances(X, True, 0.5, 'correlation', device)


def pearson(X, device='cuda'):
    """[N, N] float32 device tensor of (1 - r_ij) / 2, JAMIE's 'pearson' mode.  A constant row raises ValueError."""
    return _unit_row_distances(X, True, 0.25, 'pearson', device)


def _absdiff_rows(X, device):
    """The fp32 rows the L1 family takes differences of.  Values that are fp32 numbers already go in as they are: their
    differences then round once (integers: not at all).  Anything else is column-centred in fp64 first (the L1 family does not
    change under a column shift), which keeps the conversion to fp32 from eating the differences."""
    t = _device_input(X, device)
    if t.dtype == torch.float32:
        return t
    t32 = t.to(torch.float32)
    if bool((t32.to(torch.float64) == t).all()):
        return t32
    del t32
    return centred(t, device)


def _absdiff(X, op, device):
    Xr = _absdiff_rows(X, device)
    N = Xr.shape[0]
    D = torch.empty(N, N, dtype=torch.float32, device=Xr.device)
    nv.pairwise_absdiff(Xr, op, D)
    return D


def manhattan(X, device='cuda'):
    """[N, N] float32 device tensor of L1 distances sum_c |x_ic - x_jc| ('manhattan' = 'l1' = 'cityblock'); diagonal exactly 0,
    exactly symmetric."""
    return _absdiff(X, 0, device)


def chebyshev(X, device='cuda'):
    """[N, N] float32 device tensor of Chebyshev distances max_c |x_ic - x_jc|; diagonal exactly 0, exactly symmetric."""
    return _absdiff(X, 1, device)


def k_max(N, kmax):
    """Largest k the growth loop of geodesic_distances can reach, clipped to N: its last step is taken at some
    k <= max(kmax, N / 100), and it starts at K_MIN whatever kmax is."""
    return int(min(max(int(kmax) + 2, math.ceil(0.01 * N) + 2, K_MIN), N))


def _knn_centred(Xc, K, D):
    """Top-K of the distance rows in D, then exact weights: (idx int32 [N, K], w float32 [N, K])."""
    N = Xc.shape[0]
    idx = torch.empty(N, K, dtype=torch.int32, device=Xc.device)
    w = torch.empty(N, K, dtype=torch.float32, device=Xc.device)
    nv.knn_topk(D, K, idx)
    nv.knn_weights(Xc, idx, w)
    return idx, w


def knn(X, k, device='cuda'):
    """k nearest neighbours of every cell (itself first, weight 0), ascending: (idx int32 [N, k'], w float32 [N, k']) device
    tensors, k' = min(k, N); w by direct difference in fp32."""
    Xc = centred(X, device)
    N = Xc.shape[0]
    kk = int(min(k, N))
    if kk < 1:
        raise ValueError('knn: k must be >= 1')
    if kk > TOPK_MAX:
        raise ValueError(f'knn: k = {kk} neighbours; the device top-K takes at most {TOPK_MAX}')
    D = _euclidean_centred(Xc)
    return _knn_centred(Xc, kk, D)


def _connected(idx_host, k):
    import scipy.sparse as sp
    import scipy.sparse.csgraph as csgraph
    N = idx_host.shape[0]
    cols = idx_host[:, :k].reshape(-1)
    rows = np.repeat(np.arange(N), k)
    g = sp.csr_matrix((np.ones(N * k, np.float32), (rows, cols)), shape=(N, N))
    return csgraph.connected_components(g, directed=False)[0] == 1


def geodesic(X, kmax, return_graph=False, device='cuda'):
    """utilities.geodesic_distances on the device: [N, N] float32 tensor.  `return_graph`: also (k, idx [N, K], w [N, K]) -- the
    k the growth loop chose (clipped to N) and the top-K lists it took prefixes of, K = min(k_max(N, kmax), TOPK_MAX).
    A growth loop that needs more than TOPK_MAX neighbours raises ValueError, before the graph and Floyd-Warshall passes."""
    Xc = centred(X, device)
    N = Xc.shape[0]
    if N == 1:
        D = torch.zeros(1, 1, dtype=torch.float32, device=Xc.device)
        if return_graph:
            z = torch.zeros(1, 1, device=Xc.device)
            return D, 1, z.to(torch.int32), z
        return D
    K = min(k_max(N, kmax), TOPK_MAX)
    D = _euclidean_centred(Xc)
    idx, w = _knn_centred(Xc, K, D)
    idx_host = idx.cpu().numpy()
    # growth loop of geodesic_distances: the graph of k neighbours is the first min(k, N) columns of the top-K lists
    k = K_MIN
    while True:
        if min(k, N) > K:
            raise ValueError(f'geodesic: the kNN graph is still disconnected at k = {K} and kmax = {kmax} asks for more '
                             f'neighbours; the device top-K takes at most {TOPK_MAX} (use the host path)')
        if _connected(idx_host, min(k, N)) or k > np.max((kmax, 0.01 * N)):
            break
        k += 2
    k = min(k, N)
    nv.knn_graph_init(D, idx, w, k)
    nv.apsp_fw(D)
    partials = torch.empty(nv.dist_workspace(N), dtype=torch.float32, device=Xc.device)
    maxv = torch.empty(1, dtype=torch.float32, device=Xc.device)
    nv.apsp_finalise(D, partials, maxv)
    if return_graph:
        return D, k, idx, w
    return D

"""k-means of the pooled cells on the MI355X, and how well the clusters recover the labels: ARI and NMI.

    kmeans(X, n_clusters)                          Lloyd's k-means, k-means++ seeding, the best of n_init runs
    kmeans_plusplus(X, n_clusters, u)              the seeding alone: (centres, the cells picked)
    assign(X, centers)                             (labels, minq): the nearest centre of every row by (q, then lower index)
    step(X, centers)                               one Lloyd iteration with everything it forms (sums, counts, scalars)
    contingency(a, b, na, nb)                      the exact integer table of two code arrays
    ari_nmi(table)                                 sklearn's adjusted_rand_score and normalized_mutual_info_score ('arithmetic')
                                                   from a contingency table, float64 on the host
    clustering(embeddings, labels)                 JAMIE.test_clustering on the device

The kernels are in csrc/clustering.hip (include/jamie_hip.h, "Clustering on the device"): assignment and the fp64 cluster sums in
one pass over X, the stop rules on the device so that iterations are enqueued in batches, the running minimum and the weighted
pick of the seeding, the table by integer atomics.  Device memory is the input plus the workspace of
`_native.kmeans_workspace` plus O(N + k L).  The definition (shared with the float64 host route of jamie.py) is DESIGN.md §18.
"""
import numpy as np
import torch

from . import _native as nv
from .metrics import _device_input
from .neighbors import _n_rows, _pool, pooled_codes

KMEANS_KMAX = 1024     # largest k of jamie_kmeans_step
SEGMENT_TILE = 128     # seg_rows is a multiple of it
PICK_BLOCK = 1024      # elements per block total of jamie_weighted_pick
BATCH = 8              # iterations enqueued between two reads of the device's `done` word
VARIANCE_CHUNK = 16384


# ---- the argument checks and the definitions both routes share ----
def check_finite(arrays, what):
    for a in arrays:
        ok = bool(torch.isfinite(a).all()) if torch.is_tensor(a) else bool(np.isfinite(np.asarray(a, dtype=np.float64)).all())
        if not ok:
            raise ValueError(f'{what}: input contains NaN or infinity')


def check_kmeans(n_cells, n_features, n_clusters, n_init, max_iter, tol, init, what):
    """(k, n_init, max_iter, tol, init as float64 [k, L] or None) under the rules 1 <= k <= min(cells, 1024), init [k, L] and
    finite (it forces one run), n_init >= 1, max_iter >= 1, tol >= 0.  Shared by the device and the host route."""
    k = int(n_clusters)
    if k < 1 or k > KMEANS_KMAX:
        raise ValueError(f'{what}: n_clusters = {k}; 1 <= n_clusters <= {KMEANS_KMAX}')
    if k > n_cells:
        raise ValueError(f'{what}: n_clusters = {k} asked of {n_cells} cells')
    if init is not None:
        init = np.array(init.detach().cpu().numpy() if torch.is_tensor(init) else init, dtype=np.float64)
        if init.shape != (k, n_features):
            raise ValueError(f'{what}: init must be [{k}, {n_features}], got {init.shape}')
        if not np.isfinite(init).all():
            raise ValueError(f'{what}: init contains NaN or infinity')
    n_init, max_iter, tol = int(n_init), int(max_iter), float(tol)
    if n_init < 1:
        raise ValueError(f'{what}: n_init = {n_init}; at least 1')
    if max_iter < 1:
        raise ValueError(f'{what}: max_iter = {max_iter}; at least 1')
    if not tol >= 0.0:
        raise ValueError(f'{what}: tol = {tol}; at least 0')
    return k, (1 if init is not None else n_init), max_iter, tol, init


def check_clustering(embeddings, labels, n_clusters, n_init, max_iter, tol, init, what):
    """The checks of JAMIE.test_clustering in their order: one label per cell, finite input, k range, init shape, n_init,
    max_iter, tol.  Returns (k, n_init, max_iter, tol, init).  Nothing is allocated on a device."""
    if len(embeddings) < 1:
        raise ValueError(f'{what}: no embeddings')
    for e in embeddings:
        if len(e.shape) != 2 or e.shape[1] != embeddings[0].shape[1] or e.shape[1] < 1:
            raise ValueError(f'{what}: the embeddings must be [cells, features] with the same features')
    n_cells = [int(e.shape[0]) for e in embeddings]
    _, _, classes = pooled_codes(n_cells, labels, what)
    check_finite(embeddings, what)
    if n_clusters is None:
        if classes is None:
            raise ValueError(f'{what}: n_clusters defaults to the number of distinct labels; give labels or n_clusters')
        n_clusters = len(classes)
    return check_kmeans(int(sum(n_cells)), int(embeddings[0].shape[1]), n_clusters, n_init, max_iter, tol, init, what)


def seeding_stream(seed, run, k):
    """The k uniform numbers of run `run`: drawn on the host for both routes."""
    return np.random.default_rng([int(seed), int(run)]).random(int(k))


def ari_nmi(table):
    """(ARI, NMI) of a contingency table [clusters, labels] of non-negative integers: sklearn's `adjusted_rand_score` and
    `normalized_mutual_info_score(average_method='arithmetic')` restated on the table (empty rows and columns are clusters and
    labels that do not occur: dropped), float64 / exact integers on the host."""
    t = np.asarray(table)
    if t.ndim != 2 or t.size == 0 or np.any(t < 0):
        raise ValueError(f'ari_nmi: a non-negative [clusters, labels] table, got shape {t.shape}')
    t = t.astype(np.int64)
    t = t[t.sum(axis=1) > 0][:, t.sum(axis=0) > 0]
    n = int(t.sum())
    if n == 0:
        raise ValueError('ari_nmi: an empty table')
    rows, cols = t.sum(axis=1), t.sum(axis=0)              # cluster sizes, label sizes
    sum_squares = sum(int(v) ** 2 for v in t.ravel())
    same_cluster = sum(int(v) * int(r) for v, r in zip(t.ravel(), np.repeat(rows, t.shape[1]))) - sum_squares
    same_label = sum(int(v) * int(c) for v, c in zip(t.ravel(), np.tile(cols, t.shape[0]))) - sum_squares
    tp = sum_squares - n
    fp, fn = same_cluster, same_label
    tn = n * n - fp - fn - sum_squares
    ari = 1.0 if fn == 0 and fp == 0 else 2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))
    if t.shape[0] == 1 and t.shape[1] == 1:
        return float(ari), 1.0
    if t.shape[0] == 1 or t.shape[1] == 1:
        return float(ari), 0.0
    zx, zy = np.nonzero(t)
    nz = t[zx, zy].astype(np.float64)
    pi, pj = rows.astype(np.float64), cols.astype(np.float64)
    total = float(n)
    outer = rows.take(zx).astype(np.int64) * cols.take(zy).astype(np.int64)
    log_outer = -np.log(outer) + np.log(pi.sum()) + np.log(pj.sum())
    mi = nz / total * (np.log(nz) - np.log(total)) + nz / total * log_outer
    mi = np.where(np.abs(mi) < np.finfo(np.float64).eps, 0.0, mi)
    mi = float(np.clip(mi.sum(), 0.0, None))
    if mi == 0:
        return float(ari), 0.0

    def entropy(p):
        s = p.sum()
        return float(-np.sum((p / s) * (np.log(p) - np.log(s))))
    return float(ari), float(mi / (0.5 * (entropy(cols.astype(np.float64)) + entropy(rows.astype(np.float64)))))


def clustering_summary(km, n_cells, table_mod, table_lab, classes):
    """The dict of JAMIE.test_clustering from a k-means result and the two tables (shared by the device and the host route)."""
    lab = np.asarray(km['labels'], dtype=np.int32)
    cuts = np.cumsum(n_cells)[:-1]
    ari, nmi = ari_nmi(table_lab) if table_lab is not None else (None, None)
    return {'clusters': np.split(lab, cuts), 'centers': np.asarray(km['centers'], dtype=np.float64), 'inertia': float(km['inertia']),
            'n_iter': int(km['n_iter']), 'converged': bool(km['converged']), 'sizes': np.asarray(km['sizes'], dtype=np.int64),
            'n_empty': int(km['n_empty']), 'run': int(km['run']), 'modality_contingency': np.asarray(table_mod, dtype=np.int64),
            'ari': ari, 'nmi': nmi, 'contingency': None if table_lab is None else np.asarray(table_lab, dtype=np.int64),
            'labels': classes}


# ---- the device route ----
def _check_seg_rows(seg_rows, what):
    seg_rows = int(seg_rows)
    if seg_rows < 0 or seg_rows % SEGMENT_TILE:
        raise ValueError(f'{what}: seg_rows = {seg_rows}; 0 or a positive multiple of {SEGMENT_TILE}')
    return seg_rows


def _mean_variance(x):
    """The mean over the features of the population variance of x [N, L], fp64, two passes in row chunks."""
    N = x.shape[0]
    s = torch.zeros(x.shape[1], dtype=torch.float64, device=x.device)
    for r in range(0, N, VARIANCE_CHUNK):
        s += x[r:r + VARIANCE_CHUNK].double().sum(dim=0)
    mean = s / N
    v = torch.zeros_like(s)
    for r in range(0, N, VARIANCE_CHUNK):
        v += ((x[r:r + VARIANCE_CHUNK].double() - mean) ** 2).sum(dim=0)
    return float((v / N).mean())


class _Buffers:
    """What one Lloyd run needs on the device beside X and the centres."""

    def __init__(self, x, k, seg_rows):
        N, L = x.shape
        dev = x.device
        self.labels = torch.empty(N, dtype=torch.int32, device=dev)
        self.counts = torch.empty(k, dtype=torch.int64, device=dev)
        self.stats = torch.zeros(4, dtype=torch.float64, device=dev)
        self.state = torch.zeros(4, dtype=torch.int32, device=dev)
        self.ws = torch.empty(nv.kmeans_workspace(N, L, k, seg_rows), dtype=torch.uint8, device=dev)
        self.seg_rows = seg_rows


def _lloyd(x, C, buf, max_iter, tol_abs):
    """Iterate in place on the centres C (fp32 [k, L]) until the device raises `done`; (inertia, n_iter, converged, n_empty).
    buf.labels, buf.counts are those of the stopping iteration, C is C_{t + 1}."""
    buf.state.zero_()
    buf.labels.fill_(-1)
    issued = 0
    while True:
        n = max(1, min(BATCH, max_iter - issued))
        for _ in range(n):
            nv.kmeans_step(x, C, buf.labels, buf.counts, buf.stats, buf.state, buf.ws, tol_abs, max_iter, True, seg_rows=buf.seg_rows)
        issued += n
        state = buf.state.cpu().numpy()
        if state[0]:
            break
    stats = buf.stats.cpu().numpy()
    return float(stats[0]), int(state[1]), bool(state[2]), int(stats[3])


def _seed(x, u, C, minq, picks, pick_ws):
    N = x.shape[0]
    picks[0:1] = min(int(u[0] * N), N - 1)
    nv.kmeans_min_update(x, picks[0:1], minq, True, C[0])
    for j in range(1, len(u)):
        nv.weighted_pick(minq, u[j], picks[j:j + 1], pick_ws)
        nv.kmeans_min_update(x, picks[j:j + 1], minq, False, C[j])


def kmeans_plusplus(X, n_clusters, u, device='cuda'):
    """Plain k-means++ (D^2 sampling) from the k uniform numbers u: the first centre is cell floor(u[0] N); centre j >= 1 is the
    smallest cell whose prefix sum of minq (the running minimum of q to the centres so far) exceeds u[j] * total, floor(u[j] N)
    where total == 0.  Returns (centres fp32 device [k, L], the cells picked int64 numpy [k])."""
    k = int(n_clusters)
    u = np.asarray(u, dtype=np.float64)
    if k < 1 or k > KMEANS_KMAX or k > _n_rows(X) or u.shape != (k,) or np.any(u < 0) or np.any(u >= 1):
        raise ValueError(f'kmeans_plusplus: 1 <= n_clusters <= min(cells, {KMEANS_KMAX}) and u [n_clusters] in [0, 1)')
    x = _device_input(X, device, 'kmeans_plusplus')
    N, L = x.shape
    C = torch.empty(k, L, dtype=torch.float32, device=x.device)
    minq = torch.empty(N, dtype=torch.float32, device=x.device)
    picks = torch.empty(k, dtype=torch.int64, device=x.device)
    pick_ws = torch.empty(8 * ((N + PICK_BLOCK - 1) // PICK_BLOCK), dtype=torch.uint8, device=x.device)
    _seed(x, u, C, minq, picks, pick_ws)
    return C, picks.cpu().numpy()


def step(X, centers, labels=None, update=True, tol_abs=0.0, device='cuda', seg_rows=0):
    """One Lloyd iteration under `centers` [k, L]: dict(labels int32 [N], minq fp32 [N], sums fp64 [k, L], counts int64 [k],
    centers fp32 [k, L] (the new ones; the old ones where `update` is off), stats fp64 [inertia, shift, changed, empty]) of device
    tensors.  `labels`: the previous labels (default: none, every label counts as changed)."""
    seg_rows = _check_seg_rows(seg_rows, 'step')
    x = _device_input(X, device, 'step')
    C = _device_input(centers, device, 'step').clone()
    N, L = x.shape
    k = C.shape[0]
    if L < 1 or C.shape[1] != L or k < 1 or k > min(N, KMEANS_KMAX):
        raise ValueError(f'step: centers must be [1 <= k <= min(cells, {KMEANS_KMAX}), {L}], got {tuple(C.shape)}')
    buf = _Buffers(x, k, seg_rows)
    if labels is None:
        buf.labels.fill_(-1)
    else:
        buf.labels.copy_(torch.as_tensor(labels).to(x.device, torch.int32))
    minq = torch.empty(N, dtype=torch.float32, device=x.device)
    sums = torch.empty(k, L, dtype=torch.float64, device=x.device)
    nv.kmeans_step(x, C, buf.labels, buf.counts, buf.stats, buf.state, buf.ws, tol_abs, 1, update, minq=minq, sums=sums,
                   seg_rows=seg_rows)
    return {'labels': buf.labels, 'minq': minq, 'sums': sums, 'counts': buf.counts, 'centers': C, 'stats': buf.stats}


def assign(X, centers, device='cuda', seg_rows=0):
    """(labels int32 [N], minq fp32 [N]) device tensors: the nearest centre of every row by (q, then lower index), q by direct
    difference in fp32."""
    out = step(X, centers, update=False, device=device, seg_rows=seg_rows)
    return out['labels'], out['minq']


def _kmeans_device(x, k, n_init, max_iter, tol, seed, init, seg_rows):
    N, L = x.shape
    tol_abs = tol * _mean_variance(x)
    buf = _Buffers(x, k, seg_rows)
    C = torch.empty(k, L, dtype=torch.float32, device=x.device)
    best = None
    if init is None:
        minq = torch.empty(N, dtype=torch.float32, device=x.device)
        picks = torch.empty(k, dtype=torch.int64, device=x.device)
        pick_ws = torch.empty(8 * ((N + PICK_BLOCK - 1) // PICK_BLOCK), dtype=torch.uint8, device=x.device)
    for r in range(n_init):
        if init is None:
            _seed(x, seeding_stream(seed, r, k), C, minq, picks, pick_ws)
            seeds = picks.cpu().numpy()
        else:
            C.copy_(torch.from_numpy(init.astype(np.float32)))
            seeds = None
        inertia, n_iter, converged, n_empty = _lloyd(x, C, buf, max_iter, tol_abs)
        if best is None or inertia < best['inertia']:
            best = {'labels': buf.labels.clone(), 'centers': C.clone(), 'inertia': inertia, 'n_iter': n_iter, 'converged': converged,
                    'sizes': buf.counts.clone(), 'n_empty': n_empty, 'run': r, 'seeds': seeds}
    return best


def kmeans(X, n_clusters, n_init=4, max_iter=300, tol=1e-4, seed=0, init=None, device='cuda', seg_rows=0):
    """Lloyd's k-means of the rows of X [N, L]: dict(labels int32 [N], centers float64 [k, L], inertia, n_iter,
    converged, sizes int64 [k], n_empty, run, seeds) on the host.  Run r is seeded by k-means++ from
    `np.random.default_rng([seed, r]).random(k)`; the run of the lowest inertia is kept (ties: the lowest r); `init` [k, L]
    replaces the seeding and forces one run.  A run stops after the first iteration whose labels equal the previous ones, or whose
    centres moved by no more than tol x (the mean variance of the features) in total, or at max_iter.  Empty clusters keep
    their centre and are counted in n_empty.  `seg_rows`: rows per workgroup (0: the library's choice; else a multiple of 128)."""
    seg_rows = _check_seg_rows(seg_rows, 'kmeans')
    if not hasattr(X, 'shape') or len(X.shape) != 2 or X.shape[1] < 1:
        raise ValueError('kmeans: X must be [cells, features]')
    k, n_init, max_iter, tol, init = check_kmeans(int(X.shape[0]), int(X.shape[1]), n_clusters, n_init, max_iter, tol, init, 'kmeans')
    x = _device_input(X, device, 'kmeans')
    best = _kmeans_device(x, k, n_init, max_iter, tol, seed, init, seg_rows)
    return _to_host(best)


def _to_host(best):
    out = dict(best)
    out['labels'] = best['labels'].cpu().numpy()
    out['centers'] = best['centers'].cpu().numpy().astype(np.float64)
    out['sizes'] = best['sizes'].cpu().numpy()
    return out


def contingency(a, b, na, nb, device='cuda'):
    """table int64 numpy [na, nb]: table[x, y] = #{ i : a[i] == x and b[i] == y }, exact.  a, b: integer codes [N], numpy or
    device tensors.  A code outside its range raises ValueError."""
    nv.require_gpu()
    na, nb = int(na), int(nb)
    if na < 1 or nb < 1:
        raise ValueError(f'contingency: na = {na}, nb = {nb}; at least 1 each')
    a_d = torch.as_tensor(a).to(device, torch.int32).contiguous().reshape(-1)
    b_d = torch.as_tensor(b).to(a_d.device, torch.int32).contiguous().reshape(-1)
    if a_d.numel() != b_d.numel() or a_d.numel() < 1:
        raise ValueError(f'contingency: two code arrays of one length >= 1, got {a_d.numel()} and {b_d.numel()}')
    table = torch.zeros(na, nb, dtype=torch.int64, device=a_d.device)
    flag = torch.zeros(1, dtype=torch.int32, device=a_d.device)
    nv.contingency(a_d, b_d, na, nb, table, flag)
    if int(flag.item()):
        raise ValueError(f'contingency: a code outside [0, {na}) x [0, {nb})')
    return table.cpu().numpy()


def clustering(embeddings, labels=None, n_clusters=None, n_init=4, max_iter=300, tol=1e-4, seed=0, init=None, device='cuda',
               seg_rows=0):
    """JAMIE.test_clustering on the device: k-means of the pooled cells of M embeddings [N_m, L] (k defaults to the number of
    distinct labels), the cluster x modality table and, with labels, the cluster x label table with its ARI and NMI."""
    seg_rows = _check_seg_rows(seg_rows, 'clustering')
    k, n_init, max_iter, tol, init = check_clustering(embeddings, labels, n_clusters, n_init, max_iter, tol, init, 'clustering')
    n_cells = [_n_rows(e) for e in embeddings]
    mod, lcode, classes = pooled_codes(n_cells, labels, 'clustering')
    xs, x = _pool(embeddings, device, 'clustering')
    best = _kmeans_device(x, k, n_init, max_iter, tol, seed, init, seg_rows)
    table_mod = contingency(best['labels'], mod, k, len(xs), device=x.device)
    table_lab = None if lcode is None else contingency(best['labels'], lcode, k, len(classes), device=x.device)
    return clustering_summary(_to_host(best), n_cells, table_mod, table_lab, classes)

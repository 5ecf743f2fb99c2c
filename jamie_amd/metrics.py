"""Alignment metrics on the MI355X: the reference's acceptance numbers on whole data sets, without an N x N matrix.

    foscttm(A, B)                                  JAMIE.test_closer (reference jamie.py:892-915): fraction of samples closer
                                                   than the true match, cell i of A paired with cell i of B
    cross_knn(Q, R, k)                             sklearn NearestNeighbors(k).fit(R).kneighbors(Q), as (idx, dist) [Nq, k]
    label_transfer_accuracy(q, ql, r, rl, k=5)     JAMIE.test_LabelTA (reference jamie.py:943-961): KNeighborsClassifier(k)
                                                   fitted on (r, rl), its accuracy on (q, ql)
    label_distance_sums(Q, R, rl)                  per query the sum of its distances to the rows of R of every label
    silhouette_samples(X, labels)                  sklearn silhouette_samples(X, labels), euclidean
    silhouette(embeddings, labels)                 JAMIE.test_silhouette: silhouette widths of the pooled cells by label and by
                                                   modality within a label, and the label x label mean distances, from one pass

The kernels are in csrc/metrics.hip (include/jamie_hip.h, "Alignment metrics on the device"): all pairs between two [N, L]
embeddings in fp32 by direct difference, reduced on the fly to per-cell counts or per-query neighbour lists.  Device memory is
the two inputs plus O(N k); the pair space is walked in TILE_I x TILE_J tiles, each computed once and feeding the row counts and
the column counts of FOSCTTM together.  Labels are encoded on the host (`np.unique`), the vote runs on the device.
"""
import numpy as np
import torch

from . import _native as nv

TILE_I = 128           # pair tile of the FOSCTTM kernel (csrc/metrics.hip): rows of A ...
TILE_J = 128           # ... against rows of B
KNN_MAX = 64           # largest k of jamie_cross_knn


def _device_input(X, device='cuda', what='metrics'):
    """numpy (dense or with .toarray()) or a tensor -> contiguous fp32 device tensor [N, L]; fp64 / integer input is converted
    once.  NaN / inf raise ValueError."""
    nv.require_gpu()
    if torch.is_tensor(X):
        t = X.to(device)
    else:
        X = X.toarray() if hasattr(X, 'toarray') else np.asarray(X)
        t = torch.from_numpy(np.ascontiguousarray(X)).to(device)
    if t.dim() != 2:
        raise ValueError(f'{what}: inputs must be 2-D [cells, features], got shape {tuple(t.shape)}')
    if t.dtype != torch.float32:
        t = t.to(torch.float32)
    if not bool(torch.isfinite(t).all()):
        raise ValueError(f'{what}: input contains NaN or infinity')
    return t.contiguous()


def foscttm(A, B, return_counts=False, device='cuda'):
    """FOSCTTM of two embeddings of the same cells: (sum row_closer + sum col_closer) / (2 N^2), the divisor of the reference.
    `return_counts`: also (row_closer, col_closer) as int64 numpy [N]: row_closer[i] = #{ j != i : |A_i - B_j| < |A_i - B_i| },
    col_closer[j] = #{ i != j : |A_i - B_j| < |A_j - B_j| }."""
    a, b = _device_input(A, device, 'foscttm'), _device_input(B, device, 'foscttm')
    if a.shape[0] != b.shape[0]:
        raise ValueError(f'foscttm: the data sets must hold the same cells, got {a.shape[0]} and {b.shape[0]}')
    if a.shape[1] != b.shape[1]:
        raise ValueError(f'foscttm: the embeddings must have the same features, got {a.shape[1]} and {b.shape[1]}')
    N = a.shape[0]
    if N < 1 or a.shape[1] < 1:
        raise ValueError('foscttm: empty input')
    counts = torch.empty(2, N, dtype=torch.int32, device=a.device)
    ws = torch.empty(nv.metrics_workspace(N, N, 0), dtype=torch.uint8, device=a.device)
    nv.foscttm_counts(a, b, counts[0], counts[1], ws)
    total = int(counts.sum(dtype=torch.int64))
    value = total / (2 * N ** 2)
    if return_counts:
        c = counts.cpu().numpy().astype(np.int64)
        return value, (c[0], c[1])
    return value


def _check_k(k, n_ref, what):
    k = int(k)
    if k < 1 or k > KNN_MAX:
        raise ValueError(f'{what}: k = {k}; the device search takes 1 <= k <= {KNN_MAX}')
    if k > n_ref:
        raise ValueError(f'{what}: k = {k} neighbours asked of {n_ref} reference rows')
    return k


def cross_knn(Q, R, k, device='cuda'):
    """The k rows of R nearest to every row of Q, ascending by (distance, then lower index): (idx int32 [Nq, k], dist float32
    [Nq, k]) device tensors, euclidean distances by direct difference in fp32."""
    k = _check_k(k, R.shape[0] if hasattr(R, 'shape') and len(R.shape) == 2 else len(R), 'cross_knn')
    q, r = _device_input(Q, device, 'cross_knn'), _device_input(R, device, 'cross_knn')
    if q.shape[1] != r.shape[1]:
        raise ValueError(f'cross_knn: queries and references must have the same features, got {q.shape[1]} and {r.shape[1]}')
    if q.shape[0] < 1 or q.shape[1] < 1:
        raise ValueError('cross_knn: empty input')
    idx = torch.empty(q.shape[0], k, dtype=torch.int32, device=q.device)
    dist = torch.empty(q.shape[0], k, dtype=torch.float32, device=q.device)
    ws = torch.empty(nv.metrics_workspace(q.shape[0], r.shape[0], k), dtype=torch.uint8, device=q.device)
    nv.cross_knn(q, r, k, idx, dist, ws)
    return idx, dist


def vote(idx, ref_codes, n_classes):
    """Majority vote of the neighbours' class codes (ties to the lowest code): int32 device tensor [Nq]."""
    codes = torch.as_tensor(np.ascontiguousarray(ref_codes, dtype=np.int32)).to(idx.device)
    pred = torch.empty(idx.shape[0], dtype=torch.int32, device=idx.device)
    nv.knn_vote(idx, codes, n_classes, pred)
    return pred


def label_transfer_accuracy(query, query_labels, ref, ref_labels, k=5, return_pred=False, device='cuda'):
    """Accuracy of a k-nearest-neighbour classifier fitted on (ref, ref_labels) at predicting query_labels from query: sklearn
    `KNeighborsClassifier(n_neighbors=k).fit(ref, ref_labels).score(query, query_labels)`.  `return_pred`: also the predicted
    labels (numpy, dtype of ref_labels)."""
    ref_labels, query_labels = np.asarray(ref_labels), np.asarray(query_labels)
    n_ref = ref.shape[0]
    if ref_labels.ndim != 1 or ref_labels.shape[0] != n_ref:
        raise ValueError('label_transfer_accuracy: one label per reference row')
    if query_labels.ndim != 1 or query_labels.shape[0] != query.shape[0]:
        raise ValueError('label_transfer_accuracy: one label per query row')
    k = _check_k(k, n_ref, 'label_transfer_accuracy')
    classes, codes = np.unique(ref_labels, return_inverse=True)
    idx, _ = cross_knn(query, ref, k, device)
    pred = classes[vote(idx, codes.reshape(-1), len(classes)).cpu().numpy()]
    acc = float(np.mean(pred == query_labels))
    if return_pred:
        return acc, pred
    return acc


# ---- silhouette widths (sklearn `silhouette_samples`) from per-cell distance sums by class; DESIGN.md §16 ----
QUERY_TILE = 128       # query rows of a workgroup of jamie_label_distance_sums: the row chunks are multiples of it


def _sorted_by_class(r, codes, n_classes):
    """R gathered into class order on the device (stable argsort of the codes): (R sorted, class_off int64 device [C + 1],
    counts int64 numpy [C])."""
    codes = np.ascontiguousarray(codes, dtype=np.int64).reshape(-1)
    if codes.shape[0] != r.shape[0]:
        raise ValueError(f'one class code per reference row: {codes.shape[0]} codes for {r.shape[0]} rows')
    if codes.size and (codes.min() < 0 or codes.max() >= n_classes):
        raise ValueError(f'class codes must lie in [0, {n_classes})')
    counts = np.bincount(codes, minlength=n_classes).astype(np.int64)
    order = torch.argsort(torch.from_numpy(codes).to(r.device), stable=True)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return r.index_select(0, order).contiguous(), torch.from_numpy(off).to(r.device), counts


def _row_chunk(Nq, Nr, n_classes, seg_tiles, max_workspace, what):
    """The most query rows (a multiple of QUERY_TILE, or all Nq) whose S [rows, C] fp64 and segment partials stay under
    `max_workspace` bytes."""
    def need(rows):
        return rows * n_classes * 8 + nv.label_sums_workspace(rows, Nr, n_classes, seg_tiles)
    first = min(Nq, QUERY_TILE)
    if need(first) > max_workspace:
        raise ValueError(f'{what}: one chunk of {first} query rows needs {need(first)} bytes of workspace, max_workspace is '
                         f'{max_workspace}')
    if need(Nq) <= max_workspace:
        return Nq
    lo, hi = 1, (Nq + QUERY_TILE - 1) // QUERY_TILE          # tiles: need(lo) fits, need(hi) does not
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if need(mid * QUERY_TILE) <= max_workspace:
            lo = mid
        else:
            hi = mid
    return lo * QUERY_TILE


def _sums_chunks(q, r_sorted, class_off, n_classes, seg_tiles, max_workspace, what):
    """Yields (row0, row1, S [row1 - row0, C] fp64) over row chunks of the queries; S is reused by the next chunk."""
    Nq, Nr = q.shape[0], r_sorted.shape[0]
    rows = _row_chunk(Nq, Nr, n_classes, seg_tiles, max_workspace, what)
    S = torch.empty(rows, n_classes, dtype=torch.float64, device=q.device)
    ws = torch.empty(nv.label_sums_workspace(rows, Nr, n_classes, seg_tiles), dtype=torch.uint8, device=q.device)
    for r0 in range(0, Nq, rows):
        r1 = min(r0 + rows, Nq)
        nv.label_distance_sums(q[r0:r1], r_sorted, class_off, S[:r1 - r0], ws, seg_tiles)
        yield r0, r1, S[:r1 - r0]


def class_distance_sums(Q, R, codes, n_classes, device='cuda', seg_tiles=0):
    """S fp64 device tensor [Nq, n_classes]: S[i, c] = sum of the euclidean distances from Q[i] to the rows of R with class code c
    (integer codes in [0, n_classes); a code no row carries gives a column of exact zeros)."""
    q, r = _device_input(Q, device, 'class_distance_sums'), _device_input(R, device, 'class_distance_sums')
    if q.shape[1] != r.shape[1]:
        raise ValueError(f'class_distance_sums: queries and references must have the same features, got {q.shape[1]} and '
                         f'{r.shape[1]}')
    n_classes, seg_tiles = int(n_classes), int(seg_tiles)
    if q.shape[0] < 1 or r.shape[0] < 1 or q.shape[1] < 1 or n_classes < 1:
        raise ValueError('class_distance_sums: empty input')
    if seg_tiles < 0:
        raise ValueError('class_distance_sums: seg_tiles must be 0 (chosen by the library) or a number of 128-row tiles')
    rs, off, _ = _sorted_by_class(r, codes, n_classes)
    S = torch.empty(q.shape[0], n_classes, dtype=torch.float64, device=q.device)
    ws = torch.empty(nv.label_sums_workspace(q.shape[0], r.shape[0], n_classes, seg_tiles), dtype=torch.uint8, device=q.device)
    nv.label_distance_sums(q, rs, off, S, ws, seg_tiles)
    return S


def label_distance_sums(Q, R, ref_labels, device='cuda', seg_tiles=0):
    """(S, classes, counts): S fp64 device tensor [Nq, C], S[i, c] = sum of the euclidean distances from Q[i] to the rows of R
    labelled classes[c]; classes = np.unique(ref_labels), counts int64 numpy [C]."""
    ref_labels = np.asarray(ref_labels)
    if ref_labels.ndim != 1 or ref_labels.shape[0] != R.shape[0]:
        raise ValueError('label_distance_sums: one label per reference row')
    classes, codes = np.unique(ref_labels, return_inverse=True)
    S = class_distance_sums(Q, R, codes.reshape(-1), len(classes), device, seg_tiles)
    return S, classes, np.bincount(codes.reshape(-1), minlength=len(classes)).astype(np.int64)


def _check_label_count(n_labels, n_samples):
    if not 1 < n_labels < n_samples:                       # sklearn's check_number_of_labels
        raise ValueError(f'Number of labels is {n_labels}. Valid values are 2 to n_samples - 1 (inclusive)')


def silhouette_samples(X, labels, device='cuda', max_workspace=1 << 30, seg_tiles=0):
    """sklearn `silhouette_samples(X, labels)` (euclidean): float64 numpy [N], without an N x N matrix.  The cells go through
    the device in row chunks whose workspace stays under `max_workspace` bytes; the result does not depend on the chunking."""
    x = _device_input(X, device, 'silhouette_samples')
    labels = np.asarray(labels)
    N = x.shape[0]
    if labels.ndim != 1 or labels.shape[0] != N:
        raise ValueError(f'silhouette_samples: one label per cell, got {labels.shape} for {N} cells')
    if x.shape[1] < 1:
        raise ValueError('silhouette_samples: empty input')
    classes, codes = np.unique(labels, return_inverse=True)
    codes = codes.reshape(-1)
    C = len(classes)
    _check_label_count(C, N)
    xs, off, counts = _sorted_by_class(x, codes, C)
    counts_d = torch.from_numpy(counts).to(x.device)
    own = torch.from_numpy(codes.astype(np.int32)).to(x.device)
    out = torch.empty(N, dtype=torch.float64, device=x.device)
    for r0, r1, S in _sums_chunks(x, xs, off, C, int(seg_tiles), int(max_workspace), 'silhouette_samples'):
        nv.silhouette_widths(S, counts_d, own[r0:r1], None, C, out[r0:r1])
    return out.cpu().numpy()


def silhouette(embeddings, labels, device='cuda', max_workspace=1 << 30, seg_tiles=0):
    """Silhouette figures of M embeddings [N_m, L] of labelled cells, from ONE pass over the pooled cells with the class code
    label * M + modality:

        label_widths [sum N_m], label_asw        silhouette of the pooled cells with the labels as clusters, and its mean
        modality_asw_per_label [T], modality_asw mean of 1 - |s| over a label's cells, s their silhouette with the modality as
                                                 cluster among that label's cells (1: the modalities mix; NaN for a label present
                                                 in fewer than two modalities), and the mean over the labels that have a figure
        label_distance [T, T]                    mean distance between the cells of two labels (the diagonal with the self-pairs)
        labels [T]                               np.unique of the labels
    """
    M = len(embeddings)
    if M < 1 or len(labels) != M:
        raise ValueError(f'silhouette: one label array per embedding, got {len(labels)} for {M} embeddings')
    xs = [_device_input(e, device, 'silhouette') for e in embeddings]
    labs = [np.asarray(lab) for lab in labels]
    for m in range(M):
        if labs[m].ndim != 1 or labs[m].shape[0] != xs[m].shape[0]:
            raise ValueError(f'silhouette: one label per cell, got {labs[m].shape} for the {xs[m].shape[0]} cells of embedding {m}')
        if xs[m].shape[1] != xs[0].shape[1]:
            raise ValueError(f'silhouette: the embeddings must have the same features, got {xs[m].shape[1]} and {xs[0].shape[1]}')
    x = torch.cat(xs, dim=0)
    N = x.shape[0]
    if x.shape[1] < 1:
        raise ValueError('silhouette: empty input')
    classes, lcode = np.unique(np.concatenate(labs), return_inverse=True)
    lcode = lcode.reshape(-1).astype(np.int64)
    T = len(classes)
    _check_label_count(T, N)
    mod = np.repeat(np.arange(M, dtype=np.int64), [t.shape[0] for t in xs])
    code = lcode * M + mod
    C = T * M
    x_sorted, off, counts = _sorted_by_class(x, code, C)
    label_counts = counts.reshape(T, M).sum(axis=1)
    dev = x.device
    counts_d, label_counts_d = torch.from_numpy(counts).to(dev), torch.from_numpy(label_counts).to(dev)
    own_d = torch.from_numpy(code.astype(np.int32)).to(dev)
    lcode_d = torch.from_numpy(lcode).to(dev)
    lown_d, win0_d = lcode_d.to(torch.int32), (lcode_d * M).to(torch.int32)
    label_w = torch.empty(N, dtype=torch.float64, device=dev)
    mod_w = torch.empty(N, dtype=torch.float64, device=dev)
    D = torch.zeros(T, T, dtype=torch.float64, device=dev)
    for r0, r1, S in _sums_chunks(x, x_sorted, off, C, int(seg_tiles), int(max_workspace), 'silhouette'):
        nv.silhouette_widths(S, counts_d, own_d[r0:r1], win0_d[r0:r1], M, mod_w[r0:r1])
        S3 = S.view(r1 - r0, T, M)
        Sl = S3[:, :, 0].clone()                           # folded over the modality: explicit fp64 adds in modality order
        for m in range(1, M):
            Sl += S3[:, :, m]
        nv.silhouette_widths(Sl, label_counts_d, lown_d[r0:r1], None, T, label_w[r0:r1])
        for t in np.unique(lcode[r0:r1]):                  # column sums per label: a fixed reduction per chunk, chunks in order
            rows = torch.nonzero(lcode_d[r0:r1] == int(t)).reshape(-1)
            D[int(t)] += Sl.index_select(0, rows).sum(dim=0)
    label_w, mod_w, D = label_w.cpu().numpy(), mod_w.cpu().numpy(), D.cpu().numpy()
    per_label = np.full(T, np.nan)
    present = (counts.reshape(T, M) > 0).sum(axis=1)
    for t in range(T):
        if present[t] >= 2:
            per_label[t] = float(np.mean(1.0 - np.abs(mod_w[lcode == t])))
    have = ~np.isnan(per_label)
    return {'label_asw': float(np.mean(label_w)), 'label_widths': label_w,
            'modality_asw': float(np.mean(per_label[have])) if have.any() else float('nan'),
            'modality_asw_per_label': per_label,
            'label_distance': D / (label_counts[:, None] * label_counts[None, :]).astype(np.float64),
            'labels': classes}

"""Alignment metrics on the MI355X: the reference's acceptance numbers on whole data sets, without an N x N matrix.

    foscttm(A, B)                                  JAMIE.test_closer (reference jamie.py:892-915): fraction of samples closer
                                                   than the true match, cell i of A paired with cell i of B
    cross_knn(Q, R, k)                             sklearn NearestNeighbors(k).fit(R).kneighbors(Q), as (idx, dist) [Nq, k]
    label_transfer_accuracy(q, ql, r, rl, k=5)     JAMIE.test_LabelTA (reference jamie.py:943-961): KNeighborsClassifier(k)
                                                   fitted on (r, rl), its accuracy on (q, ql)

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

"""Imputation metrics on the MI355X: the figures the reference reports for `modal_predict` / `impute` (SURVEY.md row 12,
evaluation.py), per feature, between an imputed and a measured [N, d] matrix.

    feature_correlation_mse(imputed, measured)        (r, mse): Pearson correlation and mean squared error, float64 [d]
    feature_auroc(imputed, measured, threshold=0.0)   AUROC of the imputed value against `measured > threshold`, float64 [d]
    imputation_metrics(imputed, measured, threshold)  {'correlation', 'mse', 'auroc'}
    plan(N, d, max_workspace)                         how feature_auroc splits the features (host arithmetic only)

The kernels are in csrc/imputation.hip (include/jamie_hip.h, "Imputation metrics on the device").  The moments are fp64 sums
of values shifted by row 0 of their feature, added in a fixed order: r is NaN exactly where a column is constant.  AUROC comes
from exact integers: the negatives' scores of a group of features are sorted on the device (LDS chunk sort + rank-merge passes),
every positive is ranked in them, and U2 = sum over positives of (2 #{negatives below} + #{negatives tied}) -- twice the
Mann-Whitney U -- is divided by 2 n_pos n_neg in float64 on the host; NaN where a feature has one class.  Device memory above the
inputs is 8 bytes per cell and feature of a group; the groups are sized to `max_workspace`.
"""
import math

import numpy as np
import torch

from . import _native as nv
from .metrics import _device_input

CHUNK = 4096            # keys one workgroup sorts in LDS (csrc/key_sort.h): runs start at this length, N is padded to it
ROW_BLOCK = 512         # rows per workgroup of the moments pass
MAX_GROUP = 32768       # features per launch


def plan(N, d, max_workspace=1 << 30):
    """The schedule of feature_auroc on [N, d] under a workspace cap in bytes: `groups` [(first feature, features)], `Npad` (N up to
    a multiple of CHUNK), `runs` (sorted chunks per feature), `passes` (rank-merge passes: ceil(log2 runs)), `workspace` (bytes
    allocated: two uint32 key buffers for the largest group)."""
    N, d, max_workspace = int(N), int(d), int(max_workspace)
    if N < 2 or d < 1:
        raise ValueError(f'imputation metrics need N >= 2 cells and d >= 1 features, got N = {N}, d = {d}')
    Npad = (N + CHUNK - 1) // CHUNK * CHUNK
    per_feature = 2 * 4 * Npad
    dg = min(d, max_workspace // per_feature, MAX_GROUP)
    if dg < 1:
        raise ValueError(f'max_workspace = {max_workspace} bytes is less than the {per_feature} one feature of {N} cells needs')
    runs = Npad // CHUNK
    return {'groups': [(f0, min(dg, d - f0)) for f0 in range(0, d, dg)], 'Npad': Npad, 'runs': runs,
            'passes': int(math.ceil(math.log2(runs))) if runs > 1 else 0, 'workspace': per_feature * dg}


def _shape(X):
    return tuple(X.shape) if hasattr(X, 'shape') else np.asarray(X).shape


def _check_pair(imputed, measured, what):
    si, sm = _shape(imputed), _shape(measured)
    if len(si) != 2 or len(sm) != 2:
        raise ValueError(f'{what}: inputs must be 2-D [cells, features], got shapes {si} and {sm}')
    if si != sm:
        raise ValueError(f'{what}: imputed and measured values must have the same shape, got {si} and {sm}')
    if si[0] < 2 or si[1] < 1:
        raise ValueError(f'{what}: N >= 2 cells and d >= 1 features are needed, got shape {si}')
    return si


def _pair_on_device(imputed, measured, device, what):
    x, y = _device_input(imputed, device, what), _device_input(measured, device, what)
    if x.device != y.device:
        y = y.to(x.device)
    return x, y


def feature_correlation_mse(imputed, measured, device='cuda'):
    """(r, mse), float64 numpy [d]: per-feature Pearson correlation (NaN where a column of either input is constant) and mean
    squared error."""
    _check_pair(imputed, measured, 'feature_correlation_mse')
    return _stats(*_pair_on_device(imputed, measured, device, 'feature_correlation_mse'))


def _stats(x, y):
    N, d = x.shape
    out = torch.empty(2, d, dtype=torch.float64, device=x.device)
    ws = torch.empty(nv.imputation_workspace(N, d, 0), dtype=torch.uint8, device=x.device)
    nv.feature_stats(x, y, out[0], out[1], ws)
    o = out.cpu().numpy()
    return o[0].copy(), o[1].copy()


def _threshold(threshold, d):
    t = np.asarray(threshold, dtype=np.float64)
    if t.ndim == 0:
        t = np.full(d, float(t))
    if t.shape != (d,):
        raise ValueError(f'feature_auroc: threshold must be a scalar or one value per feature [{d}], got shape {t.shape}')
    if not np.all(np.isfinite(t)):
        raise ValueError('feature_auroc: threshold contains NaN or infinity')
    return t.astype(np.float32)


def auroc_from_counts(U2, n_pos, N):
    """U2 / (2 n_pos n_neg) in float64; NaN where a feature has no positive or no negative."""
    U2, n_pos = np.asarray(U2, dtype=np.int64), np.asarray(n_pos, dtype=np.int64)
    pairs = 2.0 * n_pos.astype(np.float64) * (int(N) - n_pos).astype(np.float64)
    out = np.full(U2.shape, np.nan)
    np.divide(U2.astype(np.float64), pairs, out=out, where=pairs > 0)
    return out


def feature_auroc(imputed, measured, threshold=0.0, max_workspace=1 << 30, return_counts=False, device='cuda'):
    """Per-feature AUROC of the imputed value as a score for `measured > threshold` (strict; a scalar or one threshold per
    feature, rounded to fp32 and compared in fp32), ties at 1/2 as sklearn's `roc_auc_score`: float64 numpy [d], NaN where a feature
    has one class.  `max_workspace`:
    cap in bytes on the device memory used above the inputs; the features go in groups that respect it.  `return_counts`: also
    (U2, n_pos) as int64 numpy [d], the exact integers the figure is formed from."""
    N, d = _check_pair(imputed, measured, 'feature_auroc')
    thr = _threshold(threshold, d)
    p = plan(N, d, max_workspace)
    auc, counts = _auroc(*_pair_on_device(imputed, measured, device, 'feature_auroc'), thr, p)
    if return_counts:
        return auc, counts
    return auc


def _auroc(x, y, thr, p):
    N, d = x.shape
    t = torch.from_numpy(thr).to(x.device)
    counts = torch.empty(2, d, dtype=torch.int64, device=x.device)
    ws = torch.empty(p['workspace'], dtype=torch.uint8, device=x.device)
    for f0, dg in p['groups']:
        nv.feature_auroc(x, y, t, f0, dg, counts[0], counts[1], ws)
    c = counts.cpu().numpy()
    n_pos, U2 = c[0].copy(), c[1].copy()
    return auroc_from_counts(U2, n_pos, N), (U2, n_pos)


def imputation_metrics(imputed, measured, threshold=0.0, max_workspace=1 << 30, device='cuda'):
    """{'correlation', 'mse', 'auroc'}: float64 numpy [d] each.  The inputs go to the device once."""
    N, d = _check_pair(imputed, measured, 'imputation_metrics')
    thr = _threshold(threshold, d)
    p = plan(N, d, max_workspace)
    x, y = _pair_on_device(imputed, measured, device, 'imputation_metrics')
    r, mse = _stats(x, y)
    return {'correlation': r, 'mse': mse, 'auroc': _auroc(x, y, thr, p)[0]}

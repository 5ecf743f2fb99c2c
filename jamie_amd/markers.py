"""Marker features per group on the MI355X: which features mark each cluster or cell type (scanpy's `rank_genes_groups`), every
group against the rest, for one [N, d] matrix of cells x features -- measured values or the matrix `modal_predict` imputes.

    rank_features(data, labels, n_top=25, tie_correct=True, max_workspace=1 << 30)   the dict below
    group_rank_sums(x, layout, plan)          (rank_sum2 [G, d], tie_term [d]): the exact integers, int64 numpy
    group_moments(x, layout)                  (pivot [d], sums [G, d, 2]): the shifted fp64 sums
    finish(groups, n, rank_sum2, tie_term, pivot, sums, n_top, tie_correct)   every statistic in float64 (host arithmetic only)
    plan(N, d, max_workspace)                 how the rank sums split the features (host arithmetic only)

The kernels are in csrc/markers.hip (include/jamie_hip.h, "Marker features on the device").  The Wilcoxon rank-sum
statistics come from exact integers: the values of a group of features are sorted on the device per feature, every cell finds lb =
#{cells below it} and ub = #{cells not above it}, lb + ub + 1 is twice its midrank and (ub - lb)^2 - 1 summed over the cells is
the tie term.  The moments are fp64 sums of values shifted by row 0 of their feature, added in a fixed order.  `finish` is shared
with the float64 host route (jamie.py `_host_rank_features`): equal integers give bit-equal `z`, `pvals`, `auroc` and `ranking`.
At most N = 2^21 = 2 097 152 cells: the tie term of a constant feature, N^3 - N, then fits 64 bits and twice a rank fits 32.
"""
import math

import numpy as np
import torch

from . import _native as nv
from .metrics import _device_input

CHUNK = 4096            # keys one workgroup sorts in LDS (csrc/key_sort.h): runs start at this length, N is padded to it
PIECE = 512             # cells per workgroup of the moments pass (csrc/markers.hip)
MAX_GROUP = 32768       # features per launch
MAX_CELLS = 1 << 21     # N^3 - N < 2^63


def plan(N, d, max_workspace=1 << 30):
    """The schedule of the rank sums on [N, d] under a workspace cap in bytes: `groups` [(first feature, features)], `Npad` (N up to
    a multiple of CHUNK), `runs` (sorted chunks per feature), `passes` (rank-merge passes: ceil(log2 runs)), `workspace` (bytes
    allocated: two uint32 key buffers for the largest group)."""
    N, d, max_workspace = int(N), int(d), int(max_workspace)
    if N < 2 or d < 1:
        raise ValueError(f'rank_features needs N >= 2 cells and d >= 1 features, got N = {N}, d = {d}')
    if N > MAX_CELLS:
        raise ValueError(f'rank_features takes at most 2^21 = {MAX_CELLS} cells (the tie term N^3 - N must fit 64 bits), got N = {N}')
    Npad = (N + CHUNK - 1) // CHUNK * CHUNK
    per_feature = 2 * 4 * Npad
    dg = min(d, max_workspace // per_feature, MAX_GROUP)
    if dg < 1:
        raise ValueError(f'max_workspace = {max_workspace} bytes is less than the {per_feature} one feature of {N} cells needs')
    runs = Npad // CHUNK
    return {'groups': [(f0, min(dg, d - f0)) for f0 in range(0, d, dg)], 'Npad': Npad, 'runs': runs,
            'passes': int(math.ceil(math.log2(runs))) if runs > 1 else 0, 'workspace': per_feature * dg}


def check_rank_features(data, labels, n_top, what='rank_features'):
    """(N, d, labels as a numpy array, n_top) from shapes alone: nothing is allocated or copied to the device."""
    shape = tuple(data.shape) if hasattr(data, 'shape') else np.asarray(data).shape
    if len(shape) != 2:
        raise ValueError(f'{what}: data must be 2-D [cells, features], got shape {shape}')
    N, d = int(shape[0]), int(shape[1])
    if N < 2 or d < 1:
        raise ValueError(f'{what}: N >= 2 cells and d >= 1 features are needed, got shape {shape}')
    if N > MAX_CELLS:
        raise ValueError(f'{what}: at most 2^21 = {MAX_CELLS} cells (the tie term N^3 - N must fit 64 bits), got N = {N}')
    labels = labels.detach().cpu().numpy() if torch.is_tensor(labels) else np.asarray(labels)
    if labels.ndim != 1 or len(labels) != N:
        raise ValueError(f'{what}: one label per cell is needed, got labels of shape {labels.shape} for {N} cells')
    if int(n_top) != n_top or n_top < 1:
        raise ValueError(f'{what}: n_top must be a positive integer, got {n_top!r}')
    return N, d, labels, int(n_top)


def group_layout(labels):
    """The cells in group order: `groups` (the sorted unique labels), `n` (their sizes, int64), `codes` (group index per cell),
    `order` (stable argsort of the codes, int32), `sorted_codes` (int32), `seg_off` [G + 1] (where each group starts in `order`)
    and `piece_off` [G + 1] (pieces of PIECE cells before each group), int32."""
    groups, codes = np.unique(labels, return_inverse=True)
    codes = codes.reshape(-1)
    n = np.bincount(codes, minlength=len(groups)).astype(np.int64)
    order = np.argsort(codes, kind='stable').astype(np.int32)
    seg_off = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
    piece_off = np.concatenate([[0], np.cumsum(-(-n // PIECE))]).astype(np.int32)
    return {'groups': groups, 'n': n, 'codes': codes, 'order': order, 'sorted_codes': codes[order].astype(np.int32),
            'seg_off': seg_off, 'piece_off': piece_off}


def _bh(p):
    """Benjamini-Hochberg over the last axis; NaN entries are left out and stay NaN."""
    out = np.full(p.shape, np.nan)
    for g in range(p.shape[0]):
        ok = np.where(~np.isnan(p[g]))[0]
        m = len(ok)
        if m == 0:
            continue
        by = ok[np.argsort(p[g, ok], kind='stable')]
        adj = p[g, by] * m / np.arange(1, m + 1)
        out[g, by] = np.minimum(np.minimum.accumulate(adj[::-1])[::-1], 1.0)
    return out


def finish(groups, n, rank_sum2, tie_term, pivot, sums, n_top=25, tie_correct=True):
    """Every statistic of `rank_features` in float64 from the group sizes `n` [G], the integers `rank_sum2` [G, d] and `tie_term`
    [d], and the moments `sums` [G, d, 2] of x - `pivot` [d].  Both routes end here."""
    from scipy.special import ndtr, stdtr
    n = np.asarray(n, dtype=np.int64)
    rank_sum2, tie_term = np.asarray(rank_sum2, dtype=np.int64), np.asarray(tie_term, dtype=np.int64)
    pivot, sums = np.asarray(pivot, dtype=np.float64), np.asarray(sums, dtype=np.float64)
    G, d = rank_sum2.shape
    N = int(n.sum())
    U2 = rank_sum2 - (n * (n + 1))[:, None]
    ng = n.astype(np.float64)[:, None]
    nr = N - ng
    pairs = ng * nr
    constant = np.array([int(t) == N ** 3 - N for t in tie_term])             # (exact: Python integers)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        auroc = np.where(pairs > 0, U2 / (2.0 * pairs), np.nan)
        tie = tie_term.astype(np.float64) / (N * (N - 1.0)) if tie_correct else np.zeros(d)
        sd = np.sqrt(pairs / 12.0 * ((N + 1.0) - tie)[None, :])
        z = np.where((pairs > 0) & ~constant[None, :] & (sd > 0), (U2 / 2.0 - pairs / 2.0) / sd, np.nan)
        pvals = np.minimum(2.0 * ndtr(-np.abs(z)), 1.0)

        # the moments of the rest: the totals, added in ascending group order, minus the group's
        total = np.add.accumulate(sums, axis=0)[-1]
        s1, s2 = sums[:, :, 0], sums[:, :, 1]
        r1, r2 = total[None, :, 0] - s1, total[None, :, 1] - s2
        shifted, shifted_rest = np.where(ng > 0, s1 / ng, np.nan), np.where(nr > 0, r1 / nr, np.nan)
        mean, mean_rest = pivot[None, :] + shifted, pivot[None, :] + shifted_rest
        var = np.where(ng > 1, np.maximum(s2 - s1 * s1 / ng, 0.0) / (ng - 1.0), np.nan)
        var_rest = np.where(nr > 1, np.maximum(r2 - r1 * r1 / nr, 0.0) / (nr - 1.0), np.nan)
        mean_difference = shifted - shifted_rest
        a, b = var / ng, var_rest / nr
        defined = (ng > 1) & (nr > 1) & ((var > 0) | (var_rest > 0))
        t = np.where(defined, mean_difference / np.sqrt(a + b), np.nan)
        t_df = np.where(defined, (a + b) ** 2 / (a * a / (ng - 1.0) + b * b / (nr - 1.0)), np.nan)
        t_pvals = np.minimum(2.0 * stdtr(t_df, -np.abs(t)), 1.0)
        logfoldchanges = np.log2((np.expm1(mean) + 1e-9) / (np.expm1(mean_rest) + 1e-9))
    top = min(int(n_top), d)
    ranking = np.stack([np.argsort(-z[g], kind='stable')[:top] for g in range(G)]).astype(np.int64)   # (NaN sorts last)
    return {'groups': groups, 'n': n, 'rank_sum2': rank_sum2, 'tie_term': tie_term, 'U2': U2, 'auroc': auroc, 'z': z, 'pvals': pvals,
            'pvals_adj': _bh(pvals), 'mean': mean, 'var': var, 'mean_rest': mean_rest, 'var_rest': var_rest, 't': t, 't_df': t_df,
            't_pvals': t_pvals, 'logfoldchanges': logfoldchanges, 'mean_difference': mean_difference, 'ranking': ranking}


def _to_device(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def group_rank_sums(x, layout, p):
    """(rank_sum2 [G, d], tie_term [d]) as int64 numpy for the fp32 device matrix `x`, a `group_layout` and a `plan`."""
    N, d = x.shape
    G = len(layout['n'])
    order, codes = _to_device(layout['order'], x.device), _to_device(layout['sorted_codes'], x.device)
    R2 = torch.empty(d, G, dtype=torch.int64, device=x.device)
    tie = torch.empty(d, dtype=torch.int64, device=x.device)
    ws = torch.empty(p['workspace'], dtype=torch.uint8, device=x.device)
    for f0, dg in p['groups']:
        nv.group_rank_sums(x, order, codes, G, f0, dg, R2, tie, ws)
    return np.ascontiguousarray(R2.cpu().numpy().T), tie.cpu().numpy()


def group_moments(x, layout):
    """(pivot [d], sums [G, d, 2]) as float64 numpy: row 0 of `x` and, per group and feature, the sum and the sum of squares of
    x - pivot."""
    N, d = x.shape
    G = len(layout['n'])
    order = _to_device(layout['order'], x.device)
    seg_off, piece_off = _to_device(layout['seg_off'], x.device), _to_device(layout['piece_off'], x.device)
    sums = torch.empty(G, d, 2, dtype=torch.float64, device=x.device)
    ws = torch.empty(nv.markers_workspace(N, d, G, 0), dtype=torch.uint8, device=x.device)
    nv.group_moments(x, order, seg_off, piece_off, G, int(layout['piece_off'][-1]), sums, ws)
    return x[0].to(torch.float64).cpu().numpy(), sums.cpu().numpy()


def rank_features(data, labels, n_top=25, tie_correct=True, max_workspace=1 << 30, device='cuda'):
    """One-vs-rest marker statistics of every feature of `data` [N, d] (numpy or a tensor; converted to fp32 once) for every group
    of `labels` [N] (any dtype `np.unique` sorts), 2 <= N <= 2^21 cells.  A dict of float64 / int64 numpy:

    `groups` [G] the sorted unique labels and `n` [G] their sizes;
    `rank_sum2` [G, d] twice the sum of the midranks of the group's cells among all N cells of the feature, `tie_term` [d] the sum
    of t^3 - t over the feature's tie groups, `U2` = rank_sum2 - n_g (n_g + 1) twice the Mann-Whitney U of group against rest: exact
    integers;
    `auroc` = U2 / (2 n_g n_rest); `z` = (U - n_g n_r / 2) / sqrt(n_g n_r / 12 ((N + 1) - tie_term / (N (N - 1)))), the normal
    approximation without continuity correction (`tie_correct=False` drops the tie term: scanpy's default); `pvals` two-sided;
    `pvals_adj` Benjamini-Hochberg over the features of each group;
    `mean`, `var` (ddof = 1), `mean_rest`, `var_rest`; `t`, `t_df`, `t_pvals` Welch's t-test of group against rest;
    `mean_difference`; `logfoldchanges` = log2((expm1(mean) + 1e-9) / (expm1(mean_rest) + 1e-9)), scanpy's formula, which assumes
    log1p data (NaN where that ratio is not positive or both sides overflow);
    `ranking` [G, min(n_top, d)] feature indices by descending `z`, NaN last, ties by ascending index.

    NaN exactly where a statistic is undefined: `auroc`, `z` and the figures of the rest with a single group (n_rest = 0); `z`
    also where the feature is constant; `var` (`var_rest`) where the group (the rest) has fewer than 2 cells; `t` where a side has
    fewer than 2 cells or both variances are 0.  Values compare as fp32 numbers, -0.0 ties with +0.0.  `max_workspace`: cap in
    bytes on the device memory of the sort (8 bytes per cell and feature of a group of features)."""
    N, d, labels, n_top = check_rank_features(data, labels, n_top)
    p = plan(N, d, max_workspace)
    layout = group_layout(labels)
    x = _device_input(data, device, 'rank_features')
    rank_sum2, tie_term = group_rank_sums(x, layout, p)
    pivot, sums = group_moments(x, layout)
    return finish(layout['groups'], layout['n'], rank_sum2, tie_term, pivot, sums, n_top, tie_correct)

"""Sparse (CSR) cell matrices on the MI355X: `preclass(axis=0)` (reference utilities.py:654-678) for a scipy sparse matrix of
[cells, features] -- the form an AnnData `.X` has -- without a dense copy of the input on the host or the device.

    canonical_csr(X)                     scipy CSR, duplicates summed, indices sorted, int64 indptr, int32 indices, fp32 / fp64 values
    standardise_csr(X, device)           (standardised fp32 [N, d] device tensor, mean f64 [d], sd f64 [d]): the sparse counterpart of
                                         `_native.standardise_columns`
    apply_csr(X, mean, sd, device)       standardised fp32 rows of a CSR matrix (or a row chunk of one) against given statistics
    plan(colptr)                         the segments of the statistics pass and its workspace (host arithmetic only)

The kernels are in csrc/sparse_input.hip (include/jamie_hip.h, "Sparse cell matrices").  Statistics: the stored values go up in CSC
order with the column pointers (no row indices); a column is cut into segments of SEGMENT stored entries, every segment gives one fp64
partial and a column's partials are added in ascending order, so the result does not depend on the grid and is bit-identical from run
to run.  mean = sum / N; sd = sqrt((sum of the stored (v - mean)^2 + (N - n_c) mean^2) / N): numpy's two-pass order with the
structural zeros' deviations taken in closed form.  Densify: `jamie_csr_standardise` writes (x - mean) / sd in fp64, NaN -> 0, rounded to
fp32 -- the expression of `jamie_standardise` and of the host's `preclass.transform(...)` followed by `.float()`, equal to both to the bit.
"""
import numpy as np
import scipy.sparse as sp
import torch

from . import _native as nv

SEGMENT = 4096          # stored entries per statistics segment (csrc/sparse_input.hip: SP_SEG)
WINDOW = 4096           # columns per LDS window of the densify kernel (SP_WIN)


def plan(colptr):
    """The statistics pass on a matrix with these column pointers: `seg_off` (int64 [d + 1]: segments of the columns before c),
    `segments` (their number) and `workspace` (bytes: one fp64 partial per segment).  Needs no GPU."""
    cp = np.asarray(colptr, dtype=np.int64)
    if cp.ndim != 1 or len(cp) < 2:
        raise ValueError(f'plan: colptr must be a 1-D array of d + 1 >= 2 entries, got shape {cp.shape}')
    n = np.diff(cp)
    if (n < 0).any():
        raise ValueError('plan: colptr decreases')
    seg_off = np.concatenate([np.zeros(1, np.int64), np.cumsum(-(-n // SEGMENT))])
    return {'seg_off': seg_off, 'segments': int(seg_off[-1]), 'workspace': 8 * int(seg_off[-1])}


def _check_compressed(X):
    """indptr / indices of a CSR or CSC matrix as handed in (scipy does not check them when a matrix is built from its arrays)."""
    major, minor = X.shape if X.format == 'csr' else X.shape[::-1]
    indptr, indices = np.asarray(X.indptr), np.asarray(X.indices)
    if len(indptr) != major + 1 or indptr[0] != 0 or indptr[-1] != len(indices) or len(indices) != len(X.data) \
            or (np.diff(indptr) < 0).any():
        raise ValueError(f'sparse input: inconsistent index pointers (format {X.format}, shape {X.shape})')
    if len(indices) and (indices.min() < 0 or indices.max() >= minor):
        raise ValueError(f'sparse input: an index lies outside [0, {minor}) (format {X.format}, shape {X.shape})')


def canonical_csr(X):
    """scipy CSR with `sum_duplicates()`, `sort_indices()`, int64 indptr and int32 indices; values fp32 or fp64 (any other dtype,
    e.g. integer counts, becomes fp64, as dense input does).  Works on a copy.  ValueError: not a sparse 2-D matrix, an index
    outside its range, 2^31 or more features."""
    if not sp.issparse(X):
        raise ValueError(f'canonical_csr needs a scipy sparse matrix, got {type(X).__name__}')
    if len(X.shape) != 2:
        raise ValueError(f'sparse input must be 2-D [cells, features], got shape {X.shape}')
    if X.shape[1] >= 2 ** 31:
        raise ValueError(f'sparse input: {X.shape[1]} features; column indices are int32 (fewer than 2^31 features)')
    if X.format in ('csr', 'csc'):
        _check_compressed(X)
    A = sp.csr_matrix(X, copy=True)
    if A.dtype not in (np.float32, np.float64):
        A = A.astype(np.float64)
    A.sum_duplicates()
    A.sort_indices()
    _check_compressed(A)
    A.indptr = np.ascontiguousarray(A.indptr, dtype=np.int64)
    A.indices = np.ascontiguousarray(A.indices, dtype=np.int32)
    return A


def _up(a, dtype, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)


def _stats_arg(v, d, dev, what):
    t = (v if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(np.asarray(v), dtype=np.float64)))
    t = t.to(dev, torch.float64).contiguous().reshape(-1)
    if t.numel() != d:
        raise ValueError(f'apply_csr: {what} has {t.numel()} entries for {d} features')
    return t


def column_stats(A, device='cuda', csc=None):
    """(mean, sd) fp64 [d] device tensors of a canonical CSR matrix (`csc`: its `.tocsc()` where the caller already holds it)."""
    dev = torch.device(device)
    N, d = A.shape
    if N < 1 or d < 1:
        raise ValueError(f'sparse input: N >= 1 cells and d >= 1 features are needed, got shape {A.shape}')
    csc = A.tocsc() if csc is None else csc
    p = plan(csc.indptr)
    vals = torch.from_numpy(np.ascontiguousarray(csc.data)).to(dev)
    colptr, seg_off = _up(csc.indptr, np.int64, dev), _up(p['seg_off'], np.int64, dev)
    del csc
    mean = torch.empty(d, dtype=torch.float64, device=dev)
    sd = torch.empty(d, dtype=torch.float64, device=dev)
    ws = torch.empty(p['workspace'], dtype=torch.uint8, device=dev)
    nv.csc_col_stats(vals, colptr, seg_off, p['segments'], N, mean, sd, ws)
    return mean, sd


def _densify(A, mean, sd, dev):
    N, d = A.shape
    out = torch.empty(N, d, dtype=torch.float32, device=dev)
    if N == 0:
        return out
    indptr, indices = _up(A.indptr, np.int64, dev), _up(A.indices, np.int32, dev)
    vals = torch.from_numpy(np.ascontiguousarray(A.data)).to(dev)
    ws = torch.empty(nv.sparse_workspace(None, d, 1), dtype=torch.uint8, device=dev)
    nv.csr_standardise(indptr, indices, vals, d, mean, sd, out, ws)
    return out


def standardise_csr(X, device='cuda'):
    """Device `preclass(axis=0)` of a scipy sparse matrix: (fp32 standardised [N, d], mean [d] f64, sd [d] f64) on `device`.  The
    CSC-ordered values and column pointers go up for the statistics and are freed, then the CSR arrays go up and are densified."""
    A = canonical_csr(X)
    mean, sd = column_stats(A, device)
    return _densify(A, mean, sd, torch.device(device)), mean, sd


def apply_csr(X, mean, sd, device='cuda', canonical=False):
    """Standardised fp32 [n, d] device rows of a sparse matrix (a row chunk of one) against `mean` / `sd` (numpy or tensors; device
    tensors are used as they are).  `canonical`: X already comes from `canonical_csr` (a row slice of such a matrix is one)."""
    dev = torch.device(device)
    A = X if canonical else canonical_csr(X)
    d = A.shape[1]
    if d < 1:
        raise ValueError(f'sparse input: d >= 1 features are needed, got shape {A.shape}')
    return _densify(A, _stats_arg(mean, d, dev, 'mean'), _stats_arg(sd, d, dev, 'sd'), dev)

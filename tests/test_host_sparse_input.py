"""Sparse cell matrices without a GPU: the exported symbols, the plan / workspace arithmetic, `canonical_csr`, the device's
statistics restated in numpy (in the kernel's segment order) against float64 numpy, the facade's host preprocessing of CSR input
and the new kernels' code objects."""
import os
import re
import sys

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import sparse_util as su  # noqa: E402

SYMBOLS = ('jamie_sparse_workspace', 'jamie_csc_col_stats', 'jamie_csr_standardise')


def test_symbols_are_declared_and_exported():
    from jamie_amd import _native as nv
    hdr = open(os.path.join(ROOT, 'include', 'jamie_hip.h')).read()
    assert 'Sparse cell matrices' in hdr
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    handle = nv.load()
    for name in SYMBOLS:
        assert re.search(r'\b' + name + r'\s*\(', code), name
        assert name in nv.EXPORTS and hasattr(handle, name), name


def _colptr(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def test_plan_agrees_with_the_workspace_function():
    from jamie_amd import _native as nv
    from jamie_amd import sparse_input as jsp
    S = jsp.SEGMENT
    assert S >= 256 and jsp.WINDOW >= 1024
    cases = [([0], 0), ([S], 1), ([S + 1], 2), ([3 * S], 3), ([0, 5, 0], 1), ([S - 1, S, S + 1, 3 * S, 0, 1, 3 * S + 1], 1 + 1 + 2 + 3 + 0 + 1 + 4),
             ([7] * 203, 203), ([0] * 9, 0)]
    for counts, segs in cases:
        cp = _colptr(counts)
        p = jsp.plan(cp)
        assert p['segments'] == segs and p['workspace'] == 8 * segs, (counts, p)
        assert nv.sparse_workspace(cp, len(counts), 0) == p['workspace'], counts
        so = p['seg_off']
        assert so.dtype == np.int64 and so[0] == 0 and so[-1] == segs and len(so) == len(cp)
        assert np.array_equal(np.diff(so), -(-np.diff(cp) // S))
    for d in (1, 3, 203, 8200):
        assert nv.sparse_workspace(None, d, 1) == 4 * d
    assert nv.sparse_workspace(None, 5, 0) == 0 and nv.sparse_workspace(_colptr([3]), 1, 2) == 0 and nv.sparse_workspace(None, 0, 1) == 0
    with pytest.raises(ValueError):
        jsp.plan(np.array([0, 5, 3]))
    with pytest.raises(ValueError):
        jsp.plan(np.array([0]))


def test_canonical_csr():
    from jamie_amd import sparse_input as jsp
    # duplicates and unsorted indices, integer counts, handed in as COO
    rows, cols = np.array([0, 0, 0, 2, 2, 1]), np.array([3, 1, 3, 0, 0, 2])
    data = np.array([1, 2, 4, 8, 16, 0], dtype=np.int64)
    X = sp.coo_matrix((data, (rows, cols)), shape=(4, 5))
    A = jsp.canonical_csr(X)
    assert sp.issparse(A) and A.format == 'csr' and A.shape == (4, 5)
    assert A.dtype == np.float64 and A.indptr.dtype == np.int64 and A.indices.dtype == np.int32
    assert A.indptr.tolist() == [0, 2, 3, 4, 4] and A.indices.tolist() == [1, 3, 2, 0] and A.data.tolist() == [2.0, 5.0, 0.0, 24.0]
    assert A.has_sorted_indices
    # ... and as an unsorted CSR with duplicates; the caller's matrix is left alone
    U = sp.csr_matrix((np.array([1., 2., 4.], np.float32), np.array([3, 1, 3]), np.array([0, 3, 3])), shape=(2, 5))
    before = (U.data.copy(), U.indices.copy(), U.indptr.copy())
    B = jsp.canonical_csr(U)
    assert B.dtype == np.float32 and B.indices.tolist() == [1, 3] and B.data.tolist() == [2.0, 5.0]
    assert np.array_equal(U.data, before[0]) and np.array_equal(U.indices, before[1]) and np.array_equal(U.indptr, before[2])
    assert U.nnz == 3
    for fmt in ('csc', 'coo', 'lil'):
        C = jsp.canonical_csr(sp.random(30, 17, 0.2, format=fmt, random_state=3, dtype=np.float64))
        assert C.format == 'csr' and C.indptr.dtype == np.int64 and C.indices.dtype == np.int32
    D = sp.random(30, 17, 0.2, format='csc', random_state=3, dtype=np.float64)
    assert np.array_equal(jsp.canonical_csr(D).toarray(), D.toarray())
    assert jsp.canonical_csr(sp.csr_matrix((3, 4), dtype=np.bool_)).dtype == np.float64
    # the documented errors
    with pytest.raises(ValueError):
        jsp.canonical_csr(np.zeros((3, 4)))
    if hasattr(sp, 'coo_array'):
        with pytest.raises(ValueError):
            jsp.canonical_csr(sp.coo_array(np.arange(5.0)))                    # 1-D
    for bad in (np.array([0, 5]), np.array([-1, 2])):                          # an index outside [0, d)
        M = sp.csr_matrix((3, 5), dtype=np.float64)
        M.data, M.indices, M.indptr = np.ones(2), bad.astype(np.int32), np.array([0, 2, 2, 2], np.int32)
        with pytest.raises(ValueError):
            jsp.canonical_csr(M)
    M = sp.csc_matrix((3, 5), dtype=np.float64)
    M.data, M.indices, M.indptr = np.ones(1), np.array([3], np.int32), np.array([0, 1, 1, 1, 1, 1], np.int32)
    with pytest.raises(ValueError):
        jsp.canonical_csr(M)                                                   # row 3 of 3
    with pytest.raises(ValueError):
        jsp.canonical_csr(sp.csr_matrix((2, 2 ** 31), dtype=np.float32))       # d >= 2^31


def test_restated_statistics_equal_float64_numpy():
    from jamie_amd import sparse_input as jsp
    S = jsp.SEGMENT
    N, d = 2 * S + 37, 203
    A, X = su.sparse_counts(N, d)
    csc = jsp.canonical_csr(A).tocsc()
    assert csc.indptr[su.FULL_COL + 1] - csc.indptr[su.FULL_COL] == N == csc.indptr[su.CONST_COL + 1] - csc.indptr[su.CONST_COL]
    assert csc.indptr[su.EMPTY_COL + 1] == csc.indptr[su.EMPTY_COL] and csc.indptr[su.ONE_COL + 1] - csc.indptr[su.ONE_COL] == 1
    assert jsp.plan(csc.indptr)['segments'] >= d - 1 + 2 * 2           # the two full columns span three segments each
    assert 0.08 < A.nnz / (N * d) < 0.16
    mean, sd = su.restated_stats(csc.data, csc.indptr, N, S)
    ref_mean, ref_sd = X.mean(0), X.std(0)
    print(f'restated statistics on {N} x {d}: max |mean - ref| {np.abs(mean - ref_mean).max():.3e}, '
          f'max relative sd error {np.max(np.abs(sd - ref_sd)[ref_sd > 0] / ref_sd[ref_sd > 0]):.3e}')
    np.testing.assert_allclose(mean, ref_mean, **su.MEAN_TOL)
    np.testing.assert_allclose(sd, ref_sd, **su.SD_TOL)
    assert sd[su.EMPTY_COL] == 0.0 and mean[su.EMPTY_COL] == 0.0
    assert sd[su.CONST_COL] == 0.0 and mean[su.CONST_COL] == su.CONST
    assert ref_mean[su.OFFSET_COL] > 500 and sd[su.OFFSET_COL] > 1000


def test_host_preprocessing_of_csr_input_equals_dense():
    """`_build_preprocessing()` densifies sparse modalities on the host: the same statistics as with the dense arrays."""
    from jamie_amd import JAMIE
    from jamie_amd.utilities import preclass
    data = [su.sparse_counts(300, 24, 1), su.sparse_counts(300, 17, 2)]
    pres = []
    for which in (0, 1):
        jm = JAMIE(preprocess='host', pca_dim=None)
        jm.dataset = [pair[which] for pair in data]
        pres.append(jm._build_preprocessing())
    for a, b in zip(*pres):
        assert isinstance(a, preclass) and a.axis == 0 and a.pca is None
        assert a.mean.shape == b.mean.shape and a.mean.ndim == 1
        assert np.array_equal(a.mean, b.mean) and np.array_equal(a.std, b.std)
    # ... and under a per-modality pca_dim of None
    jm = JAMIE(preprocess='host', pca_dim=[None, None])
    jm.dataset = [pair[0] for pair in data]
    for a, b in zip(jm._build_preprocessing(), pres[1]):
        assert np.array_equal(a.mean, b.mean) and np.array_equal(a.std, b.std)


def test_sparse_input_kernels_use_no_scratch():
    """private_segment_fixed_size == 0 for every kernel of csrc/sparse_input.hip, read from the code object hipcc built."""
    import isa_check as ic
    obj = os.path.join(ROOT, 'jamie_amd', 'csrc', '_obj', 'sparse_input.o')
    if not os.path.exists(obj):
        pytest.skip('the library is not built')
    if not os.path.exists(ic.OBJDUMP):
        pytest.skip('llvm-objdump not found')
    meta = ic.kernel_metadata(obj)
    names = ' '.join(meta)
    for kernel in ('csc_moment_kernel', 'csc_finish_kernel', 'zero_row_kernel', 'csr_standardise_kernel'):
        assert kernel in names, (kernel, names)
    assert len(meta) == 6
    for name, m in meta.items():
        assert m['private_segment_fixed_size'] == 0, (name, m)
        assert m.get('vgpr_spill_count', 0) == 0, (name, m)

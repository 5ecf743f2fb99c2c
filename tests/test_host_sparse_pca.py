"""Sparse PCA products without a GPU: the exported symbols, the workspace arithmetic against its restatement, the slot layout of
the long-row partials, the argument checks of the `_native` wrappers and the new kernels' code objects."""
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import sparse_pca_util as pu  # noqa: E402

SYMBOLS = ('jamie_spmm_workspace', 'jamie_csr_spmm', 'jamie_weighted_colsum')


def test_symbols_are_declared_and_exported():
    from jamie_amd import _native as nv
    hdr = open(os.path.join(ROOT, 'include', 'jamie_hip.h')).read()
    assert 'Sparse PCA products' in hdr
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    handle = nv.load()
    for name in SYMBOLS:
        assert re.search(r'\b' + name + r'\s*\(', code), name
        assert name in nv.EXPORTS and hasattr(handle, name), name


def _ptr(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def test_workspace_equals_its_restatement():
    """Two slots of n floats per window of SEGMENT positions, nothing while no row can be long: a function of nnz and n."""
    from jamie_amd import _native as nv
    from jamie_amd import sparse_input, sparse_pca
    S = sparse_pca.SEGMENT
    assert S >= 256 and isinstance(sparse_input.SEGMENT, int)
    for counts in ([0], [1], [S], [S + 1], [3 * S], [0, 1, S, S + 1, 3 * S], [3 * S, 0, 0, 1], [7] * 203, [7] * (S // 7 + 1), [0] * 9):
        cp = _ptr(counts)
        nnz = int(cp[-1])
        for n in (1, 26, 65, 522, 1500):
            want = 8 * n * (-(-nnz // S)) if nnz > S else 0
            assert nv.spmm_workspace(cp, n) == want == sparse_pca.workspace(cp, n), (counts, n)
            # every long-row segment has a slot inside it
            assert all(0 <= 4 * n * (slot + 1) <= want for _, _, slot in pu.slots(cp, S)), (counts, n)
    assert nv.spmm_workspace(_ptr([3 * S]), 0) == 0 and nv.spmm_workspace(_ptr([3 * S]), -1) == 0
    assert nv.spmm_workspace(np.array([0, 3 * S, 2 * S, 4 * S]), 5) == 0 == sparse_pca.workspace(np.array([0, 3 * S, 2 * S, 4 * S]), 5)
    for rows, n in ((1, 1), (512, 3), (513, 3), (5000, 522)):
        assert nv.weighted_colsum_workspace(rows, n) == 8 * n * (-(-rows // sparse_pca.COLSUM_ROWS))


def test_long_row_segments_get_distinct_slots():
    """The partial of segment i of a long row is found from the row's extent alone; no two segments of a matrix share a slot and
    every slot lies inside the workspace, for rows that start and end anywhere relative to the windows."""
    S = 16
    rng = np.random.default_rng(0)
    seen_last_in_start_window = False
    for _ in range(2000):
        counts = rng.choice([0, 1, 3, S - 1, S, S + 1, 2 * S, 2 * S + 1, 3 * S + 5, 40, 7 * S], size=rng.integers(1, 12))
        cp = _ptr(counts)
        sl = pu.slots(cp, S)
        ids = [s for _, _, s in sl]
        windows = -(-int(cp[-1]) // S) if cp[-1] > S else 0
        assert len(set(ids)) == len(ids), (counts, sl)
        assert all(0 <= s < 2 * windows for s in ids), (counts, sl)
        assert len(sl) == sum(-(-c // S) for c in counts if c > S)
        seen_last_in_start_window |= any(s % 2 for s in ids)
    assert seen_last_in_start_window


def test_wrappers_check_their_arguments():
    """Wrong dtypes, a non-unit column stride, ld < n and a short workspace are refused before anything is launched (CPU tensors
    stand in: the checks come first)."""
    from jamie_amd import _native as nv
    from jamie_amd import sparse_pca
    S = sparse_pca.SEGMENT
    E = nv.JamieHipError
    n_rows, n_inner, n = 3, 10, 4
    ptr = torch.tensor([0, 2, 2, 5], dtype=torch.int64)
    idx = torch.tensor([0, 3, 1, 2, 9], dtype=torch.int32)
    vals = torch.ones(5, dtype=torch.float32)
    B = torch.zeros(n_inner, n)
    out = torch.zeros(n_rows, n)

    def spmm(**kw):
        a = dict(indptr=ptr, indices=idx, vals=vals, n_inner=n_inner, B=B, out=out)
        a.update(kw)
        nv.csr_spmm(**a)
    for bad, match in ((dict(vals=vals.half()), 'fp32 / fp64 values'), (dict(indptr=ptr.int()), 'int64 indptr'),
                       (dict(indices=idx.long()), 'int32 indices'), (dict(B=B.double()), 'float32'), (dict(out=out.double()), 'float32'),
                       (dict(B=torch.zeros(n, n_inner).t()), 'unit column stride'), (dict(out=torch.zeros(n, n_rows).t()), 'unit column stride'),
                       (dict(B=B[:, :3], n=n), 'leading dimension'), (dict(out=out[:, :3], n=n), 'leading dimension'),
                       (dict(B=B[:5]), 'n_inner'), (dict(out=out[:2]), 'n_rows'),
                       (dict(t=torch.zeros(n, dtype=torch.float64)), 't must be'), (dict(t=torch.zeros(n), s=torch.zeros(n_rows)), 's must be'),
                       (dict(s=torch.zeros(n_rows, dtype=torch.float64)), 's without t'),
                       (dict(ws=torch.zeros(64, dtype=torch.float32)), 'workspace')):
        with pytest.raises(E, match=match):
            spmm(**bad)
    # a short workspace: nnz > SEGMENT needs 8 n ceil(nnz / SEGMENT) bytes
    nnz = S + 1
    big = dict(indptr=torch.tensor([0, nnz], dtype=torch.int64), indices=torch.zeros(nnz, dtype=torch.int32),
               vals=torch.zeros(nnz, dtype=torch.float64), out=torch.zeros(1, n))
    need = nv.spmm_workspace(np.array([0, nnz]), n)
    assert need == 8 * n * 2
    for ws in (None, torch.zeros(need - 1, dtype=torch.uint8)):
        with pytest.raises(E, match=f'{need} needed'):
            spmm(ws=ws, **big)
    # ... and the checks of the library itself, which launch nothing either
    lib = nv.load()
    buf = (np.zeros(64), np.zeros(64, np.float32))
    p = [a.ctypes.data for a in buf]
    assert lib.jamie_csr_spmm(p[0], p[0], p[0], 0, nnz, 1, n_inner, p[1], n, n, None, None, p[1], n, p[0], need - 1, None) == -1
    assert b'workspace' in lib.jamie_last_error()
    assert lib.jamie_csr_spmm(p[0], p[0], p[0], 0, 5, 1, n_inner, p[1], n - 1, n, None, None, p[1], n, None, 0, None) == -1
    assert lib.jamie_weighted_colsum(p[1], 600, n, n, None, p[1], p[0], 8 * n * 2 - 1, None) == -1

    def colsum(**kw):
        a = dict(B=B, t=torch.zeros(n), ws=torch.zeros(nv.weighted_colsum_workspace(n_inner, n), dtype=torch.uint8))
        a.update(kw)
        nv.weighted_colsum(**a)
    for bad, match in ((dict(B=B.double()), 'float32'), (dict(B=torch.zeros(n, n_inner).t()), 'unit column stride'),
                       (dict(B=B[:, :3], n=n), 'leading dimension'), (dict(t=torch.zeros(n, dtype=torch.float64)), 't must be'),
                       (dict(w=torch.zeros(n_inner)), 'w must be'), (dict(w=torch.zeros(n_inner + 1, dtype=torch.float64)), 'w must be'),
                       (dict(ws=torch.zeros(8 * n - 1, dtype=torch.uint8)), 'needed'), (dict(ws=None), 'needed')):
        with pytest.raises(E, match=match):
            colsum(**bad)


def test_sparse_pca_kernels_use_no_scratch():
    """private_segment_fixed_size == 0 for every kernel of csrc/sparse_pca.hip, read from the code object hipcc built: the
    accumulators of every panel width stay in registers."""
    import isa_check as ic
    obj = os.path.join(ROOT, 'jamie_amd', 'csrc', '_obj', 'sparse_pca.o')
    if not os.path.exists(obj):
        pytest.skip('the library is not built')
    if not os.path.exists(ic.OBJDUMP):
        pytest.skip('llvm-objdump not found')
    meta = ic.kernel_metadata(obj)
    names = ' '.join(meta)
    for kernel in ('spmm_segment_kernel', 'spmm_row_kernel', 'wcs_partial_kernel', 'wcs_finish_kernel'):
        assert kernel in names, (kernel, names)
    assert len(meta) == 2 * 2 * 8 + 2                      # (segment, row) x (fp32, fp64) x 8 panel widths + the two column-sum kernels
    for name, m in meta.items():
        assert m['private_segment_fixed_size'] == 0, (name, m)
        assert m.get('vgpr_spill_count', 0) == 0, (name, m)

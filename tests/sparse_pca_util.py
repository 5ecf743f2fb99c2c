"""Test data, float64 references and the derived error bound for the sparse PCA tests (tests/test_host_sparse_pca.py,
tests/test_hip_sparse_pca.py)."""
import numpy as np
import scipy.sparse as sp

U32 = 2.0 ** -24            # unit roundoff of fp32


def gamma(m):
    """gamma_m = m u / (1 - m u): fp32 summation of m terms in any order errs by at most gamma_m * sum |terms| (Higham, 3.1)."""
    m = np.asarray(m, dtype=np.float64)
    return m * U32 / (1.0 - m * U32)


def spmm_reference(C, B, s=None, t=None):
    """(ref, bound) for out = C B - s t^T computed in fp32: float64 numpy on the fp32-rounded operands, and
    gamma_(m_r + 3) * (sum_p |v_p B[idx_p, j]| + |s_r t_j|) per element with m_r the stored count of row r; the + 3 covers the
    rounding of the value to fp32, the correction product and the subtraction.  C: scipy CSR, B: fp32 [n_inner, n]."""
    C64 = sp.csr_matrix((C.data.astype(np.float32).astype(np.float64), C.indices, C.indptr), shape=C.shape)
    B64 = B.astype(np.float32).astype(np.float64)
    ref = C64 @ B64
    mag = abs(C64) @ np.abs(B64)
    if t is not None:
        s32 = np.ones(C.shape[0]) if s is None else np.asarray(s).astype(np.float32).astype(np.float64)
        corr = s32[:, None] * t.astype(np.float32).astype(np.float64)[None, :]
        ref = ref - corr
        mag = mag + np.abs(corr)
    m = np.diff(C.indptr)
    return ref, gamma(m + 3)[:, None] * mag


def slots(indptr, S):
    """The workspace slot of every segment of every row longer than S, restated from csrc/sparse_pca.hip: positions are cut into
    windows of S with the slots 2w and 2w + 1; a long row [b, e) touches the windows w0 .. w1; its segment i takes slot
    2 (w0 + 1 + i) while i < w1 - w0 and slot 2 w0 + 1 after that.  Returns [(row, segment, slot)]."""
    out = []
    for r in range(len(indptr) - 1):
        b, e = int(indptr[r]), int(indptr[r + 1])
        if e - b <= S:
            continue
        w0, w1 = b // S, (e - 1) // S
        for i in range(-(-(e - b) // S)):
            out.append((r, i, 2 * (w0 + 1 + i) if i < w1 - w0 else 2 * w0 + 1))
    return out


def long_rows(S, seed=0, dtype=np.float64):
    """CSR [6, 2 S + 3] with rows of 5, S, S + 1, 0, 2 S + 3 (three segments, the last ragged) and 7 stored entries."""
    rng = np.random.default_rng([seed, S])
    d = 2 * S + 3
    counts = [5, S, S + 1, 0, d, 7]
    indices = np.concatenate([np.sort(rng.choice(d, c, replace=False)) for c in counts]).astype(np.int32)
    indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    data = rng.standard_normal(len(indices)).astype(dtype)
    return sp.csr_matrix((data, indices, indptr), shape=(len(counts), d))


def block_cells(N, d, rank, seed, dtype=np.float32):
    """(csr, dense): sparse cells with a separated spectrum.  `rank` disjoint blocks (a random partition of the rows x a random
    partition of the columns), block i = 50 * 0.8^i * sqrt(N) / 10 * u v^T with positive unit vectors u, v; 0.05 * Poisson(1) added
    at 3 % of all positions; rounded to fp32.  Row 0 is empty, row 1 fully stored (column 0 as an explicit zero), column 0 empty
    otherwise: 5-8 % stored for rank 20-32."""
    rng = np.random.default_rng([seed, N, d, rank])
    X = np.zeros((N, d))
    rows = np.array_split(rng.permutation(N), rank)
    cols = np.array_split(rng.permutation(d), rank)
    for i in range(rank):
        u, v = rng.uniform(0.5, 1.5, len(rows[i])), rng.uniform(0.5, 1.5, len(cols[i]))
        u, v = u / np.linalg.norm(u), v / np.linalg.norm(v)
        X[np.ix_(rows[i], cols[i])] = 50.0 * 0.8 ** i * np.sqrt(N) / 10 * np.outer(u, v)
    noise = rng.random((N, d)) < 0.03
    X[noise] += 0.05 * rng.poisson(1.0, int(noise.sum()))
    X[0] = 0.0
    X[1] = 0.05 * (1 + rng.poisson(1.0, d))
    X[:, 0] = 0.0
    X = X.astype(np.float32).astype(np.float64)
    stored = X != 0
    stored[1] = True
    r, c = np.nonzero(stored)
    A = sp.csr_matrix((X[r, c].astype(dtype), (r, c)), shape=(N, d))
    assert A.nnz == stored.sum()
    return A, X.astype(dtype)

"""Products of a sparse cells x features matrix with dense fp32 matrices on the MI355X: what randomized PCA (jamie_amd/pca.py) and
the inference of a PCA-fitted modality (jamie_amd/jamie.py) ask of the centred cells Xc = X - 1 mean^T, without Xc or any other
[N, d] buffer on the host or the device:

    Xc Q   = X Q   - 1 (mean^T Q)              [N, l]      CSR arrays,  t = weighted_colsum(Q, mean)
    Xc^T Y = X^T Y - mean (1^T Y)              [d, l]      CSC arrays (the CSR form of X^T), s = mean, t = weighted_colsum(Y)
    Xc V^T = X V^T - 1 (mean^T V^T)            [N, k]      CSR arrays,  t = weighted_colsum(V^T, mean)

    DeviceCSR(indptr, indices, data, n_inner, device)     the arrays of a compressed matrix on the GPU
    DeviceCSR.product(B, s=None, t=None)                  rows x B - s t^T  (jamie_csr_spmm)
    weighted_colsum(B, w=None)                            sum_r w[r] B[r, :] in fp64, rounded once (jamie_weighted_colsum)

The kernels are in csrc/sparse_pca.hip (include/jamie_hip.h, "Sparse PCA products").  A row's stored entries are added in stored
order in fp32; a row of more than SEGMENT entries is cut into segments of SEGMENT counted from its own start, one fp32 partial each,
added in ascending order: the result is bit-identical from run to run and a row gives the same bits alone, in a chunk or in the
whole matrix.
"""
import numpy as np
import torch

from . import _native as nv

SEGMENT = 2048          # stored entries per segment of a long row (csrc/sparse_pca.hip: SPMM_SEG)
COLSUM_ROWS = nv.COLSUM_ROWS


def workspace(indptr, n):
    """Bytes of workspace of a product with n output columns, restated from the layout: positions are cut into windows of SEGMENT,
    two partial slots of n floats per window; nothing when no row can be longer than SEGMENT.  Needs no GPU."""
    cp = np.asarray(indptr, dtype=np.int64)
    if n < 1 or len(cp) < 2 or (np.diff(cp) < 0).any() or cp[0] < 0:
        return 0
    nnz = int(cp[-1])
    return 8 * int(n) * (-(-nnz // SEGMENT)) if nnz > SEGMENT else 0


def weighted_colsum(B, w=None):
    """fp32 [n] device tensor: sum_r w[r] B[r, :] (w fp64 [rows] or None = ones) for the fp32 device matrix B [rows, n]."""
    rows, n = B.shape
    t = torch.empty(n, dtype=torch.float32, device=B.device)
    ws = torch.empty(nv.weighted_colsum_workspace(rows, n), dtype=torch.uint8, device=B.device)
    nv.weighted_colsum(B, t, ws, w=w)
    return t


class DeviceCSR:
    """The arrays of a compressed sparse matrix [n_rows, n_inner] on the GPU: int64 pointers, int32 indices, fp32 / fp64 values as
    they are (numpy arrays of a canonical scipy matrix: `sparse_input.canonical_csr`, or its `.tocsc()` for the transposed form)."""

    def __init__(self, indptr, indices, data, n_inner, device='cuda'):
        dev = torch.device(device)
        self.n_rows, self.n_inner = len(indptr) - 1, int(n_inner)
        self.host_ptr = np.ascontiguousarray(indptr, dtype=np.int64)
        self.indptr = torch.from_numpy(self.host_ptr).to(dev)
        self.indices = torch.from_numpy(np.ascontiguousarray(indices, dtype=np.int32)).to(dev)
        self.data = torch.from_numpy(np.ascontiguousarray(data)).to(dev)
        self._ws = None

    def product(self, B, s=None, t=None, out=None):
        """fp32 [n_rows, n]: rows x B (B fp32 [n_inner, n] on the device) minus s t^T when `t` is given (s fp64 [n_rows] or None = 1)."""
        n = B.shape[1]
        out = torch.empty(self.n_rows, n, dtype=torch.float32, device=B.device) if out is None else out
        if self.n_rows == 0:
            return out
        need = nv.spmm_workspace(self.host_ptr, n)
        if need and (self._ws is None or self._ws.numel() < need):
            self._ws = torch.empty(need, dtype=torch.uint8, device=B.device)
        nv.csr_spmm(self.indptr, self.indices, self.data, self.n_inner, B, out, self._ws if need else None, n=n, s=s, t=t,
                    n_rows=self.n_rows)
        return out

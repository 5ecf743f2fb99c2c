"""Sparse PCA on the device (csrc/sparse_pca.hip, jamie_amd/sparse_pca.py, jamie_amd/pca.py, the facade): `jamie_csr_spmm` and
`jamie_weighted_colsum` against float64 numpy, `DevicePCA` on a scipy sparse matrix against sklearn's full float64 PCA of its dense
form and against the dense device fit, and `JAMIE(pca_dim=..., preprocess='device')` on sparse cells with `toarray()` forbidden.

The product's bound is derived, not measured: fp32 summation of m terms in any order errs by at most gamma_m sum |terms|,
gamma_m = m u / (1 - m u), u = 2^-24, so |out - ref| <= gamma_(m_r + 3) (sum_p |v_p B[idx_p, j]| + |s_r t_j|) with m_r the stored
count of the row (+ 3: the value's rounding to fp32, the correction product, the subtraction); ref is float64 numpy on the
fp32-rounded operands.  PCA tolerances are those of tests/test_hip_pca.py; inference against the dense call: rtol 1e-4,
atol 1e-5 * max, the project's inference tolerance."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_pca_util as pu  # noqa: E402
import sparse_util as su  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -77.0


@pytest.fixture(scope='module')
def jsp():
    from jamie_amd import sparse_input
    return sparse_input


@pytest.fixture(scope='module')
def spp():
    from jamie_amd import sparse_pca
    return sparse_pca


@pytest.fixture(scope='module')
def nv():
    from jamie_amd import _native
    _native.require_gpu()
    return _native


def _spmm(nv, C, B, s=None, t=None, pad_b=0, pad_out=0):
    """jamie_csr_spmm on the canonical CSR matrix C and the fp32 matrix B [n_inner, n], with leading dimensions n + pad; the
    padding of `out`, pre-filled with a sentinel, must come back untouched.  Returns the fp32 [n_rows, n] device result."""
    n_rows, n_inner = C.shape
    n = B.shape[1]
    Bd = torch.full((n_inner, n + pad_b), SENTINEL, dtype=torch.float32, device='cuda')
    Bd[:, :n] = torch.from_numpy(B)
    out = torch.full((n_rows + 2, n + pad_out), SENTINEL, dtype=torch.float32, device='cuda')
    ws = torch.empty(nv.spmm_workspace(C.indptr, n), dtype=torch.uint8, device='cuda')
    nv.csr_spmm(torch.from_numpy(C.indptr.astype(np.int64)).cuda(), torch.from_numpy(C.indices.astype(np.int32)).cuda(),
                torch.from_numpy(C.data).cuda(), n_inner, Bd[:, :n], out[:n_rows, :n], ws if ws.numel() else None, n=n,
                s=None if s is None else torch.from_numpy(s).cuda(), t=None if t is None else torch.from_numpy(t).cuda())
    assert bool((out[:n_rows, n:] == SENTINEL).all()) and bool((out[n_rows:] == SENTINEL).all())
    return out[:n_rows, :n]


def _within_bound(got, C, B, s, t, what):
    ref, bound = pu.spmm_reference(C, B, s, t)
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
    pos = bound > 0
    print(f'{what}: max |out - ref| {err.max():.3e}, largest share of the bound {np.max(err[pos] / bound[pos]) if pos.any() else 0.0:.4f}')
    assert (err <= bound).all(), (what, float(err.max()), np.unravel_index(np.argmax(err - bound), err.shape))


# ---- 1. the product against float64 ----
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('n', [1, 63, 64, 65, 522])
def test_csr_spmm_vs_float64(jsp, nv, n, dtype):
    """sparse_counts(257, 300): first and last rows empty but for the two fully stored columns, a row stored in all but the empty column, explicit zeros,
    an offset column of 1e4; 257 rows are no multiple of the four a workgroup takes; n = 522 is nine accumulators per lane, the
    last with ten live lanes."""
    A, _ = su.sparse_counts(257, 300, seed=2, dtype=dtype)
    C = jsp.canonical_csr(A)
    assert C.dtype == dtype and C.indptr[1] - C.indptr[0] == 2 and (np.diff(C.indptr) == 299).any() and (C.data == 0).any()
    rng = np.random.default_rng(n)
    B = rng.standard_normal((300, n)).astype(np.float32)
    s, t = rng.uniform(0.0, 3.0, 257), rng.standard_normal(n).astype(np.float32)
    for pad_b, pad_out in ((0, 0), (3, 5)):
        for sv, tv in ((None, None), (None, t), (s, t)):
            got = _spmm(nv, C, B, sv, tv, pad_b, pad_out)
            _within_bound(got, C, B, sv, tv, f'n = {n}, {np.dtype(dtype).name}, ld + ({pad_b}, {pad_out}), s {sv is not None}, t {tv is not None}')


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_csr_spmm_long_rows(jsp, spp, nv, dtype):
    """Rows of more than SEGMENT entries go through per-segment partials: the CSC side of a [2 S + 3, 3] matrix whose column 0 is
    fully stored (one row of the transposed form with three segments, the last ragged), and rows of exactly S, S + 1 and 2 S + 3
    entries between short and empty ones."""
    S = spp.SEGMENT
    rng = np.random.default_rng(7)
    M = rng.standard_normal((2 * S + 3, 3)) * (rng.random((2 * S + 3, 3)) < 0.1)
    M[:, 0] = rng.standard_normal(2 * S + 3) + 2.0
    csc = jsp.canonical_csr(sp.csr_matrix(M.astype(dtype))).tocsc()
    T = sp.csr_matrix((csc.data, csc.indices.astype(np.int32), csc.indptr.astype(np.int64)), shape=(3, 2 * S + 3))   # CSR of M^T
    assert T.indptr[1] - T.indptr[0] == 2 * S + 3 and len(pu.slots(T.indptr, S)) == 3
    L = pu.long_rows(S, dtype=dtype)
    assert np.diff(L.indptr).tolist() == [5, S, S + 1, 0, 2 * S + 3, 7] and len(pu.slots(L.indptr, S)) == 2 + 3
    for name, C in (('transposed [2 S + 3, 3]', T), ('rows of S, S + 1, 2 S + 3', L)):
        for n in (1, 65):
            B = rng.standard_normal((C.shape[1], n)).astype(np.float32)
            s, t = rng.uniform(0.0, 3.0, C.shape[0]), rng.standard_normal(n).astype(np.float32)
            for sv, tv in ((None, None), (s, t)):
                _within_bound(_spmm(nv, C, B, sv, tv, 2, 1), C, B, sv, tv, f'{name}, n = {n}, {np.dtype(dtype).name}, t {tv is not None}')


def test_csr_spmm_is_exact_on_integers(spp, nv):
    """Small integer values and B (every partial sum below 2^24): equal to int64 numpy, long rows and corrections included."""
    S = spp.SEGMENT
    rng = np.random.default_rng(3)
    L = pu.long_rows(S)
    L.data = rng.integers(-3, 4, L.nnz).astype(np.float64)
    for n in (1, 65, 522):
        B = rng.integers(-4, 5, (L.shape[1], n))
        s, t = rng.integers(0, 6, L.shape[0]), rng.integers(-9, 10, n)
        want = (L.astype(np.int64) @ B.astype(np.int64)) - s[:, None] * t[None, :]
        assert abs(L).astype(np.int64).dot(np.abs(B)).max() < 2 ** 24
        got = _spmm(nv, L, B.astype(np.float32), s.astype(np.float64), t.astype(np.float32)).cpu().numpy()
        assert np.array_equal(got.astype(np.int64), want) and np.array_equal(got, want.astype(np.float32)), n


def test_csr_spmm_is_deterministic_and_row_local(spp, nv):
    """Two calls give the same bits, and rows [a, b) sliced out as a CSR matrix of their own (rebased pointers: the segments of the
    three-segment row then lie elsewhere relative to the workspace windows) give the bits of rows [a, b) of the whole call."""
    S = spp.SEGMENT
    L = pu.long_rows(S, seed=1)
    rng = np.random.default_rng(5)
    for n in (26, 65):
        B = rng.standard_normal((L.shape[1], n)).astype(np.float32)
        s, t = rng.uniform(0.0, 3.0, L.shape[0]), rng.standard_normal(n).astype(np.float32)
        whole = _spmm(nv, L, B, s, t)
        assert torch.equal(whole, _spmm(nv, L, B, s, t, 3, 1))
        assert np.array_equal(whole[3].cpu().numpy(), -(np.float32(s[3]) * t))          # an empty row is the correction alone
        for a, b in ((2, 6), (4, 5), (0, 3), (3, 4)):
            part = sp.csr_matrix(L[a:b])
            assert part.indptr[0] == 0
            assert torch.equal(_spmm(nv, part, B, s[a:b].copy(), t), whole[a:b]), (n, a, b)


# ---- 2. the correction's row vector ----
@pytest.mark.parametrize('rows', [1, 255, 5000])
def test_weighted_colsum_vs_float64(spp, nv, rows):
    rng = np.random.default_rng(rows)
    for n in (1, 65, 522):
        B = rng.standard_normal((rows, n)).astype(np.float32)
        w = rng.uniform(0.0, 5.0, rows)
        Bd, wd = torch.from_numpy(B).cuda(), torch.from_numpy(w).cuda()
        for weights, ref in ((wd, w @ B.astype(np.float64)), (None, B.astype(np.float64).sum(0))):
            got = spp.weighted_colsum(Bd, weights)
            assert got.dtype == torch.float32 and got.shape == (n,)
            rel = np.abs(got.cpu().numpy() - ref) / np.abs(ref)
            print(f'rows = {rows}, n = {n}, weights {weights is not None}: max relative error {rel.max():.3e} (2^-23 = {2.0 ** -23:.3e})')
            np.testing.assert_allclose(got.cpu().numpy().astype(np.float64), ref, rtol=2.0 ** -23, atol=0)
            assert torch.equal(got, spp.weighted_colsum(Bd, weights))


# ---- 3. DevicePCA on a sparse matrix ----
SHAPES = [(3000, 400, 16), (600, 2000, 12), (2500, 384, 24)]


@pytest.fixture(scope='module')
def pca_fits(nv):
    """Per shape: the cells (CSR and dense), the sparse device fit with its scores, sklearn's full float64 PCA of the dense form.
    Computed once and shared."""
    from sklearn.decomposition import PCA
    from jamie_amd.pca import DevicePCA
    cache = {}

    def get(shape):
        if shape not in cache:
            N, d, k = shape
            A, X = pu.block_cells(N, d, k + 8, seed=N + d)
            full = PCA(n_components=k, svd_solver='full').fit(X.astype(np.float64))
            dp = DevicePCA(k, random_state=0)
            scores = dp.fit_transform_device(A).cpu().numpy()
            cache[shape] = {'A': A, 'X': X, 'full': full, 'dp': dp, 'scores': scores}
        return cache[shape]
    return get


@pytest.mark.parametrize('shape', SHAPES)
def test_sparse_device_pca_matches_sklearn(pca_fits, shape):
    N, d, k = shape
    c = pca_fits(shape)
    A, X, full, dp, scores = c['A'], c['X'].astype(np.float64), c['full'], c['dp'], c['scores']
    assert 0.04 < A.nnz / (N * d) < 0.09 and A.indptr[1] == 0 and A.indptr[2] == d
    assert dp.components_.shape == (k, d) and scores.shape == (N, k) and dp.n_components_ == k
    top = full.explained_variance_[0]
    print(f'{shape}: max relative explained-variance error {np.max(np.abs(dp.explained_variance_ / full.explained_variance_ - 1)):.3e}')
    np.testing.assert_allclose(dp.explained_variance_, full.explained_variance_, rtol=1e-3, atol=1e-7 * top)
    np.testing.assert_allclose(dp.explained_variance_ratio_, full.explained_variance_ratio_, rtol=1e-3, atol=1e-7)
    np.testing.assert_allclose(dp.singular_values_ ** 2, full.singular_values_ ** 2, rtol=1e-3, atol=1e-7 * full.singular_values_[0] ** 2)
    np.testing.assert_allclose(dp.mean_, full.mean_, **su.MEAN_TOL)
    sep = full.explained_variance_ > 1e-5 * top
    cos = np.sum(dp.components_ * full.components_, axis=1)
    print(f'{shape}: smallest signed component cosine {cos[sep].min():.8f} over {sep.sum()} components')
    assert cos[sep].min() > 0.999, (cos[sep].min(), sep.sum())
    np.testing.assert_allclose(dp.components_ @ dp.components_.T, np.eye(k), atol=1e-5)
    np.testing.assert_allclose(scores[:, sep], full.transform(X)[:, sep], rtol=2e-3, atol=2e-3 * np.abs(scores).max())


@pytest.mark.parametrize('shape', SHAPES)
def test_sparse_fit_agrees_with_the_dense_fit(pca_fits, shape):
    """Same cells, same random_state (so the same Omega): the implicit centring against fl(x - mean) and the MFMA GEMM."""
    from jamie_amd.pca import DevicePCA
    N, d, k = shape
    c = pca_fits(shape)
    dd = DevicePCA(k, random_state=0)
    dense_scores = dd.fit_transform_device(torch.from_numpy(c['X'])).cpu().numpy()
    dp = c['dp']
    sep = dd.explained_variance_ > 1e-5 * dd.explained_variance_[0]
    cos = np.sum(dp.components_ * dd.components_, axis=1)
    print(f'{shape}: sparse against dense fit: max relative explained-variance difference '
          f'{np.max(np.abs(dp.explained_variance_ / dd.explained_variance_ - 1)):.3e}, smallest cosine {cos[sep].min():.8f}, '
          f'max |score difference| / max |score| {np.abs(c["scores"] - dense_scores)[:, sep].max() / np.abs(dense_scores).max():.3e}')
    np.testing.assert_allclose(dp.explained_variance_, dd.explained_variance_, rtol=1e-3)
    assert cos[sep].min() > 0.999


def test_sparse_fit_draws_like_the_dense_fit(pca_fits):
    """One normal(size=(d, k + 10)) draw from numpy's global RandomState, as the dense fit and sklearn."""
    from jamie_amd.pca import DevicePCA
    A = pca_fits(SHAPES[0])['A'][:600, :120]
    np.random.seed(5)
    DevicePCA(12).fit(A)
    after = np.random.rand(3)
    np.random.seed(5)
    np.random.normal(size=(120, 22))
    np.testing.assert_array_equal(after, np.random.rand(3))


@pytest.mark.parametrize('rows', [100, 3000])
def test_sparse_transform_within_the_derived_bound(pca_fits, jsp, rows):
    """`DevicePCA.transform(csr_rows)` against float64 (X - mean_) @ components_^T on the operands the kernel sees (components
    rounded to fp32; the cells are exact in fp32), with the product's bound: s = 1, t = mean_^T components_^T, whose own single
    rounding from fp64 is one more u |t_j| -- inside the + 3, as the correction is one fused multiply-add, not two operations."""
    c = pca_fits(SHAPES[0])
    dp = c['dp']
    A = jsp.canonical_csr(c['A'][:rows])
    got = dp.transform(c['A'][:rows])
    assert got.shape == (rows, 16) and got.dtype == np.float64
    comp = dp.components_.astype(np.float32).astype(np.float64)
    t = dp.mean_ @ comp.T
    ref = (c['X'][:rows].astype(np.float64) - dp.mean_) @ comp.T
    mag = abs(A).astype(np.float64) @ np.abs(comp.T) + np.abs(t)[None, :]
    bound = pu.gamma(np.diff(A.indptr) + 3)[:, None] * mag
    err = np.abs(got - ref)
    print(f'{rows} rows: max |transform - ref| {err.max():.3e}, largest share of the bound {np.max(err / bound):.4f}')
    assert (err <= bound).all()


def test_sparse_pca_of_constant_and_zero_matrices_is_finite(nv):
    from jamie_amd.pca import DevicePCA
    for name, A in (('constant', sp.csr_matrix(np.full((600, 120), 3.25, dtype=np.float32))), ('all-zero', sp.csr_matrix((600, 120), dtype=np.float32))):
        dp = DevicePCA(8, random_state=0)
        scores = dp.fit_transform_device(A).cpu().numpy()
        print(f'{name}: max |score| {np.abs(scores).max():.3e}')
        assert scores.shape == (600, 8) and np.isfinite(scores).all() and np.abs(scores).max() < 1e-4
        assert np.isfinite(dp.components_).all() and np.isfinite(dp.explained_variance_).all()
        np.testing.assert_allclose(dp.mean_, 3.25 if name == 'constant' else 0.0)


def test_sparse_fit_stays_below_half_a_dense_copy(nv):
    """N = 20 000, d = 4000, 5 % stored, k = 16: the dense route holds Xc, N d 4 bytes, alone; the sparse route's CSR and CSC arrays
    add up to about a quarter of that."""
    from jamie_amd.pca import DevicePCA
    N, d = 20000, 4000
    A = sp.random(N, d, 0.05, format='csr', dtype=np.float32, random_state=4)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    scores = DevicePCA(16, random_state=0).fit_transform_device(A)
    torch.cuda.synchronize()
    used = torch.cuda.max_memory_allocated() - before
    print(f'peak device memory of the sparse fit: {used / 2 ** 20:.1f} MiB; a dense fp32 copy: {N * d * 4 / 2 ** 20:.1f} MiB')
    assert scores.shape == (N, 16) and bool(torch.isfinite(scores).all())
    assert used < N * d * 4 / 2


def test_dense_fit_is_the_dense_operator(nv):
    """Dense input takes the dense operator, which is the fit as it was before the operators existed: restated here from the
    module's own products, it gives the same bits."""
    from jamie_amd import pca
    X = torch.from_numpy(pu.block_cells(1500, 200, 20, seed=9)[1]).cuda()
    k, ell, n_iter = 12, 22, 7
    dp = pca.DevicePCA(k, random_state=0)
    scores = dp.fit_transform_device(X)
    Xc, mean, sd = pca._center(X)
    Q = torch.from_numpy(np.random.RandomState(0).normal(size=(200, ell)).astype(np.float32)).cuda()
    for _ in range(n_iter):
        Q = pca._whiten(pca.mm_nn(Xc, Q))
        Q = pca._orth_small(pca.mm_tn(Xc, Q))
    Q = pca._whiten(pca.mm_nn(Xc, Q), rounds=2)
    B = pca.mm_tn(Q, Xc).double().cpu().numpy()
    _, S, Vt = np.linalg.svd(B, full_matrices=False)
    Vt, S = Vt[:k], S[:k]
    Vt = Vt * np.sign(Vt[np.arange(k), np.argmax(np.abs(Vt), axis=1)])[:, None]
    assert np.array_equal(dp.components_, Vt) and np.array_equal(dp.singular_values_, S) and np.array_equal(dp.mean_, mean.cpu().numpy())
    assert torch.equal(scores, pca.mm_nt(Xc, torch.from_numpy(np.ascontiguousarray(Vt.astype(np.float32))).cuda()))


# ---- 4. the facade ----
N_FIT, DIMS, PCA_DIM = 700, (72, 40), [16, 16]
INFER_TOL = 1e-4, 1e-5


class Forbidden(AssertionError):
    pass


def _no_dense(A):
    """A copy of the sparse matrix whose `toarray` / `todense` raise."""
    A = A.copy()

    def refuse(*a, **kw):
        raise Forbidden('a dense copy of the sparse input was asked for')
    A.toarray = A.todense = refuse
    return A


@pytest.fixture(scope='module')
def cells():
    pairs = [pu.block_cells(N_FIT, d, 24, seed=11 + i, dtype=np.float64) for i, d in enumerate(DIMS)]
    new = [pu.block_cells(600, d, 24, seed=31 + i, dtype=np.float64) for i, d in enumerate(DIMS)]
    return {'csr': [p[0] for p in pairs], 'dense': [p[1] for p in pairs], 'new_csr': [p[0] for p in new], 'new_dense': [p[1] for p in new]}


@pytest.fixture(scope='module')
def fits(cells, nv):
    """JAMIE models fitted as the `fits` fixture of tests/test_hip_sparse_input.py fits them, with pca_dim = [16, 16], by
    (preprocess, input kind); numpy's global RNG (the PCA's Omega) is seeded alike before each.  Fitted once and shared."""
    from jamie_amd import JAMIE
    cache = {}

    def fit(preprocess, kind):
        key = (preprocess, kind)
        if key not in cache:
            data = {'dense': lambda: [x.copy() for x in cells['dense']], 'csr': lambda: [_no_dense(a) for a in cells['csr']],
                    'ann': lambda: [su.Ann(_no_dense(a)) for a in cells['csr']],
                    'mixed': lambda: [_no_dense(cells['csr'][0]), cells['dense'][1].copy()]}[kind]()
            np.random.seed(1)
            with contextlib.redirect_stdout(io.StringIO()):
                jm = JAMIE(output_dim=8, batch_size=64, epoch_DNN=6, min_epochs=3, pca_dim=list(PCA_DIM), use_f_tilde=False,
                           log_DNN=10 ** 9, sampler='device', preprocess=preprocess)
                jm.fit_transform(dataset=data)
            cache[key] = (jm, data)
        return cache[key]
    return fit


def _pre(jm, i):
    return jm.model.preprocessing[i].__self__


def test_no_dense_guard_raises(cells):
    with pytest.raises(Forbidden):
        _no_dense(cells['csr'][0]).toarray()
    with pytest.raises(Forbidden):
        _no_dense(cells['csr'][0]).todense()


@pytest.mark.parametrize('kind', ['csr', 'ann', 'mixed'])
def test_fit_sparse_cells_through_device_pca(fits, cells, kind):
    """Fails on the code before the sparse operator, which called `toarray()` on a sparse modality with a `pca_dim`.  The global
    mean m of the scores is zero up to rounding (the scores are centred), so "within 1e-6 relative" is taken relative to the scale
    of the quantity it shifts, the global standard deviation s; s itself is held to 1e-6 relative."""
    from jamie_amd.pca import DevicePCA
    jd, _ = fits('device', 'dense')
    js, given = fits('device', kind)
    assert js.row == [N_FIT, N_FIT] and js.col == list(PCA_DIM)
    for i in range(2):
        a, b = _pre(js, i), _pre(jd, i)
        assert a.axis is None and isinstance(a.pca, DevicePCA) and a.pca.components_.shape == (16, DIMS[i])
        assert abs(float(a.mean) - float(b.mean)) <= 1e-6 * max(abs(float(b.mean)), float(b.std)) and abs(float(a.std) / float(b.std) - 1) <= 1e-6
        print(f'{kind}, modality {i}: m {float(a.mean)!r} / {float(b.mean)!r}, s {float(a.std)!r} / {float(b.std)!r}, max relative '
              f'explained-variance difference {np.max(np.abs(a.pca.explained_variance_ / b.pca.explained_variance_ - 1)):.3e}, '
              f'max |cell difference| {np.abs(js.dataset[i] - jd.dataset[i]).max():.3e} of {np.abs(jd.dataset[i]).max():.3e}')
        np.testing.assert_allclose(a.pca.explained_variance_, b.pca.explained_variance_, rtol=1e-3)
        assert isinstance(js.dataset[i], np.ndarray) and js.dataset[i].dtype == np.float32 and js.dataset[i].shape == (N_FIT, 16)
        np.testing.assert_allclose(js.dataset[i], jd.dataset[i], rtol=2e-3, atol=2e-3 * np.abs(jd.dataset[i]).max())
    # the caller's matrices are as they were
    for i, g in enumerate(given):
        g = getattr(g, 'X', g)
        if sp.issparse(g):
            o = cells['csr'][i]
            assert g.format == 'csr' and g.dtype == np.float64 and g.shape == o.shape
            assert np.array_equal(g.data, o.data) and np.array_equal(g.indices, o.indices) and np.array_equal(g.indptr, o.indptr)


def test_inference_on_sparse_cells_through_device_pca(fits, cells):
    """600 new sparse cells, `toarray()` forbidden: three row chunks of 256 (the last ragged) give the bits of the single default
    chunk, and the dense call on the same model is met at the inference tolerance.  Fails on the code before the sparse operator."""
    jm, _ = fits('device', 'csr')
    new = [_no_dense(a) for a in cells['new_csr']]
    assert jm._csr_preclass(0) is None and jm._csr_pca_preclass(0) is not None
    emb = jm.transform(new)
    emb_c = jm.transform(new, chunk=256)
    dense = jm.transform(cells['new_dense'])
    rtol, atol = INFER_TOL
    for i in range(2):
        assert emb[i].shape == (600, 8) and emb[i].dtype == np.float32
        assert np.array_equal(emb[i], emb_c[i])
        assert np.array_equal(jm.transform_one(new[i], i), emb[i]) and np.array_equal(jm.transform_one(new[i], i, chunk=256), emb[i])
        print(f'modality {i}: max |transform(csr) - transform(dense)| {np.abs(emb[i] - dense[i]).max():.3e} of {np.abs(dense[i]).max():.3e}')
        np.testing.assert_allclose(emb[i], dense[i], rtol=rtol, atol=atol * np.abs(dense[i]).max())
        np.testing.assert_allclose(jm.transform_one(new[i], i), jm.transform_one(cells['new_dense'][i], i), rtol=rtol,
                                   atol=atol * np.abs(dense[i]).max())
    imp = jm.modal_predict(new[0], 0)
    want = jm.modal_predict(cells['new_dense'][0], 0)
    assert imp.shape == (600, DIMS[1]) and imp.dtype == want.dtype == np.float64     # back through inverse_transform, as before
    assert np.array_equal(imp, jm.modal_predict(new[0], 0, chunk=256)) and np.array_equal(imp, jm.impute(new[0], 0))
    print(f'max |modal_predict(csr) - modal_predict(dense)| {np.abs(imp - want).max():.3e} of {np.abs(want).max():.3e}')
    np.testing.assert_allclose(imp, want, rtol=rtol, atol=atol * np.abs(want).max())
    # other sparse formats, and a wrong feature count
    assert np.array_equal(jm.transform_one(cells['new_csr'][0].tocsc(), 0), emb[0])
    with pytest.raises(ValueError):
        jm.transform_one(new[1], 0)


def test_inference_on_sparse_cells_after_saving_and_loading(fits, cells, tmp_path):
    from jamie_amd import JAMIE
    jm, _ = fits('device', 'csr')
    new = [_no_dense(a) for a in cells['new_csr']]
    path = str(tmp_path / 'model.pt')
    jm.save_model(path)
    other = JAMIE()
    other.load_model(path)
    assert other._csr_pca_preclass(0) is not None and other._csr_preclass(0) is None
    assert np.array_equal(other.transform_one(new[0], 0, chunk=256), jm.transform_one(new[0], 0, chunk=256))
    assert np.array_equal(other.modal_predict(new[0], 0), jm.modal_predict(new[0], 0))


def test_host_pca_model_still_densifies(fits, cells):
    """preprocess='host' carries an sklearn PCA, which takes dense input: sparse cells are densified and give the dense call's bits."""
    jm, _ = fits('host', 'dense')
    assert jm._csr_preclass(0) is None and jm._csr_pca_preclass(0) is None and _pre(jm, 0).pca is not None
    with pytest.raises(Forbidden):
        jm.transform_one(_no_dense(cells['new_csr'][0]), 0)
    for i in range(2):
        assert np.array_equal(jm.transform_one(cells['new_csr'][i], i), jm.transform_one(cells['new_dense'][i], i))
    assert np.array_equal(jm.modal_predict(cells['new_csr'][0], 0), jm.modal_predict(cells['new_dense'][0], 0))

"""Sparse cell matrices on the device (jamie_amd/sparse_input.py, csrc/sparse_input.hip): the statistics against float64 numpy,
the densify kernel against `jamie_standardise` on the dense form (to the bit), `standardise_csr` against the dense device route,
and the facade's fit / transform / transform_one / modal_predict on CSR input against the same calls on dense input.

Tolerances: statistics rtol 1e-12 / atol 1e-12 (mean) and rtol 1e-10 / atol 1e-12 (sd), cells rtol 2e-6 / atol 1e-6, embeddings after
training rtol 1e-3 / atol 1e-4: what tests/test_hip_step.py holds the dense device preprocessing to.  Inference against the dense
facade call at its default chunk: README's rtol 1e-4 / atol 1e-5 (the eval GEMM may tile differently by row count); at the same
chunk size the results are equal to the bit."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_util as su  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -77.0
EMB_TOL = dict(rtol=1e-3, atol=1e-4)
INFER_TOL = dict(rtol=1e-4, atol=1e-5)


@pytest.fixture(scope='module')
def jsp():
    from jamie_amd import sparse_input
    return sparse_input


@pytest.fixture(scope='module')
def nv():
    from jamie_amd import _native
    return _native


def _device_stats(jsp, A, dtype):
    """jamie_csc_col_stats on the canonical form of A with values of `dtype`: (mean, sd) fp64 device tensors."""
    C = jsp.canonical_csr(A.astype(dtype))
    assert C.dtype == dtype
    return jsp.column_stats(C, 'cuda')


@pytest.fixture(scope='module')
def stats_case(jsp):
    """sparse_counts(2 S + 37, 203): a full column spans three segments with a boundary inside; d is no multiple of 4 or 64."""
    N, d = 2 * jsp.SEGMENT + 37, 203
    A, X = su.sparse_counts(N, d)
    mean, sd = _device_stats(jsp, A, np.float64)
    return {'A': A, 'X': X, 'N': N, 'd': d, 'ref': (X.mean(0), X.std(0)), 'mean': mean, 'sd': sd}


# ---- 1. statistics ----
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_csc_col_stats_vs_float64_numpy(jsp, stats_case, dtype):
    c = stats_case
    mean, sd = _device_stats(jsp, c['A'], dtype)
    m, s = mean.cpu().numpy(), sd.cpu().numpy()
    ref_mean, ref_sd = c['ref']
    pos = ref_sd > 0
    print(f"{np.dtype(dtype).name} values, {c['N']} x {c['d']}: max |mean - ref| {np.abs(m - ref_mean).max():.3e}, max relative sd error "
          f"{np.max(np.abs(s - ref_sd)[pos] / ref_sd[pos]):.3e}; empty column ({m[su.EMPTY_COL]!r}, {s[su.EMPTY_COL]!r}), constant column "
          f"({m[su.CONST_COL]!r}, {s[su.CONST_COL]!r})")
    assert m.dtype == np.float64 and s.dtype == np.float64 and m.shape == s.shape == (c['d'],)
    np.testing.assert_allclose(m, ref_mean, **su.MEAN_TOL)
    np.testing.assert_allclose(s, ref_sd, **su.SD_TOL)
    assert s[su.EMPTY_COL] == 0.0 and m[su.EMPTY_COL] == 0.0
    assert s[su.CONST_COL] == 0.0 and m[su.CONST_COL] == su.CONST
    mean2, sd2 = _device_stats(jsp, c['A'], dtype)
    assert torch.equal(mean, mean2) and torch.equal(sd, sd2)
    # the restatement of the method in numpy (tests/test_host_sparse_input.py) describes this kernel
    csc = jsp.canonical_csr(c['A']).tocsc()
    rm, rs = su.restated_stats(csc.data, csc.indptr, c['N'], jsp.SEGMENT)
    assert np.array_equal(m, rm)                       # the same sums in the same order, divided by N
    np.testing.assert_allclose(s, rs, **su.SD_TOL)


# ---- 2. densify, to the bit ----
def _dense_standardise(nv, X, mean, sd):
    N, d = X.shape
    out = torch.empty(N, d, dtype=torch.float32, device='cuda')
    nv._call('jamie_standardise', nv.ptr(X), int(X.dtype == torch.float64), N, d, d, nv.ptr(mean), nv.ptr(sd), nv.ptr(out), nv._stream())
    return out


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('d', [1, 3, 203, 8200])
def test_csr_standardise_equals_dense_standardise(jsp, nv, stats_case, d, dtype):
    """N = 517 is no multiple of the rows a workgroup walks; d = 8200 spans three LDS windows, the last of 8 columns; ld_out = d + 5
    leaves most output rows off a 16-byte boundary."""
    N = 517
    assert d <= jsp.WINDOW or d > 2 * jsp.WINDOW
    A, X = su.sparse_counts(N, d, seed=5, dtype=dtype)
    C = jsp.canonical_csr(A)
    assert C.dtype == dtype and (C.data == 0).any() and np.array_equal(C.toarray(), X)
    assert C.indptr[1] == 0 or d >= 8                                  # (an empty first row where no column is fully stored)
    Xd = torch.from_numpy(X).cuda()
    indptr, indices = torch.from_numpy(C.indptr).cuda(), torch.from_numpy(C.indices).cuda()
    vals = torch.from_numpy(C.data).cuda()
    ws = torch.empty(nv.sparse_workspace(None, d, 1), dtype=torch.uint8, device='cuda')
    # the statistics of the kernel under test 1 (for d = 203: of the larger matrix of that test), and a hand-made pair
    pairs = [(stats_case['mean'], stats_case['sd']) if d == 203 else _device_stats(jsp, A, dtype)]
    rng = np.random.default_rng(d)
    hm, hs = rng.standard_normal(d), rng.uniform(0.5, 2.0, d)
    hs[[0, d // 2]] = 0.0
    hm[[d // 3, d - 1]] = np.nan
    pairs.append((torch.from_numpy(hm).cuda(), torch.from_numpy(hs).cuda()))
    for mean, sd in pairs:
        want = _dense_standardise(nv, Xd, mean, sd)
        out = torch.full((N + 3, d + 5), SENTINEL, dtype=torch.float32, device='cuda')
        nv.csr_standardise(indptr, indices, vals, d, mean, sd, out, ws, n_rows=N)
        diff = int((out[:N, :d] != want).sum())
        print(f'd = {d}, {np.dtype(dtype).name}: {diff} of {N * d} elements differ from jamie_standardise')
        assert torch.equal(out[:N, :d], want)
        assert bool((out[:N, d:] == SENTINEL).all()) and bool((out[N:] == SENTINEL).all())
        # a row chunk with rebased pointers, as the facade streams them
        lo, hi = 100, 300
        S = C[lo:hi]
        part = torch.full((hi - lo, d), SENTINEL, dtype=torch.float32, device='cuda')
        nv.csr_standardise(torch.from_numpy(S.indptr.astype(np.int64)).cuda(), torch.from_numpy(S.indices.astype(np.int32)).cuda(),
                           torch.from_numpy(S.data).cuda(), d, mean, sd, part, ws)
        assert torch.equal(part, want[lo:hi])


# ---- 3. standardise_csr against the dense device route ----
def test_standardise_csr_equals_standardise_columns(jsp, nv, stats_case):
    c = stats_case
    for dtype in (np.float32, np.float64):
        out, mean, sd = jsp.standardise_csr(c['A'].astype(dtype))
        want, wmean, wsd = nv.standardise_columns(torch.from_numpy(c['X'].astype(dtype)).cuda())
        assert out.dtype == torch.float32 and out.shape == (c['N'], c['d']) and out.is_contiguous()
        np.testing.assert_allclose(mean.cpu().numpy(), wmean.cpu().numpy(), **su.MEAN_TOL)
        np.testing.assert_allclose(sd.cpu().numpy(), wsd.cpu().numpy(), **su.SD_TOL)
        err = float((out - want).abs().max())
        print(f'{np.dtype(dtype).name}: max |standardise_csr - standardise_columns| {err:.3e}')
        np.testing.assert_allclose(out.cpu().numpy(), want.cpu().numpy(), **su.CELL_TOL)
        assert bool((out[:, su.EMPTY_COL] == 0).all()) and bool((out[:, su.CONST_COL] == 0).all())
    # integer counts go up as fp64
    Ai = c['A'].copy()
    Ai.data = np.floor(Ai.data)
    out_i, mean_i, _ = jsp.standardise_csr(Ai.astype(np.int64))
    out_f, mean_f, _ = jsp.standardise_csr(Ai)
    assert torch.equal(out_i, out_f) and torch.equal(mean_i, mean_f)
    # a NaN stored in one column: that whole column is 0 (its statistics are NaN), everything stays finite
    B = c['A'].copy().astype(np.float64)
    col = 7
    rows = B[:, col].nonzero()[0]
    assert len(rows) > 3
    B[rows[1], col] = np.nan
    out, mean, sd = jsp.standardise_csr(B)
    assert bool(torch.isnan(mean[col])) and bool(torch.isnan(sd[col])) and int(torch.isnan(mean).sum()) == 1
    assert bool(torch.isfinite(out).all()) and bool((out[:, col] == 0).all())
    keep = [k for k in range(c['d']) if k != col]
    clean, _, _ = jsp.standardise_csr(c['A'])
    assert torch.equal(out[:, keep], clean[:, keep])


# ---- 4. / 5. the facade ----
N_FIT, DIMS = 700, (72, 40)


@pytest.fixture(scope='module')
def cells():
    pairs = [su.sparse_counts(N_FIT, d, seed=11 + i) for i, d in enumerate(DIMS)]
    return {'csr': [p[0] for p in pairs], 'dense': [p[1] for p in pairs]}


@pytest.fixture(scope='module')
def fits(cells):
    """JAMIE models fitted as tests/test_hip_step.py::test_facade_device_preprocessing_equals_host fits them, by (preprocess, input
    kind); fitted once and shared."""
    from jamie_amd import JAMIE
    cache = {}

    def fit(preprocess, kind, pca_dim=None):
        key = (preprocess, kind, None if pca_dim is None else tuple(pca_dim))
        if key not in cache:
            data = {'dense': [x.copy() for x in cells['dense']], 'csr': [a.copy() for a in cells['csr']],
                    'ann': [su.Ann(a.copy()) for a in cells['csr']], 'mixed': [cells['csr'][0].copy(), cells['dense'][1].copy()],
                    'int_dense': [np.floor(x) for x in cells['dense']]}[kind]
            with contextlib.redirect_stdout(io.StringIO()):
                jm = JAMIE(output_dim=8, batch_size=64, epoch_DNN=6, min_epochs=3, pca_dim=pca_dim, use_f_tilde=False, log_DNN=10 ** 9,
                           sampler='device', preprocess=preprocess)
                emb = jm.fit_transform(dataset=data)
            cache[key] = (jm, emb)
        return cache[key]
    return fit


def _pre(jm, i):
    return jm.model.preprocessing[i].__self__


@pytest.mark.parametrize('kind', ['csr', 'ann', 'mixed'])
def test_fit_device_preprocessing_csr_equals_dense(fits, cells, kind):
    jd, ed = fits('device', 'dense')
    js, es = fits('device', kind)
    assert js.row == [N_FIT, N_FIT] and js.col == list(DIMS)
    for i in range(2):
        a, b = _pre(js, i), _pre(jd, i)
        assert a.axis == 0 and a.pca is None and a.mean.shape == (DIMS[i],)
        np.testing.assert_allclose(a.mean, b.mean, **su.MEAN_TOL)
        np.testing.assert_allclose(a.std, b.std, **su.SD_TOL)
        assert isinstance(js.dataset[i], np.ndarray) and js.dataset[i].dtype == np.float32 and js.dataset[i].shape == (N_FIT, DIMS[i])
        np.testing.assert_allclose(js.dataset[i], jd.dataset[i], **su.CELL_TOL)
        print(f'{kind}, modality {i}: max |embedding difference| {np.abs(es[i] - ed[i]).max():.3e}')
        np.testing.assert_allclose(es[i], ed[i], **EMB_TOL)
    assert sp.issparse(cells['csr'][0]) and cells['csr'][0].dtype == np.float64          # the caller's matrices are as they were


def test_fit_host_preprocessing_csr_equals_dense(fits):
    jd, ed = fits('host', 'dense')
    js, es = fits('host', 'csr')
    for i in range(2):
        assert np.array_equal(_pre(js, i).mean, _pre(jd, i).mean) and np.array_equal(_pre(js, i).std, _pre(jd, i).std)
        assert np.array_equal(js.dataset[i], jd.dataset[i])
        np.testing.assert_allclose(es[i], ed[i], **EMB_TOL)


@pytest.fixture(scope='module')
def new_cells():
    """600 new cells per modality: three row chunks of 256, the last ragged."""
    pairs = [su.sparse_counts(600, d, seed=31 + i) for i, d in enumerate(DIMS)]
    return {'csr': [p[0] for p in pairs], 'dense': [p[1] for p in pairs]}


@pytest.mark.parametrize('preprocess', ['device', 'host'])
def test_inference_on_csr_equals_dense(fits, new_cells, preprocess):
    jm, _ = fits(preprocess, 'dense')
    m = jm.model
    chunk = 256
    # the dense eval path at the same chunk size on the host-standardised cells
    std = [m.preprocessing[i](new_cells['dense'][i].astype(np.float64)) for i in range(2)]
    want_emb = [m.embed(torch.as_tensor(std[i]).float(), i, chunk=chunk).cpu().numpy() for i in range(2)]
    got = jm.transform(new_cells['csr'], chunk=chunk)
    for i in range(2):
        assert got[i].shape == (600, 8) and got[i].dtype == np.float32
        assert np.array_equal(got[i], want_emb[i])
        assert np.array_equal(jm.transform_one(new_cells['csr'][i], i, chunk=chunk), want_emb[i])
    decoded = m.impute(torch.as_tensor(std[0]).float(), compose=[0, 1], chunk=chunk)
    want_imp = np.array(m.preprocessing_inverse[1](decoded.detach().cpu()))
    got_imp = jm.modal_predict(new_cells['csr'][0], 0, chunk=chunk)
    assert got_imp.shape == (600, DIMS[1]) and got_imp.dtype == want_imp.dtype == np.float64
    assert np.array_equal(got_imp, want_imp)
    assert np.array_equal(jm.impute(new_cells['csr'][0], 0, chunk=chunk), want_imp)
    # the plain dense facade calls at their default chunk
    dense_emb = jm.transform(new_cells['dense'])
    for i in range(2):
        print(f'{preprocess}, modality {i}: max |transform(csr) - transform(dense)| {np.abs(got[i] - dense_emb[i]).max():.3e}')
        np.testing.assert_allclose(got[i], dense_emb[i], **INFER_TOL)
        np.testing.assert_allclose(jm.transform_one(new_cells['csr'][i], i), jm.transform_one(new_cells['dense'][i], i), **INFER_TOL)
    np.testing.assert_allclose(jm.modal_predict(new_cells['csr'][0], 0), jm.modal_predict(new_cells['dense'][0], 0), **INFER_TOL)
    # other sparse formats, and a wrong feature count
    assert np.array_equal(jm.transform_one(new_cells['csr'][0].tocsc(), 0, chunk=chunk), want_emb[0])
    assert np.array_equal(jm.transform_one(new_cells['csr'][0].tocoo(), 0, chunk=chunk), want_emb[0])
    with pytest.raises(ValueError):
        jm.transform_one(new_cells['csr'][1], 0)


def test_inference_on_csr_value_types_agree(fits, new_cells):
    """fp32, fp64 and int64 values of one integer-valued CSR matrix give the same embeddings and imputations.  The model is fitted
    on the integer-valued (floored) cells, so that the constant column (3, sd 0) standardises to 0 and everything stays finite."""
    jm, _ = fits('device', 'int_dense')
    m = jm.model
    chunk = 256
    counts = new_cells['csr'][0].copy()
    counts.data = np.floor(counts.data)
    dense = np.floor(new_cells['dense'][0])
    types = (np.float32, np.float64, np.int64)
    pre = jm._csr_preclass(0)
    assert pre.mean[su.CONST_COL] == 3.0 and pre.std[su.CONST_COL] == 0.0
    chunks = [list(jm._csr_chunks(counts.astype(t), 0, pre, chunk)) for t in types]
    assert [len(x) for x in chunks[0]] == [256, 256, 88]
    for x32, x64, xi in zip(*chunks):
        assert bool(torch.isfinite(x32).all()) and torch.equal(x32, x64) and torch.equal(x64, xi)
    host_std = torch.as_tensor(m.preprocessing[0](dense.astype(np.int64))).float()
    assert torch.equal(torch.cat(chunks[2], 0).cpu(), host_std)
    outs = [jm.transform_one(counts.astype(t), 0, chunk=chunk) for t in types]
    imps = [jm.modal_predict(counts.astype(t), 0, chunk=chunk) for t in types]
    assert np.isfinite(outs[0]).all() and np.isfinite(imps[0]).all() and np.abs(outs[0]).max() > 0
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[1], outs[2])
    assert np.array_equal(imps[0], imps[1]) and np.array_equal(imps[1], imps[2])
    assert np.array_equal(outs[2], m.embed(host_std, 0, chunk=chunk).cpu().numpy())
    np.testing.assert_allclose(outs[2], jm.transform_one(dense.astype(np.int64), 0), **INFER_TOL)
    np.testing.assert_allclose(imps[2], jm.modal_predict(dense.astype(np.int64), 0), **INFER_TOL)


def test_dense_inference_does_not_pass_chunk_to_a_foreign_model(fits, new_cells):
    """A caller's model class whose `embed` / `impute` take no `chunk` keeps working on dense input at the default chunk."""
    jm, _ = fits('device', 'dense')
    real = jm.model

    class Foreign:
        preprocessing, preprocessing_inverse = real.preprocessing, real.preprocessing_inverse

        def eval(self):
            return self

        def embed(self, x, i):
            return real.embed(x, i)

        def impute(self, X, compose):
            return real.impute(X, compose)
    want = (jm.transform_one(new_cells['dense'][0], 0), jm.modal_predict(new_cells['dense'][0], 0))
    jm.model = Foreign()
    try:
        assert jm._csr_preclass(0) is None
        assert np.array_equal(jm.transform_one(new_cells['dense'][0], 0), want[0])
        assert np.array_equal(jm.modal_predict(new_cells['dense'][0], 0), want[1])
        assert np.array_equal(jm.transform_one(new_cells['csr'][0], 0), want[0])          # sparse: `toarray()`
    finally:
        jm.model = real


def test_inference_on_csr_after_saving_and_loading(fits, new_cells, tmp_path):
    """The fitted `preclass` is reached through the loaded model's bound preprocessing method."""
    from jamie_amd import JAMIE
    jm, _ = fits('device', 'dense')
    path = str(tmp_path / 'model.pt')
    jm.save_model(path)
    other = JAMIE()
    other.load_model(path)
    assert other._csr_preclass(0) is not None
    assert np.array_equal(other.transform_one(new_cells['csr'][0], 0, chunk=256), jm.transform_one(new_cells['csr'][0], 0, chunk=256))


def test_inference_on_csr_with_a_pca_model_densifies(fits, new_cells):
    jm, _ = fits('host', 'dense', pca_dim=[16, 16])
    assert jm._csr_preclass(0) is None and _pre(jm, 0).pca is not None
    for i in range(2):
        assert np.array_equal(jm.transform_one(new_cells['csr'][i], i), jm.transform_one(new_cells['dense'][i], i))
    assert np.array_equal(jm.modal_predict(new_cells['csr'][0], 0), jm.modal_predict(new_cells['dense'][0], 0))
    got = jm.transform(new_cells['csr'])
    want = jm.transform(new_cells['dense'])
    assert all(np.array_equal(a, b) for a, b in zip(got, want))

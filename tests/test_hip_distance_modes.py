"""Stage A on the MI355X for the correlation family (cosine / correlation / pearson) and the L1 family (manhattan = l1 = cityblock,
chebyshev): jamie_amd/distances.py + csrc/distances.hip against the host path's float64 calls.  Run on the GPU box:  pytest -m gpu"""
import contextlib
import io

import numpy as np
import pytest
import torch

from test_host_distance_modes import (CORR_MODES, CORR_TOL, KINDS, L1_TOL, N_COPIES, host_reference, identical_rows,   # noqa: E402
                                      mode_data)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def jd():
    from jamie_amd import _native
    _native.require_gpu()
    from jamie_amd import distances
    return distances


def _check_layout(D, N):
    assert torch.is_tensor(D) and D.is_cuda and D.dtype == torch.float32 and tuple(D.shape) == (N, N)
    h = D.cpu().numpy()
    assert np.array_equal(h, h.T)
    assert (np.diag(h) == 0).all()
    return h


_FUNCS = ('cosine', 'correlation', 'pearson', 'manhattan', 'chebyshev')


# ---- correlation family ----
@pytest.mark.parametrize('d', [3, 16, 50, 2000])
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('mode', CORR_MODES)
def test_correlation_family_vs_host(jd, mode, kind, d):
    X = mode_data(kind, d)
    want = host_reference(X, mode)
    got = _check_layout(getattr(jd, mode)(X), len(X))
    err = np.abs(got.astype(np.float64) - want).max()
    print(f'{mode} {kind} d={d}: max |dD| = {err:.3g}')
    assert err <= CORR_TOL, err
    assert got.min() >= 0 and got.max() <= (1 if mode == 'pearson' else 2) + CORR_TOL
    if kind == 'copies':
        same = identical_rows(X)
        assert same.sum() == 2 * N_COPIES and (got[same] == 0).all()      # exact duplicates: exactly 0


def test_cosine_zero_rows(jd):
    from sklearn.metrics import pairwise_distances
    X = np.random.default_rng(3).standard_normal((64, 7))
    X[[5, 40]] = 0
    want = pairwise_distances(X, metric='cosine')
    got = _check_layout(jd.cosine(X), 64)
    assert np.abs(got - want).max() <= CORR_TOL
    other = np.arange(64)
    assert (got[5, other != 5] == 1).all() and (got[40, other != 40] == 1).all() and got[5, 40] == 1


@pytest.mark.parametrize('mode', ['correlation', 'pearson'])
def test_constant_row_raises(jd, mode):
    X = np.random.default_rng(4).standard_normal((64, 9))
    X[17] = 0.1                              # (3 * 0.1 / 3 != 0.1 in float64: the flag is taken on the entries, not on the norm)
    X[30] = -2.0
    with pytest.raises(ValueError, match='row 17'):
        getattr(jd, mode)(X)
    with pytest.raises(ValueError, match='row 17'):
        getattr(jd, mode)(torch.from_numpy(X.astype(np.float32)).cuda())
    assert bool(torch.isfinite(jd.cosine(X)).all())


# ---- L1 family ----
def _l1_check(jd, X):
    from sklearn.metrics import pairwise_distances
    out = {}
    for name, metric in (('manhattan', 'manhattan'), ('chebyshev', 'chebyshev')):
        want = pairwise_distances(X, metric=metric)
        got = _check_layout(getattr(jd, name)(X), len(X)).astype(np.float64)
        err = np.abs(got - want).max() / max(want.max(), 1e-300)
        print(f'{name} {X.shape}: {err:.3g} max D')
        assert err <= L1_TOL, (name, err)
        out[name] = got
    return out


@pytest.mark.parametrize('d', [1, 3, 31, 32, 33, 50])
@pytest.mark.parametrize('N', [1, 2, 127, 128, 129, 300])
def test_l1_family_vs_sklearn_at_the_tile_edges(jd, N, d):
    X = np.random.default_rng(100 * N + d).standard_normal((N, d)) + 3.0
    got = _l1_check(jd, X)
    if N == 1:
        assert got['manhattan'].tolist() == [[0.0]] and got['chebyshev'].tolist() == [[0.0]]


def test_l1_family_vs_sklearn_d2000(jd):
    _l1_check(jd, np.random.default_rng(11).standard_normal((700, 2000)) + 3.0)


def test_l1_aliases_are_manhattan(jd):
    """'l1' and 'cityblock' go through the facade's routing to the same function: the same bits."""
    import jamie_amd
    X = np.random.default_rng(12).standard_normal((130, 17))
    want = jd.manhattan(X)
    for mode in ('manhattan', 'l1', 'cityblock'):
        f = jamie_amd.JAMIE(distances='device', distance_mode=mode)._device_distance_function()
        assert torch.equal(f(X), want), mode


@pytest.mark.parametrize('N', [90, 300])
def test_l1_family_is_exact_on_integers(jd, N):
    from sklearn.metrics import pairwise_distances
    X = np.random.default_rng(22).integers(-8, 9, (N, 50))
    for name in ('manhattan', 'chebyshev'):
        want = pairwise_distances(X, metric=name)
        for data in (X, X.astype(np.float64), X.astype(np.float32)):
            assert np.array_equal(_check_layout(getattr(jd, name)(data), N).astype(np.float64), want), name


def test_l1_family_duplicates_are_zero(jd):
    X = mode_data('copies', 50)
    same = identical_rows(X)
    for name in ('manhattan', 'chebyshev'):
        got = _check_layout(getattr(jd, name)(X), len(X))
        assert (got[same] == 0).all() and (got[~same & ~np.eye(len(X), dtype=bool)] > 0).all()


# ---- inputs ----
@pytest.mark.parametrize('name', _FUNCS)
def test_n_equals_one(jd, name):
    D = getattr(jd, name)(np.array([[1.0, 2.0, 4.0]]))
    assert _check_layout(D, 1).tolist() == [[0.0]]


@pytest.mark.parametrize('name', _FUNCS)
@pytest.mark.parametrize('bad', [np.nan, np.inf])
def test_non_finite_input_raises(jd, name, bad):
    X = np.random.default_rng(4).standard_normal((50, 5))
    X[7, 3] = bad
    with pytest.raises(ValueError):
        getattr(jd, name)(X)
    with pytest.raises(ValueError):
        getattr(jd, name)(torch.from_numpy(X).cuda())


@pytest.mark.parametrize('name', _FUNCS)
def test_fp32_numpy_equals_a_device_tensor(jd, name):
    X = (np.random.default_rng(2).standard_normal((130, 17)) + 1.0).astype(np.float32)
    assert torch.equal(getattr(jd, name)(X), getattr(jd, name)(torch.from_numpy(X).cuda()))


@pytest.mark.parametrize('name', _FUNCS)
def test_integer_and_sparse_input_equal_float64(jd, name):
    import scipy.sparse as sp
    rng = np.random.default_rng(6)
    Xi = rng.integers(-3, 4, (300, 40)) * (rng.random((300, 40)) < 0.3)
    Xi[:, :4] += 1 << 30                    # 2^30 + small: exact in float64, not in float32 (its ulp there is 128)
    Xf = Xi.astype(np.float64)
    f = getattr(jd, name)
    want = f(Xf)
    for X in (Xi, torch.from_numpy(Xi), sp.csr_matrix(Xf), sp.csr_matrix(Xi)):
        assert torch.equal(f(X), want), type(X)


def test_bad_arguments_return_an_error_before_a_launch(jd):
    from jamie_amd import _native as nv
    X = torch.zeros(8, 4, device='cuda')
    D = torch.empty(8, 8, device='cuda')
    with pytest.raises(nv.JamieHipError, match='op is 0'):
        nv.pairwise_absdiff(X, 2, D)
    with pytest.raises(nv.JamieHipError, match='scale'):
        nv.gram_to_scaled_sqdist(D, torch.zeros(8, device='cuda'), X, 0.0, torch.ones(8, device='cuda'))


# ---- facade, end to end ----
@pytest.mark.parametrize('mode', ['cosine', 'manhattan'])
def test_facade_new_modes_on_the_device(mode):
    import jamie_amd
    from jamie_amd.utilities import distance_matrix
    rng = np.random.default_rng(8)
    Z = rng.standard_normal((120, 4))
    data = [Z @ rng.standard_normal((4, 30)) + 0.1 * rng.standard_normal((120, 30)),
            Z @ rng.standard_normal((4, 20)) + 0.1 * rng.standard_normal((120, 20))]
    with contextlib.redirect_stdout(io.StringIO()):
        jm = jamie_amd.JAMIE(distance_mode=mode, use_f_tilde=True, epoch_pd=20, epoch_DNN=5, output_dim=4, batch_size=64,
                             min_epochs=3, pca_dim=None, log_DNN=10 ** 9, log_pd=10 ** 9, distances='device')
        emb = jm.fit_transform(dataset=data)
    for got, X in zip(jm.dist, data):
        assert torch.is_tensor(got) and got.is_cuda and got.dtype == torch.float32
        want = distance_matrix(X, mode)
        tol = CORR_TOL if mode == 'cosine' else L1_TOL * want.max()
        assert np.abs(got.cpu().numpy() - want).max() <= tol
    assert len(emb) == 2 and np.isfinite(emb[0]).all() and np.isfinite(emb[1]).all()

"""Stage A on the device, the correlation family (cosine / correlation / pearson) and the L1 family (manhattan / chebyshev):
the facade's keyword, and the design of jamie_amd/distances.py + csrc/distances.hip restated in numpy fp32 and checked on the CPU
against the host path's float64 calls (utilities.distance_matrix).  The data kinds are shared with test_hip_distance_modes.py."""
import numpy as np
import pytest

NEW_MODES = ('cosine', 'correlation', 'pearson', 'manhattan', 'l1', 'cityblock', 'chebyshev')
CORR_MODES = ('cosine', 'correlation', 'pearson')
KINDS = ('gaussian', 'counts', 'offset', 'copies')
N_CELLS = 400
TAU = 2.0 ** -10            # csrc/distances.hip DIST_TAU
# |dD| <= CORR_TOL absolute: these distances live in [0, 2], so this is about 32 fp32 ulp of 1
CORR_TOL = 2e-6
# |dD| <= L1_TOL * max(D): the project's EUC_TOL (tests/test_hip_distances.py)
L1_TOL = 1e-5
N_COPIES = 20               # of each sort in the 'copies' kind


def mode_data(kind, d, N=N_CELLS):
    """gaussian: N(0, 1).  counts: log1p of Poisson(5) counts (non-negative, many ties); a row that came out constant (likely at
    d = 3) has no correlation with anything and is drawn again.  offset: N(50, 1), every cosine distance tiny.  copies: Gaussian
    cells plus N_COPIES exact copies, N_COPIES cells scaled by 3 and N_COPIES copies with noise sigma = 1e-3, shuffled."""
    rng = np.random.default_rng(1000 * KINDS.index(kind) + d)
    if kind == 'gaussian':
        return rng.standard_normal((N, d))
    if kind == 'offset':
        return rng.standard_normal((N, d)) + 50.0
    if kind == 'counts':
        X = np.log1p(rng.poisson(5.0, (N, d)).astype(np.float64))
        while True:
            flat = np.nonzero((X == X[:, :1]).all(1))[0]
            if d == 1 or not len(flat):
                return X
            X[flat] = np.log1p(rng.poisson(5.0, (len(flat), d)))
    B = rng.standard_normal((N - 3 * N_COPIES, d))
    src = rng.choice(len(B), 3 * N_COPIES, replace=False)
    X = np.concatenate([B, B[src[:N_COPIES]], 3.0 * B[src[N_COPIES:2 * N_COPIES]],
                        B[src[2 * N_COPIES:]] + 1e-3 * rng.standard_normal((N_COPIES, d))])
    return X[rng.permutation(N)]


def identical_rows(X):
    """[N, N] bool: rows i != j of X are the same numbers."""
    inv = np.unique(X, axis=0, return_inverse=True)[1].reshape(-1)
    return (inv[:, None] == inv[None, :]) & ~np.eye(len(X), dtype=bool)


def host_reference(X, mode):
    from jamie_amd.utilities import distance_matrix
    return np.asarray(distance_matrix(X, mode), np.float64)


# ---- the facade keyword ----
@pytest.mark.parametrize('mode', NEW_MODES)
def test_device_distances_accept_the_new_modes(mode):
    import jamie_amd
    jm = jamie_amd.JAMIE(distances='device', distance_mode=mode)
    assert jm.distances == 'device' and jm.distance_mode == mode


@pytest.mark.parametrize('mode', ['spearman', 'jaccard', 'minkowski'])
def test_device_distances_still_refuse_other_modes(mode):
    import jamie_amd
    with pytest.raises(ValueError, match='host'):
        jamie_amd.JAMIE(distances='device', distance_mode=mode)
    assert jamie_amd.JAMIE(distances='host', distance_mode=mode).distance_mode == mode


# ---- correlation family: unit rows in fp32, the Gram form with its recompute, the scale, the zero-row rule ----
def _row_sqnorm_fp32(U):
    """row_sqnorm_kernel's order: 64 strided partial sums, then a tree."""
    N, d = U.shape
    P = np.zeros((N, -(-d // 64) * 64), np.float32)
    P[:, :d] = U
    n = np.zeros((N, 64), np.float32)
    for c in range(0, P.shape[1], 64):
        n = n + P[:, c:c + 64] * P[:, c:c + 64]
    while n.shape[1] > 1:
        n = n[:, 0::2] + n[:, 1::2]
    return n[:, 0]


def fma_chain_product(U):
    """U U^T as the fp32 matrix pipe forms it: one fma chain per entry in ascending k (a product of two fp32 numbers is exact in
    float64, so rounding acc + a b to fp32 once per step is the fma)."""
    U = U.astype(np.float64)
    acc = np.zeros((len(U), len(U)), np.float64)
    for k in range(U.shape[1]):
        acc = (acc + np.outer(U[:, k], U[:, k])).astype(np.float32).astype(np.float64)
    return acc.astype(np.float32)


def unit_row_design_fp32(X, mode, recompute=True, centre_columns=True, product=lambda U: U @ U.T):
    """jamie_row_normalise (fp64, one rounding) -> the unit rows column-centred (fp64 mean, one rounding) -> G in fp32 ->
    tile_pair_kernel<3>.  -> (D fp32, recomputed pairs)"""
    X = np.asarray(X, np.float64)
    if mode != 'cosine':
        X = X - X.mean(1, keepdims=True)
    nrm = np.sqrt((X * X).sum(1))
    U = np.where(nrm[:, None] > 0, X / np.where(nrm > 0, nrm, 1.0)[:, None], 0.0).astype(np.float32)
    if centre_columns:
        U = (U.astype(np.float64) - U.astype(np.float64).mean(0)).astype(np.float32)
    n = _row_sqnorm_fp32(U)
    s = n[:, None] + n[None, :]
    q = np.maximum(s - np.float32(2) * product(U), np.float32(0)).astype(np.float32)
    off = ~np.eye(len(X), dtype=bool)
    redo = (q < np.float32(TAU) * s) & off
    if recompute:
        for i in np.nonzero(redo.any(1))[0]:
            js = np.nonzero(redo[i])[0]
            q[i, js] = ((U[i] - U[js]) ** 2).sum(1, dtype=np.float32)
    q[~off] = 0
    D = np.float32(0.25 if mode == 'pearson' else 0.5) * q
    zero = nrm == 0
    D[(zero[:, None] | zero[None, :]) & off] = 1
    return D, redo


@pytest.mark.parametrize('d', [3, 16, 50, 2000])
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('mode', CORR_MODES)
def test_unit_row_gram_form_meets_the_bound(mode, kind, d):
    X = mode_data(kind, d)
    want = host_reference(X, mode)
    assert np.isfinite(want).all()
    got, redo = unit_row_design_fp32(X, mode)
    err = np.abs(got.astype(np.float64) - want).max()
    print(f'{mode} {kind} d={d}: max |dD| = {err:.3g}, recomputed {redo.mean():.2%}')
    assert err <= CORR_TOL, err
    assert np.array_equal(got, got.T) and (np.diag(got) == 0).all()
    assert got.min() >= 0 and got.max() <= (1 if mode == 'pearson' else 2) + CORR_TOL
    if kind == 'copies':
        same = identical_rows(X)
        assert same.sum() == 2 * N_COPIES and (got[same] == 0).all()      # exact duplicates: exactly 0
    if kind in ('gaussian', 'offset') and d >= 16:
        assert redo.mean() < 0.01


@pytest.mark.parametrize('d', [16, 50, 2000])
def test_offset_cosine_is_the_recompute_cliff_of_uncentred_unit_rows(d):
    """All-positive rows with a large common offset are nearly parallel unit rows: every cosine distance is tiny.  On the unit rows
    as they come the Gram form loses them and more than 90 % of the pairs fall to the one-pair-per-wave recompute (it restores
    the bound, slowly); column-centring the unit rows, which |u - v|^2 does not see, takes the case off the cliff."""
    X = mode_data('offset', d)
    want = host_reference(X, 'cosine')
    plain, redo = unit_row_design_fp32(X, 'cosine', recompute=False, centre_columns=False)
    assert redo.mean() > 0.9
    assert np.abs(plain - want).max() > 1e-4 * want.max()
    fixed, _ = unit_row_design_fp32(X, 'cosine', centre_columns=False)
    got, redo = unit_row_design_fp32(X, 'cosine')
    assert redo.mean() < 0.01
    for D in (fixed, got):                                  # (relative to these tiny distances: at d = 2000, max D = 4.5e-4)
        assert np.abs(D - want).max() <= (1e-5 * want.max() if d == 2000 else CORR_TOL)


def test_dense_counts_need_the_column_centring():
    """Dense log1p counts are nearly parallel too (cosine distances of a few per cent: nothing is recomputed), and every Gram entry
    is a d = 2000 fma chain that ends near 1: on the unit rows as they come the chain's rounding alone passes the bound."""
    X = mode_data('counts', 2000, N=200)
    want = host_reference(X, 'cosine')
    raw, redo = unit_row_design_fp32(X, 'cosine', centre_columns=False, product=fma_chain_product)
    assert not redo.any() and np.abs(raw - want).max() > CORR_TOL
    got, _ = unit_row_design_fp32(X, 'cosine', product=fma_chain_product)
    assert np.abs(got - want).max() <= CORR_TOL / 4


def test_cosine_zero_rows_are_at_distance_one():
    from sklearn.metrics import pairwise_distances
    X = np.random.default_rng(3).standard_normal((64, 7))
    X[[5, 40]] = 0
    want = pairwise_distances(X, metric='cosine')
    assert want[5, 40] == 1 and want[5, 6] == 1 and want[5, 5] == 0       # sklearn's rule
    got, _ = unit_row_design_fp32(X, 'cosine')
    assert np.abs(got - want).max() <= CORR_TOL
    assert (got[5, np.arange(64) != 5] == 1).all() and (got[np.arange(64) != 40, 40] == 1).all() and got[5, 5] == 0


# ---- L1 family: the chunked accumulation ----
def absdiff_design_fp32(X, op, chunk=32):
    """absdiff_kernel's arithmetic: fp32 rows (column-centred in fp64 first unless they are fp32 numbers already), one chain per
    pair in ascending c, sums in chunks of `chunk` features."""
    X = np.asarray(X, np.float64)
    R = X.astype(np.float32)
    if not (R.astype(np.float64) == X).all():
        R = (X - X.mean(0)).astype(np.float32)
    N, d = R.shape
    D = np.zeros((N, N), np.float32)
    for c0 in range(0, d, chunk):
        part = np.zeros((N, N), np.float32)
        for c in range(c0, min(c0 + chunk, d)):
            t = np.abs(R[:, c][:, None] - R[:, c][None, :])
            part = np.maximum(part, t) if op == 'max' else part + t
        D = np.maximum(D, part) if op == 'max' else D + part
    return D


def test_chunked_l1_accumulation_meets_the_bound():
    from sklearn.metrics import pairwise_distances
    X = np.random.default_rng(21).standard_normal((300, 2000)) + 3.0
    want = pairwise_distances(X, metric='manhattan')
    got = absdiff_design_fp32(X, 'sum')
    err = np.abs(got - want).max() / want.max()
    print(f'chunked L1, d = 2000: {err:.3g} max D')
    assert err <= L1_TOL, err
    assert np.array_equal(got, got.T) and (np.diag(got) == 0).all()
    one_chain = absdiff_design_fp32(X, 'sum', chunk=2000)
    assert err < np.abs(one_chain - want).max() / want.max()               # what the chunks buy


def test_l1_design_is_exact_on_integers():
    from sklearn.metrics import pairwise_distances
    X = np.random.default_rng(22).integers(-8, 9, (90, 50))
    for op, metric in (('sum', 'manhattan'), ('max', 'chebyshev')):
        assert np.array_equal(absdiff_design_fp32(X, op).astype(np.float64), pairwise_distances(X, metric=metric))

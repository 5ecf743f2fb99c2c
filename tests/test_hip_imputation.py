"""Imputation metrics on the device (jamie_amd/imputation.py, csrc/imputation.hip) against float64 references.

Correlation and MSE: the device keeps fp64 sums of values shifted by row 0 of their feature, so |r - r_ref| <= 1e-10 and the MSE
is within 1e-12 relative (the same arithmetic on the host is within 1.3e-14 of the reference at N = 5000 with the offsets used
here; fp64 sums without the shift miss by 1.6e-6, fp32 sums by 6.9e-6, a shift in fp32 by 1.9e-9).  AUROC: U2 and n_pos are
integers and must equal the reference exactly.  Before a device result is looked at, the reference alone must show that the
real-valued AUROC columns are neither degenerate nor saturated (mean in [0.55, 0.95]).  Every figure is printed before it is
asserted."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import imputation_util as iu  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ji():
    from jamie_amd import imputation
    return imputation


def _check_stats(X, Y, r, mse):
    r_ref, mse_ref = iu.reference_r_mse(X, Y)
    nan_ref = np.isnan(r_ref)
    err_r = float(np.max(np.abs(r - r_ref)[~nan_ref])) if (~nan_ref).any() else 0.0
    with np.errstate(divide='ignore', invalid='ignore'):
        rel = np.where(mse_ref > 0, np.abs(mse - mse_ref) / mse_ref, np.abs(mse))
    print(f'shape {X.shape}: NaN r at {list(np.where(np.isnan(r))[0])}, reference {list(np.where(nan_ref)[0])}; '
          f'max |r - r_ref| {err_r:.3e}, max MSE relative error {float(rel.max()):.3e}')
    assert r.dtype == np.float64 and mse.dtype == np.float64 and r.shape == mse.shape == (X.shape[1],)
    assert np.array_equal(np.isnan(r), nan_ref)
    assert err_r <= iu.R_TOL
    assert float(rel.max()) <= iu.MSE_RTOL
    return r_ref, mse_ref


@pytest.mark.parametrize('N,d', [(2, 1), (257, 33), (5000, 70), (4097, 130), (1300, 9), (1030, 8), (777, 132)])
def test_correlation_and_mse_vs_float64(ji, N, d):
    """(1300, 9) and (1030, 8) span three row blocks of the kernel's grid, the second on the 16-byte load path with a last
    block of 6 rows; (777, 132) has a third column block of one 16-byte load."""
    if N in (1300, 1030):
        assert N > 2 * ji.ROW_BLOCK
    X, Y = iu.stats_case(N, d)
    r, mse = ji.feature_correlation_mse(X, Y)
    r_ref, mse_ref = _check_stats(X, Y, r, mse)
    if d > 4:
        assert list(np.where(np.isnan(r))[0]) == [2, 4]                # the constant columns, and only they
        print(f'X == Y column: mse {mse[3]!r}, 1 - r {1 - r[3]:.3e}')
        assert mse[3] == 0.0 and abs(r[3] - 1.0) <= iu.R_TOL
        assert 1e4 - 1 < X[:, 0].mean() < 1e4 + 1 and 3e4 - 1 < Y[:, 0].mean() < 3e4 + 1
    r2, mse2 = ji.feature_correlation_mse(X, Y)
    assert r.tobytes() == r2.tobytes() and mse.tobytes() == mse2.tobytes()       # bit-identical, NaN included


def test_stats_take_device_tensors_and_float64_input(ji):
    X, Y = iu.stats_case(257, 33)
    r, mse = ji.feature_correlation_mse(X, Y)
    r2, mse2 = ji.feature_correlation_mse(torch.from_numpy(X.copy()).cuda(), Y.astype(np.float64))
    assert r.tobytes() == r2.tobytes() and mse.tobytes() == mse2.tobytes()
    bad = X.copy()
    bad[5, 7] = np.nan
    with pytest.raises(ValueError):
        ji.feature_correlation_mse(bad, Y)
    bad[5, 7] = np.inf
    with pytest.raises(ValueError):
        ji.feature_auroc(X, bad)


def _check_reference(N, d, halves=False):
    X, Y, real = iu.auroc_case(N, d, halves)
    U2, n_pos = iu.auroc_reference(N, d, halves)
    auc = iu.auroc_of(U2, n_pos, N)
    print(f'reference N = {N}, d = {d}: mean AUROC of the real-valued columns {auc[real].mean():.4f}, NaN at '
          f'{list(np.where(np.isnan(auc))[0])}')
    assert 0.55 <= auc[real].mean() <= 0.95
    if d > 7:
        assert n_pos[3] == N - 1 and n_pos[4] == 1 and n_pos[5] == N and n_pos[6] == 0
        assert U2[5] == 0 and U2[6] == 0 and list(np.where(np.isnan(auc))[0]) == [5, 6]
        assert auc[7] == 0.5                                           # every score equal: all ties
        z = X[:, 2]
        assert (np.signbit(z) & (z == 0)).any() and (~np.signbit(z) & (z == 0)).any()
    return X, Y, U2, n_pos, auc


def _check_counts(got_auc, got, U2, n_pos, auc):
    gU2, gn = got
    print(f'features with U2 off {int((gU2 != U2).sum())}, with n_pos off {int((gn != n_pos).sum())}')
    assert gU2.dtype == np.int64 and gn.dtype == np.int64
    assert np.array_equal(gn, n_pos)
    assert np.array_equal(gU2, U2)
    assert np.array_equal(np.isnan(got_auc), np.isnan(auc))
    assert np.array_equal(got_auc[~np.isnan(auc)], auc[~np.isnan(auc)])   # the same integers through the same division


def _sizes(ji):
    C = ji.CHUNK
    return [C - 1, C + 1, 2 * C + 5, 4 * C + 17]


@pytest.mark.parametrize('which', range(4))
@pytest.mark.parametrize('d', [1, 33, 70])
def test_auroc_counts_are_exact(ji, which, d):
    """N = CHUNK - 1: one run; CHUNK + 1: a second run of one real key; 2 CHUNK + 5: a run without a partner in the first merge
    pass; 4 CHUNK + 17: two full passes and a third.  Columns 1 .. 7: halves, signed zeros, one negative, one positive, one
    class only (twice), every score equal."""
    N = _sizes(ji)[which]
    X, Y, U2, n_pos, auc = _check_reference(N, d)
    got_auc, got = ji.feature_auroc(X, Y, return_counts=True)
    _check_counts(got_auc, got, U2, n_pos, auc)
    again_auc, again = ji.feature_auroc(X, Y, return_counts=True)
    assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1])
    assert again_auc.tobytes() == got_auc.tobytes()


def test_auroc_heavy_ties(ji):
    N = 2 * ji.CHUNK + 5
    X, Y, U2, n_pos, auc = _check_reference(N, 33, halves=True)
    print(f'distinct scores in column 0: {len(np.unique(X[:, 0]))} of {N}')
    assert len(np.unique(X[:, 0])) < 40
    got_auc, got = ji.feature_auroc(X, Y, return_counts=True)
    _check_counts(got_auc, got, U2, n_pos, auc)


def test_auroc_threshold_vector(ji):
    N, d = ji.CHUNK + 1, 33
    X, Y, real = iu.auroc_case(N, d)
    thr = (np.arange(d) - 16) / 32.0                                   # (exact in fp32)
    U2, n_pos = iu.reference_u2(X, Y, thr)
    auc = iu.auroc_of(U2, n_pos, N)
    print(f'reference: mean AUROC of the real-valued columns {auc[real].mean():.4f}; n_pos {n_pos[real].min()} .. {n_pos[real].max()}')
    assert 0.55 <= auc[real].mean() <= 0.95
    assert n_pos[real].max() - n_pos[real].min() > N // 8             # the thresholds do move the labels
    got_auc, got = ji.feature_auroc(X, Y, threshold=thr, return_counts=True)
    _check_counts(got_auc, got, U2, n_pos, auc)
    # a scalar threshold other than 0, on device tensors
    U2, n_pos = iu.reference_u2(X, Y, 0.25)
    got_auc, got = ji.feature_auroc(torch.from_numpy(X.copy()).cuda(), torch.from_numpy(Y.copy()).cuda(), threshold=0.25,
                                    return_counts=True)
    _check_counts(got_auc, got, U2, n_pos, iu.auroc_of(U2, n_pos, N))


def test_auroc_feature_groups_under_a_workspace_cap(ji):
    N, d = ji.CHUNK + 1, 70
    X, Y, U2, n_pos, auc = _check_reference(N, d)
    cap = 30 * 8 * 2 * ji.CHUNK
    groups = ji.plan(N, d, cap)['groups']
    print(f'groups under a cap of {cap} bytes: {groups}')
    assert len(groups) >= 3 and groups[-1][1] < groups[0][1]
    free_auc, free = ji.feature_auroc(X, Y, return_counts=True)
    got_auc, got = ji.feature_auroc(X, Y, max_workspace=cap, return_counts=True)
    _check_counts(got_auc, got, U2, n_pos, auc)
    assert np.array_equal(got[0], free[0]) and np.array_equal(got[1], free[1]) and got_auc.tobytes() == free_auc.tobytes()
    one_auc, one = ji.feature_auroc(X, Y, max_workspace=8 * 2 * ji.CHUNK, return_counts=True)     # a feature at a time
    assert np.array_equal(one[0], U2) and np.array_equal(one[1], n_pos)
    with pytest.raises(ValueError):
        ji.feature_auroc(X, Y, max_workspace=8 * 2 * ji.CHUNK - 1)


def test_facade_device_equals_the_module_and_agrees_with_the_host(ji, capsys):
    from jamie_amd import JAMIE
    N, d = ji.CHUNK + 1, 33
    X, Y, real = iu.auroc_case(N, d)
    thr = 0.125
    dev = JAMIE(metrics='device').test_imputation(X, Y, threshold=thr)
    lines = capsys.readouterr().out.strip().splitlines()[-3:]
    host = JAMIE(metrics='host').test_imputation(X, Y, threshold=thr)
    r, mse = ji.feature_correlation_mse(X, Y)
    auc = ji.feature_auroc(X, Y, threshold=thr)
    assert dev['correlation'].tobytes() == r.tobytes() and dev['mse'].tobytes() == mse.tobytes()
    assert dev['auroc'].tobytes() == auc.tobytes()
    m = ji.imputation_metrics(X, Y, threshold=thr)
    assert all(m[k].tobytes() == dev[k].tobytes() for k in ('correlation', 'mse', 'auroc'))
    assert lines == [f"imputation correlation: {float(np.nanmean(r))}", f"imputation mse: {float(np.nanmean(mse))}",
                     f"imputation auroc: {float(np.nanmean(auc))}"]
    for k, tol in (('correlation', iu.R_TOL), ('auroc', iu.AUROC_TOL)):
        nan = np.isnan(host[k])
        err = float(np.max(np.abs(dev[k] - host[k])[~nan]))
        print(f'{k}: device against host, max difference {err:.3e}; NaN at {list(np.where(nan)[0])}')
        assert np.array_equal(np.isnan(dev[k]), nan) and err <= tol
    rel = float(np.max(np.abs(dev['mse'] - host['mse']) / host['mse']))
    print(f'mse: device against host, max relative difference {rel:.3e}')
    assert rel <= iu.MSE_RTOL
    assert 0.55 <= host['auroc'][real].mean() <= 0.95

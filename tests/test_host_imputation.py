"""Imputation metrics without a GPU: the plan arithmetic, the device's AUROC pipeline restated in numpy against brute-force pair
counting, the key map, the facade's host `test_imputation` against the float64 references, the argument checks and the new
kernels' code objects."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import imputation_util as iu  # noqa: E402


def test_plan_arithmetic():
    from jamie_amd import imputation as ji
    C = ji.CHUNK
    assert C >= 256 and C & (C - 1) == 0
    for N, runs, passes in ((2, 1, 0), (C - 1, 1, 0), (C, 1, 0), (C + 1, 2, 1), (2 * C + 5, 3, 2), (4 * C, 4, 2), (4 * C + 17, 5, 3),
                            (100000, -(-100000 // C), int(np.ceil(np.log2(-(-100000 // C)))))):
        p = ji.plan(N, 10)
        assert p['Npad'] == runs * C and p['Npad'] >= N and p['Npad'] - N < C
        assert (p['runs'], p['passes']) == (runs, passes), (N, p)
        assert p['groups'] == [(0, 10)] and p['workspace'] == 8 * p['Npad'] * 10
    # a cap that holds 30 features of 70: groups 30 + 30 + 10, every feature once, the last group partial
    N, d = C + 1, 70
    per = 8 * 2 * C
    p = ji.plan(N, d, 30 * per + per - 1)
    assert p['groups'] == [(0, 30), (30, 30), (60, 10)] and p['workspace'] == 30 * per
    covered = np.concatenate([np.arange(f0, f0 + n) for f0, n in p['groups']])
    assert np.array_equal(covered, np.arange(d))
    assert ji.plan(N, d, per)['groups'] == [(f, 1) for f in range(d)]
    assert len(ji.plan(2 * ji.MAX_GROUP + 1, 3)['groups']) == 1
    assert [n for _, n in ji.plan(2, 2 * ji.MAX_GROUP + 1, 1 << 40)['groups']] == [ji.MAX_GROUP, ji.MAX_GROUP, 1]
    with pytest.raises(ValueError):
        ji.plan(N, d, per - 1)
    with pytest.raises(ValueError):
        ji.plan(1, 5)
    with pytest.raises(ValueError):
        ji.plan(5, 0)


def test_workspace_function_needs_no_gpu_and_agrees_with_the_plan():
    from jamie_amd import _native as nv
    from jamie_amd import imputation as ji
    for N, d in ((2, 1), (ji.CHUNK, 3), (ji.CHUNK + 1, 70), (100000, 2000)):
        assert nv.imputation_workspace(N, d, 1) == ji.plan(N, d, 1 << 50)['workspace']
        assert nv.imputation_workspace(N, d, 0) == -(-N // ji.ROW_BLOCK) * 6 * d * 8
    assert nv.imputation_workspace(0, 5, 0) == 0 and nv.imputation_workspace(5, 0, 1) == 0 and nv.imputation_workspace(5, 5, 2) == 0
    for name in ('jamie_imputation_workspace', 'jamie_feature_stats', 'jamie_feature_auroc'):
        assert name in nv.EXPORTS


@pytest.mark.parametrize('N,chunk', [(63, 64), (65, 64), (2 * 64 + 5, 64), (4 * 64 + 17, 64), (7 * 32, 32), (1, 8), (301, 16)])
def test_pipeline_restatement_equals_pair_counting(N, chunk):
    """Key map -> chunk sort -> rank merge (an odd number of runs included) -> count, in numpy, against all pairs."""
    rng = np.random.default_rng(N)
    runs = -(-N // chunk)
    want_passes = int(np.ceil(np.log2(runs))) if runs > 1 else 0
    for kind in ('real', 'halves', 'zeros', 'one_neg', 'one_pos', 'all_pos', 'all_neg'):
        x = rng.standard_normal(N).astype(np.float32)
        label = x + rng.standard_normal(N) > 0
        if kind == 'halves':
            x = (np.round(x * 2) / 2).astype(np.float32)
        elif kind == 'zeros':
            x = rng.choice(np.array([-0.0, 0.0, -1.0, 1.0], np.float32), N)
        elif kind == 'one_neg':
            label[:] = True
            label[N // 2] = False
        elif kind == 'one_pos':
            label[:] = False
            label[N // 2] = True
        elif kind in ('all_pos', 'all_neg'):
            label[:] = kind == 'all_pos'
        want = iu.brute_force_u2(x, label)
        got, n_pos, passes = iu.pipeline_u2(x, label, chunk)
        assert got == want and n_pos == label.sum() and passes == want_passes, (kind, got, want)
        U2, npos = iu.reference_u2(x[:, None], np.where(label, 1.0, -1.0)[:, None], 0.0)
        assert U2[0] == want and npos[0] == n_pos


@pytest.mark.parametrize('n_chunks,chunk,T,lanes', [(2, 16, 8, 4), (3, 16, 8, 4), (5, 32, 16, 4), (7, 16, 16, 64), (8, 64, 32, 64),
                                                    (5, 4096, 2048, 64)])
def test_merge_windows_equal_the_rank_merge(n_chunks, chunk, T, lanes):
    """The kernel's walk of a merge pass -- windows of T output keys, their slices of the two runs found by a many-way merge-path
    search, ranked against each other -- gives the rank merge's array in every pass, with an odd number of runs, heavy ties and
    sentinels; the split search reads inside the runs only and takes a few steps."""
    rng = np.random.default_rng(n_chunks * chunk)
    n = n_chunks * chunk
    for kind in ('real', 'ties', 'sentinels', 'skewed'):
        keys = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        if kind == 'ties':
            keys = rng.integers(5, 9, n).astype(np.uint32)
        elif kind == 'sentinels':
            keys[rng.random(n) < 0.7] = iu.SENTINEL
        elif kind == 'skewed':                                     # every key of the even chunks below every key of the odd ones
            keys = (keys >> 1) + (((np.arange(n) // chunk) % 2).astype(np.uint32) << 31)
        keys = np.sort(keys.reshape(-1, chunk), axis=1).reshape(-1)
        R = chunk
        while R < n:
            want = iu.rank_merge_pass(keys, R)
            got = iu.merge_pass_windows(keys, R, T, lanes)
            assert np.array_equal(got, want), (kind, R)
            keys, R = want, 2 * R
        assert np.all(keys[:-1] <= keys[1:])
    A = np.sort(rng.integers(0, 1000, 1 << 19).astype(np.uint32))
    B = np.sort(rng.integers(0, 1000, 1 << 19).astype(np.uint32))
    for diag in (0, 1, 12345, 1 << 19, (1 << 20) - 1, 1 << 20):
        split, steps = iu.merge_split(A, B, diag)
        merged_first = np.sort(np.concatenate([A, B]), kind='stable')[:diag]
        assert np.array_equal(np.sort(np.concatenate([A[:split], B[:diag - split]])), merged_first) and steps <= 5
        assert split == 0 or diag - split == len(B) or A[split - 1] <= B[diag - split]
        assert split == len(A) or diag == split or A[split] > B[diag - split - 1]


def test_reference_u2_is_roc_auc_score():
    from sklearn.metrics import roc_auc_score
    X, Y, real = iu.auroc_case(3000, 9)
    U2, n_pos = iu.reference_u2(X, Y, 0.0)
    auc = iu.auroc_of(U2, n_pos, len(X))
    for f in range(X.shape[1]):
        lab = Y[:, f] > 0
        if 0 < lab.sum() < len(X):
            assert abs(auc[f] - roc_auc_score(lab, X[:, f])) <= iu.AUROC_TOL
        else:
            assert np.isnan(auc[f]) and U2[f] == 0
    assert np.isnan(auc).sum() == 2


def test_key_map_is_monotone():
    tiny = np.float32(1e-45)
    fmax = np.finfo(np.float32).max
    x = np.array([-np.inf, -fmax, -1.5, -1.0, -np.finfo(np.float32).tiny, -2 * tiny, -tiny, -0.0, 0.0, tiny, 2 * tiny,
                  np.finfo(np.float32).tiny, 1.0, 1.5, fmax, np.inf], np.float32)
    assert np.all(np.diff(x.astype(np.float64)) >= 0)
    k = iu.order_keys(x).astype(np.int64)
    zero = int(np.where(x == 0)[0][0])
    assert k[zero] == k[zero + 1] and np.signbit(x[zero]) and not np.signbit(x[zero + 1])
    d = np.diff(k)
    assert np.all(np.delete(d, zero) > 0) and d[zero] == 0
    assert k[-2] < int(iu.SENTINEL) and k[-1] < int(iu.SENTINEL)        # no finite score (nor +inf) meets the sentinel
    # and on random bit patterns the keys order as the floats do
    rng = np.random.default_rng(0)
    r = rng.integers(0, 1 << 32, 20000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    r = r[np.isfinite(r)]
    order = np.argsort(iu.order_keys(r), kind='stable')
    assert np.all(np.diff(r[order].astype(np.float64)) >= 0)


def test_host_test_imputation_equals_the_references(capsys):
    from jamie_amd import JAMIE
    X, Y, real = iu.auroc_case(1500, 12)
    out = JAMIE(metrics='host').test_imputation(X, Y)
    lines = capsys.readouterr().out.strip().splitlines()[-3:]
    r, mse = iu.reference_r_mse(X, Y)
    U2, n_pos = iu.reference_u2(X, Y, 0.0)
    auc = iu.auroc_of(U2, n_pos, len(X))
    assert set(out) == {'correlation', 'mse', 'auroc'}
    assert np.array_equal(np.isnan(out['correlation']), np.isnan(r)) and np.isnan(r).sum() == 3
    assert np.nanmax(np.abs(out['correlation'] - r)) <= iu.R_TOL
    assert np.all(np.abs(out['mse'] - mse) <= iu.MSE_RTOL * mse)
    # the one-class features (all positive, all negative) have no AUROC; the others are sklearn's
    assert np.array_equal(np.isnan(out['auroc']), np.isnan(auc)) and list(np.where(np.isnan(auc))[0]) == [5, 6]
    assert np.nanmax(np.abs(out['auroc'] - auc)) <= iu.AUROC_TOL
    assert 0.55 <= auc[real].mean() <= 0.95
    assert lines == [f"imputation correlation: {float(np.nanmean(out['correlation']))}", f"imputation mse: {float(np.nanmean(out['mse']))}",
                     f"imputation auroc: {float(np.nanmean(out['auroc']))}"]
    # a threshold per feature, and torch tensors
    import torch
    thr = (np.arange(12) - 6) / 16.0
    out2 = JAMIE().test_imputation(torch.from_numpy(X.copy()), torch.from_numpy(Y.copy()), threshold=thr)
    U2, n_pos = iu.reference_u2(X, Y, thr)
    assert np.nanmax(np.abs(out2['auroc'] - iu.auroc_of(U2, n_pos, len(X)))) <= iu.AUROC_TOL
    with pytest.raises(ValueError):
        JAMIE().test_imputation(X, Y[:-1])


def test_bad_arguments_raise_value_error_without_a_gpu():
    from jamie_amd import imputation as ji
    a = np.zeros((6, 3), np.float32)
    for fn in (ji.feature_correlation_mse, ji.feature_auroc, ji.imputation_metrics):
        with pytest.raises(ValueError):
            fn(a, np.zeros((6, 4), np.float32))
        with pytest.raises(ValueError):
            fn(a, np.zeros((5, 3), np.float32))
        with pytest.raises(ValueError):
            fn(a[:1], a[:1])
        with pytest.raises(ValueError):
            fn(a[:, :0], a[:, :0])
        with pytest.raises(ValueError):
            fn(a[0], a[0])
    with pytest.raises(ValueError):
        ji.feature_auroc(a, a, max_workspace=8 * ji.CHUNK - 1)
    with pytest.raises(ValueError):
        ji.imputation_metrics(a, a, max_workspace=100)
    with pytest.raises(ValueError):
        ji.feature_auroc(a, a, threshold=np.zeros(4))
    with pytest.raises(ValueError):
        ji.feature_auroc(a, a, threshold=np.nan)


def test_imputation_kernels_use_no_scratch():
    """private_segment_fixed_size == 0 for every kernel of csrc/imputation.hip, read from the code object hipcc built."""
    import isa_check as ic
    obj = os.path.join(ROOT, 'jamie_amd', 'csrc', '_obj', 'imputation.o')
    if not os.path.exists(obj):
        pytest.skip('the library is not built')
    if not os.path.exists(ic.OBJDUMP):
        pytest.skip('llvm-objdump not found')
    meta = ic.kernel_metadata(obj)
    names = ' '.join(meta)
    for kernel in ('feature_stats_kernel', 'feature_stats_final_kernel', 'score_tile_kernel', 'chunk_sort_kernel', 'rank_merge_kernel'):
        assert kernel in names, (kernel, names)
    assert len(meta) == 6
    for name, m in meta.items():
        assert m['private_segment_fixed_size'] == 0, (name, m)
        assert m.get('vgpr_spill_count', 0) == 0, (name, m)

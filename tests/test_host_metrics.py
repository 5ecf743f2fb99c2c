"""Alignment metrics without a GPU: the tile schedule and the vote rule of csrc/metrics.hip restated in numpy against the
reference's own code, the facade's `metrics=` keyword and host `test_LabelTA`, and the new kernels' code objects."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import metrics_util as mu  # noqa: E402


@pytest.mark.parametrize('N,L', [(256, 8), (300, 5), (1, 3), (129, 33), (517, 32)])
def test_tile_schedule_equals_the_reference_loop(N, L):
    """Pair tiles of the kernel's shape, one pass feeding row and column counts, j = i excluded by index, ragged last tile: the
    counts of the loop of `test_closer`.  Integer-valued inputs, so that fp32 and float64 agree exactly and ties are common."""
    from jamie_amd import metrics as jm
    assert jm.TILE_I >= 1 and jm.TILE_J >= 1
    rng = np.random.default_rng(N + L)
    A = rng.integers(-3, 4, (N, L)).astype(np.float64)
    B = rng.integers(-3, 4, (N, L)).astype(np.float64)
    value, row, col = mu.reference_loop(A, B)
    trow, tcol = mu.tiled_counts(A, B, jm.TILE_I, jm.TILE_J)
    assert np.array_equal(trow, row) and np.array_equal(tcol, col)
    assert (trow.sum() + tcol.sum()) / (2 * N ** 2) == value
    # and on real-valued data the band of the float64 reference holds the fp32 restatement
    A32, B32 = mu.noisy_pair(N, L, 1.0, seed=N)
    ref = mu.foscttm_band(A32, B32)
    trow, tcol = mu.tiled_counts(A32, B32, jm.TILE_I, jm.TILE_J)
    assert np.all(trow >= ref['lo'][0]) and np.all(trow <= ref['hi'][0])
    assert np.all(tcol >= ref['lo'][1]) and np.all(tcol <= ref['hi'][1])


def test_metrics_keyword_and_host_test_closer(capsys):
    from jamie_amd import JAMIE
    with pytest.raises(ValueError):
        JAMIE(metrics='gpu')
    assert JAMIE().metrics == 'host'
    assert JAMIE(metrics='device').metrics == 'device'
    A, B = mu.noisy_pair(400, 6, 0.8, seed=4)
    e0, e1 = A.astype(np.float64), B.astype(np.float64)
    want = mu.reference_loop(e0, e1)[0]
    got = JAMIE(metrics='host').test_closer([e0, e1])
    assert got == want and 0.05 < got < 0.45
    assert capsys.readouterr().out.strip().splitlines()[-1] == f'foscttm: {want}'
    assert JAMIE().test_closer([e0, e1], distance_metric='cosine') == want        # (the host code ignores the argument)


@pytest.mark.parametrize('k', [1, 5, 6])
def test_host_label_transfer_equals_sklearn(k, capsys):
    from sklearn.neighbors import KNeighborsClassifier
    from jamie_amd import JAMIE
    e0, l0, e1, l1 = mu.labelled_sets()
    want = KNeighborsClassifier(n_neighbors=k).fit(e1, l1).score(e0, l0)
    got = JAMIE().test_LabelTA([e0, e1], [l0, l1], k=k)
    assert got == pytest.approx(want, abs=1e-12) and 0.3 < got < 0.99
    assert capsys.readouterr().out.strip().splitlines()[-1] == f'label transfer accuracy: {got}'
    if k == 5:
        assert JAMIE().test_LabelTA([e0, e1], [l0, l1]) == got                   # k = 5 is the default


def test_vote_rule_predicts_what_sklearn_predicts():
    """Neighbours ordered by (distance, index), majority vote, ties to the lowest class of np.unique: sklearn's
    KNeighborsClassifier(weights='uniform').predict.  The tie rule is exercised: some queries decide on a tied vote."""
    from scipy.spatial.distance import cdist
    from sklearn.neighbors import KNeighborsClassifier
    e0, l0, e1, l1 = mu.labelled_sets()
    d = cdist(e0, e1)
    for k in (1, 5, 6, 30):
        pred, tied = mu.vote_rule(d, l1, k)
        sk = KNeighborsClassifier(n_neighbors=k).fit(e1, l1).predict(e0)
        print(f'k = {k}: agreement {np.mean(pred == sk)}, tied votes {tied.mean():.4f}')
        assert np.array_equal(pred, sk)
        if k > 1:
            assert tied.mean() >= 0.001


def test_metrics_module_refuses_bad_k_without_a_gpu():
    from jamie_amd import metrics as jm
    with pytest.raises(ValueError):
        jm.cross_knn(np.zeros((4, 3)), np.zeros((100, 3)), jm.KNN_MAX + 1)
    with pytest.raises(ValueError):
        jm.cross_knn(np.zeros((4, 3)), np.zeros((3, 3)), 4)
    with pytest.raises(ValueError):
        jm.label_transfer_accuracy(np.zeros((4, 3)), np.zeros(4), np.zeros((9, 3)), np.zeros(9), k=10)


def test_metric_kernels_use_no_scratch():
    """private_segment_fixed_size == 0 for every kernel of csrc/metrics.hip, read from the code object hipcc built."""
    import isa_check as ic
    obj = os.path.join(ROOT, 'jamie_amd', 'csrc', '_obj', 'metrics.o')
    if not os.path.exists(obj):
        pytest.skip('the library is not built')
    if not os.path.exists(ic.OBJDUMP):
        pytest.skip('llvm-objdump not found')
    meta = ic.kernel_metadata(obj)
    names = ' '.join(meta)
    for kernel in ('own_pair_kernel', 'foscttm_kernel', 'knn_partial_kernel', 'knn_merge_kernel', 'knn_vote_kernel'):
        assert kernel in names, (kernel, names)
    for name, m in meta.items():
        assert m['private_segment_fixed_size'] == 0, (name, m)
        assert m.get('vgpr_spill_count', 0) == 0, (name, m)

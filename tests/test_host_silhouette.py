"""Silhouette widths, the parts that need no GPU: the error bound of DESIGN.md §16 on a numpy fp32 restatement of the device
reduction, the workspace arithmetic of the built library, and `JAMIE(metrics='host').test_silhouette` against the definition in
plain loops."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import silhouette_util as su  # noqa: E402


@pytest.fixture(scope='module')
def lib():
    import jamie_amd
    jamie_amd.build_library()
    from jamie_amd import _native
    return _native


@pytest.mark.parametrize('kind', su.KINDS)
@pytest.mark.parametrize('L', su.DIMS)
def test_restated_reduction_within_the_bound(kind, L):
    from sklearn.metrics import silhouette_samples
    X, codes = su.data(kind, 400, L)
    C = len(su.CLASS_SIZES)
    counts = np.bincount(codes, minlength=C)
    ref = su.reference_sums(X, X, codes, C)
    ref_w = su.widths_from_sums(ref, counts, codes)
    sk = silhouette_samples(X.astype(np.float64), codes)
    print(f'float64 reference against sklearn: {np.abs(ref_w - sk).max():.2e}')
    assert np.abs(ref_w - sk).max() <= 1e-10               # (sklearn takes its distances from dot products)
    for seg in (1 << 30, 1):
        S = su.restated_sums(X, X, codes, C, seg_tiles=seg)
        rel = np.abs(S - ref) / np.where(ref > 0, ref, 1.0)
        err = np.abs(su.widths_from_sums(S, counts, codes) - ref_w).max()
        print(f'{kind} L={L} seg_tiles={seg}: max |dS| / S {rel.max():.2e} (gamma {su.gamma(L):.2e}), widths {err:.2e} '
              f'(bound {su.width_bound(L):.2e})')
        assert np.all(np.abs(S - ref) <= su.gamma(L) * ref)
        assert err <= su.width_bound(L)
        assert np.all(S[np.arange(400), codes][counts[codes] == 1] == 0)        # the singleton: only its own zero self-pair


def test_workspace_arithmetic(lib):
    ws = lib.label_sums_workspace
    assert ws(0, 400, 6) == 0 and ws(400, 0, 6) == 0 and ws(400, 400, 0) == 0 and ws(-1, -1, -1) == 0
    assert ws(400, 400, 6, -1) == 0
    assert ws(1, 1, 1) > 0
    for seg in (0, 1, 3, 64):
        sizes = [ws(nq, 100000, 20, seg) for nq in (1, 127, 128, 129, 5000, 100000)]
        assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0, (seg, sizes)
    by_seg = [ws(5000, 100000, 20, seg) for seg in (1024, 64, 8, 2, 1)]         # shorter segments: more of them
    assert all(b >= a for a, b in zip(by_seg, by_seg[1:])) and by_seg[-1] > by_seg[0], by_seg
    # a class per row and one segment per tile is the most the work list can hold: it still fits 2^63
    assert 0 < ws(1 << 20, 1 << 20, 1 << 20, 1) < 1 << 62
    # the library's own choice does not depend on the queries: the partials grow in proportion to Nq
    a, b, c = ws(128, 1 << 20, 40), ws(256, 1 << 20, 40), ws(384, 1 << 20, 40)
    assert b - a == c - b > 0


def test_host_facade_against_the_definition(capsys):
    from jamie_amd import JAMIE
    e0, l0, e1, l1 = su.two_by_three()
    ref = su.silhouette_by_loops([e0, e1], [l0, l1])
    out = JAMIE().test_silhouette([e0, e1], [l0, l1])
    lines = capsys.readouterr().out.strip().splitlines()
    assert lines[-2:] == [f"label ASW: {out['label_asw']}", f"modality ASW: {out['modality_asw']}"]
    assert list(out['labels']) == ['a', 'b', 'c']
    assert set(out) == {'label_asw', 'label_widths', 'modality_asw', 'modality_asw_per_label', 'label_distance', 'labels'}
    np.testing.assert_allclose(out['label_widths'], ref['label_widths'], rtol=0, atol=1e-12)
    assert abs(out['label_asw'] - ref['label_asw']) <= 1e-12
    per = out['modality_asw_per_label']
    assert np.isnan(per[2]) and not np.isnan(per[:2]).any()          # 'c' is in one modality only
    np.testing.assert_allclose(per[:2], ref['modality_asw_per_label'][:2], rtol=0, atol=1e-12)
    assert abs(out['modality_asw'] - per[:2].mean()) <= 1e-15        # ... and is skipped in the mean
    assert abs(out['modality_asw'] - ref['modality_asw']) <= 1e-12
    D = out['label_distance']
    assert D.shape == (3, 3) and np.array_equal(D, D.T)
    np.testing.assert_allclose(D, ref['label_distance'], rtol=1e-12)
    assert np.array_equal(np.argmin(D, axis=1), np.arange(3))        # clusters: a label is nearest to itself
    assert -1 <= out['label_asw'] <= 1 and 0 <= out['modality_asw'] <= 1


def test_host_facade_singleton_modalities():
    """A label with one cell in each modality: both are singletons of their modality, s = 0 and 1 - |s| = 1."""
    from jamie_amd import JAMIE
    rng = np.random.default_rng(0)
    e0, e1 = rng.standard_normal((5, 3)), rng.standard_normal((4, 3))
    out = JAMIE().test_silhouette([e0, e1], [np.array([0, 0, 0, 1, 2]), np.array([0, 0, 1, 3])])
    assert list(out['labels']) == [0, 1, 2, 3]
    assert out['modality_asw_per_label'][1] == 1.0
    assert np.isnan(out['modality_asw_per_label'][2:]).all()


def test_value_errors():
    from jamie_amd import JAMIE
    e0, l0, e1, l1 = su.two_by_three()
    j = JAMIE()
    with pytest.raises(ValueError):
        j.test_silhouette([e0, e1], [l0])                             # a label array per embedding
    with pytest.raises(ValueError):
        j.test_silhouette([e0, e1], [l0, l1[:-1]])                    # a label per cell
    with pytest.raises(ValueError):
        j.test_silhouette([e0, e1], [np.zeros(len(l0)), np.zeros(len(l1))])          # one distinct label
    with pytest.raises(ValueError):
        j.test_silhouette([e0, e1], [np.arange(len(l0)), len(l0) + np.arange(len(l1))])      # N distinct labels
    bad = e0.copy()
    bad[4, 1] = np.nan
    with pytest.raises(ValueError):
        j.test_silhouette([bad, e1], [l0, l1])


def test_library_exports_the_silhouette_entry_points(lib):
    handle = lib.load()
    for name in ('jamie_label_distance_sums', 'jamie_label_sums_workspace', 'jamie_silhouette_widths'):
        assert name in lib.EXPORTS and hasattr(handle, name)

"""Silhouette widths on the device (jamie_amd/metrics.py, csrc/metrics.hip) against float64 references by direct difference.

Bounds (u = 2^-24): every S[i, c] within gamma = (L / 2 + 9) u relative, every silhouette width within
2 gamma / (1 - gamma) absolute.  Every figure is printed before it is asserted."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import silhouette_util as su  # noqa: E402

pytestmark = pytest.mark.gpu

N = 400
C = len(su.CLASS_SIZES)


@pytest.fixture(scope='module')
def jm():
    from jamie_amd import metrics
    return metrics


@pytest.fixture(scope='module')
def nv():
    from jamie_amd import _native
    return _native


def _check_sums(S, ref, L, what):
    rel = np.abs(S - ref) / np.where(ref > 0, ref, 1.0)
    print(f'{what}: max |dS| / S {rel.max():.2e}, gamma {su.gamma(L):.2e}')
    assert np.all(np.abs(S - ref) <= su.gamma(L) * ref)


@pytest.mark.parametrize('L', su.DIMS)
def test_label_distance_sums_vs_float64(jm, L):
    R, codes = su.data('gaussian', N, L)
    spread = np.array([0, 1, 2, 4, 5, 6])[codes]           # code 3 is carried by no row
    Qall = np.random.default_rng(50 + L).standard_normal((300, L)).astype(np.float32)
    ref_all = su.reference_sums(Qall, R, spread, 7)
    for Nq in (1, 127, 128, 129, 300):
        S = jm.class_distance_sums(Qall[:Nq], R, spread, 7)
        assert S.dtype == torch.float64 and S.shape == (Nq, 7) and S.is_cuda
        S = S.cpu().numpy()
        assert np.all(S[:, 3] == 0) and np.all(S[:, [0, 1, 2, 4, 5, 6]] > 0)
        _check_sums(S, ref_all[:Nq], L, f'L={L} Nq={Nq}')
    names = np.array(['t%d' % c for c in codes])
    S, classes, counts = jm.label_distance_sums(Qall, R, names)
    order = np.argsort(['t%d' % c for c in range(C)])      # np.unique sorts the names
    assert list(classes) == ['t%d' % c for c in order] and list(counts) == [su.CLASS_SIZES[c] for c in order]
    _check_sums(S.cpu().numpy(), ref_all[:, [0, 1, 2, 4, 5, 6]][:, order], L, f'L={L} by label')


@pytest.mark.parametrize('L', [3, 32])
def test_segments_and_repeatability(jm, L):
    rng = np.random.default_rng(L)
    R = rng.standard_normal((350, L)).astype(np.float32)
    codes = rng.permutation(np.repeat([0, 1], [300, 50]))
    Q = rng.standard_normal((200, L)).astype(np.float32)
    ref = su.reference_sums(Q, R, codes, 2)
    out = {}
    for seg in (0, 1, 2):
        a = jm.class_distance_sums(Q, R, codes, 2, seg_tiles=seg).cpu().numpy()
        b = jm.class_distance_sums(Q, R, codes, 2, seg_tiles=seg).cpu().numpy()
        assert np.array_equal(a, b)
        _check_sums(a, ref, L, f'L={L} seg_tiles={seg}')
        out[seg] = a
    print(f'seg_tiles 1 against 0: {int((out[1] != out[0]).sum())} of {out[0].size} entries differ in the last bits')
    assert np.array_equal(out[1][:, 1], out[0][:, 1])      # the 50-row class is one tile either way
    with pytest.raises(ValueError):
        jm.class_distance_sums(Q, R, codes, 2, seg_tiles=-1)


def test_query_order_does_not_matter(jm):
    R, codes = su.data('clustered', N, 33)
    rng = np.random.default_rng(4)
    Q = rng.standard_normal((300, 33)).astype(np.float32)
    perm = rng.permutation(300)
    a = jm.class_distance_sums(Q, R, codes, C).cpu().numpy()
    b = jm.class_distance_sums(Q[perm], R, codes, C).cpu().numpy()
    assert np.array_equal(a[perm], b)
    c = jm.class_distance_sums(Q[perm][:77], R, codes, C).cpu().numpy()      # nor the number of queries
    assert np.array_equal(a[perm][:77], c)


@pytest.mark.parametrize('kind', su.KINDS)
@pytest.mark.parametrize('L', su.DIMS)
def test_silhouette_samples_vs_float64(jm, kind, L):
    from sklearn.metrics import silhouette_samples
    X, codes = su.data(kind, N, L)
    counts = np.bincount(codes, minlength=C)
    ref = su.widths_from_sums(su.reference_sums(X, X, codes, C), counts, codes)
    sk = silhouette_samples(X.astype(np.float64), codes)
    got = jm.silhouette_samples(X, codes)
    assert got.dtype == np.float64 and got.shape == (N,)
    print(f'{kind} L={L}: against the float64 reference {np.abs(got - ref).max():.2e}, against sklearn {np.abs(got - sk).max():.2e}, '
          f'bound {su.width_bound(L):.2e}; reference against sklearn {np.abs(ref - sk).max():.2e}')
    assert np.abs(got - ref).max() <= su.width_bound(L)
    assert np.abs(got - sk).max() <= su.width_bound(L)
    assert np.all(got[counts[codes] == 1] == 0)            # the singleton class


def test_silhouette_samples_exact_cases(jm):
    rng = np.random.default_rng(6)
    X = rng.standard_normal((200, 5)).astype(np.float32)
    X[:150] = np.float32(0.37) * X[:150] + np.float32(10.0)
    X[150:] = X[150]                                        # 50 identical cells, apart from the rest
    labels = np.concatenate([np.repeat([0, 1], [100, 49]), [2], np.full(50, 3)])
    perm = rng.permutation(200)
    s = jm.silhouette_samples(X[perm], labels[perm])
    lab = labels[perm]
    assert np.all(s[lab == 3] == 1.0)
    assert np.all(s[lab == 2] == 0.0)
    assert np.all(np.abs(s[lab < 2]) < 1)
    same = np.tile(X[:1], (300, 1))
    assert np.all(jm.silhouette_samples(same, np.arange(300) % 3) == 0.0)


def test_silhouette_samples_chunks_and_errors(jm, nv):
    X, codes = su.data('gaussian', N, 32)
    whole = jm.silhouette_samples(X, codes)
    need = 128 * C * 8 + nv.label_sums_workspace(128, N, C, 0)
    assert 256 * C * 8 + nv.label_sums_workspace(256, N, C, 0) > need          # so `need` admits 128 rows a chunk: 4 chunks
    chunked = jm.silhouette_samples(X, codes, max_workspace=need)
    assert np.array_equal(whole, chunked)
    assert np.array_equal(whole, jm.silhouette_samples(torch.from_numpy(X).cuda(), codes, max_workspace=need + 128 * C * 8))
    with pytest.raises(ValueError, match=str(need)):
        jm.silhouette_samples(X, codes, max_workspace=need - 1)
    with pytest.raises(ValueError):
        jm.silhouette_samples(X, codes[:-1])
    with pytest.raises(ValueError):
        jm.silhouette_samples(X, np.zeros(N))
    with pytest.raises(ValueError):
        jm.silhouette_samples(X, np.arange(N))
    bad = X.copy()
    bad[7, 3] = np.inf
    with pytest.raises(ValueError):
        jm.silhouette_samples(bad, codes)


def test_facade_device_against_host(jm, capsys):
    from jamie_amd import JAMIE
    e0, l0, e1, l1 = su.two_by_three()
    L = e0.shape[1]
    host = JAMIE().test_silhouette([e0, e1], [l0, l1])
    capsys.readouterr()
    dev = JAMIE(metrics='device').test_silhouette([e0, e1], [l0, l1])
    lines = capsys.readouterr().out.strip().splitlines()
    assert lines[-2:] == [f"label ASW: {dev['label_asw']}", f"modality ASW: {dev['modality_asw']}"]
    assert set(dev) == set(host) and list(dev['labels']) == list(host['labels'])
    bound = su.width_bound(L)
    print(f"label widths {np.abs(dev['label_widths'] - host['label_widths']).max():.2e}, label ASW "
          f"{abs(dev['label_asw'] - host['label_asw']):.2e}, modality ASW {abs(dev['modality_asw'] - host['modality_asw']):.2e}, "
          f"bound {bound:.2e}; label distance {np.abs(dev['label_distance'] / host['label_distance'] - 1).max():.2e}, "
          f'gamma {su.gamma(L):.2e}')
    assert np.abs(dev['label_widths'] - host['label_widths']).max() <= bound
    assert abs(dev['label_asw'] - host['label_asw']) <= bound
    assert abs(dev['modality_asw'] - host['modality_asw']) <= bound
    hp, dp = host['modality_asw_per_label'], dev['modality_asw_per_label']
    assert np.array_equal(np.isnan(hp), np.isnan(dp)) and list(np.isnan(dp)) == [False, False, True]
    assert np.abs(dp[:2] - hp[:2]).max() <= bound
    assert np.all(np.abs(dev['label_distance'] - host['label_distance']) <= su.gamma(L) * host['label_distance'])
    # chunks of 128 cells give the same widths, bit for bit
    from jamie_amd import _native as nv
    n = len(e0) + len(e1)
    need = 128 * 6 * 8 + nv.label_sums_workspace(128, n, 6, 0)
    again = jm.silhouette([e0, e1], [l0, l1], max_workspace=need)
    assert np.array_equal(again['label_widths'], dev['label_widths'])
    assert np.array_equal(again['modality_asw_per_label'], dev['modality_asw_per_label'], equal_nan=True)
    with pytest.raises(ValueError):
        JAMIE(metrics='device').test_silhouette([e0, e1], [l0])
    with pytest.raises(ValueError):
        JAMIE(metrics='device').test_silhouette([e0, e1], [l0, l1[:-1]])


def test_abi_argument_errors(nv):
    q = torch.zeros(10, 4, device='cuda')
    r = torch.zeros(100, 4, device='cuda')
    off = torch.tensor([0, 60, 100], dtype=torch.int64, device='cuda')
    S = torch.full((10, 2), -1.0, dtype=torch.float64, device='cuda')
    ws = torch.empty(nv.label_sums_workspace(10, 100, 2, 0), dtype=torch.uint8, device='cuda')

    def call(L=4, n_classes=2, ldS=2, seg=0, ws_bytes=ws.numel(), class_off=off):
        nv._call('jamie_label_distance_sums', nv.ptr(q), 10, nv.ptr(r), 100, L, nv.ptr(class_off), n_classes, nv.ptr(S), ldS, seg,
                 nv.ptr(ws), ws_bytes, nv._stream())

    for bad in (dict(L=0), dict(n_classes=0), dict(ldS=1), dict(seg=-1), dict(ws_bytes=ws.numel() - 1),
                dict(class_off=torch.tensor([0, 60, 99], dtype=torch.int64, device='cuda')),
                dict(class_off=torch.tensor([0, 101, 100], dtype=torch.int64, device='cuda'))):
        with pytest.raises(nv.JamieHipError):
            call(**bad)
    torch.cuda.synchronize()
    assert bool((S == -1.0).all())                         # refused before a launch: nothing was written
    call()
    torch.cuda.synchronize()
    assert bool((S == 0.0).all())                          # (all rows equal: every distance is 0)
    out = torch.empty(10, dtype=torch.float64, device='cuda')
    counts = torch.tensor([60, 40], dtype=torch.int64, device='cuda')
    own = torch.zeros(10, dtype=torch.int32, device='cuda')
    with pytest.raises(nv.JamieHipError):
        nv.silhouette_widths(S, counts, own, None, 0, out)

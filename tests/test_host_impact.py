"""Feature impact without a GPU: the exported symbols, the plan arithmetic, the argument checks of `feature_impact`, of the facade
and of the `_native` wrappers (all raised before anything is launched), the rank-one identity the device route rests on, in
float64, and the new kernels' code objects."""
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import impact_util as fu  # noqa: E402

SYMBOLS = ('jamie_occlusion_rows', 'jamie_impact_accumulate')


def test_symbols_are_declared_and_exported():
    from jamie_amd import _native as nv
    hdr = open(os.path.join(ROOT, 'include', 'jamie_hip.h')).read()
    assert 'Feature impact on the device' in hdr
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    handle = nv.load()
    for name in SYMBOLS:
        assert re.search(r'\b' + name + r'\s*\(', code), name
        assert name in nv.EXPORTS and hasattr(handle, name), name


def _covered(groups):
    return np.concatenate([np.arange(a, a + b) for a, b in groups])


def test_plan_arithmetic():
    from jamie_amd import impact as fi
    G = fi.GROUP
    assert G == 8 and fi.ROW_BLOCK == 512
    # everything fits: one chunk, one group
    p = fi.plan(300, 24, 16, 24)
    assert (p['n'], p['g'], p['chunks'], p['groups']) == (300, 24, [(0, 300)], [(0, 24)])
    assert p['rows'] == 300 * 24 and p['workspace'] == p['rows'] * 4 * 48
    # config 2: the chunk is capped, the group takes what the cap leaves
    p = fi.plan(100000, 2000, 2000, 2000)
    assert p['n'] == fi.CELL_CHUNK and p['g'] == (1 << 30) // 16000 // fi.CELL_CHUNK == 8
    assert p['workspace'] <= 1 << 30 and len(p['chunks']) == -(-100000 // fi.CELL_CHUNK) and p['chunks'][-1][1] == 100000 % fi.CELL_CHUNK
    for N, di, dt, F, cap in ((300, 24, 16, 24, 4 * 48 * 450), (300, 16, 24, 16, 4 * 48 * 450), (300, 13, 10, 13, 4 * 32 * 450),
                              (7, 5, 3, 5, 4 * 10 * 3), (1000, 40, 8, 3, 4 * 80 * 999), (5, 4, 4, 4, 4 * 8), (100000, 2000, 1500, 2000, 1 << 30),
                              (8, 3, 3, 100000, 1 << 40)):
        p = fi.plan(N, di, dt, F, cap)
        row = 4 * 2 * max(di, dt)
        assert 1 <= p['n'] <= N and 1 <= p['g'] <= min(F, fi.MAX_GROUP)
        assert p['rows'] == p['g'] * p['n'] and p['rows'] * row == p['workspace'] <= cap, (N, di, dt, F, cap, p)
        assert np.array_equal(_covered(p['groups']), np.arange(F)), p['groups']          # every feature once, in order
        assert np.array_equal(_covered(p['chunks']), np.arange(N)), p['chunks']
        assert all(1 <= b <= p['g'] for _, b in p['groups']) and all(1 <= b <= p['n'] for _, b in p['chunks'])
    # a cap of 450 rows: 8 features beside each other, several ragged chunks
    p = fi.plan(300, 24, 16, 13, 4 * 48 * 450)
    assert (p['n'], p['g']) == (56, 8) and p['groups'] == [(0, 8), (8, 5)] and len(p['chunks']) == 6 and p['chunks'][-1] == (280, 20)
    # one feature of one cell
    assert fi.plan(5, 4, 4, 4, 4 * 8)['rows'] == 1
    with pytest.raises(ValueError, match='max_workspace'):
        fi.plan(5, 4, 4, 4, 4 * 8 - 1)
    for bad in ((0, 4, 4, 4), (5, 0, 4, 4), (5, 4, 0, 4), (5, 4, 4, 0)):
        with pytest.raises(ValueError):
            fi.plan(*bad)


def test_workspace_arithmetic():
    from jamie_amd import _native as nv
    assert nv.occlusion_workspace(3, 6) == 4 * 3 * 8 and nv.occlusion_workspace(7, 48) == 4 * 7 * 48
    assert nv.impact_accumulate_workspace(1, 10, 5) == 8 * 5 * 10 and nv.impact_accumulate_workspace(4097, 130, 5) == 8 * 5 * 130 * 9
    assert nv.impact_accumulate_workspace(512, 1, 1) == 8 and nv.impact_accumulate_workspace(513, 1, 1) == 16


class _FakeModel:
    """Has what feature_impact asks of a model and fails the test if any of it is called: the checks come first."""
    input_dim = [6, 4]
    pdims = [8, 8]
    p = bn = {}
    device = 'cuda'

    def _boom(self, *a, **k):
        raise AssertionError('the model was called before the arguments were checked')
    _linear = _lin_bn_act = _encode_eval = _mu_eval = _decode_eval = eval = _boom


def test_feature_impact_checks_its_arguments_before_the_gpu():
    from jamie_amd import impact as fi
    m = _FakeModel()
    X = np.zeros((5, 6), np.float32)
    nan = X.copy()
    nan[2, 3] = np.nan
    for bad, match in ((dict(X=X[0]), '2-D'), (dict(X=X[:, :5]), '6 features'), (dict(X=X[:0]), '>= 1 cell'), (dict(X=nan), 'NaN'),
                       (dict(X=torch.from_numpy(nan)), 'NaN'), (dict(X=np.zeros((5, 6, 1))), '2-D'),
                       (dict(background=np.zeros(5)), 'background'), (dict(background=np.zeros((1, 6))), 'background'),
                       (dict(background=np.full(6, np.inf)), 'background'),
                       (dict(measured=np.zeros((5, 6))), 'measured'), (dict(measured=np.zeros((4, 4))), 'measured'),
                       (dict(measured=np.full((5, 4), np.nan)), 'measured'),
                       (dict(features=[0, 6]), r'\[0, 6\)'), (dict(features=[-1]), r'\[0, 6\)'), (dict(features=[]), 'non-empty'),
                       (dict(features=[0.5]), 'integers'), (dict(features=[[0, 1]]), '1-D'),
                       (dict(from_modality=2), 'modalities'), (dict(to_modality=-1), 'modalities'),
                       (dict(max_workspace=63), 'max_workspace')):
        a = dict(model=m, X=X, from_modality=0, to_modality=1)
        a.update(bad)
        with pytest.raises(ValueError, match=match):
            fi.feature_impact(**a)
    with pytest.raises(ValueError, match='edModelVar'):
        fi.feature_impact(object(), X, 0, 1)
    # what passes the checks: the features as given (unsorted, a repeat), the plan on the padded widths
    i, t, N, feat, p = fi.check_arguments(m, X, 0, 1, features=[5, 2, 5], max_workspace=64 * 7)
    assert (i, t, N) == (0, 1, 5) and feat.dtype == np.int32 and list(feat) == [5, 2, 5] and p['rows'] <= 7
    assert list(fi.check_arguments(m, X[:, :4], 1, 0)[3]) == [0, 1, 2, 3]


def test_facade_checks_its_arguments_before_the_gpu():
    import scipy.sparse as sp
    from jamie_amd import JAMIE
    from jamie_amd.utilities import preclass
    rng = np.random.default_rng(0)
    data = [rng.standard_normal((20, 6)), rng.standard_normal((20, 4))]
    m = _FakeModel()
    pre = [preclass(d, axis=0) for d in data]
    m.preprocessing = [q.transform for q in pre]
    m.preprocessing_inverse = [q.inverse_transform for q in pre]
    jm = JAMIE()
    jm.model, jm.dataset_num = m, 2
    for bad, match in ((dict(data=data[0][:, :5]), 'features'), (dict(data=data[0][0]), '2-D'), (dict(background=np.zeros(5)), 'background'),
                       (dict(measured=data[1][:19]), 'measured'), (dict(features=[6]), r'\[0, 6\)'), (dict(modality=2), 'modalities'),
                       (dict(to_modality=5), 'modalities'), (dict(max_workspace=10), 'max_workspace'),
                       (dict(data=sp.csr_matrix(data[0]), features=[7]), r'\[0, 6\)'),
                       (dict(data=sp.csr_matrix(data[0]), measured=data[1][:3]), 'measured')):
        a = dict(data=data[0], modality=0)
        a.update(bad)
        with pytest.raises(ValueError, match=match):
            jm.feature_impact(**a)
    # a PCA'd modality (global scaling after a PCA: axis None) has no data-unit features
    class _Pca:
        def transform(self, X):
            return X[:, :3]
    m.preprocessing = [preclass(data[0][:, :3], pca=_Pca()).transform, pre[1].transform]
    with pytest.raises(ValueError, match='pre_transformed=True'):
        jm.feature_impact(data[0], 0)


def test_native_wrappers_check_their_arguments():
    """Wrong dtypes, strides, sizes, feature indices and short workspaces are refused before anything is launched (CPU tensors
    stand in), by the wrappers and by the library itself."""
    from jamie_amd import _native as nv
    E = nv.JamieHipError
    n, h, d, g = 5, 8, 4, 3
    base = dict(H=torch.zeros(n, h), X=torch.zeros(n, d), bg=torch.zeros(d), W0=torch.zeros(h, d + 2)[:, :d], feat=[3, 0, 3],
                bn=tuple(torch.ones(h) for _ in range(4)), out=torch.zeros(g * n, h),
                ws=torch.zeros(nv.occlusion_workspace(g, h), dtype=torch.uint8))
    for bad, match in ((dict(H=base['H'].double()), 'float32'), (dict(H=torch.zeros(h, n).t()), 'unit column stride'),
                       (dict(X=torch.zeros(n + 1, d)), 'rows'), (dict(out=torch.zeros(g * n - 1, h)), 'rows'),
                       (dict(W0=torch.zeros(h - 1, d)), 'rows'), (dict(bg=torch.zeros(d - 1)), 'bg'),
                       (dict(bn=tuple(torch.ones(h - 1) for _ in range(4))), 'BatchNorm'),
                       (dict(ws=torch.zeros(nv.occlusion_workspace(g, h) - 1, dtype=torch.uint8)), 'needed'),
                       (dict(feat_dev=torch.zeros(g, dtype=torch.int64)), 'feat_dev')):
        a = dict(base)
        a.update(bad)
        with pytest.raises(E, match=match):
            nv.occlusion_rows(**a)
    for feat in ([4], [-1, 0], [], [1.5]):
        with pytest.raises(ValueError):
            nv.occlusion_rows(**dict(base, feat=feat))
    acc = dict(Y=torch.zeros(g * n, 6), R=torch.zeros(n, 6), acc=torch.zeros(g, 6, dtype=torch.float64),
               ws=torch.zeros(nv.impact_accumulate_workspace(n, 6, g), dtype=torch.uint8))
    for bad, match in ((dict(acc=torch.zeros(g, 6)), 'float64'), (dict(acc=torch.zeros(g, 5, dtype=torch.float64)), 'float64'),
                       (dict(Y=torch.zeros(g * n + 1, 6)), 'rows'), (dict(Y=torch.zeros(g * n, 5)), 'leading dimension'),
                       (dict(R=torch.zeros(n, 6).double()), 'float32'),
                       (dict(ws=torch.zeros(8 * g * 6 - 1, dtype=torch.uint8)), 'needed')):
        a = dict(acc)
        a.update(bad)
        with pytest.raises(E, match=match):
            nv.impact_accumulate(**a)
    # the library's own checks launch nothing either: non-positive sizes, a feature out of range, a short workspace
    lib = nv.load()
    f32 = np.zeros(256, np.float32)
    p = f32.ctypes.data
    ok = np.array([3, 0, 3], np.int32)

    def occ(n=n, h=h, g=g, feat=ok, ws_bytes=4 * g * h):
        return lib.jamie_occlusion_rows(p, h, p, d, p, p, d, p, feat.ctypes.data, n, h, d, g, p, p, p, p, 1e-5, 0.01, p, h, p, ws_bytes, None)
    for kw, msg in ((dict(n=0), b'positive'), (dict(h=0), b'positive'), (dict(g=0), b'positive'), (dict(g=-2), b'positive'),
                    (dict(feat=np.array([3, 4, 0], np.int32)), b'feature index'), (dict(feat=np.array([0, -1, 0], np.int32)), b'feature index'),
                    (dict(ws_bytes=4 * g * h - 1), b'workspace')):
        assert occ(**kw) == -1 and msg in lib.jamie_last_error(), (kw, lib.jamie_last_error())
    f64 = np.zeros(64)
    for (n_, dt_, g_, wsb), msg in (((0, 6, 3, 1024), b'positive'), ((5, 0, 3, 1024), b'positive'), ((5, 6, 0, 1024), b'positive'),
                                    ((5, 6, 3, 8 * 18 - 1), b'workspace')):
        assert lib.jamie_impact_accumulate(p, 6, p, 6, n_, dt_, g_, f64.ctypes.data, f64.ctypes.data, wsb, None) == -1
        assert msg in lib.jamie_last_error()
    assert lib.jamie_impact_accumulate(p, 5, p, 6, 5, 6, 3, f64.ctypes.data, f64.ctypes.data, 1024, None) == -1


def test_rank_one_identity_in_float64():
    """Replacing feature f of a cell by bg[f] changes W0 x + b by (bg[f] - x[f]) W0[:, f]: the imputation through the rank-one route
    equals recomputation with the column replaced to 1e-12 relative, for both directions and every feature."""
    from oracle import jamie_oracle as orc
    torch.manual_seed(5)
    dims, L = (24, 16), 8
    P, Bf = orc.init_state(dims, L)
    sd = {k: v.detach() for k, v in P.items()}
    sd.update(Bf)
    W = fu.weights64(fu.randomise_bn_state(sd, 1))
    rng = np.random.default_rng(2)
    for i, t in ((0, 1), (1, 0)):
        X = rng.standard_normal((40, dims[i]))
        bg = 0.5 * rng.standard_normal(dims[i])
        H = fu.pre0(W, i, X)
        for f in range(dims[i]):
            a = fu.occluded_by_rank_one(W, X, i, t, f, bg, H)
            b = fu.occluded_by_replacement(W, X, i, t, f, bg)
            assert a.shape == (40, dims[t]) and np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), (i, t, f)
        assert np.abs(fu.occluded_by_replacement(W, X, i, t, 3, bg) - fu.impute64(W, X, i, t)).max() > 1e-3      # (it is no identity map)
    # and the definition's reference: impact of a feature whose background equals its value everywhere is exactly 0
    X = rng.standard_normal((10, 24))
    X[:, 7] = 0.25
    bg = np.full(24, 0.25)
    per, base = fu.reference(W, X, 0, 1, bg, [7, 2])
    assert base is None and np.all(per[0] == 0) and per[1].max() > 0
    per, base = fu.reference(W, X, 0, 1, bg, [7], measured=np.zeros((10, 16)))
    assert np.allclose(per[0], base, rtol=0, atol=0)


def test_impact_kernels_use_no_scratch():
    """private_segment_fixed_size == 0 for every kernel of csrc/impact.hip, read from the code object hipcc built: the OCC_G
    columns of W0 a lane holds stay in registers."""
    import isa_check as ic
    obj = os.path.join(ROOT, 'jamie_amd', 'csrc', '_obj', 'impact.o')
    if not os.path.exists(obj):
        pytest.skip('the library is not built')
    if not os.path.exists(ic.OBJDUMP):
        pytest.skip('llvm-objdump not found')
    meta = ic.kernel_metadata(obj)
    names = ' '.join(meta)
    for kernel in ('occlusion_stage_kernel', 'occlusion_rows_kernel', 'impact_partial_kernel', 'impact_finish_kernel'):
        assert kernel in names, (kernel, names)
    assert len(meta) == 5                                      # occlusion_rows_kernel: the 16-byte and the any-width form
    for name, m in meta.items():
        assert m['private_segment_fixed_size'] == 0, (name, m)
        assert m.get('vgpr_spill_count', 0) == 0, (name, m)

"""Shapley attributions without a GPU: the exported symbols, the plan arithmetic, the argument checks of `shapley_values`, of the
facade and of the `_native` wrappers (all raised before anything is launched), the float64 references of shapley_util.py on an
additive function, and the new kernels' code objects."""
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import shapley_util as su  # noqa: E402

SYMBOLS = ('jamie_shapley_walk_rows', 'jamie_shapley_accumulate', 'jamie_shapley_summarise')


def test_symbols_are_declared_and_exported():
    from jamie_amd import _native as nv
    hdr = open(os.path.join(ROOT, 'include', 'jamie_hip.h')).read()
    assert 'Shapley attributions on the device' in hdr
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    handle = nv.load()
    for name in SYMBOLS:
        assert re.search(r'\b' + name + r'\s*\(', code), name
        assert name in nv.EXPORTS and hasattr(handle, name), name


def _covered(groups):
    return np.concatenate([np.arange(a, a + b) for a, b in groups])


def test_plan_arithmetic():
    from jamie_amd import shapley as sh
    assert sh.GROUP == 8 and sh.CELL_CHUNK == 8192
    # everything fits: one chunk, one segment
    p = sh.plan(300, 24, 16, 24, 16)
    assert (p['n'], p['g'], p['chunks'], p['segments']) == (300, 24, [(0, 300)], [(0, 24)])
    assert p['rows'] == 300 * 25 and p['workspace'] == p['rows'] * 4 * 48 and p['accumulator'] == 8 * 300 * 24 * 16
    # config 2, all 2000 players towards 8 targets: the chunk shrinks until 8 steps and the incoming row fit the workspace
    p = sh.plan(100000, 2000, 1000, 2000, 8)
    rows = (1 << 30) // 16000
    assert p['n'] == rows // 9 == 7456 and p['g'] == 8 and p['workspace'] <= 1 << 30 and p['accumulator'] <= 1 << 30
    # config 2, 256 players towards all 1000 targets: the accumulator cap bounds the chunk
    p = sh.plan(8192, 2000, 1000, 256, 1000)
    assert p['n'] == (1 << 30) // (8 * 256 * 1000) == 524 and p['g'] == rows // 524 - 1 == 127
    assert len(p['chunks']) == -(-8192 // 524) and p['chunks'][-1][1] == 8192 % 524 and p['segments'][-1] == (254, 2)
    for N, di, dt, F, T, cap, acc in ((300, 24, 16, 24, 16, 4 * 48 * 510, 1 << 30), (300, 16, 16, 13, 10, 4 * 32 * 510, 1 << 30),
                                      (300, 24, 16, 24, 16, 1 << 30, 8 * 24 * 16 * 56), (7, 5, 3, 5, 2, 4 * 10 * 4, 8 * 10 * 3),
                                      (1000, 40, 8, 3, 8, 4 * 80 * 999, 1 << 20), (5, 4, 4, 4, 4, 4 * 8 * 2, 8 * 16),
                                      (100000, 2000, 1500, 2000, 1500, 1 << 30, 1 << 30), (8, 3, 3, 3, 3, 1 << 40, 1 << 40),
                                      (20000, 6, 6, 6, 1, 1 << 40, 1 << 40)):
        p = sh.plan(N, di, dt, F, T, cap, acc)
        row = 4 * 2 * max(di, dt)
        assert 1 <= p['n'] <= min(N, sh.CELL_CHUNK) and 1 <= p['g'] <= min(F, sh.MAX_SEGMENT), (N, di, dt, F, T, cap, acc, p)
        assert p['rows'] == (p['g'] + 1) * p['n'] and p['rows'] * row == p['workspace'] <= cap, (N, di, dt, F, T, cap, acc, p)
        assert p['accumulator'] == 8 * p['n'] * F * T <= acc, (N, di, dt, F, T, cap, acc, p)
        assert np.array_equal(_covered(p['segments']), np.arange(F)), p['segments']      # every step once, in order
        assert np.array_equal(_covered(p['chunks']), np.arange(N)), p['chunks']          # every cell once, in order
        assert all(1 <= b <= p['g'] for _, b in p['segments']) and all(1 <= b <= p['n'] for _, b in p['chunks'])
    # a workspace of 510 rows: 8 steps and the incoming row beside each other, ragged chunks; 13 players: a ragged last segment
    p = sh.plan(300, 16, 16, 13, 10, 4 * 32 * 510)
    assert (p['n'], p['g']) == (56, 8) and p['segments'] == [(0, 8), (8, 5)] and len(p['chunks']) == 6 and p['chunks'][-1] == (280, 20)
    # the accumulator cap alone: 56-cell chunks, and a workspace that leaves segments of 10, 10 and 4
    p = sh.plan(300, 24, 16, 24, 16, 4 * 48 * 56 * 11, 8 * 24 * 16 * 56 + 100)
    assert (p['n'], p['g']) == (56, 10) and p['segments'] == [(0, 10), (10, 10), (20, 4)] and p['chunks'][-1] == (280, 20)
    # one step of one cell
    p = sh.plan(5, 4, 4, 4, 4, 4 * 8 * 2, 8 * 16)
    assert (p['n'], p['g'], p['rows']) == (1, 1, 2)
    with pytest.raises(ValueError, match='max_workspace'):
        sh.plan(5, 4, 4, 4, 4, 4 * 8 * 2 - 1, 8 * 16)
    with pytest.raises(ValueError, match='max_accumulator'):
        sh.plan(5, 4, 4, 4, 4, 4 * 8 * 2, 8 * 16 - 1)
    for bad in ((0, 4, 4, 4, 4), (5, 0, 4, 4, 4), (5, 4, 0, 4, 4), (5, 4, 4, 0, 4), (5, 4, 4, 4, 0)):
        with pytest.raises(ValueError):
            sh.plan(*bad)


def test_workspace_arithmetic_and_orders():
    from jamie_amd import _native as nv
    from jamie_amd import shapley as sh
    assert nv.shapley_walk_workspace(3, 6) == 4 * 3 * 8 and nv.shapley_walk_workspace(17, 48) == 4 * 17 * 48
    assert nv.shapley_summarise_workspace(1, 10) == 160 and nv.shapley_summarise_workspace(4097, 130) == 16 * 130 * 9
    assert nv.shapley_summarise_workspace(512, 1) == 16 and nv.shapley_summarise_workspace(513, 1) == 32 and nv.SHAPLEY_ROWS == 512
    o = sh.draw_orders(7, 3, antithetic=True, seed=5)
    assert o.shape == (6, 7) and o.dtype == np.int32 and np.array_equal(o[1::2], o[0::2, ::-1])
    assert np.array_equal(np.sort(o, axis=1), np.broadcast_to(np.arange(7), (6, 7)))
    assert np.array_equal(o, sh.draw_orders(7, 3, True, 5)) and not np.array_equal(o, sh.draw_orders(7, 3, True, 6))
    assert np.array_equal(sh.draw_orders(7, 3, antithetic=False, seed=5), o[0::2])       # the same draws, without the reverses
    for bad in ((0, 3), (7, 0)):
        with pytest.raises(ValueError):
            sh.draw_orders(*bad)


class _FakeModel:
    """Has what shapley_values asks of a model and fails the test if any of it is called: the checks come first."""
    input_dim = [6, 4]
    pdims = [8, 8]
    p = bn = {}
    device = 'cuda'

    def _boom(self, *a, **k):
        raise AssertionError('the model was called before the arguments were checked')
    _linear = _lin_bn_act = _encode_eval = _mu_eval = _decode_eval = eval = _boom


@pytest.fixture
def no_gpu(monkeypatch):
    """The GPU entry fails: every refusal below is raised before it."""
    from jamie_amd import _native as nv

    def boom(*a, **k):
        raise AssertionError('the GPU was touched before the arguments were checked')
    monkeypatch.setattr(nv, 'require_gpu', boom)
    monkeypatch.setattr(nv, '_call', boom)


def test_shapley_values_checks_its_arguments_before_the_gpu(no_gpu, monkeypatch):
    from jamie_amd import shapley as sh
    m = _FakeModel()
    X = np.zeros((5, 6), np.float32)
    nan = X.copy()
    nan[2, 3] = np.nan
    o6, o3 = sh.draw_orders(6, 2), sh.draw_orders(3, 2)
    rep = o3.copy()
    rep[1, 0] = rep[1, 1]
    for bad, match in ((dict(X=X[0]), '2-D'), (dict(X=X[:, :5]), '6 features'), (dict(X=X[:0]), '>= 1 cell'), (dict(X=nan), 'NaN'),
                       (dict(X=torch.from_numpy(nan)), 'NaN'), (dict(X=np.zeros((5, 6, 1))), '2-D'),
                       (dict(background=np.zeros(5)), 'background'), (dict(background=np.zeros((1, 6))), 'background'),
                       (dict(background=np.full(6, np.inf)), 'background'),
                       (dict(features=[0, 6]), r'\[0, 6\)'), (dict(features=[-1]), r'\[0, 6\)'), (dict(features=[]), 'non-empty'),
                       (dict(features=[0.5]), 'integers'), (dict(features=[[0, 1]]), '1-D'),
                       (dict(features=[5, 2, 5], orders=o3), 'distinct'),
                       (dict(targets=[0, 4]), r'\[0, 4\)'), (dict(targets=[-1]), r'\[0, 4\)'), (dict(targets=[]), 'non-empty'),
                       (dict(targets=[1, 3, 1]), 'distinct'), (dict(targets=[1.0]), 'integers'),
                       (dict(orders=None), 'orders'), (dict(orders=o3), r'\[P >= 1, 6\]'), (dict(orders=o6[0]), r'\[P >= 1, 6\]'),
                       (dict(orders=o6[:0]), r'\[P >= 1, 6\]'), (dict(orders=o6.astype(np.float64)), r'\[P >= 1, 6\]'),
                       (dict(features=[5, 2, 4], orders=rep), 'permutation'), (dict(features=[5, 2, 4], orders=o3 + 1), 'permutation'),
                       (dict(from_modality=2), 'modalities'), (dict(to_modality=-1), 'modalities'),
                       (dict(max_workspace=127), 'max_workspace'), (dict(max_accumulator=8 * 6 * 4 - 1), 'max_accumulator')):
        a = dict(model=m, X=X, from_modality=0, to_modality=1, orders=o6)
        a.update(bad)
        with pytest.raises(ValueError, match=match):
            sh.shapley_values(**a)
    with pytest.raises(ValueError, match='edModelVar'):
        sh.shapley_values(object(), X, 0, 1, orders=o6)
    assert sh.MAX_HOST_VALUES == 1 << 32
    monkeypatch.setattr(sh, 'MAX_HOST_VALUES', 8 * 5 * 6 * 4 - 1)                        # one byte less than values [5, 6, 4] float64
    with pytest.raises(ValueError, match='return_values'):
        sh.shapley_values(m, X, 0, 1, orders=o6, return_values=True)
    monkeypatch.undo()
    # what passes the checks: players and targets as given (unsorted), the orders as int32, the plan on the padded widths
    i, t, N, feat, tcol, orders, p = sh.check_arguments(m, X, 0, 1, features=[5, 2, 4], targets=[3, 0], orders=o3.astype(np.int64),
                                                        max_workspace=64 * 9, max_accumulator=8 * 6 * 2)
    assert (i, t, N) == (0, 1, 5) and feat.dtype == tcol.dtype == orders.dtype == np.int32
    assert list(feat) == [5, 2, 4] and list(tcol) == [3, 0] and np.array_equal(orders, o3) and p['rows'] == 8 and (p['n'], p['g']) == (2, 3)
    assert sh.check_arguments(m, X[:, :4], 1, 0, orders=sh.draw_orders(4, 1))[4] is None


def test_facade_checks_its_arguments_before_the_gpu(no_gpu):
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
                       (dict(features=[6]), r'\[0, 6\)'), (dict(features=[1, 1]), 'distinct'), (dict(targets=[4]), r'\[0, 4\)'),
                       (dict(targets=[2, 2]), 'distinct'), (dict(modality=2), 'modalities'), (dict(to_modality=5), 'modalities'),
                       (dict(max_workspace=10), 'max_workspace'), (dict(max_accumulator=10), 'max_accumulator'),
                       (dict(n_permutations=0), 'permutation'), (dict(orders=np.zeros((2, 6), np.int32)), 'permutation'),
                       (dict(orders=np.arange(5)[None]), r'\[P >= 1, 6\]'),
                       (dict(data=sp.csr_matrix(data[0]), features=[7]), r'\[0, 6\)'),
                       (dict(data=sp.csr_matrix(data[0]), targets=[0, 0]), 'distinct')):
        a = dict(data=data[0], modality=0)
        a.update(bad)
        with pytest.raises(ValueError, match=match):
            jm.shapley_values(**a)
    # a PCA'd modality (global scaling after a PCA: axis None) has no data-unit features
    class _Pca:
        def transform(self, X):
            return X[:, :3]
    m.preprocessing = [preclass(data[0][:, :3], pca=_Pca()).transform, pre[1].transform]
    with pytest.raises(ValueError, match='pre_transformed=True'):
        jm.shapley_values(data[0], 0)


def test_native_wrappers_check_their_arguments(no_gpu):
    """Wrong dtypes, strides, sizes, indices and short workspaces are refused before anything is launched (CPU tensors stand in), by
    the wrappers and by the library itself."""
    from jamie_amd import _native as nv
    E = nv.JamieHipError
    n, h, d, g = 5, 8, 4, 3
    base = dict(state=torch.zeros(n, h), X=torch.zeros(n, d), bg=torch.zeros(d), W0=torch.zeros(h, d + 2)[:, :d], feat=[3, 0, 2],
                bn=tuple(torch.ones(h) for _ in range(4)), out=torch.zeros((g + 1) * n, h),
                ws=torch.zeros(nv.shapley_walk_workspace(g, h), dtype=torch.uint8))
    for bad, match in ((dict(state=base['state'].double()), 'float32'), (dict(state=torch.zeros(h, n).t()), 'unit column stride'),
                       (dict(X=torch.zeros(n + 1, d)), 'rows'), (dict(out=torch.zeros(g * n, h)), 'rows'),
                       (dict(W0=torch.zeros(h - 1, d)), 'rows'), (dict(bg=torch.zeros(d - 1)), 'bg'),
                       (dict(bn=tuple(torch.ones(h - 1) for _ in range(4))), 'BatchNorm'), (dict(bn=base['bn'][:3]), 'bn ='),
                       (dict(ws=torch.zeros(nv.shapley_walk_workspace(g, h) - 1, dtype=torch.uint8)), 'needed'),
                       (dict(feat_dev=torch.zeros(g, dtype=torch.int64)), 'feat_dev')):
        a = dict(base)
        a.update(bad)
        with pytest.raises(E, match=match):
            nv.shapley_walk_rows(**a)
    for feat in ([4], [-1, 0], [], [1.5]):
        with pytest.raises(ValueError):
            nv.shapley_walk_rows(**dict(base, feat=feat))
    F, T, dt = 6, 3, 7
    acc = dict(Y=torch.zeros((g + 1) * n, dt), pos=[4, 0, 5], phi=torch.zeros(n, F, T, dtype=torch.float64), tcol=[6, 0, 2])
    for bad, match in ((dict(phi=torch.zeros(n, F, T)), 'float64'), (dict(phi=torch.zeros(n, F * T, dtype=torch.float64)), 'float64'),
                       (dict(phi=torch.zeros(n, T, F, dtype=torch.float64).transpose(1, 2)), 'float64'),
                       (dict(Y=torch.zeros(g * n, dt)), 'rows'), (dict(Y=torch.zeros((g + 1) * n, dt).double()), 'float32'),
                       (dict(Y=torch.zeros((g + 1) * n, dt - 1), dt=dt), 'leading dimension'), (dict(tcol=None), 'target columns'),
                       (dict(tcol=[6, 0]), 'target columns'), (dict(pos_dev=torch.zeros(g, dtype=torch.int64)), 'pos_dev'),
                       (dict(tcol_dev=torch.zeros(T + 1, dtype=torch.int32)), 'tcol_dev')):
        a = dict(acc)
        a.update(bad)
        with pytest.raises(E, match=match):
            nv.shapley_accumulate(**a)
    for bad in (dict(pos=[4, 0, 4]), dict(pos=[4, 0, 6]), dict(pos=[-1, 0, 1]), dict(tcol=[6, 0, 6]), dict(tcol=[7, 0, 1]), dict(pos=[])):
        with pytest.raises(ValueError):
            nv.shapley_accumulate(**dict(acc, **bad))
    sm = dict(phi=torch.zeros(n, F, T, dtype=torch.float64), sum_abs=torch.zeros(F, T, dtype=torch.float64),
              total=torch.zeros(F, T, dtype=torch.float64), ws=torch.zeros(nv.shapley_summarise_workspace(n, F * T), dtype=torch.uint8))
    for bad, match in ((dict(phi=torch.zeros(n, F, T)), 'float64'), (dict(phi=torch.zeros(F * T, dtype=torch.float64)), 'float64'),
                       (dict(sum_abs=torch.zeros(F, T)), 'sum_abs'), (dict(total=torch.zeros(F, T + 1, dtype=torch.float64)), 'total'),
                       (dict(ws=torch.zeros(16 * F * T - 1, dtype=torch.uint8)), 'needed')):
        a = dict(sm)
        a.update(bad)
        with pytest.raises(E, match=match):
            nv.shapley_summarise(**a)


def test_library_entry_points_refuse_bad_arguments():
    """The library's own checks launch nothing: non-positive sizes, a feature out of range, a repeated or out-of-range position, an
    out-of-range or repeated target column, a short workspace -- each returns -1 with a message."""
    from jamie_amd import _native as nv
    lib = nv.load()
    n, h, d, g = 5, 8, 4, 3
    f32 = np.zeros(256, np.float32)
    p = f32.ctypes.data
    ok = np.array([3, 0, 2], np.int32)

    def walk(n=n, h=h, g=g, feat=ok, ws_bytes=4 * g * h):
        return lib.jamie_shapley_walk_rows(p, h, p, d, p, p, d, p, feat.ctypes.data, n, h, d, g, p, p, p, p, 1e-5, 0.01, p, h, p, ws_bytes,
                                           None)
    for kw, msg in ((dict(n=0), b'positive'), (dict(h=0), b'positive'), (dict(g=0), b'positive'), (dict(g=-2), b'positive'),
                    (dict(feat=np.array([3, 4, 0], np.int32)), b'feature index'), (dict(feat=np.array([0, -1, 0], np.int32)), b'feature index'),
                    (dict(ws_bytes=4 * g * h - 1), b'workspace')):
        assert walk(**kw) == -1 and msg in lib.jamie_last_error(), (kw, lib.jamie_last_error())
    f64 = np.zeros(256)
    q = f64.ctypes.data
    F, T, dt = 6, 3, 7
    pos, tc = np.array([4, 0, 5], np.int32), np.array([6, 0, 2], np.int32)

    def acc(n=n, g=g, pos=pos, tcol=tc, T=T, F=F, ldy=dt):
        th = None if tcol is None else tcol.ctypes.data
        return lib.jamie_shapley_accumulate(p, ldy, n, dt, g, pos.ctypes.data, pos.ctypes.data, F, th, th, T, q, None)
    for kw, msg in ((dict(n=0), b'positive'), (dict(g=0), b'positive'), (dict(T=0), b'positive'), (dict(F=0), b'positive'),
                    (dict(pos=np.array([4, 0, 4], np.int32)), b'pos'), (dict(pos=np.array([4, 6, 0], np.int32)), b'pos'),
                    (dict(pos=np.array([-1, 2, 0], np.int32)), b'pos'), (dict(tcol=np.array([6, 7, 2], np.int32)), b'tcol'),
                    (dict(tcol=np.array([2, 0, 2], np.int32)), b'tcol'), (dict(tcol=None), b'T must be dt'), (dict(ldy=dt - 1), b'ldy')):
        assert acc(**kw) == -1 and msg in lib.jamie_last_error(), (kw, lib.jamie_last_error())
    for (n_, e_, wsb), msg in (((0, 18, 1024), b'positive'), ((5, 0, 1024), b'positive'), ((5, 18, 16 * 18 - 1), b'workspace'),
                               ((513, 18, 16 * 18 * 2 - 1), b'workspace')):
        assert lib.jamie_shapley_summarise(q, n_, e_, q, q, q, wsb, None) == -1 and msg in lib.jamie_last_error(), (n_, e_, wsb)


def _additive_case(seed, N=7, d=9, F=5, T=3):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((d, T))
    X, bg = rng.standard_normal((N, d)), rng.standard_normal(d)
    feat = rng.permutation(d)[:F]
    return A, X, bg, feat, (lambda Xm: Xm @ A)


def test_references_on_an_additive_function():
    """f(x) = a . x: the exact Shapley value of player k is a_k (x_k - bg_k); the float64 walk over all 120 orders of 5 players
    equals the enumeration; the contributions of one order sum to v(all) - v(none).  All within 1e-12 relative."""
    A, X, bg, feat, v = _additive_case(3)
    want = (X[:, feat] - bg[feat])[:, :, None] * A[feat][None]
    scale = np.abs(want).max()
    exact = su.exact_shapley(v, X, bg, feat)
    assert exact.shape == want.shape == (7, 5, 3) and np.abs(exact - want).max() <= 1e-12 * scale
    orders = su.all_orders(5)
    assert orders.shape == (120, 5) and len({tuple(o) for o in orders}) == 120
    walk = su.walk64(v, X, bg, feat, orders)
    assert np.abs(walk - exact).max() <= 1e-12 * scale
    full, none = v(su.masked(X, bg, feat, [True] * 5)), v(su.masked(X, bg, feat, [False] * 5))
    assert np.array_equal(full, X @ A) and np.abs(full - none).max() > 0.1
    for o in (orders[17:18], orders[101:102]):
        one = su.walk64(v, X, bg, feat, o)
        assert np.abs(one.sum(axis=1) - (full - none)).max() <= 1e-12 * np.abs(full - none).max()
    assert su.err(walk, exact) <= 1e-12


def test_references_on_an_interacting_function():
    """With an interaction the single orders differ from the Shapley value and their mean over all orders does not: the walk
    really is the estimator, and a product of two players is shared equally."""
    rng = np.random.default_rng(4)
    X, bg, feat = rng.standard_normal((6, 4)), np.zeros(4), np.array([2, 0, 3])

    def v(Xm):
        return (Xm[:, 0] * Xm[:, 2] + Xm[:, 3])[:, None]
    exact = su.exact_shapley(v, X, bg, feat)
    want = np.stack([0.5 * X[:, 0] * X[:, 2], 0.5 * X[:, 0] * X[:, 2], X[:, 3]], axis=1)[:, :, None]
    assert np.abs(exact - want).max() <= 1e-12 * np.abs(want).max()
    orders = su.all_orders(3)
    assert np.abs(su.walk64(v, X, bg, feat, orders) - exact).max() <= 1e-12 * np.abs(want).max()
    assert su.err(su.walk64(v, X, bg, feat, orders[:1]), exact) > 0.1


def test_network_references_agree():
    """On the float64 network: the walk over all orders equals the enumeration (the test of the definition the GPU tests lean on), and
    one order's contributions sum to v(all) - v(none)."""
    import impact_util as fu
    from oracle import jamie_oracle as orc
    torch.manual_seed(5)
    P, Bf = orc.init_state((24, 16), 8)
    sd = {k: v.detach() for k, v in P.items()}
    sd.update(Bf)
    W = fu.weights64(fu.randomise_bn_state(sd, 1))
    rng = np.random.default_rng(2)
    X, bg, feat = rng.standard_normal((6, 24)), 0.5 * rng.standard_normal(24), np.array([7, 2, 19, 11])
    v = su.network_value(W, 0, 1, [5, 2])
    exact = su.exact_shapley(v, X, bg, feat)
    walk = su.walk64(v, X, bg, feat, su.all_orders(4))
    assert exact.shape == (6, 4, 2) and np.abs(exact).max() > 1e-3 and su.err(walk, exact) <= 1e-12
    one = su.walk64(v, X, bg, feat, [[2, 0, 3, 1]])
    gap = v(X) - v(su.masked(X, bg, feat, [False] * 4))
    assert np.abs(one.sum(axis=1) - gap).max() <= 1e-12 * np.abs(gap).max()


def test_shapley_kernels_use_no_scratch():
    """private_segment_fixed_size == 0 and no VGPR spills for every kernel of csrc/shapley.hip, read from the code object hipcc built:
    the rows of W0^T and the chains a lane holds stay in registers."""
    import isa_check as ic
    obj = os.path.join(ROOT, 'jamie_amd', 'csrc', '_obj', 'shapley.o')
    if not os.path.exists(obj):
        pytest.skip('the library is not built')
    if not os.path.exists(ic.OBJDUMP):
        pytest.skip('llvm-objdump not found')
    meta = ic.kernel_metadata(obj)
    names = ' '.join(meta)
    for kernel in ('shapley_stage_kernel', 'shapley_walk_kernel', 'shapley_accumulate_kernel', 'shapley_partial_kernel',
                   'shapley_finish_kernel'):
        assert kernel in names, (kernel, names)
    assert len(meta) == 6                                      # shapley_walk_kernel: the 16-byte and the any-width form
    for name, m in meta.items():
        assert m['private_segment_fixed_size'] == 0, (name, m)
        assert m.get('vgpr_spill_count', 0) == 0, (name, m)

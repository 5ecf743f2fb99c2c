"""Feature impact on the GPU: `jamie_occlusion_rows` against the float64 formula, `jamie_impact_accumulate` against float64 numpy on
the same fp32 inputs, `feature_impact` end to end against the loop route (replace the column, `model.impute`) and the float64
restatement of the network, and the `JAMIE.feature_impact` facade after a short fit.

Measured on an MI355X (err = max |per_target - float64| / max float64; (a) feature_impact, (b) the loop route; asserted:
err(a) <= 2 err(b)): [24, 16] 0 -> 1 6.3e-7 / 5.4e-7, 1 -> 0 3.8e-6 / 3.5e-6; [13, 10] padded 8.8e-7 / 1.0e-6 and 4.4e-7 / 3.9e-7;
with measured values 2.3e-8 / 2.0e-8; [512, 512] 3.3e-5 / 3.4e-5; jamie_impact_accumulate within 8.3e-15 at n = 4097 (bound
9.1e-13).  DESIGN.md 14 has the table; this module prints every figure before it asserts."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import impact_util as fu  # noqa: E402

pytestmark = pytest.mark.gpu

BN_EPS, SLOPE = 1e-5, 0.01


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _padded(a, ld):
    """The fp32 matrix `a` on the device inside a buffer with leading dimension `ld` (the rest NaN: reading it shows)."""
    buf = torch.full((a.shape[0], ld), float('nan'), device='cuda')
    buf[:, :a.shape[1]] = _dev(a)
    return buf[:, :a.shape[1]]


def _occlusion_case(n, h, g, seed, kink=False):
    """Inputs as the eval network meets them: the pre-activations lie around the running mean with the running variance (down to
    1e-3), so |H| stays below ~1 where 1 / sqrt(var) is ~30 and the fp32 rounding of H + delta W0 (relative 2^-24 twice), scaled by
    gamma / sqrt(var) <= 1.5 * 31.6, stays below 1.5 * 31.6 * 1.2e-7 * 1 = 6e-6 in absolute terms: inside atol 1e-5 where the
    result is small, inside rtol 1e-4 where it is large."""
    rng = np.random.default_rng(seed)
    d = max(1, h // 2)
    mean, var, gamma, beta = fu.random_bn(rng, h, 1e-3, 2.0)
    var[0] = 1e-3
    sd = np.sqrt(var)
    H = (mean + sd * rng.standard_normal((n, h))).astype(np.float32)
    X = rng.standard_normal((n, d)).astype(np.float32)
    bg = (0.5 * rng.standard_normal(d)).astype(np.float32)
    W0 = (0.3 * sd[:, None] * rng.uniform(-1, 1, (h, d))).astype(np.float32)
    feat = rng.integers(0, d, g).astype(np.int32)
    if g >= 3:
        feat[0], feat[1], feat[-1] = d - 1, 0, d - 1           # a repeat, and sorted neither way
    if kink:
        beta[:] = 0
        X[::3] = bg                                            # delta = 0 exactly: v = H
        H[::3] = mean                                          # v - mean = 0: on the kink
    return dict(H=H, X=X, bg=bg, W0=W0, feat=feat, mean=mean, var=var, gamma=gamma, beta=beta, d=d)


def _occlusion_want(c):
    H, X, W0 = (c[k].astype(np.float64) for k in ('H', 'X', 'W0'))
    out = []
    for f in c['feat']:
        v = H + (np.float64(c['bg'][f]) - X[:, f])[:, None] * W0[:, f][None, :]
        y = (v - c['mean']) / np.sqrt(c['var'].astype(np.float64) + BN_EPS) * c['gamma'] + c['beta']
        out.append(np.where(y > 0, y, SLOPE * y))
    return np.concatenate(out, 0)


def _run_occlusion(c, ldh_extra=8, ldw_extra=3):
    from jamie_amd import _native as nv
    n, h = c['H'].shape
    g, d = len(c['feat']), c['d']
    H, X, W0 = _padded(c['H'], h + ldh_extra), _padded(c['X'], d + 1), _padded(c['W0'], d + ldw_extra)
    assert H.stride(0) > h and W0.stride(0) > d
    out = torch.full((g * n, h), float('nan'), device='cuda')
    ws = torch.empty(nv.occlusion_workspace(g, h), dtype=torch.uint8, device='cuda')
    nv.occlusion_rows(H, X, _dev(c['bg']), W0, c['feat'], tuple(_dev(c[k]) for k in ('mean', 'var', 'gamma', 'beta')), out, ws,
                      eps=BN_EPS, slope=SLOPE)
    return out.cpu().numpy()


@pytest.mark.parametrize('g', [1, 3, 7])
@pytest.mark.parametrize('h', [6, 48, 130])
@pytest.mark.parametrize('n', [1, 63, 257])
def test_occlusion_rows_against_float64(n, h, g):
    c = _occlusion_case(n, h, g, 1000 * n + 10 * h + g)
    if g >= 3:
        assert len(set(c['feat'].tolist())) < g and list(c['feat']) != sorted(c['feat'])
    got, want = _run_occlusion(c), _occlusion_want(c)
    assert got.shape == want.shape == (g * n, h) and float(c['var'].min()) == pytest.approx(1e-3)
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize('n,h,g', [(70, 520, 9), (33, 262, 17), (40, 1024, 8)])
def test_occlusion_rows_several_column_tiles_and_groups(n, h, g):
    """More than 256 columns (several column tiles, the last one partial), more than 8 features (several register groups, the last
    one partial), with 16-byte accesses (h = 520, 1024) and without (h = 262)."""
    c = _occlusion_case(n, h, g, h + g)
    np.testing.assert_allclose(_run_occlusion(c), _occlusion_want(c), rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize('h', [6, 48])
def test_occlusion_rows_on_the_kink_is_exactly_zero(h):
    c = _occlusion_case(63, h, 3, 7, kink=True)
    got = _run_occlusion(c).reshape(3, 63, h)
    assert np.all(got[:, ::3] == 0) and not np.any(np.signbit(got[:, ::3]))
    assert np.count_nonzero(got[:, 1::3]) > 0.9 * got[:, 1::3].size
    np.testing.assert_allclose(got.reshape(-1, h), _occlusion_want(c), rtol=1e-4, atol=1e-5)


def _accumulate_case(n, g, dt, aligned, seed):
    rng = np.random.default_rng(seed)
    Y = rng.standard_normal((g * n, dt)).astype(np.float32)
    R = (rng.standard_normal((n, dt)) * rng.choice([1.0, 1e-3, 30.0], (1, dt))).astype(np.float32)
    ldy, ldr = ((dt + 3) // 4 * 4 + 4, (dt + 3) // 4 * 4) if aligned else (dt + 3, dt + 1)
    want = ((Y.astype(np.float64).reshape(g, n, dt) - R.astype(np.float64)[None]) ** 2).sum(1)
    return _padded(Y, ldy), _padded(R, ldr), want


@pytest.mark.parametrize('aligned', [False, True])
@pytest.mark.parametrize('dt', [1, 10, 130])
@pytest.mark.parametrize('g', [1, 5])
@pytest.mark.parametrize('n', [1, 300, 4097])
def test_impact_accumulate_against_float64(n, g, dt, aligned):
    """Every term is non-negative and exact up to one rounding each for the difference and the square, so the fp64 summation bound
    applies to the whole: relative error <= 2 (n + 2) 2^-53 (the factor 2 leaves room for numpy's own sum)."""
    _check_accumulate(n, g, dt, aligned)


def test_impact_accumulate_more_row_blocks_than_slices():
    """n = 17000: 34 row blocks for the finishing kernel's 32 slices."""
    _check_accumulate(17000, 2, 10, True)


def _check_accumulate(n, g, dt, aligned):
    from jamie_amd import _native as nv
    Y, R, want = _accumulate_case(n, g, dt, aligned, n + 7 * g + dt)
    assert Y.stride(0) > dt
    ws = torch.empty(nv.impact_accumulate_workspace(n, dt, g), dtype=torch.uint8, device='cuda')
    acc = torch.zeros(g, dt, dtype=torch.float64, device='cuda')
    nv.impact_accumulate(Y, R, acc, ws)
    once = acc.cpu().numpy()
    bound = 2 * (n + 2) * 2.0 ** -53
    rel = float((np.abs(once - want) / want).max())
    print(f'impact_accumulate n={n} g={g} dt={dt} aligned={aligned}: relative error {rel:.3e} (bound {bound:.3e})')
    assert np.all(want > 0) and rel <= bound
    nv.impact_accumulate(Y, R, acc, ws)                        # a second call adds onto acc: t + t is exact
    assert np.array_equal(acc.cpu().numpy(), 2 * once)
    again = torch.zeros_like(acc)
    ws.fill_(255)
    nv.impact_accumulate(Y, R, again, ws)
    assert np.array_equal(again.cpu().numpy(), once)           # bit-identical from run to run


# ---- end to end ----
def _model(dims, L, seed, pad=1):
    from jamie_amd.model import edModelVar
    torch.manual_seed(seed)
    model = edModelVar(list(dims), L, pad_features=pad)
    model.load_state_dict(fu.randomise_bn_state(model.state_dict(), seed + 1))
    return model.eval()


def _three_routes(model, X, i, t, bg, feat, measured=None, **kw):
    from jamie_amd.impact import feature_impact
    W = fu.weights64(model.state_dict())
    a = feature_impact(model, X, i, t, background=bg, features=feat, measured=measured, **kw)
    b, b_base = fu.loop_route(model, X, i, t, bg, feat, measured)
    c, c_base = fu.reference(W, X, i, t, bg, feat, measured)
    return a, (b, b_base), (c, c_base)


def _check_routes(tag, a, b, c):
    ea, eb = fu.err(a['per_target'], c[0]), fu.err(b[0], c[0])
    print(f'{tag}: err(a) feature_impact {ea:.3e}, err(b) loop route {eb:.3e}')
    assert a['per_target'].shape == c[0].shape and a['per_target'].dtype == np.float64
    assert np.array_equal(a['impact'], a['per_target'].mean(axis=1))
    assert ea <= 2 * eb, (tag, ea, eb)
    return ea, eb


@pytest.fixture(scope='module')
def small_models():
    return {'plain': _model((24, 16), 8, 11), 'padded': _model((13, 10), 8, 13, pad=8)}


@pytest.mark.parametrize('direction', [(0, 1), (1, 0)])
@pytest.mark.parametrize('which', ['plain', 'padded'])
def test_feature_impact_small_shapes(small_models, which, direction):
    """N = 300 cells, every feature, both directions: (a) feature_impact, (b) the loop route, (c) float64; then a workspace cap of
    450 rows (8 features beside each other, 56-cell chunks with a ragged last one, ragged last groups where the feature count is no
    multiple of 8) against the same float64 figures."""
    from jamie_amd import impact as fi
    model = small_models[which]
    i, t = direction
    rng = np.random.default_rng(17 + i)
    d = model.input_dim[i]
    X = rng.standard_normal((300, d)).astype(np.float32)
    bg = (0.3 * rng.standard_normal(d)).astype(np.float32)
    feat = np.arange(d)
    a, b, c = _three_routes(model, X, i, t, bg, feat)
    assert a['baseline'] is None and a['per_target'].shape == (d, model.input_dim[t])
    ea, eb = _check_routes(f'small {which} {i}->{t}', a, b, c)
    cap = 4 * 2 * max(model.pdims) * 450
    p = fi.plan(300, model.pdims[i], model.pdims[t], d, cap)
    assert len(p['chunks']) > 1 and len(p['groups']) > 1 and p['chunks'][-1][1] < p['n']
    chunked = fi.feature_impact(model, X, i, t, background=bg, max_workspace=cap)
    ec = fu.err(chunked['per_target'], c[0])
    print(f'small {which} {i}->{t}: err of the chunked run {ec:.3e} ({len(p["chunks"])} chunks x {len(p["groups"])} groups)')
    assert ec <= 2 * eb and np.array_equal(chunked['impact'], chunked['per_target'].mean(axis=1))
    # an unsorted feature list with a repeat: the rows of the full result
    pick = [d - 1, 2, 0, 2]
    sub = fi.feature_impact(model, X, i, t, background=bg, features=pick)
    assert np.array_equal(sub['per_target'], a['per_target'][pick])


def test_feature_impact_with_measured_values(small_models):
    model = small_models['plain']
    rng = np.random.default_rng(23)
    X = rng.standard_normal((300, 24)).astype(np.float32)
    measured = rng.standard_normal((300, 16)).astype(np.float32)
    a, b, c = _three_routes(model, X, 0, 1, np.zeros(24, np.float32), np.arange(24), measured=measured)
    _check_routes('small plain 0->1 measured', a, b, c)
    e_base = float(np.abs(a['baseline'] - c[1]).max() / c[1].max())
    print(f'baseline: feature_impact against float64 {e_base:.3e}, loop route {float(np.abs(b[1] - c[1]).max() / c[1].max()):.3e}')
    assert e_base <= 1e-4                                      # (the project's inference tolerance on the imputed values)


def test_feature_impact_mid_size_reaches_the_large_gemm_configuration():
    """edModelVar([512, 512], 32), 256 cells x 8 features = 2048 rows of 512 / 1024 columns: the eval path's large-shape GEMM
    configuration (model._eval_cfg) carries the occluded rows."""
    from jamie_amd.model import edModelVar
    model = _model((512, 512), 32, 29)
    assert edModelVar._eval_cfg(8 * 256, 512, 1024) >= 0 and edModelVar._eval_cfg(8 * 256, 1024, 512) >= 0
    rng = np.random.default_rng(31)
    X = rng.standard_normal((256, 512)).astype(np.float32)
    bg = np.zeros(512, np.float32)
    feat = [500, 3, 77, 128, 255, 256, 3, 511]
    a, b, c = _three_routes(model, X, 0, 1, bg, feat)
    _check_routes('mid-size 512 -> 512', a, b, c)


# ---- the facade ----
@pytest.fixture(scope='module')
def fitted():
    from jamie_amd import JAMIE
    rng = np.random.default_rng(3)
    Z = rng.standard_normal((160, 5))
    data = [(Z @ rng.standard_normal((5, d)) + 0.3 * rng.standard_normal((160, d)) + rng.uniform(-2, 2, d)).astype(np.float32)
            for d in (24, 16)]
    data[0][data[0] < 0.2] = 0                                 # (sparse-friendly: about half the entries are zero)
    jm = JAMIE(output_dim=8, epoch_DNN=3, min_epochs=1, batch_size=64, use_f_tilde=False, pca_dim=None, use_early_stop=False,
               manual_seed=4)
    jm.fit_transform(dataset=data, P=np.eye(160, dtype=np.float32))
    return jm, data


def test_facade_feature_impact(fitted, capsys):
    import scipy.sparse as sp
    from jamie_amd.utilities import preclass
    jm, data = fitted
    pre = [jm.model.preprocessing[i].__self__ for i in range(2)]
    assert all(isinstance(q, preclass) and q.axis == 0 and q.pca is None for q in pre)
    capsys.readouterr()
    full = jm.feature_impact(data[0], 0)
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith('feature impact 0 -> 1: 24 features')
    assert full['per_target'].shape == (24, 16) and full['baseline'] is None and np.all(full['impact'] > 0)
    # raw data with the default background == standardised cells with bg = 0
    Xs = pre[0].transform(np.asarray(data[0]))
    std = jm.feature_impact(Xs, 0, pre_transformed=True, background=np.zeros(24))
    for k in ('impact', 'per_target'):
        assert np.array_equal(std[k], full[k]), k
    # a background in data units == its standardised form
    bg = np.asarray(pre[0].mean, dtype=np.float64) + 0.5
    assert np.array_equal(jm.feature_impact(data[0], 0, background=bg)['per_target'],
                          jm.feature_impact(Xs, 0, pre_transformed=True, background=pre[0].transform(bg.copy()))['per_target'])
    sub = jm.feature_impact(data[0], 0, features=[5, 2])
    assert np.array_equal(sub['per_target'], full['per_target'][[5, 2]]) and np.array_equal(sub['impact'], full['impact'][[5, 2]])
    # measured values: the baseline is the per-feature MSE of the imputation against the standardised measured matrix
    m = jm.feature_impact(data[0], 0, measured=data[1])
    Ms = pre[1].transform(np.asarray(data[1])).astype(np.float32)
    Y = jm.model.impute(torch.from_numpy(Xs.astype(np.float32)), [0, 1]).double().cpu().numpy()
    want_base = ((Y - Ms.astype(np.float64)) ** 2).mean(0)
    np.testing.assert_allclose(m['baseline'], want_base, rtol=1e-12, atol=0)
    W = fu.weights64(jm.model.state_dict())
    Xs32 = Xs.astype(np.float32)
    c, c_base = fu.reference(W, Xs32, 0, 1, np.zeros(24), np.arange(24), Ms)
    b, _ = fu.loop_route(jm.model, Xs32, 0, 1, np.zeros(24, np.float32), np.arange(24), Ms)
    ea, eb = fu.err(m['per_target'], c), fu.err(b, c)
    print(f'facade measured: err(a) {ea:.3e}, err(b) {eb:.3e}')
    assert ea <= 2 * eb
    # the other direction and an explicit target
    back = jm.feature_impact(data[1], 1, to_modality=0)
    assert back['per_target'].shape == (16, 24)
    # scipy sparse cells: standardised on the device from the stored entries
    sparse = jm.feature_impact(sp.csr_matrix(data[0]), 0)
    np.testing.assert_allclose(sparse['per_target'], full['per_target'], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(sparse['impact'], full['impact'], rtol=1e-4, atol=1e-5)


def test_facade_refuses_a_pca_modality():
    from jamie_amd import JAMIE
    rng = np.random.default_rng(5)
    Z = rng.standard_normal((96, 4))
    data = [(Z @ rng.standard_normal((4, d)) + 0.3 * rng.standard_normal((96, d))).astype(np.float32) for d in (24, 16)]
    jm = JAMIE(output_dim=4, epoch_DNN=1, min_epochs=1, batch_size=32, use_f_tilde=False, pca_dim=[6, 5], use_early_stop=False,
               manual_seed=4)
    jm.fit_transform(dataset=data, P=np.eye(96, dtype=np.float32))
    with pytest.raises(ValueError, match='pre_transformed=True'):
        jm.feature_impact(data[0], 0)
    # ... and takes the PCA scores themselves: the features are then the network's 6 input columns
    scores = jm.model.preprocessing[0](np.asarray(data[0]))
    out = jm.feature_impact(scores, 0, pre_transformed=True)
    assert out['per_target'].shape == (6, 5)

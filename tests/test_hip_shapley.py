"""Shapley attributions on the GPU: `jamie_shapley_walk_rows` against the float64 chain (rows, carried state, segments bit for bit),
`jamie_shapley_accumulate` bit for bit against the float64 numpy loop, `jamie_shapley_summarise` against float64 numpy,
`shapley_values` end to end against the coalition enumeration, the float64 walk and the loop route (every masked input through
`model.impute`), and the `JAMIE.shapley_values` facade after a short fit.

err = max |values - float64 reference| / max |reference|; (a) shapley_values, (b) the loop route; asserted: err(a) <= 2 err(b).
Measured on an MI355X, err(a) / err(b): all 120 orders of 5 players against the coalition enumeration, [24, 16] 0 -> 1 1.6e-6 / 1.6e-6,
1 -> 0 5.4e-6 / 5.3e-6, [13, 10] padded 1.5e-6 / 1.7e-6 and 1.1e-6 / 1.1e-6; 12 sampled orders against the float64 walk, [24, 16]
1.6e-6 / 1.8e-6 (efficiency 1.9e-6 / 1.8e-6), [13, 10] padded 2.1e-6 / 1.9e-6 (1.7e-6 / 1.7e-6), the chunked and segmented runs the
same to the digits printed; [512, 512] 8.4e-5 / 8.1e-5 at 64 cells, 8.3e-5 / 9.4e-5 at 256; the fitted facade model 5.6e-7 / 7.4e-7.
Walk of 17 steps: final state error at most 0.34 of its bound, row error at most 0.57 of its bound; jamie_shapley_summarise within
5.9e-15 at n = 4097 (bound 9.1e-13).
DESIGN.md 15 has the table; this module prints every figure before it asserts."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import impact_util as fu  # noqa: E402
import shapley_util as su  # noqa: E402

pytestmark = pytest.mark.gpu

BN_EPS, SLOPE = 1e-5, 0.01
U = 2.0 ** -24                                                 # fp32 unit roundoff


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _padded(a, ld):
    """The fp32 matrix `a` on the device inside a buffer with leading dimension `ld` (the rest NaN: reading it shows)."""
    buf = torch.full((a.shape[0], ld), float('nan'), device='cuda')
    buf[:, :a.shape[1]] = _dev(a)
    return buf[:, :a.shape[1]]


# ---- jamie_shapley_walk_rows ----
def _walk_case(n, h, g, seed, kink=False, still=()):
    """Inputs as test_hip_impact._occlusion_case builds them, which is how the eval network meets them: the pre-activations lie
    around the running mean with the running variance (down to 1e-3, pinned in column 0), a column of W0 is 0.3 sd uniform, so a
    step moves a pre-activation by a fraction of its spread and |s| stays below ~1 where 1 / sqrt(var) is ~30.  The g features are
    distinct and in no order.  `still`: steps whose feature equals its background in every cell (x - bg = 0 exactly); `kink`: every
    third cell starts exactly on the LeakyReLU kink (H = mean, beta = 0)."""
    rng = np.random.default_rng(seed)
    d = max(1, h // 2, g + 3)
    mean, var, gamma, beta = fu.random_bn(rng, h, 1e-3, 2.0)
    var[0] = 1e-3
    sd = np.sqrt(var)
    H = (mean + sd * rng.standard_normal((n, h))).astype(np.float32)
    X = rng.standard_normal((n, d)).astype(np.float32)
    bg = (0.5 * rng.standard_normal(d)).astype(np.float32)
    W0 = (0.3 * sd[:, None] * rng.uniform(-1, 1, (h, d))).astype(np.float32)
    feat = rng.permutation(d)[:g].astype(np.int32)
    if g >= 3:
        lo, mid, hi = sorted(feat[:3])
        feat[:3] = hi, lo, mid                                 # sorted neither way
    for m in still:
        X[:, feat[m]] = bg[feat[m]]
    if kink:
        beta[:] = 0
        H[::3] = mean
    return dict(H=H, X=X, bg=bg, W0=W0, feat=feat, mean=mean, var=var, gamma=gamma, beta=beta, d=d)


def _bn64(c, s):
    y = (s - c['mean']) / np.sqrt(c['var'].astype(np.float64) + BN_EPS) * c['gamma'] + c['beta']
    return np.where(y > 0, y, SLOPE * y)


def _walk_want(c):
    """(rows [(g + 1) n, h], states [g + 1, n, h], moved [g + 1, n, h]) in float64 from the fp32 inputs: moved_m = |H| + the
    absolute rank-one terms up to step m, the magnitude every rounding of the fp32 chain is relative to."""
    H, X, W0, bg = (c[k].astype(np.float64) for k in ('H', 'X', 'W0', 'bg'))
    s, moved = H.copy(), np.abs(H)
    states, moves = [s.copy()], [moved.copy()]
    for f in c['feat']:
        term = (X[:, f] - bg[f])[:, None] * W0[:, f][None, :]
        s = s - term
        moved = moved + np.abs(term)
        states.append(s.copy())
        moves.append(moved.copy())
    states = np.stack(states)
    return np.concatenate([_bn64(c, s) for s in states], 0), states, np.stack(moves)


def _run_walk(c, segments=None, ld_extra=8, ldw_extra=3):
    """The walk in one launch, or in the given segments with the carried state: (rows of every launch, the final state)."""
    from jamie_amd import _native as nv
    n, h = c['H'].shape
    g, d = len(c['feat']), c['d']
    state, X, W0 = _padded(c['H'], h + ld_extra), _padded(c['X'], d + 1), _padded(c['W0'], d + ldw_extra)
    assert state.stride(0) > h and W0.stride(0) > d
    bn = tuple(_dev(c[k]) for k in ('mean', 'var', 'gamma', 'beta'))
    bg = _dev(c['bg'])
    outs, m0 = [], 0
    for gc in ([g] if segments is None else segments):
        buf = torch.full(((gc + 1) * n, h + 4), float('nan'), device='cuda')
        ws = torch.empty(nv.shapley_walk_workspace(gc, h), dtype=torch.uint8, device='cuda')
        nv.shapley_walk_rows(state, X, bg, W0, c['feat'][m0:m0 + gc], bn, buf[:, :h], ws, eps=BN_EPS, slope=SLOPE)
        got = buf.cpu().numpy()
        assert np.all(np.isnan(got[:, h:]))                   # nothing is written beyond the h columns of a row
        outs.append(got[:, :h].reshape(gc + 1, n, h))
        m0 += gc
    assert m0 == g
    full = state.as_strided((n, h + ld_extra), (h + ld_extra, 1)).cpu().numpy()
    assert np.all(np.isnan(full[:, h:]))
    return outs, full[:, :h]


@pytest.mark.parametrize('h', [6, 48, 130, 520])
@pytest.mark.parametrize('n', [1, 63, 257])
def test_walk_rows_against_float64(n, h):
    """A segment of 3 steps in unsorted order: the scalar form (h = 6, 130), one vector tile (48), a ragged tile (130) and several
    column tiles (520), padded leading dimensions, running variances down to 1e-3.  A row carries at most 3 fmaf roundings and the
    one of x - bg, each at most half an ulp of |s| < 1 (3e-8), scaled by gamma / sqrt(var) <= 1.5 * 31.6: 4e-6 in absolute terms,
    inside atol 1e-5 where the result is small, inside rtol 1e-4 where it is large."""
    c = _walk_case(n, h, 3, 1000 * n + h)
    (got,), state = _run_walk(c)
    want, states, moved = _walk_want(c)
    assert got.shape == (4, n, h) and float(c['var'].min()) == pytest.approx(1e-3)
    assert list(c['feat']) != sorted(c['feat']) and list(c['feat']) != sorted(c['feat'], reverse=True)
    np.testing.assert_allclose(got.reshape(-1, h), want, rtol=1e-4, atol=1e-5)
    assert np.all(np.abs(state - states[-1]) <= 4 * U * moved[-1])                       # (the bound of the 17-step test, g = 3)


def _row_bound(c, states, moved):
    """The bound on |row - float64| that test_walk_of_17_steps_in_segments_and_in_one_launch derives, [g + 1, n, h]."""
    scale = np.abs(c['gamma'].astype(np.float64)) / np.sqrt(c['var'].astype(np.float64) + BN_EPS)
    steps = np.arange(1, len(states) + 1)[:, None, None]
    return scale * steps * U * moved + 12 * U * (np.abs(states - c['mean']) * scale + np.abs(c['beta'].astype(np.float64)))


@pytest.mark.parametrize('h', [6, 48, 130, 520])
@pytest.mark.parametrize('n', [1, 63, 257])
def test_walk_of_17_steps_in_segments_and_in_one_launch(n, h):
    """17 steps as 8 + 8 + 1 with the carried state against one launch of g = 17: the same fmaf chain, so the rows and the final
    state are bit-identical (the rows at the seams are emitted twice).  Against float64: every element of state m is within
    (m + 1) 2^-24 (|H| + sum of |dl W0[., f]| up to m) -- one rounding per fmaf and one for x - bg, dl from the fp32 inputs in
    float64 -- and a row within that times gamma / sqrt(var + eps) (LeakyReLU is 1-Lipschitz) plus the BatchNorm expression's own
    roundings: 3.5 for the scale (var + eps, rsqrt to an ulp, times gamma), 1 for s - mean, 1 for the product and sum, 1 for the
    slope, together below 12 x 2^-24 (|(s - mean) scale| + |beta|)."""
    g = 17
    c = _walk_case(n, h, g, 77 * n + h)
    (one,), state_one = _run_walk(c)
    parts, state_seg = _run_walk(c, segments=[8, 8, 1])
    assert one.shape == (g + 1, n, h) and [p.shape[0] for p in parts] == [9, 9, 2]
    assert np.array_equal(parts[0], one[0:9]) and np.array_equal(parts[1], one[8:17]) and np.array_equal(parts[2], one[16:18])
    assert np.array_equal(state_seg, state_one)
    want, states, moved = _walk_want(c)
    bound = (g + 1) * U * moved[-1]
    excess = float((np.abs(state_one - states[-1]) / bound).max())
    print(f'walk n={n} h={h} g={g}: final state error / bound {excess:.3f}')
    assert excess <= 1.0
    row_excess = float((np.abs(one - want.reshape(g + 1, n, h)) / _row_bound(c, states, moved)).max())
    print(f'walk n={n} h={h} g={g}: row error / bound {row_excess:.3f}')
    assert row_excess <= 1.0


@pytest.mark.parametrize('h', [6, 48])
def test_walk_repeats_a_row_where_x_is_the_background_and_gives_plus_zero_on_the_kink(h):
    c = _walk_case(63, h, 9, 7, kink=True, still=(0, 4, 8))
    (got,), state = _run_walk(c)
    for m in (0, 4, 8):                                        # step m writes row m + 1
        assert np.array_equal(got[m + 1].view(np.int32), got[m].view(np.int32)), m
    assert not np.array_equal(got[2], got[1]) and not np.array_equal(got[6], got[5])
    assert np.all(got[0:2, ::3] == 0) and not np.any(np.signbit(got[0:2, ::3]))          # on the kink: +0, before and after a still step
    assert np.count_nonzero(got[0, 1::3]) > 0.9 * got[0, 1::3].size
    want, states, moved = _walk_want(c)
    assert np.all(np.abs(got - want.reshape(got.shape)) <= _row_bound(c, states, moved))  # (9 steps: the 17-step test's bounds)
    assert np.all(np.abs(state - states[-1]) <= 10 * U * moved[-1])


# ---- jamie_shapley_accumulate ----
@pytest.mark.parametrize('g', [1, 8, 17])
@pytest.mark.parametrize('T', [1, 5, 64, 130])
@pytest.mark.parametrize('n', [1, 63, 513])
def test_accumulate_is_the_float64_loop_bit_for_bit(n, T, g):
    """Three launches on different Y, a padded ldy, an unsorted subset of the columns, positions scattered in a larger F: phi equals
    the numpy loop acc += Ya.astype(f64) - Yb.astype(f64) in the same order (IEEE operations in a fixed order, nothing to
    contract), and what was not addressed keeps its sentinel."""
    from jamie_amd import _native as nv
    rng = np.random.default_rng(n + 1000 * T + g)
    dt, F = T + 7, g + 6
    free = np.array([k for k in range(F) if k not in (1, F - 2)])                       # positions 1 and F - 2 are never addressed
    tcol = rng.permutation(dt)[:T].astype(np.int32)
    sentinel = -12345.678
    phi = torch.full((n, F, T), sentinel, dtype=torch.float64, device='cuda')
    want = np.full((n, F, T), sentinel)
    touched = np.zeros(F, bool)
    for launch in range(3):
        Y = (rng.standard_normal(((g + 1) * n, dt)) * rng.choice([1.0, 1e-3, 30.0], (1, dt))).astype(np.float32)
        pos = rng.permutation(free)[:g].astype(np.int32)
        touched[pos] = True
        Yd = _padded(Y, dt + 3)
        assert Yd.stride(0) > dt
        nv.shapley_accumulate(Yd, pos, phi, tcol=tcol)
        Y3 = Y.reshape(g + 1, n, dt)[:, :, tcol]
        for m in range(g):
            want[:, pos[m], :] += Y3[m].astype(np.float64) - Y3[m + 1].astype(np.float64)
    got = phi.cpu().numpy()
    assert np.array_equal(got, want)
    assert np.all(got[:, ~touched, :] == sentinel) and (~touched).sum() >= 2 and np.all(got[:, touched, :] != sentinel)


def test_accumulate_all_columns_in_order():
    """tcol = None: all dt columns in order, T == dt."""
    from jamie_amd import _native as nv
    rng = np.random.default_rng(5)
    n, g, dt, F = 63, 8, 19, 11
    Y = rng.standard_normal(((g + 1) * n, dt)).astype(np.float32)
    pos = rng.permutation(F)[:g].astype(np.int32)
    phi = torch.zeros(n, F, dt, dtype=torch.float64, device='cuda')
    nv.shapley_accumulate(_padded(Y, dt + 1), pos, phi)
    Y3 = Y.reshape(g + 1, n, dt).astype(np.float64)
    want = np.zeros((n, F, dt))
    for m in range(g):
        want[:, pos[m]] += Y3[m] - Y3[m + 1]
    assert np.array_equal(phi.cpu().numpy(), want)


# ---- jamie_shapley_summarise ----
@pytest.mark.parametrize('shape', [(7, 19), (3, 130)])
@pytest.mark.parametrize('n', [1, 511, 4097])
def test_summarise_against_float64(n, shape):
    """Every partial sum is one of at most n + 8 ordered additions: relative to sum |phi| the error is below the fp64 summation
    bound 2 (n + 2) 2^-53 (the factor 2 leaves room for numpy's own sum).  A second call doubles the outputs exactly and repeated
    runs are bit-identical."""
    from jamie_amd import _native as nv
    rng = np.random.default_rng(n + shape[1])
    phi = rng.standard_normal((n,) + shape) * rng.choice([1.0, 1e-3, 30.0], shape)
    phid = _dev(phi)
    ws = torch.empty(nv.shapley_summarise_workspace(n, shape[0] * shape[1]), dtype=torch.uint8, device='cuda')
    sa, ss = (torch.zeros(shape, dtype=torch.float64, device='cuda') for _ in range(2))
    nv.shapley_summarise(phid, sa, ss, ws)
    a1, s1 = sa.cpu().numpy(), ss.cpu().numpy()
    ref_a, ref_s = np.abs(phi).sum(0), phi.sum(0)
    bound = 2 * (n + 2) * 2.0 ** -53
    rel_a, rel_s = float((np.abs(a1 - ref_a) / ref_a).max()), float((np.abs(s1 - ref_s) / ref_a).max())
    print(f'shapley_summarise n={n} elems={shape[0] * shape[1]}: relative error of sum |phi| {rel_a:.3e}, of sum phi {rel_s:.3e} '
          f'(bound {bound:.3e})')
    assert np.all(ref_a > 0) and rel_a <= bound and rel_s <= bound
    nv.shapley_summarise(phid, sa, ss, ws)                     # a second call adds onto the outputs: t + t is exact
    assert np.array_equal(sa.cpu().numpy(), 2 * a1) and np.array_equal(ss.cpu().numpy(), 2 * s1)
    sa2, ss2 = torch.zeros_like(sa), torch.zeros_like(ss)
    ws.fill_(255)
    nv.shapley_summarise(phid, sa2, ss2, ws)
    assert np.array_equal(sa2.cpu().numpy(), a1) and np.array_equal(ss2.cpu().numpy(), s1)


# ---- end to end ----
def _model(dims, L, seed, pad=1):
    from jamie_amd.model import edModelVar
    torch.manual_seed(seed)
    model = edModelVar(list(dims), L, pad_features=pad)
    model.load_state_dict(fu.randomise_bn_state(model.state_dict(), seed + 1))
    return model.eval()


@pytest.fixture(scope='module')
def small_models():
    return {'plain': _model((24, 16), 8, 11), 'padded': _model((13, 10), 8, 13, pad=8)}


def _check_routes(tag, a, b, ref):
    ea, eb = su.err(a, ref), su.err(b, ref)
    print(f'{tag}: err(a) shapley_values {ea:.3e}, err(b) loop route {eb:.3e}')
    assert a.shape == b.shape == ref.shape and a.dtype == np.float64
    assert ea <= 2 * eb, (tag, ea, eb)
    return ea, eb


@pytest.mark.parametrize('direction', [(0, 1), (1, 0)])
@pytest.mark.parametrize('which', ['plain', 'padded'])
def test_exact_shapley_over_all_orders(small_models, which, direction):
    """40 cells, 5 players given unsorted, a random background, all 120 orders: `values` against the enumeration of the 32
    coalitions in float64 -- the test of the definition itself."""
    from jamie_amd import shapley as sh
    model = small_models[which]
    i, t = direction
    d = model.input_dim[i]
    rng = np.random.default_rng(41 + i)
    X = rng.standard_normal((40, d)).astype(np.float32)
    bg = (0.5 * rng.standard_normal(d)).astype(np.float32)
    feat = np.array([d - 1, 2, 7, 0, 5])
    orders = su.all_orders(5)
    W = fu.weights64(model.state_dict())
    ref = su.exact_shapley(su.network_value(W, i, t), X, bg, feat)
    out = sh.shapley_values(model, X, i, t, background=bg, features=feat, orders=orders, return_values=True)
    b = su.loop_route(model, X, i, t, bg, feat, orders)
    assert out['values'].shape == (40, 5, model.input_dim[t]) and np.array_equal(out['orders'], orders)
    _check_routes(f'exact {which} {i}->{t}', out['values'], b, ref)


@pytest.fixture(scope='module')
def sampled(small_models):
    """Per model: 300 cells, every feature of modality 0 a player (feature 7 equal to its background in every cell), 6 drawn orders
    and their reverses; the single-pass result, the loop route and the float64 walk with the same orders, computed once."""
    from jamie_amd import shapley as sh
    out = {}
    for which, model in small_models.items():
        d = model.input_dim[0]
        rng = np.random.default_rng(17)
        X = rng.standard_normal((300, d)).astype(np.float32)
        bg = (0.3 * rng.standard_normal(d)).astype(np.float32)
        X[:, 7] = bg[7]
        feat = np.arange(d)
        orders = sh.draw_orders(d, 6, antithetic=True, seed=3)
        W = fu.weights64(model.state_dict())
        a = sh.shapley_values(model, X, 0, 1, background=bg, orders=orders, return_values=True)
        out[which] = dict(model=model, X=X, bg=bg, feat=feat, orders=orders, W=W, a=a,
                          b=su.loop_route(model, X, 0, 1, bg, feat, orders),
                          ref=su.walk64(su.network_value(W, 0, 1), X, bg, feat, orders))
    return out


def _check_summaries(a):
    """`mean_abs` and `mean` are the cell means of `values` within the fp64 summation bound 2 (N + 2) 2^-53 (+ 4 for the roundings of
    the divisions by P and by P N) of mean |values|; `importance` is the row mean of `mean_abs` exactly."""
    N = a['values'].shape[0]
    bound = (2 * (N + 2) + 4) * 2.0 ** -53 * np.abs(a['values']).mean(0)
    assert np.all(np.abs(a['mean_abs'] - np.abs(a['values']).mean(0)) <= bound)
    assert np.all(np.abs(a['mean'] - a['values'].mean(0)) <= bound)
    assert np.array_equal(a['importance'], a['mean_abs'].mean(axis=1)) and a['mean_abs'].shape == a['mean'].shape == a['values'].shape[1:]


@pytest.mark.parametrize('which', ['plain', 'padded'])
def test_sampled_orders(sampled, which):
    """The reference is the float64 walk with the same orders, so there is no sampling error in the comparison.  Efficiency: the
    contributions of a cell sum to v(all) - v(none).  The null player (feature 7) has values == 0 exactly -- at these widths a row's
    GEMM sums do not depend on its neighbours, so equal rows in give equal rows out; not claimed beyond them."""
    s = sampled[which]
    a, d = s['a'], len(s['feat'])
    assert s['orders'].shape == (12, d) and a['values'].shape == (300, d, s['model'].input_dim[1])
    _check_routes(f'sampled {which}', a['values'], s['b'], s['ref'])
    v = su.network_value(s['W'], 0, 1)
    gap = v(s['X'].astype(np.float64)) - v(su.masked(s['X'], s['bg'], s['feat'], [False] * d))
    ea, eb = su.err(a['values'].sum(axis=1), gap), su.err(s['b'].sum(axis=1), gap)
    print(f'sampled {which}: efficiency err(a) {ea:.3e}, err(b) {eb:.3e}')
    assert ea <= 2 * eb
    assert np.all(a['values'][:, 7, :] == 0) and np.all(s['ref'][:, 7, :] == 0) and np.abs(a['values'][:, 6, :]).max() > 0
    _check_summaries(a)


@pytest.mark.parametrize('which', ['plain', 'padded'])
def test_sampled_orders_in_ragged_chunks_and_segments(sampled, which):
    """A workspace of 510 rows: 56-cell chunks over 300 cells (the last one 20), segments of 8 steps -- 8, 8, 8 for the 24 players,
    8 and a last one of 5 for the 13 -- and for the 24 players also the accumulator cap at 56 cells with segments of 10, 10 and 4.
    The result matches the single pass in err to the digits printed."""
    from jamie_amd import shapley as sh
    s = sampled[which]
    model, d = s['model'], len(s['feat'])
    row = 4 * 2 * max(model.pdims)
    caps = [dict(max_workspace=row * 510)]
    if which == 'plain':
        caps.append(dict(max_workspace=row * 56 * 11, max_accumulator=8 * d * model.input_dim[1] * 56 + 100))
    e1, eb = su.err(s['a']['values'], s['ref']), su.err(s['b'], s['ref'])
    ragged = False
    for cap in caps:
        p = sh.plan(300, model.pdims[0], model.pdims[1], d, model.input_dim[1], **cap)
        assert p['n'] == 56 and len(p['chunks']) == 6 and p['chunks'][-1] == (280, 20) and len(p['segments']) > 1
        ragged = ragged or p['segments'][-1][1] < p['g']
        c = sh.shapley_values(model, s['X'], 0, 1, background=s['bg'], orders=s['orders'], return_values=True, **cap)
        ec = su.err(c['values'], s['ref'])
        print(f'sampled {which}: err of the chunked run {ec:.3e} against {e1:.3e} in one pass ({len(p["chunks"])} chunks x segments '
              f'{[b for _, b in p["segments"]]}), err(b) {eb:.3e}')
        assert ec <= 2 * eb and f'{ec:.2e}' == f'{e1:.2e}'
        _check_summaries(c)
    assert ragged


def test_targets_are_the_columns_of_the_full_result(sampled):
    from jamie_amd import shapley as sh
    s = sampled['plain']
    sub = sh.shapley_values(s['model'], s['X'], 0, 1, background=s['bg'], targets=[5, 2], orders=s['orders'], return_values=True)
    assert sub['values'].shape == (300, 24, 2)
    for k in ('values', 'mean_abs', 'mean'):
        assert np.array_equal(sub[k], s['a'][k][..., [5, 2]]), k
    assert np.array_equal(sub['importance'], sub['mean_abs'].mean(axis=1))
    assert sh.shapley_values(s['model'], s['X'], 0, 1, background=s['bg'], targets=[5, 2], orders=s['orders'])['values'] is None


@pytest.mark.parametrize('cells', [64, 256])
def test_wide_layers(cells):
    """edModelVar([512, 512], 32), 8 players, 4 orders: 64 cells, and 256 cells where the 9 x 256 = 2304 rows of a segment reach the
    eval path's large-shape GEMM configuration (model._eval_cfg)."""
    from jamie_amd import shapley as sh
    from jamie_amd.model import edModelVar
    model = _model((512, 512), 32, 29)
    assert (edModelVar._eval_cfg(9 * cells, 512, 1024) >= 0) == (cells == 256)
    rng = np.random.default_rng(31)
    X = rng.standard_normal((cells, 512)).astype(np.float32)
    bg = np.zeros(512, np.float32)
    feat = np.array([500, 3, 77, 128, 255, 256, 4, 511])
    orders = sh.draw_orders(8, 2, antithetic=True, seed=1)
    W = fu.weights64(model.state_dict())
    ref = su.walk64(su.network_value(W, 0, 1), X, bg, feat, orders)
    out = sh.shapley_values(model, X, 0, 1, background=bg, features=feat, orders=orders, return_values=True)
    b = su.loop_route(model, X, 0, 1, bg, feat, orders)
    _check_routes(f'wide 512 -> 512, {cells} cells', out['values'], b, ref)


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


def test_facade_shapley_values(fitted, capsys):
    import scipy.sparse as sp
    from jamie_amd import shapley as sh
    from jamie_amd.utilities import preclass
    jm, data = fitted
    pre = [jm.model.preprocessing[i].__self__ for i in range(2)]
    assert all(isinstance(q, preclass) and q.axis == 0 and q.pca is None for q in pre)
    capsys.readouterr()
    full = jm.shapley_values(data[0], 0, n_permutations=3, seed=9, return_values=True)
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith('shapley values 0 -> 1: 24 features, 6 orders')
    assert full['values'].shape == (160, 24, 16) and full['orders'].shape == (6, 24) and full['orders'].dtype == np.int32
    assert np.array_equal(full['orders'], sh.draw_orders(24, 3, True, 9)) and np.all(full['importance'] > 0)
    # data units with the default background == the library call on the standardised cells with bg = 0
    Xs = pre[0].transform(np.asarray(data[0]))
    lib = sh.shapley_values(jm.model, Xs, 0, 1, background=np.zeros(24), orders=full['orders'], return_values=True)
    for k in ('values', 'mean_abs', 'mean', 'importance'):
        assert np.array_equal(lib[k], full[k]), k
    # the same seed: the same orders and bit-identical results; another seed: other orders
    again = jm.shapley_values(data[0], 0, n_permutations=3, seed=9, return_values=True)
    assert np.array_equal(again['orders'], full['orders']) and np.array_equal(again['values'], full['values'])
    assert not np.array_equal(jm.shapley_values(data[0], 0, n_permutations=3, seed=10)['orders'], full['orders'])
    # explicit orders override the drawing; without antithetic the reverses are left out
    assert np.array_equal(jm.shapley_values(data[0], 0, orders=full['orders'][:2], n_permutations=50)['orders'], full['orders'][:2])
    assert np.array_equal(jm.shapley_values(data[0], 0, n_permutations=3, seed=9, antithetic=False)['orders'], full['orders'][0::2])
    # a background in data units == its standardised form; players and targets by index
    bg = np.asarray(pre[0].mean, dtype=np.float64) + 0.5
    kw = dict(features=[5, 2, 11], targets=[3, 0], orders=su.all_orders(3), return_values=True)
    a = jm.shapley_values(data[0], 0, background=bg, **kw)
    b = jm.shapley_values(Xs, 0, pre_transformed=True, background=pre[0].transform(bg.copy()), **kw)
    assert a['values'].shape == (160, 3, 2) and np.array_equal(a['values'], b['values'])
    # against float64 on the fitted weights
    W = fu.weights64(jm.model.state_dict())
    Xs32, bgs = Xs.astype(np.float32), pre[0].transform(bg.copy()).astype(np.float32)
    ref = su.exact_shapley(su.network_value(W, 0, 1, [3, 0]), Xs32, bgs, [5, 2, 11])
    loop = su.loop_route(jm.model, Xs32, 0, 1, bgs, [5, 2, 11], su.all_orders(3), tcol=[3, 0])
    _check_routes('facade, fitted model', a['values'], loop, ref)
    # the other direction
    back = jm.shapley_values(data[1], 1, to_modality=0, n_permutations=1)
    assert back['mean_abs'].shape == (16, 24) and back['values'] is None
    # scipy sparse cells: standardised on the device from the stored entries
    sparse = jm.shapley_values(sp.csr_matrix(data[0]), 0, n_permutations=3, seed=9, return_values=True)
    np.testing.assert_allclose(sparse['values'], full['values'], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(sparse['mean_abs'], full['mean_abs'], rtol=1e-4, atol=1e-5)


def test_facade_refuses_a_pca_modality():
    from jamie_amd import JAMIE
    rng = np.random.default_rng(5)
    Z = rng.standard_normal((96, 4))
    data = [(Z @ rng.standard_normal((4, d)) + 0.3 * rng.standard_normal((96, d))).astype(np.float32) for d in (24, 16)]
    jm = JAMIE(output_dim=4, epoch_DNN=1, min_epochs=1, batch_size=32, use_f_tilde=False, pca_dim=[6, 5], use_early_stop=False,
               manual_seed=4)
    jm.fit_transform(dataset=data, P=np.eye(96, dtype=np.float32))
    with pytest.raises(ValueError, match='pre_transformed=True'):
        jm.shapley_values(data[0], 0)
    # ... and takes the PCA scores themselves: the players are then the network's 6 input columns
    scores = jm.model.preprocessing[0](np.asarray(data[0]))
    out = jm.shapley_values(scores, 0, pre_transformed=True, n_permutations=2)
    assert out['mean_abs'].shape == (6, 5) and out['orders'].shape == (4, 6)

"""The t-SNE layout on the device (jamie_amd/tsne.py, csrc/tsne.hip) against the float64 references of tsne_util.py.

Affinities: the device solve on the device's own lists equals the float64 loop (beta within 1e-12, the stored fp32 C within 2^-24
relative, equal tries; cells whose trace comes within 1e-11 of a branch are left out, at most 0.5 % of them).  Joint P: the
pattern of (C + C^T) exactly, symmetric to the bit, rows in the defined order.  Gradient: every sum within tsne_util.GRAD_TOL of
float64 numpy, relative to the float64 sum of its terms' magnitudes.  Every figure is printed before it is asserted."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lisi_util as lu  # noqa: E402
import tsne_util as tu  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
SIZES = sorted(tu.SHAPES)


@pytest.fixture(scope='module')
def jt():
    from jamie_amd import tsne
    return tsne


_cache = {}


def device_case(jt, N):
    """self_knn, affinities and P of SHAPES[N] on the device, once."""
    if N not in _cache:
        from jamie_amd.neighbors import self_knn
        c = tu.shape_case(N)
        idx, dist = self_knn(c['X'], c['K'])
        C, beta, tries = jt.affinities(idx, dist, c['u'])
        P = jt.joint_from_affinities(idx, C)
        _cache[N] = dict(idx=idx, dist=dist, C=C, beta=beta, tries=tries, P=P)
    return _cache[N]


def _scipy(P):
    S = P.to_scipy().astype(np.float64)
    S.sort_indices()
    return S


@pytest.mark.parametrize('N', SIZES)
def test_affinities_equal_the_float64_loop(jt, N):
    d = device_case(jt, N)
    c = tu.shape_case(N)
    K = c['K']
    assert d['C'].dtype == torch.float32 and d['C'].shape == (N, K) and d['beta'].dtype == torch.float64
    C, beta, tries = d['C'].cpu().numpy(), d['beta'].cpu().numpy(), d['tries'].cpu().numpy()
    rC, rbeta, rtries, _, margin = tu.affinity_reference(d['dist'].cpu().numpy(), c['u'])
    near = margin < tu.NEAR_BRANCH
    keep = ~near
    rel_beta = np.max(np.abs(beta[keep] - rbeta[keep]) / rbeta[keep])
    err_C = np.abs(C[keep].astype(np.float64) - rC[keep])
    bound_C = (EPS + 1e-12) * rC[keep] + 2.0 ** -150
    rows = np.abs(C.astype(np.float64).sum(axis=1) - 1.0).max()
    print(f'N = {N} K = {K}: near a branch {near.mean():.4f}, beta within {rel_beta:.2e}, C within {np.max(err_C / (rC[keep] + 1e-300)):.3e} '
          f'relative, tries {tries.min()} .. {tries.max()}, rows sum to 1 within {rows:.2e}')
    assert near.mean() <= tu.NEAR_BRANCH_CAP
    assert np.array_equal(tries[keep], rtries[keep])
    assert rel_beta <= 1e-12
    assert np.all(err_C <= bound_C)
    assert rows <= K * EPS and np.all(np.isfinite(C)) and np.all(tries < 100)


def test_affinities_on_duplicates_and_an_outlier(jt):
    N, K = 70, 12
    idx = torch.from_numpy(lu.knn_reference(np.random.default_rng(0).standard_normal((N, 3)), K)[0].astype(np.int32))
    C, beta, tries = jt.affinities(idx, torch.zeros(N, K), 4.0)
    print(f'all distances 0: C {C.min().item()} .. {C.max().item()}, tries {tries.min().item()}, beta {beta.max().item():.3e}')
    assert torch.all(C == np.float32(1.0 / K)) and torch.all(tries == 100) and torch.all(torch.isfinite(beta))
    dist = np.sort(np.random.default_rng(1).random((N, K)).astype(np.float32) + 0.5, axis=1)
    dist[7] *= 1e4
    C, beta, tries = jt.affinities(idx, dist, 4.0)
    rC, rbeta, rtries, _, margin = tu.affinity_reference(dist, 4.0)
    print(f'one row 1e4 times farther: its beta {beta[7].item():.3e} ({rbeta[7]:.3e}), tries {tries[7].item()}, margin {margin[7]:.1e}')
    assert torch.all(torch.isfinite(C)) and torch.all(torch.isfinite(beta)) and beta[7].item() > 0
    assert abs(C[7].double().sum().item() - 1) <= K * EPS
    assert margin[7] < tu.NEAR_BRANCH or (tries[7].item() == rtries[7] and abs(beta[7].item() - rbeta[7]) <= 1e-12 * rbeta[7])


def _check_joint(jt, idx, C, P):
    N, K = idx.shape
    idx_h, C_h = idx.cpu().numpy().astype(np.int64), C.cpu().numpy()
    ref = tu.joint_reference(idx_h, C_h)
    S = _scipy(P)
    rowptr, col = P.rowptr.cpu().numpy(), P.col.cpu().numpy()
    assert P.rowptr.dtype == torch.int64 and P.col.dtype == torch.int32 and P.val.dtype == torch.float32
    assert np.array_equal(S.indptr, ref.indptr) and np.array_equal(S.indices, ref.indices)
    rel = np.max(np.abs(S.data - ref.data) / ref.data)
    T = S.T.tocsr()
    T.sort_indices()
    total = float(S.data.sum())
    print(f'N = {N} K = {K}: nnz {S.nnz}, longest row {np.diff(rowptr).max()}, values within {rel:.3e} relative, |sum - 1| '
          f'{abs(total - 1):.2e}')
    assert rel <= 2 * EPS
    assert np.array_equal(T.indices, S.indices) and np.array_equal(T.data, S.data)          # symmetric to the bit
    assert abs(total - 1) <= 1e-6
    order = tu.row_order(idx_h)
    for i in range(N):
        assert list(col[rowptr[i]:rowptr[i + 1]]) == order[i], i
    return rowptr


@pytest.mark.parametrize('N', SIZES)
def test_joint_probabilities(jt, N):
    d = device_case(jt, N)
    _check_joint(jt, d['idx'], d['C'], d['P'])


def test_joint_probabilities_with_a_hub(jt):
    """299 cells on a sphere and its centre: every cell lists the centre, so the centre's row has about 299 entries."""
    from jamie_amd.neighbors import self_knn
    rng = np.random.default_rng(4)
    X = rng.standard_normal((300, 16))
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    X[123] = 0.0
    idx, dist = self_knn(X.astype(np.float32), 30)
    C, _, _ = jt.affinities(idx, dist, 10.0)
    P = jt.joint_from_affinities(idx, C)
    rowptr = _check_joint(jt, idx, C, P)
    print(f'the centre\'s row: {rowptr[124] - rowptr[123]} entries')
    assert rowptr[124] - rowptr[123] > 256
    Y = rng.standard_normal((300, 2)).astype(np.float32)
    _, _, _, parts = jt.gradient(P, Y, return_parts=True)
    err = tu.gradient_errors({'A': parts['A'].cpu().numpy(), 'R': parts['R'].cpu().numpy(), 'z': parts['z'].cpu().numpy(), 'Z': 0, 'KL': 0},
                             dict(tu.gradient_reference(_scipy(P), Y), Z=0, KL=0, KL_mag=1))
    print(f'attraction over the long row within {err["A"]:.3e}')
    assert err['A'] <= tu.GRAD_TOL


def _device_gradient(jt, P, Y, alpha=1.0, seg_rows=0):
    grad, Z, KL, parts = jt.gradient(P, Y, alpha, seg_rows, return_parts=True)
    return {'grad': grad.cpu().numpy(), 'Z': Z, 'KL': KL, 'A': parts['A'].cpu().numpy(), 'R': parts['R'].cpu().numpy(),
            'z': parts['z'].cpu().numpy()}


def _check_gradient(got, ref, alpha, what):
    err = tu.gradient_errors(got, ref)
    g_ref = 4.0 * (alpha * ref['A'] - ref['R'] / ref['Z'])
    g_mag = 4.0 * (alpha * ref['A_mag'] + ref['R_mag'] / ref['Z'])
    # (R / Z carries the error of R and of Z; the gradient is rounded to fp32 once)
    g_bound = 2 * tu.GRAD_TOL * g_mag + EPS * np.abs(g_ref) + 1e-300
    g_err = np.abs(got['grad'] - g_ref)
    colsum = np.abs(got['grad'].astype(np.float64).sum(axis=0))
    print(f'{what}: ' + ', '.join(f'{k} {v:.3e}' for k, v in err.items()) + f'; gradient at {np.max(g_err / g_bound):.3f} of its bound, '
          f'column sums at {np.max(colsum / g_bound.sum(axis=0)):.3f} of theirs')
    assert np.all(np.isfinite(got['grad'])) and np.isfinite(got['Z']) and np.isfinite(got['KL'])
    assert max(err.values()) <= tu.GRAD_TOL
    assert np.all(g_err <= g_bound)
    assert np.all(colsum <= g_bound.sum(axis=0))
    return err


@pytest.mark.parametrize('N', SIZES)
def test_gradient_against_float64(jt, N):
    """Three layouts at every size.  The sizes up to 1000 are one block of rows and one staged chunk per segment; 2600 is three
    blocks of rows, chunks that hold no row of their workgroup, and at tsne_util.SEG_ROWS_LONG segments of several chunks."""
    d = device_case(jt, N)
    c = tu.shape_case(N)
    S = _scipy(d['P'])
    states = [('zero', np.zeros((N, 2), np.float32)), ('init', jt.initial_layout(c['X'], 'pca', 0)), ('spread', tu.spread_layout(N))]
    worst = 0.0
    for name, Y in states:
        ref = tu.gradient_reference(S, Y)
        first = None
        for seg in tu.seg_rows_of(N):
            got = _device_gradient(jt, d['P'], Y, 1.0, seg)
            again = _device_gradient(jt, d['P'], Y, 1.0, seg)
            for k in ('grad', 'A', 'R', 'z'):
                assert np.array_equal(got[k], again[k]), (name, seg, k)
            assert got['Z'] == again['Z'] and got['KL'] == again['KL']
            worst = max(worst, *_check_gradient(got, ref, 1.0, f'N = {N} {name} seg_rows = {seg}').values())
            if name == 'zero':
                assert got['Z'] == N * (N - 1) and np.all(got['R'] == 0) and np.all(got['z'] == N - 1)
            if first is None:
                first = got
            else:
                assert np.all(np.abs(got['R'] - first['R']) <= 2 * tu.GRAD_TOL * ref['R_mag'])
                assert abs(got['Z'] - first['Z']) <= 2 * tu.GRAD_TOL * ref['Z']
    Y = states[-1][1]
    _check_gradient(_device_gradient(jt, d['P'], Y, 12.0), tu.gradient_reference(S, Y), 12.0, f'N = {N} exaggeration 12')
    print(f'N = {N}: largest relative error {worst:.3e}, GRAD_TOL {tu.GRAD_TOL:.3e}')


def test_gradient_with_coincident_points(jt):
    N = 130
    d = device_case(jt, N)
    Y = jt.initial_layout(tu.shape_case(N)['X'], 'pca', 0) * np.float32(1e4)
    Y[20:25] = Y[20]
    got = _device_gradient(jt, d['P'], Y)
    ref = tu.gradient_reference(_scipy(d['P']), Y)
    _check_gradient(got, ref, 1.0, 'five copies of one point among 130')
    others = np.delete(np.arange(N), np.arange(20, 25))
    w = 1.0 / (1.0 + ((Y[20].astype(np.float64) - Y[others].astype(np.float64)) ** 2).sum(axis=1))
    print(f'z of a copy {got["z"][20]:.9f}; 4 + the other cells {4 + w.sum():.9f}')
    assert abs(got['z'][20] - (4 + w.sum())) <= tu.GRAD_TOL * (4 + w.sum())


def _numpy_update(Y, u, gain, g, momentum, lr):
    """Step 5 in fp32 numpy; also the magnitude one rounding of u's longer operand has (a contracted fma rounds once)."""
    f = np.float32
    gain = np.where(u * g < 0, gain + f(0.2), gain * f(0.8)).astype(f)
    gain = np.maximum(gain, f(0.01))
    a, b = f(momentum) * u, f(lr) * (gain * g)
    u2 = (a - b).astype(f)
    return (Y + u2).astype(f), u2, gain, np.maximum(np.abs(a), np.abs(b))


def test_step_equals_the_fp32_restatement(jt):
    N = 257
    d = device_case(jt, N)
    rng = np.random.default_rng(9)
    Y0 = tu.spread_layout(N)
    u0 = (rng.standard_normal((N, 2)) * 0.1).astype(np.float32)
    u0[::7] = 0.0                                           # u g == 0: the gain shrinks
    gain0 = (0.01 + rng.random((N, 2)) * 2).astype(np.float32)
    alpha, momentum, lr = 12.0, 0.5, 50.0
    g = jt.gradient(d['P'], Y0, alpha)[0].cpu().numpy()
    Y, u, gain = (torch.from_numpy(a.copy()).cuda() for a in (Y0, u0, gain0))
    jt.descend(d['P'], Y, u, gain, [(alpha, momentum)], lr)
    rY, ru, rgain, big = _numpy_update(Y0, u0, gain0, g, momentum, lr)
    ulp_u = np.spacing(np.maximum(big, np.abs(ru)).astype(np.float32))
    ulp_y = np.spacing(np.maximum(np.abs(Y0), np.abs(rY)).astype(np.float32))
    du, dy = np.abs(u.cpu().numpy() - ru), np.abs(Y.cpu().numpy() - rY)
    print(f'one step: gain equal {np.array_equal(gain.cpu().numpy(), rgain)}, u within {np.max(du / ulp_u):.2f} ulp, y within '
          f'{np.max(dy / (ulp_y + ulp_u)):.2f} of an ulp of y and one of u; {int((u0 * g == 0).sum())} elements with u g == 0')
    assert (u0 * g == 0).sum() > 0
    assert np.array_equal(gain.cpu().numpy(), rgain)
    assert np.all(du <= ulp_u) and np.all(dy <= ulp_y + ulp_u)


def test_exaggeration_ends_at_exaggeration_iter(jt):
    """Three iterations with exaggeration_iter = 1: bit-identical to one iteration at (12, 0.5) and two at (1, 0.8) issued one by
    one, and the logged gradient norms are those of the gradient with the exaggeration of the NEXT iteration."""
    N = 130
    d = device_case(jt, N)
    Y0 = jt.initial_layout(tu.shape_case(N)['X'], 'pca', 0)
    phases, logged_at = jt.schedule(3, 1, 12.0, 1)
    assert phases == [(12.0, 0.5), (1.0, 0.8), (1.0, 0.8)] and logged_at == [1, 2, 3]

    def start():
        return torch.from_numpy(Y0.copy()).cuda(), torch.zeros(N, 2, device='cuda'), torch.ones(N, 2, device='cuda')
    Y, u, gain = start()
    hist = jt.descend(d['P'], Y, u, gain, phases, 50.0, logged_at).cpu().numpy()
    Ys, us, gains = start()
    norms = []
    for alpha, momentum in phases:
        jt.descend(d['P'], Ys, us, gains, [(alpha, momentum)], 50.0)
        norms.append(float((jt.gradient(d['P'], Ys, 1.0)[0].double() ** 2).sum().item()))
    Yw, uw, gainw = start()
    jt.descend(d['P'], Yw, uw, gainw, [(12.0, 0.5)] * 3, 50.0)
    print(f'squared gradient norms logged {hist[1]}, recomputed at exaggeration 1 {norms}')
    assert torch.equal(Y, Ys) and torch.equal(u, us) and torch.equal(gain, gains)
    assert not torch.equal(Y, Yw)
    assert np.allclose(hist[1], norms, rtol=1e-12, atol=0)


def test_end_to_end_on_four_blobs(jt):
    from sklearn.manifold import trustworthiness
    from jamie_amd.neighbors import self_knn
    emb, lab = tu.blobs()
    X, labels = np.concatenate(emb), np.concatenate(lab)
    kw = dict(n_iter=300, exaggeration_iter=100, log_every=50, init='random')
    host = [tu.host_run(seed) for seed in (0, 1, 2)]
    host_kl = [h['kl'] for h in host]
    host_tw = [trustworthiness(X, np.concatenate(h['layout']), n_neighbors=10) for h in host]
    spread = (max(host_kl) - min(host_kl)) / min(host_kl)
    spread_tw = max(host_tw) - min(host_tw)
    print(f'host route: final KL {host_kl} (relative spread {spread:.3e}), trustworthiness {host_tw}')
    idx, dist = self_knn(X, 90)
    S = _scipy(jt.joint_probabilities(idx, dist, 30.0))
    for seed in (0, 1, 2):
        out = jt.tsne(emb, seed=seed, **kw)
        Y = np.concatenate(out['layout'])
        ref = tu.gradient_reference(S, Y)
        p, tw = tu.purity(Y, labels), trustworthiness(X, Y, n_neighbors=10)
        print(f'seed {seed}: KL {out["kl"]:.9f} (float64 on its layout {ref["KL"]:.9f}; host route {host_kl[seed]:.9f}), KL history '
              f'{np.round(out["kl_history"], 4)}, |grad| {out["grad_norm_history"][-1]:.2e}, purity {p}, trustworthiness {tw:.5f}')
        assert [a.shape for a in out['layout']] == [(200, 2), (200, 2)] and out['layout'][0].dtype == np.float32
        assert list(out['logged_at']) == [50, 100, 150, 200, 250, 300] and out['n_neighbors'] == 90 and out['learning_rate'] == 50.0
        assert out['kl'] == out['kl_history'][-1] and np.all(np.isfinite(Y))
        assert abs(out['kl'] - ref['KL']) <= tu.GRAD_TOL * ref['KL_mag']
        assert out['kl'] <= host_kl[seed] * (1 + 3 * spread)
        assert tu.purity(np.concatenate(host[seed]['layout']), labels) == 1.0 and p >= 0.99
        assert tw >= min(host_tw) - spread_tw
    again = jt.tsne(emb, seed=2, **kw)
    assert all(np.array_equal(a, b) for a, b in zip(again['layout'], out['layout']))
    assert np.array_equal(again['kl_history'], out['kl_history']) and np.array_equal(again['grad_norm_history'], out['grad_norm_history'])


def test_memory_at_20000_cells(jt):
    """20 000 pooled cells, L = 32, K = 90, two iterations: peak device memory above the resident inputs under a quarter of an
    N x N fp32 matrix (1.6 GB)."""
    emb, _ = lu.mixture(21, 6, 32, (10000, 10000), shift=0.0)
    xs = [torch.from_numpy(e).cuda() for e in emb]
    N = 20000
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = jt.tsne(xs, n_iter=2, exaggeration_iter=1, init='random')
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    print(f'device memory above the resident inputs {extra / 2 ** 20:.1f} MiB; a quarter of N x N fp32 {N * N / 2 ** 20:.1f} MiB; KL '
          f'{out["kl"]:.4f}')
    assert extra < N * N * 4 / 4
    assert out['n_neighbors'] == 90 and np.isfinite(out['kl']) and [a.shape for a in out['layout']] == [(10000, 2), (10000, 2)]


def test_facade_routes_return_the_same_keys(jt):
    from jamie_amd import JAMIE
    emb, _ = tu.blobs()
    kw = dict(n_iter=20, exaggeration_iter=10, log_every=5, perplexity=10)
    dev = JAMIE(metrics='device').tsne(emb, **kw)
    host = JAMIE(metrics='host').tsne(emb, **kw)
    assert set(dev) == set(host) == {'layout', 'kl', 'kl_history', 'grad_norm_history', 'logged_at', 'n_neighbors', 'learning_rate',
                                     'n_iter'}
    for k in dev:
        a, b = dev[k], host[k]
        if k == 'layout':
            assert [x.shape for x in a] == [x.shape for x in b] and all(x.dtype == y.dtype for x, y in zip(a, b))
        else:
            assert np.shape(a) == np.shape(b) and type(a) is type(b), k
    assert np.array_equal(dev['logged_at'], host['logged_at']) and dev['n_neighbors'] == host['n_neighbors'] == 30
    # the first logged layout is five iterations from identical bits: the two routes still agree closely there
    print(f'KL after 5 iterations: device {dev["kl_history"][0]:.9f}, host {host["kl_history"][0]:.9f}')
    assert abs(dev['kl_history'][0] - host['kl_history'][0]) <= 1e-4 * abs(host['kl_history'][0])

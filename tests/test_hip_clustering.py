"""Clustering on the device (jamie_amd/clustering.py, csrc/clustering.hip) against the float64 reference and the numpy restatement
of clustering_util.py.

One step: no cell may sit at a centre that float64 puts more than band(L) = 4 (L + 2) 2^-24 (relative) behind the nearest, the
label is the float64 argmin wherever the two nearest centres are further apart than that, and at most 1 % of the cells may be
closer than that; sums against `math.fsum`, centres within one fp32 ulp of the rounded exact mean, inertia within (L + 3) 2^-24,
counts and changed labels exactly.  Integer-valued data: labels, minq and the seeding picks bit for bit.  Whole runs: the device
route equals the host route in clusters, iterations, winning run and sizes on the cases whose margin test_host_clustering.py
asserts.  Every figure is printed before it is asserted.  Measured on an MI355X: no cell inside the band on any case, sums equal
to fsum, centres 0 ulp off, largest relative inertia error 7.2e-9, whole runs equal to the host route with centres within 5.2e-8."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clustering_util as cu  # noqa: E402
import lisi_util as lu  # noqa: E402

pytestmark = pytest.mark.gpu

K_VALUES = (1, 2, 5, 17, 128, 129, 300)        # one centre tile, the 128 | 129 seam, more than two tiles (k = N on a 300-cell slice)
SEGS = (0, 128, 256)


@pytest.fixture(scope='module')
def jc():
    from jamie_amd import clustering
    return clustering


def _host(out):
    return {name: t.cpu().numpy() for name, t in out.items()}


def _check_step(X, C, prev, out, k):
    """Everything one step forms, against float64 on the same fp32 cells and centres."""
    N, L = X.shape
    lab, minq, stats = out['labels'].astype(np.int64), out['minq'], out['stats']
    q = cu.q_float64(X, C)
    assert lab.min() >= 0 and lab.max() < k
    own = q[np.arange(N), lab]
    best = q.min(axis=1)
    band = cu.band(L)
    worst = np.max((own - best) / np.where(best > 0, best, 1.0))
    if k > 1:
        two = np.partition(q, 1, axis=1)[:, :2]
        inside = (two[:, 1] - two[:, 0]) <= band * two[:, 1]
    else:
        inside = np.zeros(N, bool)
    differ = lab != np.argmin(q, axis=1)
    print(f'N={N} L={L} k={k}: cells inside the band {inside.mean():.4f}, labels off the float64 argmin {int(differ.sum())} '
          f'(outside the band {int((differ & ~inside).sum())}), worst q behind the nearest {worst:.2e} (band {band:.2e})')
    assert np.all(own <= best * (1 + band))
    assert not np.any(differ & ~inside)
    assert inside.mean() <= 0.01
    assert np.all(np.abs(minq.astype(np.float64) - own) <= (L + 3) * cu.U32 * own)
    # counts, changed labels, empty clusters: exact
    counts = np.bincount(lab, minlength=k)
    assert np.array_equal(out['counts'], counts)
    assert stats[2] == np.count_nonzero(prev != lab) and stats[3] == np.count_nonzero(counts == 0)
    # sums against math.fsum by cluster, centres within one fp32 ulp of the rounded exact mean
    X64 = X.astype(np.float64)
    worst_sum, worst_ulp = 0.0, 0.0
    for j in range(k):
        rows = X64[lab == j]
        if len(rows) == 0:
            assert not out['sums'][j].any() and np.array_equal(out['centers'][j], C[j])
            continue
        exact = np.array([math.fsum(col) for col in rows.T])
        slack = len(rows) * 2.0 ** -52 * np.abs(rows).sum(axis=0)
        err = np.abs(out['sums'][j] - exact)
        assert np.all(err <= slack), j
        worst_sum = max(worst_sum, float(np.max(err / np.where(slack > 0, slack, 1.0))))
        mean = (exact / len(rows)).astype(np.float32)
        ulp = np.abs(out['centers'][j].astype(np.float64) - mean.astype(np.float64)) / np.spacing(np.abs(mean)).astype(np.float64)
        assert np.all(ulp <= 1.0), j
        worst_ulp = max(worst_ulp, float(ulp.max()))
    inertia = math.fsum(own)
    rel = abs(stats[0] - inertia) / inertia if inertia > 0 else abs(stats[0])
    print(f'    sums: largest error {worst_sum:.2e} of the allowance; centres: {worst_ulp:.2f} ulp; inertia: relative error '
          f'{rel:.2e} (bound {(L + 3) * cu.U32:.2e})')
    assert abs(stats[0] - inertia) <= cu.inertia_bound_same_centres(L, inertia)
    shift = float(((out['centers'].astype(np.float64) - C.astype(np.float64)) ** 2).sum())
    assert abs(stats[1] - shift) <= 1e-12 * max(shift, 1e-300)
    return rel


@pytest.mark.parametrize('which', range(len(lu.SHAPES)))
def test_one_step_against_float64(jc, which):
    X = cu.case_data(which, 0)[2]
    rng = np.random.default_rng(40 + which)
    worst = 0.0
    for n, k in enumerate(K_VALUES):
        x = X[:300] if k == 300 else X
        C = x[rng.permutation(len(x))[:k]].copy()
        if 1 < k < 300:
            C += (0.05 * rng.standard_normal(C.shape)).astype(np.float32)
        prev = rng.integers(0, k, len(x)).astype(np.int32)
        seg = SEGS[(n + which) % 3]
        out = _host(jc.step(x, C, labels=prev, seg_rows=seg))
        worst = max(worst, _check_step(x, C, prev, out, k))
        for other in SEGS:
            if other != seg and k in (5, 129):
                again = _host(jc.step(x, C, labels=prev, seg_rows=other))
                assert np.array_equal(again['labels'], out['labels']) and np.array_equal(again['minq'], out['minq'])
                assert np.array_equal(again['counts'], out['counts'])
        lab, minq = jc.assign(x, C, seg_rows=seg)
        assert np.array_equal(lab.cpu().numpy(), out['labels']) and np.array_equal(minq.cpu().numpy(), out['minq'])
    print(f'largest relative inertia error: {worst:.2e}')


@pytest.mark.parametrize('L', [3, 8])
def test_integer_data_bit_for_bit(jc, L):
    X = lu.integer_cells(n=900, L=L)
    X64 = X.astype(np.float64)
    rng = np.random.default_rng(L)
    for k in (1, 6, 40, 130):
        picks = rng.integers(0, len(X), k)
        picks[k // 2:] = picks[:k - k // 2]                 # duplicate centres: every tie goes to the lower index
        C = X[picks]
        q = cu.q_float64(X, C)
        for seg in SEGS:
            out = _host(jc.step(X, C, seg_rows=seg))
            assert np.array_equal(out['labels'], np.argmin(q, axis=1)), (k, seg)
            assert np.array_equal(out['minq'], q.min(axis=1).astype(np.float32)), (k, seg)
            assert out['stats'][0] == q.min(axis=1).sum() and out['stats'][2] == len(X)
            sums = np.zeros((k, L))
            np.add.at(sums, out['labels'], X64)
            assert np.array_equal(out['sums'], sums)
        if k > 1:
            assert out['labels'].max() < k // 2            # (k is even: the second half repeats the first)
        # the seeding: np.cumsum's picks
        u = rng.random(k)
        _, got = jc.kmeans_plusplus(X, k, u)
        assert np.array_equal(got, cu.seeds(X64, u, False)) and np.array_equal(got, cu.seeds(X, u, True)), k
    # all cells identical: total == 0, the pick is floor(u N)
    same = np.tile(X[:1], (2500, 1))
    u = np.array([0.5, 0.0, 0.37, 0.9999])
    centres, got = jc.kmeans_plusplus(same, 4, u)
    assert np.array_equal(got, (u * 2500).astype(np.int64)) and np.array_equal(centres.cpu().numpy(), same[:4])
    out = _host(jc.step(same, same[:4]))
    assert not out['labels'].any() and not out['minq'].any() and out['stats'][3] == 3


def test_weighted_pick_in_the_stated_order(jc):
    from jamie_amd import _native as nv
    rng = np.random.default_rng(2)
    pick = torch.zeros(1, dtype=torch.int64, device='cuda')
    for n in (1, 700, 1024, 1025, 5000):
        w = (rng.random(n) ** 4).astype(np.float32)
        w[rng.integers(0, n, n // 4)] = 0
        w_d = torch.from_numpy(w).cuda()
        ws = torch.empty(8 * ((n + 1023) // 1024), dtype=torch.uint8, device='cuda')
        for u in list(rng.random(12)) + [0.0, 1.0 - 2.0 ** -53]:
            nv.weighted_pick(w_d, u, pick, ws)
            assert int(pick.item()) == cu.pick_restated(w, u), (n, u)
    with pytest.raises(nv.JamieHipError):
        nv.weighted_pick(w_d, 1.0, pick, ws)
    with pytest.raises(nv.JamieHipError):
        nv.weighted_pick(w_d, 0.5, pick, ws[:8])


def test_edge_cases(jc):
    emb, lab, X = cu.case_data(1, 0)
    rng = np.random.default_rng(6)
    # a centre far from every cell: empty, unchanged, and no NaN anywhere
    C = X[rng.permutation(len(X))[:6]].copy()
    C[3] = 1e6
    out = _host(jc.step(X, C))
    assert out['stats'][3] == 1 and out['counts'][3] == 0 and np.array_equal(out['centers'][3], C[3])
    assert all(np.isfinite(out[name]).all() for name in ('centers', 'sums', 'minq', 'stats'))
    _check_step(X, C, np.full(len(X), -1), out, 6)
    km = jc.kmeans(X, 6, init=C, max_iter=50)
    assert km['n_empty'] == 1 and km['sizes'][3] == 0 and np.array_equal(km['centers'][3], C[3].astype(np.float64))
    assert np.isfinite(km['centers']).all() and np.isfinite(km['inertia'])
    # a cluster of one cell: its centre is the cell
    Y = X.copy()
    Y[100] = 500.0
    C = np.concatenate([Y[100:101], X[rng.permutation(len(X))[:4]]])
    out = _host(jc.step(Y, C))
    assert out['counts'][0] == 1 and out['labels'][100] == 0 and np.array_equal(out['centers'][0], Y[100])
    # N = k: every cell its own cluster
    Z = X[:200]
    out = _host(jc.step(Z, Z))
    assert np.array_equal(out['labels'], np.arange(200)) and not out['minq'].any() and np.array_equal(out['centers'], Z)
    km = jc.kmeans(Z, 200, n_init=1)
    assert km['inertia'] >= 0 and km['sizes'].sum() == 200 and km['n_empty'] == (km['sizes'] == 0).sum()
    # L = 1
    W = X[:, :1].copy()
    C = W[rng.permutation(len(W))[:9]].copy()
    out = _host(jc.step(W, C, seg_rows=256))
    _check_step(W, C, np.full(len(W), -1), out, 9)
    # L >= 256: one owner group that strides over the features; the table in LDS (k = 3) and in the workspace (k = 20)
    V = np.random.default_rng(9).standard_normal((333, 260)).astype(np.float32)
    for k in (3, 20):
        C = V[rng.permutation(len(V))[:k]] + np.float32(0.1)
        out = _host(jc.step(V, C, seg_rows=128))
        _check_step(V, C, np.full(len(V), -1), out, k)
    # one cell
    out = _host(jc.step(X[:1], X[:1]))
    assert out['labels'][0] == 0 and out['counts'][0] == 1


@pytest.mark.parametrize('case', cu.CASES)
def test_whole_runs_device_vs_host(case, capsys):
    from jamie_amd import JAMIE
    which, k, seed = case
    emb, lab, X = cu.case_data(which, seed)
    host = JAMIE().test_clustering(emb, lab, n_clusters=k, n_init=cu.N_INIT, seed=seed)
    capsys.readouterr()
    dev = JAMIE(metrics='device').test_clustering(emb, lab, n_clusters=k, n_init=cu.N_INIT, seed=seed)
    lines = capsys.readouterr().out.strip().splitlines()[-2:]
    assert lines == [f"ARI: {dev['ari']}", f"NMI: {dev['nmi']}"]
    rel_c = np.max(np.abs(dev['centers'] - host['centers'])) / np.max(np.abs(host['centers']))
    print(f"n_iter {dev['n_iter']} / {host['n_iter']}, run {dev['run']} / {host['run']}, centres differ by {rel_c:.2e} of the "
          f"largest, inertia by {abs(dev['inertia'] - host['inertia']) / host['inertia']:.2e}")
    assert all(a.dtype == np.int32 and np.array_equal(a, b) for a, b in zip(dev['clusters'], host['clusters']))
    assert dev['n_iter'] == host['n_iter'] and dev['run'] == host['run'] and np.array_equal(dev['sizes'], host['sizes'])
    assert dev['converged'] == host['converged'] and dev['n_empty'] == host['n_empty']
    assert dev['centers'].dtype == np.float64 and rel_c <= 1e-6
    assert abs(dev['ari'] - host['ari']) <= 1e-12 and abs(dev['nmi'] - host['nmi']) <= 1e-12
    assert np.array_equal(dev['contingency'], host['contingency'])
    assert np.array_equal(dev['modality_contingency'], host['modality_contingency'])
    assert np.array_equal(dev['labels'], host['labels'])
    centre_sq = float((host['centers'][np.concatenate(host['clusters'])] ** 2).sum())
    assert abs(dev['inertia'] - host['inertia']) <= cu.inertia_bound_rounded_centres(X.shape[1], host['inertia'], centre_sq)


@pytest.mark.parametrize('case', [cu.CASES[1], cu.CASES[6], cu.CASES[11]])
def test_runs_are_bit_identical(jc, case):
    """Labels, iterations and the winning run do not depend on seg_rows; the centres' last fp32 bit may (the fp64 sums are grouped
    by segment), and two runs with the same seg_rows are the same bits throughout."""
    which, k, seed = case
    X = cu.case_data(which, seed)[2]
    x = torch.from_numpy(X).cuda()
    first = jc.kmeans(x, k, n_init=cu.N_INIT, seed=seed)
    again = jc.kmeans(x, k, n_init=cu.N_INIT, seed=seed)
    for name in ('labels', 'centers', 'sizes', 'seeds'):
        assert np.array_equal(first[name], again[name]), name
    assert (first['inertia'], first['n_iter'], first['run']) == (again['inertia'], again['n_iter'], again['run'])
    for seg in (128, 384):
        other = jc.kmeans(x, k, n_init=cu.N_INIT, seed=seed, seg_rows=seg)
        assert np.array_equal(other['labels'], first['labels']) and other['n_iter'] == first['n_iter']
        assert other['run'] == first['run'] and np.array_equal(other['sizes'], first['sizes'])
        c32 = first['centers'].astype(np.float32)
        ulp = np.abs(other['centers'] - first['centers']) / np.spacing(np.abs(c32)).astype(np.float64)
        print(f'seg_rows {seg}: centres differ from seg_rows 0 by at most {ulp.max():.1f} fp32 ulp')
        assert ulp.max() <= 1.0


def test_stopping_at_the_iteration_that_met_the_rule(jc):
    """The device enqueues iterations in batches of 8; the result is the state of the stopping iteration, not of the batch's end."""
    seen = set()
    for which, k, seed in cu.CASES[:8]:
        X = cu.case_data(which, seed)[2]
        u = np.random.default_rng([seed, 0]).random(k)
        init = X[cu.seeds(X, u, True)]
        for tol in (1e-4, 0.0):
            tol_abs = tol * float(np.mean(np.var(X.astype(np.float64), axis=0)))
            want = cu.lloyd(X, init.copy(), 300, tol_abs, True)
            got = jc.kmeans(X, k, init=init, max_iter=300, tol=tol)
            print(f"case {(which, k, seed)} tol {tol:g}: n_iter {got['n_iter']} (restated {want['n_iter']})")
            assert got['n_iter'] == want['n_iter'] and got['converged'] and want['converged']
            assert np.array_equal(got['labels'], want['labels']) and np.array_equal(got['sizes'], want['sizes'])
            c32 = want['centers']
            ulp = np.abs(got['centers'] - c32.astype(np.float64)) / np.spacing(np.abs(c32)).astype(np.float64)
            assert ulp.max() <= 1.0                          # C_{t + 1} of the stopping iteration
            # (both are within the bound of the float64 inertia under the unrounded centres)
            centre_sq = float((c32.astype(np.float64)[want['labels']] ** 2).sum())
            assert abs(got['inertia'] - want['inertia']) <= 2 * cu.inertia_bound_rounded_centres(X.shape[1], want['inertia'], centre_sq)
            seen.add(got['n_iter'] % 8)
            # cut short: max_iter below the stopping iteration is reached exactly and reported as not converged
            if want['n_iter'] > 3:
                cut = jc.kmeans(X, k, init=init, max_iter=want['n_iter'] - 2, tol=tol)
                assert cut['n_iter'] == want['n_iter'] - 2 and not cut['converged']
        one = jc.kmeans(X, k, init=init, max_iter=1)
        lab, _ = jc.assign(X, init)
        assert one['n_iter'] == 1 and not one['converged'] and np.array_equal(one['labels'], lab.cpu().numpy())
        loose = jc.kmeans(X, k, init=init, tol=1e9)
        assert loose['n_iter'] == 1 and loose['converged'] and np.array_equal(loose['labels'], one['labels'])
    assert len(seen) > 2                                   # (stops at several places inside a batch)


def test_contingency(jc):
    from jamie_amd import _native as nv
    rng = np.random.default_rng(10)
    for N, na, nb in ((1, 1, 1), (63, 1, 7), (1000, 9, 1), (4099, 40, 5), (20001, 1024, 3)):
        a, b = rng.integers(0, na, N), rng.integers(0, nb, N)
        got = jc.contingency(a, b, na, nb)
        assert got.dtype == np.int64 and np.array_equal(got, cu.contingency_reference(a, b, na, nb))
        assert np.array_equal(jc.contingency(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), na, nb), got)
    a, b = rng.integers(0, 5, 300), rng.integers(0, 4, 300)
    for i, (x, y) in enumerate(((5, 0), (-1, 0), (0, 4), (0, -1))):
        a2, b2 = a.copy(), b.copy()
        a2[17 * i], b2[17 * i] = x, y
        with pytest.raises(ValueError):
            jc.contingency(a2, b2, 5, 4)
    # the launch adds nothing for the pair it reports
    a2 = a.copy()
    a2[3] = 9
    table = torch.zeros(5, 4, dtype=torch.int64, device='cuda')
    flag = torch.zeros(1, dtype=torch.int32, device='cuda')
    nv.contingency(torch.from_numpy(a2).cuda().int(), torch.from_numpy(b).cuda().int(), 5, 4, table, flag)
    keep = np.arange(300) != 3
    assert int(flag.item()) == 1 and np.array_equal(table.cpu().numpy(), cu.contingency_reference(a[keep], b[keep], 5, 4))
    with pytest.raises(ValueError):
        jc.contingency(a, b[:-1], 5, 4)
    with pytest.raises(ValueError):
        jc.contingency(a, b, 0, 4)


def test_refusals_before_allocating(jc):
    from jamie_amd import JAMIE
    from jamie_amd import _native as nv
    x = torch.zeros(100, 4, device='cuda')
    C = torch.zeros(5, 4, device='cuda')
    big = torch.zeros(101, 4, device='cuda')
    labels = torch.zeros(100, dtype=torch.int32, device='cuda')
    counts = torch.zeros(1025, dtype=torch.int64, device='cuda')
    stats = torch.zeros(4, dtype=torch.float64, device='cuda')
    state = torch.zeros(4, dtype=torch.int32, device='cuda')
    ws = torch.empty(1 << 20, dtype=torch.uint8, device='cuda')
    bad = np.zeros((100, 4), np.float32)
    bad[3, 2] = np.nan
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    for kw in (dict(n_clusters=0), dict(n_clusters=101), dict(n_clusters=5, n_init=0), dict(n_clusters=5, max_iter=0),
               dict(n_clusters=5, tol=-1.0), dict(n_clusters=5, init=np.zeros((4, 4))), dict(n_clusters=5, seg_rows=100)):
        with pytest.raises(ValueError):
            jc.kmeans(x, **kw)
    with pytest.raises(ValueError):
        jc.step(x, C, seg_rows=64)
    # the ABI refuses them too, before a launch
    with pytest.raises(nv.JamieHipError):
        nv.kmeans_step(x, big, labels, counts, stats, state, ws)                         # k > N
    with pytest.raises(nv.JamieHipError):
        nv.kmeans_step(x, C[:0], labels, counts, stats, state, ws)                       # k = 0
    with pytest.raises(nv.JamieHipError):
        nv.kmeans_step(x[:, :0], C[:, :0], labels, counts, stats, state, ws)             # L = 0
    with pytest.raises(nv.JamieHipError):
        nv.kmeans_step(x, C, labels, counts, stats, state, ws, seg_rows=100)
    with pytest.raises(nv.JamieHipError):
        nv.kmeans_step(x, C, labels, counts, stats, state, ws[:nv.kmeans_workspace(100, 4, 5) - 1])
    with pytest.raises(nv.JamieHipError):
        nv.kmeans_step(x, C, labels, counts, stats, state, ws, max_iter=0)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() == before
    assert not state.cpu().numpy().any()
    with pytest.raises(ValueError):
        jc.kmeans(bad, 5)
    with pytest.raises(ValueError):
        JAMIE(metrics='device').test_clustering([bad], n_clusters=5)


def test_memory_at_20000_cells(jc):
    """20 000 pooled cells, L = 32, k = 40: peak device memory above the resident inputs under the pooled copy + the workspace
    formula + 16 bytes per cell (labels twice, minq, slack) + 64 MiB (the fp64 row chunks of the variance; nothing N x k, which
    would be 3.2 MB here and 1 GB at 10^6 cells and k = 256)."""
    from jamie_amd import _native as nv
    emb, lab = lu.mixture(21, 40, 32, (10000, 10000), spread=0.4)
    xs = [torch.from_numpy(e).cuda() for e in emb]
    N, L, k = 20000, 32, 40
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = jc.clustering(xs, lab, n_init=2)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    budget = N * L * 4 + nv.kmeans_workspace(N, L, k) + 16 * N + 64 * 2 ** 20
    print(f"device memory above the resident inputs {extra / 2 ** 20:.1f} MiB, budget {budget / 2 ** 20:.1f} MiB; n_iter "
          f"{out['n_iter']}, ARI {out['ari']:.4f}, NMI {out['nmi']:.4f}")
    assert extra < budget
    assert out['centers'].shape == (k, L) and out['sizes'].sum() == N and out['ari'] > 0.5

"""The spectral embedding on the device (jamie_amd/spectral.py, csrc/spectral.hip) against float64 numpy (spectral_util.py).

Kernels, element by element: the row sum and the step equal their numpy restatement to the bit and the step is within
(len + 8) 2^-53 of the sum of its terms' magnitudes against an extended-precision sum; the Gram matrix within (chain + segments)
2^-53 of sum |y z|, equal bits from run to run, symmetric to the bit for Y == Z; the rotation within (B + 2) 2^-53.  Solver: the
derived checks (a) .. (f) of spectral_util.check_solution against `numpy.linalg.eigh` of the dense S built in float64 from the
device's own graph.  Routes, facade, memory.  Every figure is printed before it is asserted."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spectral_util as su  # noqa: E402
import umap_util as uu  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-8
KERNEL_CASES = ('cells16', 'cells17', 'cells40', 130, 257, 600, 1000, 'hub', 'special')
COEFF = (1.7, -0.3, 0.6)


@pytest.fixture(scope='module')
def jsp():
    from jamie_amd import spectral
    return spectral


_graphs, _refs = {}, {}


def device_graph(jsp, name):
    """The fuzzy graph of a case on the device, once, as `spectral.spectral` builds it; its arrays on the host."""
    if name not in _graphs:
        if name in su.BLOBS or name in ('sheet', 'apart'):
            emb, nn, _ = su.cells(name)
            X = np.concatenate(emb, axis=0)
        else:
            c = uu.shape_case(name)
            X, nn = c['X'], c['nn']
        G = jsp.build_graph(torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).cuda(), nn)
        _graphs[name] = dict(G=G, rowptr=G.rowptr.cpu().numpy(), col=G.col.cpu().numpy(), val=G.val.cpu().numpy(), nn=nn)
    return _graphs[name]


def device_reference(jsp, name, dn):
    """(lambda descending, V, S) by `numpy.linalg.eigh` of the dense S built in float64 from the device's own graph."""
    if (name, dn) not in _refs:
        d = device_graph(jsp, name)
        S, _, _ = su.dense_operator(d['rowptr'], d['col'], d['val'], dn)
        w, V = np.linalg.eigh(S)
        _refs[(name, dn)] = (w[::-1].copy(), np.ascontiguousarray(V[:, ::-1]), S)
    return _refs[(name, dn)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize('name', KERNEL_CASES)
def test_rowsum_equals_the_restated_sum(jsp, name):
    d = device_graph(jsp, name)
    G = d['G']
    N = G.n
    w = np.random.default_rng(0).uniform(0.5, 2.0, N)
    got, got_w = jsp.rowsum(G).cpu().numpy(), jsp.rowsum(G, dev(w)).cpu().numpy()
    want, want_w = su.restated_rowsum(d['rowptr'], d['col'], d['val']), su.restated_rowsum(d['rowptr'], d['col'], d['val'], w)
    lens = np.diff(d['rowptr'])
    print(f'{name}: N = {N}, rows of {lens.min()} .. {lens.max()} entries, degree {got.min():.4f} .. {got.max():.4f}, '
          f'differs in {int((got != want).sum())} + {int((got_w != want_w).sum())} cells')
    assert got.dtype == np.float64 and np.array_equal(got, want) and np.array_equal(got_w, want_w)
    if name == 'hub':
        assert lens[uu.HUB] == uu.LONGEST_ROW
    for dn in (False, True):
        scale, degree = jsp.normalised_operator(G, dn)
        _, deg_h, scale_h = su.dense_operator(d['rowptr'], d['col'], d['val'], dn)
        rel = max(np.max(np.abs(scale.cpu().numpy() - scale_h) / scale_h), np.max(np.abs(degree.cpu().numpy() - deg_h) / deg_h))
        print(f'   density_normalize = {dn}: scale and degree within {rel:.2e} relative of float64 numpy')
        assert rel <= (lens.max() + 8) * su.U


@pytest.mark.parametrize('B', [16, 32])
@pytest.mark.parametrize('name', KERNEL_CASES)
def test_cheb_step_element_by_element(jsp, name, B):
    d = device_graph(jsp, name)
    G = d['G']
    N = G.n
    rng = np.random.default_rng(1)
    X, prev = rng.standard_normal((N, B)), rng.standard_normal((N, B))
    scale = 1.0 / np.sqrt(su.restated_rowsum(d['rowptr'], d['col'], d['val']))
    al, ga, be = COEFF
    Xd, sd = dev(X), dev(scale)
    out = jsp.cheb_step(G, sd, Xd, dev(prev), torch.empty_like(Xd), al, ga, be).cpu().numpy()
    aliased = dev(prev)
    jsp.cheb_step(G, sd, Xd, aliased, aliased, al, ga, be)
    ref, mag, lens = su.cheb_reference(d['rowptr'], d['col'], d['val'], scale, X, prev, al, ga, be)
    rel = np.abs(out - ref) / mag
    want = su.restated_cheb_step(d['rowptr'], d['col'], d['val'], scale, X, prev, al, ga, be)
    worst = float(np.max(rel / su.cheb_bound(lens)))
    print(f'{name} B = {B}: longest row {lens.max()}, error at most {float(rel.max()) / su.U:.2f} u of the magnitudes, {worst:.3f} of '
          f'the bound (len + 8) u; {int((out != want).sum())} elements differ from the restatement')
    assert np.all(np.isfinite(out)) and np.all(rel <= su.cheb_bound(lens))
    assert np.array_equal(out, want)
    assert np.array_equal(aliased.cpu().numpy(), out)
    plain = jsp.apply(G, sd, Xd).cpu().numpy()
    assert np.array_equal(plain, su.restated_cheb_step(d['rowptr'], d['col'], d['val'], scale, X, None, 1.0, 0.0, 0.0))
    assert torch.equal(Xd, dev(X))                           # the input is left as it was


def test_cheb_step_skips_columns_outside_the_graph(jsp):
    """An entry whose column is outside [0, N) contributes nothing (the kernel reads nothing for it); the Python layer refuses
    such a graph, so the entry point is called directly."""
    from jamie_amd import _native as nv
    d = device_graph(jsp, 130)
    N, B = d['G'].n, 16
    col = d['col'].copy()
    rng = np.random.default_rng(2)
    hit = rng.choice(len(col), 40, replace=False)
    col[hit[:20]], col[hit[20:]] = -1, N
    keep = np.ones(len(col), bool)
    keep[hit] = False
    row = np.repeat(np.arange(N), np.diff(d['rowptr']))
    rowptr = np.zeros(N + 1, np.int64)
    rowptr[1:] = np.cumsum(np.bincount(row[keep], minlength=N))
    X, scale = rng.standard_normal((N, B)), rng.uniform(0.5, 2.0, N)
    out = torch.empty(N, B, dtype=torch.float64, device='cuda')
    nv.graph_cheb_step(d['G'].rowptr, dev(col), d['G'].val, dev(scale), dev(X), None, out, 1.3, 0.2, 0.0)
    want = su.restated_cheb_step(rowptr, d['col'][keep], d['val'][keep], scale, X, None, 1.3, 0.2, 0.0)
    assert np.array_equal(out.cpu().numpy(), want)
    bad = type(d['G'])(d['G'].rowptr, dev(col), d['G'].val, N, d['G'].k)
    with pytest.raises(ValueError, match='spectral'):
        jsp.apply(bad, dev(scale), dev(X))
    with pytest.raises(ValueError, match='spectral'):
        jsp.cheb_step(d['G'], dev(scale), out, None, out, 1.0, 0.0, 0.0)


@pytest.mark.parametrize('B', [16, 32])
@pytest.mark.parametrize('N', [16, 17, 40, 130, 257, 600, 1000, 1537])
def test_gram_and_rotate(jsp, N, B):
    rng = np.random.default_rng(3)
    Y, Z = rng.standard_normal((N, B)) * 10.0 ** rng.uniform(-2, 2, B), rng.standard_normal((N, B))
    Yd, Zd = dev(Y), dev(Z)
    ld = np.longdouble
    G1, G2 = jsp.gram(Yd, Zd).cpu().numpy(), jsp.gram(Yd, Zd).cpu().numpy()
    ref = Y.T.astype(ld) @ Z.astype(ld)
    mag = np.abs(Y).T.astype(ld) @ np.abs(Z).astype(ld)
    segments = -(-N // su.GRAM_ROWS)
    bound = (min(N, su.GRAM_ROWS) + segments) * su.U
    rel = float(np.max(np.abs(G1 - ref) / mag))
    GY = jsp.gram(Yd, Yd).cpu().numpy()
    rel_y = float(np.max(np.abs(GY - Y.T.astype(ld) @ Y.astype(ld)) / (np.abs(Y).T.astype(ld) @ np.abs(Y).astype(ld))))
    print(f'N = {N}, B = {B}: gram within {rel / su.U:.2f} u and {rel_y / su.U:.2f} u (Y == Z) of the magnitudes, bound {bound / su.U:.0f} u')
    assert rel <= bound and rel_y <= bound
    assert np.array_equal(G1, G2)
    assert np.array_equal(GY, GY.T)
    M1, M2 = rng.standard_normal((B, B)), rng.standard_normal((B, B))
    for Y2, Mb in ((None, None), (Z, M2)):
        got = jsp.rotate(Yd, M1, None if Y2 is None else Zd, Mb).cpu().numpy()
        ref = Y.astype(ld) @ M1.astype(ld)
        mag = np.abs(Y).astype(ld) @ np.abs(M1).astype(ld)
        if Y2 is not None:
            ref, mag = ref + Z.astype(ld) @ M2.astype(ld), mag + np.abs(Z).astype(ld) @ np.abs(M2).astype(ld)
        rel = float(np.max(np.abs(got - ref) / mag))
        print(f'   rotate ({1 if Y2 is None else 2} products) within {rel / su.U:.2f} u of the magnitudes, bound {B + 2} u')
        assert rel <= (B + 2) * su.U
    assert np.array_equal(jsp.rotate(Yd, np.eye(B)).cpu().numpy(), Y)
    with pytest.raises(Exception, match='out must differ'):
        jsp.rotate(Yd, M1, out=Yd)


@pytest.mark.parametrize('density_normalize', [False, True])
@pytest.mark.parametrize('name', sorted(su.SOLVER_CASES))
def test_solver_against_eigh_of_the_device_graph(jsp, name, density_normalize):
    d = device_graph(jsp, name)
    lam, V, S = device_reference(jsp, name, density_normalize)
    scale, degree = jsp.normalised_operator(d['G'], density_normalize)
    for k in su.SOLVER_CASES[name]:
        out = jsp.eigen(d['G'], scale, k, tol=TOL, max_iter=100, max_degree=60, seed=0, degree=degree)
        print(f'{name} k = {k}: {out["iterations"]} outer iterations, {out["applies"]} applies, degrees {out["degrees"]}')
        assert out['converged'] and out['iterations'] <= 100                       # (a)
        assert np.all(out['residuals'] <= TOL) and out['vectors'].shape == (d['G'].n, k)
        assert np.all(np.diff(out['eigenvalues']) <= 0)
        Q = jsp.fix_signs(out['vectors'])
        su.check_solution(Q, out['eigenvalues'], S, lam, V, k, jsp.block_width(k), tol=TOL, subspace_only=name == 'apart',
                          tag=f'{name} dn={density_normalize} k={k}')
        if name == 'apart':
            assert np.all(np.abs(out['eigenvalues'][:2] - 1.0) <= TOL)


def test_unconverged_run_says_so(jsp):
    d = device_graph(jsp, 'sheet')
    scale, degree = jsp.normalised_operator(d['G'], False)
    out = jsp.eigen(d['G'], scale, 3, tol=1e-12, max_iter=1, max_degree=4, degree=degree)
    print(out['residuals'], out['degrees'])
    assert not out['converged'] and out['iterations'] == 1 and out['degrees'] == [4] and out['applies'] == 5


@pytest.mark.parametrize('kind', ['laplacian', 'diffmap'])
def test_routes_agree_on_four_blobs(jsp, kind):
    from jamie_amd import JAMIE
    emb, nn, _ = su.cells('blobs4')
    k = 5
    got = JAMIE(metrics='device').spectral(list(emb), n_components=k - 1, kind=kind, return_graph=True)
    host = JAMIE(metrics='host').spectral(list(emb), n_components=k - 1, kind=kind)
    again = JAMIE(metrics='device').spectral(list(emb), n_components=k - 1, kind=kind)
    other = JAMIE(metrics='device').spectral(list(emb), n_components=k - 1, kind=kind, seed=9)
    dn = kind == 'diffmap'
    lam, V, S, _, _ = su.reference('blobs4', dn)             # the host route's graph, degree and eigh
    Q = np.concatenate(got['vectors'], axis=0)
    assert got['converged'] and got['iterations'] >= 1 and got['applies'] == 1 + sum(got['degrees']) and len(got['degrees']) == got['iterations']
    assert Q.dtype == np.float64 and [v.shape for v in got['vectors']] == [(150, k), (150, k)]
    assert np.array_equal(np.concatenate(got['embedding'], axis=0), Q[:, 1:])
    assert got['n_neighbors'] == nn and got['n_edges'] == got['graph'].nnz and got['density_normalize'] == dn
    su.check_solution(Q, got['eigenvalues'], S, lam, V, k, 16, same_graph=False, tag=f'device against the host route, {kind}')
    deg_d, deg_h = np.concatenate(got['degree']), np.concatenate(host['degree'])
    rel = float(np.max(np.abs(deg_d - deg_h) / deg_h))
    g = got['graph']
    # the degree is held to the host's arithmetic on the device's own graph, to the bit: between the routes the fp32 graph values
    # themselves differ (the distances are fp32 on the device, float64 on the host; measured 3.7e-6 relative on this degree)
    rowsum = su.restated_rowsum(g.indptr.astype(np.int64), g.indices, g.data)
    if dn:
        rowsum = su.restated_rowsum(g.indptr.astype(np.int64), g.indices, g.data, 1.0 / rowsum) * (1.0 / rowsum)
    print(f'{kind}: degree within {rel:.2e} relative between the routes, {int((deg_d != rowsum).sum())} cells differ from the host '
          f'arithmetic on the device graph; eigenvalues {got["eigenvalues"]} against {host["eigenvalues"]}')
    assert np.array_equal(deg_d, rowsum)
    init = got['umap_init']
    assert init.shape == (300, 2) and init.dtype == np.float32 and init.min() >= 0.0 and init.max() <= 10.0
    for key in ('eigenvalues', 'residuals', 'umap_init'):
        assert np.array_equal(got[key], again[key]), key
    for key in ('vectors', 'degree'):
        assert all(np.array_equal(a, b) for a, b in zip(got[key], again[key])), key
    assert (got['iterations'], got['applies'], got['degrees']) == (again['iterations'], again['applies'], again['degrees'])
    print(f'another seed: eigenvalues differ by {np.max(np.abs(got["eigenvalues"] - other["eigenvalues"])):.2e}')
    assert np.max(np.abs(got['eigenvalues'] - other['eigenvalues'])) <= 2 * TOL
    if not dn:
        lay = JAMIE(metrics='device').umap(list(emb), init=init, n_epochs=5)
        assert [y.shape for y in lay['layout']] == [(150, 2), (150, 2)] and all(np.isfinite(y).all() for y in lay['layout'])


def test_two_components_and_pseudotime_on_the_sheet(jsp):
    from jamie_amd import JAMIE
    emb, _, _ = su.cells('apart')
    out = JAMIE(metrics='device').spectral(list(emb))
    print(f'two components: eigenvalues {out["eigenvalues"]}')
    assert out['converged'] and np.all(np.abs(out['eigenvalues'][:2] - 1.0) <= TOL)
    with pytest.raises(ValueError, match='spectral'):
        jsp.pseudotime(out, 0)
    emb, _, s = su.cells('sheet')
    got = JAMIE(metrics='device').spectral(list(emb), n_components=10, kind='diffmap')
    host = JAMIE(metrics='host').spectral(list(emb), n_components=10, kind='diffmap')
    pt, pt_host = jsp.pseudotime(got, 0), jsp.pseudotime(host, 0)
    rho = su.spearman(pt, pt_host)
    print(f'sheet: Spearman between the routes {rho:.6f}, of the device route against the unrolled coordinate {su.spearman(pt, s):.6f}')
    assert pt[0] == 0.0 and np.all(pt >= 0)
    assert rho >= 0.999


def test_memory_at_20000_cells(jsp):
    """The peak above the resident cells stays below a quarter of an N x N fp32 matrix (the cap of DESIGN.md §20); the enumerated
    need is the graph and six [N, 16] float64 blocks."""
    N, L = 20000, 32
    rng = np.random.default_rng(4)
    centres = rng.standard_normal((10, L)) * 1.2
    x = torch.from_numpy((centres[rng.integers(0, 10, N)] + rng.standard_normal((N, L))).astype(np.float32)).cuda()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = jsp.spectral([x], n_components=2)
    peak = torch.cuda.max_memory_allocated() - base
    print(f'N = {N}: peak {peak / 2 ** 20:.1f} MiB above the cells (cap {N * N / 2 ** 20:.0f} MiB), {out["n_edges"]} entries, '
          f'{out["iterations"]} outer iterations, {out["applies"]} applies, converged {out["converged"]}')
    assert out['converged'] and peak < N * N

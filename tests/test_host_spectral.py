"""The spectral embedding, the parts that need no GPU: the numpy restatement of the solver (spectral_util.restated_eigen, block
for block the definition of DESIGN.md §21) against `numpy.linalg.eigh` with the derived checks (a) .. (f), the filter's degree cap,
the sign rule, `umap_init`, `pseudotime`, the restated operation order of the kernels against an extended-precision sum, the
argument checks on both routes, `JAMIE(metrics='host').spectral` end to end, the exports and the code object.  Every figure is
printed before it is asserted."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lisi_util as lu  # noqa: E402
import spectral_util as su  # noqa: E402
import tsne_util as tu  # noqa: E402
import umap_util as uu  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
SYMBOLS = ('jamie_graph_rowsum', 'jamie_graph_cheb_step', 'jamie_block_gram_workspace', 'jamie_block_gram', 'jamie_block_rotate')
TOL = 1e-8


def _sparse(S):
    from scipy.sparse import csr_matrix
    return csr_matrix(S)


@pytest.mark.parametrize('density_normalize', [False, True])
@pytest.mark.parametrize('name', sorted(su.SOLVER_CASES))
def test_restated_solver_against_eigh(name, density_normalize):
    from jamie_amd import spectral as jsp
    lam, V, S, degree, _ = su.reference(name, density_normalize)
    Ssp = _sparse(S)
    for k in su.SOLVER_CASES[name]:
        out = su.restated_eigen(lambda X: Ssp @ X, degree, k, tol=TOL)
        print(f'{name} k = {k}: {out["iterations"]} outer iterations, {out["applies"]} applies, degrees {out["degrees"]}')
        assert out['converged'] and out['iterations'] <= 100                       # (a)
        assert np.all(out['residuals'] <= TOL)
        Q = jsp.fix_signs(out['vectors'])
        su.check_solution(Q, out['eigenvalues'], S, lam, V, k, jsp.block_width(k), tol=TOL, subspace_only=name == 'apart',
                          tag=f'{name} dn={density_normalize} k={k}')
        if name == 'apart':
            assert np.all(np.abs(out['eigenvalues'][:2] - 1.0) <= TOL)


def test_unconverged_run_says_so():
    lam, V, S, degree, _ = su.reference('sheet', False)
    Ssp = _sparse(S)
    out = su.restated_eigen(lambda X: Ssp @ X, degree, 3, tol=1e-12, max_iter=1, max_degree=4)
    print(out['residuals'], out['degrees'])
    assert not out['converged'] and out['iterations'] == 1 and out['degrees'] == [4] and out['applies'] == 5


def test_filter_plan_and_degree_cap():
    from jamie_amd import spectral as jsp
    theta = np.linspace(1.0, 0.9, 16)
    p, e, c, s1 = jsp.filter_plan(theta, 60)
    t = (1.0 - c) / e
    rho = t + np.sqrt(t * t - 1.0)
    assert abs(e - 0.95) < 1e-15 and abs(c + 0.05) < 1e-15 and s1 == e / (1.0 - c)
    assert rho ** p >= 2e6 > rho ** (p - 1) and 2 <= p <= 60
    assert jsp.filter_plan(np.linspace(1.0, 0.9999999, 16), 60)[0] == 60          # the cap; a = 1 - 1e-6 at the latest
    assert abs(jsp.filter_plan(np.linspace(1.0, 0.9999999, 16), 60)[1] - (1.0 - 5e-7)) < 1e-15
    assert jsp.filter_plan(np.linspace(1.0, -0.9999999, 16), 60)[0] == 2              # the floor
    assert abs(jsp.filter_plan(np.linspace(1.0 + 1e-9, 0.5, 16), 60)[3] - 0.75 / (1.25 + 1e-9)) < 1e-15      # top = max(theta_1, 1)
    # the recurrence reproduces the scaled Chebyshev polynomial: T_p((x - c) / e) / T_p((top - c) / e) on scalars
    steps = jsp.filter_coefficients(p, e, c, s1)
    assert len(steps) == p and steps[0][2] == 0.0
    for x in (1.0, 0.97, 0.5, -1.0):
        prev, cur = None, 1.0
        for al, ga, be in steps:
            prev, cur = cur, al * x * cur + ga * cur - (be * prev if prev is not None else 0.0)
        u, top = (x - c) / e, (1.0 - c) / e
        cheb = (np.cosh(p * np.arccosh(u)) if u > 1 else np.cos(p * np.arccos(u))) / np.cosh(p * np.arccosh(top))
        print(f'x = {x}: filter {cur:.6e}, closed form {cheb:.6e}')
        assert abs(cur - cheb) <= 1e-9 * max(1.0, abs(cheb))
    assert jsp.block_width(12) == 16 and jsp.block_width(13) == 32


def test_sign_rule_whitening_and_ritz():
    from jamie_amd import spectral as jsp
    Q = np.array([[0.1, -0.5, 0.5], [-0.9, 0.5, -0.5], [0.2, 0.1, 0.1]])
    F = jsp.fix_signs(Q)
    assert np.array_equal(F[:, 0], -Q[:, 0]) and np.array_equal(F[:, 1], -Q[:, 1]) and np.array_equal(F[:, 2], Q[:, 2])
    rng = np.random.default_rng(0)
    Y = rng.standard_normal((200, 16)) * 10.0 ** rng.uniform(-3, 3, 16)
    for _ in range(2):
        Y = Y @ jsp.whitening(Y.T @ Y)
    err = np.max(np.abs(Y.T @ Y - np.eye(16)))
    print(f'whitening twice: |Y^T Y - I| = {err:.2e}')
    assert err <= 6 * (200 * 16 + 16 * 17) * su.U
    H = rng.standard_normal((16, 16))
    theta, V = jsp.ritz(H)
    assert np.all(np.diff(theta) <= 0) and np.allclose(V.T @ ((H + H.T) / 2) @ V, np.diag(theta), atol=1e-12)


def test_umap_init_is_initial_layouts_mapping():
    from jamie_amd import spectral as jsp
    from jamie_amd import umap as jum
    rng = np.random.default_rng(1)
    Q = rng.standard_normal((50, 4))
    Y = jsp.umap_init(Q)
    assert Y.shape == (50, 2) and Y.dtype == np.float32 and Y.min() == 0.0 and Y.max() == 10.0
    lo, hi = Q[:, 1:3].min(axis=0), Q[:, 1:3].max(axis=0)
    assert np.array_equal(Y, (jum.INIT_SPAN * (Q[:, 1:3] - lo) / (hi - lo)).astype(np.float32))
    Q[:, 2] = 3.0
    assert np.all(jsp.umap_init(Q)[:, 1] == 5.0)
    one = jsp.umap_init(Q[:, :2])                            # n_components = 1: the missing column is constant
    assert one.shape == (50, 2) and np.all(one[:, 1] == 5.0) and np.array_equal(one[:, 0], Y[:, 0])


def test_pseudotime_is_the_definition():
    from jamie_amd import spectral as jsp
    rng = np.random.default_rng(2)
    Q = rng.standard_normal((30, 4))
    theta = np.array([1.0, 0.9, 0.5, -0.2])
    out = dict(vectors=[Q[:12], Q[12:]], eigenvalues=theta, tol=1e-8)
    pt = jsp.pseudotime(out, 7)
    want = np.array([np.sqrt(sum((theta[m] / (1 - theta[m])) ** 2 * (Q[x, m] - Q[7, m]) ** 2 for m in (1, 2, 3))) for x in range(30)])
    assert pt[7] == 0.0 and np.allclose(pt, want, rtol=1e-14, atol=0)
    for root in (-1, 30):
        with pytest.raises(ValueError, match='spectral'):
            jsp.pseudotime(out, root)
    with pytest.raises(ValueError, match='spectral'):
        jsp.pseudotime(dict(out, eigenvalues=np.array([1.0, 1.0 - 5e-8, 0.5, 0.1])), 0)


@pytest.mark.parametrize('name', [130, 'hub', 'special'])
def test_restated_kernel_orders_meet_their_bounds(name):
    """The chosen operation orders, restated in numpy, against an extended-precision sum: the bound the device is held to
    (test_hip_spectral.py) is met by the arithmetic itself."""
    c = uu.shape_case(name)
    W = uu.smooth_reference(c['dist'], c['nn'])['W'].astype(np.float32)
    rowptr, col, val, _ = uu.graph_arrays(c['idx'], W)
    N = len(rowptr) - 1
    rng = np.random.default_rng(3)
    d = su.restated_rowsum(rowptr, col, val)
    exact = np.array([np.sum(val[rowptr[i]:rowptr[i + 1]].astype(np.longdouble)) for i in range(N)])
    lens = np.diff(rowptr)
    err = np.abs(d - exact) / exact
    print(f'{name}: rowsum within {float(err.max()) / su.U:.2f} u of the extended sum, longest row {lens.max()}')
    assert np.all(err <= (np.ceil(lens / 16) + 4) * su.U)
    scale = 1.0 / np.sqrt(d)
    for B in (16, 32):
        X, prev = rng.standard_normal((N, B)), rng.standard_normal((N, B))
        out = su.restated_cheb_step(rowptr, col, val, scale, X, prev, 1.7, -0.3, 0.6)
        ref, mag, lens = su.cheb_reference(rowptr, col, val, scale, X, prev, 1.7, -0.3, 0.6)
        rel = np.abs(out - ref) / mag
        print(f'{name} B = {B}: cheb_step within {float(rel.max()) / su.U:.2f} u of the magnitudes (bound len + 8 = {lens.max() + 8})')
        assert np.all(rel <= su.cheb_bound(lens))


@pytest.mark.parametrize('route', ['host', 'device'])
def test_value_errors_on_both_routes(route):
    """Every refusal comes from the shared argument checks, names spectral, and comes before either route touches a device."""
    from jamie_amd import JAMIE
    from jamie_amd import spectral as jsp
    j = JAMIE(metrics=route)
    emb, _ = lu.mixture(1, 3, 4, (60, 50))
    bad_nan = [emb[0].copy(), emb[1]]
    bad_nan[0][3, 2] = np.nan
    bad_inf = [emb[0], emb[1].copy()]
    bad_inf[1][0, 0] = np.inf
    cases = [dict(kind='laplace'), dict(kind=None), dict(n_components=0), dict(n_components=28), dict(n_components=2.5),
             dict(n_neighbors=1), dict(n_neighbors=111), dict(n_neighbors=130), dict(tol=0.0), dict(tol=1.0), dict(tol=float('nan')),
             dict(max_iter=0), dict(max_degree=1)]

    def refused(call):
        with pytest.raises(ValueError, match='spectral'):
            call()
    for kw in cases:
        refused(lambda: j.spectral(emb, **kw))
        refused(lambda: jsp.check_spectral(emb, **kw))
    for bad in (bad_nan, bad_inf, [emb[0], emb[1][:, :3]], [], [emb[0][:15]], [emb[0][:10], emb[1][:5]]):
        refused(lambda: j.spectral(bad))
    refused(lambda: j.spectral([emb[0][:31]], n_components=12))           # a block of 32 needs 32 cells
    with pytest.raises(ValueError, match='umap'):                         # the string option stays refused: the init is an array
        j.umap(emb, init='spectral', n_epochs=5)
    assert jsp.check_spectral(emb, kind='diffmap')[3] is True and jsp.check_spectral(emb)[3] is False
    assert jsp.check_spectral(emb, kind='diffmap', density_normalize=False)[3] is False
    with pytest.raises(ValueError, match='spectral'):
        jsp.check_degree(np.array([1.0, 0.0, 2.0]))
    with pytest.raises(ValueError, match='spectral'):
        jsp.check_degree(np.array([1.0, np.inf]))


@pytest.mark.parametrize('kind', ['laplacian', 'diffmap'])
def test_host_route_on_four_blobs(kind):
    from jamie_amd import JAMIE
    from jamie_amd import spectral as jsp
    emb, nn, _ = su.cells('blobs4')
    out = JAMIE(metrics='host').spectral(list(emb), n_components=4, kind=kind, return_graph=True)
    dn = kind == 'diffmap'
    lam, V, S, degree, _ = su.reference('blobs4', dn)
    k, N = 5, 300
    Q = np.concatenate(out['vectors'], axis=0)
    assert Q.shape == (N, k) and Q.dtype == np.float64 and [v.shape for v in out['vectors']] == [(150, k), (150, k)]
    assert [e.shape for e in out['embedding']] == [(150, k - 1), (150, k - 1)]
    assert np.array_equal(np.concatenate(out['embedding'], axis=0), Q[:, 1:])
    assert out['iterations'] == 0 and out['applies'] == 0 and out['degrees'] == [] and out['converged']
    assert out['n_neighbors'] == nn and out['n_edges'] == out['graph'].nnz and out['density_normalize'] == dn
    assert np.allclose(np.concatenate(out['degree']), degree, rtol=1e-14, atol=0)
    assert np.allclose(out['eigenvalues'], lam[:k], rtol=0, atol=1e-13) and abs(out['eigenvalues'][0] - 1.0) <= 1e-13
    assert np.all(out['residuals'] <= 1e-12)
    trivial = np.sqrt(degree) / np.linalg.norm(np.sqrt(degree))
    print(f'{kind}: eigenvalues {out["eigenvalues"]}, trivial vector within {np.max(np.abs(Q[:, 0] - trivial)):.2e}')
    assert np.max(np.abs(Q[:, 0] - trivial)) <= 1e-12
    for i in range(k):
        assert Q[np.argmax(np.abs(Q[:, i])), i] > 0 and abs(np.linalg.norm(Q[:, i]) - 1.0) <= 1e-14
    init = out['umap_init']
    assert init.shape == (N, 2) and init.dtype == np.float32 and init.min() == 0.0 and init.max() == 10.0
    assert np.array_equal(init, jsp.umap_init(Q))
    pt = jsp.pseudotime(out, 11)
    assert pt[11] == 0.0 and np.all(pt >= 0) and np.all(np.isfinite(pt))


def test_host_route_two_components_and_the_sheet():
    from jamie_amd import JAMIE
    from jamie_amd import spectral as jsp
    emb, _, _ = su.cells('apart')
    out = JAMIE(metrics='host').spectral(list(emb))
    assert np.all(np.abs(out['eigenvalues'][:2] - 1.0) <= 1e-13)
    with pytest.raises(ValueError, match='spectral'):
        jsp.pseudotime(out, 0)
    emb, _, s = su.cells('sheet')
    host = JAMIE(metrics='host').spectral(list(emb), n_components=10, kind='diffmap')
    lam, V, S, degree, _ = su.reference('sheet', True)
    Ssp = _sparse(S)
    rest = su.restated_eigen(lambda X: Ssp @ X, degree, 11, tol=TOL)
    rest = dict(vectors=[jsp.fix_signs(rest['vectors'])], eigenvalues=rest['eigenvalues'], tol=TOL)
    pt_host, pt_rest = jsp.pseudotime(host, 0), jsp.pseudotime(rest, 0)
    rho, along = su.spearman(pt_rest, pt_host), su.spearman(pt_host, s)
    print(f'sheet: Spearman of the restated solver against the host route {rho:.6f}; of the host route against the coordinate {along:.6f}')
    assert pt_host[0] == 0.0 and pt_rest[0] == 0.0
    assert rho >= 0.999


def test_exports_and_bindings():
    from jamie_amd import _native as nv
    hdr = open(os.path.join(ROOT, 'include', 'jamie_hip.h')).read()
    for s in SYMBOLS:
        assert s in nv.EXPORTS and f'{s}(' in hdr, s
    lib = nv.load()
    assert lib.jamie_block_gram_workspace(1, 16) == 256 * 8 and lib.jamie_block_gram_workspace(513, 32) == 2 * 1024 * 8
    assert lib.jamie_block_gram_workspace(512, 16) == 256 * 8
    assert lib.jamie_block_gram_workspace(10, 8) == 0 and lib.jamie_block_gram_workspace(0, 16) == 0
    # the refusals come before any launch: no device is needed to see them
    assert lib.jamie_graph_cheb_step(8, 8, 8, 0, 8, 16, None, 16, 4, 16, 1.0, 0.0, 0.0, None) != 0 and b'in must differ' in lib.jamie_last_error()
    assert lib.jamie_graph_cheb_step(8, 8, 8, 0, 8, 16, 16, 24, 4, 16, 1.0, 0.0, 0.0, None) != 0
    assert lib.jamie_graph_cheb_step(8, 8, 8, 0, 8, 16, None, 24, 4, 8, 1.0, 0.0, 0.0, None) != 0 and b'16 or 32' in lib.jamie_last_error()
    assert lib.jamie_graph_cheb_step(8, 8, 8, 0, 8, 16, None, 24, 4, 16, float('nan'), 0.0, 0.0, None) != 0
    assert lib.jamie_graph_rowsum(None, 8, 8, None, 4, 0, 8, None) != 0 and b'null' in lib.jamie_last_error()
    assert lib.jamie_block_gram(8, 8, 4, 16, 16, 8, 24, None) != 0 and b'workspace' in lib.jamie_last_error()
    assert lib.jamie_block_rotate(8, 16, None, None, 4, 16, 8, None) != 0 and b'out must differ' in lib.jamie_last_error()
    assert lib.jamie_block_rotate(8, 16, 24, None, 4, 16, 32, None) != 0 and b'together' in lib.jamie_last_error()


def test_spectral_kernels_use_no_scratch():
    """private_segment_fixed_size == 0 and no VGPR spills for the kernels of csrc/spectral.hip, read from the code object hipcc
    built; the step kernel asks for no LDS either."""
    import isa_check as ic
    obj = os.path.join(ROOT, 'jamie_amd', 'csrc', '_obj', 'spectral.o')
    if not os.path.exists(obj):
        pytest.skip('the library is not built')
    if not os.path.exists(ic.OBJDUMP):
        pytest.skip('llvm-objdump not found')
    meta = ic.kernel_metadata(obj)
    names = ' '.join(meta)
    for kernel in ('spectral_rowsum_kernel', 'spectral_cheb_kernel', 'spectral_gram_kernel', 'spectral_gram_sum_kernel',
                   'spectral_rotate_kernel'):
        assert kernel in names, (kernel, names)
    assert len(meta) == 8                                     # the step, the Gram and the rotation at B = 16 and 32
    for name, m in meta.items():
        print(name, {k: m.get(k) for k in ('vgpr_count', 'sgpr_count', 'group_segment_fixed_size', 'private_segment_fixed_size')})
        assert m['private_segment_fixed_size'] == 0, (name, m)
        assert m.get('vgpr_spill_count', 0) == 0 and m.get('sgpr_spill_count', 0) == 0, (name, m)
        if 'spectral_cheb_kernel' in name or 'spectral_rowsum_kernel' in name:
            assert m.get('group_segment_fixed_size', 0) == 0, (name, m)

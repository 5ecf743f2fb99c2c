"""The UMAP layout, the parts that need no GPU: the curve fit, the numpy Philox and the draws, the float64 references of
umap_util.py on inputs whose answer is known, the fp32 restatement of the epoch kernel (where UPDATE_TOL is checked on the CPU),
`JAMIE(metrics='host').umap` on four blobs, the argument checks on both routes, the exports and the code object."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_util as bn  # noqa: E402
import lisi_util as lu  # noqa: E402
import tsne_util as tu  # noqa: E402
import umap_util as uu  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
SYMBOLS = ('jamie_umap_smooth_knn', 'jamie_umap_mutual', 'jamie_umap_epoch')


def test_find_ab_reproduces_the_published_default():
    from jamie_amd import umap as jum
    a, b = jum.find_ab(1.0, 0.1)
    print(f'a = {a:.7f}, b = {b:.7f}')
    assert abs(a - 1.5769435) <= 1e-6 and abs(b - 0.8950609) <= 1e-6
    emb, _ = lu.mixture(1, 3, 4, (60, 50))
    checked = jum.check_umap(emb, 15, 0.1, 1.0, None, 1.0, 5, 1.0, 'pca', 1.2, 0.7)
    assert checked[-2:] == (1.2, 0.7) and checked[1] == 500
    fitted = jum.check_umap(emb, 15, 0.1, 1.0, 30, 1.0, 5, 1.0, 'pca', None, None)
    assert fitted[-2:] == (a, b) and fitted[1] == 30
    assert jum.default_epochs(10000) == 500 and jum.default_epochs(10001) == 200


def test_numpy_philox_equals_the_test_twin():
    from jamie_amd import umap as jum
    rng = np.random.default_rng(0)
    counter = [rng.integers(0, 2 ** 32, 1000, dtype=np.uint64) for _ in range(4)]
    key = [rng.integers(0, 2 ** 32, 1000, dtype=np.uint64) for _ in range(2)]
    got, ref = jum.philox4x32_10(counter, key), bn.philox4x32_10(counter, key)
    assert all(np.array_equal(g, r) for g, r in zip(got, ref))
    # the published known answer of Random123 for the all-ones counter and key
    kat = jum.philox4x32_10([0xffffffff] * 4, [0xffffffff] * 2)
    assert [int(w) for w in kat] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]


def test_draws_are_a_function_of_seed_entry_epoch_and_draw():
    from jamie_amd import umap as jum
    e = np.array([0, 1, 2, 2 ** 32 + 5, 7], dtype=np.int64)
    for N in (2, 130, 2 ** 31 - 1):
        c = jum.negative_cells(3, e, 11, 9, N)
        assert c.shape == (5, 9) and c.min() >= 0 and c.max() < N
        # the same (seed, e, n, r) whatever else is asked in the same call; a shorter call is a prefix
        assert np.array_equal(jum.negative_cells(3, e[::-1], 11, 9, N), c[::-1])
        assert np.array_equal(jum.negative_cells(3, e[2:3], 11, 5, N), c[2:3, :5])
    big = jum.negative_cells(3, e, 11, 9, 10 ** 6)
    assert not np.array_equal(jum.negative_cells(4, e, 11, 9, 10 ** 6), big)
    assert not np.array_equal(jum.negative_cells(3, e, 12, 9, 10 ** 6), big)
    assert not np.array_equal(big[3], jum.negative_cells(3, np.array([5]), 11, 9, 10 ** 6)[0])      # (the high word of e counts)
    # written out for one draw: word r & 3 of the block r >> 2
    words = bn.philox4x32_10((7, 0, 11, 1), (3, 0))
    assert big[4, 6] == (int(words[2]) * 10 ** 6) >> 32
    seed = 2 ** 40 + 9
    words = bn.philox4x32_10((2, 0, 0, 0), (seed & 0xffffffff, seed >> 32))
    assert jum.negative_cells(seed, e[2:3], 0, 1, 1000)[0, 0] == (int(words[0]) * 1000) >> 32
    counts = np.bincount(jum.negative_cells(0, np.arange(20000), 0, 5, 10).reshape(-1), minlength=10)
    print(f'100 000 draws over 10 cells: {counts}')
    assert counts.min() > 9500 and counts.max() < 10500


@pytest.mark.parametrize('name', uu.CASES)
def test_smooth_reference_and_the_host_route(name):
    """Rows of psi sum to log2(n_neighbors) within 1e-5 wherever the floor did not bind; the margins of the float64 trace stay
    under the cap of the device comparison; the host route's solve is this loop."""
    from jamie_amd.jamie import _host_smooth_knn
    c = uu.shape_case(name)
    ref = uu.smooth_reference(c['dist'], c['nn'])
    target = np.log2(c['nn'])
    free = ~ref['floored'] & (ref['tries'] < 64)
    near = ref['margin'] < uu.NEAR_BRANCH
    off = np.abs(ref['psi_sum'] - target)
    print(f'{name}: n_neighbors {c["nn"]}, tries {ref["tries"].min()} .. {ref["tries"].max()}, floored {int(ref["floored"].sum())}, at the '
          f'cap {int((ref["tries"] == 64).sum())}, near a branch {near.mean():.4f}, |sum - target| {off[free].max():.2e}, sigma '
          f'{ref["sigma"].min():.3e} .. {ref["sigma"].max():.3e}')
    assert np.all(off[free] < 1e-5)
    assert near.mean() <= uu.NEAR_BRANCH_CAP
    assert np.all(ref['W'] >= 0) and np.all(np.diff(ref['W'], axis=1) <= 0)
    assert np.all(ref['W'] <= 1) and np.all(ref['W'][:, 0] == 1)       # (the nearest cell is at rho or, a copy, below it)
    W, rho, sigma, tries = _host_smooth_knn(c['dist'], c['nn'])
    assert np.array_equal(W, ref['W'].astype(np.float32)) and np.array_equal(rho, ref['rho'])
    assert np.array_equal(sigma, ref['sigma']) and np.array_equal(tries, ref['tries'])
    if name == 'special':
        blk, trip = np.arange(*uu.BLOCK), uu.TRIPLE[0]
        assert np.all(ref['rho'][blk] == 0) and np.all(ref['W'][blk] == 1) and np.all(ref['tries'][blk] == 64)
        assert np.all(ref['sigma'][blk] == 2.0 ** -64)                                    # halved 64 times and never used
        assert np.all(c['dist'][trip, :3] == 0) and ref['rho'][trip] == c['dist'][trip, 3] > 0
        assert np.all(ref['W'][trip, :4] == 1) and ref['W'][trip, 4] < 1
        o = uu.OUTLIER
        print(f'the outlier: distances {c["dist"][o, 0]:.1f} .. {c["dist"][o, -1]:.1f}, sigma {ref["sigma"][o]:.4f}, tries {ref["tries"][o]}')
        assert ref['floored'][o] and ref['sigma'][o] == 1e-3 * c['dist'][o].sum() / c['nn']
    if name == 8:
        assert c['K'] == 7 and len(c['X']) == 8


def test_the_doubling_branch_and_a_known_answer():
    """Distances 1, 2, 3, ..., K with n_neighbors = K + 1: the solve can be followed by hand."""
    d = np.arange(1, 101, dtype=np.float64)[None, :] * 10.0
    ref = uu.smooth_reference(d, 101)
    e = d[0] - 10.0
    s = np.where(e > 0, np.exp(-e / ref['sigma'][0]), 1.0).sum()
    print(f'sigma {ref["sigma"][0]:.6f} after {ref["tries"][0]} tries, sum {s:.8f}, log2(101) {np.log2(101):.8f}')
    assert ref['sigma'][0] > 16 and abs(s - np.log2(101)) < 1e-5 and ref['rho'][0] == 10.0 and not ref['floored'][0]
    one = uu.smooth_reference(np.array([[2.0]]), 2)         # K = 1: the sum is 1 = log2(2) at the first try
    assert one['tries'][0] == 1 and one['sigma'][0] == 1.0 and one['W'][0, 0] == 1.0


@pytest.mark.parametrize('name', [8, 130, 600, 'hub', 'special'])
def test_union_reference_and_the_host_graph(name):
    from jamie_amd.jamie import _host_fuzzy_graph
    c = uu.shape_case(name)
    N = len(c['X'])
    W = uu.smooth_reference(c['dist'], c['nn'])['W'].astype(np.float32)
    A = uu.union_reference(c['idx'], W)
    dense = np.zeros((N, N))
    np.put_along_axis(dense, c['idx'], W.astype(np.float64), axis=1)
    want = dense + dense.T - dense * dense.T
    assert np.array_equal(np.asarray(A.todense()), want) and abs(A - A.T).max() == 0
    rowptr, col, val, row = uu.graph_arrays(c['idx'], W)
    hrowptr, hcol, hval = _host_fuzzy_graph(c['idx'], W)
    assert np.array_equal(rowptr, hrowptr) and np.array_equal(col, hcol) and np.array_equal(val, hval)
    listed = dense > 0
    np.put_along_axis(listed, c['idx'], True, axis=1)      # (a weight that underflowed to 0 is still an entry)
    assert np.array_equal(val, want[row, col].astype(np.float32)) and len(col) == int((listed | listed.T).sum()) >= A.nnz
    K = c['K']
    for i in (0, N // 2, N - 1):
        own, rest = col[rowptr[i]:rowptr[i] + K], col[rowptr[i] + K:rowptr[i + 1]]
        assert np.array_equal(own, c['idx'][i]) and np.all(np.diff(rest) > 0) and not set(rest) & set(own)
        assert all(i in c['idx'][j] for j in rest)
    print(f'{name}: nnz {len(col)}, rows of {np.diff(rowptr).min()} .. {np.diff(rowptr).max()} entries, values {val.min():.3e} .. {val.max()}')
    assert val.max() == 1.0
    if name == 'hub':
        assert rowptr[uu.HUB + 1] - rowptr[uu.HUB] == N - 1 == uu.LONGEST_ROW
    if name == 8:
        assert np.all(np.diff(rowptr) == 7)


def test_schedule_matches_a_scalar_loop():
    from jamie_amd import umap as jum
    c = uu.shape_case(130)
    W = uu.smooth_reference(c['dist'], c['nn'])['W'].astype(np.float32)
    _, _, val, _ = uu.graph_arrays(c['idx'], W)
    eps_s, nxt_s, fired_s = uu.schedule_scalar(val, 40, 40)
    eps, nxt = jum.schedule_arrays(val, 40)
    assert eps.dtype == np.float32 and np.array_equal(eps, eps_s) and np.array_equal(nxt, eps)
    for n in range(40):
        fire = nxt <= np.float32(n)
        assert np.array_equal(fire, fired_s[n]), n
        nxt[fire] = nxt[fire] + eps[fire]
    assert np.array_equal(nxt, nxt_s)
    pruned = np.isinf(eps)
    print(f'{len(val)} entries, {int(pruned.sum())} never fire at n_epochs = 40, firings {int(fired_s.sum())}, in epoch 0 '
          f'{int(fired_s[0].sum())}, in epoch 1 {int(fired_s[1].sum())}')
    assert pruned.sum() > 0 and np.all(val[pruned] < val.max() / 40) and not fired_s[:, pruned].any()
    assert fired_s[0].sum() == 0 and np.all(fired_s[1] == (val == val.max()))               # the heaviest edge first fires in epoch 1
    assert np.all(fired_s[:, val == val.max()].sum(axis=0) == 39)


def _epoch_inputs(name, n_epochs=40):
    from jamie_amd import umap as jum
    c = uu.shape_case(name)
    W = uu.smooth_reference(c['dist'], c['nn'])['W'].astype(np.float32)
    rowptr, col, val, row = uu.graph_arrays(c['idx'], W)
    eps, nxt = jum.schedule_arrays(val, n_epochs)
    return c, rowptr, col, row, eps, nxt


@pytest.mark.parametrize('name', uu.CASES)
def test_design_restated(name):
    """The fp32 operation order of the epoch kernel in numpy against all-float64 on the same firing entries and draws: inside
    UPDATE_TOL on every case, and on a layout with coincident points."""
    from jamie_amd import umap as jum
    from jamie_amd.jamie import _host_umap_epoch
    a, b = jum.curve32(*jum.find_ab(1.0, 0.1))
    c, rowptr, col, row, eps, nxt = _epoch_inputs(name)
    n = 20
    fire = nxt <= np.float32(n)
    layouts = [('spread', uu.spread_layout(name))]
    if name == 130:
        Y = uu.spread_layout(name).copy()
        Y[20:25] = Y[20]
        layouts.append(('five copies of one point', Y))
    for what, Y in layouts:
        ref = uu.epoch_reference(row, col, fire, Y, n, a, b, 1.0, uu.NEG, 5)
        got = uu.restated_epoch(rowptr, col, fire, Y, n, a, b, 1.0, uu.NEG, 5)
        worst = uu.update_error(got, ref)
        print(f'{name} {what}: {int(fire.sum())} of {len(fire)} entries fire, {ref["self_draws"]} draws of the cell itself, '
              f'{ref["zero_terms"]} terms at distance 0, largest error {worst:.3e} of the magnitudes; UPDATE_TOL {uu.UPDATE_TOL:.3e}')
        assert fire.mean() > 0.2
        assert worst <= uu.UPDATE_TOL
        assert np.array_equal(ref['fired'], np.bincount(row[fire], minlength=len(Y)))
        if what != 'spread':
            assert ref['zero_terms'] > 0 and ref['self_draws'] > 0
        # the host route's epoch is this reference
        Y1, fired = _host_umap_epoch(row, col.astype(np.int64), eps, nxt.copy(), Y.astype(np.float64), n, 0.5, a, b, 1.0, uu.NEG, 5)
        assert fired == int(fire.sum())
        assert np.allclose(Y1, Y.astype(np.float64) + 0.5 * ref['delta'], rtol=0, atol=1e-12)


def test_update_tol_is_the_derived_figure():
    assert uu.ADD_DEPTH == 5 + 19 + 4 and uu.TERM_ROUNDINGS == 8 * 1 + 15
    assert uu.UPDATE_TOL == 52 * 2.0 ** -24


def test_initial_layout():
    from jamie_amd import umap as jum
    X = np.concatenate(tu.blobs()[0])
    for init in ('pca', 'random'):
        y, again = jum.initial_layout(X, init, 3), jum.initial_layout(X, init, 3)
        assert y.dtype == np.float32 and y.shape == (400, 2) and np.array_equal(y, again)
        assert np.all(y.min(axis=0) == 0) and np.all(y.max(axis=0) == 10)
    assert not np.array_equal(jum.initial_layout(X, 'random', 3), jum.initial_layout(X, 'random', 4))
    given = np.arange(800, dtype=np.float32).reshape(400, 2)
    assert np.array_equal(jum.initial_layout(X, given, 0), given)
    flat = jum.initial_layout(np.ones((30, 1), np.float32) * np.arange(30, dtype=np.float32)[:, None], 'pca', 0)
    assert np.all(flat[:, 1] == 5) and flat[:, 0].min() == 0 and flat[:, 0].max() == 10


@pytest.mark.parametrize('route', ['host', 'device'])
def test_value_errors_on_both_routes(route):
    """Every refusal comes from the shared argument checks, names umap, and comes before either route touches a device."""
    from jamie_amd import JAMIE
    from jamie_amd import umap as jum
    j = JAMIE(metrics=route)
    emb, _ = lu.mixture(1, 3, 4, (60, 50))
    N = 110
    bad_nan = [emb[0].copy(), emb[1]]
    bad_nan[0][3, 2] = np.nan
    bad_inf = [emb[0].copy(), emb[1]]
    bad_inf[1][0, 0] = np.inf
    init_nan = np.zeros((N, 2), np.float32)
    init_nan[5, 1] = np.nan
    cases = [dict(n_neighbors=1), dict(n_neighbors=111), dict(n_neighbors=130), dict(min_dist=2.0), dict(min_dist=0.5, spread=0.25),
             dict(min_dist=-0.1), dict(spread=0.0), dict(n_epochs=0), dict(n_epochs=-3), dict(learning_rate=0), dict(learning_rate=-1.0),
             dict(learning_rate=float('nan')), dict(learning_rate=float('inf')), dict(negative_sample_rate=0),
             dict(negative_sample_rate=-2), dict(negative_sample_rate=65), dict(repulsion_strength=0.0), dict(repulsion_strength=-1.0),
             dict(init='spectral'), dict(init=np.zeros((N, 3))), dict(init=np.zeros((N - 1, 2))), dict(init=init_nan), dict(a=1.0),
             dict(a=-1.0, b=1.0), dict(a=1.0, b=0.0)]

    def refused(call):
        with pytest.raises(ValueError, match='umap'):
            call()
    for kw in cases:
        kw = dict(dict(n_epochs=5), **kw)
        refused(lambda: j.umap(emb, **kw))
        args = [kw.get(k, d) for k, d in (('n_neighbors', 15), ('min_dist', 0.1), ('spread', 1.0), ('n_epochs', None), ('learning_rate', 1.0),
                                          ('negative_sample_rate', 5), ('repulsion_strength', 1.0), ('init', 'pca'), ('a', None), ('b', None))]
        refused(lambda: jum.check_umap(emb, *args))
    for bad in (bad_nan, bad_inf, [emb[0], emb[1][:, :3]], []):
        refused(lambda: j.umap(bad, n_epochs=5))
        refused(lambda: jum.check_umap(bad, 15, 0.1, 1.0, 5, 1.0, 5, 1.0, 'pca', None, None))
    # n_neighbors = cells is the largest list there is
    assert jum.check_umap([emb[0][:9]], 9, 0.1, 1.0, 5, 1.0, 5, 1.0, 'random', None, None)[0] == 9


def test_host_route_on_four_blobs():
    emb, lab = tu.blobs()
    labels = np.concatenate(lab)
    for seed in (0, 1):
        out = uu.host_run(seed)
        Y = np.concatenate(out['layout'])
        p = tu.purity(Y, labels)
        print(f'seed {seed}: {out["n_edges"]} edges, {out["n_fired"]} firings, a {out["a"]:.7f}, b {out["b"]:.7f}, layout within '
              f'{Y.min():.2f} .. {Y.max():.2f}, 10-NN purity {p}')
        assert [a.shape for a in out['layout']] == [(200, 2), (200, 2)] and out['layout'][0].dtype == np.float32
        assert out['n_epochs'] == 200 and out['n_neighbors'] == 15 and out['graph'] is None and type(out['n_fired']) is int
        assert np.all(np.isfinite(Y)) and p == 1.0
    from jamie_amd import JAMIE
    again = JAMIE(metrics='host').umap(emb, n_epochs=200, init='random', seed=1, return_graph=True)
    assert all(np.array_equal(x, y) for x, y in zip(again['layout'], out['layout'])) and again['n_fired'] == out['n_fired']
    G = again['graph']
    assert G.shape == (400, 400) and G.dtype == np.float32 and G.nnz == out['n_edges'] and abs(G - G.T).max() == 0
    assert not np.array_equal(np.concatenate(uu.host_run(0)['layout']), Y)


def test_exports_and_header():
    import jamie_amd
    jamie_amd.build_library()
    from jamie_amd import _native as lib
    hdr = open(os.path.join(ROOT, 'include', 'jamie_hip.h')).read()
    assert 'UMAP layout on the device' in hdr
    handle = lib.load()
    for name in SYMBOLS:
        assert name in lib.EXPORTS and hasattr(handle, name), name
        assert re.search(r'\b' + name + r'\s*\(', hdr), name


def test_umap_kernels_use_no_scratch():
    """private_segment_fixed_size == 0 and no VGPR spills for the three kernels of csrc/umap.hip, read from the code object hipcc
    built; the epoch kernel asks for no LDS either."""
    import isa_check as ic
    obj = os.path.join(ROOT, 'jamie_amd', 'csrc', '_obj', 'umap.o')
    if not os.path.exists(obj):
        pytest.skip('the library is not built')
    if not os.path.exists(ic.OBJDUMP):
        pytest.skip('llvm-objdump not found')
    meta = ic.kernel_metadata(obj)
    names = ' '.join(meta)
    for kernel in ('umap_smooth_knn_kernel', 'umap_mutual_kernel', 'umap_epoch_kernel'):
        assert kernel in names, (kernel, names)
    assert len(meta) == 3
    for name, m in meta.items():
        assert m['private_segment_fixed_size'] == 0, (name, m)
        assert m.get('vgpr_spill_count', 0) == 0, (name, m)
        if 'umap_epoch_kernel' in name:
            assert m.get('group_segment_fixed_size', 0) == 0, (name, m)

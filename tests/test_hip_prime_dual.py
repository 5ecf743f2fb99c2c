"""The Prime_Dual kernels (csrc/prime_dual.hip: jamie_pd_step, jamie_pd_alpha) one call at a time through the C ABI against the
float64 reference of tests/pd_util.py, from states the iteration does not reach on its own, at the tile edges and on both the
float4 and the scalar path; then `PrimeDual.step()` product by product.  Every buffer sits between guard words, and the
workspaces are NaN before every call.  Run on the GPU box:  pytest -m gpu"""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pd_util as pu  # noqa: E402

pytestmark = pytest.mark.gpu
MATRICES = ('F', 'G1', 'G2', 'm1', 'm2')
f32 = np.float32


@pytest.fixture(scope='module')
def nv():
    from jamie_amd import _native
    _native.require_gpu()
    return _native


class Dev:
    """A case on the device: every member of jamie_pd_state carved out of one guarded arena (the five matrices on 16-byte
    boundaries, the vectors one float past one), rowpart and colpart left as NaN."""

    def __init__(self, nv, case):
        st = case['state']
        self.case, (self.m, self.n) = case, st['F'].shape
        m, n = self.m, self.n
        ra, ca = nv.pd_workspace(m, n)
        assert (ra, ca) == (m * -(-n // 256), -(-m // 32) * n)
        sizes = dict(F=m * n, Mu=m, G1=m * n, Lambda=n, G2=m * n, S=n, m1=m * n, rowsum=m, m2=m * n, colsum=n, alpha=1,
                     rowpart=ra, colpart=ca)
        self.arena = pu.Arena(sizes, MATRICES)
        host = dict(st, G1=case['G1'], G2=case['G2'], alpha=np.array([case['alpha']], f32))
        for k, v in host.items():
            self.arena.t[k].copy_(torch.from_numpy(np.ascontiguousarray(v, f32).ravel()))
        self.state = nv.PdState()
        for k in sizes:
            setattr(self.state, k, nv.ptr(self.arena.t[k]))
        self.state.m, self.state.n, self.state.rho, self.state.epsilon = m, n, case['rho'], case['epsilon']

    def bits(self):
        torch.cuda.synchronize()
        return self.arena.bits.cpu().numpy().copy()

    def read(self):
        torch.cuda.synchronize()
        out = {k: t.cpu().numpy() for k, t in self.arena.t.items()}
        for k in MATRICES:
            out[k] = out[k].reshape(self.m, self.n)
        return out


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, f32).ravel(), np.ascontiguousarray(b, f32).ravel()
    return np.array_equal(a.view(np.int32), b.view(np.int32))


def _run_and_check(nv, case):
    """One jamie_pd_step from `case`; asserts every property of the one-step test and returns the outputs."""
    d = Dev(nv, case)
    nv.pd_step(d.state, case['iteration'])
    got = d.read()
    assert d.arena.violations() == [], 'guard words changed'
    for k, want in (('G1', case['G1']), ('G2', case['G2']), ('alpha', case['alpha'])):
        assert _same_bits(got[k], want), f'{k} was written'
    # the workspaces were NaN: a NaN anywhere is a read of a partial sum that this call did not write
    for k in pu.STATE_KEYS + ('rowpart', 'colpart'):
        assert not np.isnan(got[k]).any(), f'NaN in {k}'
    bad = pu.check_one_step(case, got)
    assert bad == [], bad
    assert (got['F'] >= 0).all()
    return got


@pytest.mark.parametrize('spec', pu.one_step_specs(), ids=pu.spec_id)
def test_one_step_every_output(nv, spec):
    """m1, m2 against pd_step_ref within 4 x the float32 restatement's measured error; F against float64 of the device's own
    moments; rowsum, colsum against float64 sums of the device's F; S, Mu, Lambda against float64 of the device's sums (bounds
    derived in pd_util.py).  F >= 0, the inputs bit-unchanged, the guards intact, nothing NaN."""
    print(pu.spec_id(spec))
    _run_and_check(nv, pu.make_case(spec))


@pytest.mark.parametrize('m,n', pu.DYADIC_SHAPES)
def test_dyadic_state_is_exact(nv, m, n):
    """Every input a small multiple of a power of two (float4 path at 40 x 252, scalar path at 33 x 257): F, rowsum, colsum, S,
    Mu and Lambda equal the float64 reference bit for bit.  m1 and m2 equal the single roundings fl(fl(0.1) g) and fl(fl(fl(0.001)
    g) g) of the exact gradient g (pd_step_f32) bit for bit; no float32 result can equal the float64 one there, since 0.1 and
    0.001 are no float32 numbers (tests/test_host_correspondence.py::test_dyadic_states_are_exact)."""
    case = pu.dyadic(m, n)
    got = _run_and_check(nv, case)
    ref, _ = pu.run_ref(case)
    for k in ('F', 'rowsum', 'colsum', 'S', 'Mu', 'Lambda'):
        assert _same_bits(got[k], ref[k].astype(f32)), k
    plain = pu.run_f32(case)
    assert _same_bits(got['m1'], plain['m1']) and _same_bits(got['m2'], plain['m2'])


@pytest.mark.parametrize('m,n', [(32, 256), (33, 257)])
def test_true_first_iteration_is_constant(nv, m, n):
    """All zeros and alpha = sqrt(dy / dx): the gradient is -2 rho everywhere.  F is one value, the float32 rounding of the
    reference's; every vector is one value (each entry is summed in the same order), within the derived bounds of the
    reference (a sum of n equal terms is exact in no order, so bit equality is asked of F only)."""
    case = pu.zero(m, n, 1, 1e-3)
    got = _run_and_check(nv, case)
    ref, _ = pu.run_ref(case)
    for k in pu.STATE_KEYS:
        assert (got[k].view(np.int32) == got[k].view(np.int32).flat[0]).all(), f'{k} is not constant'
    assert _same_bits(got['F'], ref['F'].astype(f32)), (float(got['F'][0, 0]), float(ref['F'][0, 0]))
    assert got['m1'][0, 0] == f32(1 - pu.PHO1) * f32(-20) and got['m2'][0, 0] == (f32(1 - pu.PHO2) * f32(-20)) * f32(-20)


def test_same_element_on_the_float4_and_the_scalar_path(nv):
    """A 33 x 260 problem (float4 loads, a second column tile of four columns) embedded in a 33 x 261 one (scalar loads) whose
    shared columns have identical inputs, rowsum and colsum given explicitly: m1, m2 and F of the shared columns are
    bit-identical."""
    a = pu.adversarial(33, 260, 10, 1e-2)
    r = np.random.default_rng(5)
    wide = lambda M: np.concatenate([M, r.standard_normal((M.shape[0], 1)).astype(f32) ** 2], axis=1)   # noqa: E731
    more = lambda v: np.concatenate([v, np.abs(r.standard_normal(1)).astype(f32)])   # noqa: E731
    st = a['state']
    b_state = dict(F=wide(st['F']), m1=wide(st['m1']), m2=wide(st['m2']), Mu=st['Mu'], rowsum=st['rowsum'],
                   Lambda=more(st['Lambda']), S=more(st['S']), colsum=more(st['colsum']))
    b = dict(a, state=b_state, G1=wide(a['G1']), G2=wide(a['G2']))
    got_a, got_b = Dev(nv, a), Dev(nv, b)
    nv.pd_step(got_a.state, a['iteration'])
    nv.pd_step(got_b.state, b['iteration'])
    ra, rb = got_a.read(), got_b.read()
    assert got_a.arena.violations() == [] and got_b.arena.violations() == []
    for k in ('m1', 'm2', 'F'):
        assert _same_bits(ra[k], rb[k][:, :260]), k
        assert not _same_bits(rb[k][:, 260], b_state[k][:, 260])          # the extra column was updated too


def test_two_calls_from_the_same_state_are_bit_identical(nv):
    case = pu.adversarial(70, 260, 10, 1e-2)
    runs = []
    for _ in range(2):
        d = Dev(nv, case)
        nv.pd_step(d.state, case['iteration'])
        runs.append(d.read())
    for k in pu.STATE_KEYS:
        assert _same_bits(runs[0][k], runs[1][k]), k


# ---------------------------------------------------------------------------------------------------
# jamie_pd_alpha
# ---------------------------------------------------------------------------------------------------
def _alpha_arena(count, n_partials):
    return pu.Arena(dict(G2=max(count, 1), alpha=1, F=max(count, 1), partials=max(n_partials, 1)), ('G2', 'F'))


def _alpha_raw(nv, ar, count, n_partials, inv_trkk, G2=None):
    t = ar.t
    nv._call('jamie_pd_alpha', nv.ptr(t['G2'] if G2 is None else G2), nv.ptr(t['F']), count, nv.ptr(t['partials']), n_partials,
             float(inv_trkk), nv.ptr(t['alpha']), nv._stream())


@pytest.mark.parametrize('count', [1, 2, 3, 4, 5, 1023, 1024, 1025, 3073, 262147])
def test_pd_alpha(nv, count):
    """sum(G2 o F) / tr(Kx Kx) for signed inputs against the float64 dot product within the chain-length bound of the launch
    (pd_util.alpha_chain); small integers exactly.  n_partials of 1 to 3 forces the grid-stride loop at the larger counts.  The
    partials buffer is NaN before every call: the entries beyond the grid keep their bits and none reaches alpha; G2 and F are
    not written; the guards stay intact."""
    r = np.random.default_rng(count)
    inv = float(f32(0.37))
    for n_partials in (1, 2, 3, 2048):
        for kind in ('normal', 'integer'):
            if kind == 'normal':
                x, y, scale = r.standard_normal(count).astype(f32), r.standard_normal(count).astype(f32), inv
            else:
                x, y, scale = r.integers(-3, 4, count).astype(f32), r.integers(-3, 4, count).astype(f32), 0.25
            ar = _alpha_arena(count, n_partials)
            ar.t['G2'].copy_(torch.from_numpy(x))
            ar.t['F'].copy_(torch.from_numpy(y))
            nv.pd_alpha(ar.t['G2'], ar.t['F'], ar.t['partials'], scale, ar.t['alpha'])
            torch.cuda.synchronize()
            got = float(ar.t['alpha'].item())
            want = float(np.dot(x.astype(np.float64), y.astype(np.float64))) * scale
            grid = pu.alpha_grid(count, n_partials)
            part = ar.t['partials'].cpu().numpy()
            assert ar.violations() == []
            assert np.isfinite(part[:grid]).all() and (part[grid:].view(np.int32) == np.int32(pu.SENTINEL_BITS)).all()
            assert _same_bits(ar.t['G2'].cpu().numpy(), x) and _same_bits(ar.t['F'].cpu().numpy(), y)
            if kind == 'integer':
                assert got == want, (n_partials, got, want)
            else:
                bound = pu.alpha_bound(x, y, scale, n_partials)
                print(f'count {count} n_partials {n_partials} grid {grid}: error / bound = {abs(got - want) / bound:.3f}')
                assert abs(got - want) <= bound, (n_partials, got, want, bound)


def test_pd_alpha_of_a_zero_product_is_nan(nv):
    """G2 = 0 (a zero Kx) with 1 / tr(Kx Kx) = inf: 0 * inf = NaN, the reference's 0 / 0."""
    ar = _alpha_arena(1025, 2048)
    ar.t['G2'].zero_()
    ar.t['F'].fill_(0.5)
    nv.pd_alpha(ar.t['G2'], ar.t['F'], ar.t['partials'], float('inf'), ar.t['alpha'])
    torch.cuda.synchronize()
    assert math.isnan(float(ar.t['alpha'].item())) and ar.violations() == []
    assert float(ar.t['partials'][0].item()) == 0.0


# ---------------------------------------------------------------------------------------------------
# argument errors come before a launch
# ---------------------------------------------------------------------------------------------------
def test_pd_step_argument_errors_launch_nothing(nv):
    case = pu.adversarial(33, 257, 10, 1e-2)
    d = Dev(nv, case)
    before = d.bits()

    def attempt(iteration=10, **change):
        st = nv.PdState()
        for name, _ in nv.PdState._fields_:
            setattr(st, name, getattr(d.state, name))
        for k, v in change.items():
            setattr(st, k, v)
        with pytest.raises(nv.JamieHipError):
            nv.pd_step(st, iteration)
        assert np.array_equal(d.bits(), before), f'{change or iteration}: memory changed'

    for member in ('F', 'G2', 'S', 'alpha', 'colpart'):
        attempt(**{member: None})
    attempt(m=0)
    attempt(n=0)
    attempt(iteration=0)
    attempt(F=d.state.F + 4)                       # one float off the 16-byte boundary
    attempt(m2=d.state.m2 + 4)
    nv.pd_step(d.state, 10)                        # and the untouched state still runs
    assert not np.array_equal(d.bits(), before) and d.arena.violations() == []


def test_pd_alpha_argument_errors_launch_nothing(nv):
    ar = _alpha_arena(1028, 4097)
    ar.t['G2'].fill_(1.0)
    ar.t['F'].fill_(1.0)
    torch.cuda.synchronize()
    before = ar.bits.cpu().numpy().copy()
    limit = nv.load().jamie_max_partials()
    assert limit == 4096
    for kw in (dict(count=0, n_partials=8), dict(count=1028, n_partials=0), dict(count=1028, n_partials=limit + 1),
               dict(count=1024, n_partials=8, G2=ar.t['G2'][1:])):
        with pytest.raises(nv.JamieHipError):
            _alpha_raw(nv, ar, kw['count'], kw['n_partials'], 1.0, G2=kw.get('G2'))
        torch.cuda.synchronize()
        assert np.array_equal(ar.bits.cpu().numpy(), before), kw
    _alpha_raw(nv, ar, 1028, limit, 0.5)
    torch.cuda.synchronize()
    assert float(ar.t['alpha'].item()) == 514.0


# ---------------------------------------------------------------------------------------------------
# PrimeDual: the host side and the four products
# ---------------------------------------------------------------------------------------------------
def _np64(t):
    return t.detach().double().cpu().numpy()


def _within(name, got, want, bound):
    err = np.abs(got - want)
    ratio = float(np.max(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))))
    print(f'  {name}: max error / bound = {ratio:.3f}')
    assert ratio <= 1.0, name


@pytest.mark.parametrize('gemm_cfg', [None, 17])
@pytest.mark.parametrize('m,n', [(130, 117), (64, 512)])
def test_prime_dual_products_after_each_of_four_steps(nv, m, n, gemm_cfg):
    """After step k = 1..4 (delay 3): FKy = F Ky and G2 = Kx FKy of the new F, T1 = F^T FKy and G1 = FKy T1 of the F held before
    the step, each against the float64 product of the device's own operands within K 2^-24 (|A| |B|) (K roundings of the inner
    dimension); alpha against the float64 trace formula of the device's F; the iteration count and the delay rule: alpha
    keeps the bits of sqrt(dy / dx) below `delay` and changes at it."""
    from jamie_amd.correspondence import PrimeDual
    Kx, Ky = pu.distances(m, n, seed=2)
    delay = 3
    pd = PrimeDual(Kx, Ky, pu.DX, pu.DY, rho=pu.RHO, epsilon=1e-2, delay=delay, gemm_cfg=gemm_cfg)
    assert pd.gemm_cfg == (-1 if gemm_cfg is None else 17)
    Kx64, Ky64 = _np64(pd.Kx), _np64(pd.Ky)
    trkk = float((Kx64 * Kx64.T).sum())
    assert abs(pd.inv_trkk * trkk - 1) < 1e-12
    a0 = f32(math.sqrt(pu.DY / pu.DX))
    for k in range(1, 5):
        F_prev, FKy_prev = _np64(pd.F), _np64(pd.FKy)
        pd.step()
        torch.cuda.synchronize()
        print(f'step {k}')
        assert pd.iteration == k
        F, FKy, G1, G2, T1 = (_np64(x) for x in (pd.F, pd.FKy, pd.G1, pd.G2, pd.T1))
        _within('FKy', FKy, F @ Ky64, n * pu.U * (np.abs(F) @ np.abs(Ky64)))
        _within('G2', G2, Kx64 @ FKy, m * pu.U * (np.abs(Kx64) @ np.abs(FKy)))
        if k == 1:
            assert not T1.any() and not G1.any()
        else:
            _within('T1', T1, F_prev.T @ FKy_prev, m * pu.U * (np.abs(F_prev).T @ np.abs(FKy_prev)))
            _within('G1', G1, FKy_prev @ T1, n * pu.U * (np.abs(FKy_prev) @ np.abs(T1)))
        alpha = pd.alpha.cpu().numpy()[0]
        if k < delay:
            assert alpha.view(np.int32) == a0.view(np.int32)
        else:
            assert alpha != a0
            want = np.trace(Kx64 @ ((F @ Ky64) @ F.T)) / np.trace(Kx64 @ Kx64)
            # G2's own bound (above, with FKy's inside it) summed against F, then the chain of the dot product and the rounding
            # of 1 / tr(Kx Kx) to float32
            g2_err = m * pu.U * (np.abs(Kx64) @ np.abs(FKy)) + np.abs(Kx64) @ (n * pu.U * (np.abs(F) @ np.abs(Ky64)))
            chain = pu.alpha_chain(m * n, 2048) + 1
            bound = ((g2_err * np.abs(F)).sum() + chain * pu.U * np.abs(G2 * F).sum()) / trkk
            print(f'  alpha {alpha:.6f}: error / bound = {abs(alpha - want) / bound:.3f}')
            assert abs(alpha - want) <= bound


def test_inv_trkk_of_a_non_symmetric_kx_beyond_one_chunk(nv):
    """4097 rows: the chunked tr(Kx Kx) of PrimeDual.__init__ takes a second block, and with a non-symmetric Kx a missing
    transpose would show: 1 / sum(Kx o Kx^T), not 1 / sum(Kx o Kx).  Then one step() of this 4097 x 8 problem (129 row tiles)
    passes the one-step checks."""
    from jamie_amd.correspondence import PrimeDual
    m, n = 4097, 8
    r = np.random.default_rng(7)
    Kx, Ky = r.random((m, m)), pu.distances(n, n, seed=3)[1]
    eps = 1e-2
    pd = PrimeDual(Kx, Ky, pu.DX, pu.DY, rho=pu.RHO, epsilon=eps)
    Kxs = (Kx / m).astype(f32).astype(np.float64)
    assert np.array_equal(Kxs, _np64(pd.Kx))
    want, wrong = 1.0 / float((Kxs * Kxs.T).sum()), 1.0 / float((Kxs * Kxs).sum())
    assert abs(wrong / want - 1) > 1e-2                      # the two readings are far apart for this Kx
    assert abs(pd.inv_trkk / want - 1) <= 1e-6
    case = pu.zero(m, n, 1, eps)
    pd.rowpart.fill_(float('nan'))
    pd.colpart.fill_(float('nan'))
    pd.step()
    torch.cuda.synchronize()
    got = {k: getattr(pd, k).cpu().numpy() for k in pu.STATE_KEYS}
    assert pu.check_one_step(case, got) == [] and (got['F'] >= 0).all()
    G2 = _np64(pd.G2)
    alpha = float(pd.alpha.item())
    want_a = float((G2 * got['F']).sum()) * pd.inv_trkk
    assert abs(alpha - want_a) <= pu.alpha_bound(G2, got['F'], pd.inv_trkk, 2048) + 2 * pu.U * abs(want_a)   # (+ 1 / tr as float32)

"""The reference the one-step Prime_Dual GPU tests (tests/test_hip_prime_dual.py) compare against, checked on the CPU:
pd_step_ref iterated against the float64 oracle and the reference's golden, the staged references against pd_step_ref, the
float32 restatement that fixes the moment bounds, the derived bounds on plain float32 arithmetic, and the dyadic states."""
import ast
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pd_util as pu  # noqa: E402
from oracle import jamie_oracle as orc  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), 'golden')


@pytest.fixture(scope='module')
def cases():
    return pu.measured_cases()


@pytest.mark.parametrize('m,n,delay,eps', [(13, 9, 0, 1e-3), (10, 17, 5, 1e-2)])
def test_iterated_reference_reproduces_the_float64_oracle(m, n, delay, eps):
    """20 iterations of pd_step_ref with the seven products in float64 numpy against orc.prime_dual(dtype=float64).  The
    scaling factor, a float64 function of the whole of F, agrees to 1e-12 in every iteration; the oracle hands F back rounded
    to float32, so F agrees to that rounding (2^-24 relative) on top of 1e-12."""
    Kx, Ky = pu.distances(m, n, seed=1)
    hist, mine = [], []
    want = orc.prime_dual(Kx, Ky, pu.DX, pu.DY, 20, pu.RHO, eps, delay, dtype=torch.float64, history=hist)
    st = pu.pd_iterate_ref(Kx, Ky, pu.DX, pu.DY, 20, pu.RHO, eps, delay, history=mine)
    np.testing.assert_allclose(mine, hist, rtol=1e-12, atol=0)
    assert mine[0] == np.sqrt(pu.DY / pu.DX) if delay > 1 else mine[0] != np.sqrt(pu.DY / pu.DX)
    err = np.abs(st['F'] - want.astype(np.float64))
    assert (err <= (pu.U + 1e-12) * np.abs(st['F'])).all(), float((err / np.abs(st['F']).max()).max())
    # the form the warm states are made with (no [m, m] product for the scaling factor) is the same iteration
    fast = []
    st2 = pu.pd_iterate_ref(Kx, Ky, pu.DX, pu.DY, 20, pu.RHO, eps, delay, literal=False, history=fast)
    np.testing.assert_allclose(fast, hist, rtol=1e-12, atol=0)
    np.testing.assert_allclose(st2['F'], st['F'], rtol=1e-12, atol=0)


def test_iterated_reference_stays_within_the_golden_tolerance():
    """All 150 iterations of tests/golden/pd1_delay0.npz (the reference's own float32 run) within the tolerance the device
    run is held to (test_hip_correspondence.py)."""
    g = np.load(os.path.join(GOLD, 'pd1_delay0.npz'))
    meta = ast.literal_eval(str(g['meta']))
    st = pu.pd_iterate_ref(g['Kx'], g['Ky'], meta['dx'], meta['dy'], meta['epoch_pd'], meta['rho'], meta['epsilon'], meta['delay'])
    np.testing.assert_allclose(st['F'], g['F'], rtol=2e-3, atol=2e-6)
    assert np.linalg.norm(st['F'] - g['F']) / np.linalg.norm(g['F']) < 2e-4


def test_staged_references_compose_to_the_one_step_reference(cases):
    """f_from_moments, sums and duals chained equal pd_step_ref (which forms everything with column vectors and products with
    vectors of ones) to the last bits of float64."""
    for name, c in cases:
        ref, _ = pu.run_ref(c)
        got = pu.pd_step_staged(c['state'], c['G1'], c['G2'], c['alpha'], c['iteration'], c['rho'], c['epsilon'])
        for k in pu.STATE_KEYS:
            np.testing.assert_allclose(got[k], ref[k], rtol=1e-13, atol=1e-300, err_msg=f'{name} {k}')


def test_case_list_covers_what_the_issue_names():
    adv = [c for _, c in pu.one_step_cases() if c['name'] == 'adversarial']
    assert {c['state']['F'].shape for c in adv} == set(pu.SHAPES)
    assert {c['iteration'] for c in adv} == set(pu.ITERATIONS)
    assert {c['epsilon'] for c in adv} == set(pu.EPSILONS)
    assert {c['name'] for _, c in pu.one_step_cases()} == {'zero', 'warm', 'adversarial'}
    ids = [i for i, _ in pu.measured_cases()]
    assert len(ids) == len(set(ids))


def test_adversarial_states_are_what_they_claim():
    for m, n, it, eps in ((33, 257, 10, 1e-2), (97, 1024, 100000, 1e-3)):
        c = pu.adversarial(m, n, it, eps)
        st = c['state']
        assert (st['F'] >= 0).all() and (st['F'] == 0).mean() > 0.1 and (st['m2'] >= 0).all() and (st['m2'] == 0).any()
        assert (st['m1'] < 0).any() and (st['m1'] > 0).any() and (st['Mu'] < 0).any() and (st['Lambda'] < 0).any()
        assert (st['S'] == 0).any()
        # the gradient's two large terms cancel to ~1e-3 of their size
        big = 4 * np.abs(c['G1'].astype(np.float64))
        assert np.median(np.abs(4 * c['G1'].astype(np.float64) - 4 * float(c['alpha']) * c['G2']) / big) < 2e-3
        # a share of the columns sits within a few float32 ulp (times rho) of the slack update's kink
        ref, _ = pu.run_ref(c)
        S, lam = st['S'].astype(np.float64), st['Lambda'].astype(np.float64)
        arg = S - (lam + c['rho'] * (ref['colsum'] - 1 + S))
        near = np.abs(arg) <= 8 * c['rho'] * np.spacing(np.abs(st['S']) + np.float32(1)).astype(np.float64)
        assert near.mean() > 0.2, near.mean()
        assert (arg[near] > 0).any() and (arg[near] < 0).any()


def test_fp32_restatement_fixes_the_moment_bounds(cases):
    """pd_step_f32 against pd_step_ref over every state family, shape and iteration number of the GPU tests: the two maxima are
    the constants F32_E_M1 and F32_E_M2 of pd_util.py, and the GPU bounds are 4 times them."""
    worst = {'m1': (0.0, ''), 'm2': (0.0, '')}
    for name, c in cases:
        ref, T = pu.run_ref(c)
        got = pu.run_f32(c)
        e1, e2 = pu.moment_errors(got['m1'], got['m2'], ref, c['state'], T)
        print(f'{name}: e_m1 {e1:.4e} e_m2 {e2:.4e}')
        worst['m1'] = max(worst['m1'], (e1, name))
        worst['m2'] = max(worst['m2'], (e2, name))
    print('pd_step_f32 against the float64 reference:', worst)
    assert 0.9 * pu.F32_E_M1 <= worst['m1'][0] <= pu.F32_E_M1, worst
    assert 0.9 * pu.F32_E_M2 <= worst['m2'][0] <= pu.F32_E_M2, worst
    assert (pu.BOUND_M1, pu.BOUND_M2) == (4 * pu.F32_E_M1, 4 * pu.F32_E_M2)


def test_derived_bounds_hold_for_plain_float32_arithmetic(cases):
    """The bounds of pd_util.py (F given the moments, the sums of k non-negative terms, the dual updates; each derived in its
    docstring) hold for the numpy float32 restatement in every case, each stage against float64 of the restatement's own
    upstream values, exactly as the GPU test applies them; and the dual bounds stay under `4 roundings of |Lambda| + rho(|cs| +
    1 + |S|)`."""
    for name, c in cases:
        got = pu.run_f32(c)
        print(name)
        assert pu.check_one_step(c, got) == [], name
        st = c['state']
        tight = pu.dual_bounds(st['S'], st['Mu'], st['Lambda'], got['rowsum'], got['colsum'], c['rho'], c['epsilon'])
        plain = pu.plain_dual_bounds(st['S'], st['Mu'], st['Lambda'], got['rowsum'], got['colsum'], c['rho'])
        for t, p in zip(tight, plain):
            assert (t <= p).all(), name


def test_one_step_check_sees_a_wrong_constant():
    """check_one_step is not vacuous: the restatement with `- 2` dropped from the column term, or with the old slack in the
    Lambda update, fails it."""
    c = pu.adversarial(33, 257, 10, 1e-2)
    good = pu.run_f32(c)
    shifted = dict(c, state=dict(c['state'], colsum=c['state']['colsum'] + np.float32(2)))
    bad = dict(good, m1=pu.run_f32(shifted)['m1'])
    assert any(s.startswith('m1') for s in pu.check_one_step(c, bad, say=lambda s: None))
    eps, st = np.float32(c['epsilon']), c['state']
    old_s = dict(good, Lambda=st['Lambda'] + eps * ((good['colsum'] - np.float32(1)) + st['S']))
    assert any(s.startswith('Lambda') for s in pu.check_one_step(c, old_s, say=lambda s: None))


@pytest.mark.parametrize('m,n', pu.DYADIC_SHAPES)
def test_dyadic_states_are_exact(m, n):
    """On a dyadic state the gradient, F, the sums, the slack and the duals of the float32 restatement equal the float64
    reference bit for bit.  The moments cannot: 0.1 and 0.001 are no float32 numbers, so m1 = fl(fl(0.1) g) and m2 =
    fl(fl(fl(0.001) g) g) of the exact gradient g, at most 1.5 and 2.5 ulp from the float64 value."""
    c = pu.dyadic(m, n)
    ref, _ = pu.run_ref(c)
    got = pu.run_f32(c)
    f = np.float32
    for k in ('F', 'rowsum', 'colsum', 'S', 'Mu', 'Lambda', 'grad'):
        assert np.array_equal(ref[k].astype(f).astype(np.float64), ref[k]), f'{k} is not a float32 number'
    for k in ('F', 'rowsum', 'colsum', 'S', 'Mu', 'Lambda'):
        assert np.array_equal(got[k], ref[k].astype(f)), k
    g = ref['grad'].astype(f)
    assert (g >= 4).all()
    assert np.array_equal(got['m1'], f(1 - pu.PHO1) * g) and np.array_equal(got['m2'], (f(1 - pu.PHO2) * g) * g)
    assert (np.abs(got['m1'] - ref['m1']) <= 1.5 * np.spacing(got['m1'])).all()
    assert (np.abs(got['m2'] - ref['m2']) <= 2.5 * np.spacing(got['m2'])).all()
    # both sides of the slack's kink occur, and F really moved
    arg = c['state']['S'] - (c['state']['Lambda'] + c['rho'] * (ref['colsum'] - 1 + c['state']['S']))
    assert (arg > 0).any() and (arg < 0).any() and (ref['S'] != c['state']['S']).any()
    assert np.array_equal(ref['F'], (1 - pu.DYADIC_EPSILON) * c['state']['F']) and (ref['F'] > 0).any()


def test_first_iteration_is_constant():
    """All zeros, alpha = sqrt(dy / dx): the gradient is -2 rho everywhere, so F and every vector are constant."""
    c = pu.zero(33, 257, 1, 1e-3)
    ref, T = pu.run_ref(c)
    assert (ref['grad'] == -2 * pu.RHO).all() and (T == 2 * pu.RHO).all()
    for k in pu.STATE_KEYS:
        assert np.ptp(ref[k]) <= 1e-15 * np.abs(ref[k]).max(), k
    np.testing.assert_allclose(ref['F'], 1e-3 * (1 - pu.DELTA / 20), rtol=1e-9)


@pytest.mark.parametrize('count,n_partials,grid,trips', [(1, 2048, 1, 0), (5, 1, 1, 1), (1025, 2048, 1, 1), (1028, 2048, 2, 1), (3073, 2, 2, 2),
                                                         (262147, 3, 3, 86), (262147, 2048, 256, 1), (262147, 1, 1, 256)])
def test_alpha_chain_follows_the_launch(count, n_partials, grid, trips):
    """alpha_grid / alpha_chain state the launch jamie_pd_alpha makes (one block per 1024 elements, clamped to n_partials) and
    the chain of roundings of its summation order; float32 arithmetic along a tree of that shape lies inside the bound they
    give, and is exact on small integers."""
    assert pu.alpha_grid(count, n_partials) == grid
    assert pu.alpha_chain(count, n_partials) == 3 + trips + 1 + 10 + 1 + 10 + 1
    r = np.random.default_rng(count)
    x, y = r.standard_normal(count).astype(np.float32), r.standard_normal(count).astype(np.float32)
    inv = float(np.float32(0.37))
    want = float(np.dot(x.astype(np.float64), y.astype(np.float64))) * inv
    err, bound = abs(float(pu.alpha_f32(x, y, inv, n_partials)) - want), pu.alpha_bound(x, y, inv, n_partials)
    print(f'count {count} n_partials {n_partials}: error / bound = {err / bound:.3f}')
    assert err <= bound
    xi, yi = r.integers(-3, 4, count).astype(np.float32), r.integers(-3, 4, count).astype(np.float32)
    assert float(pu.alpha_f32(xi, yi, 0.25, n_partials)) == float(np.dot(xi.astype(np.float64), yi)) * 0.25

"""The reference the GPU optimiser tests (tests/test_hip_optim.py) compare against, checked on the CPU: adam_ref against real
torch, the fp32 restatement that fixes the GPU bounds, the distance between the two readings of the hyper-parameters, and the
oracle on non-finite gradients."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_util as ou  # noqa: E402
from oracle import jamie_oracle as orc  # noqa: E402

N_HOST = 100_003
HOST_T = (1, 10, 1000, 100_000)


@pytest.mark.parametrize('hyper', [ou.DEFAULT, ou.NON_DEFAULT], ids=['default', 'non-default'])
@pytest.mark.parametrize('p_scale', [1e-3, 1.0])
@pytest.mark.parametrize('t', HOST_T)
def test_reference_equals_torch_clip_and_adam(t, p_scale, hyper):
    """adam_ref(hyper_as='torch') is clip_grad_norm_ + torch.optim.Adam in float64, from injected warm state."""
    c = ou.warm(N_HOST, t, p_scale, hyper=hyper)
    p = torch.nn.Parameter(c['p0'].double().clone())
    p.grad = c['g'].double().clone()
    opt = torch.optim.Adam([p], lr=hyper.lr, betas=(hyper.b1, hyper.b2), eps=hyper.eps)
    opt.state[p] = {'step': torch.tensor(float(t - 1)), 'exp_avg': c['m0'].double().clone(),
                    'exp_avg_sq': c['v0'].double().clone()}
    total = torch.nn.utils.clip_grad_norm_([p], hyper.max_norm)
    opt.step()
    ref = ou.ref_of(c, 'torch')
    assert float(opt.state[p]['step']) == t
    assert abs(float(total) - float(ref['total'])) <= 1e-12 * float(total)
    e_p, e_m, e_v = ou.scaled_errors(p.detach(), opt.state[p]['exp_avg'], opt.state[p]['exp_avg_sq'], ref)
    print(f't={t} p_scale={p_scale}: e_p {e_p:.2e} e_m {e_m:.2e} e_v {e_v:.2e}')
    assert e_m <= 1e-12 and e_v <= 1e-12
    # the update itself, p' - p0 (e_p's scale holds |p0| as well)
    d, dr = p.detach() - ref['p0'], ref['p'] - ref['p0']
    assert float((d - dr).abs().max()) <= 1e-12 * float(dr.abs().max())
    assert e_p <= 1e-12


def test_fp32_restatement_stays_below_the_recorded_errors():
    """adam_f32 against adam_ref('given') over every input family and size of the GPU tests: the three maxima are the
    constants F32_E_* of optim_util.py, and the GPU bounds are 4 times them."""
    worst = {}
    for name, n, c in ou.measured_cases():
        ref = ou.ref_of(c)
        e = ou.scaled_errors(*ou.adam_f32(c['p0'], c['g'], c['m0'], c['v0'], c['t'], c['hyper'], c['g_norm']), ref)
        for k, x in zip('pmv', e):
            if x > worst.get(k, (0, ''))[0]:
                worst[k] = (x, f'{name} n={n}')
    print('adam_f32 against the float64 reference:', worst)
    assert worst['p'][0] <= ou.F32_E_P and worst['m'][0] <= ou.F32_E_M and worst['v'][0] <= ou.F32_E_V, worst
    # the constants are the measurement, not a loose cap on it
    assert worst['p'][0] >= 0.9 * ou.F32_E_P and worst['m'][0] >= 0.9 * ou.F32_E_M and worst['v'][0] >= 0.9 * ou.F32_E_V, worst
    assert (ou.BOUND_P, ou.BOUND_M, ou.BOUND_V) == (4 * ou.F32_E_P, 4 * ou.F32_E_M, 4 * ou.F32_E_V)


def test_distance_between_the_given_and_the_torch_hyper_parameters():
    """What handing the kernel fl32(0.999) and letting it form 1.f - beta2 costs against torch's double 1 - 0.999, in float64:
    e_v = |fl32(0.999) - 0.999| / 0.001 = 1.29e-5 at every t.  With the two 1 - beta slots filled the distance is gone."""
    worst_p = worst_v = 0.0
    for p_scale in (1e-3, 1.0):
        for t in HOST_T:
            c = ou.warm(N_HOST, t, p_scale)
            rt, rg = ou.ref_of(c, 'torch'), ou.ref_of(c, 'given')
            e_p, e_m, e_v = ou.scaled_errors(rg['p'], rg['m'], rg['v'], rt)
            print(f't={t} p_scale={p_scale}: e_p {e_p:.3e} e_m {e_m:.3e} e_v {e_v:.3e}')
            assert 1.2e-5 <= e_v <= ou.GIVEN_VS_TORCH_E_V
            assert e_m <= 2.5e-7                      # |fl32(0.9) - 0.9| / 0.1 = 2.4e-7
            worst_p, worst_v = max(worst_p, e_p), max(worst_v, e_v)
            c['hyper'] = ou.Hyper(slots=True)
            rs = ou.ref_of(c, 'given')
            s_p, s_m, s_v = ou.scaled_errors(rs['p'], rs['m'], rs['v'], rt)
            # what is left is one fp32 rounding of each hyper-parameter (|fl32(0.1) - 0.1| / 0.1 = 1.5e-8,
            # |fl32(0.001) - 0.001| / 0.001 = 4.7e-8), and on p the same cancellation in m' that fp32 arithmetic meets
            assert s_p <= ou.F32_E_P and s_m <= 1.5e-8 and s_v <= 4.8e-8, (s_p, s_m, s_v)
    assert worst_v > ou.BOUND_V                        # many times what the GPU tests allow: it cannot hide in the bound
    assert 0.9 * ou.GIVEN_VS_TORCH_E_P <= worst_p <= ou.GIVEN_VS_TORCH_E_P


def test_hyper_tensor_rounds_once():
    """The fp32 block the tests hand the kernel: python doubles rounded once, 1 - beta formed in double (engine.py writes the
    same; tests/test_hip_optim.py compares the two on the GPU)."""
    h = ou.Hyper(slots=True).tensor()
    e = torch.zeros(16)
    e[8], e[9], e[10], e[11], e[12], e[13], e[14], e[15] = 1e-3, 0.9, 0.999, 1e-8, 1.0, 1.0, 1 - 0.9, 1 - 0.999
    assert torch.equal(h, e)
    assert float(h[15]) == float(torch.tensor(0.001)) and float(1 - h[10]) != float(h[15])
    assert torch.equal(ou.DEFAULT.tensor()[14:], torch.zeros(2))


@pytest.mark.parametrize('bad', [float('nan'), float('inf')])
def test_oracle_clip_on_non_finite_gradients(bad):
    """clip_grad_norm_ clamps a NaN norm to a NaN coefficient (every gradient becomes NaN); an inf norm gives coefficient 0
    (finite entries 0, the inf one NaN).  adam_ref does the same."""
    grads = [torch.tensor([1.0, 2.0]), torch.tensor([bad, 3.0])]
    orc.clip_grad_norm(grads)
    flat = torch.cat(grads)
    if bad != bad:
        assert bool(torch.isnan(flat).all())
    else:
        assert torch.equal(flat[[0, 1, 3]], torch.zeros(3)) and bool(torch.isnan(flat[2]))
    z = torch.zeros(4)
    ref = ou.adam_ref(z, torch.tensor([1.0, 2.0, bad, 3.0]), z, z, 1, ou.DEFAULT)
    assert torch.equal(torch.isnan(ref['gg']), torch.isnan(flat)) and torch.equal(torch.isnan(ref['p']), torch.isnan(flat))

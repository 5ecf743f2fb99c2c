"""csrc/optim.hip against the float64 reference of tests/optim_util.py: the sum-of-squares kernels, the partial sums as
clip + Adam re-adds them, and one clip + Adam step from arbitrary state with an fp32 and with a bf16 gradient.
Run on the MI355X box:  pytest -m gpu tests/test_hip_optim.py

The sizes below sit on the launch shapes, which are compile-time constants of optim.hip -- a retune has to move them:
  jamie_grad_sqnorm[_bf16]: 256 threads, one float4 (8 bf16) per lane, <= 2048 workgroups -> one grid is 2 097 152 floats;
                            workgroup 0 adds the scalar tail (n mod 4, n mod 8).
  jamie_clip_adam[_g16]:    JAMIE_ADAM_T = 512 threads x JAMIE_ADAM_U = 1 float4, <= JAMIE_ADAM_GRID = 256 streaming workgroups
                            -> one workgroup covers 2048 elements, one sweep 524 288; workgroup 0 updates the tail (n mod 4).
  partial sums:             every workgroup re-adds all of them, 8 x 512 = 4096 up front, then a loop in rounds of 4096, up to
                            JAMIE_MAX_NORM_PARTIALS = 32768."""
import dataclasses
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_util as ou  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINELS = 64
SENTINEL = -7.5                  # exact in fp32 and bf16
MAX_PARTIALS = 32768
SQ_SIZES = [1, 2, 3, 4, 5, 7, 8, 9, 15, 1023, 1024, 1025, 4099, 2_097_152, 2_097_156, 3_000_017]
STEP_SIZES = [1, 3, 4, 5, 2047, 2048, 2049, 524_288, 524_292, 526_339, 1_048_583, 3_000_017]
PARTIAL_LENGTHS = [1, 2, 511, 512, 513, 4095, 4096, 4097, 8191, 8192, 8193, 12289, 32768]


@pytest.fixture(scope='module')
def nv():
    from jamie_amd import _native
    _native.require_gpu()
    return _native


def padded(t):
    """A device copy of `t` with SENTINELS sentinel elements behind it: (whole buffer, view of the first n)."""
    n = t.numel()
    full = torch.full((n + SENTINELS,), SENTINEL, dtype=t.dtype, device='cuda')
    full[:n] = t.cuda()
    return full, full[:n]


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def sentinels_intact(full):
    return bool((full[-SENTINELS:] == SENTINEL).all())


def new_state(step):
    return torch.tensor([0, step, 0, 0], dtype=torch.int64, device='cuda')


def nan_partials(nv, n):
    return torch.full((nv.optim_blocks(n),), float('nan'), device='cuda')


def run_step(nv, c, with_bf16=True, slices=None):
    """The norm launch and clip + Adam on padded device copies of the case `c`, with the assertions every launch must meet.
    `slices`: cut points; clip + Adam then runs once per slice on views that share the partial sums.  Returns CPU tensors."""
    n, t = c['p0'].numel(), c['t']
    bufs = {k: padded(c[k]) for k in ('p0', 'g', 'm0', 'v0')}
    (pf, p), (gf, g), (mf, m), (vf, v) = (bufs[k] for k in ('p0', 'g', 'm0', 'v0'))
    gnf, gn = padded(c['g_norm']) if c['g_norm'] is not None else (gf, g)
    bf, b = padded(torch.zeros(n, dtype=torch.bfloat16)) if with_bf16 else (None, None)
    g_before, gn_before = bits(gf).clone(), bits(gnf).clone()
    hyper = c['hyper'].tensor().cuda()
    state = new_state(t - 1)                                   # a resumed run: the norm launch moves it to t
    part = nan_partials(nv, n)
    nv.grad_sqnorm(gn, part, state)
    assert state.tolist() == [0, t, 0, 0]
    cuts = [0] + list(slices or []) + [n]
    for a, e in zip(cuts[:-1], cuts[1:]):
        nv.clip_adam(p[a:e], g[a:e], m[a:e], v[a:e], part, hyper, state, None if b is None else b[a:e])
    torch.cuda.synchronize()
    assert state.tolist() == [0, t, 0, 0]
    assert all(sentinels_intact(x) for x in (pf, mf, vf, gf, gnf) + ((bf,) if with_bf16 else ())), 'a sentinel was overwritten'
    assert torch.equal(bits(gf), g_before) and torch.equal(bits(gnf), gn_before), 'the gradient was modified'
    assert torch.equal(hyper.cpu(), c['hyper'].tensor())
    return dict(p=p.cpu(), m=m.cpu(), v=v.cpu(), pb=b.cpu() if with_bf16 else None, part=part.cpu())


@functools.lru_cache(maxsize=2)
def case_and_ref(n, name, hyper_as='given', slots=False):
    c = ou.family(n, name)
    if slots:
        c['hyper'] = dataclasses.replace(c['hyper'], slots=True)
    return c, ou.ref_of(c, hyper_as)


def check_step(out, ref, label):
    e_p, e_m, e_v = ou.scaled_errors(out['p'], out['m'], out['v'], ref)
    print(f'OPTIM {label} e_p={e_p:.3e} e_m={e_m:.3e} e_v={e_v:.3e}')
    assert e_p <= ou.BOUND_P and e_m <= ou.BOUND_M and e_v <= ou.BOUND_V, (label, e_p, e_m, e_v)
    if out['pb'] is not None:      # the bf16 weight copy is the rounding of the kernel's own new p, tail included
        assert torch.equal(bits(out['pb']), bits(out['p'].to(torch.bfloat16))), f'{label}: p_bf16'
    return e_p, e_m, e_v


def same_bits(a, b, keys=('p', 'm', 'v')):
    return all(torch.equal(bits(a[k]), bits(b[k])) for k in keys)


# ------------------------------------------------------------------------------------------------
# sum of squares
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('n', SQ_SIZES)
def test_sum_of_squares(nv, n, dtype):
    r = torch.Generator().manual_seed(n)
    data = [torch.randn(n, generator=r).to(dtype)]
    if n <= 131_072:     # integers in -8..8: the sum stays below 2^24 and is exact in any order -- a dropped or doubly counted
        data.append(torch.randint(-8, 9, (n,), generator=r).to(dtype))         # element shows as an integer difference
    for exact, gc in zip((False, True), data):
        gf, g = padded(gc)
        before = bits(gf).clone()
        part = nan_partials(nv, n)
        state = new_state(41)
        nv.grad_sqnorm(g, part, state)
        torch.cuda.synchronize()
        assert state.tolist() == [0, 42, 0, 0]
        assert torch.equal(bits(gf), before)
        assert bool(torch.isfinite(part).all()), 'a partial sum was not written'
        got, want = float(part.double().sum()), float((gc.double() ** 2).sum())
        print(f'OPTIM sqnorm n={n} {dtype} exact={exact} rel={abs(got - want) / max(want, 1e-300):.3e}')
        if exact:
            assert got == want
        else:
            assert abs(got - want) <= ou.SUMSQ_RTOL * want
        again = nan_partials(nv, n)
        nv.grad_sqnorm(g, again, None)                 # no state: nothing to count
        torch.cuda.synchronize()
        assert torch.equal(again, part) and state.tolist() == [0, 42, 0, 0]


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_sum_of_squares_argument_checks(nv, dtype):
    n = 4099
    g = torch.ones(n + 8, dtype=dtype, device='cuda')
    state = new_state(0)
    nb = nv.optim_blocks(n)
    for bad in (nb - 1, nb + 1):
        with pytest.raises(nv.JamieHipError):
            nv.grad_sqnorm(g[:n], torch.zeros(bad, device='cuda'), state)
    with pytest.raises(nv.JamieHipError):
        nv.grad_sqnorm(g[1:n + 1], torch.zeros(nb, device='cuda'), state)         # a view that starts one element in
    torch.cuda.synchronize()
    assert state.tolist() == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------
# the partial sums as clip + Adam reads them
# ------------------------------------------------------------------------------------------------
def coef_from_unit_step(nv, part):
    """clip + Adam with p0 = m0 = v0 = 0, t = 1, g = 1 on n = 2052 (two workgroups): m' = (1 - beta1) * coef in every
    element, so the coefficient both workgroups derived from `part` is read back from m."""
    n = 2052
    z = torch.zeros(n)
    c = dict(p0=z, m0=z, v0=z, g=torch.ones(n))
    (pf, p), (gf, g), (mf, m), (vf, v) = (padded(c[k]) for k in ('p0', 'g', 'm0', 'v0'))
    before = part.clone()
    nv.clip_adam(p, g, m, v, part, ou.DEFAULT.tensor().cuda(), new_state(1))
    torch.cuda.synchronize()
    assert all(sentinels_intact(x) for x in (pf, gf, mf, vf)) and torch.equal(part, before)
    m = m.cpu()
    assert bool((m == m[0]).all()), 'the workgroups (or lanes) disagree on the norm'
    return float(m[0].double() / (1.0 - ou.DEFAULT.tensor()[9].double()))


@pytest.mark.parametrize('length', PARTIAL_LENGTHS)
def test_every_partial_sum_is_added_once(nv, length):
    probes = sorted({i for i in (0, 511, 512, 4095, 4096, 4097, length - 1) if i < length})
    part = torch.zeros(length)
    part[probes] = 1.0                                  # total^2 = the probe count, exact: a missed probe moves coef by >= 3 %
    coef = coef_from_unit_step(nv, part.cuda())
    want = min(1.0 / (len(probes) ** 0.5 + 1e-6), 1.0)
    print(f'OPTIM partials length={length} probes={len(probes)} coef rel={abs(coef - want) / want:.3e}')
    assert abs(coef - want) <= 1e-6 * want
    part = 1.0 + torch.rand(length, generator=torch.Generator().manual_seed(length))
    coef = coef_from_unit_step(nv, part.cuda())
    total, want = 1.0 / coef - 1e-6, float(part.double().sum().sqrt())
    print(f'OPTIM partials length={length} random total rel={abs(total - want) / want:.3e}')
    assert abs(total - want) <= ou.SUMSQ_RTOL * want


@pytest.mark.parametrize('length', [0, MAX_PARTIALS + 1])
def test_partial_count_out_of_range_raises(nv, length):
    with pytest.raises(nv.JamieHipError):
        coef_from_unit_step(nv, torch.ones(MAX_PARTIALS + 8, device='cuda')[:length])      # (a view: never a null pointer)


# ------------------------------------------------------------------------------------------------
# one step from arbitrary state
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['warm-t10-p1e-3', 'bf16-warm-t10', 'bf16-warm-t10-gscale-eighth', 'bf16-single-gpu'])
@pytest.mark.parametrize('n', STEP_SIZES)
def test_one_step_at_every_launch_boundary(nv, n, name):
    c, ref = case_and_ref(n, name)
    out = run_step(nv, c)
    check_step(out, ref, f'sizes family={name} n={n}')
    assert same_bits(out, run_step(nv, c, with_bf16=False)), 'p, m, v depend on whether the bf16 copy is written'


@pytest.mark.parametrize('name', list(ou.FP32_FAMILIES) + list(ou.BF16_FAMILIES))
@pytest.mark.parametrize('n', ou.FAMILY_SIZES)
def test_one_step_of_every_family(nv, n, name):
    c, ref = case_and_ref(n, name)
    check_step(run_step(nv, c), ref, f'family={name} n={n}')


@pytest.mark.parametrize('name', ['warm-t10-p1e-3', 'bf16-warm-t10'])
@pytest.mark.parametrize('n,cuts', [(2049, (4, 2044)), (526_339, (2048, 262_148)), (1_048_583, (524_288, 524_292))])
def test_slices_sharing_the_partial_sums_equal_one_launch(nv, n, cuts, name):
    """The pipelined optimiser updates [0, n) in slices that start at multiples of 4 and read the same partial sums."""
    c, _ = case_and_ref(n, name)
    assert same_bits(run_step(nv, c), run_step(nv, c, slices=cuts), ('p', 'm', 'v', 'pb'))


@pytest.mark.parametrize('name', ['warm-t10-p1e-3', 'bf16-warm-t10'])
def test_clip_adam_argument_checks(nv, name):
    n = 2049
    c = ou.family(n, name)
    p, g, m, v = (torch.cat([c[k], c[k][:8]]).cuda() for k in ('p0', 'g', 'm0', 'v0'))
    part, hyper, state = torch.ones(4, device='cuda'), c['hyper'].tensor().cuda(), new_state(3)
    keep = [x.clone() for x in (p, m, v)]
    with pytest.raises(nv.JamieHipError):
        nv.clip_adam(p[1:n + 1], g[:n], m[:n], v[:n], part, hyper, state)           # p starts one element in
    with pytest.raises(nv.JamieHipError):
        nv.clip_adam(p[:n], g[1:n + 1], m[:n], v[:n], part, hyper, state)           # the (fp32 / bf16) gradient does
    with pytest.raises(nv.JamieHipError):
        nv.clip_adam(p[:n], g[:n], m[:n], v[:n], part, hyper, state, torch.zeros(n + 8, dtype=torch.bfloat16, device='cuda')[1:n + 1])
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(keep, (p, m, v)))


# ------------------------------------------------------------------------------------------------
# non-finite gradients: the oracle's result (clip_grad_norm_ + Adam)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('where', ['float4', 'tail', 'bf16', 'bf16-tail'])
@pytest.mark.parametrize('bad', [float('nan'), float('inf')], ids=['nan', 'inf'])
def test_non_finite_gradient(nv, bad, where):
    """One NaN makes the norm, the coefficient and so every p, m, v NaN.  One inf makes the coefficient 0: every finite entry
    takes the step of a zero gradient (m' = 0.9 m0, v' = 0.999 v0; p stays where m0 = 0) and the inf entry becomes NaN."""
    n = 2049
    c = ou.warm(n, 10, bf16=where.startswith('bf16'))
    for k in ('m0', 'v0'):
        c[k][::3] = 0                                        # every third element cold
    at = 2048 if where.endswith('tail') else 1001
    c['g'][at] = bad
    out = run_step(nv, c)
    if bad != bad:
        assert all(bool(torch.isnan(out[k]).all()) for k in ('p', 'm', 'v', 'pb'))
        return
    ref = ou.ref_of(c)
    assert float(ref['coef']) == 0 and bool(torch.isnan(ref['p'][at]))
    assert all(bool(torch.isnan(out[k][at])) for k in ('p', 'm', 'v', 'pb'))
    fin = torch.ones(n, dtype=torch.bool)
    fin[at] = False
    sub = {k: (x[fin] if torch.is_tensor(x) and x.dim() else x) for k, x in ref.items()}
    check_step({k: out[k][fin] for k in ('p', 'm', 'v', 'pb')}, sub, f'inf {where}')
    cold = fin & (c['m0'] == 0)
    assert torch.equal(out['p'][cold], c['p0'][cold]) and not out['m'][cold].any() and not out['v'][cold].any()


# ------------------------------------------------------------------------------------------------
# 1 - beta: the kernel against torch's own reading of the hyper-parameters
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('t', [10, 1000])
@pytest.mark.parametrize('n', [2049, 526_339])
def test_one_step_against_the_torch_hyper_parameters(nv, n, t):
    """adam_ref('torch') takes 0.9, 0.999, ... as python doubles, as torch.optim.Adam does.  With hyper[14] and hyper[15] holding
    1 - beta (double, rounded once: what TrainEngine(torch_one_minus_beta=True) writes) the kernel meets the same bounds against it.  Without them it forms
    1.f - fl32(0.999), and v is off by the derived |fl32(0.999) - 0.999| / 0.001 = 1.29e-5 -- 7 x BOUND_V."""
    name = f'warm-t{t}-p1e-3'
    c, ref = case_and_ref(n, name, 'torch', True)
    check_step(run_step(nv, c), ref, f'torch-hyper slots family={name} n={n}')
    c, ref = case_and_ref(n, name, 'torch', False)
    e_p, e_m, e_v = ou.scaled_errors(*(run_step(nv, c)[k] for k in 'pmv'), ref)
    print(f'OPTIM torch-hyper no-slots family={name} n={n} e_p={e_p:.3e} e_m={e_m:.3e} e_v={e_v:.3e}')
    assert e_v <= ou.GIVEN_VS_TORCH_E_V + ou.BOUND_V        # (measured 1.28e-5 .. 1.30e-5: the derived distance)


@pytest.mark.parametrize('on', [False, True], ids=['kernel-forms-them', 'torch-one-minus-beta'])
def test_engine_steps_with_and_without_one_minus_beta(nv, on):
    """TrainEngine(torch_one_minus_beta=True), what the JAMIE facade and the torch-compatible model build, hands the kernel
    1 - beta as the test above does and trains: three steps against the oracle (torch's Adam arithmetic), the losses at the tolerance of
    __graft_entry__.smoke().  Without it the slots stay 0."""
    import numpy as np
    from jamie_amd.engine import TrainEngine
    from jamie_amd.model import edModelVar
    from oracle import jamie_oracle as orc
    dims, L, B, p = (96, 72), 8, 128, 0.6
    torch.manual_seed(666)
    model = edModelVar(dims, L)
    torch.manual_seed(666)
    P, Bf = orc.init_state(dims, L)
    for x in P.values():
        x.requires_grad_(True)
    eng = TrainEngine(model, B, torch_one_minus_beta=on)
    assert torch.equal(eng.hyper.cpu()[8:], ou.Hyper(slots=on).tensor()[8:])
    opt = orc.Adam(P.values(), 1e-3)
    rng = np.random.default_rng(0)
    Z = rng.standard_normal((B, 6))
    X = [torch.from_numpy((Z @ rng.standard_normal((6, d)) + .1 * rng.standard_normal((B, d))).astype(np.float32)) for d in dims]
    for i in range(2):
        eng.ws[i]['x'].copy_(X[i])
    eng.set_kl_anneal(0.5)
    for step in range(3):
        torch.manual_seed(1 + step)
        noise = orc.draw_noise(dims, L, B, p)
        st = orc.train_step(P, Bf, opt, X, torch.eye(B), torch.zeros(B, B), noise, p, 0.5)
        eng.step(None, None, {'eps': [e.cuda() for e in noise['eps']],
                              'enc_masks': [[m.to(torch.uint8).cuda() for m in pr] for pr in noise['enc_masks']],
                              'dec_masks': [[m.to(torch.uint8).cuda() for m in pr] for pr in noise['dec_masks']]})
        np.testing.assert_allclose(eng.read_losses()[0], st['losses'], rtol=2e-4, atol=1e-6, err_msg=f'step {step}')
    assert int(eng.state[1]) == 3
    sd = model.state_dict()
    for k, x in P.items():
        if not orc.is_dead_bias(k):
            # (after the first step an element whose gradient is rounding noise moves by +-lr in either implementation:
            # test_hip_step.py's three-step comparison holds the tensors to this relative L2 as well)
            got, want = sd[k].cpu().double(), x.detach().double()
            assert float((got - want).norm()) <= 2e-3 * float(want.norm()), k


# ------------------------------------------------------------------------------------------------
# beyond 32-bit offsets
# ------------------------------------------------------------------------------------------------
def test_one_step_beyond_32_bit_offsets(nv):
    """n = 2^31 + 2055: byte offsets pass 2^32 at 2^30 elements, element indices pass 2^31.  Buffers from torch.randn on the
    GPU, the reference is adam_ref in torch float64 on the GPU in chunks of 2^26.  About 40 GiB.
    Warm state at t = 10 with p0 ~ N(0,1): e_p's largest values come from the rare elements where p0 and the update both nearly
    vanish, and the largest of n of them grows with n (the fp32 restatement: x 1.5 per x 5.7 elements with p0 ~ 1e-3 N, none with
    p0 ~ N).  The bounds were measured at 3e6 elements; this test is about addressing, so it takes the p0 that leaves them valid
    at 700 times as many."""
    if torch.cuda.mem_get_info()[0] < 64 << 30:
        pytest.skip('needs 64 GiB of free device memory')
    n, chunk, t = (1 << 31) + 2055, 1 << 26, 10
    starts = range(0, n, chunk)

    def draw(which, a):                       # the same values whenever it is asked again
        r = torch.Generator(device='cuda').manual_seed(1000 * which + a // chunk)
        x = torch.randn(min(chunk, n - a), generator=r, device='cuda')
        return [x, x * 1e-2, (x * 1e-2) ** 2, x * 1e-2][which]

    bufs = []
    for which in range(4):                    # p, m, v, g
        full = torch.empty(n + SENTINELS, device='cuda')
        full[n:] = SENTINEL
        for a in starts:
            full[a:a + chunk][:min(chunk, n - a)] = draw(which, a)
        bufs.append(full)
    p, m, v, g = (x[:n] for x in bufs)
    sumsq = sum(float((draw(3, a).double() ** 2).sum()) for a in starts)
    hyper, state, part = ou.DEFAULT.tensor().cuda(), new_state(t - 1), nan_partials(nv, n)
    nv.grad_sqnorm(g, part, state)
    nv.clip_adam(p, g, m, v, part, hyper, state)
    torch.cuda.synchronize()
    assert state.tolist() == [0, t, 0, 0] and all(sentinels_intact(x) for x in bufs)
    assert bool(torch.isfinite(part).all())
    got = float(part.double().sum())
    print(f'OPTIM 2^31 sumsq rel={abs(got - sumsq) / sumsq:.3e}')
    assert abs(got - sumsq) <= ou.SUMSQ_RTOL * sumsq
    worst = [0.0, 0.0, 0.0]
    for a in starts:
        e = min(a + chunk, n)
        g0 = draw(3, a)
        assert torch.equal(g[a:e], g0), 'the gradient was modified'
        ref = ou.adam_ref(draw(0, a), g0, draw(1, a), draw(2, a), t, ou.DEFAULT, sumsq=sumsq)
        worst = [max(x, y) for x, y in zip(worst, ou.scaled_errors(p[a:e], m[a:e], v[a:e], ref))]
        del ref, g0
    print('OPTIM 2^31 e_p=%.3e e_m=%.3e e_v=%.3e' % tuple(worst))
    del bufs, p, m, v, g
    torch.cuda.empty_cache()
    assert worst[0] <= ou.BOUND_P and worst[1] <= ou.BOUND_M and worst[2] <= ou.BOUND_V, worst

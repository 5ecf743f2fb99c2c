"""Shared by tests/test_host_optim.py and tests/test_hip_optim.py: the float64 reference of one clip + Adam step
(csrc/optim.hip), its float32 restatement, the scaled errors and the seeded input families.  Plain torch, no GPU code: every
function works on whatever device its tensors live on."""
import dataclasses
import math

import torch


@dataclasses.dataclass(frozen=True)
class Hyper:
    """The optimiser's hyper-parameters as python doubles (what torch.optim.Adam is given).  `slots`: also hand the kernel
    1 - beta1 and 1 - beta2, computed in double and rounded once, in hyper[14] and hyper[15] (as
    TrainEngine(torch_one_minus_beta=True) does)."""
    lr: float = 1e-3
    b1: float = 0.9
    b2: float = 0.999
    eps: float = 1e-8
    max_norm: float = 1.0
    gscale: float = 1.0
    slots: bool = False

    def tensor(self):
        """float32[16] as the kernel reads it: [8] lr, [9] beta1, [10] beta2, [11] eps, [12] max_norm, [13] grad_scale,
        [14] 1 - beta1, [15] 1 - beta2 (0 = not given)."""
        h = torch.zeros(16)
        h[8:14] = torch.tensor([self.lr, self.b1, self.b2, self.eps, self.max_norm, self.gscale], dtype=torch.float64).float()
        if self.slots:
            h[14:16] = torch.tensor([1 - self.b1, 1 - self.b2], dtype=torch.float64).float()
        return h


DEFAULT = Hyper()
NON_DEFAULT = Hyper(lr=3e-4, b1=0.8, b2=0.99, eps=1e-6, max_norm=0.5)


def _resolve(hyper, hyper_as):
    """(lr, b1, b2, eps, max_norm, gscale, 1 - b1, 1 - b2, base of bias correction 1, of 2) as python doubles."""
    if hyper_as == 'torch':
        return (hyper.lr, hyper.b1, hyper.b2, hyper.eps, hyper.max_norm, hyper.gscale, 1 - hyper.b1, 1 - hyper.b2,
                hyper.b1, hyper.b2)
    assert hyper_as == 'given'
    h = [float(x) for x in hyper.tensor().double()]         # the fp32 numbers, widened
    lr, b1, b2, eps, max_norm, gscale = h[8:14]
    omb1, base1 = (h[14], 1.0 - h[14]) if h[14] != 0 else (1.0 - b1, b1)      # (1.f - b is exact in fp32 for b in [0.5, 1])
    omb2, base2 = (h[15], 1.0 - h[15]) if h[15] != 0 else (1.0 - b2, b2)
    return lr, b1, b2, eps, max_norm, gscale, omb1, omb2, base1, base2


def adam_ref(p0, g, m0, v0, t, hyper, g_norm=None, hyper_as='given', sumsq=None):
    """One step in float64.  `g_norm`: the buffer the partial sums came from (default g); `sumsq`: its sum of squares if the
    caller has it already (chunked evaluation).  Returns a dict of float64 tensors: p, m, v, gg (the clipped gradient), p0, m0,
    omb1 and the 0-dim total and coef."""
    lr, b1, b2, eps, max_norm, gscale, omb1, omb2, base1, base2 = _resolve(hyper, hyper_as)
    p0, g, m0, v0 = p0.double(), g.double(), m0.double(), v0.double()
    if sumsq is None:
        sumsq = ((g if g_norm is None else g_norm.double()) ** 2).sum()
    total = gscale * torch.sqrt(torch.as_tensor(sumsq, dtype=torch.float64))
    coef = torch.clamp(max_norm / (total + 1e-6), max=1.0) * gscale            # (clamp hands a NaN on, as clip_grad_norm_ does)
    gg = g * coef
    m = m0 + (gg - m0) * omb1
    v = b2 * v0 + omb2 * gg * gg
    p = p0 - lr / (1 - base1 ** t) * m / (torch.sqrt(v) / math.sqrt(1 - base2 ** t) + eps)
    return dict(p=p, m=m, v=v, gg=gg, p0=p0, m0=m0, omb1=omb1, total=total, coef=coef)


def tree_sum_f32(x):
    """Sum of a float32 vector by halving, in float32: elementwise additions only, so the result does not depend on the
    machine's thread count or vector width."""
    x = x.flatten().float()
    size = 1 << max(0, (x.numel() - 1).bit_length())
    x = torch.cat([x, x.new_zeros(size - x.numel())])
    while x.numel() > 1:
        half = x.numel() // 2
        x = x[:half] + x[half:]
    return x[0]


def adam_f32(p0, g, m0, v0, t, hyper, g_norm=None):
    """The same formula step by step in torch float32, the hyper-parameters as the kernel is handed them and the bias
    corrections as the kernel forms them (in double, rounded once): what fp32 arithmetic alone costs.  Returns p, m, v."""
    h = hyper.tensor()
    lr, b1, b2, eps, max_norm, gscale = h[8], h[9], h[10], h[11], h[12], h[13]
    one = torch.tensor(1.0)
    omb1 = h[14] if h[14] != 0 else one - b1
    omb2 = h[15] if h[15] != 0 else one - b2
    base1 = 1.0 - float(h[14]) if h[14] != 0 else float(b1)
    base2 = 1.0 - float(h[15]) if h[15] != 0 else float(b2)
    bc1 = torch.tensor(1.0 - base1 ** t, dtype=torch.float64).float()
    bc2s = torch.tensor(math.sqrt(1.0 - base2 ** t), dtype=torch.float64).float()
    gn = (g if g_norm is None else g_norm).float()
    total = torch.sqrt(tree_sum_f32(gn * gn)) * gscale
    coef = torch.clamp(max_norm / (total + torch.tensor(1e-6)), max=1.0) * gscale
    gg = g.float() * coef
    m = m0 + (gg - m0) * omb1
    v = v0 * b2 + omb2 * gg * gg
    denom = torch.sqrt(v) / bc2s + eps
    p = p0 - (lr / bc1) * (m / denom)
    assert p.dtype == m.dtype == v.dtype == torch.float32
    return p, m, v


def scaled_errors(p_k, m_k, v_k, ref):
    """(e_p, e_m, e_v): elementwise errors of a kernel's (or restatement's) p, m, v scaled by the reference's operands, maximum
    over the elements.  Where a denominator is 0 the value must equal the reference exactly."""
    out = []
    for name, got, den in (('p', p_k, ref['p0'].abs() + (ref['p'] - ref['p0']).abs()),
                           ('m', m_k, ref['m0'].abs() + ref['omb1'] * ref['gg'].abs()),
                           ('v', v_k, ref['v'])):
        err = (got.double() - ref[name]).abs()
        zero = den == 0
        bad = int((zero & (err != 0)).sum())
        assert bad == 0, f'{name}: {bad} elements differ from the reference where its scale is 0'
        e = torch.where(zero, torch.zeros_like(err), err / den)
        assert bool(torch.isfinite(e).all()), f'{name}: non-finite scaled error'
        out.append(float(e.max()))
    return tuple(out)


# ---------------------------------------------------------------------------------------------------
# Bounds.  adam_f32 against adam_ref('given'), maximum over measured_cases() (tests/test_host_optim.py asserts that the
# restatement stays below these, so they cannot drift).  The GPU kernel is held to 4 x: hipcc may or may not contract
# m + (gg - m) * omb1 and the v update into fma, and the kernel adds the norm up in another order (a few 1e-7 on coef).
# ---------------------------------------------------------------------------------------------------
F32_E_P = 2.0e-6     # measured 1.9935e-06 (warm, t = 100000, p0 ~ 1e-3 N, n = 3000017: m' nearly cancels where p0 is small too)
F32_E_M = 2.8e-7     # measured 2.7971e-07 (single-GPU bf16 arrangement, n = 3000017)
F32_E_V = 4.2e-7     # measured 4.1994e-07 (bf16 gradient, warm, t = 10, n = 526339)
BOUND_P, BOUND_M, BOUND_V = 4 * F32_E_P, 4 * F32_E_M, 4 * F32_E_V

# adam_ref('given') against adam_ref('torch') in float64, default hyper-parameters without the two 1 - beta slots, warm
# inputs, t in {1, 10, 1000, 100000}: what the fp32 rounding of beta2 = 0.999 alone costs.  e_v is derived:
# |fl32(0.999) - 0.999| / 0.001 = 1.29e-5 on every increment of v.
GIVEN_VS_TORCH_E_V = 1.3e-5      # derived; measured 1.2875e-05 at every t
GIVEN_VS_TORCH_E_P = 1.7e-5      # measured 1.6074e-05 (t = 100000, p0 ~ 1e-3 N, n = 100003)

SUMSQ_RTOL = 2e-6    # sum of squares / norm against float64 (test_fused_gradient_norm_equals_the_norm_of_the_gradient's bound)

# ---------------------------------------------------------------------------------------------------
# Input families (fp32 CPU tensors from seeded generators)
# ---------------------------------------------------------------------------------------------------
FAMILY_SIZES = (5, 2049, 526_339, 3_000_017)
WARM_T = (2, 10, 1000, 100_000)


def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1_000_003 + int(k)) % (1 << 62)
    return torch.Generator().manual_seed(seed)


def _case(p0, g, m0, v0, t, hyper=DEFAULT, g_norm=None):
    return dict(p0=p0, g=g, m0=m0, v0=v0, t=t, hyper=hyper, g_norm=g_norm)


def warm(n, t, p_scale=1e-3, hyper=DEFAULT, ranks=1, bf16=False, seed=0):
    """A resumed run: m0 ~ 1e-2 N, v0 = (1e-2 N)^2, g ~ 1e-2 N (times `ranks`: the SUM an all-reduce leaves, averaged by
    gscale = 1 / ranks), p0 ~ p_scale N.  `bf16`: g is a bf16 tensor."""
    r = _gen(1, n, t, seed)
    p0 = torch.randn(n, generator=r) * p_scale
    m0 = torch.randn(n, generator=r) * 1e-2
    v0 = (torch.randn(n, generator=r) * 1e-2) ** 2
    g = torch.randn(n, generator=r) * (1e-2 * ranks)
    if bf16:
        g = g.to(torch.bfloat16)
    return _case(p0, g, m0, v0, t, dataclasses.replace(hyper, gscale=1.0 / ranks))


def cold(n, clipped):
    """p0 = m0 = v0 = 0, t = 1; g ~ 3 N (clipped) or 1e-3 N / sqrt(n) (not clipped)."""
    r = _gen(2, n, clipped)
    z = torch.zeros(n)
    g = torch.randn(n, generator=r) * (3.0 if clipped else 1e-3 / math.sqrt(n))
    return _case(z.clone(), g, z.clone(), z.clone(), 1)


def wide(n):
    """g = N(0,1) * 10^U(-10,0) with every 7th element 0, cold: sqrt(v) / sqrt(bc2) crosses eps."""
    r = _gen(3, n)
    z = torch.zeros(n)
    g = torch.randn(n, generator=r) * 10.0 ** (-10.0 * torch.rand(n, generator=r, dtype=torch.float64)).float()
    g[::7] = 0
    return _case(z.clone(), g, z.clone(), z.clone(), 1)


def single_gpu(n, t):
    """The single-GPU arrangement of the bf16 step: the norm from the fp32 gradient, the update from its bf16 rounding."""
    c = warm(n, t, seed=1)
    c['g_norm'] = c['g']
    c['g'] = c['g'].to(torch.bfloat16)
    return c


def _families():
    fp32 = {'cold-clipped': lambda n: cold(n, True), 'cold-unclipped': lambda n: cold(n, False), 'wide': wide}
    bf16 = {}
    for t in WARM_T:
        fp32[f'warm-t{t}-p1e-3'] = lambda n, t=t: warm(n, t, 1e-3)
        fp32[f'warm-t{t}-p1'] = lambda n, t=t: warm(n, t, 1.0)
        bf16[f'bf16-warm-t{t}'] = lambda n, t=t: warm(n, t, bf16=True)
        bf16[f'bf16-warm-t{t}-gscale-eighth'] = lambda n, t=t: warm(n, t, ranks=8, bf16=True)
    fp32['gscale-quarter'] = lambda n: warm(n, 10, ranks=4)
    fp32['non-default'] = lambda n: warm(n, 10, hyper=NON_DEFAULT)
    bf16['bf16-single-gpu'] = lambda n: single_gpu(n, 10)
    return fp32, bf16


# name -> case(n): the families every one-step test runs at the sizes FAMILY_SIZES, with an fp32 and with a bf16 gradient
FP32_FAMILIES, BF16_FAMILIES = _families()


def family(n, name):
    return (FP32_FAMILIES.get(name) or BF16_FAMILIES[name])(n)


def measured_cases():
    """Every (name, n, case) the fp32 restatement is measured over."""
    for n in FAMILY_SIZES:
        for name in list(FP32_FAMILIES) + list(BF16_FAMILIES):
            yield name, n, family(n, name)


def ref_of(c, hyper_as='given'):
    return adam_ref(c['p0'], c['g'], c['m0'], c['v0'], c['t'], c['hyper'], g_norm=c['g_norm'], hyper_as=hyper_as)
